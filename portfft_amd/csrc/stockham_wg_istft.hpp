// Inverse short-time Fourier transform (overlap-add synthesis) of REAL signals in ONE kernel: the C2R untangle-in step
// and the M-point backward passes of stockham_wg_real.hpp, run LDS to LDS, in front of an overlap-add step over a
// circular accumulator in LDS.  A row of the kernel is one (signal i, frame f) pair: the M + 1 bins of a frame are read
// once from the frame-major input (what stockham_wg_stft.hpp writes), transformed to N = 2 * M scalars, multiplied with
// the synthesis window and added to the frames they overlap; a sample leaves -- one plain store -- when no later frame
// reaches it.  No frame buffer, no atomics, no zeroed output.
//
// No counterpart in the reference; reached through pfft_execute_istft on a plan of the REAL domain whose synthesis window
// was set (pfft_plan_set_synthesis_window).
//
// Geometry (all kernel arguments; out_length, out_pitch, lead and hop count SCALARS, frame_pitch and in_pitch complex
// elements).  With u = t + lead the position of output sample t on the frames' axis (frame f covers [f hop, f hop + N)):
//   ola[i][t] = sum over f of w[u - f hop] * g[i][f][u - f hop],   g = scale * N * irfft(bins of frame f)
//   env[t]    = sum over f of w[u - f hop]^2                        over the frames with 0 <= u - f hop < N
//   NORMALIZE: ola / env where env > ISTFT_ENV_MIN, else exactly 0;  otherwise ola
// BOTH SUMS RUN IN ASCENDING f, ONE FRAME AFTER THE OTHER, wherever the work is cut: the result does not depend on
// chunk_frames or on the grid, bit for bit.
//
// Overlap-add by chunks with a recomputed halo (overlap-save's idea turned round).  A group of the persistent loop owns
// (signal i, chunk c): the frames [c C, min(F, (c + 1) C)), C = chunk_frames, and the output samples
// [c C hop - lead, (c + 1) C hop - lead) cut to [0, out_length) -- the last chunk of a signal everything up to
// out_length.  It runs the frames max(0, c C - H) ... end of chunk in ascending order, FPW per step, H = ceil(N / hop) - 1:
// the first H frames are the halo, the only earlier frames that reach an owned sample.  They are transformed and
// accumulated like the others and what they complete lies in front of the chunk: its stores are dropped.
//
// Overlap-add step (behind the barrier that ends the last pass).  First the window: a sweep over the group's images turns
// each into its N scalars w[j] * g[j] in place -- the window is read as M aligned pairs through L1 / L2 inside the loop,
// as in stockham_wg_stft.hpp, in batches of 8 (fp32) / 4 (fp64) independent loads per lane that are in flight together.  Then every lane owns the
// positions d = lane, lane + WG, ... counted from the step's first: it takes the partial sum the earlier steps left for
// d (the first N - hop positions have one), adds the scalars of the step's live frames that cover d, ascending, and
// either emits the sum -- the first FPW_live * hop positions are complete -- or keeps it.  What is kept, N - hop
// scalars whatever FPW is, lives in a circular accumulator behind the images (and the TWL copy): position p of the
// frames' axis in slot p mod CAP, CAP = N rounded up to a multiple of WG.  No slot is ever cleared: which slots hold a
// partial sum is known from d alone.  Positions d and d + CAP share a slot and, CAP being a multiple of WG, a lane,
// which takes them in ascending order: the old sum of d is read before the new one of d + CAP is written; the kept
// positions span less than CAP, so no two of them meet; different lanes never meet in a step.
//
// The emit store is a scalar store; each scalar is predicated on its OWN index relative to the chunk's first owned
// sample: one add and one unsigned compare, never parity, never the range check of the buffer resource
// (stockham_wg_ols.hpp's rule).  NORMALIZE sums w^2 over the covering frames on the fly at emission, ceil(N / hop)
// window reads per sample: an envelope accumulator in LDS would put fp32 N = 16384 and fp64 N = 8192 over 160 KiB.
//
// Rows behind the last frame of a chunk are dead: they load nothing, still reach every barrier, and nothing reads their
// images.  The input resource starts at the first frame of the group's run and the output resource at the chunk's first
// owned sample, so only one group's span has to lie within 4 GiB.  `in` and `out` must not overlap.
#pragma once
#include "stockham_wg_real.hpp"

namespace pfa {

/// the envelope at or below which NORMALIZE writes 0: the constant torch.istft tests its envelope against
/// (PFFT_ISTFT_ENV_MIN of the C header)
constexpr double ISTFT_ENV_MIN = 1e-11;

/// slots of the circular accumulator: N = 2 * Cfg::N rounded up to whole sweeps of the group's lanes
template <typename Cfg>
constexpr unsigned istft_acc_slots() {
  return unsigned((2 * Cfg::N + Cfg::WG - 1) / Cfg::WG) * Cfg::WG;
}

/// LDS of the inverse STFT kernels of configuration Cfg (an M-point wg_cfg): the real kernels', and the accumulator
/// behind it
template <typename Cfg>
constexpr size_t istft_lds_bytes() {
  return real_lds_bytes<Cfg>() + size_t(istft_acc_slots<Cfg>()) * sizeof(typename Cfg::T);
}

/// floor(a / b) for a < 2^22 with rb = 1.0f / b: the rounded quotient is off by at most one
PFA_DEV unsigned istft_div(unsigned a, unsigned b, float rb) {
  unsigned q = static_cast<unsigned>(static_cast<float>(a) * rb);
  const unsigned p = q * b;
  if (p > a) {
    --q;
  } else if (a - p >= b) {
    ++q;
  }
  return q;
}

/// what the LDS-to-LDS passes are given as io: they touch none of it
struct istft_no_io {
  static PFA_DEV unsigned in_off(unsigned, unsigned j) { return j; }
  static PFA_DEV unsigned out_off(unsigned, unsigned j) { return j; }
  static constexpr unsigned in_step(int k) { return k; }
  static constexpr unsigned out_step(int k) { return k; }
};

/// n_frames frames of Cfg::N + 1 bins per signal (pitches frame_pitch / in_pitch, complex elements) -> out_length real
/// scalars per signal (pitch out_pitch).  tw: the real plan's tables.  win: the synthesis window, N = 2 * Cfg::N scalars.
/// chunk: frames per chunk, 1 ... n_frames.  See the head of the file; the prologue is wg_twiddle_prologue.
template <typename Cfg, bool NORMALIZE>
__global__ __launch_bounds__(Cfg::WG, Cfg::OCC) void stockham_wg_istft_kernel(
    const void* in, void* out, const cx<typename Cfg::T>* __restrict__ tw, const void* __restrict__ win, unsigned n_signals,
    unsigned n_frames, typename Cfg::T scale, unsigned lead, unsigned hop, unsigned out_length, unsigned frame_pitch,
    unsigned in_pitch, unsigned out_pitch, unsigned chunk) {
  using T = typename Cfg::T;
  using Seq = typename Cfg::Seq;
  constexpr int M = Cfg::N;
  constexpr unsigned N = 2u * M;
  constexpr unsigned CAP = istft_acc_slots<Cfg>();  // accumulator slots
  constexpr int CH = Cfg::FPW * M;                   // elements of the group's images (the window sweep)
  constexpr int WB = sizeof(T) == 4 ? 8 : 4;         // window pairs in flight per lane
  constexpr unsigned SB = sizeof(T);
  constexpr unsigned ES = sizeof(cx<T>);
  static_assert(Cfg::LDS_PER_FFT > 0, "LDS-resident configurations only");
  static_assert(unsigned(Cfg::FPW) * N < (1u << 22), "istft_div");
  constexpr int KH = M / 2 + 1;                        // work items of the untangle step: k = 0 ... M/2
  constexpr int UPT = (KH + Cfg::TPF - 1) / Cfg::TPF;  // ... per lane
  extern __shared__ __attribute__((aligned(16))) char pfa_smem[];
  const int f = threadIdx.x / Cfg::TPF;
  const int tid = threadIdx.x % Cfg::TPF;
  cx<T>* all = reinterpret_cast<cx<T>*>(pfa_smem);
  cx<T>* lds = all + f * Cfg::LDS_PER_FFT;
  T* acc = reinterpret_cast<T*>(pfa_smem + real_lds_bytes<Cfg>());

  cx<T> twr[Cfg::TWR_TOTAL];
  wg_twiddle_prologue<Cfg>(tw, tid, twr, all);
  const float rhop = 1.0f / static_cast<float>(hop);
  const unsigned halo = (N + hop - 1) / hop - 1;                // H
  const unsigned n_chunks = (n_frames + chunk - 1) / chunk;     // (the host keeps chunk within 1 ... n_frames)
  const unsigned ngroups = n_signals * n_chunks;                // (... and the row count below 2^31)
  for (unsigned g = blockIdx.x; g < ngroups; g += gridDim.x) {
    const cx<T>* twp = tw;
    const void* winp = win;
    if constexpr (Cfg::TWM == TW_GLOBAL) {
      asm volatile("" : "+s"(twp));  // (stockham_wg_body: keep the table reads inside the loop)
    }
    asm volatile("" : "+s"(winp));  // (... and the window's: it stays in L1 / L2, not in registers across the loop)
    const T* wp = static_cast<const T*>(winp);
    const cx<T>* wpair = static_cast<const cx<T>*>(winp);  // the window as M aligned pairs
    const cx<T>* wk = twp + Seq::tw_total;
    // the group's chunk (all uniform)
    const unsigned sig = g / n_chunks;
    const unsigned c = g - sig * n_chunks;
    const unsigned cf0 = c * chunk;
    const bool last_chunk = c == n_chunks - 1;
    const unsigned fe = last_chunk ? n_frames : cf0 + chunk;
    const unsigned fs = cf0 > halo ? cf0 - halo : 0u;
    long long lo = static_cast<long long>(cf0) * hop - lead;
    if (lo < 0) lo = 0;
    long long hi = last_chunk ? static_cast<long long>(out_length) : static_cast<long long>(fe) * hop - lead;
    if (hi > static_cast<long long>(out_length)) hi = out_length;
    if (hi < lo) hi = lo;
    const unsigned n_own = static_cast<unsigned>(hi - lo);  // (the host keeps one group's span within 4 GiB)
    const unsigned long long ifirst =
        static_cast<unsigned long long>(sig) * in_pitch + static_cast<unsigned long long>(fs) * frame_pitch;
    const unsigned long long ibytes = (static_cast<unsigned long long>(fe - fs - 1) * frame_pitch + M + 1) * ES;
    const unsigned long long ofirst = static_cast<unsigned long long>(sig) * out_pitch + static_cast<unsigned long long>(lo);
    const __amdgpu_buffer_rsrc_t rin = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<char*>(static_cast<const char*>(in)) + ifirst * ES, 0,
        ibytes > 0xFFFFFFFFull ? 0xFFFFFFFFu : static_cast<unsigned>(ibytes), 0x00020000);
    const __amdgpu_buffer_rsrc_t rout =
        __builtin_amdgcn_make_buffer_rsrc(static_cast<char*>(out) + ofirst * SB, 0, n_own * SB, 0x00020000);
    unsigned abase = 0;  // the slot of the step's first position
    unsigned kept = 0;   // positions of the step, from its first on, that the steps before left a partial sum for
    for (unsigned f0 = fs; f0 < fe; f0 += Cfg::FPW) {
      const unsigned live = fe - f0 < unsigned(Cfg::FPW) ? fe - f0 : unsigned(Cfg::FPW);  // FPW_live
      // the C2R untangle-in step of stockham_wg_real_body: bins k and M - k of the lane's own frame
      if (Cfg::FPW == 1 || static_cast<unsigned>(f) < live) {
        const unsigned row = (f0 - fs + (Cfg::FPW == 1 ? 0u : static_cast<unsigned>(f))) * frame_pitch;
        sfor<0, UPT>([&](auto i_) PFA_LAMBDA {
          const unsigned k = tid + decltype(i_)::value * Cfg::TPF;
          if (KH % Cfg::TPF == 0 || k < KH) {
            cx<T> x = buf_load<T, Cfg::AUX>(rin, (row + k) * ES, 0), y = buf_load<T, Cfg::AUX>(rin, (row + M - k) * ES, 0);
            if (k == 0) x.im = y.im = T(0);
            const cx<T> s{x.re + y.re, x.im - y.im}, d{x.re - y.re, x.im + y.im};
            const cx<T> w = wk[k];
            const cx<T> q{w.re * d.re + w.im * d.im, w.re * d.im - w.im * d.re};  // conj(w) d;  P = i q
            lds[lds_pad<Cfg>(k)] = cx<T>{s.re - q.im, -(s.im + q.re)};
            if (k != 0 && 2 * k != M) lds[lds_pad<Cfg>(M - k)] = cx<T>{s.re + q.im, s.im - q.re};
          }
        });
      }
      __syncthreads();
      // conj(z') of every frame, unscaled, in its image (the last pass ends with a barrier)
      wg_passes<Cfg, true, 0, WG_FIRST_FROM_LDS | WG_LAST_TO_LDS>(istft_no_io{}, f, lds, tid, twp, twr, scale);
      // the window: every image becomes the N scalars w[j] * g[j] in place (what the C2R kernel stores, times the window),
      // the whole group at once, the window as M aligned pairs in batches of WB independent loads
#pragma unroll 1
      for (unsigned e0 = threadIdx.x; e0 < unsigned(CH); e0 += WB * Cfg::WG) {  // (rolled: its addresses stay out of the registers)
        cx<T> wv[WB];
        sfor<0, WB>([&](auto u_) PFA_LAMBDA {
          const unsigned e = e0 + decltype(u_)::value * Cfg::WG;
          if (e < unsigned(CH)) wv[decltype(u_)::value] = wpair[e % M];
        });
        sfor<0, WB>([&](auto u_) PFA_LAMBDA {
          const unsigned e = e0 + decltype(u_)::value * Cfg::WG;
          if (e < unsigned(CH)) {
            cx<T>* p = all + (e / M) * Cfg::LDS_PER_FFT + lds_pad<Cfg>(e % M);
            const cx<T> v = *p;
            *p = cx<T>{wv[decltype(u_)::value].re * (v.re * scale), wv[decltype(u_)::value].im * -(v.im * scale)};
          }
        });
      }
      __syncthreads();
      // the overlap-add step
      const unsigned span = (live - 1) * hop + N;
      const bool all_out = last_chunk && f0 + live == fe;  // the signal's last step: everything that is left leaves
      const unsigned emit_end = all_out ? span : live * hop;
      // position d of this step is output sample rel0 + d of the chunk's own (wrapped when in front of them: beyond n_own)
      const unsigned rel0 = static_cast<unsigned>(static_cast<long long>(f0) * hop - lead - lo);
      unsigned slot = abase + threadIdx.x;  // (abase < CAP, a lane index is below WG <= CAP)
      if (slot >= CAP) slot -= CAP;
      for (unsigned d = threadIdx.x; d < span; d += Cfg::WG) {
        T a = d < kept ? acc[slot] : T(0);
        const unsigned l_lo = d < N ? 0u : istft_div(d - N, hop, rhop) + 1;  // the first frame of the step that covers d
        if constexpr (Cfg::FPW == 1) {
          a += reinterpret_cast<const T*>(all)[2 * lds_pad<Cfg>(d >> 1) + (d & 1)];  // (span = N)
        } else {
          const unsigned qd = istft_div(d, hop, rhop);
          const unsigned l_hi = qd < live - 1 ? qd : live - 1;
          for (unsigned l = l_lo; l <= l_hi; ++l) {  // ascending f
            const unsigned off = d - l * hop;
            a += reinterpret_cast<const T*>(all + l * Cfg::LDS_PER_FFT)[2 * lds_pad<Cfg>(off >> 1) + (off & 1)];
          }
        }
        if (d < emit_end) {
          const unsigned r = rel0 + d;
          if (r < n_own) {
            if constexpr (NORMALIZE) {
              // w^2 over ALL frames of the signal that cover the position, ascending f -- window offsets descending by hop
              // from the first covering frame's: up to min(f0, (N - 1 - d) / hop) frames in front of the step, then the
              // step's first to the last of the signal that starts at or before d.  Four loads go out together; a frame
              // that does not exist adds +0, which leaves the sum as it is.
              unsigned first = d - l_lo * hop;
              int count = 1 - static_cast<int>(l_lo);
              if (d < N) {
                const unsigned back = istft_div(N - 1 - d, hop, rhop);
                const unsigned jb = back < f0 ? back : f0;
                first = d + jb * hop;
                count = 1 + static_cast<int>(jb);
              }
              const unsigned qd = istft_div(d, hop, rhop);
              const unsigned ahead = n_frames - 1 - f0;
              count += static_cast<int>(qd < ahead ? qd : ahead);
              T env = T(0);
              for (; count > 0; count -= 4, first -= 4 * hop) {
                const T w0 = wp[first];
                const T w1 = count > 1 ? wp[first - hop] : T(0);
                const T w2 = count > 2 ? wp[first - 2 * hop] : T(0);
                const T w3 = count > 3 ? wp[first - 3 * hop] : T(0);
                env += w0 * w0;
                env += w1 * w1;
                env += w2 * w2;
                env += w3 * w3;
              }
              a = env > T(ISTFT_ENV_MIN) ? a / env : T(0);
            }
            buf_store_scalar<T, Cfg::AUX>(a, rout, r * SB, 0);
          }
        } else {
          acc[slot] = a;
        }
        slot += Cfg::WG;
        if (slot >= CAP) slot -= CAP;
      }
      kept = span - live * hop;  // N - hop (nothing is read after the signal's last step)
      abase = (abase + live * hop) % CAP;
      __syncthreads();  // the next step's untangle step overwrites the images, and its slots are other lanes'
    }
  }
}

}  // namespace pfa
