// Short-time Fourier transform of long REAL signals in ONE kernel: the windowed io of stockham_wg_rols.hpp in front of
// the M-point passes and the R2C untangle step of stockham_wg_real.hpp.  A row of the kernel is one (signal i, frame f)
// pair: a frame of N = 2 * M input scalars is read as M scalar pairs straight from the signal, multiplied with the
// window on the way in, transformed, and its M + 1 bins are stored at their place in the frame-major output.  Nothing is
// gathered or copied around the kernel: per sample a signal is read about N / hop times (through L2) and a bin is
// written once.
//
// No counterpart in the reference; reached through pfft_execute_stft on a plan of the REAL domain whose window was set
// (pfft_plan_set_window).
//
// Geometry (all kernel arguments; lengths, the input pitch, lead and hop count SCALARS, the output pitches complex
// elements):
//   rows      r = i * n_frames + f,  i < n_signals,  f < n_frames;  FPW consecutive rows per group
//   frame     image slot j of row (i, f) holds the pair (w[2j] * xe_i[e0 + 2j], w[2j + 1] * xe_i[e0 + 2j + 1]),
//             e0 = f * hop - lead;  xe_i is x_i extended outside [0, in_length): by zeros (REFLECT = false) or by
//             reflection without repeating the edge sample, xe[-p] = x[p], xe[L - 1 + p] = x[L - 1 - p] (REFLECT = true)
//   stores    bin k <= M of row (i, f) goes to out + i * out_pitch + f * frame_pitch + k; nothing else is written
// `hop` and `lead` may be ODD, so e0 may be, and a pair can be cut at BOTH ends of a signal -- (xe[-1], x[0]) at the
// front, (x[L-1], xe[L]) at the back, possibly in one frame.  Every scalar is therefore predicated on its own index: one
// add and one unsigned compare per scalar, never "p is even, so p + 1 does not wrap", never 32-bit wrap-around of an
// offset and never the range check of the buffer resource (stockham_wg_ols.hpp's rule).  A pair access is only
// scalar-aligned, as in stockham_wg_rols.hpp.
//
// Zero extension: the input resource starts `lead` scalars in front of the signal of the group's first row, so that no
// part of an address is negative (ols_row); what lies in front of a signal is never dereferenced (the predicate).
// Reflection: the resource starts AT that signal.  A row whose frame lies inside [0, in_length) takes the pair loads
// unpredicated; any other row maps each scalar index back into the signal (the host admits only frames inside the signal
// padded by `lead` <= in_length - 1 on both sides, so an index is reflected at most once; an index that would still lie
// outside reads as zero) and loads scalars: no address outside the signal is ever formed.
//
// The window table holds N scalars and is read as the aligned pairs w[2 (j + step)] through L1 / L2, next to w_k, inside
// the persistent loop.  NULL at pfft_plan_set_window uploads ones: one kernel form, no windowless twin.  A direct-io
// multi-pass configuration has all R inputs of a butterfly in flight at once; as many window pairs next to them would
// double that register image (and spilled where the R2C kernel does not), so its pass 0 takes the window in chunks of a
// few pairs, one chunk ahead of the multiply (stft_pass0).
//
// As in stockham_wg_rols.hpp: FPW = 1 keeps the frame uniform; STAGED configurations multiply in the staged copy and keep
// the FPW row windows in LDS behind the images; rows behind the last one have empty windows, still reach every barrier,
// and their stores are dropped.  The output resource starts at the group's first ROW, so only the rows of one group have
// to lie within 4 GiB.  In place is NOT safe (frames overlap); the host refuses overlapping buffers.
#pragma once
#include "stockham_wg_real.hpp"
#include "stockham_wg_rols.hpp"

namespace pfa {

/// LDS of the STFT kernels of configuration Cfg (an M-point wg_cfg): rols_lds_bytes
template <typename Cfg>
constexpr size_t stft_lds_bytes() {
  return rols_lds_bytes<Cfg>();
}

/// what ols_row::nvalid says about a row here
enum : unsigned { STFT_ROW_DEAD = 0, STFT_ROW_INSIDE = 1, STFT_ROW_EDGE = 2 };

/// Addressing of one group's rows.  ols_row: e0 as in rols_io (scalars, wrapped when negative); ibase the scalar of the
/// input resource that image slot 0 reads (zero extension, and the inside rows of reflection); obase the complex element
/// of the output resource that bin 0 goes to; nvalid the row's kind (STFT_ROW_*).
template <typename T, int M, int FPW, int AUX, bool REFLECT>
struct stft_io : slot_io {
  static constexpr unsigned SB = sizeof(T);
  static constexpr unsigned ES = sizeof(cx<T>);
  __amdgpu_buffer_rsrc_t rin, rout;
  const cx<T>* win;  // the window as M aligned pairs
  unsigned in_length;
  ols_row own;  // the window of this lane's row

  PFA_DEV stft_io(const void* in, void* out, const void* win_, unsigned g, unsigned f, unsigned n_signals,
                  unsigned n_frames, unsigned lead, unsigned hop, unsigned in_length_, unsigned in_pitch,
                  unsigned frame_pitch, unsigned out_pitch)
      : win(static_cast<const cx<T>*>(win_)), in_length(in_length_) {
    const unsigned r0 = g * FPW;  // (uniform; the group exists, so i0 < n_signals)
    const unsigned i0 = r0 / n_frames;
    const unsigned f0 = r0 - i0 * n_frames;
    const unsigned shift = REFLECT ? 0u : lead;
    const unsigned long long after = n_signals - 1 - i0;
    const unsigned long long ibytes = (after * in_pitch + in_length + shift) * SB;
    const unsigned long long ofirst = static_cast<unsigned long long>(i0) * out_pitch + static_cast<unsigned long long>(f0) * frame_pitch;
    const unsigned long long obytes =
        (after * out_pitch + static_cast<unsigned long long>(n_frames - 1 - f0) * frame_pitch + M + 1) * ES;
    const long long ifirst = static_cast<long long>(i0) * in_pitch - shift;
    rin = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(static_cast<const char*>(in)) + ifirst * SB, 0,
                                            ibytes > 0xFFFFFFFFull ? 0xFFFFFFFFu : static_cast<unsigned>(ibytes), 0x00020000);
    rout = __builtin_amdgcn_make_buffer_rsrc(static_cast<char*>(out) + ofirst * ES, 0,
                                             obytes > 0xFFFFFFFFull ? 0xFFFFFFFFu : static_cast<unsigned>(obytes), 0x00020000);
    const unsigned r = r0 + (FPW == 1 ? 0u : f);  // (one row per group: the window is uniform, and kept in SGPRs)
    const unsigned sig = r / n_frames;
    const unsigned fr = r - sig * n_frames;
    const unsigned di = sig - i0;
    const bool live = sig < n_signals;
    const unsigned e0 = fr * hop - lead;
    own.e0 = live ? e0 : 0xC0000000u;
    own.ibase = di * in_pitch + shift + e0;  // (not negative where it is used: e0 >= -lead, an inside row has e0 >= 0)
    // (the host keeps the rows of a group within 4 GiB: the difference fits also where a product wrapped)
    own.obase = di * out_pitch + fr * frame_pitch - f0 * frame_pitch;
    unsigned kind = live ? STFT_ROW_INSIDE : STFT_ROW_DEAD;
    if constexpr (REFLECT) {
      // inside: 0 <= e0 and e0 + N <= in_length, in unsigned arithmetic (a negative e0 wrapped is beyond every length)
      if (live && !(e0 < in_length && in_length - e0 >= 2u * M)) kind = STFT_ROW_EDGE;
    }
    own.nvalid = kind;
  }
  /// for a kernel with a row mapping of its own (stockham_wg_periodogram.hpp): it fills rin, rout and own itself
  PFA_DEV stft_io(const void* win_, unsigned in_length_) : win(static_cast<const cx<T>*>(win_)), in_length(in_length_) {}
  // the passes' side: the lane's own row, addressed by image slot (slot_io); they end in the image (WG_LAST_TO_LDS)
  PFA_DEV void store(cx<T>, unsigned, unsigned) const {}

  /// the scalar pair of slot j + step of the row with window w, unwindowed; every scalar on its own predicate
  PFA_DEV cx<T> load_pair(const ols_row& w, unsigned j, unsigned step) const {
    cx<T> x{T(0), T(0)};
    if constexpr (!REFLECT) {
      const unsigned p0 = w.e0 + 2 * (j + step);
      const unsigned p1 = p0 + 1;  // (p0 = -1 wraps to the valid index 0: compared on its own)
      const bool ok0 = p0 < in_length, ok1 = p1 < in_length;
      if (ok0 && ok1) {
        x = buf_load<T, AUX>(rin, (w.ibase + 2 * j) * SB, step * ES);
      } else if (ok0) {  // the last scalar of the signal
        x.re = buf_load_scalar<T, AUX>(rin, (w.ibase + 2 * j) * SB, step * ES);
      } else if (ok1) {  // the first scalar of the signal
        x.im = buf_load_scalar<T, AUX>(rin, (w.ibase + 2 * j + 1) * SB, step * ES);
      }
    } else {
      if (w.nvalid == STFT_ROW_INSIDE) {
        x = buf_load<T, AUX>(rin, (w.ibase + 2 * j) * SB, step * ES);
      } else if (w.nvalid == STFT_ROW_EDGE) {
        const unsigned sbase = w.ibase - w.e0;  // the signal's first scalar in the resource
        const int p0 = static_cast<int>(w.e0) + static_cast<int>(2 * (j + step));
        const unsigned m0 = reflect(p0), m1 = reflect(p0 + 1);
        if (m0 < in_length) x.re = buf_load_scalar<T, AUX>(rin, (sbase + m0) * SB, 0);
        if (m1 < in_length) x.im = buf_load_scalar<T, AUX>(rin, (sbase + m1) * SB, 0);
      }
    }
    return x;
  }
  /// index p of the extended signal -> the index inside [0, in_length) it mirrors (one reflection: the host's bound)
  PFA_DEV unsigned reflect(int p) const {
    const int last = static_cast<int>(in_length) - 1;
    return static_cast<unsigned>(p < 0 ? -p : (p > last ? 2 * last - p : p));
  }
  /// ... times the window's pair
  PFA_DEV cx<T> load_in(const ols_row& w, unsigned j, unsigned step = 0) const {
    const cx<T> x = load_pair(w, j, step);
    const cx<T> wv = win[j + step];
    return cx<T>{x.re * wv.re, x.im * wv.im};
  }
  PFA_DEV cx<T> load(unsigned slot, unsigned step) const { return load_in(own, slot, step); }
  /// bin k of the lane's own row
  PFA_DEV void bin_store(cx<T> v, unsigned k) const {
    if (own.nvalid != STFT_ROW_DEAD) buf_store<T, AUX>(v, rout, (own.obase + k) * ES, 0);
  }
};

/// the passes' view of stft_io without the window: what stft_pass0 loads
template <typename IO>
struct stft_raw_io {
  const IO& io;
  static PFA_DEV unsigned in_off(unsigned, unsigned j) { return j; }
  static constexpr unsigned in_step(int k) { return k; }
  PFA_DEV auto load(unsigned slot, unsigned step) const { return io.load_pair(io.own, slot, step); }
};

/// Pass 0 of a direct-io multi-pass configuration: wg_pass0_load of the unwindowed pairs, the window in chunks of WCH
/// pairs -- chunk c + 1 is requested before chunk c is multiplied, and the scheduler may not gather the requests -- and
/// wg_pass0_compute.  The same arithmetic in the same order as wg_pass<Cfg, false, 0> on windowed loads.
template <typename Cfg, typename IO>
PFA_DEV void stft_pass0(const IO& io, unsigned f, cx<typename Cfg::T>* lds, int tid) {
  using T = typename Cfg::T;
  constexpr int R = Cfg::Seq::r[0];
  constexpr int NB = Cfg::N / R;
  constexpr int BPT = Cfg::bpt(0);
  constexpr bool ragged = (NB % Cfg::TPF) != 0;
  constexpr int WCH = sizeof(T) == 4 ? 4 : 2;
  constexpr int NC = (R + WCH - 1) / WCH;
  cx<T> v[BPT][R];
  wg_pass0_load<Cfg, false>(stft_raw_io<IO>{io}, f, tid, v);
  sfor<0, BPT>([&](auto i_) PFA_LAMBDA {
    constexpr int i = decltype(i_)::value;
    const unsigned j = tid + i * Cfg::TPF;
    if (!ragged || j < NB) {
      const cx<T>* wp = io.win + j;
      cx<T> w[2][WCH];
      sfor<0, WCH>([&](auto u_) PFA_LAMBDA {
        constexpr int u = decltype(u_)::value;
        if constexpr (u < R) w[0][u] = wp[u * NB];
      });
      sfor<0, NC>([&](auto c_) PFA_LAMBDA {
        constexpr int c = decltype(c_)::value;
        sfor<0, WCH>([&](auto u_) PFA_LAMBDA {
          constexpr int t = (c + 1) * WCH + decltype(u_)::value;
          if constexpr (t < R) w[(c + 1) & 1][decltype(u_)::value] = wp[t * NB];
        });
        __builtin_amdgcn_sched_barrier(0);
        sfor<0, WCH>([&](auto u_) PFA_LAMBDA {
          constexpr int t = c * WCH + decltype(u_)::value;
          if constexpr (t < R) {
            v[i][t].re *= w[c & 1][decltype(u_)::value].re;
            v[i][t].im *= w[c & 1][decltype(u_)::value].im;
          }
        });
        __builtin_amdgcn_sched_barrier(0);
      });
    }
  });
  wg_pass0_compute<Cfg>(v, lds, tid);
}

/// `n_signals` signals of in_length real scalars (pitch in_pitch) -> n_frames frames of Cfg::N + 1 bins each (pitches
/// frame_pitch / out_pitch, complex elements); `in` and `out` must not overlap.  tw: the real plan's tables.  win: the
/// window, N = 2 * Cfg::N scalars.  lead / hop: see the head of the file.  wg_twiddle_prologue; the persistent loop and
/// the passes are stockham_wg_rols_kernel's, the untangle step is stockham_wg_real_body's.
template <typename Cfg, bool REFLECT>
__global__ __launch_bounds__(Cfg::WG, Cfg::OCC) void stockham_wg_stft_kernel(
    const void* in, void* out, const cx<typename Cfg::T>* __restrict__ tw, const void* __restrict__ win, unsigned n_signals,
    unsigned n_frames, typename Cfg::T scale, unsigned lead, unsigned hop, unsigned in_length, unsigned in_pitch,
    unsigned frame_pitch, unsigned out_pitch) {
  using T = typename Cfg::T;
  using Seq = typename Cfg::Seq;
  constexpr int M = Cfg::N;
  static_assert(Cfg::LDS_PER_FFT > 0, "LDS-resident configurations only");
  constexpr int KH = M / 2 + 1;                        // work items of the untangle step: k = 0 ... M/2
  constexpr int UPT = (KH + Cfg::TPF - 1) / Cfg::TPF;  // ... per lane
  constexpr int CH = Cfg::FPW * M;                     // staged copies (STAGED configurations)
  constexpr int EPT = (CH + Cfg::WG - 1) / Cfg::WG;
  extern __shared__ __attribute__((aligned(16))) char pfa_smem[];
  const int f = threadIdx.x / Cfg::TPF;
  const int tid = threadIdx.x % Cfg::TPF;
  cx<T>* all = reinterpret_cast<cx<T>*>(pfa_smem);
  cx<T>* lds = all + f * Cfg::LDS_PER_FFT;

  cx<T> twr[Cfg::TWR_TOTAL];
  wg_twiddle_prologue<Cfg>(tw, tid, twr, all);
  const unsigned ngroups = (n_signals * n_frames + Cfg::FPW - 1) / Cfg::FPW;  // (the host keeps the row count below 2^31)
  for (unsigned g = blockIdx.x; g < ngroups; g += gridDim.x) {
    const cx<T>* twp = tw;
    const void* winp = win;
    if constexpr (Cfg::TWM == TW_GLOBAL) {
      asm volatile("" : "+s"(twp));  // (stockham_wg_body: keep the table reads inside the loop)
    }
    asm volatile("" : "+s"(winp));  // (... and the window's: it stays in L1 / L2, not in registers across the loop)
    const stft_io<T, M, Cfg::FPW, Cfg::AUX, REFLECT> io(in, out, winp, g, f, n_signals, n_frames, lead, hop, in_length,
                                                        in_pitch, frame_pitch, out_pitch);
    const cx<T>* wk = twp + Seq::tw_total;
    if constexpr (Cfg::STAGED) {
      ols_row* rows = reinterpret_cast<ols_row*>(pfa_smem + real_lds_bytes<Cfg>());
      if (tid == 0) rows[f] = io.own;
      __syncthreads();
      sfor<0, EPT>([&](auto k_) PFA_LAMBDA {
        const unsigned e = threadIdx.x + decltype(k_)::value * Cfg::WG;
        if (CH % Cfg::WG == 0 || e < CH) {
          all[(e / M) * Cfg::LDS_PER_FFT + lds_pad<Cfg>(e % M)] = io.load_in(rows[e / M], e % M);
        }
      });
      __syncthreads();
    }
    // Z = DFT_M(windowed frame as pairs), natural order, unscaled, in the image (the last pass ends with a barrier)
    if constexpr (!Cfg::STAGED && Cfg::NP >= 2) {
      stft_pass0<Cfg>(io, f, lds, tid);
      wg_passes<Cfg, false, 1, WG_LAST_TO_LDS>(io, f, lds, tid, twp, twr, scale);
    } else {
      wg_passes<Cfg, false, 0, WG_LAST_TO_LDS>(io, f, lds, tid, twp, twr, scale);
    }
    // the R2C untangle step of stockham_wg_real_body: bins k and M - k of the lane's own row
    const T h = scale * T(0.5);
    sfor<0, UPT>([&](auto i_) PFA_LAMBDA {
      const unsigned k = tid + decltype(i_)::value * Cfg::TPF;
      if (KH % Cfg::TPF == 0 || k < KH) {
        const cx<T> a = lds[lds_pad<Cfg>(k)];
        if (k == 0) {
          io.bin_store(cx<T>{scale * (a.re + a.im), T(0)}, 0);
          io.bin_store(cx<T>{scale * (a.re - a.im), T(0)}, M);
        } else {
          const cx<T> b = lds[lds_pad<Cfg>(M - k)];
          const cx<T> s{a.re + b.re, a.im - b.im}, d{a.re - b.re, a.im + b.im};
          const cx<T> t = cmul(d, wk[k]);
          io.bin_store(cx<T>{h * (s.re + t.im), h * (s.im - t.re)}, k);
          if (2 * k != M) io.bin_store(cx<T>{h * (s.re - t.im), -(h * (s.im + t.re))}, M - k);
        }
      }
    });
    __syncthreads();  // the next group's passes (and row windows) overwrite the images
  }
}

}  // namespace pfa
