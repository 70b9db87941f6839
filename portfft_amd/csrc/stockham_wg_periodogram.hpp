// Power spectrogram and Welch periodogram of long REAL signals in ONE kernel: the io, pass 0 and passes of
// stockham_wg_stft.hpp, with the square taken in the untangle step and consecutive frames summed before anything is
// stored.  A row of the kernel is one OUTPUT row, a unit u = i * R + c (signal i, row c < R = ceil(n_frames / avg_frames)):
//   P_i[c][k] = sum over f = c * A ... min((c + 1) * A, n_frames) - 1 of |X_i[f][k]|^2,   k = 0 ... M,  A = avg_frames
// X_i[f] is what stockham_wg_stft_kernel stores for frame f (window, extension, hop, lead and `scale` as there).  A = 1
// is the power spectrogram, A = n_frames Welch's sum with one row per signal.  A sum, not a mean; no one-sided doubling.
//
// No counterpart in the reference; reached through pfft_execute_periodogram on a plan of the REAL domain whose window
// was set (pfft_plan_set_periodogram_window).
//
// Geometry (all kernel arguments; lengths, pitches, lead and hop count SCALARS on both sides):
//   units     u = i * R + c; FPW consecutive units per group, one per lane-set
//   frames    all lane-sets of a group run a = 0 ... A - 1 together (the barriers are group-wide); lane-set f transforms
//             frame fr = c * A + a of its unit, the row facts (e0, ibase, kind) rebuilt per a.  A frame behind the last one
//             of its row, or a unit behind the last one, is a DEAD row (STFT_ROW_DEAD): it loads nothing, reaches every
//             barrier and adds nothing.
//   stores    bin k <= M of unit (i, c) goes to out + i * out_pitch + c * row_pitch + k, once, after the loop; nothing
//             else is written
// Every (i, c, k) has ONE accumulator -- a register of the lane that untangles bin k of that row -- and it takes its
// frames in ascending f: the result does not depend on the grid, on FPW or on how many signals share a call, bit for
// bit.  No atomics.  The accumulators are 2 * UPT scalars per lane, UPT = ceil((M / 2 + 1) / TPF).
//
// The rules at the head of stockham_wg_stft.hpp stay in force: every scalar is predicated on its own index, no part of
// an address is negative, the range check of a resource is never relied upon.  The input resource starts at the group's
// first signal (`lead` in front of it for zero extension), the output resource at the group's first unit; the host
// (periodogram_geometry_of) keeps both reaches below 4 GiB.  The lane-sets of a group read frames A * hop apart; each
// walks the overlapping frames of its own row one after the other.
//
// Barriers: one at the end of every frame (the next frame's passes, staged copies and row windows overwrite the images
// the untangle step read).  The stores of a group come behind its last barrier and touch no LDS, so none follows them.
#pragma once
#include "stockham_wg_stft.hpp"

namespace pfa {

/// LDS of the periodogram kernels of configuration Cfg: the STFT kernels' (images, row windows of STAGED configurations)
template <typename Cfg>
constexpr size_t periodogram_lds_bytes() {
  return stft_lds_bytes<Cfg>();
}

/// stft_io with the unit mapping: the resources and the lane's unit once per group, the frame's row facts per step
template <typename T, int M, int FPW, int AUX, bool REFLECT>
struct periodogram_io : stft_io<T, M, FPW, AUX, REFLECT> {
  using base = stft_io<T, M, FPW, AUX, REFLECT>;
  static constexpr unsigned SB = sizeof(T);
  unsigned first;  // the first frame of the lane's unit
  unsigned count;  // live frames of the lane's unit (0: a unit behind the last one)
  unsigned ioff;   // scalar of the input resource where the unit's signal starts, `lead` included (zero extension)
  unsigned obase;  // scalar of the output resource that bin 0 of the unit goes to

  PFA_DEV periodogram_io(const void* in, void* out, const void* win_, unsigned g, unsigned f, unsigned n_signals,
                         unsigned n_frames, unsigned n_rows, unsigned avg, unsigned lead, unsigned in_length_,
                         unsigned in_pitch, unsigned row_pitch, unsigned out_pitch)
      : base(win_, in_length_) {
    const unsigned r0 = g * FPW;  // (uniform; the group exists, so i0 < n_signals)
    const unsigned i0 = r0 / n_rows;
    const unsigned c0 = r0 - i0 * n_rows;
    const unsigned shift = REFLECT ? 0u : lead;
    const unsigned long long after = n_signals - 1 - i0;
    const unsigned long long ibytes = (after * in_pitch + in_length_ + shift) * SB;
    const unsigned long long ofirst = static_cast<unsigned long long>(i0) * out_pitch + static_cast<unsigned long long>(c0) * row_pitch;
    const unsigned long long obytes =
        (after * out_pitch + static_cast<unsigned long long>(n_rows - 1 - c0) * row_pitch + M + 1) * SB;
    const long long ifirst = static_cast<long long>(i0) * in_pitch - shift;
    this->rin = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(static_cast<const char*>(in)) + ifirst * SB, 0,
                                                  ibytes > 0xFFFFFFFFull ? 0xFFFFFFFFu : static_cast<unsigned>(ibytes), 0x00020000);
    this->rout = __builtin_amdgcn_make_buffer_rsrc(static_cast<char*>(out) + ofirst * SB, 0,
                                                   obytes > 0xFFFFFFFFull ? 0xFFFFFFFFu : static_cast<unsigned>(obytes), 0x00020000);
    const unsigned u = r0 + (FPW == 1 ? 0u : f);  // (one unit per group: the row is uniform, and kept in SGPRs)
    const unsigned sig = u / n_rows;
    const unsigned c = u - sig * n_rows;
    const unsigned di = sig - i0;
    first = c * avg;  // (c < n_rows: below n_frames)
    const unsigned left = n_frames - first;
    count = sig < n_signals ? (left < avg ? left : avg) : 0u;
    ioff = di * in_pitch + shift;
    // (the host keeps the units of a group within 4 GiB: the difference fits also where a product wrapped)
    obase = di * out_pitch + c * row_pitch - c0 * row_pitch;
  }
  /// the row facts of step a: frame first + a of the lane's unit, or a dead row
  PFA_DEV void set_frame(unsigned a, unsigned lead, unsigned hop) {
    const bool live = a < count;
    const unsigned e0 = (first + a) * hop - lead;  // (a live frame: the host's bound on the last frame keeps it exact)
    this->own.e0 = live ? e0 : 0xC0000000u;
    this->own.ibase = ioff + e0;  // (not negative where it is used: e0 >= -lead, an inside row has e0 >= 0)
    this->own.obase = obase;
    unsigned kind = live ? STFT_ROW_INSIDE : STFT_ROW_DEAD;
    if constexpr (REFLECT) {
      if (live && !(e0 < this->in_length && this->in_length - e0 >= 2u * M)) kind = STFT_ROW_EDGE;
    }
    this->own.nvalid = kind;
  }
  /// the sum of bin k of the lane's own unit
  PFA_DEV void sum_store(T v, unsigned k) const {
    if (count != 0) buf_store_scalar<T, AUX>(v, this->rout, (obase + k) * SB, 0);
  }
};

/// `n_signals` signals of in_length real scalars (pitch in_pitch) -> ceil(n_frames / avg_frames) rows of Cfg::N + 1 real
/// sums each (pitches row_pitch / out_pitch, scalars); `in` and `out` must not overlap.  tw: the real plan's tables.
/// win: the window, N = 2 * Cfg::N scalars.  lead / hop / scale: as stockham_wg_stft_kernel.  The persistent loop, the
/// staged copy, the passes and the untangle arithmetic are that kernel's; see the head of the file for the rest.
template <typename Cfg, bool REFLECT>
__global__ __launch_bounds__(Cfg::WG, Cfg::OCC) void stockham_wg_periodogram_kernel(
    const void* in, void* out, const cx<typename Cfg::T>* __restrict__ tw, const void* __restrict__ win, unsigned n_signals,
    unsigned n_frames, typename Cfg::T scale, unsigned lead, unsigned hop, unsigned in_length, unsigned in_pitch,
    unsigned row_pitch, unsigned out_pitch, unsigned avg_frames) {
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
  // R = ceil(n_frames / avg_frames), without the sum that could pass 2^32
  const unsigned rows_of = n_frames / avg_frames + (n_frames % avg_frames != 0 ? 1u : 0u);
  const unsigned ngroups = (n_signals * rows_of + Cfg::FPW - 1) / Cfg::FPW;  // (the host keeps the unit count below 2^31)
  const T h = scale * T(0.5);
  for (unsigned g = blockIdx.x; g < ngroups; g += gridDim.x) {
    periodogram_io<T, M, Cfg::FPW, Cfg::AUX, REFLECT> io(in, out, win, g, f, n_signals, n_frames, rows_of, avg_frames, lead,
                                                         in_length, in_pitch, row_pitch, out_pitch);
    T acc[UPT][2];  // [i][0]: bin k = tid + i * TPF, [i][1]: bin M - k
    sfor<0, UPT>([&](auto i_) PFA_LAMBDA { acc[decltype(i_)::value][0] = acc[decltype(i_)::value][1] = T(0); });
    for (unsigned a = 0; a < avg_frames; ++a) {
      const cx<T>* twp = tw;
      const void* winp = win;
      if constexpr (Cfg::TWM == TW_GLOBAL) {
        asm volatile("" : "+s"(twp));  // (stockham_wg_body: keep the table reads inside the loop)
      }
      asm volatile("" : "+s"(winp));  // (... and the window's: it stays in L1 / L2, not in registers across the loop)
      io.win = static_cast<const cx<T>*>(winp);
      io.set_frame(a, lead, hop);
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
      // the untangle step of stockham_wg_stft_kernel, squared; a dead row adds nothing (its image need not be finite:
      // zero times the window)
      const bool live = a < io.count;
      sfor<0, UPT>([&](auto i_) PFA_LAMBDA {
        constexpr int i = decltype(i_)::value;
        const unsigned k = tid + i * Cfg::TPF;
        if ((KH % Cfg::TPF == 0 || k < KH) && live) {
          const cx<T> x = lds[lds_pad<Cfg>(k)];
          if (k == 0) {
            const T v0 = scale * (x.re + x.im), vm = scale * (x.re - x.im);
            acc[i][0] += v0 * v0;
            acc[i][1] += vm * vm;
          } else {
            const cx<T> b = lds[lds_pad<Cfg>(M - k)];
            const cx<T> s{x.re + b.re, x.im - b.im}, d{x.re - b.re, x.im + b.im};
            const cx<T> t = cmul(d, wk[k]);
            const cx<T> vk{h * (s.re + t.im), h * (s.im - t.re)}, vm{h * (s.re - t.im), -(h * (s.im + t.re))};
            acc[i][0] += vk.re * vk.re + vk.im * vk.im;
            acc[i][1] += vm.re * vm.re + vm.im * vm.im;  // (2k = M: never stored)
          }
        }
      });
      __syncthreads();  // the next frame's passes (and row windows) overwrite the images
    }
    sfor<0, UPT>([&](auto i_) PFA_LAMBDA {
      constexpr int i = decltype(i_)::value;
      const unsigned k = tid + i * Cfg::TPF;
      if (KH % Cfg::TPF == 0 || k < KH) {
        io.sum_store(acc[i][0], k);
        if (2 * k != M) io.sum_store(acc[i][1], M - k);
      }
    });
  }
}

}  // namespace pfa
