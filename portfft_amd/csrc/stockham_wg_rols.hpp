// Overlap-save FIR filtering of long REAL signals in ONE kernel: stockham_wg_rconv.hpp's pass structure and pair step
// behind the windowed io of stockham_wg_ols.hpp, restated for scalars.  A row of the kernel is one (signal i, segment s)
// pair: a window of N = 2 * M input scalars is read as M scalar pairs, transformed, multiplied with the filter's half
// spectrum and transformed back, and only the outputs that circular aliasing did not touch are stored, at their place
// in the output signal.  Nothing is gathered, converted or copied around the kernel.
//
// No counterpart in the reference; reached through pfft_execute_filter on a plan with PFFT_EXT_REAL_CONVOLUTION whose
// filter was given as taps (pfft_plan_set_filter_taps).
//
// Geometry (all kernel arguments; lengths, pitches, lead and hop count SCALARS):
//   rows      r = i * n_seg + s,  i < n_signals,  s < n_seg = ceil(out_length / hop);  FPW consecutive rows per group
//   window    image slot j of row (i, s) holds the pair (x_i[e0 + 2j], x_i[e0 + 2j + 1]), e0 = s * hop - lead, zero
//             outside [0, in_length)
//   stores    result scalar lead + m goes to y_i[s * hop + m] for m < nvalid = min(hop, out_length - s * hop)
//   filter    row (i, s) takes half spectrum i mod n_filters; CORR conjugates it
// The host chooses `lead` and `hop` EVEN (convolution: lead = K - 1 rounded up, hop = N - lead; correlation: lead = 0,
// hop = N - K + 1 rounded down), so every window and every store starts on a pair.  A pair is then cut only by the end
// of a signal -- an odd in_length on load, an odd last nvalid on store -- and those two cases are predicated per
// scalar, explicitly: one add and one unsigned compare per scalar, never 32-bit wrap-around of an offset and never the
// range check of the buffer resource (stockham_wg_ols.hpp's rule).  Signals start at i * pitch scalars, so a pair
// access is only scalar-aligned, as the accesses of the R2C kernel with an odd forward_offset are.
//
// As in stockham_wg_ols.hpp: the resources start `lead` scalars in front of the group's first signal so that no part of
// an address is negative; FPW = 1 keeps the window uniform; STAGED configurations keep the FPW windows in LDS behind the
// images; rows behind the last signal have empty windows and still reach every barrier; in place is NOT safe and the
// host refuses overlapping buffers.
#pragma once
#include "stockham_wg_ols.hpp"
#include "stockham_wg_rconv.hpp"

namespace pfa {

/// LDS of the real overlap-save kernels of configuration Cfg (an M-point wg_cfg): the real kernels', and the windows of
/// the group's rows (ols_row, in scalars) behind it where the staged copies need them
template <typename Cfg>
constexpr size_t rols_lds_bytes() {
  return real_lds_bytes<Cfg>() + (Cfg::STAGED ? size_t(Cfg::FPW) * sizeof(ols_row) : 0);
}

/// Addressing of one group's rows: window_io counting scalars (stockham_wg_ols.hpp)
template <typename T, int M, int FPW, int AUX>
using rols_io = window_io<T, M, FPW, AUX, true>;

/// `n_signals` signals of in_length real scalars (pitch in_pitch) -> as many of out_length (pitch out_pitch), each in
/// n_seg segments of N = 2 * Cfg::N scalars; `in` and `out` must not overlap.  tw: the real plan's tables.  filt:
/// n_filters half spectra of Cfg::N + 1 bins, packed (of taps zero-padded to N); signal i takes i mod n_filters.  CORR:
/// the conjugate spectrum.  lead / hop: even, see the head of the file.  wg_twiddle_prologue; the persistent loop, the
/// passes and the pair step are stockham_wg_rconv_kernel's.
template <typename Cfg, bool CORR>
__global__ __launch_bounds__(Cfg::WG, Cfg::OCC) void stockham_wg_rols_kernel(
    const void* in, void* out, const cx<typename Cfg::T>* __restrict__ tw, const cx<typename Cfg::T>* __restrict__ filt,
    unsigned n_signals, unsigned n_seg, unsigned n_filters, typename Cfg::T scale, unsigned lead, unsigned hop,
    unsigned in_length, unsigned out_length, unsigned in_pitch, unsigned out_pitch) {
  using T = typename Cfg::T;
  using Seq = typename Cfg::Seq;
  constexpr int M = Cfg::N;
  static_assert(Cfg::LDS_PER_FFT > 0, "LDS-resident configurations only");
  constexpr int CH = Cfg::FPW * M;  // staged copies (STAGED configurations)
  constexpr int EPT = (CH + Cfg::WG - 1) / Cfg::WG;
  extern __shared__ __attribute__((aligned(16))) char pfa_smem[];
  const int f = threadIdx.x / Cfg::TPF;
  const int tid = threadIdx.x % Cfg::TPF;
  cx<T>* all = reinterpret_cast<cx<T>*>(pfa_smem);
  cx<T>* lds = all + f * Cfg::LDS_PER_FFT;

  cx<T> twr[Cfg::TWR_TOTAL];
  wg_twiddle_prologue<Cfg>(tw, tid, twr, all);
  const unsigned ngroups = (n_signals * n_seg + Cfg::FPW - 1) / Cfg::FPW;  // (the host keeps the row count below 2^31)
  for (unsigned g = blockIdx.x; g < ngroups; g += gridDim.x) {
    const rols_io<T, M, Cfg::FPW, Cfg::AUX> io(in, out, g, f, n_signals, n_seg, lead, hop, in_length, out_length, in_pitch,
                                               out_pitch);
    const cx<T>* twp = tw;
    if constexpr (Cfg::TWM == TW_GLOBAL) {
      asm volatile("" : "+s"(twp));  // (stockham_wg_body: keep the table reads inside the loop)
    }
    const cx<T>* wk = twp + Seq::tw_total;
    // the filter belongs to the signal (one modulo per group trip)
    const cx<T>* hp = filt + static_cast<size_t>(io.sig % n_filters) * (M + 1);
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
    // 1. Z = DFT_M(window as pairs), natural order, unscaled, in the image (the last pass ends with a barrier)
    wg_passes<Cfg, false, 0, WG_LAST_TO_LDS>(io, f, lds, tid, twp, twr, scale);
    // 2. untangle, product, re-tangle: every lane rewrites the two slots it read
    rconv_pair_step<Cfg, CORR, 2>(lds, tid, wk, hp);
    __syncthreads();
    // 3. scale * conj(DFT_M(image)); only the alias-free scalars of a row leave
    wg_passes<Cfg, true, 0, WG_FIRST_FROM_LDS>(io, f, lds, tid, twp, twr, scale);
    if constexpr (Cfg::STAGED) {
      const ols_row* rows = reinterpret_cast<const ols_row*>(pfa_smem + real_lds_bytes<Cfg>());
      sfor<0, EPT>([&](auto k_) PFA_LAMBDA {
        const unsigned e = threadIdx.x + decltype(k_)::value * Cfg::WG;
        if (CH % Cfg::WG == 0 || e < CH) {
          const cx<T> y = all[(e / M) * Cfg::LDS_PER_FFT + lds_pad<Cfg>(e % M)];
          io.store_out(cx<T>{y.re * scale, -(y.im * scale)}, rows[e / M], e % M);
        }
      });
      __syncthreads();  // (the images and the windows are the next trip's to write)
    }
  }
}

}  // namespace pfa
