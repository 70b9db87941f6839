// Circular convolution (or correlation) of every row with a filter given in the frequency domain, in ONE kernel: the
// forward N-point passes of stockham_wg.hpp straight from HBM into the LDS image, a pointwise product with the filter
// spectrum on the image, and the inverse passes from the image straight to HBM -- a row is read once and written once,
// where forward transform, multiply and backward transform move six arrays through HBM.
//
// No counterpart in the reference; reached through PFFT_EXT_CONVOLUTION (pfft_execute_convolve).
//
// With X = DFT_N(x) and H the filter spectrum of the row (filter `row mod n_filters`, N elements each, packed):
//   1. image = X, natural order, unscaled                         HBM -> LDS: passes with WG_LAST_TO_LDS (as R2C)
//   2. image[k] = conj(X[k] H[k])      (CORR: conj(X[k] conj(H[k])))   lanes take consecutive k; H through L1 / L2
//   3. out = scale * conj(DFT_N(image)) = scale * N * IDFT_N(X H)  LDS -> HBM: passes with WG_FIRST_FROM_LDS (as C2R)
// The inverse is the conjugate-in / conjugate-out form of the forward passes: step 2 writes the conjugate (no
// conjugating pass over the data) and the last pass conjugates and scales on its way to HBM as it always does.
// `scale` is forward_scale * backward_scale of the descriptor: what compute_forward, a multiply and compute_backward of
// the same descriptor produce.
//
// Step 2 on the image: lane `tid` of a row takes k = tid, tid + TPF, ...: a wave reads and writes consecutive 8- or
// 16-byte slots (ds_read_b64 / ds_read_b128 on consecutive banks, the padding of lds_pad aside), and the H reads of a
// wave are one contiguous segment.  Every lane rewrites exactly the slots it read, so the step needs no barrier inside.
// It walks its slots in chunks of at most 4 per lane inside a rolled loop (stockham_wg_bluestein.hpp, step 3: unrolled
// whole, its loads would all be in flight at once and push the passes' registers into scratch).
//
// LDS: the images (and the TWL copy) of the complex kernel of N points; a single-pass configuration, which needs no
// image for the complex transform, gets one here (conv_lds_bytes = real_lds_bytes).  Twiddles: the N-point tables of
// the complex kernel, nothing behind them.
//
// In place is safe by construction: every HBM load of a group happens before the first barrier of its passes (the
// staged copy-in or pass 0) and every store behind the last one (the last pass or the staged copy-out), and groups own
// disjoint rows.  Rows may be padded (pitches idist / odist >= N); only the N elements of a row are read or written.
#pragma once
#include "stockham_wg_real.hpp"

namespace pfa {

/// LDS of the convolution kernels of configuration Cfg (an N-point wg_cfg): an image also for single-pass configurations
template <typename Cfg>
constexpr size_t conv_lds_bytes() {
  return real_lds_bytes<Cfg>();
}

/// Addressing of one group's rows: element j of row f at f * pitch + j, pitches in complex elements.  The resources
/// cover the rows of the group that exist: missing rows read zeros, their stores are dropped by the range check
/// (packed_io).
template <typename T, int N, int FPW, int AUX>
struct conv_io {
  static constexpr unsigned ES = sizeof(cx<T>);
  __amdgpu_buffer_rsrc_t rin, rout;
  unsigned ip, op;  // row pitches in bytes
  PFA_DEV conv_io(const void* in, void* out, long long g, long long nfft, unsigned idist, unsigned odist)
      : ip(idist * ES), op(odist * ES) {
    wg_live_rows<FPW>(rin, rout, in, out, g, nfft, ip, op);
  }
  PFA_DEV unsigned in_off(unsigned f, unsigned j) const { return f * ip + j * ES; }
  PFA_DEV unsigned out_off(unsigned f, unsigned j) const { return f * op + j * ES; }
  static constexpr unsigned in_step(int k) { return k * ES; }
  static constexpr unsigned out_step(int k) { return k * ES; }
  // the staged copies: element e of the group's FPW * N
  PFA_DEV unsigned in_elem(unsigned e) const { return (e / N) * ip + (e % N) * ES; }
  PFA_DEV unsigned out_elem(unsigned e) const { return (e / N) * op + (e % N) * ES; }
  PFA_DEV cx<T> load(unsigned voff, unsigned soff) const { return buf_load<T, AUX>(rin, voff, soff); }
  PFA_DEV void store(cx<T> v, unsigned voff, unsigned soff) const { buf_store<T, AUX>(v, rout, voff, soff); }
};

/// `nfft` rows of Cfg::N complex elements (pitch idist) -> as many rows (pitch odist); `in` and `out` may be the same
/// buffer.  tw: the Cfg::N-point tables.  filt: n_filters spectra of Cfg::N elements, packed; row t takes t mod n_filters.
/// CORR: the conjugate spectrum (correlation, the adjoint).  wg_twiddle_prologue and the persistent loop of
/// stockham_wg_real_body.
template <typename Cfg, bool CORR>
__global__ __launch_bounds__(Cfg::WG, Cfg::OCC) void stockham_wg_conv_kernel(
    const void* in, void* out, const cx<typename Cfg::T>* __restrict__ tw, const cx<typename Cfg::T>* __restrict__ filt,
    long long nfft, unsigned n_filters, typename Cfg::T scale, unsigned idist, unsigned odist) {
  using T = typename Cfg::T;
  constexpr int N = Cfg::N;
  static_assert(Cfg::LDS_PER_FFT > 0, "LDS-resident configurations only");
  constexpr int UPT = (N + Cfg::TPF - 1) / Cfg::TPF;  // image slots per lane in step 2
  constexpr int UCH = UPT < 4 ? UPT : 4;              // ... per trip of its loop
  constexpr int CH = Cfg::FPW * N;                    // staged copies (STAGED configurations)
  constexpr int EPT = (CH + Cfg::WG - 1) / Cfg::WG;
  extern __shared__ __attribute__((aligned(16))) char pfa_smem[];
  const int f = threadIdx.x / Cfg::TPF;
  const int tid = threadIdx.x % Cfg::TPF;
  cx<T>* all = reinterpret_cast<cx<T>*>(pfa_smem);
  cx<T>* lds = all + f * Cfg::LDS_PER_FFT;

  cx<T> twr[Cfg::TWR_TOTAL];
  wg_twiddle_prologue<Cfg>(tw, tid, twr, all);
  // filter of this lane's row: (g * FPW + f) mod n_filters, kept up to date by adding the loop's step mod n_filters
  const unsigned long long nf = n_filters;
  unsigned hrow = static_cast<unsigned>((static_cast<unsigned long long>(blockIdx.x) * Cfg::FPW + f) % nf);
  const unsigned hstep = static_cast<unsigned>((static_cast<unsigned long long>(gridDim.x) * Cfg::FPW) % nf);
  const long long ngroups = (nfft + Cfg::FPW - 1) / Cfg::FPW;
  for (long long g = blockIdx.x; g < ngroups; g += gridDim.x) {
    const conv_io<T, N, Cfg::FPW, Cfg::AUX> io(in, out, g, nfft, idist, odist);
    const cx<T>* twp = tw;
    if constexpr (Cfg::TWM == TW_GLOBAL) {
      asm volatile("" : "+s"(twp));  // (stockham_wg_body: keep the table reads inside the loop)
    }
    const cx<T>* hp = filt + static_cast<size_t>(hrow) * N;
    hrow = hrow >= n_filters - hstep ? hrow - (n_filters - hstep) : hrow + hstep;
    if constexpr (Cfg::STAGED) {
      sfor<0, EPT>([&](auto k_) PFA_LAMBDA {
        const unsigned e = threadIdx.x + decltype(k_)::value * Cfg::WG;
        if (CH % Cfg::WG == 0 || e < CH) {
          all[(e / N) * Cfg::LDS_PER_FFT + lds_pad<Cfg>(e % N)] = io.load(io.in_elem(e), 0);
        }
      });
      __syncthreads();
    }
    // 1. X = DFT_N(x), natural order, unscaled, in the image (the last pass ends with a barrier)
    wg_passes<Cfg, false, 0, WG_LAST_TO_LDS>(io, f, lds, tid, twp, twr, scale);
    // 2. conj(X H): what the conjugate-in backward passes read; every lane rewrites the slots it read
#pragma nounroll
    for (int c = 0; c < UPT; c += UCH) {
      sfor<0, UCH>([&](auto i_) PFA_LAMBDA {
        const unsigned k = tid + (c + decltype(i_)::value) * Cfg::TPF;
        if (k < N) {
          cx<T> h = hp[k];
          if constexpr (CORR) h.im = -h.im;
          const cx<T> y = cmul(lds[lds_pad<Cfg>(k)], h);
          lds[lds_pad<Cfg>(k)] = cx<T>{y.re, -y.im};
        }
      });
    }
    __syncthreads();
    // 3. scale * conj(DFT_N(image)).  (Every lane has read the image into registers before the last pass stores: the
    // next group's passes may write it.)
    wg_passes<Cfg, true, 0, WG_FIRST_FROM_LDS>(io, f, lds, tid, twp, twr, scale);
    if constexpr (Cfg::STAGED) {
      sfor<0, EPT>([&](auto k_) PFA_LAMBDA {
        const unsigned e = threadIdx.x + decltype(k_)::value * Cfg::WG;
        if (CH % Cfg::WG == 0 || e < CH) {
          const cx<T> y = all[(e / N) * Cfg::LDS_PER_FFT + lds_pad<Cfg>(e % N)];
          io.store(cx<T>{y.re * scale, -(y.im * scale)}, io.out_elem(e), 0);
        }
      });
      __syncthreads();
    }
  }
}

}  // namespace pfa
