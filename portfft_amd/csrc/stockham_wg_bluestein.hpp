// Complex 1-D transforms of ANY length N in ONE kernel (Bluestein's chirp-z algorithm): the DFT of N points written as
// a circular convolution of P >= 2N - 1 points, P a length with a work-group plan, with everything of length P kept
// in LDS -- a row is read once (N elements) and written once (N elements), as a smooth length is.
//
// No counterpart in the reference (it refuses lengths with a prime factor above its largest radix); reached through
// PFFT_EXT_ANY_LENGTH, and only for the lengths the ordinary planner refuses for their prime factor.
//
// With w[j] = exp(-i pi j^2 / N) and jk = (j^2 + k^2 - (k - j)^2) / 2:
//   X[k] = sum_j x[j] exp(-2 pi i jk / N) = w[k] * sum_j (x[j] w[j]) * conj(w[k - j])               k = 0 ... N - 1
// The sum is the convolution of a[j] = x[j] w[j] (j < N, zero up to P) with b[m] = conj(w[m]), |m| < N, placed
// circularly in P slots; k - j stays inside (-N, N), so P >= 2N - 1 slots do not alias.  With Bh = DFT_P(b) / P:
//   1. image[j] = x[j] w[j] (j < N), 0 (N <= j < P)                 HBM -> LDS, lanes take consecutive j
//   2. A = DFT_P(image)                                             the P-point passes of stockham_wg.hpp, LDS -> LDS
//   3. image[k] = conj(A[k] Bh[k])                                  Bh through L1 / L2
//   4. image = DFT_P(image) = conj(P * IDFT_P(A Bh))                the same passes: an LDS-to-LDS pass conjugates nothing
//   5. out[k] = scale * w[k] * conj(image[k])   (k < N)             LDS -> HBM, lanes take consecutive k
// The descriptor's backward transform is conj o forward o conj on the same tables (BWD): step 1 conjugates x, step 5
// the result; it is unnormalised like every backward transform here.
//
// N is a runtime argument: one code object per P serves every N with 2N - 1 <= P.
//
// LDS: the images (and the TWL copy) of the complex kernel of P points (bluestein_lds_bytes).  Tables: the plan's table
// carries w[0 ... N-1] and then Bh[0 ... P-1] behind the P-point twiddles (offset radix_list::tw_total), both computed
// on the host in long double.
//
// In place is safe by construction: every HBM load of a group happens before its first barrier and every store behind
// its last one, and groups own disjoint rows.  Rows may be padded (pitches idist / odist >= N); only the N elements of
// a row are read or written.
#pragma once
#include "stockham_wg.hpp"

namespace pfa {

/// LDS of the Bluestein kernel of configuration Cfg (a P-point wg_cfg)
template <typename Cfg>
constexpr size_t bluestein_lds_bytes() {
  return size_t(Cfg::LDS_PER_FFT * Cfg::FPW + Cfg::TWL_ELEMS) * sizeof(cx<typename Cfg::T>);
}

/// Addressing of one group's rows: element j of row f at f * pitch + j, pitches in complex elements.  The resources
/// cover the rows of the group that exist: missing rows read zeros, their stores are dropped by the range check
/// (packed_io).  The passes never touch HBM (LDS to LDS); they take the object for its type only.
template <typename T, int FPW, int AUX>
struct bluestein_io {
  static constexpr unsigned ES = sizeof(cx<T>);
  __amdgpu_buffer_rsrc_t rin, rout;
  unsigned ip, op;  // row pitches in bytes
  PFA_DEV bluestein_io(const void* in, void* out, long long g, long long nfft, unsigned idist, unsigned odist)
      : ip(idist * ES), op(odist * ES) {
    wg_live_rows<FPW>(rin, rout, in, out, g, nfft, ip, op);
  }
  PFA_DEV unsigned in_off(unsigned f, unsigned j) const { return f * ip + j * ES; }
  PFA_DEV unsigned out_off(unsigned f, unsigned j) const { return f * op + j * ES; }
  static constexpr unsigned in_step(int k) { return k * ES; }
  static constexpr unsigned out_step(int k) { return k * ES; }
  PFA_DEV cx<T> load(unsigned voff, unsigned soff) const { return buf_load<T, AUX>(rin, voff, soff); }
  PFA_DEV void store(cx<T> v, unsigned voff, unsigned soff) const { buf_store<T, AUX>(v, rout, voff, soff); }
};

/// wg_twiddle_prologue and the persistent loop of stockham_wg_real_body.
template <typename Cfg, bool BWD>
PFA_DEV void stockham_wg_bluestein_body(const void* in, void* out, const cx<typename Cfg::T>* __restrict__ tw,
                                        long long nfft, unsigned n, typename Cfg::T scale, unsigned idist,
                                        unsigned odist) {
  using T = typename Cfg::T;
  using Seq = typename Cfg::Seq;
  constexpr int P = Cfg::N;
  constexpr int EPT = P / Cfg::TPF;  // image slots per lane; the data (n <= P / 2) sits in the first half of them
  static_assert(Cfg::NP > 1 && P % Cfg::TPF == 0 && EPT % 2 == 0, "an LDS-resident power-of-two configuration");
  constexpr int DPT = EPT / 2;
  constexpr int CH = DPT < 4 ? DPT : 4;  // slots per lane and trip of steps 1, 3 and 5
  extern __shared__ __attribute__((aligned(16))) char pfa_smem[];
  const int f = threadIdx.x / Cfg::TPF;
  const int tid = threadIdx.x % Cfg::TPF;
  cx<T>* all = reinterpret_cast<cx<T>*>(pfa_smem);
  cx<T>* lds = all + f * Cfg::LDS_PER_FFT;

  cx<T> twr[Cfg::TWR_TOTAL];
  wg_twiddle_prologue<Cfg>(tw, tid, twr, all);
  const long long ngroups = (nfft + Cfg::FPW - 1) / Cfg::FPW;
  for (long long g = blockIdx.x; g < ngroups; g += gridDim.x) {
    const bluestein_io<T, Cfg::FPW, Cfg::AUX> io(in, out, g, nfft, idist, odist);
    const cx<T>* twp = tw;
    if constexpr (Cfg::TWM == TW_GLOBAL) {
      asm volatile("" : "+s"(twp));  // (stockham_wg_body: keep the table reads inside the loop)
    }
    const cx<T>* wj = twp + Seq::tw_total;  // w[0 ... n-1]
    const cx<T>* bh = wj + n;               // Bh[0 ... P-1]
    // 1. load and chirp; the zeros are written every time (the passes overwrite the image).  Steps 1, 3 and 5 walk
    // their slots in chunks of CH per lane inside rolled loops: unrolled whole, their loads would all be in flight at
    // once and push the passes' registers (TW_REGS: the resident twiddles) into scratch.
#pragma nounroll
    for (int c = 0; c < DPT; c += CH) {
      cx<T> x[CH], w[CH];
      sfor<0, CH>([&](auto i_) PFA_LAMBDA {
        constexpr int i = decltype(i_)::value;
        const unsigned j = tid + (c + i) * Cfg::TPF;
        x[i] = cx<T>{T(0), T(0)};
        w[i] = cx<T>{T(0), T(0)};
        if (j < n) {
          x[i] = io.load(io.in_off(f, j), 0);
          w[i] = wj[j];
        }
      });
      sfor<0, CH>([&](auto i_) PFA_LAMBDA {
        constexpr int i = decltype(i_)::value;
        const unsigned j = tid + (c + i) * Cfg::TPF;
        if constexpr (BWD) x[i].im = -x[i].im;
        lds[lds_pad<Cfg>(j)] = cmul(x[i], w[i]);
        lds[lds_pad<Cfg>(j + P / 2)] = cx<T>{T(0), T(0)};
      });
    }
    __syncthreads();
    // 2. A = DFT_P(a), natural order, in the image (the last pass ends with a barrier)
    wg_passes<Cfg, false, 0, WG_FIRST_FROM_LDS | WG_LAST_TO_LDS>(io, f, lds, tid, twp, twr, scale);
    // 3. conj(A Bh): what the conjugate-in backward passes read; every lane rewrites the slots it read
#pragma nounroll
    for (int c = 0; c < EPT; c += CH) {
      sfor<0, CH>([&](auto i_) PFA_LAMBDA {
        const unsigned k = tid + (c + decltype(i_)::value) * Cfg::TPF;
        const cx<T> y = cmul(lds[lds_pad<Cfg>(k)], bh[k]);
        lds[lds_pad<Cfg>(k)] = cx<T>{y.re, -y.im};
      });
    }
    __syncthreads();
    // 4. conj(P * IDFT_P(A Bh)).  BWD = true names the intent only: an LDS-to-LDS pass neither conjugates nor scales,
    // so this is the code of step 2; the two conjugations of the inverse are in step 3 and step 5.
    wg_passes<Cfg, true, 0, WG_FIRST_FROM_LDS | WG_LAST_TO_LDS>(io, f, lds, tid, twp, twr, scale);
    // 5. chirp and store
#pragma nounroll
    for (int c = 0; c < DPT; c += CH) {
      sfor<0, CH>([&](auto i_) PFA_LAMBDA {
        const unsigned k = tid + (c + decltype(i_)::value) * Cfg::TPF;
        if (k < n) {
          const cx<T> v = lds[lds_pad<Cfg>(k)];
          const cx<T> w = wj[k];
          cx<T> y{w.re * v.re + w.im * v.im, w.im * v.re - w.re * v.im};  // w conj(v)
          if constexpr (BWD) y.im = -y.im;
          y.re *= scale;
          y.im *= scale;
          io.store(y, io.out_off(f, k), 0);
        }
      });
    }
    __syncthreads();  // the next group's step 1 overwrites the images
  }
}

/// `n` complex elements per row (pitch idist) -> `n` complex elements (pitch odist), 2 * n - 1 <= Cfg::N; `in` and `out`
/// may be the same buffer.  tw: the Cfg::N-point tables, then w[0 ... n-1], then Bh[0 ... Cfg::N - 1].
template <typename Cfg, bool BWD>
__global__ __launch_bounds__(Cfg::WG, Cfg::OCC) void stockham_wg_bluestein_kernel(
    const void* in, void* out, const cx<typename Cfg::T>* __restrict__ tw, long long nfft, unsigned n,
    typename Cfg::T scale, unsigned idist, unsigned odist) {
  stockham_wg_bluestein_body<Cfg, BWD>(in, out, tw, nfft, n, scale, idist, odist);
}

}  // namespace pfa
