// Circular convolution (or correlation) of every REAL row of N = 2 * M scalars with a filter given as the M + 1 bins of
// its half spectrum, in ONE kernel: the R2C half of stockham_wg_real.hpp (M-point forward passes into the LDS image and
// the untangle step), the pointwise product of stockham_wg_conv.hpp and the C2R half (the re-tangle step and the M-point
// inverse passes from the image) -- the three steps between the pass sets fused into one pair step on the image.  A row
// is read once and written once, as scalars; the pass work is M points, not N.
//
// No counterpart in the reference; reached through PFFT_EXT_REAL_CONVOLUTION (pfft_execute_convolve on a REAL plan).
//
// With z[j] = x[2j] + i x[2j+1], Z = DFT_M(z), w_k = exp(-2 pi i k / N), H the filter of the row (filter `row mod
// n_filters`, M + 1 bins each, packed), work item k = 0 ... floor(M/2):
//   A = Z[k], B = conj(Z[M-k])
//   X[k] = ((A + B) - i w_k (A - B)) / 2          X[M-k] = conj((A + B) + i w_k (A - B)) / 2         (R2C)
//   Y[k] = X[k] H[k]                              Y[M-k] = X[M-k] H[M-k]                  (CORR: conj(H))
//   S = Y[k] + conj(Y[M-k]),  P = i conj(w_k) (Y[k] - conj(Y[M-k]))                                  (C2R)
//   slot k <- conj(S + P)                         slot M-k <- S - P
//   k = 0:  X[0] = Re Z0 + Im Z0, X[M] = Re Z0 - Im Z0, times Re H[0] and Re H[M] (their imaginary parts are ignored, as
//           C2R ignores them): slot 0 <- conj((Y0 + YM) + i (Y0 - YM));   2k = M: one slot
// The conjugates are what the conjugate-in backward passes read; the last pass conjugates and scales on its way to HBM,
// and x'[2j] = Re z'[j], x'[2j+1] = Im z'[j]:  out = scale * N * irfft(rfft(x) . H), scale = forward_scale *
// backward_scale (the 1/2 of R2C and the unnormalised C2R give the N).
//
// A lane rewrites exactly the two slots it read, so the pair step needs no barrier inside.  H[k] is read by ascending k
// and H[M-k] by descending k: one contiguous segment per wave each.  The step walks its work items in chunks of at most
// 4 per lane inside a rolled loop (stockham_wg_conv.hpp, step 2: unrolled whole, its loads would all be in flight at
// once and push the passes' registers into scratch).
//
// LDS: real_lds_bytes.  Twiddles: the real plan's table, the floor(M/2) + 1 values w_k behind the M-point tables.
//
// In place is safe by construction: every HBM load of a group happens before the first barrier of its passes (the
// staged copy-in or pass 0) and every store behind the last one, and groups own disjoint rows.
#pragma once
#include "stockham_wg_real.hpp"

namespace pfa {

/// Addressing of one group's rows: both sides are rows of N scalars with a pitch of `dist` SCALARS, accessed as M complex
/// elements per row (what the passes load and store).  The resources cover the rows of the group that exist: missing
/// rows read zeros, their stores are dropped by the range check (packed_io).
template <typename T, int M, int FPW, int AUX>
struct rconv_io {
  static constexpr unsigned ES = sizeof(cx<T>);
  __amdgpu_buffer_rsrc_t rin, rout;
  unsigned rp;  // row pitch in bytes
  PFA_DEV rconv_io(const void* in, void* out, long long g, long long nfft, unsigned dist)
      : rp(dist * static_cast<unsigned>(sizeof(T))) {
    const long long first = g * FPW;
    const long long left = nfft - first;
    const unsigned live = static_cast<unsigned>(left < FPW ? left : FPW);
    rin = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(static_cast<const char*>(in)) + first * rp, 0, live * rp,
                                            0x00020000);
    rout = __builtin_amdgcn_make_buffer_rsrc(static_cast<char*>(out) + first * rp, 0, live * rp, 0x00020000);
  }
  PFA_DEV unsigned in_off(unsigned f, unsigned j) const { return f * rp + j * ES; }
  PFA_DEV unsigned out_off(unsigned f, unsigned j) const { return f * rp + j * ES; }
  static constexpr unsigned in_step(int k) { return k * ES; }
  static constexpr unsigned out_step(int k) { return k * ES; }
  PFA_DEV unsigned in_elem(unsigned e) const { return (e / M) * rp + (e % M) * ES; }
  PFA_DEV unsigned out_elem(unsigned e) const { return (e / M) * rp + (e % M) * ES; }
  PFA_DEV cx<T> load(unsigned voff, unsigned soff) const { return buf_load<T, AUX>(rin, voff, soff); }
  PFA_DEV void store(cx<T> v, unsigned voff, unsigned soff) const { buf_store<T, AUX>(v, rout, voff, soff); }
};

/// The fused pair step on the image `lds` of this lane's row (see the head of the file).  wk: the w_k table; hp: the
/// M + 1 bins of the row's filter.  No barrier inside; the caller puts one behind it.  CHUNK: work items per lane and
/// trip of the rolled loop (the overlap-save kernel takes 2: with 4 its fp32 M = 8192 instantiation spilled two
/// twiddle registers).
template <typename Cfg, bool CORR, int CHUNK = 4>
PFA_DEV void rconv_pair_step(cx<typename Cfg::T>* lds, int tid, const cx<typename Cfg::T>* __restrict__ wk,
                             const cx<typename Cfg::T>* __restrict__ hp) {
  using T = typename Cfg::T;
  constexpr int M = Cfg::N;
  constexpr int KH = M / 2 + 1;                        // work items: k = 0 ... M/2
  constexpr int UPT = (KH + Cfg::TPF - 1) / Cfg::TPF;  // ... per lane
  constexpr int UCH = UPT < CHUNK ? UPT : CHUNK;       // ... per trip of the loop
#pragma nounroll
  for (int c = 0; c < UPT; c += UCH) {
    sfor<0, UCH>([&](auto i_) PFA_LAMBDA {
      const unsigned k = tid + (c + decltype(i_)::value) * Cfg::TPF;
      if (k < KH) {
        cx<T> hk = hp[k], hm = hp[M - k];
        if constexpr (CORR) {
          hk.im = -hk.im;
          hm.im = -hm.im;
        }
        const cx<T> a = lds[lds_pad<Cfg>(k)];
        if (k == 0) {
          const T y0 = (a.re + a.im) * hk.re, ym = (a.re - a.im) * hm.re;
          lds[lds_pad<Cfg>(0)] = cx<T>{y0 + ym, ym - y0};
        } else {
          const cx<T> b = lds[lds_pad<Cfg>(M - k)];
          const cx<T> w = wk[k];
          // R2C: X[k], X[M-k]
          const cx<T> s{a.re + b.re, a.im - b.im}, d{a.re - b.re, a.im + b.im};
          const cx<T> t = cmul(d, w);
          const cx<T> xk{T(0.5) * (s.re + t.im), T(0.5) * (s.im - t.re)};
          const cx<T> xm{T(0.5) * (s.re - t.im), -(T(0.5) * (s.im + t.re))};
          // the product
          const cx<T> yk = cmul(xk, hk), ym = cmul(xm, hm);
          // C2R: conj(Z'[k]) and conj(Z'[M-k]), what the conjugate-in backward passes read
          const cx<T> s2{yk.re + ym.re, yk.im - ym.im}, d2{yk.re - ym.re, yk.im + ym.im};
          const cx<T> q{w.re * d2.re + w.im * d2.im, w.re * d2.im - w.im * d2.re};  // conj(w) d2;  P = i q
          lds[lds_pad<Cfg>(k)] = cx<T>{s2.re - q.im, -(s2.im + q.re)};
          if (2 * k != M) lds[lds_pad<Cfg>(M - k)] = cx<T>{s2.re + q.im, s2.im - q.re};
        }
      }
    });
  }
}

/// `nfft` rows of N = 2 * Cfg::N real scalars (pitch `dist` scalars) -> as many rows of the same layout; `in` and `out`
/// may be the same buffer.  tw: the real plan's tables (M-point tables, then w_k).  filt: n_filters half spectra of
/// Cfg::N + 1 bins, packed; row t takes t mod n_filters.  CORR: the conjugate spectrum (correlation, the adjoint).  The
/// prologue (twiddles into registers / LDS), the persistent loop and the staged copies are stockham_wg_real_body's.
template <typename Cfg, bool CORR>
__global__ __launch_bounds__(Cfg::WG, Cfg::OCC) void stockham_wg_rconv_kernel(
    const void* in, void* out, const cx<typename Cfg::T>* __restrict__ tw, const cx<typename Cfg::T>* __restrict__ filt,
    long long nfft, unsigned n_filters, typename Cfg::T scale, unsigned dist) {
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
  if constexpr (Cfg::TWM == TW_REGS) {
    sfor<1, Cfg::NP>([&](auto p_) PFA_LAMBDA {
      constexpr int p = decltype(p_)::value;
      constexpr int R = Seq::r[p];
      constexpr int Ns = Seq::ns(p);
      sfor<0, Cfg::bpt(p)>([&](auto i_) PFA_LAMBDA {
        constexpr int i = decltype(i_)::value;
        const int q = (tid + i * Cfg::TPF) % Ns;
        sfor<1, R>([&](auto t_) PFA_LAMBDA {
          constexpr int t = decltype(t_)::value;
          twr[Cfg::twr_off(p) + i * (R - 1) + (t - 1)] = tw[Seq::tw_off(p) + (t - 1) * Ns + q];
        });
      });
    });
  }
  if constexpr (Cfg::TWL > 0) {
    cx<T>* twl = all + Cfg::FPW * Cfg::LDS_PER_FFT;
    for (int i = threadIdx.x; i < Cfg::TWL_ELEMS; i += Cfg::WG) twl[i] = tw[i];
    __syncthreads();
  }
  // filter of this lane's row: (g * FPW + f) mod n_filters, kept up to date by adding the loop's step mod n_filters
  const unsigned long long nf = n_filters;
  unsigned hrow = static_cast<unsigned>((static_cast<unsigned long long>(blockIdx.x) * Cfg::FPW + f) % nf);
  const unsigned hstep = static_cast<unsigned>((static_cast<unsigned long long>(gridDim.x) * Cfg::FPW) % nf);
  const long long ngroups = (nfft + Cfg::FPW - 1) / Cfg::FPW;
  for (long long g = blockIdx.x; g < ngroups; g += gridDim.x) {
    const rconv_io<T, M, Cfg::FPW, Cfg::AUX> io(in, out, g, nfft, dist);
    const cx<T>* twp = tw;
    if constexpr (Cfg::TWM == TW_GLOBAL) {
      asm volatile("" : "+s"(twp));  // (stockham_wg_body: keep the table reads inside the loop)
    }
    const cx<T>* wk = twp + Seq::tw_total;
    const cx<T>* hp = filt + static_cast<size_t>(hrow) * (M + 1);
    hrow = hrow >= n_filters - hstep ? hrow - (n_filters - hstep) : hrow + hstep;
    if constexpr (Cfg::STAGED) {
      sfor<0, EPT>([&](auto k_) PFA_LAMBDA {
        const unsigned e = threadIdx.x + decltype(k_)::value * Cfg::WG;
        if (CH % Cfg::WG == 0 || e < CH) {
          all[(e / M) * Cfg::LDS_PER_FFT + lds_pad<Cfg>(e % M)] = io.load(io.in_elem(e), 0);
        }
      });
      __syncthreads();
    }
    // 1. Z = DFT_M(z), natural order, unscaled, in the image (the last pass ends with a barrier)
    wg_passes<Cfg, false, 0, WG_LAST_TO_LDS>(io, f, lds, tid, twp, twr, scale);
    // 2. untangle, product, re-tangle: every lane rewrites the two slots it read
    rconv_pair_step<Cfg, CORR>(lds, tid, wk, hp);
    __syncthreads();
    // 3. scale * conj(DFT_M(image)).  (Every lane has read the image into registers before the last pass stores: the
    // next group's passes may write it.)
    wg_passes<Cfg, true, 0, WG_FIRST_FROM_LDS>(io, f, lds, tid, twp, twr, scale);
    if constexpr (Cfg::STAGED) {
      sfor<0, EPT>([&](auto k_) PFA_LAMBDA {
        const unsigned e = threadIdx.x + decltype(k_)::value * Cfg::WG;
        if (CH % Cfg::WG == 0 || e < CH) {
          const cx<T> y = all[(e / M) * Cfg::LDS_PER_FFT + lds_pad<Cfg>(e % M)];
          io.store(cx<T>{y.re * scale, -(y.im * scale)}, io.out_elem(e), 0);
        }
      });
      __syncthreads();
    }
  }
}

}  // namespace pfa
