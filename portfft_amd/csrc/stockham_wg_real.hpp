// Real-to-complex and complex-to-real 1-D transforms of even length N = 2 * M in ONE kernel: the M-point passes of
// stockham_wg.hpp on the row read as M complex numbers, and an "untangle" step over the pairs (k, M - k) that runs on
// the LDS image -- the input is read once (N reals) and the output written once (M + 1 complex), or the reverse.
//
// No counterpart in the reference (its descriptor refuses the REAL domain); reached through PFFT_EXT_REAL_TRANSFORMS.
//
// With z[j] = x[2j] + i x[2j+1], Z = DFT_M(z), w_k = exp(-2 pi i k / N), A = Z[k], B = conj(Z[M-k]) (Z[M] = Z[0]):
//   R2C  X[k]   = ((A + B) - i w_k (A - B)) / 2        X[M-k] = conj((A + B) + i w_k (A - B)) / 2      k = 0 ... M/2
//        k = 0:  X[0] = Re Z0 + Im Z0,  X[M] = Re Z0 - Im Z0 (both exactly real);  2k = M: one value, one store
//   C2R  S = X[k] + conj(X[M-k]),  P = i conj(w_k) (X[k] - conj(X[M-k])):   Z'[k] = S + P,   Z'[M-k] = conj(S - P)
//        (the imaginary parts of X[0] and X[M] are dropped), then the unnormalised inverse M-point transform of Z'
//        gives z' with x[2j] = Re z'[j], x[2j+1] = Im z'[j]: N * irfft(X).
// The backward passes are the conjugate-in / conjugate-out form of the forward ones: C2R writes conj(Z') into the image
// (no conjugating pass over the data) and the last pass conjugates on its way to HBM as it always does.
//
// LDS: the images (and the TWL copy) of the complex kernel of M points; a single-pass configuration, which needs no
// image for the complex transform, gets one here (real_lds_bytes).  Twiddles: the plan's table carries the
// floor(M/2) + 1 values w_k behind the M-point tables (offset radix_list::tw_total), read through L1 / L2.
//
// In place (the padded-row convention: row t holds N scalars in M + 1 complex slots) is safe by construction: every
// HBM load of a group happens before the first barrier of its passes and every store behind the last one, and groups
// own disjoint rows.  After a backward transform the two pad scalars of a row are not written.
#pragma once
#include "stockham_wg.hpp"

namespace pfa {

/// LDS of the real kernels of configuration Cfg (an M-point wg_cfg)
template <typename Cfg>
constexpr size_t real_lds_bytes() {
  return size_t(Cfg::LDS_PER_FFT * Cfg::FPW + Cfg::TWL_ELEMS) * sizeof(cx<typename Cfg::T>);
}

/// Addressing of one group's rows: the real side has a pitch of `rdist` SCALARS and is accessed as M complex elements
/// per row (what the passes load or store), the complex side a pitch of `cdist` complex elements (what the untangle
/// step loads or stores).  The resources cover the rows of the group that exist: missing rows read zeros, their stores
/// are dropped by the range check (packed_io).
template <typename T, int M, int FPW, int AUX, bool C2R>
struct real_io {
  static constexpr unsigned ES = sizeof(cx<T>);
  __amdgpu_buffer_rsrc_t rin, rout;
  unsigned rp, cp;  // row pitches in bytes: real side, complex side
  PFA_DEV real_io(const void* in, void* out, long long g, long long nfft, unsigned rdist, unsigned cdist)
      : rp(rdist * static_cast<unsigned>(sizeof(T))), cp(cdist * ES) {
    wg_live_rows<FPW>(rin, rout, in, out, g, nfft, C2R ? cp : rp, C2R ? rp : cp);
  }
  // the passes' side: element j of the M complex elements of row f
  PFA_DEV unsigned in_off(unsigned f, unsigned j) const { return f * rp + j * ES; }
  PFA_DEV unsigned out_off(unsigned f, unsigned j) const { return f * rp + j * ES; }
  static constexpr unsigned in_step(int k) { return k * ES; }
  static constexpr unsigned out_step(int k) { return k * ES; }
  PFA_DEV unsigned in_elem(unsigned e) const { return (e / M) * rp + (e % M) * ES; }
  PFA_DEV unsigned out_elem(unsigned e) const { return (e / M) * rp + (e % M) * ES; }
  PFA_DEV cx<T> load(unsigned voff, unsigned soff) const { return buf_load<T, AUX>(rin, voff, soff); }
  PFA_DEV void store(cx<T> v, unsigned voff, unsigned soff) const { buf_store<T, AUX>(v, rout, voff, soff); }
  // the untangle step's side: bin k of row f
  PFA_DEV cx<T> bin_load(unsigned f, unsigned k) const { return buf_load<T, AUX>(rin, f * cp + k * ES, 0); }
  PFA_DEV void bin_store(cx<T> v, unsigned f, unsigned k) const { buf_store<T, AUX>(v, rout, f * cp + k * ES, 0); }
};

/// Body of both kernels: wg_twiddle_prologue and the persistent loop of stockham_wg_body.
template <typename Cfg, bool C2R>
PFA_DEV void stockham_wg_real_body(const void* in, void* out, const cx<typename Cfg::T>* __restrict__ tw,
                                   long long nfft, typename Cfg::T scale, unsigned rdist, unsigned cdist) {
  using T = typename Cfg::T;
  using Seq = typename Cfg::Seq;
  constexpr int M = Cfg::N;
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
  const long long ngroups = (nfft + Cfg::FPW - 1) / Cfg::FPW;
  for (long long g = blockIdx.x; g < ngroups; g += gridDim.x) {
    const real_io<T, M, Cfg::FPW, Cfg::AUX, C2R> io(in, out, g, nfft, rdist, cdist);
    const cx<T>* twp = tw;
    if constexpr (Cfg::TWM == TW_GLOBAL) {
      asm volatile("" : "+s"(twp));  // (stockham_wg_body: keep the table reads inside the loop)
    }
    const cx<T>* wk = twp + Seq::tw_total;
    if constexpr (!C2R) {
      if constexpr (Cfg::STAGED) {
        sfor<0, EPT>([&](auto k_) PFA_LAMBDA {
          const unsigned e = threadIdx.x + decltype(k_)::value * Cfg::WG;
          if (CH % Cfg::WG == 0 || e < CH) {
            all[(e / M) * Cfg::LDS_PER_FFT + lds_pad<Cfg>(e % M)] = io.load(io.in_elem(e), 0);
          }
        });
        __syncthreads();
      }
      // Z = DFT_M(z), natural order, unscaled, in the image (the last pass ends with a barrier)
      wg_passes<Cfg, false, 0, WG_LAST_TO_LDS>(io, f, lds, tid, twp, twr, scale);
      const T h = scale * T(0.5);
      sfor<0, UPT>([&](auto i_) PFA_LAMBDA {
        const unsigned k = tid + decltype(i_)::value * Cfg::TPF;
        if (KH % Cfg::TPF == 0 || k < KH) {
          const cx<T> a = lds[lds_pad<Cfg>(k)];
          if (k == 0) {
            io.bin_store(cx<T>{scale * (a.re + a.im), T(0)}, f, 0);
            io.bin_store(cx<T>{scale * (a.re - a.im), T(0)}, f, M);
          } else {
            const cx<T> b = lds[lds_pad<Cfg>(M - k)];
            const cx<T> s{a.re + b.re, a.im - b.im}, d{a.re - b.re, a.im + b.im};
            const cx<T> t = cmul(d, wk[k]);
            io.bin_store(cx<T>{h * (s.re + t.im), h * (s.im - t.re)}, f, k);
            if (2 * k != M) io.bin_store(cx<T>{h * (s.re - t.im), -(h * (s.im + t.re))}, f, M - k);
          }
        }
      });
      __syncthreads();  // the next group's passes overwrite the images
    } else {
      sfor<0, UPT>([&](auto i_) PFA_LAMBDA {
        const unsigned k = tid + decltype(i_)::value * Cfg::TPF;
        if (KH % Cfg::TPF == 0 || k < KH) {
          cx<T> x = io.bin_load(f, k), y = io.bin_load(f, M - k);
          if (k == 0) x.im = y.im = T(0);
          const cx<T> s{x.re + y.re, x.im - y.im}, d{x.re - y.re, x.im + y.im};
          const cx<T> w = wk[k];
          const cx<T> q{w.re * d.re + w.im * d.im, w.re * d.im - w.im * d.re};  // conj(w) d;  P = i q
          // conj(Z'[k]) and conj(Z'[M-k]): what the conjugate-in backward passes read
          lds[lds_pad<Cfg>(k)] = cx<T>{s.re - q.im, -(s.im + q.re)};
          if (k != 0 && 2 * k != M) lds[lds_pad<Cfg>(M - k)] = cx<T>{s.re + q.im, s.im - q.re};
        }
      });
      __syncthreads();
      // (every lane has read the image into registers before the last pass stores: the next group's untangle step may
      //  write it)
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
}

/// N = 2 * Cfg::N real scalars per row (pitch fdist scalars) -> Cfg::N + 1 complex bins (pitch bdist complex elements).
/// `in` and `out` may be the same buffer (fdist == 2 * bdist).  Same argument list for both kernels.
template <typename Cfg>
__global__ __launch_bounds__(Cfg::WG, Cfg::OCC) void stockham_wg_r2c_kernel(const void* in, void* out,
                                                                            const cx<typename Cfg::T>* __restrict__ tw,
                                                                            long long nfft, typename Cfg::T scale,
                                                                            unsigned fdist, unsigned bdist) {
  stockham_wg_real_body<Cfg, false>(in, out, tw, nfft, scale, fdist, bdist);
}

/// Cfg::N + 1 complex bins per row (pitch bdist) -> 2 * Cfg::N real scalars (pitch fdist), unnormalised
template <typename Cfg>
__global__ __launch_bounds__(Cfg::WG, Cfg::OCC) void stockham_wg_c2r_kernel(const void* in, void* out,
                                                                            const cx<typename Cfg::T>* __restrict__ tw,
                                                                            long long nfft, typename Cfg::T scale,
                                                                            unsigned fdist, unsigned bdist) {
  stockham_wg_real_body<Cfg, true>(in, out, tw, nfft, scale, fdist, bdist);
}

}  // namespace pfa
