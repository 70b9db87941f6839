// Discrete cosine transforms of type 2 and type 3 of packed REAL rows of even length N = 2 * M in ONE kernel each: the
// M-point passes and the untangle step of stockham_wg_real.hpp with another way into and out of the LDS image (Makhoul's
// permutation in front, a quarter-wave twiddle step behind).  A row is read once (N scalars) and written once (N scalars).
//
// No counterpart in the reference; reached through pfft_execute_dct on a plan of the REAL domain after
// pfft_plan_prepare_dct.
//
//   type 2:  y[k] = scale * 2 * sum_n x[n] cos(pi k (2n + 1) / (2N))                 k = 0 ... N - 1
//   type 3:  y[n] = scale * (x[0] + 2 * sum_{k >= 1} x[k] cos(pi k (2n + 1) / (2N)))  n = 0 ... N - 1
//
// With v[n] = x[2n], v[N - 1 - n] = x[2n + 1] (n = 0 ... M - 1), V = rfft(v), c_k = exp(-i pi k / (2N)):
//   type 2   y[k] = 2 Re(c_k V[k]),  y[N - k] = -2 Im(c_k V[k])      (k = 0 ... M; y[0] = 2 V[0], y[M] = sqrt(2) V[M])
//   type 3   V'[k] = conj(c_k) (x[k] - i x[N - k]),  V'[0] = x[0],  V'[M] = sqrt(2) x[M];  v = N * irfft(V')
// and V comes from z[j] = v[2j] + i v[2j + 1], Z = DFT_M(z) by the untangle formulas at the head of stockham_wg_real.hpp
// (repeated below, not shared through a function template: DESIGN 3.1k).
//
// The image of a row holds N scalars: scalar slot s is .re (s even) or .im (s odd) of complex slot lds_pad(s / 2).
//
// Type 2, per group of FPW rows:
//   copy-in   the rows as M aligned pairs (x[2n], x[2n + 1]), coalesced over the whole group; x[2n] goes to scalar slot n,
//             x[2n + 1] to scalar slot N - 1 - n (both streams unit-stride across lanes); barrier
//   passes    forward, LDS to LDS: Z in natural order in the image
//   items     k = 0 ... M/2: A = Z[k], B = conj(Z[M - k]) -> V[k], V[M - k]; t = c_k V[k], t' = c_{M-k} V[M - k];
//             y[k] = 2 Re t, y[N - k] = -2 Im t, y[M - k] = 2 Re t', y[M + k] = -2 Im t': four scalar store streams, each
//             contiguous across lanes.  k = 0 writes y[0] and y[M] only, 2k = M writes y[M/2] and y[3M/2] only.
//   barrier   the next group's copy-in overwrites the images
// Type 3:
//   items     k = 0 ... M/2: x[k], x[N - k], x[M - k], x[M + k] as scalars straight from HBM -> V'[k], V'[M - k] -> the
//             untangle-in formulas of the C2R kernel, conj(Z') into the image; barrier
//   passes    backward (conjugate-in / conjugate-out), LDS to LDS: scalar slot s holds v[s] for even s, -v[s] for odd s
//   copy-out  output pair n = (v[n], v[N - 1 - n]) * scale, read as two scalars, stored as one aligned pair, coalesced
//             over the whole group; barrier
//
// LDS: what the real kernels of the configuration take (real_lds_bytes).  ctab: c_0 ... c_M, M + 1 complex values in a
// device buffer of the plan, read through L1 / L2 inside the loop as wk is.  Pitches count SCALARS.
//
// In place (in == out, equal pitches) is safe for the reason R2C is: every HBM load of a group happens before the first
// barrier of its passes, every store behind the last one, and groups own disjoint rows.  The resources cover the rows of
// the group that exist (wg_live_rows): a missing row of a ragged last group reads zeros and its stores are dropped.  That
// rests on the range check alone -- the slot of a missing row still computes its 32-bit offset f * pitch -- so the host
// keeps FPW * pitch * sizeof(T) below 2^32 on both sides whatever the row count is (plan_t::dct): no offset wraps.
#pragma once
#include "stockham_wg_real.hpp"

namespace pfa {

/// LDS of the DCT kernels of configuration Cfg (an M-point wg_cfg): the real kernels'
template <typename Cfg>
constexpr size_t dct_lds_bytes() {
  return real_lds_bytes<Cfg>();
}

/// what the LDS-to-LDS passes are given as io: they touch none of it
struct dct_no_io {
  static PFA_DEV unsigned in_off(unsigned, unsigned j) { return j; }
  static PFA_DEV unsigned out_off(unsigned, unsigned j) { return j; }
  static constexpr unsigned in_step(int k) { return k; }
  static constexpr unsigned out_step(int k) { return k; }
};

/// n_rows rows of N = 2 * Cfg::N real scalars (pitch in_pitch scalars) -> n_rows rows of N scalars (pitch out_pitch).
/// tw: the real plan's tables.  ctab: c_0 ... c_M.  INVERSE = false: type 2, true: type 3.  See the head of the file.
template <typename Cfg, bool INVERSE>
__global__ __launch_bounds__(Cfg::WG, Cfg::OCC) void stockham_wg_dct_kernel(
    const void* in, void* out, const cx<typename Cfg::T>* __restrict__ tw, const void* __restrict__ ctab, long long n_rows,
    typename Cfg::T scale, unsigned in_pitch, unsigned out_pitch) {
  using T = typename Cfg::T;
  using Seq = typename Cfg::Seq;
  constexpr int M = Cfg::N;
  constexpr unsigned N = 2u * M;
  constexpr unsigned SB = sizeof(T);
  constexpr unsigned ES = sizeof(cx<T>);
  constexpr int KH = M / 2 + 1;                        // work items of the untangle step: k = 0 ... M/2
  constexpr int UPT = (KH + Cfg::TPF - 1) / Cfg::TPF;  // ... per lane
  // ... per trip of the item loop.  From M = 128 on the loop is rolled, two items a trip: unrolled, fp32 M >= 1024 spilled
  // (M = 8192: 122 VGPRs) where the R2C / C2R twins do not, and every length lost occupancy; rolled, nothing spills and
  // N >= 512 runs 1-2x faster.  Below, the few items stay unrolled (N = 64, type 3: 1003 us against 1198 us rolled).
  constexpr int IB = (UPT > 4 && M >= 128) ? 2 : UPT;
  constexpr unsigned CH = unsigned(Cfg::FPW) * M;      // pairs of the group (copy-in, copy-out)
  constexpr int CB = sizeof(T) == 4 ? 8 : 4;           // pairs in flight per lane
  constexpr T SQRT2 = T(1.4142135623730951);
  static_assert(Cfg::LDS_PER_FFT > 0, "LDS-resident configurations only");
  extern __shared__ __attribute__((aligned(16))) char pfa_smem[];
  const int f = threadIdx.x / Cfg::TPF;
  const int tid = threadIdx.x % Cfg::TPF;
  cx<T>* all = reinterpret_cast<cx<T>*>(pfa_smem);
  cx<T>* lds = all + f * Cfg::LDS_PER_FFT;

  cx<T> twr[Cfg::TWR_TOTAL];
  wg_twiddle_prologue<Cfg>(tw, tid, twr, all);
  const unsigned ip = in_pitch * SB, op = out_pitch * SB;  // row pitches in bytes
  const long long ngroups = (n_rows + Cfg::FPW - 1) / Cfg::FPW;
  for (long long g = blockIdx.x; g < ngroups; g += gridDim.x) {
    __amdgpu_buffer_rsrc_t rin, rout;
    wg_live_rows<Cfg::FPW>(rin, rout, in, out, g, n_rows, ip, op);
    const cx<T>* twp = tw;
    const void* ctp = ctab;
    if constexpr (Cfg::TWM == TW_GLOBAL) {
      asm volatile("" : "+s"(twp));  // (stockham_wg_body: keep the table reads inside the loop)
    }
    asm volatile("" : "+s"(ctp));  // (... and the quarter-wave table's: it stays in L1 / L2, not in registers across the loop)
    const cx<T>* wk = twp + Seq::tw_total;
    const cx<T>* ck = static_cast<const cx<T>*>(ctp);
    if constexpr (!INVERSE) {
      // copy-in: pair n of row r -> scalar slots n and N - 1 - n of the row's image
#pragma unroll 1
      for (unsigned e0 = threadIdx.x; e0 < CH; e0 += CB * Cfg::WG) {  // (rolled: its addresses stay out of the registers)
        cx<T> p[CB];
        sfor<0, CB>([&](auto u_) PFA_LAMBDA {
          const unsigned e = e0 + decltype(u_)::value * Cfg::WG;
          if (e < CH) {
            const unsigned r = Cfg::FPW == 1 ? 0u : e / M, n = Cfg::FPW == 1 ? e : e % M;
            p[decltype(u_)::value] = buf_load<T, Cfg::AUX>(rin, r * ip + n * ES, 0);
          }
        });
        sfor<0, CB>([&](auto u_) PFA_LAMBDA {
          const unsigned e = e0 + decltype(u_)::value * Cfg::WG;
          if (e < CH) {
            const unsigned r = Cfg::FPW == 1 ? 0u : e / M, n = Cfg::FPW == 1 ? e : e % M;
            T* img = reinterpret_cast<T*>(all + r * Cfg::LDS_PER_FFT);
            const unsigned hi = N - 1 - n;
            img[2 * lds_pad<Cfg>(n >> 1) + (n & 1)] = p[decltype(u_)::value].re;
            img[2 * lds_pad<Cfg>(hi >> 1) + (hi & 1)] = p[decltype(u_)::value].im;
          }
        });
      }
      __syncthreads();
      // Z = DFT_M(z), natural order, unscaled, in the image (the last pass ends with a barrier)
      wg_passes<Cfg, false, 0, WG_FIRST_FROM_LDS | WG_LAST_TO_LDS>(dct_no_io{}, f, lds, tid, twp, twr, scale);
      const unsigned row = f * op;
      const T h = scale;  // 2 * (scale / 2): the untangle step's half and the transform's 2
#pragma unroll 1
      for (int i0 = 0; i0 < UPT; i0 += IB) {  // (one trip where the loop is not rolled: IB)
        sfor<0, IB>([&](auto i_) PFA_LAMBDA {
          const unsigned k = tid + (i0 + decltype(i_)::value) * Cfg::TPF;
          if (k < KH) {
            const cx<T> a = lds[lds_pad<Cfg>(k)];
            if (k == 0) {
              buf_store_scalar<T, Cfg::AUX>(T(2) * scale * (a.re + a.im), rout, row, 0);
              buf_store_scalar<T, Cfg::AUX>(SQRT2 * scale * (a.re - a.im), rout, row + M * SB, 0);
            } else {
              const cx<T> b = lds[lds_pad<Cfg>(M - k)];
              const cx<T> s{a.re + b.re, a.im - b.im}, d{a.re - b.re, a.im + b.im};
              const cx<T> t = cmul(d, wk[k]);
              const cx<T> vk{s.re + t.im, s.im - t.re};      // 2 V[k]
              const cx<T> vm{s.re - t.im, -(s.im + t.re)};   // 2 V[M - k]
              const cx<T> u = cmul(vk, ck[k]);
              buf_store_scalar<T, Cfg::AUX>(h * u.re, rout, row + k * SB, 0);
              buf_store_scalar<T, Cfg::AUX>(-(h * u.im), rout, row + (N - k) * SB, 0);
              if (2 * k != M) {
                const cx<T> u2 = cmul(vm, ck[M - k]);
                buf_store_scalar<T, Cfg::AUX>(h * u2.re, rout, row + (M - k) * SB, 0);
                buf_store_scalar<T, Cfg::AUX>(-(h * u2.im), rout, row + (M + k) * SB, 0);
              }
            }
          }
        });
      }
      __syncthreads();  // the next group's copy-in overwrites the images
    } else {
      const unsigned row = f * ip;
#pragma unroll 1
      for (int i0 = 0; i0 < UPT; i0 += IB) {  // (one trip where the loop is not rolled: IB)
        sfor<0, IB>([&](auto i_) PFA_LAMBDA {
          const unsigned k = tid + (i0 + decltype(i_)::value) * Cfg::TPF;
          if (k < KH) {
            cx<T> x, y;
            if (k == 0) {
              x = cx<T>{buf_load_scalar<T, Cfg::AUX>(rin, row, 0), T(0)};                      // V'[0]
              y = cx<T>{SQRT2 * buf_load_scalar<T, Cfg::AUX>(rin, row + M * SB, 0), T(0)};     // V'[M]
            } else {
              const T x0 = buf_load_scalar<T, Cfg::AUX>(rin, row + k * SB, 0);
              const T x1 = buf_load_scalar<T, Cfg::AUX>(rin, row + (N - k) * SB, 0);
              const T x2 = buf_load_scalar<T, Cfg::AUX>(rin, row + (M - k) * SB, 0);
              const T x3 = buf_load_scalar<T, Cfg::AUX>(rin, row + (M + k) * SB, 0);
              const cx<T> c0 = ck[k], c1 = ck[M - k];
              // conj(c) (p - i q)
              x = cx<T>{c0.re * x0 - c0.im * x1, -(c0.re * x1) - c0.im * x0};
              y = cx<T>{c1.re * x2 - c1.im * x3, -(c1.re * x3) - c1.im * x2};
            }
            const cx<T> s{x.re + y.re, x.im - y.im}, d{x.re - y.re, x.im + y.im};
            const cx<T> w = wk[k];
            const cx<T> q{w.re * d.re + w.im * d.im, w.re * d.im - w.im * d.re};  // conj(w) d;  P = i q
            // conj(Z'[k]) and conj(Z'[M-k]): what the conjugate-in backward passes read
            lds[lds_pad<Cfg>(k)] = cx<T>{s.re - q.im, -(s.im + q.re)};
            if (k != 0 && 2 * k != M) lds[lds_pad<Cfg>(M - k)] = cx<T>{s.re + q.im, s.im - q.re};
          }
        });
      }
      __syncthreads();
      // conj(z') of every row, unscaled, in its image (the last pass ends with a barrier)
      wg_passes<Cfg, true, 0, WG_FIRST_FROM_LDS | WG_LAST_TO_LDS>(dct_no_io{}, f, lds, tid, twp, twr, scale);
      // copy-out: output pair n of row r = (v[n], v[N - 1 - n]); an odd scalar slot holds -v
#pragma unroll 1
      for (unsigned e0 = threadIdx.x; e0 < CH; e0 += CB * Cfg::WG) {  // (rolled, as the copy-in)
        sfor<0, CB>([&](auto u_) PFA_LAMBDA {
          const unsigned e = e0 + decltype(u_)::value * Cfg::WG;
          if (e < CH) {
            const unsigned r = Cfg::FPW == 1 ? 0u : e / M, n = Cfg::FPW == 1 ? e : e % M;
            const T* img = reinterpret_cast<const T*>(all + r * Cfg::LDS_PER_FFT);
            const unsigned hi = N - 1 - n;
            const T lo_v = img[2 * lds_pad<Cfg>(n >> 1) + (n & 1)];
            const T hi_v = img[2 * lds_pad<Cfg>(hi >> 1) + (hi & 1)];
            // n and N - 1 - n have opposite parity: exactly one of the two carries the sign
            const T sl = (n & 1) ? -scale : scale;
            buf_store<T, Cfg::AUX>(cx<T>{lo_v * sl, -(hi_v * sl)}, rout, r * op + n * ES, 0);
          }
        });
      }
      __syncthreads();  // the next group's items overwrite the images
    }
  }
}

}  // namespace pfa
