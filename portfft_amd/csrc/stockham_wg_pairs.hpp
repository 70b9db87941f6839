// Circular convolution or correlation of PAIRS of real rows of N = 2 * M scalars in ONE kernel: both operands are data of
// the call.  Row t of x and row t of y are read once, as scalars, zero-extended to N on the way in; both are transformed
// (two M-point forward pass sets into two LDS images), one pair step untangles both images, multiplies the two half
// spectra -- optionally normalised to unit magnitude, the phase transform of generalised cross-correlation (GCC-PHAT) --
// and re-tangles the product into the first image, and one M-point inverse pass set stores the first out_length scalars
// of the result row.  3 N scalars per row pair cross HBM; the spectra never reach memory.
//
// No counterpart in the reference; reached through pfft_execute_pairs on every plan of the REAL domain, after
// pfft_plan_prepare_pairs.
//
// With x~, y~ the rows extended by zeros to N, X = rfft(x~), Y = rfft(y~) (unscaled):
//   CORR = false   r[l] = scale * N * sum_n x~[n] y~[(l - n) mod N]       = scale * N * irfft(X Y)
//   CORR = true    r[l] = scale * N * sum_n x~[(n + l) mod N] y~[n]       = scale * N * irfft(X conj(Y))
// (irfft as NumPy's, which divides by N: the inverse passes are unnormalised, as in stockham_wg_rconv.hpp)
//   floor > 0      P = X conj(Y) (or X Y),  W[k] = P[k] / max(|P[k]|, floor),  r = scale * N * irfft(W)
// With x_length + y_length - 1 <= N nothing aliases: the convolution is scale * N * np.convolve(x, y) followed by zeros; the
// correlation holds the lags 0 ... x_length - 1 at r[0 ...] and the lags -1 ... -(y_length - 1) at r[N - 1] downwards.
// The sign convention is that of stockham_wg_rconv.hpp with CORR (filter(correlate=True)): y takes the place of the filter.
//
// The pair step, work item k = 0 ... floor(M/2), on the images ZA = DFT_M(x~ as pairs) and ZB = DFT_M(y~ as pairs), with
// w_k = exp(-2 pi i k / N) (the algebra of rconv_pair_step, twice on the way in):
//   A = ZA[k], B = conj(ZA[M-k]):   X[k] = ((A + B) - i w_k (A - B)) / 2,   X[M-k] = conj((A + B) + i w_k (A - B)) / 2
//   the same for Y from ZB;  CORR: Y <- conj(Y)
//   P[k] = X[k] Y[k],  P[M-k] = X[M-k] Y[M-k];   floor > 0: P <- P / max(|P|, floor)       (a uniform branch)
//   S = P[k] + conj(P[M-k]),  Q = i conj(w_k) (P[k] - conj(P[M-k])):   slot k <- conj(S + Q),   slot M-k <- S - Q
//   k = 0:  X[0] = Re ZA0 + Im ZA0, X[M] = Re ZA0 - Im ZA0, Y likewise, all real: P0 = X0 Y0, PM = XM YM, with a floor
//           P / max(|P|, floor) -- a sign, or a fraction below the floor;  slot 0 <- conj((P0 + PM) + i (P0 - PM))
//   2k = M: one slot
// Only image A is rewritten, and a lane rewrites exactly the two slots of it that it read: no barrier inside the step,
// one behind it.  The halves of R2C are kept (X and Y are the true bins), so that the floor compares with |X conj(Y)|.
//
// LDS (pairs_lds_bytes): the FPW images of y, then what the real kernels take -- the FPW images of x and the TWL copy
// behind them -- and, where Cfg::STAGED, the 2 FPW windows (ols_row) of the group's rows.  The passes find the TWL copy
// from their image pointer and row, `image + (FPW - f) * LDS_PER_FFT`: image f of y is image f - FPW of that numbering, so
// one copy serves both sets.  Twiddles: the real plan's table, the w_k behind the M-point tables.
//
// Loads and stores are window_io<..., REAL = true> of stockham_wg_ols.hpp with one segment per row (n_seg 1, lead 0, hop
// N): the explicit per-scalar predicate cuts a row at x_length / y_length / out_length, rows behind the last one have an
// empty window and still reach every barrier.  Two io objects, one per operand; the second one's output side is unused.
//
// x and y may be the same buffer (autocorrelation).  In place is NOT offered: the host refuses an output that overlaps
// either input.
#pragma once
#include "stockham_wg_ols.hpp"
#include "stockham_wg_real.hpp"

namespace pfa {

/// LDS of the pair kernels of configuration Cfg (an M-point wg_cfg): the real kernels', a second set of FPW images, and
/// the windows of both operands' rows behind them where the staged copies need them
template <typename Cfg>
constexpr size_t pairs_lds_bytes() {
  return real_lds_bytes<Cfg>() + size_t(Cfg::LDS_PER_FFT) * Cfg::FPW * sizeof(cx<typename Cfg::T>) +
         (Cfg::STAGED ? 2 * size_t(Cfg::FPW) * sizeof(ols_row) : 0);
}

/// the bins k and M - k of a real row from slots k (a) and M - k (b) of its image, w = w_k (stockham_wg_real.hpp, R2C)
template <typename T>
PFA_DEV void pairs_untangle(cx<T> a, cx<T> b, cx<T> w, cx<T>& xk, cx<T>& xm) {
  const cx<T> s{a.re + b.re, a.im - b.im}, d{a.re - b.re, a.im + b.im};
  const cx<T> t = cmul(d, w);
  xk = cx<T>{T(0.5) * (s.re + t.im), T(0.5) * (s.im - t.re)};
  xm = cx<T>{T(0.5) * (s.re - t.im), -(T(0.5) * (s.im + t.re))};
}

/// v * 2^e and the binary exponent of v, exactly, in the scalar type
PFA_DEV float pairs_ldexp(float v, int e) { return __builtin_ldexpf(v, e); }
PFA_DEV double pairs_ldexp(double v, int e) { return __builtin_ldexp(v, e); }
PFA_DEV int pairs_exponent(float v) {
  int e;
  (void)__builtin_frexpf(v, &e);
  return e;
}
PFA_DEV int pairs_exponent(double v) {
  int e;
  (void)__builtin_frexp(v, &e);
  return e;
}

/// p / max(|p|, floor), floor > 0: unit magnitude above the floor, p / floor below it (0 stays 0; a NaN stays one).  |p| is
/// formed on the components scaled by a power of two to order 1, so that their squares neither underflow nor overflow
/// wherever p itself is a finite number of the type: the branch is taken on |p|, not on a flushed or infinite square.
/// The quotients are divisions, not products with a reciprocal, which would be subnormal for |p| near the top of the range.
template <typename T>
PFA_DEV cx<T> pairs_phat(cx<T> p, T floor) {
  const T ar = __builtin_elementwise_abs(p.re), ai = __builtin_elementwise_abs(p.im);
  const int e = pairs_exponent(ar > ai ? ar : ai);
  const T sr = pairs_ldexp(p.re, -e), si = pairs_ldexp(p.im, -e);
  const T m = pairs_ldexp(__builtin_elementwise_sqrt(sr * sr + si * si), e);
  const T d = m > floor ? m : floor;
  return cx<T>{p.re / d, p.im / d};
}
template <typename T>
PFA_DEV T pairs_phat(T p, T floor) {
  const T m = __builtin_elementwise_abs(p);
  return p / (m > floor ? m : floor);
}

/// The fused pair step on the images `la` (x, rewritten) and `lb` (y, read) of this lane's row: see the head of the
/// file.  wk: the w_k table.  No barrier inside; the caller puts one behind it.  CHUNK: work items per lane and trip of
/// the rolled loop -- two operands' untangled bins are live at once, so 2 as in stockham_wg_rols.hpp.
template <typename Cfg, bool CORR, int CHUNK = 2>
PFA_DEV void pairs_pair_step(cx<typename Cfg::T>* la, const cx<typename Cfg::T>* lb, int tid,
                             const cx<typename Cfg::T>* __restrict__ wk, typename Cfg::T floor) {
  using T = typename Cfg::T;
  constexpr int M = Cfg::N;
  constexpr int KH = M / 2 + 1;                        // work items: k = 0 ... M/2
  constexpr int UPT = (KH + Cfg::TPF - 1) / Cfg::TPF;  // ... per lane
  constexpr int UCH = UPT < CHUNK ? UPT : CHUNK;       // ... per trip of the loop
  const bool phat = floor > T(0);
#pragma nounroll
  for (int c = 0; c < UPT; c += UCH) {
    sfor<0, UCH>([&](auto i_) PFA_LAMBDA {
      const unsigned k = tid + (c + decltype(i_)::value) * Cfg::TPF;
      if (k < KH) {
        const cx<T> a = la[lds_pad<Cfg>(k)], ya = lb[lds_pad<Cfg>(k)];
        if (k == 0) {
          T p0 = (a.re + a.im) * (ya.re + ya.im), pm = (a.re - a.im) * (ya.re - ya.im);
          if (phat) {
            p0 = pairs_phat(p0, floor);
            pm = pairs_phat(pm, floor);
          }
          la[lds_pad<Cfg>(0)] = cx<T>{p0 + pm, pm - p0};
        } else {
          const cx<T> b = la[lds_pad<Cfg>(M - k)], yb = lb[lds_pad<Cfg>(M - k)];
          const cx<T> w = wk[k];
          // R2C of both operands: X[k], X[M-k], Y[k], Y[M-k]
          cx<T> xk, xm, yk, ym;
          pairs_untangle(a, b, w, xk, xm);
          pairs_untangle(ya, yb, w, yk, ym);
          if constexpr (CORR) {
            yk.im = -yk.im;
            ym.im = -ym.im;
          }
          // the product, and its phase alone
          cx<T> pk = cmul(xk, yk), pm = cmul(xm, ym);
          if (phat) {
            pk = pairs_phat(pk, floor);
            pm = pairs_phat(pm, floor);
          }
          // C2R: conj(Z'[k]) and conj(Z'[M-k]), what the conjugate-in backward passes read
          const cx<T> s2{pk.re + pm.re, pk.im - pm.im}, d2{pk.re - pm.re, pk.im + pm.im};
          const cx<T> q{w.re * d2.re + w.im * d2.im, w.re * d2.im - w.im * d2.re};  // conj(w) d2;  Q = i q
          la[lds_pad<Cfg>(k)] = cx<T>{s2.re - q.im, -(s2.im + q.re)};
          if (2 * k != M) la[lds_pad<Cfg>(M - k)] = cx<T>{s2.re + q.im, s2.im - q.re};
        }
      }
    });
  }
}

/// `n_rows` rows of x (x_length scalars, pitch x_pitch) and of y (y_length, y_pitch) -> as many rows of out_length
/// scalars (pitch out_pitch); lengths at most N = 2 * Cfg::N, zero-extended on load; `out` must overlap neither input, x
/// and y may be the same.  tw: the real plan's tables (M-point tables, then w_k).  CORR: the conjugate spectrum of y.
/// floor: 0, or the floor of the phase transform.  wg_twiddle_prologue; the persistent loop and the staged copies are
/// stockham_wg_rols_kernel's, once per operand.
template <typename Cfg, bool CORR>
__global__ __launch_bounds__(Cfg::WG, Cfg::OCC) void stockham_wg_pairs_kernel(
    const void* x, const void* y, void* out, const cx<typename Cfg::T>* __restrict__ tw, unsigned n_rows,
    typename Cfg::T scale, typename Cfg::T floor, unsigned x_length, unsigned x_pitch, unsigned y_length, unsigned y_pitch,
    unsigned out_length, unsigned out_pitch) {
  using T = typename Cfg::T;
  using Seq = typename Cfg::Seq;
  constexpr int M = Cfg::N;
  static_assert(Cfg::LDS_PER_FFT > 0, "LDS-resident configurations only");
  constexpr int SET = Cfg::FPW * Cfg::LDS_PER_FFT;  // elements of one image set
  constexpr int CH = Cfg::FPW * M;                  // staged copies (STAGED configurations)
  constexpr int EPT = (CH + Cfg::WG - 1) / Cfg::WG;
  extern __shared__ __attribute__((aligned(16))) char pfa_smem[];
  const int f = threadIdx.x / Cfg::TPF;
  const int tid = threadIdx.x % Cfg::TPF;
  cx<T>* ally = reinterpret_cast<cx<T>*>(pfa_smem);  // the images of y ...
  cx<T>* all = ally + SET;                           // ... and, behind them, the real kernels' LDS: the images of x, TWL
  cx<T>* lds = all + f * Cfg::LDS_PER_FFT;
  cx<T>* ldsy = ally + f * Cfg::LDS_PER_FFT;
  // The row the passes are given for an image of y: image f - FPW counted from `all`, so that they find the TWL copy.
  // This leans on two things in other headers, which tests/test_pairs_host.py pins by their text so that a change there
  // is seen here: wg_pass (stockham_wg.hpp) takes `unsigned f` and uses it for nothing but `lds + (Cfg::FPW - f) *
  // Cfg::LDS_PER_FFT` (modulo 2^32: FPW - fy = 2 FPW - f) and the io's offsets, and slot_io (stockham_wg_ols.hpp) ignores
  // the row in in_off / out_off.  The TWL lines (M = 32 ... 128) run in test_gpu_pairs.py and test_gpu_pairs_registry.py.
  const unsigned fy = static_cast<unsigned>(f - Cfg::FPW);

  cx<T> twr[Cfg::TWR_TOTAL];
  wg_twiddle_prologue<Cfg>(tw, tid, twr, all);
  const unsigned ngroups = (n_rows + Cfg::FPW - 1) / Cfg::FPW;  // (the host keeps the row count below 2^31)
  for (unsigned g = blockIdx.x; g < ngroups; g += gridDim.x) {
    using io_t = window_io<T, M, Cfg::FPW, Cfg::AUX, true>;
    const io_t iox(x, out, g, f, n_rows, 1u, 0u, 2u * M, x_length, out_length, x_pitch, out_pitch);
    const io_t ioy(y, out, g, f, n_rows, 1u, 0u, 2u * M, y_length, out_length, y_pitch, out_pitch);
    const cx<T>* twp = tw;
    if constexpr (Cfg::TWM == TW_GLOBAL) {
      asm volatile("" : "+s"(twp));  // (stockham_wg_body: keep the table reads inside the loop)
    }
    const cx<T>* wk = twp + Seq::tw_total;
    if constexpr (Cfg::STAGED) {
      ols_row* rows = reinterpret_cast<ols_row*>(pfa_smem + real_lds_bytes<Cfg>() + size_t(SET) * sizeof(cx<T>));
      if (tid == 0) {
        rows[f] = iox.own;
        rows[Cfg::FPW + f] = ioy.own;
      }
      __syncthreads();
      sfor<0, EPT>([&](auto k_) PFA_LAMBDA {
        const unsigned e = threadIdx.x + decltype(k_)::value * Cfg::WG;
        if (CH % Cfg::WG == 0 || e < CH) {
          all[(e / M) * Cfg::LDS_PER_FFT + lds_pad<Cfg>(e % M)] = iox.load_in(rows[e / M], e % M);
          ally[(e / M) * Cfg::LDS_PER_FFT + lds_pad<Cfg>(e % M)] = ioy.load_in(rows[Cfg::FPW + e / M], e % M);
        }
      });
      __syncthreads();
    }
    // 1. ZA = DFT_M(x~ as pairs), ZB = DFT_M(y~ as pairs), natural order, unscaled, in the images (a last pass ends
    // with a barrier)
    wg_passes<Cfg, false, 0, WG_LAST_TO_LDS>(iox, f, lds, tid, twp, twr, scale);
    wg_passes<Cfg, false, 0, WG_LAST_TO_LDS>(ioy, fy, ldsy, tid, twp, twr, scale);
    // 2. untangle both, product, phase transform, re-tangle: every lane rewrites the two slots of image A it read
    pairs_pair_step<Cfg, CORR>(lds, ldsy, tid, wk, floor);
    __syncthreads();
    // 3. scale * conj(DFT_M(image A)); only the first out_length scalars of a row leave.  (Every lane has read image A
    // into registers before the last pass stores, and image B is not read behind the barrier: the next trip may write both.)
    wg_passes<Cfg, true, 0, WG_FIRST_FROM_LDS>(iox, f, lds, tid, twp, twr, scale);
    if constexpr (Cfg::STAGED) {
      const ols_row* rows = reinterpret_cast<const ols_row*>(pfa_smem + real_lds_bytes<Cfg>() + size_t(SET) * sizeof(cx<T>));
      sfor<0, EPT>([&](auto k_) PFA_LAMBDA {
        const unsigned e = threadIdx.x + decltype(k_)::value * Cfg::WG;
        if (CH % Cfg::WG == 0 || e < CH) {
          const cx<T> r = all[(e / M) * Cfg::LDS_PER_FFT + lds_pad<Cfg>(e % M)];
          iox.store_out(cx<T>{r.re * scale, -(r.im * scale)}, rows[e / M], e % M);
        }
      });
      __syncthreads();  // (the images and the windows are the next trip's to write)
    }
  }
}

}  // namespace pfa
