// Discrete cosine transform of type 4 of packed REAL rows of even length N = 2 * M, and the modified discrete cosine
// transform (MDCT) of long REAL signals in frames of 2N samples at hop N, in ONE kernel each: an M-point complex
// transform between two twiddle multiplies, all in the LDS image.  There is no untangle step.  A row is read once
// (MDCT: every sample twice, by the two frames that cover it, the second time through L2) and written once.
//
// No counterpart in the reference; reached through pfft_execute_dct4 on a plan of the REAL domain after
// pfft_plan_prepare_dct4, and through pfft_execute_mdct after pfft_plan_set_mdct_window.
//
//   dct4:  y[k] = scale * 2 * sum_{n<N} x[n] cos(pi (2n + 1)(2k + 1) / (4N))                              k = 0 ... N - 1
//   mdct:  X[i,f,k] = scale * 2 * sum_{n<2N} w[n] xe_i[f N - lead + n] cos(pi (2n + 1 + N)(2k + 1) / (4N))   k = 0 ... N - 1
// xe_i is signal i extended by zeros outside [0, in_length).  The type-4 transform is its own inverse up to 2N.
//
// With a_n = exp(-i pi (4n + 1) / (4N)), b_k = exp(-i pi k / N), n, k = 0 ... M - 1:
//   t[n] = (x[2n] + i x[N - 1 - 2n]) a_n,   T = DFT_M(t),   u[k] = T[k] b_k,   y[2k] = 2 Re u[k],   y[N - 1 - 2k] = -2 Im u[k]
// (the post-twiddle is b_k, not a_k: with a_k every output is rotated by pi / (4N), which a round trip does not notice).
// The MDCT of a frame is the type-4 transform of the folded frame x': with v[n] = w[n] xe[f N - lead + n], n < 2N,
//   x'[m] = -v[3M - 1 - m] - v[3M + m]   (m < M),     x'[m] = v[m - M] - v[3M - 1 - m]   (M <= m < N).
//
// Per group of FPW rows; item j = 0 ... ceil(M / 2) - 1 of a row belongs to lane j mod TPF of the row's lanes:
//   items in   the aligned input pairs j and M - 1 - j, (x[2j], x[2j + 1]) and (x[N - 2 - 2j], x[N - 1 - 2j]), two streams that
//              are contiguous across lanes; they hold exactly t0[j] = x[2j] + i x[N - 1 - 2j] and t0[M - 1 - j] =
//              x[N - 2 - 2j] + i x[2j + 1]; times a_j, a_{M-1-j} in registers, into the complex slots lds_pad(j) and
//              lds_pad(M - 1 - j).  Odd M: the middle item is its own partner and writes one slot.  Barrier.
//   passes     forward, LDS to LDS: T in natural order in the image (the last pass ends with a barrier)
//   items out  the same item reads T[k], T[M - 1 - k], multiplies by b_k, b_{M-1-k} and stores output pair k,
//              (Re u[k], -Im u[M - 1 - k]) * 2 scale, and output pair M - 1 - k, (Re u[M - 1 - k], -Im u[k]) * 2 scale: aligned
//              pairs, no scalar store streams.  Barrier: the next group's items overwrite the images.
// Two barriers fewer than type 2 of stockham_wg_dct.hpp.  The items are the row's own lanes' (as the untangle items of
// the other real kernels), not spread over the whole group: an MDCT item needs its row's (signal, frame), a division by the
// run-time frame count, which a lane does once per group for its own row and would do per item for a foreign one; both
// streams of a row are coalesced either way.
//
// MDCT = true changes only the way in and where the stores go.  A row is a (signal i, frame f) pair, r = i * n_frames + f,
// FPW consecutive pairs a group (stockham_wg_stft.hpp).  Each of an item's two x' pairs comes from two frame pairs and two
// window pairs: x'[2j], x'[2j + 1] from (v[3M - 2 - 2j], v[3M - 1 - 2j]) and (v[3M + 2j], v[3M + 2j + 1]); x'[N - 2 - 2j],
// x'[N - 1 - 2j] from (v[M - 2 - 2j], v[M - 1 - 2j]) and (v[M + 2j], v[M + 2j + 1]).  The middle item of an odd M needs one
// scalar of each pair -- the other would lie outside the frame -- and loads those four as scalars.  The rules at the head
// of stockham_wg_stft.hpp hold: every frame scalar is predicated on its own index against [0, in_length) -- q = f N + n is
// the sample's index plus lead, valid when lead <= q < lead + in_length, two compares and no wrap-around; the range check
// of the resource is never relied on; the input resource starts `lead` scalars in front of the group's first signal, so
// the address of sample q of the d-th signal behind it is (d * in_pitch + q) scalars and no part of it is negative.  Pair
// accesses are scalar-aligned only (lead and M may be odd).  Coefficient pair k of row (i, f) goes to out + i * out_pitch +
// f * frame_pitch + 2k through a resource that starts at the group's first row; nothing else is written.  Rows behind the
// last one load nothing, reach every barrier, and their stores are dropped.
//
// tab: a_0 ... a_{M-1} followed by b_0 ... b_{M-1}, one device buffer of the plan, read through L1 / L2 inside the loop as
// w_k is.  win: the 2N scalars of the MDCT window (ones when none was given).  LDS: what the real kernels of the
// configuration take (real_lds_bytes) -- no row windows behind the images, a lane keeps its own row's in registers.
// Pitches, lead and in_length count SCALARS.
//
// Both cells take one argument list (kernels_impl.hpp, WF_DCT4).  MDCT = false reads n_signals as the row count and
// ignores n_frames, win, lead, in_length and frame_pitch.  In place (in == out, equal pitches) is safe for MDCT = false for
// the reason R2C is: every load of a group happens before its first barrier, every store behind its last, groups own
// disjoint rows; the missing rows of a ragged last group rest on wg_live_rows' range check, so the host keeps
// FPW * pitch * sizeof(T) below 2^32 on both sides (stockham_wg_dct.hpp).  The MDCT cannot run in place: frames overlap.
#pragma once
#include "stockham_wg_real.hpp"

namespace pfa {

/// LDS of the DCT-IV / MDCT kernels of configuration Cfg (an M-point wg_cfg): the real kernels'
template <typename Cfg>
constexpr size_t dct4_lds_bytes() {
  return real_lds_bytes<Cfg>();
}

/// what the LDS-to-LDS passes are given as io: they touch none of it
struct dct4_no_io {
  static PFA_DEV unsigned in_off(unsigned, unsigned j) { return j; }
  static PFA_DEV unsigned out_off(unsigned, unsigned j) { return j; }
  static constexpr unsigned in_step(int k) { return k; }
  static constexpr unsigned out_step(int k) { return k; }
};

/// One lane's row of an MDCT group: where its frame starts in the input resource and its coefficients in the output one.
template <typename T, int M, int FPW, int AUX>
struct mdct_row {
  static constexpr unsigned SB = sizeof(T);
  __amdgpu_buffer_rsrc_t rin, rout;
  const T* win;
  unsigned lead, end;  // a sample's index plus lead is valid in [lead, end), end = lead + in_length
  unsigned q0;         // ... of the frame's first sample: f * N
  unsigned ibase;      // scalar of the input resource the frame's first sample would be read from
  unsigned obase;      // scalar of the output resource coefficient 0 goes to
  bool live;

  PFA_DEV mdct_row(const void* in, void* out, const void* win_, unsigned g, unsigned f, unsigned n_signals,
                   unsigned n_frames, unsigned lead_, unsigned in_length, unsigned in_pitch, unsigned frame_pitch,
                   unsigned out_pitch)
      : win(static_cast<const T*>(win_)), lead(lead_), end(lead_ + in_length) {
    constexpr unsigned N = 2u * M;
    const unsigned r0 = g * FPW;  // (uniform; the group exists, so i0 < n_signals)
    const unsigned i0 = r0 / n_frames;
    const unsigned f0 = r0 - i0 * n_frames;
    const unsigned long long after = n_signals - 1 - i0;
    const unsigned long long ibytes = (after * in_pitch + in_length + lead) * SB;
    const unsigned long long ofirst =
        static_cast<unsigned long long>(i0) * out_pitch + static_cast<unsigned long long>(f0) * frame_pitch;
    const unsigned long long obytes =
        (after * out_pitch + static_cast<unsigned long long>(n_frames - 1 - f0) * frame_pitch + N) * SB;
    const long long ifirst = static_cast<long long>(i0) * in_pitch - lead;
    rin = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(static_cast<const char*>(in)) + ifirst * SB, 0,
                                            ibytes > 0xFFFFFFFFull ? 0xFFFFFFFFu : static_cast<unsigned>(ibytes), 0x00020000);
    rout = __builtin_amdgcn_make_buffer_rsrc(static_cast<char*>(out) + ofirst * SB, 0,
                                             obytes > 0xFFFFFFFFull ? 0xFFFFFFFFu : static_cast<unsigned>(obytes), 0x00020000);
    const unsigned r = r0 + (FPW == 1 ? 0u : f);  // (one row per group: the row is uniform, and kept in SGPRs)
    const unsigned sig = r / n_frames;
    const unsigned fr = r - sig * n_frames;
    const unsigned di = sig - i0;
    live = sig < n_signals;
    // (a row that does not exist gets the first row's place: nothing of it is dereferenced, and no product of it wraps)
    q0 = live ? fr * N : 0u;
    ibase = live ? di * in_pitch + q0 : 0u;
    // (the host keeps the rows of a group within 4 GiB: fr >= f0 when di == 0, and the sum fits otherwise)
    obase = live ? di * out_pitch + fr * frame_pitch - f0 * frame_pitch : 0u;
  }
  /// is frame scalar n of the row a sample of its signal?
  PFA_DEV bool inside(unsigned n) const {
    const unsigned q = q0 + n;
    return live && q >= lead && q < end;
  }
  /// v[n] = w[n] * xe[frame's first sample + n]
  PFA_DEV T scalar(unsigned n) const {
    T x = T(0);
    if (inside(n)) x = buf_load_scalar<T, AUX>(rin, (ibase + n) * SB, 0);
    return x * win[n];
  }
  /// (v[n], v[n + 1]), n + 1 < 2N; every scalar on its own predicate
  PFA_DEV cx<T> pair(unsigned n) const {
    cx<T> x{T(0), T(0)};
    const bool ok0 = inside(n), ok1 = inside(n + 1);
    if (ok0 && ok1) {
      x = buf_load<T, AUX>(rin, (ibase + n) * SB, 0);
    } else if (ok0) {  // the last scalar of the signal
      x.re = buf_load_scalar<T, AUX>(rin, (ibase + n) * SB, 0);
    } else if (ok1) {  // the first scalar of the signal
      x.im = buf_load_scalar<T, AUX>(rin, (ibase + n + 1) * SB, 0);
    }
    return cx<T>{x.re * win[n], x.im * win[n + 1]};
  }
  /// coefficient pair k of the row
  PFA_DEV void store(cx<T> v, unsigned k) const {
    if (live) buf_store<T, AUX>(v, rout, (obase + 2 * k) * SB, 0);
  }
};

/// MDCT = false: n_signals rows of N = 2 * Cfg::N real scalars (pitch in_pitch scalars) -> as many rows of N scalars (pitch
/// out_pitch).  MDCT = true: n_signals signals of in_length scalars (pitch in_pitch) -> n_frames frames of N coefficients
/// each (pitches frame_pitch / out_pitch, scalars); `in` and `out` must not overlap.  tw: the real plan's tables.  tab:
/// a_0 ... a_{M-1}, b_0 ... b_{M-1}.  win: the window, 2N scalars.  See the head of the file.
template <typename Cfg, bool MDCT>
__global__ __launch_bounds__(Cfg::WG, Cfg::OCC) void stockham_wg_dct4_kernel(
    const void* in, void* out, const cx<typename Cfg::T>* __restrict__ tw, const void* __restrict__ tab,
    const void* __restrict__ win, unsigned n_signals, unsigned n_frames, typename Cfg::T scale, unsigned lead,
    unsigned in_length, unsigned in_pitch, unsigned frame_pitch, unsigned out_pitch) {
  using T = typename Cfg::T;
  constexpr int M = Cfg::N;
  constexpr unsigned N = 2u * M;
  constexpr unsigned SB = sizeof(T);
  constexpr unsigned ES = sizeof(cx<T>);
  constexpr int KH = (M + 1) / 2;                      // work items of a row: j = 0 ... ceil(M/2) - 1
  constexpr int UPT = (KH + Cfg::TPF - 1) / Cfg::TPF;  // ... per lane
  // ... per trip of the item loops: rolled from M = 128 on, two items a trip, where stockham_wg_dct.hpp rolls its own (IB
  // there) and for its reason -- unrolled, the long lengths spill where the R2C twin does not.
  constexpr int IB = (UPT > 4 && M >= 128) ? 2 : UPT;
  static_assert(Cfg::LDS_PER_FFT > 0, "LDS-resident configurations only");
  extern __shared__ __attribute__((aligned(16))) char pfa_smem[];
  const int f = threadIdx.x / Cfg::TPF;
  const int tid = threadIdx.x % Cfg::TPF;
  cx<T>* all = reinterpret_cast<cx<T>*>(pfa_smem);
  cx<T>* lds = all + f * Cfg::LDS_PER_FFT;

  cx<T> twr[Cfg::TWR_TOTAL];
  wg_twiddle_prologue<Cfg>(tw, tid, twr, all);
  const unsigned ip = in_pitch * SB, op = out_pitch * SB;  // row pitches in bytes (MDCT = false)
  const T s2 = T(2) * scale;
  // (the host keeps the row count below 2^31)
  const unsigned n_rows = MDCT ? n_signals * n_frames : n_signals;
  const unsigned ngroups = (n_rows + Cfg::FPW - 1) / Cfg::FPW;
  for (unsigned g = blockIdx.x; g < ngroups; g += gridDim.x) {
    const cx<T>* twp = tw;
    const void* tabp = tab;
    const void* winp = win;
    if constexpr (Cfg::TWM == TW_GLOBAL) {
      asm volatile("" : "+s"(twp));  // (stockham_wg_body: keep the table reads inside the loop)
    }
    asm volatile("" : "+s"(tabp));  // (... and the a / b table's: it stays in L1 / L2, not in registers across the loop)
    const cx<T>* ak = static_cast<const cx<T>*>(tabp);
    const cx<T>* bk = ak + M;
    if constexpr (MDCT) {
      asm volatile("" : "+s"(winp));  // (... and the window's)
      const mdct_row<T, M, Cfg::FPW, Cfg::AUX> row(in, out, winp, g, f, n_signals, n_frames, lead, in_length, in_pitch,
                                                   frame_pitch, out_pitch);
#pragma unroll 1
      for (int i0 = 0; i0 < UPT; i0 += IB) {  // (one trip where the loop is not rolled: IB)
        sfor<0, IB>([&](auto i_) PFA_LAMBDA {
          const unsigned j = tid + (i0 + decltype(i_)::value) * Cfg::TPF;
          if (j < KH) {
            if ((M & 1) != 0 && 2 * j + 1 == M) {  // x'[M - 1] + i x'[M]
              const cx<T> t{-row.scalar(N) - row.scalar(2 * N - 1), row.scalar(0) - row.scalar(N - 1)};
              lds[lds_pad<Cfg>(j)] = cmul(t, ak[j]);
            } else {
              const cx<T> c1 = row.pair(3 * M - 2 - 2 * j), c2 = row.pair(3 * M + 2 * j);
              const cx<T> c3 = row.pair(M - 2 - 2 * j), c4 = row.pair(M + 2 * j);
              // x'[2j] + i x'[N - 1 - 2j]  and  x'[N - 2 - 2j] + i x'[2j + 1]
              const cx<T> ta{-c1.im - c2.re, c3.im - c4.re}, tb{c3.re - c4.im, -c1.re - c2.im};
              lds[lds_pad<Cfg>(j)] = cmul(ta, ak[j]);
              lds[lds_pad<Cfg>(M - 1 - j)] = cmul(tb, ak[M - 1 - j]);
            }
          }
        });
      }
      __syncthreads();
      // T = DFT_M(t), natural order, unscaled, in the image (the last pass ends with a barrier)
      wg_passes<Cfg, false, 0, WG_FIRST_FROM_LDS | WG_LAST_TO_LDS>(dct4_no_io{}, f, lds, tid, twp, twr, scale);
#pragma unroll 1
      for (int i0 = 0; i0 < UPT; i0 += IB) {
        sfor<0, IB>([&](auto i_) PFA_LAMBDA {
          const unsigned k = tid + (i0 + decltype(i_)::value) * Cfg::TPF;
          if (k < KH) {
            const cx<T> u = cmul(lds[lds_pad<Cfg>(k)], bk[k]);
            const cx<T> v = cmul(lds[lds_pad<Cfg>(M - 1 - k)], bk[M - 1 - k]);
            row.store(cx<T>{s2 * u.re, -(s2 * v.im)}, k);
            if (2 * k + 1 != M) row.store(cx<T>{s2 * v.re, -(s2 * u.im)}, M - 1 - k);
          }
        });
      }
    } else {
      __amdgpu_buffer_rsrc_t rin, rout;
      wg_live_rows<Cfg::FPW>(rin, rout, in, out, g, n_rows, ip, op);
      const unsigned irow = f * ip, orow = f * op;
#pragma unroll 1
      for (int i0 = 0; i0 < UPT; i0 += IB) {  // (one trip where the loop is not rolled: IB)
        sfor<0, IB>([&](auto i_) PFA_LAMBDA {
          const unsigned j = tid + (i0 + decltype(i_)::value) * Cfg::TPF;
          if (j < KH) {
            const cx<T> pa = buf_load<T, Cfg::AUX>(rin, irow + j * ES, 0);
            const cx<T> pb = buf_load<T, Cfg::AUX>(rin, irow + (M - 1 - j) * ES, 0);
            lds[lds_pad<Cfg>(j)] = cmul(cx<T>{pa.re, pb.im}, ak[j]);
            if (2 * j + 1 != M) lds[lds_pad<Cfg>(M - 1 - j)] = cmul(cx<T>{pb.re, pa.im}, ak[M - 1 - j]);
          }
        });
      }
      __syncthreads();
      // T = DFT_M(t), natural order, unscaled, in the image (the last pass ends with a barrier)
      wg_passes<Cfg, false, 0, WG_FIRST_FROM_LDS | WG_LAST_TO_LDS>(dct4_no_io{}, f, lds, tid, twp, twr, scale);
#pragma unroll 1
      for (int i0 = 0; i0 < UPT; i0 += IB) {
        sfor<0, IB>([&](auto i_) PFA_LAMBDA {
          const unsigned k = tid + (i0 + decltype(i_)::value) * Cfg::TPF;
          if (k < KH) {
            const cx<T> u = cmul(lds[lds_pad<Cfg>(k)], bk[k]);
            const cx<T> v = cmul(lds[lds_pad<Cfg>(M - 1 - k)], bk[M - 1 - k]);
            buf_store<T, Cfg::AUX>(cx<T>{s2 * u.re, -(s2 * v.im)}, rout, orow + k * ES, 0);
            if (2 * k + 1 != M) buf_store<T, Cfg::AUX>(cx<T>{s2 * v.re, -(s2 * u.im)}, rout, orow + (M - 1 - k) * ES, 0);
          }
        });
      }
    }
    __syncthreads();  // the next group's items overwrite the images
  }
}

}  // namespace pfa
