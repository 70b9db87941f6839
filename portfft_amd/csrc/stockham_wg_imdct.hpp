// Inverse modified discrete cosine transform (windowed TDAC overlap-add synthesis) of REAL signals in ONE kernel: the
// type-4 transform of stockham_wg_dct4.hpp, run LDS to LDS, in front of an emission step that unfolds, windows and adds
// the two frames that cover a sample.  A row of the kernel is one (signal i, frame f) pair: the N = 2 * M coefficients of
// a frame are read once from the frame-major input (what the MDCT cell of stockham_wg_dct4.hpp writes) and every output
// sample leaves with one plain store.  No frame buffer, no atomics, no zeroed output.
//
// No counterpart in the reference; reached through pfft_execute_imdct on a plan of the REAL domain whose window was set
// (pfft_plan_set_imdct_window).
//
// For a coefficient row X let Y = dct4(X) unscaled, Y[k] = 2 sum_n X[n] cos(pi (2n + 1)(2k + 1) / (4N)), Y = [p, q] in
// halves of M.  The unfolded frame is g = [q, -rev q, -rev p, -p], 2N scalars: g[n] = 2 sum_k X[k] cos(pi (2n + 1 + N)
// (2k + 1) / (4N)), the transpose of the MDCT matrix.  With u = t + lead the position of output sample t on the frames'
// axis (frame f covers [f N, f N + 2N); the hop is N), block B = floor(u / N) and j = u - B N:
//   y[i][t] = scale * (prev + cur)
//   prev = w[N + j] * g[B - 1][N + j] = w[N + j] * -Y_{B-1}[M - 1 - j]   (j < M),   w[N + j] * -Y_{B-1}[j - M]      (j >= M)
//   cur  = w[j]     * g[B][j]         = w[j]     *  Y_B[M + j]           (j < M),   w[j]     * -Y_B[3M - 1 - j]     (j >= M)
// in ascending f; a frame that does not exist (B - 1 < 0, B >= n_frames) adds +0.  prev needs only the p half of the
// frame in front: the carry between two steps is M scalars.  EVERY sample is computed by that one expression wherever
// the work is cut: the result does not depend on chunk_frames or on the grid, bit for bit.
//
// Chunks with a recomputed halo (stockham_wg_istft.hpp with N -> 2N and hop -> N).  A group of the persistent loop owns
// (signal i, chunk c): the frames [c C, min(F, (c + 1) C)), C = chunk_frames, and the output samples [c C N - lead,
// (c + 1) C N - lead) cut to [0, out_length) -- the last chunk of a signal everything up to out_length, which includes
// the block behind the last frame (cur = +0).  It runs the frames max(0, c C - 1) ... end of chunk in ascending order,
// FPW per step: the halo is one frame, whose own block lies in front of the chunk and is dropped.
//
// Per step (t, a_n, b_k as in stockham_wg_dct4.hpp):
//   items in   the dct4 rows cell's: the aligned pairs j and M - 1 - j of the row's coefficients, times a_j, a_{M-1-j}, into
//              the slots lds_pad(j), lds_pad(M - 1 - j) of the row's image.  Barrier.
//   passes     forward, LDS to LDS (the last pass ends with a barrier)
//   items out  the same item turns T[k], T[M - 1 - k] into u[k] = T[k] b_k, u[M - 1 - k] IN ITS OWN SLOTS: slot k then holds
//              (Y[2k], -Y[N - 1 - 2k]) / 2.  No barrier between the read and the write: the item owns both slots.  Barrier.
//   emission   lane-strided entries e = l M + j, j < M, of the step's FPW_live blocks (the signal's last step: one block
//              more).  Positions j and N - 1 - j of a block take the same two values -- g is [q, -rev q | -rev p, -p] --, so
//              an entry reads yc = Y_B[M + j] / 2 from image l and yp = Y_{B-1}[M - 1 - j] / 2 from image l - 1 (block 0: from
//              the carry, or +0 in the first step of a run) once and stores both samples, 2 scale * (w[j'] yc' - w[N + j'] yp)
//              with yc' = yc at j' = j and -yc at j' = N - 1 - j: two scalar store streams, one ascending, one descending.
//              Several entries a trip, so that their LDS and window reads are in flight together.
//   carry      when the run has another step: barrier (the emission reads the old carry), then the halved p half of the
//              last image goes to the carry.  Barrier: the next step's items overwrite the images.
// The barrier in front of the carry is a departure from a carry written straight behind the emission: slot m of the
// carry is read by the entry j = M - 1 - m of block 0, which is not the lane that would overwrite it.  A run of one step
// (a short chunk of a wide group) does not pay it.
//
// The emit store is a scalar store; each scalar is predicated on its OWN index relative to the chunk's first owned
// sample: one add and one unsigned compare, never parity, never the range check of the buffer resource
// (stockham_wg_ols.hpp's rule).  A position in front of the chunk wraps to an index beyond every n_own (the host bounds
// one group's span).  Rows behind the last frame of a chunk are dead: they load nothing, still reach every barrier, and
// nothing reads their images.  The input resource starts at the first frame of the group's run and the output resource
// at the chunk's first owned sample, so only one group's span has to lie within 4 GiB.  Coefficient pairs are
// scalar-aligned only (frame_pitch may be odd).  `in` and `out` must not overlap.
//
// tab: the plan's dct4 table, a_0 ... a_{M-1} followed by b_0 ... b_{M-1}.  win: the 2N scalars of the synthesis window,
// read through L1 / L2 inside the loop.  LDS: what the real kernels of the configuration take, and the carry of M scalars
// behind it (imdct_lds_bytes).  Pitches, lead and out_length count SCALARS.
#pragma once
#include "stockham_wg_dct4.hpp"

namespace pfa {

/// LDS of the inverse MDCT kernel of configuration Cfg (an M-point wg_cfg): the real kernels', and the carry behind it
template <typename Cfg>
constexpr size_t imdct_lds_bytes() {
  return real_lds_bytes<Cfg>() + size_t(Cfg::N) * sizeof(typename Cfg::T);
}

/// Y[m] / 2 of the image `img` (scalars) whose slot k holds (Y[2k], -Y[N - 1 - 2k]) / 2, N = 2 * Cfg::N
template <typename Cfg>
PFA_DEV typename Cfg::T imdct_half(const typename Cfg::T* img, unsigned m) {
  constexpr unsigned N = 2u * Cfg::N;
  return (m & 1u) != 0 ? -img[2 * lds_pad<Cfg>((N - 1 - m) >> 1) + 1] : img[2 * lds_pad<Cfg>(m >> 1)];
}

/// n_frames frames of N = 2 * Cfg::N coefficients per signal (pitches frame_pitch / in_pitch, scalars) -> out_length real
/// scalars per signal (pitch out_pitch).  tw: the real plan's tables.  tab: a_0 ... a_{M-1}, b_0 ... b_{M-1}.  win: the
/// synthesis window, 2N scalars.  chunk: frames per chunk, 1 ... n_frames.  See the head of the file.
template <typename Cfg>
__global__ __launch_bounds__(Cfg::WG, Cfg::OCC) void stockham_wg_imdct_kernel(
    const void* in, void* out, const cx<typename Cfg::T>* __restrict__ tw, const void* __restrict__ tab,
    const void* __restrict__ win, unsigned n_signals, unsigned n_frames, typename Cfg::T scale, unsigned lead,
    unsigned out_length, unsigned frame_pitch, unsigned in_pitch, unsigned out_pitch, unsigned chunk) {
  using T = typename Cfg::T;
  constexpr int M = Cfg::N;
  constexpr unsigned N = 2u * M;
  constexpr unsigned SB = sizeof(T);
  constexpr unsigned IMG = 2u * Cfg::LDS_PER_FFT;      // scalars of an image
  constexpr int KH = (M + 1) / 2;                      // work items of a row: j = 0 ... ceil(M/2) - 1
  constexpr int UPT = (KH + Cfg::TPF - 1) / Cfg::TPF;  // ... per lane
  constexpr int IB = (UPT > 4 && M >= 128) ? 2 : UPT;  // ... per trip of the item loops (stockham_wg_dct4.hpp)
  // entries per lane and trip of the emission loop: two, whose LDS and window reads are in flight together; one where two
  // spill registers at the configuration's occupancy (fp32 M = 512; four spill on five fp32 lines: DESIGN 3.1n)
  constexpr int EU = (sizeof(T) == 4 && M == 512) ? 1 : 2;
  static_assert(Cfg::LDS_PER_FFT > 0, "LDS-resident configurations only");
  extern __shared__ __attribute__((aligned(16))) char pfa_smem[];
  const int f = threadIdx.x / Cfg::TPF;
  const int tid = threadIdx.x % Cfg::TPF;
  cx<T>* all = reinterpret_cast<cx<T>*>(pfa_smem);
  cx<T>* lds = all + f * Cfg::LDS_PER_FFT;
  const T* imgs = reinterpret_cast<const T*>(pfa_smem);
  T* carry = reinterpret_cast<T*>(pfa_smem + real_lds_bytes<Cfg>());

  cx<T> twr[Cfg::TWR_TOTAL];
  wg_twiddle_prologue<Cfg>(tw, tid, twr, all);
  const T s2 = T(2) * scale;
  const unsigned n_chunks = (n_frames + chunk - 1) / chunk;  // (the host keeps chunk within 1 ... n_frames)
  const unsigned ngroups = n_signals * n_chunks;             // (... and the row count below 2^31)
  for (unsigned g = blockIdx.x; g < ngroups; g += gridDim.x) {
    const cx<T>* twp = tw;
    const void* tabp = tab;
    const void* winp = win;
    if constexpr (Cfg::TWM == TW_GLOBAL) {
      asm volatile("" : "+s"(twp));  // (stockham_wg_body: keep the table reads inside the loop)
    }
    asm volatile("" : "+s"(tabp));  // (... and the a / b table's: it stays in L1 / L2, not in registers across the loop)
    asm volatile("" : "+s"(winp));  // (... and the window's)
    const cx<T>* ak = static_cast<const cx<T>*>(tabp);
    const cx<T>* bk = ak + M;
    const T* wp = static_cast<const T*>(winp);
    // the group's chunk (all uniform)
    const unsigned sig = g / n_chunks;
    const unsigned c = g - sig * n_chunks;
    const unsigned cf0 = c * chunk;
    const bool last_chunk = c == n_chunks - 1;
    const unsigned fe = last_chunk ? n_frames : cf0 + chunk;
    const unsigned fs = cf0 > 0 ? cf0 - 1 : 0u;
    long long lo = static_cast<long long>(cf0) * N - lead;
    if (lo < 0) lo = 0;
    long long hi = last_chunk ? static_cast<long long>(out_length) : static_cast<long long>(fe) * N - lead;
    if (hi > static_cast<long long>(out_length)) hi = out_length;
    if (hi < lo) hi = lo;
    const unsigned n_own = static_cast<unsigned>(hi - lo);  // (the host keeps one group's span within 4 GiB)
    const unsigned long long ifirst =
        static_cast<unsigned long long>(sig) * in_pitch + static_cast<unsigned long long>(fs) * frame_pitch;
    const unsigned long long ibytes = (static_cast<unsigned long long>(fe - fs - 1) * frame_pitch + N) * SB;
    const unsigned long long ofirst = static_cast<unsigned long long>(sig) * out_pitch + static_cast<unsigned long long>(lo);
    const __amdgpu_buffer_rsrc_t rin = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<char*>(static_cast<const char*>(in)) + ifirst * SB, 0,
        ibytes > 0xFFFFFFFFull ? 0xFFFFFFFFu : static_cast<unsigned>(ibytes), 0x00020000);
    const __amdgpu_buffer_rsrc_t rout =
        __builtin_amdgcn_make_buffer_rsrc(static_cast<char*>(out) + ofirst * SB, 0, n_own * SB, 0x00020000);
    for (unsigned f0 = fs; f0 < fe; f0 += Cfg::FPW) {
      const unsigned live = fe - f0 < unsigned(Cfg::FPW) ? fe - f0 : unsigned(Cfg::FPW);  // FPW_live
      const bool row_live = Cfg::FPW == 1 || static_cast<unsigned>(f) < live;
      // items in: the rows cell of stockham_wg_dct4.hpp on the lane's own frame
      if (row_live) {
        const unsigned row = (f0 - fs + (Cfg::FPW == 1 ? 0u : static_cast<unsigned>(f))) * frame_pitch;
#pragma unroll 1
        for (int i0 = 0; i0 < UPT; i0 += IB) {  // (one trip where the loop is not rolled: IB)
          sfor<0, IB>([&](auto i_) PFA_LAMBDA {
            const unsigned j = tid + (i0 + decltype(i_)::value) * Cfg::TPF;
            if (j < KH) {
              const cx<T> pa = buf_load<T, Cfg::AUX>(rin, (row + 2 * j) * SB, 0);
              const cx<T> pb = buf_load<T, Cfg::AUX>(rin, (row + 2 * (M - 1 - j)) * SB, 0);
              lds[lds_pad<Cfg>(j)] = cmul(cx<T>{pa.re, pb.im}, ak[j]);
              if (2 * j + 1 != M) lds[lds_pad<Cfg>(M - 1 - j)] = cmul(cx<T>{pb.re, pa.im}, ak[M - 1 - j]);
            }
          });
        }
      }
      __syncthreads();
      // T = DFT_M(t), natural order, unscaled, in the image (the last pass ends with a barrier)
      wg_passes<Cfg, false, 0, WG_FIRST_FROM_LDS | WG_LAST_TO_LDS>(dct4_no_io{}, f, lds, tid, twp, twr, scale);
      // items out, into their own slots: slot k becomes u[k] = (Y[2k], -Y[N - 1 - 2k]) / 2
      if (row_live) {
#pragma unroll 1
        for (int i0 = 0; i0 < UPT; i0 += IB) {
          sfor<0, IB>([&](auto i_) PFA_LAMBDA {
            const unsigned k = tid + (i0 + decltype(i_)::value) * Cfg::TPF;
            if (k < KH) {
              const cx<T> u = cmul(lds[lds_pad<Cfg>(k)], bk[k]);
              const cx<T> v = cmul(lds[lds_pad<Cfg>(M - 1 - k)], bk[M - 1 - k]);
              lds[lds_pad<Cfg>(k)] = u;
              if (2 * k + 1 != M) lds[lds_pad<Cfg>(M - 1 - k)] = v;
            }
          });
        }
      }
      __syncthreads();
      // emission
      const bool all_out = last_chunk && f0 + live == fe;  // the signal's last step: the block behind the last frame leaves too
      const unsigned ents = (all_out ? live + 1 : live) * M;
      const bool carried = f0 != fs;  // an earlier step of the run left the p half of its last frame
      // position d of this step is output sample rel0 + d of the chunk's own (wrapped when in front of them: beyond n_own)
      const unsigned rel0 = static_cast<unsigned>(static_cast<long long>(f0) * N - lead - lo);
      // Entry e = l M + j, j < M, stands for the positions j and N - 1 - j of block l (frame f0 + l): they take the same two
      // values, yc = Y_B[M + j] / 2 = -(-Y_B[3M - 1 - (N - 1 - j)]) / 2 and yp = Y_{B-1}[M - 1 - j] / 2, under four window
      // scalars.  EU entries a trip: their LDS and window reads go out together, then the stores.
#pragma unroll 1
      for (unsigned e0 = threadIdx.x; e0 < ents; e0 += EU * Cfg::WG) {
        T yp[EU], yc[EU], w0[EU], w1[EU], w2[EU], w3[EU];
        sfor<0, EU>([&](auto u_) PFA_LAMBDA {
          constexpr int u = decltype(u_)::value;
          const unsigned e = e0 + u * Cfg::WG;
          yp[u] = yc[u] = w0[u] = w1[u] = w2[u] = w3[u] = T(0);
          if (e < ents) {
            const unsigned l = e / unsigned(M), j = e - l * M;
            const unsigned r = rel0 + l * N;
            if (r + j < n_own || r + (N - 1 - j) < n_own) {
              if (l > 0 || carried) {  // the p half of the frame in front
                yp[u] = l > 0 ? imdct_half<Cfg>(imgs + (l - 1) * IMG, M - 1 - j) : carry[M - 1 - j];
                w2[u] = wp[N + j];
                w3[u] = wp[2 * N - 1 - j];
              }
              if (l < live) {
                yc[u] = imdct_half<Cfg>(imgs + l * IMG, M + j);
                w0[u] = wp[j];
                w1[u] = wp[N - 1 - j];
              }
            }
          }
        });
        sfor<0, EU>([&](auto u_) PFA_LAMBDA {
          constexpr int u = decltype(u_)::value;
          const unsigned e = e0 + u * Cfg::WG;
          if (e < ents) {
            const unsigned l = e / unsigned(M), j = e - l * M;
            const unsigned ra = rel0 + l * N + j, rb = rel0 + l * N + (N - 1 - j);
            // one expression for every sample: 2 scale (w[j'] yc' - w[N + j'] yp), yc' = -yc in the second half of a block
            if (ra < n_own) buf_store_scalar<T, Cfg::AUX>(s2 * (w0[u] * yc[u] - w2[u] * yp[u]), rout, ra * SB, 0);
            if (rb < n_own) buf_store_scalar<T, Cfg::AUX>(s2 * (w1[u] * -yc[u] - w3[u] * yp[u]), rout, rb * SB, 0);
          }
        });
      }
      if (f0 + Cfg::FPW < fe) {  // (uniform; live == FPW)
        __syncthreads();        // the emission read the old carry
        const T* last = imgs + (Cfg::FPW - 1) * IMG;
        for (unsigned m = threadIdx.x; m < unsigned(M); m += Cfg::WG) carry[m] = imdct_half<Cfg>(last, m);
      }
      __syncthreads();  // the next step's items overwrite the images
    }
  }
}

}  // namespace pfa
