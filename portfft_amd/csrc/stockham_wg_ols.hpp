// Overlap-save FIR filtering of long signals in ONE kernel: linear convolution (or correlation) of signals of any length
// with filters of K <= N taps, on the pass structure of stockham_wg_conv.hpp.  A row of the kernel is one (signal i,
// segment s) pair: a window of N input samples is transformed, multiplied with the filter spectrum and transformed back,
// and only the hop = N - K + 1 outputs that circular aliasing did not touch are stored, at their place in the output
// signal.  Nothing is gathered or copied around the kernel: per sample a signal is read N / hop times and written once.
//
// No counterpart in the reference; reached through pfft_execute_filter on a plan with PFFT_EXT_CONVOLUTION whose
// filter was given as taps (pfft_plan_set_filter_taps: zero-padded to N and transformed by the plan).
//
// Geometry (all kernel arguments: one code object per configuration serves every K and both modes' addressing):
//   rows      r = i * n_seg + s,  i < n_signals,  s < n_seg = ceil(out_length / hop);  FPW consecutive rows per group
//   window    image slot j of row (i, s) holds x_i[e0 + j], e0 = s * hop - lead, zero outside [0, in_length)
//             lead = K - 1 for convolution (the window reaches back over the filter's history), 0 for correlation
//   stores    result slot lead + m goes to y_i[s * hop + m] for m < min(hop, out_length - s * hop); nothing else
//   filter    row (i, s) takes spectrum i mod n_filters; CORR conjugates it, as in stockham_wg_conv_kernel
//
// The window is a row's, not a lane's: every access is predicated on it explicitly -- one add and one unsigned compare
// -- and never on 32-bit wrap-around of an offset (no part of an address is ever negative: ols_row) or on the range
// check of the buffer resource, which stays what it is everywhere else: a backstop that ends at the last signal.  The
// passes address the lane's own row, so they use the window the lane computed (one division per group trip, which also
// gives the filter's row).  The STAGED copies address element e -> (row e / N, slot e % N), which is some other lane's
// row: those configurations keep the FPW windows in LDS behind the images (ols_lds_bytes), written once per group trip
// in front of a barrier.
//
// Rows beyond the last signal have an empty window: they load nothing, compute on zeros and store nothing -- every lane
// of the group reaches every barrier.
//
// In place is NOT safe: segment s + 1 reads the K - 1 samples that the group of segment s overwrites.  The host refuses
// overlapping buffers.
#pragma once
#include "stockham_wg_conv.hpp"

namespace pfa {

/// the window of one row, in complex elements.  `e0` of a row whose window starts in front of its signal is the wrapped
/// negative number and only ever compared; the two bases are offsets into the group's resources, which start `lead`
/// elements in front of a signal so that no part of an address is negative: the passes split an offset into a lane
/// part (base + slot) and a compile-time part, and the hardware adds the two without wrap-around.
struct ols_row {
  unsigned e0;      // input sample of image slot 0, relative to the row's signal; an empty window: 0xC0000000
  unsigned ibase;   // element of the input resource that image slot 0 reads
  unsigned obase;   // element of the output resource that result slot 0 would go to
  unsigned nvalid;  // result slots [lead, lead + nvalid) are stored
};

/// LDS of the overlap-save kernels of configuration Cfg: the convolution kernel's, and the windows of the group's rows
/// behind it where the staged copies need them
template <typename Cfg>
constexpr size_t ols_lds_bytes() {
  return conv_lds_bytes<Cfg>() + (Cfg::STAGED ? size_t(Cfg::FPW) * sizeof(ols_row) : 0);
}

/// what the passes see of an io that addresses the lane's own row by image slot: the slot and a compile-time step in slots
struct slot_io {
  static PFA_DEV unsigned in_off(unsigned, unsigned j) { return j; }
  static PFA_DEV unsigned out_off(unsigned, unsigned j) { return j; }
  static constexpr unsigned in_step(int k) { return k; }
  static constexpr unsigned out_step(int k) { return k; }
};

/// Addressing of one group's rows.  The passes hand load / store the image slot and a compile-time step in slots
/// (slot_io); the staged copies name the row.  The resources start `lead` units in front of sample 0 of the signal of
/// the group's first row (never dereferenced there: the predicate) and end with the last signal (at most 4 GiB on).
/// REAL = false (ols_io): lengths, pitches, lead, hop and the fields of ols_row count complex elements, an image slot is
/// one of them.  REAL = true (rols_io, stockham_wg_rols.hpp): they count SCALARS and are even, apart from nvalid; image
/// slot j (+ the passes' compile-time step) is the scalar pair 2 (j + step), 2 (j + step) + 1.
template <typename T, int N, int FPW, int AUX, bool REAL>
struct window_io : slot_io {
  static constexpr unsigned ES = sizeof(cx<T>);
  static constexpr unsigned UB = REAL ? sizeof(T) : sizeof(cx<T>);  // bytes of the unit the geometry counts
  __amdgpu_buffer_rsrc_t rin, rout;
  unsigned in_length, lead;
  ols_row own;   // the window of this lane's row
  unsigned sig;  // ... and its signal (also of a row beyond the last signal: the filter index stays defined)

  PFA_DEV window_io(const void* in, void* out, unsigned g, unsigned f, unsigned n_signals, unsigned n_seg, unsigned lead_,
                    unsigned hop, unsigned in_length_, unsigned out_length, unsigned in_pitch, unsigned out_pitch)
      : in_length(in_length_), lead(lead_) {
    const unsigned i0 = (g * FPW) / n_seg;  // (uniform; the group exists, so i0 < n_signals)
    const unsigned long long after = n_signals - 1 - i0;
    const unsigned long long ibytes = (after * in_pitch + in_length + lead) * UB;
    const unsigned long long obytes = (after * out_pitch + out_length + lead) * UB;
    const long long ifirst = static_cast<long long>(i0) * in_pitch - lead, ofirst = static_cast<long long>(i0) * out_pitch - lead;
    rin = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(static_cast<const char*>(in)) + ifirst * UB, 0,
                                            ibytes > 0xFFFFFFFFull ? 0xFFFFFFFFu : static_cast<unsigned>(ibytes), 0x00020000);
    rout = __builtin_amdgcn_make_buffer_rsrc(static_cast<char*>(out) + ofirst * UB, 0,
                                             obytes > 0xFFFFFFFFull ? 0xFFFFFFFFu : static_cast<unsigned>(obytes), 0x00020000);
    const unsigned r = g * FPW + (FPW == 1 ? 0u : f);  // (one row per group: the window is uniform, and kept in SGPRs)
    sig = r / n_seg;
    const unsigned s = r - sig * n_seg;
    const unsigned first = s * hop;  // the row's first output sample (below out_length: n_seg = ceil(out_length / hop))
    const unsigned di = sig - i0;
    const bool live = sig < n_signals;
    const unsigned left = out_length - first;
    own.e0 = live ? first - lead : 0xC0000000u;
    own.nvalid = live ? (left < hop ? left : hop) : 0u;
    own.ibase = di * in_pitch + first;
    own.obase = di * out_pitch + first;
  }
  // slot j + step of the row with window w; `step` is the passes' compile-time part and rides the scalar offset, so
  // the butterflies of a lane share one address register.  The predicate decides, not the range check; neither part of
  // the address is negative (ols_row).
  PFA_DEV cx<T> load_in(const ols_row& w, unsigned j, unsigned step = 0) const {
    cx<T> x{T(0), T(0)};
    if constexpr (!REAL) {
      if (w.e0 + j + step < in_length) x = buf_load<T, AUX>(rin, (w.ibase + j) * ES, step * ES);
    } else {
      // p is even (e0 is), so p + 1 does not wrap; a window that starts in front of its signal has the wrapped negative
      // e0, and p is then either beyond every in_length or a small valid index.
      const unsigned p = w.e0 + 2 * (j + step);
      if (p < in_length) {
        if (p + 1 < in_length) {
          x = buf_load<T, AUX>(rin, (w.ibase + 2 * j) * UB, step * ES);
        } else {  // the last scalar of a signal of odd length
          x.re = buf_load_scalar<T, AUX>(rin, (w.ibase + 2 * j) * UB, step * ES);
        }
      }
    }
    return x;
  }
  PFA_DEV void store_out(cx<T> v, const ols_row& w, unsigned j, unsigned step = 0) const {
    if constexpr (!REAL) {
      if (j + step - lead < w.nvalid) buf_store<T, AUX>(v, rout, (w.obase + j) * ES, step * ES);
    } else {
      const unsigned m = 2 * (j + step) - lead;  // (even, or the wrapped negative even number: m + 1 does not wrap)
      if (m < w.nvalid) {
        if (m + 1 < w.nvalid) {
          buf_store<T, AUX>(v, rout, (w.obase + 2 * j) * UB, step * ES);
        } else {  // the last scalar of an odd count
          buf_store_scalar<T, AUX>(v.re, rout, (w.obase + 2 * j) * UB, step * ES);
        }
      }
    }
  }
  PFA_DEV cx<T> load(unsigned slot, unsigned step) const { return load_in(own, slot, step); }
  PFA_DEV void store(cx<T> v, unsigned slot, unsigned step) const { store_out(v, own, slot, step); }
};
template <typename T, int N, int FPW, int AUX>
using ols_io = window_io<T, N, FPW, AUX, false>;

/// `n_signals` signals of in_length complex samples (pitch in_pitch) -> as many of out_length (pitch out_pitch), each
/// in n_seg segments of Cfg::N points; `in` and `out` must not overlap.  tw: the Cfg::N-point tables.  filt: n_filters
/// spectra of Cfg::N elements, packed (of taps zero-padded to N); signal i takes i mod n_filters.  CORR: the conjugate
/// spectrum.  lead / hop: see the head of the file.  wg_twiddle_prologue; the persistent loop, the passes and the product
/// are stockham_wg_conv_kernel's.
template <typename Cfg, bool CORR>
__global__ __launch_bounds__(Cfg::WG, Cfg::OCC) void stockham_wg_ols_kernel(
    const void* in, void* out, const cx<typename Cfg::T>* __restrict__ tw, const cx<typename Cfg::T>* __restrict__ filt,
    unsigned n_signals, unsigned n_seg, unsigned n_filters, typename Cfg::T scale, unsigned lead, unsigned hop,
    unsigned in_length, unsigned out_length, unsigned in_pitch, unsigned out_pitch) {
  using T = typename Cfg::T;
  constexpr int N = Cfg::N;
  static_assert(Cfg::LDS_PER_FFT > 0, "LDS-resident configurations only");
  constexpr int UPT = (N + Cfg::TPF - 1) / Cfg::TPF;  // image slots per lane in the product
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
  const unsigned ngroups = (n_signals * n_seg + Cfg::FPW - 1) / Cfg::FPW;  // (the host keeps the row count below 2^31)
  for (unsigned g = blockIdx.x; g < ngroups; g += gridDim.x) {
    const ols_io<T, N, Cfg::FPW, Cfg::AUX> io(in, out, g, f, n_signals, n_seg, lead, hop, in_length, out_length, in_pitch,
                                              out_pitch);
    const cx<T>* twp = tw;
    if constexpr (Cfg::TWM == TW_GLOBAL) {
      asm volatile("" : "+s"(twp));  // (stockham_wg_body: keep the table reads inside the loop)
    }
    // the filter belongs to the signal (one modulo per group trip)
    const cx<T>* hp = filt + static_cast<size_t>(io.sig % n_filters) * N;
    if constexpr (Cfg::STAGED) {
      ols_row* rows = reinterpret_cast<ols_row*>(pfa_smem + conv_lds_bytes<Cfg>());
      if (tid == 0) rows[f] = io.own;
      __syncthreads();
      sfor<0, EPT>([&](auto k_) PFA_LAMBDA {
        const unsigned e = threadIdx.x + decltype(k_)::value * Cfg::WG;
        if (CH % Cfg::WG == 0 || e < CH) {
          all[(e / N) * Cfg::LDS_PER_FFT + lds_pad<Cfg>(e % N)] = io.load_in(rows[e / N], e % N);
        }
      });
      __syncthreads();
    }
    // 1. X = DFT_N(window), natural order, unscaled, in the image (the last pass ends with a barrier)
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
    // 3. scale * conj(DFT_N(image)); only the alias-free slots of a row leave
    wg_passes<Cfg, true, 0, WG_FIRST_FROM_LDS>(io, f, lds, tid, twp, twr, scale);
    if constexpr (Cfg::STAGED) {
      const ols_row* rows = reinterpret_cast<const ols_row*>(pfa_smem + conv_lds_bytes<Cfg>());
      sfor<0, EPT>([&](auto k_) PFA_LAMBDA {
        const unsigned e = threadIdx.x + decltype(k_)::value * Cfg::WG;
        if (CH % Cfg::WG == 0 || e < CH) {
          const cx<T> y = all[(e / N) * Cfg::LDS_PER_FFT + lds_pad<Cfg>(e % N)];
          io.store_out(cx<T>{y.re * scale, -(y.im * scale)}, rows[e / N], e % N);
        }
      });
      __syncthreads();  // (the images and the windows are the next trip's to write)
    }
  }
}

}  // namespace pfa
