// Shared body of kernels_f32.hip / kernels_f64.hip: turns wg_cfg<...> variants into registry entries.
#pragma once
#include <cstdlib>
#include <vector>

#include <hip/hip_ext.h>

#include "../../include/portfft_amd.h"
#include "generic_kernel.hpp"
#include "kernels.hpp"
#include "stockham_rows2d.hpp"
#include "stockham_strided.hpp"
#include "stockham_wg.hpp"
#include "stockham_wg_hx.hpp"
#include "stockham_wg_real.hpp"
#include "stockham_xlane.hpp"

#include <tuple>
#include <type_traits>
#include <utility>

namespace pfa {

/// Every launch of a pre-compiled kernel: the ordinary launch, or -- when the submission's completion event is armed
/// (kernels.hpp: arm_stop_event) -- hipExtLaunchKernel with that event as the dispatch's stop event.  The arguments
/// are converted to the kernel's formal parameter types before they are packed.
template <typename... KArgs, typename... Args, size_t... I>
inline hipError_t launch_with_stop_event(void (*kernel)(KArgs...), dim3 g, dim3 b, size_t lds, hipStream_t stream,
                                         hipEvent_t stop, std::index_sequence<I...>, Args&&... args) {
  std::tuple<KArgs...> formal(static_cast<KArgs>(args)...);
  void* p[] = {static_cast<void*>(&std::get<I>(formal))...};
  return hipExtLaunchKernel(reinterpret_cast<const void*>(kernel), g, b, p, lds, stream, nullptr, stop, 0);
}
template <typename... KArgs, typename... Args>
inline void launch_kernel(void (*kernel)(KArgs...), dim3 g, dim3 b, size_t lds, hipStream_t stream, Args&&... args) {
  static_assert(sizeof...(KArgs) == sizeof...(Args), "kernel argument count");
  if (hipEvent_t stop = take_stop_event()) {
    (void)launch_with_stop_event(kernel, g, b, lds, stream, stop, std::index_sequence_for<KArgs...>{},
                                 std::forward<Args>(args)...);
    return;
  }
  kernel<<<g, b, lds, stream>>>(static_cast<KArgs>(args)...);
}
}  // namespace pfa
// (hip_runtime.h defines hipLaunchKernelGGL as a macro; inside this library's device translation units every use of it
//  goes through pfa::launch_kernel)
#undef hipLaunchKernelGGL
#define hipLaunchKernelGGL(kernel, grid, block, lds, stream, ...) \
  ::pfa::launch_kernel(kernel, grid, block, lds, stream, __VA_ARGS__)

namespace pfa {

/// the same configuration with another cache policy (AUX)
template <typename Cfg, int AUX2>
struct with_aux;
template <typename T, typename Seq, int WG, int FPW, int PADS, int PADW, int TWM, int OCC, int AUX, int STAGED, int TWL,
          int AUX2>
struct with_aux<wg_cfg<T, Seq, WG, FPW, PADS, PADW, TWM, OCC, AUX, STAGED, TWL>, AUX2> {
  using type = wg_cfg<T, Seq, WG, FPW, PADS, PADW, TWM, OCC, AUX2, STAGED, TWL>;
};
template <typename Cfg, int AUX2>
using with_aux_t = typename with_aux<Cfg, AUX2>::type;

/// S: the storage scalar of the data (Cfg::T, or half_t for the fp16 forms: stockham_wg_*half*_kernel)
template <typename Cfg, typename S = typename Cfg::T>
hipError_t launch_spec_prefetch(hipStream_t stream, unsigned grid, const void* in, void* out, const void* tw,
                                long long nfft, double scale, int backward) {
  using T = typename Cfg::T;
  constexpr bool half = !std::is_same<S, T>::value;
  const auto* i = static_cast<const cx<S>*>(in);
  auto* o = static_cast<cx<S>*>(out);
  const auto* t = static_cast<const cx<T>*>(tw);
  // two-tier grid for large launches: `grid` is the planner's uniform grid (k groups per work-group); three quarters
  // of the groups keep that shape, the last quarter goes to work-groups of 2 groups each
  const long long ngroups = (nfft + Cfg::FPW - 1) / Cfg::FPW;
  const long long k = grid > 0 ? (ngroups + grid - 1) / grid : 1;
  long long n_main = 0;
  static const bool uniform_only = getenv("PFFT_UNIFORM_GRID") != nullptr;  // A/B switch (profiles/r2_notes.md)
  if (k >= 4 && grid >= 4096 && !uniform_only) {
    n_main = (static_cast<long long>(grid) * 3 / 4) & ~255ll;
    const long long rest = ngroups - k * n_main;
    grid = static_cast<unsigned>(n_main + (rest + 1) / 2);
  }
  const int main_k = static_cast<int>(k);
  if constexpr (half) {
    if (backward) {
      hipLaunchKernelGGL((stockham_wg_prefetch_half_kernel<Cfg, true>), dim3(grid), dim3(Cfg::WG), Cfg::LDS_BYTES, stream,
                         i, o, t, nfft, static_cast<T>(scale), n_main, main_k);
    } else {
      hipLaunchKernelGGL((stockham_wg_prefetch_half_kernel<Cfg, false>), dim3(grid), dim3(Cfg::WG), Cfg::LDS_BYTES,
                         stream, i, o, t, nfft, static_cast<T>(scale), n_main, main_k);
    }
  } else if (backward) {
    hipLaunchKernelGGL((stockham_wg_prefetch_kernel<Cfg, true>), dim3(grid), dim3(Cfg::WG), Cfg::LDS_BYTES, stream, i,
                       o, t, nfft, static_cast<T>(scale), n_main, main_k);
  } else {
    hipLaunchKernelGGL((stockham_wg_prefetch_kernel<Cfg, false>), dim3(grid), dim3(Cfg::WG), Cfg::LDS_BYTES, stream,
                       i, o, t, nfft, static_cast<T>(scale), n_main, main_k);
  }
  return hipGetLastError();
}

template <typename Cfg, typename S = typename Cfg::T>
hipError_t launch_spec(hipStream_t stream, unsigned grid, const void* in, void* out, const void* tw, long long nfft,
                       double scale, int backward) {
  using T = typename Cfg::T;
  const auto* i = static_cast<const cx<S>*>(in);
  auto* o = static_cast<cx<S>*>(out);
  const auto* t = static_cast<const cx<T>*>(tw);
  if constexpr (!std::is_same<S, T>::value) {
    if (backward) {
      hipLaunchKernelGGL((stockham_wg_half_kernel<Cfg, true>), dim3(grid), dim3(Cfg::WG), Cfg::LDS_BYTES, stream, i, o,
                         t, nfft, static_cast<T>(scale));
    } else {
      hipLaunchKernelGGL((stockham_wg_half_kernel<Cfg, false>), dim3(grid), dim3(Cfg::WG), Cfg::LDS_BYTES, stream, i, o,
                         t, nfft, static_cast<T>(scale));
    }
  } else if (backward) {
    hipLaunchKernelGGL((stockham_wg_kernel<Cfg, true>), dim3(grid), dim3(Cfg::WG), Cfg::LDS_BYTES, stream, i, o, t,
                       nfft, static_cast<T>(scale));
  } else {
    hipLaunchKernelGGL((stockham_wg_kernel<Cfg, false>), dim3(grid), dim3(Cfg::WG), Cfg::LDS_BYTES, stream, i, o, t,
                       nfft, static_cast<T>(scale));
  }
  return hipGetLastError();
}

template <typename Cfg, typename S = typename Cfg::T>
hipError_t launch_spec_split(hipStream_t stream, unsigned grid, const void* in_re, const void* in_im, void* out_re,
                             void* out_im, const void* tw, long long nfft, double scale, int backward) {
  using T = typename Cfg::T;
  const auto* t = static_cast<const cx<T>*>(tw);
  const dim3 g(grid), b(Cfg::WG);
  if constexpr (!std::is_same<S, T>::value) {
    const auto *ir = static_cast<const S*>(in_re), *ii = static_cast<const S*>(in_im);
    auto *orr = static_cast<S*>(out_re), *oi = static_cast<S*>(out_im);
    if (backward) {
      hipLaunchKernelGGL((stockham_wg_half_split_kernel<Cfg, true>), g, b, Cfg::LDS_BYTES, stream, ir, ii, orr, oi, t,
                         nfft, static_cast<T>(scale));
    } else {
      hipLaunchKernelGGL((stockham_wg_half_split_kernel<Cfg, false>), g, b, Cfg::LDS_BYTES, stream, ir, ii, orr, oi, t,
                         nfft, static_cast<T>(scale));
    }
  } else if (backward) {
    hipLaunchKernelGGL((stockham_wg_split_kernel<Cfg, true>), g, b, Cfg::LDS_BYTES, stream, static_cast<const T*>(in_re),
                       static_cast<const T*>(in_im), static_cast<T*>(out_re), static_cast<T*>(out_im), t, nfft,
                       static_cast<T>(scale));
  } else {
    hipLaunchKernelGGL((stockham_wg_split_kernel<Cfg, false>), g, b, Cfg::LDS_BYTES, stream,
                       static_cast<const T*>(in_re), static_cast<const T*>(in_im), static_cast<T*>(out_re),
                       static_cast<T*>(out_im), t, nfft, static_cast<T>(scale));
  }
  return hipGetLastError();
}

template <typename Cfg>
spec_kernel make_spec_entry(int groups_per_wg = 1);

/// software-pipelined form (stockham_wg_prefetch_kernel) of a direct-I/O multi-pass variant
template <typename Cfg>
spec_kernel make_spec_entry_prefetch(int groups_per_wg = 4) {
  spec_kernel k = make_spec_entry<Cfg>(groups_per_wg);
  k.fn[0] = reinterpret_cast<const void*>(&stockham_wg_prefetch_kernel<Cfg, false>);
  k.fn[1] = reinterpret_cast<const void*>(&stockham_wg_prefetch_kernel<Cfg, true>);
  k.launch = &launch_spec_prefetch<Cfg>;
  return k;
}

/// the fields every form of a packed configuration shares (no kernel is instantiated by this)
template <typename Cfg>
spec_kernel spec_entry_fields(int groups_per_wg) {
  spec_kernel k{};
  k.groups_per_wg = groups_per_wg;
  k.precision = sizeof(typename Cfg::T) == 8 ? PFFT_PRECISION_F64 : PFFT_PRECISION_F32;
  k.n = Cfg::N;
  k.wg = Cfg::WG;
  k.fpw = Cfg::FPW;
  k.lds_bytes = Cfg::LDS_BYTES;
  k.n_radices = Cfg::NP;
  for (int i = 0; i < Cfg::NP; ++i) k.radices[i] = Cfg::Seq::r[i];
  k.tw_total = Cfg::Seq::tw_total;
  k.tw_in_regs = Cfg::TWM == TW_REGS ? 1 : 0;
  k.pads = Cfg::PADS;
  k.padw = Cfg::PADW;
  k.twm = Cfg::TWM;
  k.occ = Cfg::OCC;
  k.aux = Cfg::AUX;
  k.staged = Cfg::STAGED;
  k.twl = Cfg::TWL;
  return k;
}

template <typename Cfg>
spec_kernel make_spec_entry(int groups_per_wg) {
  spec_kernel k = spec_entry_fields<Cfg>(groups_per_wg);
  k.fn[0] = reinterpret_cast<const void*>(&stockham_wg_kernel<Cfg, false>);
  k.fn[1] = reinterpret_cast<const void*>(&stockham_wg_kernel<Cfg, true>);
  k.launch = &launch_spec<Cfg>;
  k.fn_split[0] = reinterpret_cast<const void*>(&stockham_wg_split_kernel<Cfg, false>);
  k.fn_split[1] = reinterpret_cast<const void*>(&stockham_wg_split_kernel<Cfg, true>);
  k.launch_split = &launch_spec_split<Cfg>;
  return k;
}

template <typename Cfg>
hipError_t launch_spec_xlane(hipStream_t stream, unsigned grid, const void* in, void* out, const void* tw,
                             long long nfft, double scale, int backward) {
  using T = typename Cfg::T;
  const auto* i = static_cast<const cx<T>*>(in);
  auto* o = static_cast<cx<T>*>(out);
  const auto* t = static_cast<const cx<T>*>(tw);
  if (backward) {
    hipLaunchKernelGGL((stockham_wg_xlane_kernel<Cfg, true>), dim3(grid), dim3(Cfg::WG), Cfg::LDS_BYTES, stream, i, o,
                       t, nfft, static_cast<T>(scale));
  } else {
    hipLaunchKernelGGL((stockham_wg_xlane_kernel<Cfg, false>), dim3(grid), dim3(Cfg::WG), Cfg::LDS_BYTES, stream, i, o,
                       t, nfft, static_cast<T>(scale));
  }
  return hipGetLastError();
}

/// cross-lane form (stockham_xlane.hpp) of an N = R * R staged variant; interleaved storage (split storage keeps
/// the LDS form of the same configuration)
template <typename Cfg>
spec_kernel make_spec_entry_xlane(int groups_per_wg = 1) {
  spec_kernel k = make_spec_entry<Cfg>(groups_per_wg);
  k.fn[0] = reinterpret_cast<const void*>(&stockham_wg_xlane_kernel<Cfg, false>);
  k.fn[1] = reinterpret_cast<const void*>(&stockham_wg_xlane_kernel<Cfg, true>);
  k.launch = &launch_spec_xlane<Cfg>;
  k.xlane = 1;
  return k;
}

template <typename Cfg, bool PF = false, typename S = typename Cfg::T>
hipError_t launch_spec_hx(hipStream_t stream, unsigned grid, const void* in, void* out, const void* tw, long long nfft,
                          double scale, int backward) {
  using T = typename Cfg::T;
  const auto* i = static_cast<const cx<S>*>(in);
  auto* o = static_cast<cx<S>*>(out);
  const auto* t = static_cast<const cx<T>*>(tw);
  constexpr size_t lds = wg_hx_lds_bytes<Cfg>();
  if constexpr (!std::is_same<S, T>::value) {
    if (backward) {
      hipLaunchKernelGGL((stockham_wg_hx_half_kernel<Cfg, true, PF>), dim3(grid), dim3(Cfg::WG), lds, stream, i, o, t, nfft, static_cast<T>(scale));
    } else {
      hipLaunchKernelGGL((stockham_wg_hx_half_kernel<Cfg, false, PF>), dim3(grid), dim3(Cfg::WG), lds, stream, i, o, t, nfft, static_cast<T>(scale));
    }
  } else if (backward) {
    hipLaunchKernelGGL((stockham_wg_hx_kernel<Cfg, true, PF>), dim3(grid), dim3(Cfg::WG), lds, stream, i, o, t, nfft, static_cast<T>(scale));
  } else {
    hipLaunchKernelGGL((stockham_wg_hx_kernel<Cfg, false, PF>), dim3(grid), dim3(Cfg::WG), lds, stream, i, o, t, nfft, static_cast<T>(scale));
  }
  return hipGetLastError();
}

template <typename Cfg, bool PF = false, typename S = typename Cfg::T>
hipError_t launch_spec_hx_split(hipStream_t stream, unsigned grid, const void* in_re, const void* in_im, void* out_re,
                                void* out_im, const void* tw, long long nfft, double scale, int backward) {
  using T = typename Cfg::T;
  const auto* t = static_cast<const cx<T>*>(tw);
  const dim3 g(grid), b(Cfg::WG);
  constexpr size_t lds = wg_hx_lds_bytes<Cfg>();
  if constexpr (!std::is_same<S, T>::value) {
    const auto *ir = static_cast<const S*>(in_re), *ii = static_cast<const S*>(in_im);
    auto *orr = static_cast<S*>(out_re), *oi = static_cast<S*>(out_im);
    if (backward) {
      hipLaunchKernelGGL((stockham_wg_hx_half_split_kernel<Cfg, true, PF>), g, b, lds, stream, ir, ii, orr, oi, t, nfft, static_cast<T>(scale));
    } else {
      hipLaunchKernelGGL((stockham_wg_hx_half_split_kernel<Cfg, false, PF>), g, b, lds, stream, ir, ii, orr, oi, t, nfft, static_cast<T>(scale));
    }
  } else if (backward) {
    hipLaunchKernelGGL((stockham_wg_hx_split_kernel<Cfg, true, PF>), g, b, lds, stream, static_cast<const T*>(in_re),
                       static_cast<const T*>(in_im), static_cast<T*>(out_re), static_cast<T*>(out_im), t, nfft, static_cast<T>(scale));
  } else {
    hipLaunchKernelGGL((stockham_wg_hx_split_kernel<Cfg, false, PF>), g, b, lds, stream, static_cast<const T*>(in_re),
                       static_cast<const T*>(in_im), static_cast<T*>(out_re), static_cast<T*>(out_im), t, nfft, static_cast<T>(scale));
  }
  return hipGetLastError();
}

/// register-resident form (stockham_wg_hx.hpp) of a packed length; PF: its software-pipelined form
template <typename Cfg, bool PF = false>
spec_kernel make_spec_entry_hx(int groups_per_wg = 0) {
  // (fields only: the LDS-resident stockham_wg kernels of such a configuration -- fp32 32768 would need a 256 KiB image --
  //  are never instantiated, and every pointer of the entry is the register-resident kernel's: ADVICE r5)
  spec_kernel k = spec_entry_fields<Cfg>(groups_per_wg);
  k.lds_bytes = wg_hx_lds_bytes<Cfg>();
  k.fn[0] = reinterpret_cast<const void*>(&stockham_wg_hx_kernel<Cfg, false, PF>);
  k.fn[1] = reinterpret_cast<const void*>(&stockham_wg_hx_kernel<Cfg, true, PF>);
  k.launch = &launch_spec_hx<Cfg, PF>;
  k.fn_split[0] = reinterpret_cast<const void*>(&stockham_wg_hx_split_kernel<Cfg, false, PF>);
  k.fn_split[1] = reinterpret_cast<const void*>(&stockham_wg_hx_split_kernel<Cfg, true, PF>);
  k.launch_split = &launch_spec_hx_split<Cfg, PF>;
  k.hx = 1;
  return k;
}

/// fp16 storage (PFFT_PRECISION_F16) forms of an fp32 configuration: the same kernels behind converting I/O objects
/// (stockham_wg.hpp, packed_io / packed_split_io with S = half_t); the LDS, twiddles and grid rule are the fp32 entry's
template <typename Cfg>
spec_kernel make_spec_entry_half(int groups_per_wg = 1) {
  static_assert(sizeof(typename Cfg::T) == 4, "fp16 storage computes in fp32");
  spec_kernel k = spec_entry_fields<Cfg>(groups_per_wg);
  k.precision = PFFT_PRECISION_F16;
  k.fn[0] = reinterpret_cast<const void*>(&stockham_wg_half_kernel<Cfg, false>);
  k.fn[1] = reinterpret_cast<const void*>(&stockham_wg_half_kernel<Cfg, true>);
  k.launch = &launch_spec<Cfg, half_t>;
  k.fn_split[0] = reinterpret_cast<const void*>(&stockham_wg_half_split_kernel<Cfg, false>);
  k.fn_split[1] = reinterpret_cast<const void*>(&stockham_wg_half_split_kernel<Cfg, true>);
  k.launch_split = &launch_spec_split<Cfg, half_t>;
  return k;
}

template <typename Cfg>
spec_kernel make_spec_entry_prefetch_half(int groups_per_wg = 4) {
  spec_kernel k = make_spec_entry_half<Cfg>(groups_per_wg);
  k.fn[0] = reinterpret_cast<const void*>(&stockham_wg_prefetch_half_kernel<Cfg, false>);
  k.fn[1] = reinterpret_cast<const void*>(&stockham_wg_prefetch_half_kernel<Cfg, true>);
  k.launch = &launch_spec_prefetch<Cfg, half_t>;
  return k;
}

template <typename Cfg, bool PF = false>
spec_kernel make_spec_entry_hx_half(int groups_per_wg = 0) {
  static_assert(sizeof(typename Cfg::T) == 4, "fp16 storage computes in fp32");
  spec_kernel k = spec_entry_fields<Cfg>(groups_per_wg);
  k.precision = PFFT_PRECISION_F16;
  k.lds_bytes = wg_hx_lds_bytes<Cfg>();
  k.fn[0] = reinterpret_cast<const void*>(&stockham_wg_hx_half_kernel<Cfg, false, PF>);
  k.fn[1] = reinterpret_cast<const void*>(&stockham_wg_hx_half_kernel<Cfg, true, PF>);
  k.launch = &launch_spec_hx<Cfg, PF, half_t>;
  k.fn_split[0] = reinterpret_cast<const void*>(&stockham_wg_hx_half_split_kernel<Cfg, false, PF>);
  k.fn_split[1] = reinterpret_cast<const void*>(&stockham_wg_hx_half_split_kernel<Cfg, true, PF>);
  k.launch_split = &launch_spec_hx_split<Cfg, PF, half_t>;
  k.hx = 1;
  return k;
}

/// real-data forms (stockham_wg_real.hpp) of the M-point configuration Cfg: R2C / C2R of N = 2 * Cfg::N
template <typename Cfg>
real_kernel make_spec_entry_real(int groups_per_wg = 1) {
  static_assert(Cfg::LDS_PER_FFT > 0, "LDS-resident configurations only");
  real_kernel k{};
  k.cfg = spec_entry_fields<Cfg>(groups_per_wg);
  k.lds_bytes = real_lds_bytes<Cfg>();
  k.fn[0] = kernel_fn{reinterpret_cast<const void*>(&stockham_wg_r2c_kernel<Cfg>), nullptr, false};
  k.fn[1] = kernel_fn{reinterpret_cast<const void*>(&stockham_wg_c2r_kernel<Cfg>), nullptr, false};
  return k;
}

/// one form of a pre-compiled entry: the forward / backward host symbols; any_order: the form honours the stage's
/// any_order (kernel_fn)
template <typename... A>
inline void set_form(kernel_fn (&f)[2], void (*fwd)(A...), void (*bwd)(A...), bool any_order) {
  f[0] = kernel_fn{reinterpret_cast<const void*>(fwd), nullptr, any_order};
  f[1] = kernel_fn{reinterpret_cast<const void*>(bwd), nullptr, any_order};
}

template <typename Cfg>
rows2d_kernel make_rows2d_entry(int groups_per_wg);

/// the entry for Cfg (cache policy nt) and its writer twin (default-policy stores)
template <typename Cfg>
void add_rows2d_entries(std::vector<rows2d_kernel>& v, int groups_per_wg) {
  rows2d_kernel k = make_rows2d_entry<Cfg>(groups_per_wg);
  set_form(k.form[R2_SPLIT], &stockham_rows2d_kernel<Cfg, false, true>, &stockham_rows2d_kernel<Cfg, true, true>, false);
  v.push_back(k);
  rows2d_kernel w = make_rows2d_entry<with_aux_t<Cfg, PFA_AUX_WRITER>>(groups_per_wg);
  w.policy = 1;
  // (round 6: the split-storage form of the writer twin too -- the two-pass 2-D plan of SPLIT_COMPLEX data in cache-sized chunks)
  using WCfg = with_aux_t<Cfg, PFA_AUX_WRITER>;
  set_form(w.form[R2_SPLIT], &stockham_rows2d_kernel<WCfg, false, true>, &stockham_rows2d_kernel<WCfg, true, true>, false);
  v.push_back(w);
}

/// Cfg: the row FFT's wg_cfg with FPW = rows per work-group (= the column radix)
template <typename Cfg>
rows2d_kernel make_rows2d_entry(int groups_per_wg) {
  rows2d_kernel k{};
  k.precision = sizeof(typename Cfg::T) == 8 ? PFFT_PRECISION_F64 : PFFT_PRECISION_F32;
  k.n = Cfg::N;
  k.rc = Cfg::FPW;
  k.wg = Cfg::WG;
  k.lds_bytes = Cfg::LDS_BYTES;
  k.n_radices = Cfg::NP;
  for (int i = 0; i < Cfg::NP; ++i) k.radices[i] = Cfg::Seq::r[i];
  k.groups_per_wg = groups_per_wg;
  set_form(k.form[R2_INTERLEAVED], &stockham_rows2d_kernel<Cfg, false>, &stockham_rows2d_kernel<Cfg, true>, true);
  return k;
}

/// mark an entry as the wide-group alternative of its length (strided_kernel::wide)
inline strided_kernel wide(strided_kernel k) {
  k.wide = 1;
  return k;
}

/// mark an entry as the alternative of its length for stages with a row-shaped side (strided_kernel::rowish)
inline strided_kernel rowish(strided_kernel k) {
  k.rowish = 1;
  return k;
}

/// add the row-staged forms to an entry (fp32: a wave covers only 64/FPW * 8 B of a row when addressed f-fastest)
template <typename Cfg>
strided_kernel with_rows(strided_kernel k) {
  set_form(k.form[SF_ROW_IN], &stockham_strided_row_kernel<Cfg, false, true, false>,
           &stockham_strided_row_kernel<Cfg, true, true, false>, false);
  set_form(k.form[SF_ROW_OUT], &stockham_strided_row_kernel<Cfg, false, false, true>,
           &stockham_strided_row_kernel<Cfg, true, false, true>, false);
  k.lds_bytes_row = strided_row_lds_bytes<Cfg>();
  return k;
}

/// add the tiled-input form (four-step stage B reading a group-major intermediate) to an entry
/// (PF: the software-pipelined kernel's tiled-input form; LTW: ... carrying the inter-stage twiddles on its loads, tables
/// in LDS behind the kernel's own: strided_kernel::fs_ltw)
template <typename Cfg, bool PF = false, int LTW = 0>
strided_kernel with_tin(strided_kernel k) {
  static_assert(tin_supported<Cfg>(), "see tin_supported()");
  if constexpr (PF) {
    set_form(k.form[SF_TIN], &stockham_strided_prefetch_kernel<Cfg, false, 0, 0, true, LTW>,
             &stockham_strided_prefetch_kernel<Cfg, true, 0, 0, true, LTW>, true);
  } else {
    static_assert(LTW == 0, "the load-side modifier exists in the software-pipelined kernel only");
    set_form(k.form[SF_TIN], &stockham_strided_kernel<Cfg, false, 0, 0, true>, &stockham_strided_kernel<Cfg, true, 0, 0, true>,
             true);
  }
  return k;
}

/// tiled-input form for tiles twice as wide as the entry's groups (SF_TIN_W)
template <typename Cfg>
strided_kernel with_tin_w(strided_kernel k) {
  static_assert(tin_supported<Cfg, 2 * Cfg::FPW>(), "see tin_supported()");
  set_form(k.form[SF_TIN_W], &stockham_strided_kernel<Cfg, false, 0, 0, 2 * Cfg::FPW>,
           &stockham_strided_kernel<Cfg, true, 0, 0, 2 * Cfg::FPW>, true);
  k.tin_w = 2 * Cfg::FPW;
  return k;
}

/// the plain and store-modifier forms of a pre-compiled entry, in the order [backward * 2 + store_modifier]
template <typename... A>
inline void set_plain_stw(strided_kernel& k, void (*f0)(A...), void (*f1)(A...), void (*b0)(A...), void (*b1)(A...)) {
  set_form(k.form[SF_PLAIN], f0, b0, true);
  set_form(k.form[SF_STW], f1, b1, true);
}

template <typename Cfg>
strided_kernel make_strided_entry(int groups_per_wg = 1);

template <typename Cfg>
strided_kernel make_strided_entry_prefetch(int groups_per_wg = 4) {
  strided_kernel k = make_strided_entry<Cfg>(groups_per_wg);
  set_plain_stw(k, &stockham_strided_prefetch_kernel<Cfg, false, false>, &stockham_strided_prefetch_kernel<Cfg, false, true>,
                &stockham_strided_prefetch_kernel<Cfg, true, false>, &stockham_strided_prefetch_kernel<Cfg, true, true>);
  return k;
}

/// flags of add_strided_entries
/// SE_FS_A / SE_FS_B: the entry of its length for the four-step stage A / stage B (strided_kernel::fs_a / fs_b)
enum : unsigned { SE_ROWS = 1, SE_TIN = 2, SE_WIDE = 4, SE_ROWISH = 8, SE_PREFETCH = 16, SE_FS_A = 32, SE_FS_B = 64, SE_FS_ONLY = 128,
                SE_LTW = 256 /* fs_b entry carrying the modifier on its loads (strided_kernel::fs_ltw) */,
                SE_PLAIN_WRITER = 512 /* the writer twin also carries the forms without store modifier (stage A of an SE_LTW pair) */,
                SE_TIN_W = 1024 /* ... and the tiled-input form for tiles of 2 * FPW elements (SF_TIN_W) */ };

template <typename Cfg, unsigned F>
strided_kernel make_strided_entry_flags(int groups_per_wg) {
  strided_kernel k = (F & SE_PREFETCH) ? make_strided_entry_prefetch<Cfg>(groups_per_wg) : make_strided_entry<Cfg>(groups_per_wg);
  if constexpr ((F & SE_ROWS) != 0) k = with_rows<Cfg>(k);
  if constexpr ((F & SE_TIN) != 0) k = with_tin<Cfg, (F & SE_PREFETCH) != 0, (F & SE_LTW) != 0 ? 1 : 0>(k);
  if constexpr ((F & SE_TIN_W) != 0) k = with_tin_w<Cfg>(k);
  k.fs_ltw = (F & SE_LTW) != 0;
  k.wide = (F & SE_WIDE) != 0;
  k.rowish = (F & SE_ROWISH) != 0;
  k.fs_a = (F & SE_FS_A) != 0;
  k.fs_b = (F & SE_FS_B) != 0;
  k.fs_only = (F & SE_FS_ONLY) != 0;
  static_assert((F & SE_FS_B) == 0 || (F & SE_TIN) != 0, "a four-step stage-B entry needs its tiled-input form");
  return k;
}

/// policy twin of `base` (the nt entry of the same shape): Cfg carries the twin's AUX; only the forms a writer
/// (policy 1: with the store modifier, four-step stage A) or a reader (policy 2: without it, stage B and the second pass
/// of the two-pass 2-D plan) is ever launched in are instantiated, the others stay empty
template <typename Cfg, unsigned F>
strided_kernel make_strided_twin(const strided_kernel& base, int policy) {
  constexpr bool PF = (F & SE_PREFETCH) != 0;
  strided_kernel k = base;
  k.policy = policy;
  for (auto& f : k.form) f[0] = f[1] = kernel_fn{};
  k.tin_w = 0;
  if (policy == 1) {
    if constexpr (PF) {
      set_form(k.form[SF_STW], &stockham_strided_prefetch_kernel<Cfg, false, true>, &stockham_strided_prefetch_kernel<Cfg, true, true>,
               true);
    } else {
      set_form(k.form[SF_STW], &stockham_strided_kernel<Cfg, false, true>, &stockham_strided_kernel<Cfg, true, true>, true);
    }
    if constexpr ((F & SE_PLAIN_WRITER) != 0) {  // stage A of a pair whose stage B carries the modifier: no store modifier
      static_assert(!PF, "plain writer forms: the non-pipelined kernel");
      set_form(k.form[SF_PLAIN], &stockham_strided_kernel<Cfg, false, false>, &stockham_strided_kernel<Cfg, true, false>, true);
    }
  } else {
    if constexpr (PF) {
      set_form(k.form[SF_PLAIN], &stockham_strided_prefetch_kernel<Cfg, false, false>,
               &stockham_strided_prefetch_kernel<Cfg, true, false>, true);
    } else {
      set_form(k.form[SF_PLAIN], &stockham_strided_kernel<Cfg, false, false>, &stockham_strided_kernel<Cfg, true, false>, true);
    }
    if constexpr ((F & SE_ROWS) != 0) {
      set_form(k.form[SF_ROW_IN], &stockham_strided_row_kernel<Cfg, false, true, false>,
               &stockham_strided_row_kernel<Cfg, true, true, false>, false);
    }
    if constexpr ((F & SE_TIN) != 0) k = with_tin<Cfg, PF, (F & SE_LTW) != 0 ? 1 : 0>(k);
    if constexpr ((F & SE_TIN_W) != 0) k = with_tin_w<Cfg>(k);
    // (round 6: the reader twin of a wide entry -- the second pass of the two-pass 2-D plan -- carries its split-storage form)
    if constexpr ((F & SE_WIDE) != 0 && !PF) {
      set_form(k.form[SF_SPLIT], &stockham_strided_kernel<Cfg, false, false, true>, &stockham_strided_kernel<Cfg, true, false, true>,
               false);
    }
  }
  return k;
}

/// the entry for Cfg (cache policy nt) and its writer / reader twins
template <typename Cfg, unsigned F = 0>
void add_strided_entries(std::vector<strided_kernel>& v, int groups_per_wg = 1, int fs_groups_per_wg = 0) {
  strided_kernel base = make_strided_entry_flags<Cfg, F>(groups_per_wg);
  base.fs_groups_per_wg = fs_groups_per_wg;
  v.push_back(base);
  v.push_back(make_strided_twin<with_aux_t<Cfg, PFA_AUX_WRITER>, F>(base, 1));
  v.push_back(make_strided_twin<with_aux_t<Cfg, PFA_AUX_READER>, F>(base, 2));
}

template <typename Cfg>
strided_kernel make_strided_entry(int groups_per_wg) {
  strided_kernel k{};
  k.groups_per_wg = groups_per_wg;
  k.precision = sizeof(typename Cfg::T) == 8 ? PFFT_PRECISION_F64 : PFFT_PRECISION_F32;
  k.n = Cfg::N;
  k.wg = Cfg::WG;
  k.fpw = Cfg::FPW;
  k.lds_bytes = strided_lds_bytes<Cfg>();
  k.stw_mode = 1;
  k.n_radices = Cfg::NP;
  for (int i = 0; i < Cfg::NP; ++i) k.radices[i] = Cfg::Seq::r[i];
  set_plain_stw(k, &stockham_strided_kernel<Cfg, false, false>, &stockham_strided_kernel<Cfg, false, true>,
                &stockham_strided_kernel<Cfg, true, false>, &stockham_strided_kernel<Cfg, true, true>);
  set_form(k.form[SF_SPLIT], &stockham_strided_kernel<Cfg, false, false, true>, &stockham_strided_kernel<Cfg, true, false, true>,
           false);
  return k;
}

}  // namespace pfa
