// DCT-IV / MDCT kernel instantiations for gfx950 (stockham_wg_dct4.hpp): rows and frames of N = 2 * M real scalars over
// the configuration list of wg_fused_cfg.hpp, fp32 M = 2 ... 8192 and fp64 M = 2 ... 4096.  Every entry is a spec_kernel
// that carries WF_DCT4 only ([0] type-4 transform of rows, [1] MDCT of signals).  Other lengths are specialised at
// pfft_plan_prepare_dct4 / pfft_plan_set_mdct_window (jit.cpp: jit_fused_kernel, JF_DCT4).
#include "kernels_impl.hpp"
#include "wg_fused_cfg.hpp"

namespace pfa {

const spec_kernel* dct4_kernels(int* count) {
  static const fused_registry reg([](auto c) {
    using Cfg = typename decltype(c)::cfg;
    return make_fused_entry<WF_DCT4, Cfg>(c.groups_per_wg, dct4_lds_bytes<Cfg>(), &stockham_wg_dct4_kernel<Cfg, false>,
                                          &stockham_wg_dct4_kernel<Cfg, true>);
  });
  return reg.entries(count);
}

}  // namespace pfa
