// Inverse MDCT kernel instantiations for gfx950 (stockham_wg_imdct.hpp): frames of N = 2 * M coefficients over the
// configuration list of wg_fused_cfg.hpp, fp32 M = 2 ... 8192 and fp64 M = 2 ... 4096.  Every entry is a spec_kernel that
// carries WF_IMDCT only; the form has one kernel, which fills both cells.  Other lengths are specialised at
// pfft_plan_set_imdct_window (jit.cpp: jit_fused_kernel, JF_IMDCT).
#include "kernels_impl.hpp"
#include "wg_fused_cfg.hpp"

namespace pfa {

const spec_kernel* imdct_kernels(int* count) {
  static const fused_registry reg([](auto c) {
    using Cfg = typename decltype(c)::cfg;
    return make_fused_entry<WF_IMDCT, Cfg>(c.groups_per_wg, imdct_lds_bytes<Cfg>(), &stockham_wg_imdct_kernel<Cfg>,
                                           &stockham_wg_imdct_kernel<Cfg>);
  });
  return reg.entries(count);
}

}  // namespace pfa
