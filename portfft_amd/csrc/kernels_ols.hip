// Overlap-save filter kernel instantiations for gfx950 (stockham_wg_ols.hpp): segments of N points over the
// configuration list of wg_fused_cfg.hpp, fp32 N = 2 ... 8192 and fp64 N = 2 ... 4096.  Every entry is a spec_kernel that
// carries WF_OLS only ([0] convolve, [1] correlate).  Other lengths are specialised at commit time (jit.cpp:
// jit_fused_kernel, JF_OLS).
#include "kernels_impl.hpp"
#include "wg_fused_cfg.hpp"

namespace pfa {

const spec_kernel* ols_kernels(int* count) {
  static const fused_registry reg([](auto c) {
    using Cfg = typename decltype(c)::cfg;
    return make_fused_entry<WF_OLS, Cfg>(c.groups_per_wg, ols_lds_bytes<Cfg>(), &stockham_wg_ols_kernel<Cfg, false>,
                                         &stockham_wg_ols_kernel<Cfg, true>);
  });
  return reg.entries(count);
}

}  // namespace pfa
