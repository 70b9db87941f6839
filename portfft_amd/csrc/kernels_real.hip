// Real-data kernel instantiations for gfx950 (stockham_wg_real.hpp): R2C / C2R of N = 2 * M over the configuration list
// of wg_fused_cfg.hpp, fp32 M = 2 ... 8192 and fp64 M = 2 ... 4096.  Every entry is a spec_kernel that carries WF_REAL
// only.  Other lengths are specialised at commit time (jit.cpp: jit_fused_kernel, JF_REAL).
#include "kernels_impl.hpp"
#include "wg_fused_cfg.hpp"

namespace pfa {

const spec_kernel* real_kernels(int* count) {
  static const fused_registry reg([](auto c) {
    using Cfg = typename decltype(c)::cfg;
    return make_fused_entry<WF_REAL, Cfg>(c.groups_per_wg, real_lds_bytes<Cfg>(), &stockham_wg_r2c_kernel<Cfg>,
                                          &stockham_wg_c2r_kernel<Cfg>);
  });
  return reg.entries(count);
}

}  // namespace pfa
