// Discrete cosine transform kernel instantiations for gfx950 (stockham_wg_dct.hpp): rows of N = 2 * M real scalars over
// the configuration list of wg_fused_cfg.hpp, fp32 M = 2 ... 8192 and fp64 M = 2 ... 4096.  Every entry is a spec_kernel
// that carries WF_DCT only ([0] type 2, [1] type 3).  Other lengths are specialised at pfft_plan_prepare_dct (jit.cpp:
// jit_fused_kernel, JF_DCT).
#include "kernels_impl.hpp"
#include "wg_fused_cfg.hpp"

namespace pfa {

const spec_kernel* dct_kernels(int* count) {
  static const fused_registry reg([](auto c) {
    using Cfg = typename decltype(c)::cfg;
    return make_fused_entry<WF_DCT, Cfg>(c.groups_per_wg, dct_lds_bytes<Cfg>(), &stockham_wg_dct_kernel<Cfg, false>,
                                         &stockham_wg_dct_kernel<Cfg, true>);
  });
  return reg.entries(count);
}

}  // namespace pfa
