// Pair convolution / correlation kernel instantiations for gfx950 (stockham_wg_pairs.hpp): pairs of rows of N = 2 * M real
// scalars over the configuration list of wg_fused_cfg.hpp, fp32 M = 2 ... 8192 and fp64 M = 2 ... 4096.  Every entry is a
// spec_kernel that carries WF_PAIRS only ([0] product, [1] conjugate product; the phase transform is an argument).  Other
// lengths are specialised at pfft_plan_prepare_pairs (jit.cpp: jit_fused_kernel, JF_PAIRS).
#include "kernels_impl.hpp"
#include "wg_fused_cfg.hpp"

namespace pfa {

const spec_kernel* pairs_kernels(int* count) {
  static const fused_registry reg([](auto c) {
    using Cfg = typename decltype(c)::cfg;
    return make_fused_entry<WF_PAIRS, Cfg>(c.groups_per_wg, pairs_lds_bytes<Cfg>(), &stockham_wg_pairs_kernel<Cfg, false>,
                                           &stockham_wg_pairs_kernel<Cfg, true>);
  });
  return reg.entries(count);
}

}  // namespace pfa
