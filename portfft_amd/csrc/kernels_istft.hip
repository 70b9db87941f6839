// Inverse short-time Fourier transform kernel instantiations for gfx950 (stockham_wg_istft.hpp): frames of N = 2 * M
// real scalars over the configuration list of wg_fused_cfg.hpp, fp32 M = 2 ... 8192 and fp64 M = 2 ... 4096.  Every entry
// is a spec_kernel that carries WF_ISTFT only ([0] plain overlap-add, [1] normalised).  Other lengths are specialised
// when the synthesis window is set (jit.cpp: jit_fused_kernel, JF_ISTFT).
#include "kernels_impl.hpp"
#include "wg_fused_cfg.hpp"

namespace pfa {

const spec_kernel* istft_kernels(int* count) {
  static const fused_registry reg([](auto c) {
    using Cfg = typename decltype(c)::cfg;
    return make_fused_entry<WF_ISTFT, Cfg>(c.groups_per_wg, istft_lds_bytes<Cfg>(), &stockham_wg_istft_kernel<Cfg, false>,
                                           &stockham_wg_istft_kernel<Cfg, true>);
  });
  return reg.entries(count);
}

}  // namespace pfa
