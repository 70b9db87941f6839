// Real convolution kernel instantiations for gfx950 (stockham_wg_rconv.hpp): rows of N = 2 * M real scalars over the
// configuration list of wg_fused_cfg.hpp, fp32 M = 2 ... 8192 and fp64 M = 2 ... 4096.  Every entry is a spec_kernel
// that carries WF_RCONV only ([0] convolve, [1] correlate).  Other lengths are specialised at commit time (jit.cpp:
// jit_fused_kernel, JF_RCONV).
#include "kernels_impl.hpp"
#include "wg_fused_cfg.hpp"

namespace pfa {

const spec_kernel* rconv_kernels(int* count) {
  static const fused_registry reg([](auto c) {
    using Cfg = typename decltype(c)::cfg;
    return make_fused_entry<WF_RCONV, Cfg>(c.groups_per_wg, real_lds_bytes<Cfg>(), &stockham_wg_rconv_kernel<Cfg, false>,
                                           &stockham_wg_rconv_kernel<Cfg, true>);
  });
  return reg.entries(count);
}

}  // namespace pfa
