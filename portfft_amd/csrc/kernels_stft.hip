// Short-time Fourier transform kernel instantiations for gfx950 (stockham_wg_stft.hpp): frames of N = 2 * M real
// scalars over the configuration list of wg_fused_cfg.hpp, fp32 M = 2 ... 8192 and fp64 M = 2 ... 4096.  Every entry is a
// spec_kernel that carries WF_STFT only ([0] zero extension, [1] reflection).  Other lengths are specialised when the
// window is set (jit.cpp: jit_fused_kernel, JF_STFT).
#include "kernels_impl.hpp"
#include "wg_fused_cfg.hpp"

namespace pfa {

const spec_kernel* stft_kernels(int* count) {
  static const fused_registry reg([](auto c) {
    using Cfg = typename decltype(c)::cfg;
    return make_fused_entry<WF_STFT, Cfg>(c.groups_per_wg, stft_lds_bytes<Cfg>(), &stockham_wg_stft_kernel<Cfg, false>,
                                          &stockham_wg_stft_kernel<Cfg, true>);
  });
  return reg.entries(count);
}

}  // namespace pfa
