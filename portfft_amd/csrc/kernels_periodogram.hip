// Power spectrogram / periodogram kernel instantiations for gfx950 (stockham_wg_periodogram.hpp): frames of N = 2 * M real
// scalars over the configuration list of wg_fused_cfg.hpp, fp32 M = 2 ... 8192 and fp64 M = 2 ... 4096.  Every entry is a
// spec_kernel that carries WF_PERIODOGRAM only ([0] zero extension, [1] reflection).  Other lengths are specialised at
// pfft_plan_set_periodogram_window (jit.cpp: jit_fused_kernel, JF_PERIODOGRAM).
#include "kernels_impl.hpp"
#include "wg_fused_cfg.hpp"

namespace pfa {

const spec_kernel* periodogram_kernels(int* count) {
  static const fused_registry reg([](auto c) {
    using Cfg = typename decltype(c)::cfg;
    return make_fused_entry<WF_PERIODOGRAM, Cfg>(c.groups_per_wg, periodogram_lds_bytes<Cfg>(),
                                                 &stockham_wg_periodogram_kernel<Cfg, false>,
                                                 &stockham_wg_periodogram_kernel<Cfg, true>);
  });
  return reg.entries(count);
}

}  // namespace pfa
