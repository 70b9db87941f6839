// Bluestein kernel instantiations for gfx950 (stockham_wg_bluestein.hpp): one entry per convolution length P, a power
// of two, on the configuration wg_pow2_cfg.hpp names for that length -- the one the real-data entry of M = P runs
// (LDS-resident, no software pipeline).  Every entry is a spec_kernel that carries WF_BLUESTEIN only.  The
// transform length N is a runtime argument: the entry of P serves every N with P / 4 < N <= P / 2.  N needs a prime
// factor above 61 and so is at least 67: P = 256 ... 8192 in fp32 (N <= 4096), 256 ... 4096 in fp64 (N <= 2048).
#include "kernels_impl.hpp"
#include "stockham_wg_bluestein.hpp"
#include "wg_pow2_cfg.hpp"

namespace pfa {

namespace {
template <typename T, int P>
spec_kernel make_entry() {
  using Cfg = typename pow2_cfg<T, P>::cfg;
  return make_fused_entry<WF_BLUESTEIN, Cfg>(pow2_cfg<T, P>::groups_per_wg, bluestein_lds_bytes<Cfg>(),
                                             &stockham_wg_bluestein_kernel<Cfg, false>, &stockham_wg_bluestein_kernel<Cfg, true>);
}

const spec_kernel g_bluestein[] = {
    make_entry<float, 256>(),  make_entry<float, 512>(),  make_entry<float, 1024>(),
    make_entry<float, 2048>(), make_entry<float, 4096>(), make_entry<float, 8192>(),
    make_entry<double, 256>(), make_entry<double, 512>(), make_entry<double, 1024>(),
    make_entry<double, 2048>(), make_entry<double, 4096>(),
};
}  // namespace

const spec_kernel* bluestein_kernels(int* count) {
  *count = static_cast<int>(sizeof(g_bluestein) / sizeof(g_bluestein[0]));
  return g_bluestein;
}

}  // namespace pfa
