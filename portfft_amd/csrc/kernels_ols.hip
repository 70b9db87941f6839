// Overlap-save filter kernel instantiations for gfx950 (stockham_wg_ols.hpp): segments of N points for the
// configuration lines of kernels_conv.hip, fp32 N = 2 ... 8192 and fp64 N = 2 ... 4096; N >= 256 reads them from
// wg_pow2_cfg.hpp.  Every entry is a spec_kernel that carries WF_OLS only ([0] convolve, [1] correlate).  Other lengths
// are specialised at commit time (jit.cpp: jit_ols_kernel).
#include "kernels_impl.hpp"
#include "wg_pow2_cfg.hpp"

namespace pfa {

namespace {
template <typename T, int N>
spec_kernel pow2_entry() {
  return make_spec_entry_ols<typename pow2_cfg<T, N>::cfg>(pow2_cfg<T, N>::groups_per_wg);
}

using f = float;
using d = double;
constexpr int NT = 2;
const spec_kernel g_ols[] = {
    make_spec_entry_ols<wg_cfg<f, radix_list<2>, 256, 256, 0, 0, TW_GLOBAL, 4, NT, 1>>(),     // N = 2
    make_spec_entry_ols<wg_cfg<f, radix_list<4>, 256, 256, 4, 1, TW_GLOBAL, 4, NT, 1>>(),     // 4
    make_spec_entry_ols<wg_cfg<f, radix_list<8>, 256, 256, 8, 1, TW_GLOBAL, 4, NT, 1>>(),     // 8
    make_spec_entry_ols<wg_cfg<f, radix_list<16>, 256, 256, 16, 1, TW_GLOBAL, 4, NT, 1>>(),   // 16
    make_spec_entry_ols<wg_cfg_twl<f, radix_list<8, 4>, 256, 64, 8, 1, 4, NT, 1>>(),          // 32
    make_spec_entry_ols<wg_cfg_twl<f, radix_list<8, 8>, 256, 32, 8, 1, 4, NT, 1>>(),          // 64
    make_spec_entry_ols<wg_cfg_twl<f, radix_list<16, 8>, 256, 32, 16, 1, 4, NT, 1>>(),        // 128
    pow2_entry<f, 256>(), pow2_entry<f, 512>(), pow2_entry<f, 1024>(),                         // 256, 512, 1024
    pow2_entry<f, 2048>(), pow2_entry<f, 4096>(), pow2_entry<f, 8192>(),                       // 2048, 4096, 8192
    make_spec_entry_ols<wg_cfg<d, radix_list<2>, 256, 256, 0, 0, TW_GLOBAL, 2, NT, 1>>(),     // N = 2
    make_spec_entry_ols<wg_cfg<d, radix_list<4>, 256, 256, 4, 1, TW_GLOBAL, 2, NT, 1>>(),     // 4
    make_spec_entry_ols<wg_cfg<d, radix_list<8>, 256, 256, 8, 1, TW_GLOBAL, 2, NT, 1>>(),     // 8
    make_spec_entry_ols<wg_cfg<d, radix_list<16>, 256, 128, 16, 1, TW_GLOBAL, 2, NT, 1>>(),   // 16
    make_spec_entry_ols<wg_cfg_twl<d, radix_list<8, 4>, 256, 64, 8, 1, 2, NT, 1>>(),          // 32
    make_spec_entry_ols<wg_cfg_twl<d, radix_list<8, 8>, 256, 32, 8, 1, 2, NT, 1>>(),          // 64
    make_spec_entry_ols<wg_cfg_twl<d, radix_list<16, 8>, 256, 32, 16, 1, 2, NT, 1>>(),        // 128
    pow2_entry<d, 256>(), pow2_entry<d, 512>(), pow2_entry<d, 1024>(),                         // 256, 512, 1024
    pow2_entry<d, 2048>(), pow2_entry<d, 4096>(),                                              // 2048, 4096
};
}  // namespace

const spec_kernel* ols_kernels(int* count) {
  *count = static_cast<int>(sizeof(g_ols) / sizeof(g_ols[0]));
  return g_ols;
}

}  // namespace pfa
