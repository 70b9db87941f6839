// Inverse short-time Fourier transform kernel instantiations for gfx950 (stockham_wg_istft.hpp): frames of N = 2 * M
// real scalars, for the configuration lines of kernels_real.hip, fp32 M = 2 ... 8192 and fp64 M = 2 ... 4096;
// M >= 256 reads them from wg_pow2_cfg.hpp.  Every entry is a spec_kernel that carries WF_ISTFT only
// ([0] plain overlap-add, [1] normalised).  Other lengths are specialised when the synthesis window is set (jit.cpp:
// jit_istft_kernel).
#include "kernels_impl.hpp"
#include "wg_pow2_cfg.hpp"

namespace pfa {

namespace {
template <typename T, int M>
spec_kernel pow2_entry() {
  return make_spec_entry_istft<typename pow2_cfg<T, M>::cfg>(pow2_cfg<T, M>::groups_per_wg);
}

using f = float;
using d = double;
constexpr int NT = 2;
const spec_kernel g_istft[] = {
    make_spec_entry_istft<wg_cfg<f, radix_list<2>, 256, 256, 0, 0, TW_GLOBAL, 4, NT, 1>>(),     // N = 4
    make_spec_entry_istft<wg_cfg<f, radix_list<4>, 256, 256, 4, 1, TW_GLOBAL, 4, NT, 1>>(),     // 8
    make_spec_entry_istft<wg_cfg<f, radix_list<8>, 256, 256, 8, 1, TW_GLOBAL, 4, NT, 1>>(),     // 16
    make_spec_entry_istft<wg_cfg<f, radix_list<16>, 256, 256, 16, 1, TW_GLOBAL, 4, NT, 1>>(),   // 32
    make_spec_entry_istft<wg_cfg_twl<f, radix_list<8, 4>, 256, 64, 8, 1, 4, NT, 1>>(),          // 64
    make_spec_entry_istft<wg_cfg_twl<f, radix_list<8, 8>, 256, 32, 8, 1, 4, NT, 1>>(),          // 128
    make_spec_entry_istft<wg_cfg_twl<f, radix_list<16, 8>, 256, 32, 16, 1, 4, NT, 1>>(),        // 256
    pow2_entry<f, 256>(), pow2_entry<f, 512>(), pow2_entry<f, 1024>(),                         // 512, 1024, 2048
    pow2_entry<f, 2048>(), pow2_entry<f, 4096>(), pow2_entry<f, 8192>(),                       // 4096, 8192, 16384
    make_spec_entry_istft<wg_cfg<d, radix_list<2>, 256, 256, 0, 0, TW_GLOBAL, 2, NT, 1>>(),     // N = 4
    make_spec_entry_istft<wg_cfg<d, radix_list<4>, 256, 256, 4, 1, TW_GLOBAL, 2, NT, 1>>(),     // 8
    make_spec_entry_istft<wg_cfg<d, radix_list<8>, 256, 256, 8, 1, TW_GLOBAL, 2, NT, 1>>(),     // 16
    make_spec_entry_istft<wg_cfg<d, radix_list<16>, 256, 128, 16, 1, TW_GLOBAL, 2, NT, 1>>(),   // 32
    make_spec_entry_istft<wg_cfg_twl<d, radix_list<8, 4>, 256, 64, 8, 1, 2, NT, 1>>(),          // 64
    make_spec_entry_istft<wg_cfg_twl<d, radix_list<8, 8>, 256, 32, 8, 1, 2, NT, 1>>(),          // 128
    make_spec_entry_istft<wg_cfg_twl<d, radix_list<16, 8>, 256, 32, 16, 1, 2, NT, 1>>(),        // 256
    pow2_entry<d, 256>(), pow2_entry<d, 512>(), pow2_entry<d, 1024>(),                         // 512, 1024, 2048
    pow2_entry<d, 2048>(), pow2_entry<d, 4096>(),                                              // 4096, 8192
};
}  // namespace

const spec_kernel* istft_kernels(int* count) {
  *count = static_cast<int>(sizeof(g_istft) / sizeof(g_istft[0]));
  return g_istft;
}

}  // namespace pfa
