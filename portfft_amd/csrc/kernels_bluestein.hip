// Bluestein kernel instantiations for gfx950 (stockham_wg_bluestein.hpp): one entry per convolution length P, a power
// of two, with the wg_cfg line of the same length in kernels_real.hip (LDS-resident, no software pipeline; copies: a
// retune there belongs here too, and that file says so).  The
// transform length N is a runtime argument: the entry of P serves every N with P / 4 < N <= P / 2.  N needs a prime
// factor above 61 and so is at least 67: P = 256 ... 8192 in fp32 (N <= 4096), 256 ... 4096 in fp64 (N <= 2048).
#include "kernels_impl.hpp"
#include "stockham_wg_bluestein.hpp"

namespace pfa {

namespace {
template <typename Cfg>
bluestein_kernel make_entry(int groups_per_wg = 1) {
  bluestein_kernel k{};
  k.cfg = spec_entry_fields<Cfg>(groups_per_wg);
  k.lds_bytes = bluestein_lds_bytes<Cfg>();
  k.fn[0] = kernel_fn{reinterpret_cast<const void*>(&stockham_wg_bluestein_kernel<Cfg, false>), nullptr, false};
  k.fn[1] = kernel_fn{reinterpret_cast<const void*>(&stockham_wg_bluestein_kernel<Cfg, true>), nullptr, false};
  return k;
}

using f = float;
using d = double;
constexpr int NT = 2;
const bluestein_kernel g_bluestein[] = {
    make_entry<wg_cfg_twl<f, radix_list<16, 16>, 256, 16, 16, 1, 4, NT, 1>>(2),              // P = 256
    make_entry<wg_cfg<f, radix_list<8, 8, 8>, 256, 4, 16, 1, TW_GLOBAL, 4, NT, 0, 2>>(2),    // 512
    make_entry<wg_cfg<f, radix_list<16, 8, 8>, 256, 4, 16, 1, TW_GLOBAL, 4, NT, 0, 2>>(2),   // 1024
    make_entry<wg_cfg<f, radix_list<16, 16, 8>, 256, 2, 16, 1, TW_GLOBAL, 4, NT, 0, 2>>(4),  // 2048
    make_entry<wg_cfg<f, radix_list<16, 16, 16>, 256, 1, 16, 1, TW_REGS, 3, NT>>(4),         // 4096
    make_entry<wg_cfg<f, radix_list<32, 16, 16>, 256, 1, 16, 1, TW_REGS, 2, NT>>(4),         // 8192
    make_entry<wg_cfg_twl<d, radix_list<16, 16>, 256, 16, 16, 1, 2, NT>>(),                  // P = 256
    make_entry<wg_cfg_twl<d, radix_list<8, 8, 8>, 256, 4, 16, 1, 2, NT>>(),                  // 512
    make_entry<wg_cfg_twl<d, radix_list<16, 8, 8>, 256, 4, 16, 1, 2, NT>>(2),                // 1024
    make_entry<wg_cfg_twl<d, radix_list<16, 16, 8>, 256, 2, 16, 1, 2, NT>>(2),               // 2048
    make_entry<wg_cfg<d, radix_list<16, 16, 16>, 256, 1, 16, 1, TW_REGS, 1, NT>>(1),         // 4096
};
}  // namespace

const bluestein_kernel* bluestein_kernels(int* count) {
  *count = static_cast<int>(sizeof(g_bluestein) / sizeof(g_bluestein[0]));
  return g_bluestein;
}

}  // namespace pfa
