// Real-data kernel instantiations for gfx950 (stockham_wg_real.hpp): R2C / C2R of N = 2 * M for the LDS-resident
// power-of-two entries of kernels_f32.hip (M = 2 ... 8192) and kernels_f64.hip (M = 2 ... 4096), with those files' own
// wg_cfg lines.  fp32 M = 4096 is the headline entry's configuration without the software pipeline (a prefetching real
// form would be a second kernel to verify).  Other lengths are specialised at commit time (jit.cpp: jit_real_kernel).
// kernels_bluestein.hip repeats the lines of M = 256 ... 8192 (fp64: ... 4096) for its convolution lengths: a retune of
// one of them here belongs there too.
#include "kernels_impl.hpp"

namespace pfa {

namespace {
using f = float;
using d = double;
constexpr int NT = 2;
const real_kernel g_real[] = {
    make_spec_entry_real<wg_cfg<f, radix_list<2>, 256, 256, 0, 0, TW_GLOBAL, 4, NT, 1>>(),                  // N = 4
    make_spec_entry_real<wg_cfg<f, radix_list<4>, 256, 256, 4, 1, TW_GLOBAL, 4, NT, 1>>(),                  // 8
    make_spec_entry_real<wg_cfg<f, radix_list<8>, 256, 256, 8, 1, TW_GLOBAL, 4, NT, 1>>(),                  // 16
    make_spec_entry_real<wg_cfg<f, radix_list<16>, 256, 256, 16, 1, TW_GLOBAL, 4, NT, 1>>(),                // 32
    make_spec_entry_real<wg_cfg_twl<f, radix_list<8, 4>, 256, 64, 8, 1, 4, NT, 1>>(),                       // 64
    make_spec_entry_real<wg_cfg_twl<f, radix_list<8, 8>, 256, 32, 8, 1, 4, NT, 1>>(),                       // 128
    make_spec_entry_real<wg_cfg_twl<f, radix_list<16, 8>, 256, 32, 16, 1, 4, NT, 1>>(),                     // 256
    make_spec_entry_real<wg_cfg_twl<f, radix_list<16, 16>, 256, 16, 16, 1, 4, NT, 1>>(2),                   // 512
    make_spec_entry_real<wg_cfg<f, radix_list<8, 8, 8>, 256, 4, 16, 1, TW_GLOBAL, 4, NT, 0, 2>>(2),         // 1024
    make_spec_entry_real<wg_cfg<f, radix_list<16, 8, 8>, 256, 4, 16, 1, TW_GLOBAL, 4, NT, 0, 2>>(2),        // 2048
    make_spec_entry_real<wg_cfg<f, radix_list<16, 16, 8>, 256, 2, 16, 1, TW_GLOBAL, 4, NT, 0, 2>>(4),       // 4096
    make_spec_entry_real<wg_cfg<f, radix_list<16, 16, 16>, 256, 1, 16, 1, TW_REGS, 3, NT>>(4),              // 8192
    make_spec_entry_real<wg_cfg<f, radix_list<32, 16, 16>, 256, 1, 16, 1, TW_REGS, 2, NT>>(4),              // 16384
    make_spec_entry_real<wg_cfg<d, radix_list<2>, 256, 256, 0, 0, TW_GLOBAL, 2, NT, 1>>(),                  // N = 4
    make_spec_entry_real<wg_cfg<d, radix_list<4>, 256, 256, 4, 1, TW_GLOBAL, 2, NT, 1>>(),                  // 8
    make_spec_entry_real<wg_cfg<d, radix_list<8>, 256, 256, 8, 1, TW_GLOBAL, 2, NT, 1>>(),                  // 16
    make_spec_entry_real<wg_cfg<d, radix_list<16>, 256, 128, 16, 1, TW_GLOBAL, 2, NT, 1>>(),                // 32
    make_spec_entry_real<wg_cfg_twl<d, radix_list<8, 4>, 256, 64, 8, 1, 2, NT, 1>>(),                       // 64
    make_spec_entry_real<wg_cfg_twl<d, radix_list<8, 8>, 256, 32, 8, 1, 2, NT, 1>>(),                       // 128
    make_spec_entry_real<wg_cfg_twl<d, radix_list<16, 8>, 256, 32, 16, 1, 2, NT, 1>>(),                     // 256
    make_spec_entry_real<wg_cfg_twl<d, radix_list<16, 16>, 256, 16, 16, 1, 2, NT>>(),                       // 512
    make_spec_entry_real<wg_cfg_twl<d, radix_list<8, 8, 8>, 256, 4, 16, 1, 2, NT>>(),                       // 1024
    make_spec_entry_real<wg_cfg_twl<d, radix_list<16, 8, 8>, 256, 4, 16, 1, 2, NT>>(2),                     // 2048
    make_spec_entry_real<wg_cfg_twl<d, radix_list<16, 16, 8>, 256, 2, 16, 1, 2, NT>>(2),                    // 4096
    make_spec_entry_real<wg_cfg<d, radix_list<16, 16, 16>, 256, 1, 16, 1, TW_REGS, 1, NT>>(1),              // 8192
};
}  // namespace

const real_kernel* real_kernels(int* count) {
  *count = static_cast<int>(sizeof(g_real) / sizeof(g_real[0]));
  return g_real;
}

}  // namespace pfa
