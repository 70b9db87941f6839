// fp16 storage (PFFT_PRECISION_F16) kernel instantiations for gfx950: the power-of-two entries of kernels_f32.hip with
// the same wg_cfg -- fp32 arithmetic, LDS images and twiddles, fp16 only in HBM (stockham_wg.hpp: packed_io /
// packed_split_io with S = half_t).  Other lengths are specialised at commit time (jit.cpp) from the fp32 plan.
#include "kernels_impl.hpp"

namespace pfa {

namespace {
using f = float;
constexpr int NT = 2;
const spec_kernel g_spec_f16[] = {
    make_spec_entry_half<wg_cfg<f, radix_list<2>, 256, 256, 0, 0, TW_GLOBAL, 4, NT, 1>>(),                   // 2
    make_spec_entry_half<wg_cfg<f, radix_list<4>, 256, 256, 4, 1, TW_GLOBAL, 4, NT, 1>>(),                   // 4
    make_spec_entry_half<wg_cfg<f, radix_list<8>, 256, 256, 8, 1, TW_GLOBAL, 4, NT, 1>>(),                   // 8
    make_spec_entry_half<wg_cfg<f, radix_list<16>, 256, 256, 16, 1, TW_GLOBAL, 4, NT, 1>>(),                 // 16
    make_spec_entry_half<wg_cfg_twl<f, radix_list<8, 4>, 256, 64, 8, 1, 4, NT, 1>>(),                        // 32
    make_spec_entry_half<wg_cfg_twl<f, radix_list<8, 8>, 256, 32, 8, 1, 4, NT, 1>>(),                        // 64
    make_spec_entry_half<wg_cfg_twl<f, radix_list<16, 8>, 256, 32, 16, 1, 4, NT, 1>>(),                     // 128
    make_spec_entry_half<wg_cfg_twl<f, radix_list<16, 16>, 256, 16, 16, 1, 4, NT, 1>>(2),                   // 256
    make_spec_entry_half<wg_cfg<f, radix_list<8, 8, 8>, 256, 4, 16, 1, TW_GLOBAL, 4, NT, 0, 2>>(2),          // 512
    make_spec_entry_half<wg_cfg<f, radix_list<16, 8, 8>, 256, 4, 16, 1, TW_GLOBAL, 4, NT, 0, 2>>(2),         // 1024
    make_spec_entry_half<wg_cfg<f, radix_list<16, 16, 8>, 256, 2, 16, 1, TW_GLOBAL, 4, NT, 0, 2>>(4),        // 2048
    make_spec_entry_prefetch_half<wg_cfg<f, radix_list<16, 16, 16>, 256, 1, 16, 1, TW_REGS, 3, NT>>(4),      // 4096
    make_spec_entry_half<wg_cfg<f, radix_list<32, 16, 16>, 256, 1, 16, 1, TW_REGS, 2, NT>>(4),               // 8192
    make_spec_entry_hx_half<wg_cfg<f, radix_list<32, 32, 16>, 512, 1, 32, 1, TW_GLOBAL, 4, NT, 0, 1>>(1),    // 16384
    make_spec_entry_hx_half<wg_cfg<f, radix_list<32, 32, 32>, 1024, 1, 32, 1, TW_GLOBAL, 4, NT, 0, 1>>(4),   // 32768
};
}  // namespace

const spec_kernel* spec_kernels_f16(int* count) {
  *count = static_cast<int>(sizeof(g_spec_f16) / sizeof(g_spec_f16[0]));
  return g_spec_f16;
}

}  // namespace pfa
