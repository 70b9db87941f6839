// The LDS-resident power-of-two configurations the fused registries (wg_fused_cfg.hpp: kernels_real.hip and the seven
// beside it) and the Bluestein registry (kernels_bluestein.hip, convolution length P) share: one wg_cfg and its grid rule per (scalar
// type, length), the lines of kernels_f32.hip / kernels_f64.hip for these lengths -- except fp32 4096, the headline
// entry's configuration without the software pipeline (a prefetching real or Bluestein form would be a second kernel to
// verify).  A retune of a line here retunes all of them.
#pragma once
#include "stockham_wg.hpp"

namespace pfa {

template <typename T, int N>
struct pow2_cfg;  // cfg: the wg_cfg of N points; groups_per_wg: spec_kernel::groups_per_wg

#define PFA_POW2_CFG(T, N, GPW, ...)              \
  template <>                                     \
  struct pow2_cfg<T, N> {                         \
    using cfg = __VA_ARGS__;                      \
    static constexpr int groups_per_wg = GPW;     \
  }
PFA_POW2_CFG(float, 256, 2, wg_cfg_twl<float, radix_list<16, 16>, 256, 16, 16, 1, 4, 2, 1>);
PFA_POW2_CFG(float, 512, 2, wg_cfg<float, radix_list<8, 8, 8>, 256, 4, 16, 1, TW_GLOBAL, 4, 2, 0, 2>);
PFA_POW2_CFG(float, 1024, 2, wg_cfg<float, radix_list<16, 8, 8>, 256, 4, 16, 1, TW_GLOBAL, 4, 2, 0, 2>);
PFA_POW2_CFG(float, 2048, 4, wg_cfg<float, radix_list<16, 16, 8>, 256, 2, 16, 1, TW_GLOBAL, 4, 2, 0, 2>);
PFA_POW2_CFG(float, 4096, 4, wg_cfg<float, radix_list<16, 16, 16>, 256, 1, 16, 1, TW_REGS, 3, 2>);
PFA_POW2_CFG(float, 8192, 4, wg_cfg<float, radix_list<32, 16, 16>, 256, 1, 16, 1, TW_REGS, 2, 2>);
PFA_POW2_CFG(double, 256, 1, wg_cfg_twl<double, radix_list<16, 16>, 256, 16, 16, 1, 2, 2>);
PFA_POW2_CFG(double, 512, 1, wg_cfg_twl<double, radix_list<8, 8, 8>, 256, 4, 16, 1, 2, 2>);
PFA_POW2_CFG(double, 1024, 2, wg_cfg_twl<double, radix_list<16, 8, 8>, 256, 4, 16, 1, 2, 2>);
PFA_POW2_CFG(double, 2048, 2, wg_cfg_twl<double, radix_list<16, 16, 8>, 256, 2, 16, 1, 2, 2>);
PFA_POW2_CFG(double, 4096, 1, wg_cfg<double, radix_list<16, 16, 16>, 256, 1, 16, 1, TW_REGS, 1, 2>);
#undef PFA_POW2_CFG

}  // namespace pfa
