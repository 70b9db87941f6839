// The LDS-resident power-of-two configurations every fused form registers (kernels_real.hip, _conv, _ols, _rconv, _rols,
// _stft, _istft, _dct, _dct4, _imdct, _periodogram, _pairs): fp32 of 2 ... 8192 points and fp64 of 2 ... 4096, the lines of kernels_f32.hip / kernels_f64.hip
// for these lengths; 256 points and up read them from wg_pow2_cfg.hpp, which kernels_bluestein.hip shares.  One list: a
// retune of a line here retunes all twelve registries, and their order and contents are the list's
// (tests/test_gpu_fused_registry.py, test_gpu_dct4_registry.py, test_gpu_imdct_registry.py, test_gpu_periodogram_registry.py and test_gpu_pairs_registry.py run every line of every registry).
#pragma once
#include "kernels.hpp"
#include "wg_pow2_cfg.hpp"

namespace pfa {

/// one entry of the list: the wg_cfg and spec_kernel::groups_per_wg
template <typename Cfg, int GPW = 1>
struct fused_cfg {
  using cfg = Cfg;
  static constexpr int groups_per_wg = GPW;
};
template <typename T, int N>
using fused_pow2_cfg = fused_cfg<typename pow2_cfg<T, N>::cfg, pow2_cfg<T, N>::groups_per_wg>;

template <typename... E>
struct fused_cfg_list {
  static constexpr int count = sizeof...(E);
};

/// the configurations of 2 ... 128 points (T: the scalar; OCC; F16: the transforms per work-group at 16 points) and the
/// wg_pow2_cfg.hpp lines behind them
template <typename T, int OCC, int F16, typename... Pow2>
using fused_cfgs_of = fused_cfg_list<fused_cfg<wg_cfg<T, radix_list<2>, 256, 256, 0, 0, TW_GLOBAL, OCC, 2, 1>>,     // 2
                                     fused_cfg<wg_cfg<T, radix_list<4>, 256, 256, 4, 1, TW_GLOBAL, OCC, 2, 1>>,     // 4
                                     fused_cfg<wg_cfg<T, radix_list<8>, 256, 256, 8, 1, TW_GLOBAL, OCC, 2, 1>>,     // 8
                                     fused_cfg<wg_cfg<T, radix_list<16>, 256, F16, 16, 1, TW_GLOBAL, OCC, 2, 1>>,   // 16
                                     fused_cfg<wg_cfg_twl<T, radix_list<8, 4>, 256, 64, 8, 1, OCC, 2, 1>>,          // 32
                                     fused_cfg<wg_cfg_twl<T, radix_list<8, 8>, 256, 32, 8, 1, OCC, 2, 1>>,          // 64
                                     fused_cfg<wg_cfg_twl<T, radix_list<16, 8>, 256, 32, 16, 1, OCC, 2, 1>>,        // 128
                                     Pow2...>;
using fused_cfgs_f32 =
    fused_cfgs_of<float, 4, 256, fused_pow2_cfg<float, 256>, fused_pow2_cfg<float, 512>, fused_pow2_cfg<float, 1024>,
                  fused_pow2_cfg<float, 2048>, fused_pow2_cfg<float, 4096>, fused_pow2_cfg<float, 8192>>;
using fused_cfgs_f64 =
    fused_cfgs_of<double, 2, 128, fused_pow2_cfg<double, 256>, fused_pow2_cfg<double, 512>, fused_pow2_cfg<double, 1024>,
                  fused_pow2_cfg<double, 2048>, fused_pow2_cfg<double, 4096>>;

/// A registry of one fused form: make(fused_cfg<...>{}) -> spec_kernel for every line, the float list first.
struct fused_registry {
  static constexpr int count = fused_cfgs_f32::count + fused_cfgs_f64::count;
  spec_kernel k[count];
  template <typename Make>
  explicit fused_registry(Make make) {
    fill(make, 0, fused_cfgs_f32{});
    fill(make, fused_cfgs_f32::count, fused_cfgs_f64{});
  }
  const spec_kernel* entries(int* n) const {
    *n = count;
    return k;
  }

 private:
  template <typename Make, typename... E>
  void fill(Make& make, int at, fused_cfg_list<E...>) {
    ((k[at++] = make(E{})), ...);
  }
};

}  // namespace pfa
