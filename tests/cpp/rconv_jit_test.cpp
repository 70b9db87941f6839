// The real convolution kernels (stockham_wg_rconv_kernel, stockham_wg_rconv.hpp) and the real overlap-save kernels
// (stockham_wg_rols_kernel, stockham_wg_rols.hpp) under the runtime compiler, without a GPU: the families are appended
// and their spelling is pinned against literals, and for half lengths M that are not powers of two, one fp32 and one
// fp64, and for one STAGED configuration (row windows in LDS) and one TW_REGS configuration, both modes of both
// families compile for gfx950 through hiprtc from the headers embedded in the library.
//   hipcc -std=c++17 tests/cpp/rconv_jit_test.cpp -L portfft_amd -lportfft_amd -o build/rconv_jit_test
#include <cstdio>
#include <cstring>
#include <string>

#include "../../portfft_amd/csrc/jit.hpp"
#include "../../include/portfft_amd.h"

int main() {
  int fails = 0;
  auto expect = [&](bool ok, const char* what) {
    if (!ok) {
      std::printf("FAIL %s\n", what);
      ++fails;
    }
  };
  // the spelling: one header per family, [0] the convolving and [1] the correlating kernel
  const pfa::jit_names rc = pfa::jit_instantiation(pfa::jit_form{pfa::JF_RCONV}, "CFG");
  expect(std::strcmp(rc.header, "stockham_wg_rconv.hpp") == 0, "rconv header");
  expect(rc.expr[0] == "pfa::stockham_wg_rconv_kernel<CFG, false>", "rconv convolve spelling");
  expect(rc.expr[1] == "pfa::stockham_wg_rconv_kernel<CFG, true>", "rconv correlate spelling");
  const pfa::jit_names ro = pfa::jit_instantiation(pfa::jit_form{pfa::JF_ROLS}, "CFG");
  expect(std::strcmp(ro.header, "stockham_wg_rols.hpp") == 0, "rols header");
  expect(ro.expr[0] == "pfa::stockham_wg_rols_kernel<CFG, false>", "rols convolve spelling");
  expect(ro.expr[1] == "pfa::stockham_wg_rols_kernel<CFG, true>", "rols correlate spelling");
  // (the neighbouring families keep their own, and the families in front of the new ones their values)
  expect(pfa::jit_instantiation(pfa::jit_form{pfa::JF_OLS}, "CFG").expr[0] == "pfa::stockham_wg_ols_kernel<CFG, false>", "ols spelling");
  expect(pfa::jit_instantiation(pfa::jit_form{pfa::JF_REAL}, "CFG").expr[0] == "pfa::stockham_wg_r2c_kernel<CFG>", "r2c spelling");
  static_assert(pfa::JF_CONV == 4 && pfa::JF_ND == 9 && pfa::JF_OLS == 10, "the earlier families keep their numbers");
  static_assert(pfa::JF_RCONV == 11 && pfa::JF_ROLS == 12, "the families are appended");

  const size_t max_lds = 160 * 1024;
  auto compile = [&](const char* what, const pfa::wg_params& p) {
    const std::string cfg = pfa::wg_cfg_type_name(p);
    const struct {
      pfa::jit_family family;
      const char* name;
    } families[] = {{pfa::JF_RCONV, "rconv"}, {pfa::JF_ROLS, "rols"}};
    for (const auto& f : families) {
      size_t bytes = 0;
      std::string why;
      const bool built = pfa::jit_compile_only(pfa::jit_form{f.family}, cfg, "gfx950", &bytes, &why);
      std::printf("hiprtc %s %s %s: %zu bytes %s\n", f.name, what, cfg.c_str(), bytes, built ? "" : why.c_str());
      if (!built || bytes < 1000) ++fails;
    }
  };
  struct {
    int precision;
    long long m;  // the half length: N = 2000 and N = 6000
  } planned[] = {{PFFT_PRECISION_F32, 1000}, {PFFT_PRECISION_F64, 3000}};
  for (const auto& c : planned) {
    pfa::wg_params p;
    if (!pfa::choose_spec_params(c.precision, c.m, max_lds, &p)) {
      std::printf("FAIL no plan for M=%lld\n", c.m);
      ++fails;
      continue;
    }
    compile(c.precision == PFFT_PRECISION_F32 ? "planned f32" : "planned f64", p);
  }
  {  // a STAGED single-pass configuration: the staged copies read the row windows from LDS
    pfa::wg_params p;
    p.precision = PFFT_PRECISION_F32;
    p.n = 12;
    p.radices = {12};
    p.wg = 240, p.fpw = 240, p.pads = 0, p.padw = 0, p.twm = 0, p.occ = 4, p.aux = 2, p.staged = 1, p.twl = 0;
    compile("staged", p);
  }
  {  // twiddles resident in registers (TW_REGS = 1)
    pfa::wg_params p;
    p.precision = PFFT_PRECISION_F32;
    p.n = 3375;
    p.radices = {15, 15, 15};
    p.wg = 225, p.fpw = 1, p.pads = 15, p.padw = 1, p.twm = 1, p.occ = 3, p.aux = 2, p.staged = 0, p.twl = 0;
    compile("tw_regs", p);
  }
  std::printf(fails == 0 ? "rconv jit OK\n" : "rconv jit FAILED\n");
  return fails == 0 ? 0 : 1;
}
