// The overlap-save filter kernels (stockham_wg_ols_kernel, stockham_wg_ols.hpp) under the runtime compiler, without a
// GPU: the family's spelling is pinned against literals, and for lengths that are not pre-compiled, one fp32 and one
// fp64, and for one STAGED configuration (row windows in LDS) and one TW_REGS configuration, both modes compile for
// gfx950 through hiprtc from the headers embedded in the library.
//   hipcc -std=c++17 tests/cpp/ols_jit_test.cpp -L portfft_amd -lportfft_amd -o build/ols_jit_test
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
  // the spelling: one header, [0] the convolving and [1] the correlating kernel
  const pfa::jit_names names = pfa::jit_instantiation(pfa::jit_form{pfa::JF_OLS}, "CFG");
  expect(std::strcmp(names.header, "stockham_wg_ols.hpp") == 0, "header");
  expect(names.expr[0] == "pfa::stockham_wg_ols_kernel<CFG, false>", "convolve spelling");
  expect(names.expr[1] == "pfa::stockham_wg_ols_kernel<CFG, true>", "correlate spelling");
  // (the neighbouring family keeps its own, and the families in front of the new one their values)
  expect(pfa::jit_instantiation(pfa::jit_form{pfa::JF_CONV}, "CFG").expr[0] == "pfa::stockham_wg_conv_kernel<CFG, false>", "conv spelling");
  static_assert(pfa::JF_CONV == 4 && pfa::JF_ND == 9 && pfa::JF_OLS == 10, "the family is appended");

  const size_t max_lds = 160 * 1024;
  auto compile = [&](const char* what, const pfa::wg_params& p) {
    size_t bytes = 0;
    std::string why;
    const std::string cfg = pfa::wg_cfg_type_name(p);
    const bool built = pfa::jit_compile_only(pfa::jit_form{pfa::JF_OLS}, cfg, "gfx950", &bytes, &why);
    std::printf("hiprtc ols %s %s: %zu bytes %s\n", what, cfg.c_str(), bytes, built ? "" : why.c_str());
    if (!built || bytes < 1000) ++fails;
  };
  struct {
    int precision;
    long long n;
  } planned[] = {{PFFT_PRECISION_F32, 1000}, {PFFT_PRECISION_F64, 3000}};
  for (const auto& c : planned) {
    pfa::wg_params p;
    if (!pfa::choose_spec_params(c.precision, c.n, max_lds, &p)) {
      std::printf("FAIL no plan for N=%lld\n", c.n);
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
  std::printf(fails == 0 ? "ols jit OK\n" : "ols jit FAILED\n");
  return fails == 0 ? 0 : 1;
}
