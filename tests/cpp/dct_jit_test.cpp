// The discrete cosine transform kernels (stockham_wg_dct_kernel, stockham_wg_dct.hpp) under the runtime compiler, without a
// GPU: the family is appended and its spelling is pinned against literals, the form is a LATE form -- numbered behind the
// pinned table, kept in spec_kernel::late_form and reached through spec_kernel::cells -- and for the half lengths M of
// N = 2000 and N = 12000 in fp32 and N = 6000 in fp64, the odd M of N = 30, and for one STAGED and one TW_REGS
// configuration, both types compile for gfx950 through hiprtc from the headers embedded in the library.
//   hipcc -std=c++17 tests/cpp/dct_jit_test.cpp -L portfft_amd -lportfft_amd -o build/dct_jit_test
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
  // the spelling: one header, [0] type 2 and [1] type 3
  const pfa::jit_names st = pfa::jit_instantiation(pfa::jit_form{pfa::JF_DCT}, "CFG");
  expect(std::strcmp(st.header, "stockham_wg_dct.hpp") == 0, "dct header");
  expect(st.expr[0] == "pfa::stockham_wg_dct_kernel<CFG, false>", "dct type 2 spelling");
  expect(st.expr[1] == "pfa::stockham_wg_dct_kernel<CFG, true>", "dct type 3 spelling");
  // (the neighbouring families keep their own, and the families in front of the new one their values)
  expect(pfa::jit_instantiation(pfa::jit_form{pfa::JF_ISTFT}, "CFG").expr[1] == "pfa::stockham_wg_istft_kernel<CFG, true>", "istft spelling");
  expect(pfa::jit_instantiation(pfa::jit_form{pfa::JF_REAL}, "CFG").expr[1] == "pfa::stockham_wg_c2r_kernel<CFG>", "c2r spelling");
  static_assert(pfa::JF_CONV == 4 && pfa::JF_ND == 9 && pfa::JF_OLS == 10 && pfa::JF_RCONV == 11 && pfa::JF_ROLS == 12,
                "the earlier families keep their numbers");
  static_assert(pfa::JF_STFT == 13 && pfa::JF_ISTFT == 14 && pfa::JF_DCT == 15, "the family is appended");
  static_assert(pfa::WF_ROLS == 9 && pfa::WF_STFT == 10 && pfa::N_SPEC_FORMS == 11, "the commit-time forms are what they were");
  static_assert(pfa::WF_ISTFT == 11 && pfa::N_SPEC_FORMS_ALL == 12, "... and the pinned table");
  static_assert(sizeof(pfa::spec_kernel{}.form) == sizeof(pfa::kernel_fn) * 2 * pfa::N_SPEC_FORMS_ALL, "... and its size");
  static_assert(pfa::WF_DCT == pfa::N_SPEC_FORMS_ALL && pfa::N_LATE_FORMS == 1 && pfa::N_SPEC_FORMS_END == 13,
                "the form is numbered behind the table");
  static_assert(sizeof(pfa::spec_kernel{}.late_form) == sizeof(pfa::kernel_fn) * 2 * pfa::N_LATE_FORMS, "a table of its own");
  {  // one accessor serves both tables
    pfa::spec_kernel k{};
    expect(&k.cells(pfa::WF_REAL)[0] == &k.form[pfa::WF_REAL][0], "cells() of a table form");
    expect(&k.cells(pfa::WF_ISTFT)[1] == &k.form[pfa::WF_ISTFT][1], "cells() of the last table form");
    expect(&k.cells(pfa::WF_DCT)[0] == &k.late_form[0][0] && &k.cells(pfa::WF_DCT)[1] == &k.late_form[0][1], "cells() of the late form");
    const pfa::spec_kernel& ck = k;
    expect(&ck.cells(pfa::WF_DCT)[1] == &k.late_form[0][1], "cells() const");
  }

  const size_t max_lds = 160 * 1024;
  auto compile = [&](const char* what, const pfa::wg_params& p) {
    const std::string cfg = pfa::wg_cfg_type_name(p);
    size_t bytes = 0;
    std::string why;
    const bool built = pfa::jit_compile_only(pfa::jit_form{pfa::JF_DCT}, cfg, "gfx950", &bytes, &why);
    std::printf("hiprtc dct %s %s: %zu bytes %s\n", what, cfg.c_str(), bytes, built ? "" : why.c_str());
    if (!built || bytes < 1000) ++fails;
  };
  struct {
    int precision;
    long long m;  // the half length: N = 2000, N = 12000, N = 6000 and N = 30
  } planned[] = {{PFFT_PRECISION_F32, 1000}, {PFFT_PRECISION_F32, 6000}, {PFFT_PRECISION_F64, 3000}, {PFFT_PRECISION_F32, 15}};
  for (const auto& c : planned) {
    pfa::wg_params p;
    if (!pfa::choose_spec_params(c.precision, c.m, max_lds, &p)) {
      std::printf("FAIL no plan for M=%lld\n", c.m);
      ++fails;
      continue;
    }
    compile(c.precision == PFFT_PRECISION_F32 ? "planned f32" : "planned f64", p);
  }
  {  // a STAGED single-pass configuration: 240 rows a group
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
  std::printf(fails == 0 ? "dct jit OK\n" : "dct jit FAILED\n");
  return fails == 0 ? 0 : 1;
}
