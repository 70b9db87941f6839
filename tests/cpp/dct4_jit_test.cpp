// The DCT-IV / MDCT kernels (stockham_wg_dct4_kernel, stockham_wg_dct4.hpp) under the runtime compiler, without a GPU: the
// family is appended and its spelling is pinned against literals, the form is an OPEN form -- numbered behind both pinned
// tables, kept in spec_kernel::open_form and reached through spec_kernel::cells, checked by relations only so that the
// next verb can append a line -- and for the half lengths M of N = 2000 and N = 12000 in fp32 and N = 6000 in fp64, the
// odd M of N = 30, and for one STAGED and one TW_REGS configuration, both cells compile for gfx950 through hiprtc from the
// headers embedded in the library.
//   hipcc -std=c++17 tests/cpp/dct4_jit_test.cpp -L portfft_amd -lportfft_amd -o build/dct4_jit_test
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
  // the spelling: one header, [0] rows and [1] MDCT
  const pfa::jit_names st = pfa::jit_instantiation(pfa::jit_form{pfa::JF_DCT4}, "CFG");
  expect(std::strcmp(st.header, "stockham_wg_dct4.hpp") == 0, "dct4 header");
  expect(st.expr[0] == "pfa::stockham_wg_dct4_kernel<CFG, false>", "dct4 rows spelling");
  expect(st.expr[1] == "pfa::stockham_wg_dct4_kernel<CFG, true>", "mdct spelling");
  // (the neighbouring families keep their own, and the families in front of the new one their values)
  expect(pfa::jit_instantiation(pfa::jit_form{pfa::JF_DCT}, "CFG").expr[1] == "pfa::stockham_wg_dct_kernel<CFG, true>", "dct spelling");
  expect(pfa::jit_instantiation(pfa::jit_form{pfa::JF_REAL}, "CFG").expr[1] == "pfa::stockham_wg_c2r_kernel<CFG>", "c2r spelling");
  static_assert(pfa::JF_CONV == 4 && pfa::JF_ND == 9 && pfa::JF_OLS == 10 && pfa::JF_RCONV == 11 && pfa::JF_ROLS == 12,
                "the earlier families keep their numbers");
  static_assert(pfa::JF_STFT == 13 && pfa::JF_ISTFT == 14 && pfa::JF_DCT == 15 && pfa::JF_DCT4 == 16, "the family is appended");
  static_assert(pfa::WF_ISTFT == 11 && pfa::N_SPEC_FORMS_ALL == 12 && pfa::WF_DCT == 12, "the pinned tables are what they were");
  // the open form: relations only
  static_assert(pfa::WF_DCT4 >= pfa::N_SPEC_FORMS_END, "the form is numbered behind the late table");
  static_assert(pfa::WF_DCT4 < pfa::N_SPEC_FORMS_TOP, "... and in front of the end of the open one");
  static_assert(pfa::N_OPEN_FORMS == pfa::N_SPEC_FORMS_TOP - pfa::N_SPEC_FORMS_END && pfa::N_OPEN_FORMS >= 1, "the open table's count follows from the enum");
  static_assert(sizeof(pfa::spec_kernel{}.open_form) == sizeof(pfa::kernel_fn) * 2 * pfa::N_OPEN_FORMS, "a table of its own");
  {  // one accessor serves the three tables
    pfa::spec_kernel k{};
    const char* lo = reinterpret_cast<const char*>(&k.open_form[0][0]);
    const char* hi = lo + sizeof(k.open_form);
    const char* c0 = reinterpret_cast<const char*>(&k.cells(pfa::WF_DCT4)[0]);
    const char* c1 = reinterpret_cast<const char*>(&k.cells(pfa::WF_DCT4)[1]);
    expect(c0 >= lo && c1 < hi && c1 == c0 + sizeof(pfa::kernel_fn), "cells() of the open form points into open_form");
    expect(&k.cells(pfa::WF_DCT4)[0] == &k.open_form[pfa::WF_DCT4 - pfa::N_SPEC_FORMS_END][0], "... at its own line");
    expect(&k.cells(pfa::WF_REAL)[0] == &k.form[pfa::WF_REAL][0], "cells() of a table form");
    expect(&k.cells(pfa::WF_DCT)[1] == &k.late_form[0][1], "cells() of the late form");
    const pfa::spec_kernel& ck = k;
    expect(reinterpret_cast<const char*>(&ck.cells(pfa::WF_DCT4)[1]) == c1, "cells() const");
  }

  const size_t max_lds = 160 * 1024;
  auto compile = [&](const char* what, const pfa::wg_params& p) {
    const std::string cfg = pfa::wg_cfg_type_name(p);
    size_t bytes = 0;
    std::string why;
    const bool built = pfa::jit_compile_only(pfa::jit_form{pfa::JF_DCT4}, cfg, "gfx950", &bytes, &why);
    std::printf("hiprtc dct4 %s %s: %zu bytes %s\n", what, cfg.c_str(), bytes, built ? "" : why.c_str());
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
  std::printf(fails == 0 ? "dct4 jit OK\n" : "dct4 jit FAILED\n");
  return fails == 0 ? 0 : 1;
}
