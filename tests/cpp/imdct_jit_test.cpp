// The inverse MDCT kernel (stockham_wg_imdct_kernel, stockham_wg_imdct.hpp) under the runtime compiler, without a GPU: the
// family is appended (JF_IMDCT = 17, the older numbers unchanged) and its spelling is pinned against literals -- one
// kernel, spelled the same for both cells; the form is an OPEN form, numbered behind both pinned tables and reached through
// spec_kernel::cells, checked by relations only; the LDS rule, the real form's bytes and a carry of M scalars, on the host
// mirror fused_lds_bytes_of against the real and the dct4 family's; and for the half lengths M = 3 (N = 6)
// and M = 296 (N = 592), the half lengths of N = 2000 and 12000 in fp32 and of N = 6000 in fp64, and the odd M of N = 30,
// the kernel compiles for gfx950 through hiprtc from the headers embedded in the library.
//   hipcc -std=c++17 tests/cpp/imdct_jit_test.cpp -L portfft_amd -lportfft_amd -o build/imdct_jit_test
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
  // the spelling: one header, one kernel in both cells, no mode argument
  const pfa::jit_names st = pfa::jit_instantiation(pfa::jit_form{pfa::JF_IMDCT}, "CFG");
  expect(std::strcmp(st.header, "stockham_wg_imdct.hpp") == 0, "imdct header");
  expect(st.expr[0] == "pfa::stockham_wg_imdct_kernel<CFG>", "imdct spelling");
  expect(st.expr[1] == st.expr[0], "both cells are the one kernel");
  // (the neighbouring families keep their own, and the families in front of the new one their values)
  expect(pfa::jit_instantiation(pfa::jit_form{pfa::JF_DCT4}, "CFG").expr[1] == "pfa::stockham_wg_dct4_kernel<CFG, true>", "mdct spelling");
  expect(pfa::jit_instantiation(pfa::jit_form{pfa::JF_ISTFT}, "CFG").expr[1] == "pfa::stockham_wg_istft_kernel<CFG, true>", "istft spelling");
  static_assert(pfa::JF_CONV == 4 && pfa::JF_ND == 9 && pfa::JF_OLS == 10 && pfa::JF_RCONV == 11 && pfa::JF_ROLS == 12,
                "the earlier families keep their numbers");
  static_assert(pfa::JF_STFT == 13 && pfa::JF_ISTFT == 14 && pfa::JF_DCT == 15 && pfa::JF_DCT4 == 16, "... and the later ones");
  static_assert(pfa::JF_IMDCT == 17, "the family is appended");
  static_assert(pfa::WF_ISTFT == 11 && pfa::N_SPEC_FORMS_ALL == 12 && pfa::WF_DCT == 12, "the pinned tables are what they were");
  // the open form: relations only
  static_assert(pfa::WF_DCT4 == pfa::N_SPEC_FORMS_END, "the first open form keeps its number");
  static_assert(pfa::WF_IMDCT > pfa::WF_DCT4, "the form is appended behind the open forms there were");
  static_assert(pfa::WF_IMDCT < pfa::N_SPEC_FORMS_TOP, "... in front of the end of the open table");
  static_assert(pfa::N_OPEN_FORMS == pfa::N_SPEC_FORMS_TOP - pfa::N_SPEC_FORMS_END && pfa::N_OPEN_FORMS >= 2, "the open table's count follows from the enum");
  static_assert(sizeof(pfa::spec_kernel{}.open_form) == sizeof(pfa::kernel_fn) * 2 * pfa::N_OPEN_FORMS, "the open table holds every open form");
  {  // reached through cells()
    pfa::spec_kernel k{};
    expect(&k.cells(pfa::WF_IMDCT)[0] == &k.open_form[pfa::WF_IMDCT - pfa::N_SPEC_FORMS_END][0], "cells() of the form points at its own line of open_form");
    expect(&k.cells(pfa::WF_IMDCT)[1] == &k.cells(pfa::WF_IMDCT)[0] + 1, "... two cells");
    expect(&k.cells(pfa::WF_DCT4)[0] == &k.open_form[0][0], "cells() of the form in front of it");
    expect(&k.cells(pfa::WF_DCT)[1] == &k.late_form[0][1], "cells() of the late form");
    const pfa::spec_kernel& ck = k;
    expect(&ck.cells(pfa::WF_IMDCT)[1] == &k.cells(pfa::WF_IMDCT)[1], "cells() const");
  }

  const size_t max_lds = 160 * 1024;
  auto compile = [&](const char* what, const pfa::wg_params& p) {
    const std::string cfg = pfa::wg_cfg_type_name(p);
    size_t bytes = 0;
    std::string why;
    const bool built = pfa::jit_compile_only(pfa::jit_form{pfa::JF_IMDCT}, cfg, "gfx950", &bytes, &why);
    std::printf("hiprtc imdct %s %s: %zu bytes %s\n", what, cfg.c_str(), bytes, built ? "" : why.c_str());
    if (!built || bytes < 1000) ++fails;
  };
  struct {
    int precision;
    long long m;  // the half length: N = 6, 592, 2000, 12000, 6000 (fp64) and 30
  } planned[] = {{PFFT_PRECISION_F32, 3},    {PFFT_PRECISION_F32, 296},  {PFFT_PRECISION_F32, 1000},
                 {PFFT_PRECISION_F32, 6000}, {PFFT_PRECISION_F64, 3000}, {PFFT_PRECISION_F32, 15}};
  for (const auto& c : planned) {
    pfa::wg_params p;
    if (!pfa::choose_spec_params(c.precision, c.m, max_lds, &p)) {
      std::printf("FAIL no plan for M=%lld\n", c.m);
      ++fails;
      continue;
    }
    compile(c.precision == PFFT_PRECISION_F32 ? "planned f32" : "planned f64", p);
    // the LDS rule: what the real form of the configuration takes, and M scalars behind it
    pfa::spec_kernel like{};  // (the fields fused_lds_bytes_of reads of an entry)
    like.precision = p.precision, like.n = p.n, like.wg = p.wg, like.fpw = p.fpw;
    like.n_radices = static_cast<int>(p.radices.size());
    for (int i = 0; i < like.n_radices; ++i) like.radices[i] = p.radices[static_cast<size_t>(i)];
    like.pads = p.pads, like.padw = p.padw, like.twm = p.twm, like.occ = p.occ, like.aux = p.aux;
    like.staged = p.staged, like.twl = p.twl;
    const size_t sb = c.precision == PFFT_PRECISION_F64 ? 8 : 4;
    const size_t real = pfa::fused_lds_bytes_of(pfa::JF_REAL, &like), dct4 = pfa::fused_lds_bytes_of(pfa::JF_DCT4, &like);
    const size_t imdct = pfa::fused_lds_bytes_of(pfa::JF_IMDCT, &like);
    std::printf("lds M=%lld: real %zu dct4 %zu imdct %zu\n", c.m, real, dct4, imdct);
    expect(dct4 == real, "dct4 keeps the real form's LDS");
    expect(imdct == real + static_cast<size_t>(c.m) * sb, "imdct: the real form's LDS and a carry of M scalars");
  }
  std::printf(fails == 0 ? "imdct jit OK\n" : "imdct jit FAILED\n");
  return fails == 0 ? 0 : 1;
}
