// The periodogram kernel (stockham_wg_periodogram_kernel, stockham_wg_periodogram.hpp) under the runtime compiler, without a
// GPU.  Relations only: the family is appended behind JF_IMDCT and the older numbers are what they were; the form is an
// OPEN form, at or behind N_SPEC_FORMS_END and in front of N_SPEC_FORMS_TOP, and cells() points into open_form; the
// spelling is one template with the extension as its trailing bool; the LDS rule is the STFT form's on the host mirror
// fused_lds_bytes_of; and for M = 3 (N = 6), M = 296 (N = 592), the half length of N = 2000 in fp32 and of N = 6000 in
// fp64 both kernels compile for gfx950 through hiprtc from the headers embedded in the library.
//   hipcc -std=c++17 tests/cpp/periodogram_jit_test.cpp -L portfft_amd -lportfft_amd -o build/periodogram_jit_test
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
  const pfa::jit_names st = pfa::jit_instantiation(pfa::jit_form{pfa::JF_PERIODOGRAM}, "CFG");
  expect(std::strcmp(st.header, "stockham_wg_periodogram.hpp") == 0, "periodogram header");
  expect(st.expr[0] == "pfa::stockham_wg_periodogram_kernel<CFG, false>", "zero-extension spelling");
  expect(st.expr[1] == "pfa::stockham_wg_periodogram_kernel<CFG, true>", "reflection spelling");
  expect(pfa::jit_instantiation(pfa::jit_form{pfa::JF_STFT}, "CFG").expr[1] == "pfa::stockham_wg_stft_kernel<CFG, true>", "stft spelling");
  expect(pfa::jit_instantiation(pfa::jit_form{pfa::JF_IMDCT}, "CFG").expr[0] == "pfa::stockham_wg_imdct_kernel<CFG>", "imdct spelling");
  static_assert(pfa::JF_STFT == 13 && pfa::JF_ISTFT == 14 && pfa::JF_DCT == 15 && pfa::JF_DCT4 == 16 && pfa::JF_IMDCT == 17,
                "the earlier families keep their numbers");
  static_assert(pfa::JF_PERIODOGRAM > pfa::JF_IMDCT, "the family is appended");
  static_assert(pfa::WF_ISTFT == 11 && pfa::N_SPEC_FORMS_ALL == 12 && pfa::WF_DCT == 12, "the pinned tables are what they were");
  // the open form: relations only
  static_assert(pfa::WF_DCT4 == pfa::N_SPEC_FORMS_END, "the first open form keeps its number");
  static_assert(pfa::WF_PERIODOGRAM >= pfa::N_SPEC_FORMS_END, "an open form");
  static_assert(pfa::WF_PERIODOGRAM > pfa::WF_IMDCT, "appended behind the open forms there were");
  static_assert(pfa::WF_PERIODOGRAM < pfa::N_SPEC_FORMS_TOP, "in front of the end of the open table");
  static_assert(pfa::N_OPEN_FORMS == pfa::N_SPEC_FORMS_TOP - pfa::N_SPEC_FORMS_END, "the open table's count follows from the enum");
  static_assert(sizeof(pfa::spec_kernel{}.open_form) == sizeof(pfa::kernel_fn) * 2 * pfa::N_OPEN_FORMS, "the open table holds every open form");
  {  // reached through cells()
    pfa::spec_kernel k{};
    expect(&k.cells(pfa::WF_PERIODOGRAM)[0] == &k.open_form[pfa::WF_PERIODOGRAM - pfa::N_SPEC_FORMS_END][0],
           "cells() of the form points at its own line of open_form");
    expect(&k.cells(pfa::WF_PERIODOGRAM)[1] == &k.cells(pfa::WF_PERIODOGRAM)[0] + 1, "... two cells");
    expect(&k.cells(pfa::WF_IMDCT)[0] == &k.open_form[pfa::WF_IMDCT - pfa::N_SPEC_FORMS_END][0], "cells() of the form in front of it");
    expect(&k.cells(pfa::WF_STFT)[0] != &k.cells(pfa::WF_PERIODOGRAM)[0], "... apart from the STFT's cells");
    const pfa::spec_kernel& ck = k;
    expect(&ck.cells(pfa::WF_PERIODOGRAM)[1] == &k.cells(pfa::WF_PERIODOGRAM)[1], "cells() const");
  }

  const size_t max_lds = 160 * 1024;
  auto compile = [&](const char* what, const pfa::wg_params& p) {
    const std::string cfg = pfa::wg_cfg_type_name(p);
    size_t bytes = 0;
    std::string why;
    const bool built = pfa::jit_compile_only(pfa::jit_form{pfa::JF_PERIODOGRAM}, cfg, "gfx950", &bytes, &why);
    std::printf("hiprtc periodogram %s %s: %zu bytes %s\n", what, cfg.c_str(), bytes, built ? "" : why.c_str());
    if (!built || bytes < 1000) ++fails;
  };
  struct {
    int precision;
    long long m;  // the half length: N = 6, 592, 2000 and 6000 (fp64)
  } planned[] = {{PFFT_PRECISION_F32, 3}, {PFFT_PRECISION_F32, 296}, {PFFT_PRECISION_F32, 1000}, {PFFT_PRECISION_F64, 3000}};
  for (const auto& c : planned) {
    pfa::wg_params p;
    if (!pfa::choose_spec_params(c.precision, c.m, max_lds, &p)) {
      std::printf("FAIL no plan for M=%lld\n", c.m);
      ++fails;
      continue;
    }
    compile(c.precision == PFFT_PRECISION_F32 ? "planned f32" : "planned f64", p);
    // the LDS rule: what the STFT form of the configuration takes (images, and row windows where the copy is staged)
    pfa::spec_kernel like{};  // (the fields fused_lds_bytes_of reads of an entry)
    like.precision = p.precision, like.n = p.n, like.wg = p.wg, like.fpw = p.fpw;
    like.n_radices = static_cast<int>(p.radices.size());
    for (int i = 0; i < like.n_radices; ++i) like.radices[i] = p.radices[static_cast<size_t>(i)];
    like.pads = p.pads, like.padw = p.padw, like.twm = p.twm, like.occ = p.occ, like.aux = p.aux;
    like.staged = p.staged, like.twl = p.twl;
    const size_t stft = pfa::fused_lds_bytes_of(pfa::JF_STFT, &like), pg = pfa::fused_lds_bytes_of(pfa::JF_PERIODOGRAM, &like);
    std::printf("lds M=%lld: stft %zu periodogram %zu\n", c.m, stft, pg);
    expect(pg == stft, "periodogram keeps the STFT form's LDS");
    expect(pg >= pfa::fused_lds_bytes_of(pfa::JF_REAL, &like), "... at least the real form's");
  }
  std::printf(fails == 0 ? "periodogram jit OK\n" : "periodogram jit FAILED\n");
  return fails == 0 ? 0 : 1;
}
