// The pair kernel (stockham_wg_pairs_kernel, stockham_wg_pairs.hpp) under the runtime compiler, without a GPU.  Relations
// only: the family is appended behind JF_PERIODOGRAM and the older numbers are what they were; the form is an OPEN form, at
// or behind N_SPEC_FORMS_END and in front of N_SPEC_FORMS_TOP, and cells() points into open_form; the row of the family
// table exists and spells one template with the conjugate as its trailing bool; the LDS rule on the host mirror
// fused_lds_bytes_of is the real form's plus a second image set (the real form's without its twiddle copy) plus two
// windows per row where the copies are staged; and for M = 3 (N = 6), M = 296 (N = 592), the half length of N = 2000 in
// fp32 and of N = 6000 in fp64 both kernels compile for gfx950 through hiprtc from the headers embedded in the library.
//   hipcc -std=c++17 tests/cpp/pairs_jit_test.cpp -L portfft_amd -lportfft_amd -o build/pairs_jit_test
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
  const pfa::jit_names st = pfa::jit_instantiation(pfa::jit_form{pfa::JF_PAIRS}, "CFG");
  expect(std::strcmp(st.header, "stockham_wg_pairs.hpp") == 0, "pairs header");
  expect(st.expr[0] == "pfa::stockham_wg_pairs_kernel<CFG, false>", "product spelling");
  expect(st.expr[1] == "pfa::stockham_wg_pairs_kernel<CFG, true>", "conjugate product spelling");
  expect(pfa::jit_instantiation(pfa::jit_form{pfa::JF_PERIODOGRAM}, "CFG").expr[1] == "pfa::stockham_wg_periodogram_kernel<CFG, true>",
         "periodogram spelling");
  static_assert(pfa::JF_STFT == 13 && pfa::JF_ISTFT == 14 && pfa::JF_DCT == 15 && pfa::JF_DCT4 == 16 && pfa::JF_IMDCT == 17,
                "the earlier families keep their numbers");
  static_assert(pfa::JF_PAIRS > pfa::JF_PERIODOGRAM && pfa::JF_PERIODOGRAM > pfa::JF_IMDCT, "the family is appended");
  static_assert(pfa::WF_ISTFT == 11 && pfa::N_SPEC_FORMS_ALL == 12 && pfa::WF_DCT == 12, "the pinned tables are what they were");
  // the open form: relations only
  static_assert(pfa::WF_DCT4 == pfa::N_SPEC_FORMS_END, "the first open form keeps its number");
  static_assert(pfa::WF_PAIRS >= pfa::N_SPEC_FORMS_END, "an open form");
  static_assert(pfa::WF_PAIRS > pfa::WF_PERIODOGRAM && pfa::WF_PERIODOGRAM > pfa::WF_IMDCT, "appended behind the open forms there were");
  static_assert(pfa::WF_PAIRS < pfa::N_SPEC_FORMS_TOP, "in front of the end of the open table");
  static_assert(pfa::N_OPEN_FORMS == pfa::N_SPEC_FORMS_TOP - pfa::N_SPEC_FORMS_END, "the open table's count follows from the enum");
  static_assert(sizeof(pfa::spec_kernel{}.open_form) == sizeof(pfa::kernel_fn) * 2 * pfa::N_OPEN_FORMS, "the open table holds every open form");
  {  // reached through cells()
    pfa::spec_kernel k{};
    expect(&k.cells(pfa::WF_PAIRS)[0] == &k.open_form[pfa::WF_PAIRS - pfa::N_SPEC_FORMS_END][0],
           "cells() of the form points at its own line of open_form");
    expect(&k.cells(pfa::WF_PAIRS)[1] == &k.cells(pfa::WF_PAIRS)[0] + 1, "... two cells");
    expect(&k.cells(pfa::WF_PERIODOGRAM)[0] == &k.open_form[pfa::WF_PERIODOGRAM - pfa::N_SPEC_FORMS_END][0], "cells() of the form in front of it");
    expect(&k.cells(pfa::WF_RCONV)[0] != &k.cells(pfa::WF_PAIRS)[0], "... apart from the real convolution's cells");
    const pfa::spec_kernel& ck = k;
    expect(&ck.cells(pfa::WF_PAIRS)[1] == &k.cells(pfa::WF_PAIRS)[1], "cells() const");
  }

  const size_t max_lds = 160 * 1024;
  auto compile = [&](const char* what, const pfa::wg_params& p) {
    const std::string cfg = pfa::wg_cfg_type_name(p);
    size_t bytes = 0;
    std::string why;
    const bool built = pfa::jit_compile_only(pfa::jit_form{pfa::JF_PAIRS}, cfg, "gfx950", &bytes, &why);
    std::printf("hiprtc pairs %s %s: %zu bytes %s\n", what, cfg.c_str(), bytes, built ? "" : why.c_str());
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
    // the LDS rule: the real form's, the images once more, two windows of 16 bytes per row where the copies are staged
    pfa::spec_kernel like{};  // (the fields fused_lds_bytes_of reads of an entry)
    like.precision = p.precision, like.n = p.n, like.wg = p.wg, like.fpw = p.fpw;
    like.n_radices = static_cast<int>(p.radices.size());
    for (int i = 0; i < like.n_radices; ++i) like.radices[i] = p.radices[static_cast<size_t>(i)];
    like.pads = p.pads, like.padw = p.padw, like.twm = p.twm, like.occ = p.occ, like.aux = p.aux;
    like.staged = p.staged, like.twl = p.twl;
    pfa::wg_params images = p;  // the image set alone: an image also for a single pass, no twiddle copy behind it
    images.staged = 1;
    images.twl = 0;
    const size_t real = pfa::fused_lds_bytes_of(pfa::JF_REAL, &like), pairs = pfa::fused_lds_bytes_of(pfa::JF_PAIRS, &like);
    const size_t set = pfa::spec_lds_bytes(images), rows = p.staged != 0 ? 2 * static_cast<size_t>(p.fpw) * 16 : 0;
    std::printf("lds M=%lld: real %zu image set %zu windows %zu pairs %zu\n", c.m, real, set, rows, pairs);
    expect(pairs == real + set + rows, "pairs: the real form's LDS, a second image set and the windows");
    expect(set >= static_cast<size_t>(c.m) * static_cast<size_t>(p.fpw) * (c.precision == PFFT_PRECISION_F64 ? 16 : 8),
           "an image set holds fpw rows of M complex elements");
    expect(set <= real, "... and no more than the real form's LDS");
  }
  std::printf(fails == 0 ? "pairs jit OK\n" : "pairs jit FAILED\n");
  return fails == 0 ? 0 : 1;
}
