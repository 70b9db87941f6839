// fp16 storage under the runtime compiler, without a GPU: the converting forms (stockham_wg_half_*, stockham_wg_hx_half_*)
// of fp32 plans compile for gfx950 through hiprtc from the headers embedded in the library -- a registered length, a
// length only hiprtc serves, and a register-resident one.
//   hipcc -std=c++17 tests/cpp/half_jit_test.cpp -L portfft_amd -lportfft_amd -o build/half_jit_test
#include <cstdio>
#include <string>

#include "../../portfft_amd/csrc/jit.hpp"
#include "../../include/portfft_amd.h"

int main() {
  int fails = 0;
  const size_t max_lds = 160 * 1024;
  struct {
    long long n;
    pfa::jit_form form;  // {family, split, half}
  } cases[] = {{4096, {pfa::JF_PACKED, false, true}}, {10000, {pfa::JF_PACKED, true, true}}, {24000, {pfa::JF_PACKED_HX, false, true}}};
  for (const auto& c : cases) {
    pfa::wg_params p;
    // fp16 storage is planned as fp32
    const bool planned = c.form.family == pfa::JF_PACKED_HX ? pfa::choose_hx_params(PFFT_PRECISION_F32, c.n, max_lds, &p)
                                      : pfa::choose_spec_params(PFFT_PRECISION_F32, c.n, max_lds, &p);
    if (!planned) {
      std::printf("FAIL no fp32 plan for n=%lld\n", c.n);
      ++fails;
      continue;
    }
    size_t bytes = 0;
    std::string why;
    const bool built = pfa::jit_compile_only(c.form, pfa::wg_cfg_type_name(p), "gfx950", &bytes, &why);
    std::printf("hiprtc half n=%lld %s %s: %zu bytes %s\n", c.n, pfa::jit_instantiation(c.form, "CFG").expr[0].c_str(), pfa::wg_cfg_type_name(p).c_str(), bytes,
                built ? "" : why.c_str());
    if (!built || bytes < 1000) ++fails;
  }
  std::printf(fails == 0 ? "half jit OK\n" : "half jit FAILED\n");
  return fails == 0 ? 0 : 1;
}
