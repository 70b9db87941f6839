// The real-data kernel forms (stockham_wg_r2c_kernel / stockham_wg_c2r_kernel, stockham_wg_real.hpp) under the runtime
// compiler, without a GPU: for half lengths that are not pre-compiled, one fp32 and one fp64, they compile for gfx950
// through hiprtc from the headers embedded in the library.
//   hipcc -std=c++17 tests/cpp/real_jit_test.cpp -L portfft_amd -lportfft_amd -o build/real_jit_test
#include <cstdio>
#include <string>

#include "../../portfft_amd/csrc/jit.hpp"
#include "../../include/portfft_amd.h"

int main() {
  int fails = 0;
  const size_t max_lds = 160 * 1024;
  struct {
    int precision;
    long long n;  // the real length; the kernels are those of M = n / 2 points
  } cases[] = {{PFFT_PRECISION_F32, 20000}, {PFFT_PRECISION_F64, 6000}, {PFFT_PRECISION_F32, 30}};
  for (const auto& c : cases) {
    pfa::wg_params p;
    if (!pfa::choose_spec_params(c.precision, c.n / 2, max_lds, &p)) {
      std::printf("FAIL no plan for M=%lld\n", c.n / 2);
      ++fails;
      continue;
    }
    size_t bytes = 0;
    std::string why;
    const bool built = pfa::jit_compile_only(pfa::jit_form{pfa::JF_REAL}, pfa::wg_cfg_type_name(p), "gfx950", &bytes, &why);
    std::printf("hiprtc real n=%lld %s: %zu bytes %s\n", c.n, pfa::wg_cfg_type_name(p).c_str(), bytes,
                built ? "" : why.c_str());
    if (!built || bytes < 1000) ++fails;
  }
  std::printf(fails == 0 ? "real jit OK\n" : "real jit FAILED\n");
  return fails == 0 ? 0 : 1;
}
