// C++ user-code test of the facade with fp16 storage: descriptor<_Float16, domain::COMPLEX> -> commit -> forward and
// backward, against a double-precision DFT of the same (fp16) input.
//   hipcc -std=c++17 -I include tests/cpp/half_facade_test.cpp -L portfft_amd -lportfft_amd -o build/half_facade_test
// With argument "host" only the host-side checks run (no GPU needed).
#include <hip/hip_runtime.h>

#include <cmath>
#include <complex>
#include <cstdio>
#include <cstring>
#include <type_traits>
#include <vector>

#include <portfft/portfft.hpp>

#define REQUIRE(c)                                               \
  do {                                                           \
    if (!(c)) {                                                  \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
      return 1;                                                  \
    }                                                            \
  } while (0)

using half = _Float16;
using chalf = std::complex<half>;

int host_checks() {
  using namespace portfft;
  static_assert(sizeof(chalf) == 4, "two binary16 values per complex element");
  static_assert(std::is_same_v<descriptor<half, domain::COMPLEX>::scale_type, float>, "fp32 scales");
  static_assert(std::is_same_v<committed_descriptor<half, domain::COMPLEX>::complex_type, chalf>, "complex<_Float16>");
  descriptor<half, domain::COMPLEX> desc({24000});
  desc.forward_scale = 1.0f / 24000;
  REQUIRE(desc.get_scale(direction::FORWARD) == 1.0f / 24000);
  REQUIRE(desc.get_input_count(direction::FORWARD) == 24000);
  queue q;
  bool threw = false;
  try {
    descriptor<half, domain::COMPLEX> nd({64, 64});
    nd.commit(q);
  } catch (const unsupported_configuration&) {
    threw = true;
  }
  REQUIRE(threw);
  threw = false;
  try {
    descriptor<half, domain::REAL> real({64});
    real.commit(q);
  } catch (const unsupported_configuration&) {
    threw = true;
  }
  REQUIRE(threw);
  std::printf("half host checks OK\n");
  return 0;
}

int device_checks(std::size_t n, std::size_t batch) {
  using namespace portfft;
  std::vector<chalf> h(n * batch), r(n * batch);
  for (std::size_t i = 0; i < h.size(); ++i) {
    h[i] = chalf(static_cast<half>(std::sin(0.37 * i + 0.1)), static_cast<half>(std::cos(1.7 * i + 0.3)));
  }
  chalf *din, *dout;
  REQUIRE(hipMalloc(&din, h.size() * sizeof(chalf)) == hipSuccess);
  REQUIRE(hipMalloc(&dout, h.size() * sizeof(chalf)) == hipSuccess);
  REQUIRE(hipMemcpy(din, h.data(), h.size() * sizeof(chalf), hipMemcpyHostToDevice) == hipSuccess);
  hipStream_t stream;
  REQUIRE(hipStreamCreate(&stream) == hipSuccess);
  queue q(stream);
  descriptor<half, domain::COMPLEX> desc({n});
  desc.number_of_transforms = batch;
  desc.backward_scale = 1.0f / static_cast<float>(n);
  auto committed = desc.commit(q);
  committed.compute_forward(din, dout).wait();
  REQUIRE(hipMemcpy(r.data(), dout, r.size() * sizeof(chalf), hipMemcpyDeviceToHost) == hipSuccess);
  auto wide = [](chalf x) { return std::complex<double>(static_cast<double>(x.real()), static_cast<double>(x.imag())); };
  double worst = 0;
  for (std::size_t b = 0; b < batch; ++b) {
    double num = 0, den = 0;
    for (std::size_t k = 0; k < n; ++k) {
      std::complex<double> s = 0;
      for (std::size_t i = 0; i < n; ++i) {
        s += wide(h[b * n + i]) * std::polar(1.0, -2 * M_PI * double((i * k) % n) / double(n));
      }
      num += std::norm(s - wide(r[b * n + k]));
      den += std::norm(s);
    }
    worst = std::max(worst, std::sqrt(num / den));
  }
  std::printf("N=%zu batch=%zu f16 forward rel-L2 %.3e\n", n, batch, worst);
  REQUIRE(worst < 6e-4);  // fp16 output rounding: about 2e-4
  // in-place backward with backward_scale = 1/N returns the input (two fp16 roundings)
  committed.compute_backward(dout).wait();
  REQUIRE(hipMemcpy(r.data(), dout, r.size() * sizeof(chalf), hipMemcpyDeviceToHost) == hipSuccess);
  double num = 0, den = 0;
  for (std::size_t i = 0; i < h.size(); ++i) {
    num += std::norm(wide(r[i]) - wide(h[i]));
    den += std::norm(wide(h[i]));
  }
  std::printf("N=%zu batch=%zu f16 round trip rel-L2 %.3e\n", n, batch, std::sqrt(num / den));
  REQUIRE(std::sqrt(num / den) < 1e-3);
  (void)hipFree(din);
  (void)hipFree(dout);
  (void)hipStreamDestroy(stream);
  return 0;
}

int main(int argc, char** argv) {
  if (host_checks() != 0) return 1;
  if (argc > 1 && std::strcmp(argv[1], "host") == 0) return 0;
  if (device_checks(64, 3) != 0) return 1;
  if (device_checks(4096, 2) != 0) return 1;
  std::printf("half facade OK\n");
  return 0;
}
