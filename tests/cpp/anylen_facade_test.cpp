// C++ user-code test of any-length transforms through the facade: portfft::amd::any_length_descriptor<float> and
// <double> -> commit -> forward against a double-precision DFT, backward round trip; a plain descriptor of the same
// length is still refused.
//   hipcc -std=c++17 -I include tests/cpp/anylen_facade_test.cpp -L portfft_amd -lportfft_amd -o build/anylen_facade_test
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

int host_checks() {
  using namespace portfft;
  amd::any_length_descriptor<float> desc({4093});
  desc.number_of_transforms = 3;
  REQUIRE(desc.forward_distance == 4093 && desc.backward_distance == 4093);
  REQUIRE(desc.get_input_count(direction::FORWARD) == 3 * 4093);
  REQUIRE(desc.get_output_count(direction::FORWARD) == 3 * 4093);
  static_assert(std::is_same_v<decltype(desc.commit(std::declval<queue&>())), committed_descriptor<float, domain::COMPLEX>>,
                "a COMPLEX plan");
  static_assert(PFFT_EXT_ANY_LENGTH == 2, "the extension bit");
  pfft_desc_t c = desc.c_descriptor();
  REQUIRE(c.extensions == PFFT_EXT_ANY_LENGTH && c.domain == PFFT_DOMAIN_COMPLEX && c.lengths[0] == 4093);
  REQUIRE(pfft_desc_validate(&c) == PFFT_OK);
  amd::any_length_descriptor<double> dd({2039});
  pfft_desc_t cd = dd.c_descriptor();
  REQUIRE(cd.extensions == PFFT_EXT_ANY_LENGTH && cd.precision == PFFT_PRECISION_F64);
  REQUIRE(pfft_desc_validate(&cd) == PFFT_OK);
  c.extensions = PFFT_EXT_ANY_LENGTH | PFFT_EXT_REAL_TRANSFORMS;
  REQUIRE(pfft_desc_validate(&c) == PFFT_INVALID_CONFIGURATION);
  REQUIRE(std::strstr(pfft_last_error(), "extension") != nullptr);
  c.extensions = 4;
  REQUIRE(pfft_desc_validate(&c) == PFFT_INVALID_CONFIGURATION);
  // rank 2 with such a length is refused by validate(), before any device is touched
  queue q;
  bool threw = false;
  try {
    amd::any_length_descriptor<float> nd({127, 4});
    nd.commit(q);
  } catch (const unsupported_configuration& e) {
    threw = std::strstr(e.what(), "1-D") != nullptr;
  }
  REQUIRE(threw);
  std::printf("anylen host checks OK\n");
  return 0;
}

template <typename T>
int device_checks(std::size_t n, std::size_t batch, double tol) {
  using namespace portfft;
  using C = std::complex<T>;
  std::vector<C> h(n * batch), r(n * batch), back(n * batch);
  for (std::size_t i = 0; i < h.size(); ++i) {
    h[i] = C(static_cast<T>(std::sin(0.37 * i + 0.1)), static_cast<T>(0.5 * std::cos(1.7 * i)));
  }
  C *din, *dout, *dback;
  REQUIRE(hipMalloc(&din, h.size() * sizeof(C)) == hipSuccess);
  REQUIRE(hipMalloc(&dout, h.size() * sizeof(C)) == hipSuccess);
  REQUIRE(hipMalloc(&dback, h.size() * sizeof(C)) == hipSuccess);
  REQUIRE(hipMemcpy(din, h.data(), h.size() * sizeof(C), hipMemcpyHostToDevice) == hipSuccess);
  hipStream_t stream;
  REQUIRE(hipStreamCreate(&stream) == hipSuccess);
  queue q(stream);
  amd::any_length_descriptor<T> desc({n});
  desc.number_of_transforms = batch;
  desc.backward_scale = static_cast<T>(1.0 / static_cast<double>(n));
  auto committed = desc.commit(q);
  committed.compute_forward(static_cast<const C*>(din), dout).wait();
  REQUIRE(hipMemcpy(r.data(), dout, r.size() * sizeof(C), hipMemcpyDeviceToHost) == hipSuccess);
  double worst = 0;
  for (std::size_t b = 0; b < batch; ++b) {
    double num = 0, den = 0;
    for (std::size_t k = 0; k < n; ++k) {
      std::complex<double> s = 0;
      for (std::size_t i = 0; i < n; ++i) {
        s += std::complex<double>(h[b * n + i]) * std::polar(1.0, -2 * M_PI * double((i * k) % n) / double(n));
      }
      num += std::norm(s - std::complex<double>(r[b * n + k]));
      den += std::norm(s);
    }
    worst = std::max(worst, std::sqrt(num / den));
  }
  std::printf("N=%zu batch=%zu %s forward rel-L2 %.3e\n", n, batch, sizeof(T) == 4 ? "f32" : "f64", worst);
  REQUIRE(worst < tol);
  committed.compute_backward(static_cast<const C*>(dout), dback).wait();
  REQUIRE(hipMemcpy(back.data(), dback, back.size() * sizeof(C), hipMemcpyDeviceToHost) == hipSuccess);
  double num = 0, den = 0;
  for (std::size_t i = 0; i < h.size(); ++i) {
    num += std::norm(std::complex<double>(back[i]) - std::complex<double>(h[i]));
    den += std::norm(std::complex<double>(h[i]));
  }
  std::printf("N=%zu batch=%zu round trip rel-L2 %.3e\n", n, batch, std::sqrt(num / den));
  REQUIRE(std::sqrt(num / den) < tol);
  // a plain descriptor keeps the refusal
  bool threw = false;
  try {
    descriptor<T, domain::COMPLEX> plain({n});
    plain.commit(q);
  } catch (const unsupported_configuration&) {
    threw = true;
  }
  REQUIRE(threw);
  (void)hipFree(din);
  (void)hipFree(dout);
  (void)hipFree(dback);
  (void)hipStreamDestroy(stream);
  return 0;
}

int main(int argc, char** argv) {
  if (host_checks() != 0) return 1;
  if (argc > 1 && std::strcmp(argv[1], "host") == 0) return 0;
  if (device_checks<float>(127, 3, 2e-6) != 0) return 1;
  if (device_checks<float>(4093, 2, 2e-6) != 0) return 1;
  if (device_checks<double>(2039, 2, 5e-15) != 0) return 1;
  std::printf("anylen facade OK\n");
  return 0;
}
