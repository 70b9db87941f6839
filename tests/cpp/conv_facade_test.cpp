// C++ user-code test of the fused convolution through the facade: portfft::amd::convolution_descriptor<float> and
// <double> -> commit -> the filter spectrum made with the same plan's compute_forward -> set_filter -> convolve and
// correlate against a double-precision circular convolution.
//   hipcc -std=c++17 -I include tests/cpp/conv_facade_test.cpp -L portfft_amd -lportfft_amd -o build/conv_facade_test
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
  amd::convolution_descriptor<float> desc({1000});
  desc.number_of_transforms = 3;
  REQUIRE(desc.forward_distance == 1000 && desc.backward_distance == 1000);
  REQUIRE(desc.get_input_count(direction::FORWARD) == 3 * 1000);
  REQUIRE(desc.get_output_count(direction::FORWARD) == 3 * 1000);
  using committed = decltype(desc.commit(std::declval<queue&>()));
  static_assert(std::is_same_v<committed, committed_descriptor<float, domain::COMPLEX>>, "a COMPLEX plan");
  static_assert(PFFT_EXT_CONVOLUTION == 8, "the extension bit");
  static_assert(PFFT_CONVOLVE == 0 && PFFT_CORRELATE == 1, "the modes");
  using C = std::complex<float>;
  static_assert(std::is_same_v<decltype(std::declval<committed&>().convolve(std::declval<const C*>(), std::declval<C*>())), event>,
                "out of place");
  static_assert(std::is_same_v<decltype(std::declval<committed&>().correlate(std::declval<C*>(), std::vector<event>{})), event>,
                "in place, with dependencies");
  static_assert(std::is_same_v<decltype(std::declval<committed&>().set_filter(std::declval<const C*>(), std::size_t{3})), void>,
                "the filter");
  pfft_desc_t c = desc.c_descriptor();
  REQUIRE(c.extensions == PFFT_EXT_CONVOLUTION && c.domain == PFFT_DOMAIN_COMPLEX && c.lengths[0] == 1000);
  REQUIRE(pfft_desc_validate(&c) == PFFT_OK);
  amd::convolution_descriptor<double> dd({4096});
  pfft_desc_t cd = dd.c_descriptor();
  REQUIRE(cd.extensions == PFFT_EXT_CONVOLUTION && cd.precision == PFFT_PRECISION_F64);
  REQUIRE(pfft_desc_validate(&cd) == PFFT_OK);
  for (int32_t bad : {8 | 1, 8 | 2, 8 | 4, 4}) {
    c.extensions = bad;
    REQUIRE(pfft_desc_validate(&c) == PFFT_INVALID_CONFIGURATION);
    REQUIRE(std::strstr(pfft_last_error(), "extension") != nullptr);
  }
  c.extensions = PFFT_EXT_CONVOLUTION;
  c.domain = PFFT_DOMAIN_REAL;
  REQUIRE(pfft_desc_validate(&c) == PFFT_INVALID_CONFIGURATION);
  // rank 2 and split storage are refused by validate(), before any device is touched
  queue q;
  bool threw = false;
  try {
    amd::convolution_descriptor<float> nd({128, 4});
    nd.commit(q);
  } catch (const unsupported_configuration& e) {
    threw = std::strstr(e.what(), "1-D") != nullptr;
  }
  REQUIRE(threw);
  threw = false;
  try {
    amd::convolution_descriptor<float> sp({128});
    sp.complex_storage = complex_storage::SPLIT_COMPLEX;
    sp.commit(q);
  } catch (const unsupported_configuration& e) {
    threw = std::strstr(e.what(), "SPLIT_COMPLEX") != nullptr;
  }
  REQUIRE(threw);
  // the verbs of the C ABI on no plan
  REQUIRE(pfft_plan_set_filter(nullptr, nullptr, 1) == PFFT_INVALID_CONFIGURATION);
  REQUIRE(pfft_execute_convolve(nullptr, PFFT_CONVOLVE, nullptr, nullptr) == PFFT_INVALID_CONFIGURATION);
  std::printf("conv host checks OK\n");
  return 0;
}

template <typename T>
int device_checks(std::size_t n, std::size_t batch, std::size_t n_filters, double tol) {
  using namespace portfft;
  using C = std::complex<T>;
  using Z = std::complex<double>;
  std::vector<C> h(n * batch), filt(n * n_filters), got(n * batch);
  for (std::size_t i = 0; i < h.size(); ++i) {
    h[i] = C(static_cast<T>(std::sin(0.37 * i + 0.1)), static_cast<T>(0.5 * std::cos(1.7 * i)));
  }
  for (std::size_t i = 0; i < filt.size(); ++i) {  // time-domain filters
    filt[i] = C(static_cast<T>(std::cos(0.11 * i) / (1.0 + (i % n))), static_cast<T>(std::sin(0.23 * i) / (2.0 + (i % n))));
  }
  C *din, *dout, *dfilt, *dspec;
  REQUIRE(hipMalloc(&din, h.size() * sizeof(C)) == hipSuccess);
  REQUIRE(hipMalloc(&dout, h.size() * sizeof(C)) == hipSuccess);
  REQUIRE(hipMalloc(&dfilt, filt.size() * sizeof(C)) == hipSuccess);
  REQUIRE(hipMalloc(&dspec, filt.size() * sizeof(C)) == hipSuccess);
  REQUIRE(hipMemcpy(din, h.data(), h.size() * sizeof(C), hipMemcpyHostToDevice) == hipSuccess);
  REQUIRE(hipMemcpy(dfilt, filt.data(), filt.size() * sizeof(C), hipMemcpyHostToDevice) == hipSuccess);
  hipStream_t stream;
  REQUIRE(hipStreamCreate(&stream) == hipSuccess);
  queue q(stream);
  // the spectra with a plan of the same kind (batch = n_filters): compute_forward is the ordinary transform
  amd::convolution_descriptor<T> fdesc({n});
  fdesc.number_of_transforms = n_filters;
  auto fplan = fdesc.commit(q);
  fplan.compute_forward(static_cast<const C*>(dfilt), dspec).wait();
  amd::convolution_descriptor<T> desc({n});
  desc.number_of_transforms = batch;
  desc.backward_scale = static_cast<T>(1.0 / static_cast<double>(n));
  auto committed = desc.commit(q);
  bool threw = false;
  try {
    committed.convolve(static_cast<const C*>(din), dout);
  } catch (const invalid_configuration&) {
    threw = true;  // no filter yet
  }
  REQUIRE(threw);
  committed.set_filter(dspec, n_filters);
  for (int corr = 0; corr < 2; ++corr) {
    if (corr) {
      committed.correlate(static_cast<const C*>(din), dout).wait();
    } else {
      committed.convolve(static_cast<const C*>(din), dout).wait();
    }
    REQUIRE(hipMemcpy(got.data(), dout, got.size() * sizeof(C), hipMemcpyDeviceToHost) == hipSuccess);
    // circular convolution with g (correlation: with conj(g[-m])) in double
    double worst = 0;
    for (std::size_t b = 0; b < batch; ++b) {
      const C* g = filt.data() + (b % n_filters) * n;
      double num = 0, den = 0;
      for (std::size_t k = 0; k < n; ++k) {
        Z s = 0;
        for (std::size_t j = 0; j < n; ++j) {
          const std::size_t m = (k + n - j) % n;
          s += Z(h[b * n + j]) * (corr ? std::conj(Z(g[(n - m) % n])) : Z(g[m]));
        }
        num += std::norm(s - Z(got[b * n + k]));
        den += std::norm(s);
      }
      worst = std::max(worst, std::sqrt(num / den));
    }
    std::printf("N=%zu batch=%zu filters=%zu %s %s rel-L2 %.3e\n", n, batch, n_filters, sizeof(T) == 4 ? "f32" : "f64",
                corr ? "correlate" : "convolve", worst);
    REQUIRE(worst < tol);
  }
  // a plain descriptor's plan has no such verb
  threw = false;
  try {
    descriptor<T, domain::COMPLEX> plain({n});
    auto p = plain.commit(q);
    p.set_filter(dspec, 1);
  } catch (const invalid_configuration&) {
    threw = true;
  }
  REQUIRE(threw);
  (void)hipFree(din);
  (void)hipFree(dout);
  (void)hipFree(dfilt);
  (void)hipFree(dspec);
  (void)hipStreamDestroy(stream);
  return 0;
}

int main(int argc, char** argv) {
  if (host_checks() != 0) return 1;
  if (argc > 1 && std::strcmp(argv[1], "host") == 0) return 0;
  // (the spectrum goes through fp32 / fp64 once more than the data: twice the transforms' tolerance)
  if (device_checks<float>(256, 5, 2, 4e-6) != 0) return 1;
  if (device_checks<float>(1000, 3, 1, 4e-6) != 0) return 1;
  if (device_checks<double>(512, 3, 3, 1e-14) != 0) return 1;
  std::printf("conv facade OK\n");
  return 0;
}
