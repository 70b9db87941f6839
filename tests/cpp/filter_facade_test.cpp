// C++ user-code test of overlap-save filtering through the facade: portfft::amd::convolution_descriptor<float> and
// <double> -> commit -> set_filter_taps -> filter in both modes against the direct sums in double precision
//   convolve  y_i[n] = c sum_k h_i[k] x_i[n - k]      correlate  y_i[n] = c sum_k conj(h_i[k]) x_i[n + k]
// at N = 64, K = 9, 3 signals of 200 samples (pitched buffers; the elements between the signals must stay untouched).
//   hipcc -std=c++17 -I include tests/cpp/filter_facade_test.cpp -L portfft_amd -lportfft_amd -o build/filter_facade_test
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
  amd::convolution_descriptor<float> desc({64});
  using committed = decltype(desc.commit(std::declval<queue&>()));
  using C = std::complex<float>;
  static_assert(std::is_same_v<decltype(std::declval<committed&>().set_filter_taps(std::declval<const C*>(), std::size_t{9},
                                                                                   std::size_t{3})),
                               void>,
                "the taps");
  static_assert(std::is_same_v<decltype(std::declval<committed&>().filter(
                                   PFFT_CORRELATE, std::declval<const C*>(), std::declval<C*>(), std::size_t{3}, std::size_t{200},
                                   std::size_t{200}, std::size_t{200}, std::size_t{200}, std::vector<event>{})),
                               event>,
                "the verb returns the event, like convolve");
  // the verbs of the C ABI on no plan
  REQUIRE(pfft_plan_set_filter_taps(nullptr, nullptr, 1, 1) == PFFT_INVALID_CONFIGURATION);
  REQUIRE(std::strstr(pfft_last_error(), "null plan") != nullptr);
  REQUIRE(pfft_execute_filter(nullptr, PFFT_CONVOLVE, nullptr, nullptr, 1, 1, 1, 1, 1) == PFFT_INVALID_CONFIGURATION);
  void* ev = nullptr;
  REQUIRE(pfft_execute_filter_ex(nullptr, PFFT_CONVOLVE, nullptr, nullptr, 1, 1, 1, 1, 1, 0, nullptr, &ev) ==
          PFFT_INVALID_CONFIGURATION);
  REQUIRE(ev == nullptr);
  std::printf("filter host checks OK\n");
  return 0;
}

template <typename T>
int device_checks(std::size_t n, std::size_t k, std::size_t n_signals, std::size_t length, std::size_t n_filters, double tol) {
  using namespace portfft;
  using C = std::complex<T>;
  using Z = std::complex<double>;
  const std::size_t in_pitch = length + 3, out_len_conv = length + k - 1, out_pitch = out_len_conv + 5;
  const C pad(static_cast<T>(-5), static_cast<T>(0));
  std::vector<C> x(n_signals * in_pitch, pad), taps(n_filters * k), got(n_signals * out_pitch);
  for (std::size_t i = 0; i < n_signals; ++i) {
    for (std::size_t j = 0; j < length; ++j) {
      const double a = static_cast<double>(i * length + j);
      x[i * in_pitch + j] = C(static_cast<T>(std::sin(0.37 * a + 0.1)), static_cast<T>(0.5 * std::cos(1.7 * a)));
    }
  }
  for (std::size_t i = 0; i < taps.size(); ++i) {
    taps[i] = C(static_cast<T>(std::cos(0.11 * i) / 3.0), static_cast<T>(std::sin(0.23 * i + 0.4) / 3.0));
  }
  C *din, *dout, *dtaps;
  REQUIRE(hipMalloc(&din, x.size() * sizeof(C)) == hipSuccess);
  REQUIRE(hipMalloc(&dout, got.size() * sizeof(C)) == hipSuccess);
  REQUIRE(hipMalloc(&dtaps, taps.size() * sizeof(C)) == hipSuccess);
  REQUIRE(hipMemcpy(din, x.data(), x.size() * sizeof(C), hipMemcpyHostToDevice) == hipSuccess);
  REQUIRE(hipMemcpy(dtaps, taps.data(), taps.size() * sizeof(C), hipMemcpyHostToDevice) == hipSuccess);
  hipStream_t stream;
  REQUIRE(hipStreamCreate(&stream) == hipSuccess);
  queue q(stream);
  amd::convolution_descriptor<T> desc({n});
  desc.backward_scale = static_cast<T>(1.0 / static_cast<double>(n));  // c = 1
  auto committed = desc.commit(q);
  bool threw = false;
  try {
    committed.filter(PFFT_CONVOLVE, static_cast<const C*>(din), dout, n_signals, length, in_pitch, out_len_conv, out_pitch);
  } catch (const invalid_configuration&) {
    threw = true;  // no taps yet
  }
  REQUIRE(threw);
  committed.set_filter_taps(dtaps, k, n_filters);
  for (int corr = 0; corr < 2; ++corr) {
    const std::size_t out_len = corr ? length : out_len_conv;
    std::vector<C> fill(got.size(), pad);
    REQUIRE(hipMemcpy(dout, fill.data(), fill.size() * sizeof(C), hipMemcpyHostToDevice) == hipSuccess);
    committed.filter(corr ? PFFT_CORRELATE : PFFT_CONVOLVE, static_cast<const C*>(din), dout, n_signals, length, in_pitch,
                     out_len, out_pitch).wait();
    REQUIRE(hipMemcpy(got.data(), dout, got.size() * sizeof(C), hipMemcpyDeviceToHost) == hipSuccess);
    double worst = 0;
    for (std::size_t i = 0; i < n_signals; ++i) {
      const C* h = taps.data() + (i % n_filters) * k;
      double num = 0, den = 0;
      for (std::size_t m = 0; m < out_len; ++m) {
        Z s = 0;
        for (std::size_t t = 0; t < k; ++t) {
          if (corr) {
            if (m + t < length) s += std::conj(Z(h[t])) * Z(x[i * in_pitch + m + t]);
          } else {
            if (m >= t && m - t < length) s += Z(h[t]) * Z(x[i * in_pitch + m - t]);
          }
        }
        num += std::norm(s - Z(got[i * out_pitch + m]));
        den += std::norm(s);
      }
      worst = std::max(worst, std::sqrt(num / den));
      for (std::size_t m = out_len; m < out_pitch; ++m) REQUIRE(got[i * out_pitch + m] == pad);  // not written
    }
    std::printf("N=%zu K=%zu signals=%zu length=%zu filters=%zu %s %s rel-L2 %.3e\n", n, k, n_signals, length, n_filters,
                sizeof(T) == 4 ? "f32" : "f64", corr ? "correlate" : "convolve", worst);
    REQUIRE(worst < tol);
  }
  // in place is refused; a plain descriptor's plan has no such verb
  threw = false;
  try {
    committed.filter(PFFT_CORRELATE, static_cast<const C*>(din), din, n_signals, length, in_pitch, length, in_pitch);
  } catch (const invalid_configuration&) {
    threw = true;
  }
  REQUIRE(threw);
  threw = false;
  try {
    descriptor<T, domain::COMPLEX> plain({n});
    auto p = plain.commit(q);
    p.set_filter_taps(dtaps, k, 1);
  } catch (const invalid_configuration&) {
    threw = true;
  }
  REQUIRE(threw);
  (void)hipFree(din);
  (void)hipFree(dout);
  (void)hipFree(dtaps);
  (void)hipStreamDestroy(stream);
  return 0;
}

int main(int argc, char** argv) {
  if (host_checks() != 0) return 1;
  if (argc > 1 && std::strcmp(argv[1], "host") == 0) return 0;
  // (helpers.REL_L2_TOL of the Python suite: 2e-6 / 5e-15)
  if (device_checks<float>(64, 9, 3, 200, 2, 2e-6) != 0) return 1;
  if (device_checks<double>(64, 9, 3, 200, 3, 5e-15) != 0) return 1;
  std::printf("filter facade OK\n");
  return 0;
}
