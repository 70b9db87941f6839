// C++ user-code test of fused convolution and overlap-save filtering of REAL data through the facade:
// portfft::amd::real_convolution_descriptor<float> and <double> -> commit -> compute_forward (the filter spectrum) ->
// set_filter -> convolve / correlate against the direct circular sums, and set_filter_taps -> filter in both modes
// against the direct sums
//   convolve  y_i[n] = c sum_k h_i[k] x_i[n - k]      correlate  y_i[n] = c sum_k h_i[k] x_i[n + k]
// in double precision, at N = 64, K = 9, 3 signals of 201 samples (odd pitches; the scalars between the signals must
// stay untouched).
//   hipcc -std=c++17 -I include tests/cpp/rconv_facade_test.cpp -L portfft_amd -lportfft_amd -o build/rconv_facade_test
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
  amd::real_convolution_descriptor<float> desc(64);
  using committed = decltype(desc.commit(std::declval<queue&>()));
  using C = std::complex<float>;
  static_assert(std::is_same_v<committed, committed_descriptor<float, domain::REAL>>, "the committed type of a real plan");
  static_assert(std::is_same_v<decltype(std::declval<committed&>().set_filter(std::declval<const C*>(), std::size_t{3})), void>,
                "the filter: bins");
  static_assert(std::is_same_v<decltype(std::declval<committed&>().convolve(std::declval<float*>())), event>, "in place");
  static_assert(std::is_same_v<decltype(std::declval<committed&>().convolve(std::declval<const float*>(), std::declval<float*>(),
                                                                            std::vector<event>{})),
                               event>,
                "out of place, with dependencies");
  static_assert(std::is_same_v<decltype(std::declval<committed&>().correlate(std::declval<float*>())), event>, "in place");
  static_assert(std::is_same_v<decltype(std::declval<committed&>().correlate(std::declval<const float*>(), std::declval<float*>())),
                               event>,
                "out of place");
  static_assert(std::is_same_v<decltype(std::declval<committed&>().set_filter_taps(std::declval<const float*>(), std::size_t{9},
                                                                                   std::size_t{3})),
                               void>,
                "the taps: real scalars");
  static_assert(std::is_same_v<decltype(std::declval<committed&>().filter(
                                   PFFT_CORRELATE, std::declval<const float*>(), std::declval<float*>(), std::size_t{3},
                                   std::size_t{200}, std::size_t{201}, std::size_t{200}, std::size_t{203}, std::vector<event>{})),
                               event>,
                "the verb returns the event, like convolve");
  // the descriptor: the real defaults and the bit, and the C constructor agrees
  amd::real_descriptor<float> plain(64);
  const pfft_desc_t c = desc.c_descriptor();
  REQUIRE(PFFT_EXT_REAL_CONVOLUTION == 16 && c.extensions == PFFT_EXT_REAL_CONVOLUTION);
  REQUIRE(c.domain == PFFT_DOMAIN_REAL && c.rank == 1 && c.lengths[0] == 64);
  REQUIRE(c.forward_distance == 64 && c.backward_distance == 33);
  REQUIRE(desc.get_input_count(direction::FORWARD) == plain.get_input_count(direction::FORWARD));
  REQUIRE(desc.get_output_count(direction::FORWARD) == plain.get_output_count(direction::FORWARD));
  REQUIRE(pfft_desc_validate(&c) == PFFT_OK);
  pfft_desc_t byc;
  REQUIRE(pfft_desc_init_real_convolution(&byc, PFFT_PRECISION_F32, 64) == PFFT_OK);
  REQUIRE(byc.extensions == c.extensions && byc.domain == c.domain && byc.forward_distance == c.forward_distance &&
          byc.backward_distance == c.backward_distance && byc.placement == c.placement);
  pfft_desc_t bad = c;
  bad.extensions = PFFT_EXT_REAL_CONVOLUTION | PFFT_EXT_REAL_TRANSFORMS;
  REQUIRE(pfft_desc_validate(&bad) == PFFT_INVALID_CONFIGURATION);
  REQUIRE(std::strstr(pfft_last_error(), "extension") != nullptr);
  bad = c;
  bad.domain = PFFT_DOMAIN_COMPLEX;
  REQUIRE(pfft_desc_validate(&bad) == PFFT_INVALID_CONFIGURATION);
  REQUIRE(std::strstr(pfft_last_error(), "extension") != nullptr);
  std::printf("rconv host checks OK\n");
  return 0;
}

template <typename T>
int device_checks(std::size_t n, std::size_t k, std::size_t n_signals, std::size_t length, std::size_t n_filters, double tol) {
  using namespace portfft;
  using C = std::complex<T>;
  const std::size_t bins = n / 2 + 1;
  hipStream_t stream;
  REQUIRE(hipStreamCreate(&stream) == hipSuccess);
  queue q(stream);
  const T pad = static_cast<T>(-5);
  std::vector<T> taps(n_filters * k);
  for (std::size_t i = 0; i < taps.size(); ++i) taps[i] = static_cast<T>(std::cos(0.11 * i + 0.3) / 3.0);
  T* dtaps;
  REQUIRE(hipMalloc(&dtaps, taps.size() * sizeof(T)) == hipSuccess);
  REQUIRE(hipMemcpy(dtaps, taps.data(), taps.size() * sizeof(T), hipMemcpyHostToDevice) == hipSuccess);

  {  // circular: n_signals rows of n scalars, the filter spectra made by the plan itself (scale 1)
    amd::real_convolution_descriptor<T> desc(n);
    desc.number_of_transforms = n_signals;
    auto plan = desc.commit(q);
    std::vector<T> rows(n_signals * n), h(n_signals * n, T(0)), got(n_signals * n);
    for (std::size_t i = 0; i < rows.size(); ++i) rows[i] = static_cast<T>(std::sin(0.37 * i + 0.1));
    for (std::size_t i = 0; i < n_signals; ++i) {
      for (std::size_t t = 0; t < k; ++t) h[i * n + t] = taps[(i % n_filters) * k + t];
    }
    T *drows, *dh, *dgot;
    C* dspec;
    REQUIRE(hipMalloc(&drows, rows.size() * sizeof(T)) == hipSuccess);
    REQUIRE(hipMalloc(&dh, h.size() * sizeof(T)) == hipSuccess);
    REQUIRE(hipMalloc(&dgot, got.size() * sizeof(T)) == hipSuccess);
    REQUIRE(hipMalloc(&dspec, n_signals * bins * sizeof(C)) == hipSuccess);
    REQUIRE(hipMemcpy(drows, rows.data(), rows.size() * sizeof(T), hipMemcpyHostToDevice) == hipSuccess);
    REQUIRE(hipMemcpy(dh, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice) == hipSuccess);
    bool threw = false;
    try {
      plan.convolve(static_cast<const T*>(drows), dgot);
    } catch (const invalid_configuration&) {
      threw = true;  // no filter yet
    }
    REQUIRE(threw);
    plan.compute_forward(static_cast<const T*>(dh), dspec).wait();
    plan.set_filter(dspec, n_signals);
    for (int corr = 0; corr < 2; ++corr) {
      if (corr) {
        plan.correlate(static_cast<const T*>(drows), dgot).wait();
      } else {
        plan.convolve(static_cast<const T*>(drows), dgot).wait();
      }
      REQUIRE(hipMemcpy(got.data(), dgot, got.size() * sizeof(T), hipMemcpyDeviceToHost) == hipSuccess);
      double worst = 0;
      for (std::size_t i = 0; i < n_signals; ++i) {
        double num = 0, den = 0;
        for (std::size_t m = 0; m < n; ++m) {
          double s = 0;
          for (std::size_t t = 0; t < k; ++t) {
            s += static_cast<double>(h[i * n + t]) * static_cast<double>(rows[i * n + (corr ? (m + t) % n : (m + n - t) % n)]);
          }
          s *= static_cast<double>(n);  // c = forward_scale * backward_scale * N
          num += (s - got[i * n + m]) * (s - got[i * n + m]);
          den += s * s;
        }
        worst = std::max(worst, std::sqrt(num / den));
      }
      std::printf("N=%zu rows=%zu %s circular %s rel-L2 %.3e\n", n, n_signals, sizeof(T) == 4 ? "f32" : "f64",
                  corr ? "correlate" : "convolve", worst);
      REQUIRE(worst < tol);
    }
    (void)hipFree(drows);
    (void)hipFree(dh);
    (void)hipFree(dgot);
    (void)hipFree(dspec);
  }

  // overlap-save: signals of `length` scalars at odd pitches
  const std::size_t in_pitch = length + 3 + length % 2, out_len_conv = length + k - 1, out_pitch = out_len_conv + 5 + out_len_conv % 2;
  std::vector<T> x(n_signals * in_pitch, pad), got(n_signals * out_pitch);
  for (std::size_t i = 0; i < n_signals; ++i) {
    for (std::size_t j = 0; j < length; ++j) x[i * in_pitch + j] = static_cast<T>(std::sin(0.37 * (i * length + j) + 0.1));
  }
  T *din, *dout;
  REQUIRE(hipMalloc(&din, x.size() * sizeof(T)) == hipSuccess);
  REQUIRE(hipMalloc(&dout, got.size() * sizeof(T)) == hipSuccess);
  REQUIRE(hipMemcpy(din, x.data(), x.size() * sizeof(T), hipMemcpyHostToDevice) == hipSuccess);
  amd::real_convolution_descriptor<T> desc(n);
  desc.backward_scale = static_cast<T>(1.0 / static_cast<double>(n));  // c = 1
  auto plan = desc.commit(q);
  bool threw = false;
  try {
    plan.filter(PFFT_CONVOLVE, static_cast<const T*>(din), dout, n_signals, length, in_pitch, out_len_conv, out_pitch);
  } catch (const invalid_configuration&) {
    threw = true;  // no taps yet
  }
  REQUIRE(threw);
  plan.set_filter_taps(static_cast<const T*>(dtaps), k, n_filters);
  for (int corr = 0; corr < 2; ++corr) {
    const std::size_t out_len = corr ? length : out_len_conv;
    std::vector<T> fill(got.size(), pad);
    REQUIRE(hipMemcpy(dout, fill.data(), fill.size() * sizeof(T), hipMemcpyHostToDevice) == hipSuccess);
    plan.filter(corr ? PFFT_CORRELATE : PFFT_CONVOLVE, static_cast<const T*>(din), dout, n_signals, length, in_pitch, out_len,
                out_pitch).wait();
    REQUIRE(hipMemcpy(got.data(), dout, got.size() * sizeof(T), hipMemcpyDeviceToHost) == hipSuccess);
    double worst = 0;
    for (std::size_t i = 0; i < n_signals; ++i) {
      const T* h = taps.data() + (i % n_filters) * k;
      double num = 0, den = 0;
      for (std::size_t m = 0; m < out_len; ++m) {
        double s = 0;
        for (std::size_t t = 0; t < k; ++t) {
          if (corr) {
            if (m + t < length) s += static_cast<double>(h[t]) * static_cast<double>(x[i * in_pitch + m + t]);
          } else {
            if (m >= t && m - t < length) s += static_cast<double>(h[t]) * static_cast<double>(x[i * in_pitch + m - t]);
          }
        }
        num += (s - got[i * out_pitch + m]) * (s - got[i * out_pitch + m]);
        den += s * s;
      }
      worst = std::max(worst, std::sqrt(num / den));
      for (std::size_t m = out_len; m < out_pitch; ++m) REQUIRE(got[i * out_pitch + m] == pad);  // not written
    }
    std::printf("N=%zu K=%zu signals=%zu length=%zu filters=%zu %s %s rel-L2 %.3e\n", n, k, n_signals, length, n_filters,
                sizeof(T) == 4 ? "f32" : "f64", corr ? "correlate" : "convolve", worst);
    REQUIRE(worst < tol);
  }
  // in place is refused; a real_descriptor's plan has no such verb
  threw = false;
  try {
    plan.filter(PFFT_CORRELATE, static_cast<const T*>(din), din, n_signals, length, in_pitch, length, in_pitch);
  } catch (const invalid_configuration&) {
    threw = true;
  }
  REQUIRE(threw);
  threw = false;
  try {
    amd::real_descriptor<T> plain(n);
    auto p = plain.commit(q);
    p.set_filter_taps(static_cast<const T*>(dtaps), k, 1);
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
  if (device_checks<float>(64, 9, 3, 201, 2, 2e-6) != 0) return 1;
  if (device_checks<double>(64, 9, 3, 201, 3, 5e-15) != 0) return 1;
  std::printf("rconv facade OK\n");
  return 0;
}
