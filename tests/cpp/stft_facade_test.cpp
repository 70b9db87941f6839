// C++ user-code test of the short-time Fourier transform through the facade: portfft::amd::real_descriptor<float> and
// <double> -> commit -> set_window -> stft in both pad modes against the direct sums
//   X_i[f][k] = forward_scale * sum_n w[n] xe_i[f * hop - lead + n] exp(-2 pi i k n / N)
// in double precision, at N = 64, hop = 17, lead = 31, 3 signals of 201 samples (odd pitches; the elements between the
// frames and between the signals must stay untouched); a plan of the COMPLEX domain refuses both verbs.
//   hipcc -std=c++17 -I include tests/cpp/stft_facade_test.cpp -L portfft_amd -lportfft_amd -o build/stft_facade_test
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
  amd::real_descriptor<float> desc(64);
  using committed = decltype(desc.commit(std::declval<queue&>()));
  using C = std::complex<float>;
  static_assert(std::is_same_v<committed, committed_descriptor<float, domain::REAL>>, "the committed type of a real plan");
  static_assert(std::is_same_v<decltype(std::declval<committed&>().set_window(std::declval<const float*>())), void>,
                "the window: real scalars");
  static_assert(std::is_same_v<decltype(std::declval<committed&>().stft(
                                   std::declval<const float*>(), std::declval<C*>(), std::size_t{3}, std::size_t{201},
                                   std::size_t{203}, std::size_t{17}, std::size_t{31}, PFFT_PAD_REFLECT, std::size_t{12},
                                   std::size_t{34}, std::size_t{500}, std::vector<event>{})),
                               event>,
                "the verb returns the event, like filter");
  // the convolving real plan has the same verbs
  using rc = decltype(std::declval<amd::real_convolution_descriptor<double>&>().commit(std::declval<queue&>()));
  static_assert(std::is_same_v<decltype(std::declval<rc&>().stft(std::declval<const double*>(), std::declval<std::complex<double>*>(),
                                                                 std::size_t{1}, std::size_t{64}, std::size_t{64}, std::size_t{64},
                                                                 std::size_t{0}, PFFT_PAD_ZERO, std::size_t{1}, std::size_t{33},
                                                                 std::size_t{33})),
                               event>,
                "on a real_convolution_descriptor's plan too");
  REQUIRE(PFFT_PAD_ZERO == 0 && PFFT_PAD_REFLECT == 1);
  // no extension bit: 32 stays invalid
  pfft_desc_t c;
  REQUIRE(pfft_desc_init_real(&c, PFFT_PRECISION_F32, 64) == PFFT_OK);
  REQUIRE(c.extensions == PFFT_EXT_REAL_TRANSFORMS && pfft_desc_validate(&c) == PFFT_OK);
  c.extensions = 32;
  REQUIRE(pfft_desc_validate(&c) == PFFT_INVALID_CONFIGURATION);
  // the C entry points answer a null plan
  REQUIRE(pfft_plan_set_window(nullptr, nullptr) == PFFT_INVALID_CONFIGURATION);
  REQUIRE(std::strstr(pfft_last_error(), "null plan") != nullptr);
  REQUIRE(pfft_execute_stft(nullptr, nullptr, nullptr, 1, 1, 1, 1, 0, PFFT_PAD_ZERO, 1, 1, 1) == PFFT_INVALID_CONFIGURATION);
  void* ev = nullptr;
  REQUIRE(pfft_execute_stft_ex(nullptr, nullptr, nullptr, 1, 1, 1, 1, 0, PFFT_PAD_ZERO, 1, 1, 1, 0, nullptr, &ev) ==
          PFFT_INVALID_CONFIGURATION);
  REQUIRE(ev == nullptr);
  std::printf("stft host checks OK\n");
  return 0;
}

template <typename T>
int device_checks(std::size_t n, std::size_t hop, std::size_t lead, std::size_t n_signals, std::size_t length, double tol) {
  using namespace portfft;
  using C = std::complex<T>;
  const std::size_t m = n / 2;
  const double pi = std::acos(-1.0);
  hipStream_t stream;
  REQUIRE(hipStreamCreate(&stream) == hipSuccess);
  queue q(stream);
  const std::size_t in_pitch = length + 3 + length % 2, frame_pitch = m + 2;
  std::vector<T> x(n_signals * in_pitch, static_cast<T>(-5)), w(n);
  for (std::size_t i = 0; i < n_signals; ++i) {
    for (std::size_t j = 0; j < length; ++j) x[i * in_pitch + j] = static_cast<T>(std::sin(0.37 * (i * length + j) + 0.1));
  }
  for (std::size_t j = 0; j < n; ++j) w[j] = static_cast<T>(0.5 - 0.5 * std::cos(2 * pi * j / n));
  T *din, *dw;
  REQUIRE(hipMalloc(&din, x.size() * sizeof(T)) == hipSuccess);
  REQUIRE(hipMalloc(&dw, w.size() * sizeof(T)) == hipSuccess);
  REQUIRE(hipMemcpy(din, x.data(), x.size() * sizeof(T), hipMemcpyHostToDevice) == hipSuccess);
  REQUIRE(hipMemcpy(dw, w.data(), w.size() * sizeof(T), hipMemcpyHostToDevice) == hipSuccess);
  amd::real_descriptor<T> desc(n);
  desc.forward_scale = static_cast<T>(0.5);
  auto plan = desc.commit(q);
  for (int reflect = 0; reflect < 2; ++reflect) {
    // zeros: frames while one holds a sample; reflection: frames inside the signal padded by lead on both sides
    const std::size_t n_frames = reflect ? (length + 2 * lead - n) / hop + 1 : (length + lead - 1) / hop + 1;
    const std::size_t out_pitch = n_frames * frame_pitch + 3;
    const C pad(static_cast<T>(-7), static_cast<T>(9));
    std::vector<C> got(n_signals * out_pitch, pad);
    C* dout;
    REQUIRE(hipMalloc(&dout, got.size() * sizeof(C)) == hipSuccess);
    REQUIRE(hipMemcpy(dout, got.data(), got.size() * sizeof(C), hipMemcpyHostToDevice) == hipSuccess);
    if (!reflect) {
      bool threw = false;
      try {
        plan.stft(din, dout, n_signals, length, in_pitch, hop, lead, PFFT_PAD_ZERO, n_frames, frame_pitch, out_pitch);
      } catch (const invalid_configuration&) {
        threw = true;  // no window yet
      }
      REQUIRE(threw);
      plan.set_window(dw);
    }
    plan.stft(din, dout, n_signals, length, in_pitch, hop, lead, reflect ? PFFT_PAD_REFLECT : PFFT_PAD_ZERO, n_frames,
              frame_pitch, out_pitch).wait();
    REQUIRE(hipMemcpy(got.data(), dout, got.size() * sizeof(C), hipMemcpyDeviceToHost) == hipSuccess);
    double worst = 0;
    const long long last = static_cast<long long>(length) - 1;
    for (std::size_t i = 0; i < n_signals; ++i) {
      double num = 0, den = 0;
      for (std::size_t f = 0; f < n_frames; ++f) {
        std::vector<double> frame(n);
        for (std::size_t j = 0; j < n; ++j) {
          long long p = static_cast<long long>(f * hop + j) - static_cast<long long>(lead);
          double v = 0;
          if (reflect) {
            p = p < 0 ? -p : (p > last ? 2 * last - p : p);
            v = x[i * in_pitch + p];
          } else if (p >= 0 && p <= last) {
            v = x[i * in_pitch + p];
          }
          frame[j] = v * static_cast<double>(w[j]);
        }
        for (std::size_t k = 0; k <= m; ++k) {
          std::complex<double> s = 0;
          for (std::size_t j = 0; j < n; ++j) s += frame[j] * std::polar(1.0, -2 * pi * static_cast<double>((k * j) % n) / n);
          s *= 0.5;
          const C g = got[i * out_pitch + f * frame_pitch + k];
          num += std::norm(s - std::complex<double>(g.real(), g.imag()));
          den += std::norm(s);
          if (k == 0 || k == m) REQUIRE(g.imag() == T(0));
        }
        for (std::size_t k = m + 1; k < frame_pitch; ++k) REQUIRE(got[i * out_pitch + f * frame_pitch + k] == pad);
      }
      for (std::size_t k = n_frames * frame_pitch; k < out_pitch; ++k) REQUIRE(got[i * out_pitch + k] == pad);
      worst = std::max(worst, std::sqrt(num / den));
    }
    std::printf("N=%zu hop=%zu lead=%zu signals=%zu length=%zu frames=%zu %s %s rel-L2 %.3e\n", n, hop, lead, n_signals, length,
                n_frames, sizeof(T) == 4 ? "f32" : "f64", reflect ? "reflect" : "zero", worst);
    REQUIRE(worst < tol);
    (void)hipFree(dout);
  }
  // a plan of the COMPLEX domain refuses both verbs
  {
    descriptor<T, domain::COMPLEX> cd({n});
    auto cp = cd.commit(q);
    int threw = 0;
    try {
      cp.set_window(dw);
    } catch (const invalid_configuration&) {
      ++threw;
    }
    try {
      cp.stft(din, reinterpret_cast<C*>(din), 1, n, n, n, 0, PFFT_PAD_ZERO, 1, m + 1, m + 1);
    } catch (const invalid_configuration&) {
      ++threw;
    }
    REQUIRE(threw == 2);
  }
  (void)hipFree(din);
  (void)hipFree(dw);
  (void)hipStreamDestroy(stream);
  return 0;
}

int main(int argc, char** argv) {
  if (host_checks() != 0) return 1;
  if (argc > 1 && std::strcmp(argv[1], "host") == 0) return 0;
  // (helpers.REL_L2_TOL of the Python suite: 2e-6 / 5e-15)
  if (device_checks<float>(64, 17, 31, 3, 201, 2e-6) != 0) return 1;
  if (device_checks<double>(64, 17, 31, 3, 201, 5e-15) != 0) return 1;
  std::printf("stft facade OK\n");
  return 0;
}
