// C++ user-code test of the inverse short-time Fourier transform through the facade: portfft::amd::real_descriptor<float>
// and <double> -> commit -> set_synthesis_window -> istft in both modes against the direct sums
//   g_i[f][j] = backward_scale * (Re X[0] + (-1)^j Re X[M] + 2 sum_{0<k<M} Re(X[k] exp(2 pi i k j / N)))
//   y_i[t]    = sum_f w[u - f * hop] * g_i[f][u - f * hop],  u = t + lead;  NORMALIZE: / sum_f w[u - f * hop]^2
// in double precision, at N = 64, hop = 17, lead = 31, 3 signals of 12 frames (odd pitches; the elements behind out_length
// and between the signals must stay untouched); a plan of the COMPLEX domain refuses both verbs.
//   hipcc -std=c++17 -I include tests/cpp/istft_facade_test.cpp -L portfft_amd -lportfft_amd -o build/istft_facade_test
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
  static_assert(std::is_same_v<decltype(std::declval<committed&>().set_synthesis_window(std::declval<const float*>())), void>,
                "the synthesis window: real scalars");
  static_assert(std::is_same_v<decltype(std::declval<committed&>().istft(
                                   std::declval<const C*>(), std::declval<float*>(), std::size_t{3}, std::size_t{12},
                                   std::size_t{34}, std::size_t{500}, std::size_t{17}, std::size_t{31}, PFFT_ISTFT_NORMALIZE,
                                   std::size_t{220}, std::size_t{223}, std::size_t{0}, std::vector<event>{})),
                               event>,
                "the verb returns the event, like stft");
  // the convolving real plan has the same verbs; chunk_frames and the dependencies are optional
  using rc = decltype(std::declval<amd::real_convolution_descriptor<double>&>().commit(std::declval<queue&>()));
  static_assert(std::is_same_v<decltype(std::declval<rc&>().istft(std::declval<const std::complex<double>*>(),
                                                                  std::declval<double*>(), std::size_t{1}, std::size_t{1},
                                                                  std::size_t{33}, std::size_t{33}, std::size_t{64},
                                                                  std::size_t{0}, PFFT_ISTFT_PLAIN, std::size_t{64},
                                                                  std::size_t{64})),
                               event>,
                "on a real_convolution_descriptor's plan too");
  REQUIRE(PFFT_ISTFT_PLAIN == 0 && PFFT_ISTFT_NORMALIZE == 1);
  REQUIRE(PFFT_ISTFT_ENV_MIN == 1e-11);
  // no extension bit: 32 stays invalid
  pfft_desc_t c;
  REQUIRE(pfft_desc_init_real(&c, PFFT_PRECISION_F32, 64) == PFFT_OK);
  REQUIRE(c.extensions == PFFT_EXT_REAL_TRANSFORMS && pfft_desc_validate(&c) == PFFT_OK);
  c.extensions = 32;
  REQUIRE(pfft_desc_validate(&c) == PFFT_INVALID_CONFIGURATION);
  // the C entry points answer a null plan
  REQUIRE(pfft_plan_set_synthesis_window(nullptr, nullptr) == PFFT_INVALID_CONFIGURATION);
  REQUIRE(std::strstr(pfft_last_error(), "null plan") != nullptr);
  REQUIRE(pfft_execute_istft(nullptr, nullptr, nullptr, 1, 1, 1, 1, 1, 0, PFFT_ISTFT_PLAIN, 1, 1, 0) == PFFT_INVALID_CONFIGURATION);
  void* ev = nullptr;
  REQUIRE(pfft_execute_istft_ex(nullptr, nullptr, nullptr, 1, 1, 1, 1, 1, 0, PFFT_ISTFT_PLAIN, 1, 1, 0, 0, nullptr, &ev) ==
          PFFT_INVALID_CONFIGURATION);
  REQUIRE(ev == nullptr);
  uint64_t chunk = 7;
  REQUIRE(pfft_plan_istft_chunk_frames(nullptr, 1, 1, 1, &chunk) == PFFT_INVALID_CONFIGURATION && chunk == 7);
  std::printf("istft host checks OK\n");
  return 0;
}

template <typename T>
int device_checks(std::size_t n, std::size_t hop, std::size_t lead, std::size_t n_signals, std::size_t n_frames, double tol) {
  using namespace portfft;
  using C = std::complex<T>;
  const std::size_t m = n / 2;
  const double pi = std::acos(-1.0);
  hipStream_t stream;
  REQUIRE(hipStreamCreate(&stream) == hipSuccess);
  queue q(stream);
  const std::size_t frame_pitch = m + 2, in_pitch = n_frames * frame_pitch + 3;
  const std::size_t out_length = (n_frames - 1) * hop + n - lead - 2, out_pitch = out_length + 3 + out_length % 2;
  std::vector<C> y(n_signals * in_pitch, C(static_cast<T>(-5), static_cast<T>(-5)));
  std::vector<T> w(n);
  for (std::size_t i = 0; i < n_signals; ++i) {
    for (std::size_t f = 0; f < n_frames; ++f) {
      for (std::size_t k = 0; k <= m; ++k) {
        const double a = 0.37 * ((i * n_frames + f) * (m + 1) + k) + 0.1;
        y[i * in_pitch + f * frame_pitch + k] = C(static_cast<T>(std::sin(a)), static_cast<T>(std::cos(1.7 * a)));
      }
    }
  }
  // (a window that is nowhere small: the envelope stays far above the threshold)
  for (std::size_t j = 0; j < n; ++j) w[j] = static_cast<T>(0.75 - 0.25 * std::cos(2 * pi * j / n));
  C* din;
  T* dw;
  REQUIRE(hipMalloc(&din, y.size() * sizeof(C)) == hipSuccess);
  REQUIRE(hipMalloc(&dw, w.size() * sizeof(T)) == hipSuccess);
  REQUIRE(hipMemcpy(din, y.data(), y.size() * sizeof(C), hipMemcpyHostToDevice) == hipSuccess);
  REQUIRE(hipMemcpy(dw, w.data(), w.size() * sizeof(T), hipMemcpyHostToDevice) == hipSuccess);
  amd::real_descriptor<T> desc(n);
  desc.backward_scale = static_cast<T>(0.5);
  auto plan = desc.commit(q);
  // the frames in double, by direct sums
  std::vector<double> g(n_signals * n_frames * n);
  for (std::size_t i = 0; i < n_signals; ++i) {
    for (std::size_t f = 0; f < n_frames; ++f) {
      const C* bins = &y[i * in_pitch + f * frame_pitch];
      for (std::size_t j = 0; j < n; ++j) {
        double s = static_cast<double>(bins[0].real()) + (j % 2 ? -1.0 : 1.0) * static_cast<double>(bins[m].real());
        for (std::size_t k = 1; k < m; ++k) {
          const std::complex<double> x(bins[k].real(), bins[k].imag());
          s += 2 * (x * std::polar(1.0, 2 * pi * static_cast<double>((k * j) % n) / n)).real();
        }
        g[(i * n_frames + f) * n + j] = 0.5 * s;
      }
    }
  }
  for (int normalize = 0; normalize < 2; ++normalize) {
    const T pad = static_cast<T>(-7);
    std::vector<T> got(n_signals * out_pitch, pad);
    T* dout;
    REQUIRE(hipMalloc(&dout, got.size() * sizeof(T)) == hipSuccess);
    REQUIRE(hipMemcpy(dout, got.data(), got.size() * sizeof(T), hipMemcpyHostToDevice) == hipSuccess);
    if (!normalize) {
      bool threw = false;
      try {
        plan.istft(din, dout, n_signals, n_frames, frame_pitch, in_pitch, hop, lead, PFFT_ISTFT_PLAIN, out_length, out_pitch);
      } catch (const invalid_configuration&) {
        threw = true;  // no synthesis window yet
      }
      REQUIRE(threw);
      plan.set_synthesis_window(dw);
    }
    // (three chunks of five frames, and the plan's own choice)
    plan.istft(din, dout, n_signals, n_frames, frame_pitch, in_pitch, hop, lead, normalize ? PFFT_ISTFT_NORMALIZE : PFFT_ISTFT_PLAIN,
               out_length, out_pitch, normalize ? 0 : 5).wait();
    REQUIRE(hipMemcpy(got.data(), dout, got.size() * sizeof(T), hipMemcpyDeviceToHost) == hipSuccess);
    double worst = 0;
    for (std::size_t i = 0; i < n_signals; ++i) {
      double num = 0, den = 0;
      for (std::size_t t = 0; t < out_length; ++t) {
        const std::size_t u = t + lead;
        double ola = 0, env = 0;
        for (std::size_t f = 0; f < n_frames; ++f) {
          if (u >= f * hop && u - f * hop < n) {
            const double wv = static_cast<double>(w[u - f * hop]);
            ola += wv * g[(i * n_frames + f) * n + (u - f * hop)];
            env += wv * wv;
          }
        }
        const double want = normalize ? ola / env : ola;
        num += (want - static_cast<double>(got[i * out_pitch + t])) * (want - static_cast<double>(got[i * out_pitch + t]));
        den += want * want;
      }
      for (std::size_t t = out_length; t < out_pitch; ++t) REQUIRE(got[i * out_pitch + t] == pad);
      worst = std::max(worst, std::sqrt(num / den));
    }
    std::printf("N=%zu hop=%zu lead=%zu signals=%zu frames=%zu out_length=%zu %s %s rel-L2 %.3e\n", n, hop, lead, n_signals,
                n_frames, out_length, sizeof(T) == 4 ? "f32" : "f64", normalize ? "normalize" : "plain", worst);
    REQUIRE(worst < tol);
    (void)hipFree(dout);
  }
  // a plan of the COMPLEX domain refuses both verbs
  {
    descriptor<T, domain::COMPLEX> cd({n});
    auto cp = cd.commit(q);
    int threw = 0;
    try {
      cp.set_synthesis_window(dw);
    } catch (const invalid_configuration&) {
      ++threw;
    }
    try {
      cp.istft(din, dw, 1, 1, m + 1, m + 1, n, 0, PFFT_ISTFT_PLAIN, n, n);
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
  if (device_checks<float>(64, 17, 31, 3, 12, 2e-6) != 0) return 1;
  if (device_checks<double>(64, 17, 31, 3, 12, 5e-15) != 0) return 1;
  std::printf("istft facade OK\n");
  return 0;
}
