// C++ user-code test of the DCT-IV and the MDCT through the facade: portfft::amd::real_descriptor<float> and <double> ->
// commit -> prepare_dct4 -> dct4, set_mdct_window -> mdct, against the direct sums
//   dct4:  y[k] = scale * 2 * sum_n x[n] cos(pi (2n + 1)(2k + 1) / (4N))
//   mdct:  X[f][k] = forward_scale * 2 * sum_{n<2N} w[n] xe[f N - lead + n] cos(pi (2n + 1 + N)(2k + 1) / (4N))
// in double precision with the argument reduced mod 8N in integers, at N = 64: 5 rows with odd pitches (the scalars between
// the rows must stay untouched), in place, forward and inverse; 2 signals of 4 frames with lead N and a window.  The verbs
// before their prepare call, the refusals of the C ABI (a pitch below N, lead 2N, overlapping buffers) and all four verbs on
// a plan of the COMPLEX domain throw invalid_configuration.
//   hipcc -std=c++17 -I include tests/cpp/dct4_facade_test.cpp -L portfft_amd -lportfft_amd -o build/dct4_facade_test
// With argument "host" only the host-side checks run (no GPU needed).
#include <hip/hip_runtime.h>

#include <cmath>
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
  static_assert(std::is_same_v<committed, committed_descriptor<float, domain::REAL>>, "the committed type of a real plan");
  static_assert(std::is_same_v<decltype(std::declval<committed&>().prepare_dct4()), void>, "prepare_dct4 takes no data");
  static_assert(std::is_same_v<decltype(std::declval<committed&>().set_mdct_window(std::declval<const float*>())), void>,
                "set_mdct_window takes the window");
  static_assert(std::is_same_v<decltype(std::declval<committed&>().dct4(std::declval<const float*>(), std::declval<float*>(), true,
                                                                        std::size_t{5}, std::size_t{67}, std::size_t{71},
                                                                        std::vector<event>{})),
                               event>,
                "dct4 returns the event, like dct");
  static_assert(std::is_same_v<decltype(std::declval<committed&>().mdct(std::declval<const float*>(), std::declval<float*>(),
                                                                        std::size_t{2}, std::size_t{200}, std::size_t{203},
                                                                        std::size_t{64}, std::size_t{4}, std::size_t{67},
                                                                        std::size_t{271}, std::vector<event>{})),
                               event>,
                "mdct returns the event, like stft");
  // the convolving real plan has the same verbs; the dependencies are optional
  using rc = decltype(std::declval<amd::real_convolution_descriptor<double>&>().commit(std::declval<queue&>()));
  static_assert(std::is_same_v<decltype(std::declval<rc&>().dct4(std::declval<const double*>(), std::declval<double*>(), false,
                                                                 std::size_t{1}, std::size_t{64}, std::size_t{64})),
                               event>,
                "on a real_convolution_descriptor's plan too");
  // no extension bit: 32 stays invalid
  pfft_desc_t c;
  REQUIRE(pfft_desc_init_real(&c, PFFT_PRECISION_F32, 64) == PFFT_OK);
  REQUIRE(c.extensions == PFFT_EXT_REAL_TRANSFORMS && pfft_desc_validate(&c) == PFFT_OK);
  c.extensions = 32;
  REQUIRE(pfft_desc_validate(&c) == PFFT_INVALID_CONFIGURATION);
  // the C entry points answer a null plan
  void* ev = nullptr;
  REQUIRE(pfft_plan_prepare_dct4(nullptr) == PFFT_INVALID_CONFIGURATION);
  REQUIRE(std::strstr(pfft_last_error(), "null plan") != nullptr);
  REQUIRE(pfft_execute_dct4(nullptr, 0, nullptr, nullptr, 1, 64, 64) == PFFT_INVALID_CONFIGURATION);
  REQUIRE(std::strstr(pfft_last_error(), "null plan") != nullptr);
  REQUIRE(pfft_execute_dct4_ex(nullptr, 1, nullptr, nullptr, 1, 64, 64, 0, nullptr, &ev) == PFFT_INVALID_CONFIGURATION);
  REQUIRE(pfft_plan_set_mdct_window(nullptr, nullptr) == PFFT_INVALID_CONFIGURATION);
  REQUIRE(std::strstr(pfft_last_error(), "null plan") != nullptr);
  REQUIRE(pfft_execute_mdct(nullptr, nullptr, nullptr, 1, 192, 192, 64, 4, 64, 256) == PFFT_INVALID_CONFIGURATION);
  REQUIRE(std::strstr(pfft_last_error(), "null plan") != nullptr);
  REQUIRE(pfft_execute_mdct_ex(nullptr, nullptr, nullptr, 1, 192, 192, 64, 4, 64, 256, 0, nullptr, &ev) == PFFT_INVALID_CONFIGURATION);
  REQUIRE(ev == nullptr);
  std::printf("dct4 host checks OK\n");
  return 0;
}

template <typename F>
static bool throws_invalid(F&& f) {
  try {
    f();
  } catch (const portfft::invalid_configuration&) {
    return true;
  }
  return false;
}

template <typename T>
int device_checks(std::size_t n, std::size_t rows, double tol) {
  using namespace portfft;
  const double pi = std::acos(-1.0);
  hipStream_t stream;
  REQUIRE(hipStreamCreate(&stream) == hipSuccess);
  queue q(stream);
  const std::size_t in_pitch = n + 3, out_pitch = n + 7;
  const T pad = static_cast<T>(-7);
  std::vector<T> x(rows * in_pitch, pad);
  for (std::size_t r = 0; r < rows; ++r) {
    for (std::size_t j = 0; j < n; ++j) x[r * in_pitch + j] = static_cast<T>(std::sin(0.37 * (r * n + j) + 0.1));
  }
  T *din, *dout;
  REQUIRE(hipMalloc(&din, x.size() * sizeof(T)) == hipSuccess);
  REQUIRE(hipMalloc(&dout, rows * out_pitch * sizeof(T)) == hipSuccess);
  REQUIRE(hipMemcpy(din, x.data(), x.size() * sizeof(T), hipMemcpyHostToDevice) == hipSuccess);
  amd::real_descriptor<T> desc(n);
  desc.forward_scale = static_cast<T>(0.5);
  desc.backward_scale = static_cast<T>(0.25);
  auto plan = desc.commit(q);
  REQUIRE(throws_invalid([&] { plan.dct4(din, dout, false, rows, in_pitch, out_pitch); }));  // not prepared yet
  REQUIRE(throws_invalid([&] { plan.mdct(din, dout, 1, 3 * n, 3 * n, n, 4, n, 4 * n); }));   // no window yet
  plan.prepare_dct4();
  plan.prepare_dct4();  // (idempotent)
  REQUIRE(throws_invalid([&] { plan.mdct(din, dout, 1, 3 * n, 3 * n, n, 4, n, 4 * n); }));   // prepared, but still no window
  // what the C ABI refuses, the facade throws
  REQUIRE(throws_invalid([&] { plan.dct4(din, dout, false, rows, n - 1, out_pitch); }));
  REQUIRE(throws_invalid([&] { plan.dct4(din, din, false, rows, in_pitch, in_pitch + 1); }));
  REQUIRE(throws_invalid([&] { plan.dct4(din, din + 1, false, rows, in_pitch, in_pitch); }));
  for (int inverse = 0; inverse < 2; ++inverse) {
    for (int in_place = 0; in_place < 2; ++in_place) {
      const std::size_t op = in_place ? in_pitch : out_pitch;
      std::vector<T> got(rows * op, pad);
      T* dst = dout;
      if (in_place) {
        dst = din;
      } else {
        REQUIRE(hipMemcpy(dout, got.data(), got.size() * sizeof(T), hipMemcpyHostToDevice) == hipSuccess);
      }
      plan.dct4(din, dst, inverse != 0, rows, in_pitch, op).wait();
      REQUIRE(hipMemcpy(got.data(), dst, got.size() * sizeof(T), hipMemcpyDeviceToHost) == hipSuccess);
      if (in_place) REQUIRE(hipMemcpy(din, x.data(), x.size() * sizeof(T), hipMemcpyHostToDevice) == hipSuccess);
      double worst = 0;
      for (std::size_t r = 0; r < rows; ++r) {
        double num = 0, den = 0;
        for (std::size_t k = 0; k < n; ++k) {
          double s = 0;
          for (std::size_t j = 0; j < n; ++j) {
            const double c = std::cos(pi * static_cast<double>(((2 * k + 1) * (2 * j + 1)) % (8 * n)) / static_cast<double>(4 * n));
            s += 2.0 * static_cast<double>(x[r * in_pitch + j]) * c;
          }
          const double want = (inverse ? 0.25 : 0.5) * s;
          const double d = want - static_cast<double>(got[r * op + k]);
          num += d * d;
          den += want * want;
        }
        for (std::size_t t = n; t < op; ++t) REQUIRE(got[r * op + t] == pad);
        worst = std::max(worst, std::sqrt(num / den));
      }
      std::printf("N=%zu rows=%zu %s dct4 %s %s rel-L2 %.3e\n", n, rows, sizeof(T) == 4 ? "f32" : "f64",
                  inverse ? "inverse" : "forward", in_place ? "in place" : "out of place", worst);
      REQUIRE(worst < tol);
    }
  }
  // MDCT: 2 signals of 3N + 5 samples, lead N, 4 frames (the first starts at -N, the last is cut), a window off symmetry
  {
    const std::size_t n_sig = 2, length = 3 * n + 5, sp = length + 2, frames = 4, fp = n + 3, op = frames * fp + 1, lead = n;
    std::vector<T> sig(n_sig * sp, pad), w(2 * n), coeff(n_sig * op, pad);
    for (std::size_t i = 0; i < n_sig; ++i) {
      for (std::size_t j = 0; j < length; ++j) sig[i * sp + j] = static_cast<T>(std::cos(0.41 * (i * length + j) + 0.2));
    }
    for (std::size_t j = 0; j < 2 * n; ++j) w[j] = static_cast<T>(0.5 + 0.4 * std::sin(0.13 * j));
    T *dsig, *dw, *dc;
    REQUIRE(hipMalloc(&dsig, sig.size() * sizeof(T)) == hipSuccess);
    REQUIRE(hipMalloc(&dw, w.size() * sizeof(T)) == hipSuccess);
    REQUIRE(hipMalloc(&dc, coeff.size() * sizeof(T)) == hipSuccess);
    REQUIRE(hipMemcpy(dsig, sig.data(), sig.size() * sizeof(T), hipMemcpyHostToDevice) == hipSuccess);
    REQUIRE(hipMemcpy(dw, w.data(), w.size() * sizeof(T), hipMemcpyHostToDevice) == hipSuccess);
    REQUIRE(hipMemcpy(dc, coeff.data(), coeff.size() * sizeof(T), hipMemcpyHostToDevice) == hipSuccess);
    plan.set_mdct_window(dw);
    REQUIRE(throws_invalid([&] { plan.mdct(dsig, dc, n_sig, length, sp, 2 * n, frames, fp, op); }));      // lead 2N
    REQUIRE(throws_invalid([&] { plan.mdct(dsig, dc, n_sig, length, sp, lead, frames, n - 1, op); }));    // frame_pitch
    REQUIRE(throws_invalid([&] { plan.mdct(dsig, dsig, 1, length, sp, lead, 1, n, n); }));               // in place
    plan.mdct(dsig, dc, n_sig, length, sp, lead, frames, fp, op).wait();
    REQUIRE(hipMemcpy(coeff.data(), dc, coeff.size() * sizeof(T), hipMemcpyDeviceToHost) == hipSuccess);
    double worst = 0;
    for (std::size_t i = 0; i < n_sig; ++i) {
      for (std::size_t f = 0; f < frames; ++f) {
        double num = 0, den = 0;
        for (std::size_t k = 0; k < n; ++k) {
          double s = 0;
          for (std::size_t j = 0; j < 2 * n; ++j) {
            const long long t = static_cast<long long>(f * n + j) - static_cast<long long>(lead);
            if (t < 0 || t >= static_cast<long long>(length)) continue;
            const double c = std::cos(pi * static_cast<double>(((2 * k + 1) * (2 * j + 1 + n)) % (8 * n)) / static_cast<double>(4 * n));
            s += 2.0 * static_cast<double>(w[j]) * static_cast<double>(sig[i * sp + static_cast<std::size_t>(t)]) * c;
          }
          const double want = 0.5 * s;
          const double d = want - static_cast<double>(coeff[i * op + f * fp + k]);
          num += d * d;
          den += want * want;
        }
        for (std::size_t t = n; t < fp; ++t) REQUIRE(coeff[i * op + f * fp + t] == pad);
        worst = std::max(worst, std::sqrt(num / den));
      }
      REQUIRE(coeff[i * op + frames * fp] == pad);
    }
    std::printf("N=%zu %s mdct %zu signals x %zu frames rel-L2 %.3e\n", n, sizeof(T) == 4 ? "f32" : "f64", n_sig, frames, worst);
    REQUIRE(worst < tol);
    (void)hipFree(dsig);
    (void)hipFree(dw);
    (void)hipFree(dc);
  }
  // a plan of the COMPLEX domain refuses the four verbs
  {
    descriptor<T, domain::COMPLEX> cd({n});
    auto cp = cd.commit(q);
    REQUIRE(throws_invalid([&] { cp.prepare_dct4(); }));
    REQUIRE(throws_invalid([&] { cp.dct4(din, dout, false, 1, n, n); }));
    REQUIRE(throws_invalid([&] { cp.set_mdct_window(nullptr); }));
    REQUIRE(throws_invalid([&] { cp.mdct(din, dout, 1, 3 * n, 3 * n, n, 4, n, 4 * n); }));
  }
  (void)hipFree(din);
  (void)hipFree(dout);
  (void)hipStreamDestroy(stream);
  return 0;
}

int main(int argc, char** argv) {
  if (host_checks() != 0) return 1;
  if (argc > 1 && std::strcmp(argv[1], "host") == 0) return 0;
  // (helpers.REL_L2_TOL of the Python suite: 2e-6 / 5e-15)
  if (device_checks<float>(64, 5, 2e-6) != 0) return 1;
  if (device_checks<double>(64, 5, 5e-15) != 0) return 1;
  std::printf("dct4 facade OK\n");
  return 0;
}
