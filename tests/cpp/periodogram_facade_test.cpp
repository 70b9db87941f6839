// C++ user-code test of the power spectrogram / periodogram through the facade: portfft::amd::real_descriptor<float> and
// <double> -> commit -> set_periodogram_window -> periodogram, against the direct sum in the program itself
//   P[i][c][k] = sum over f = c A ... min((c + 1) A, F) - 1 of | forward_scale * sum_n w[n] xe_i[f hop - lead + n] exp(-2 pi i k n / N) |^2
// in double precision with the argument reduced mod N in integers, at N = 64: 2 signals of 7 frames in rows of 3 (the last
// row holds one frame), an odd hop and lead, both extensions, odd pitches (the scalars between the rows and behind the
// signals must stay untouched), forward_scale 0.5.  The yardstick is the Python suite's for sums of squares: relative L1
// per row <= 2 tau + tau^2 + (A + 2) u with tau = REL_L2_TOL.  A second call gives the same bits.  The verb before its
// window, the refusals of the C ABI and both verbs on a plan of the COMPLEX domain throw invalid_configuration.
//   hipcc -std=c++17 -I include tests/cpp/periodogram_facade_test.cpp -L portfft_amd -lportfft_amd -o build/periodogram_facade_test
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
  static_assert(std::is_same_v<decltype(std::declval<committed&>().set_periodogram_window(std::declval<const float*>())), void>,
                "set_periodogram_window takes the window");
  static_assert(std::is_same_v<decltype(std::declval<committed&>().periodogram(
                                   std::declval<const float*>(), std::declval<float*>(), std::size_t{2}, std::size_t{300},
                                   std::size_t{301}, std::size_t{17}, std::size_t{31}, int32_t{PFFT_PAD_ZERO}, std::size_t{7},
                                   std::size_t{3}, std::size_t{35}, std::size_t{107}, std::vector<event>{})),
                               event>,
                "periodogram writes real scalars and returns the event, like stft");
  // the convolving real plan has the same verbs; the dependencies are optional
  using rc = decltype(std::declval<amd::real_convolution_descriptor<double>&>().commit(std::declval<queue&>()));
  static_assert(std::is_same_v<decltype(std::declval<rc&>().periodogram(std::declval<const double*>(), std::declval<double*>(),
                                                                        std::size_t{1}, std::size_t{300}, std::size_t{300},
                                                                        std::size_t{16}, std::size_t{0}, int32_t{PFFT_PAD_REFLECT},
                                                                        std::size_t{4}, std::size_t{4}, std::size_t{33},
                                                                        std::size_t{33})),
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
  REQUIRE(pfft_plan_set_periodogram_window(nullptr, nullptr) == PFFT_INVALID_CONFIGURATION);
  REQUIRE(std::strstr(pfft_last_error(), "null plan") != nullptr);
  REQUIRE(pfft_execute_periodogram(nullptr, nullptr, nullptr, 1, 300, 300, 16, 0, 0, 4, 2, 33, 66) == PFFT_INVALID_CONFIGURATION);
  REQUIRE(std::strstr(pfft_last_error(), "null plan") != nullptr);
  REQUIRE(pfft_execute_periodogram_ex(nullptr, nullptr, nullptr, 1, 300, 300, 16, 0, 0, 4, 2, 33, 66, 0, nullptr, &ev) ==
          PFFT_INVALID_CONFIGURATION);
  REQUIRE(std::strstr(pfft_last_error(), "null plan") != nullptr);
  REQUIRE(ev == nullptr);
  std::printf("periodogram host checks OK\n");
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
int device_checks(std::size_t n, double tau, double u) {
  using namespace portfft;
  const double pi = std::acos(-1.0);
  hipStream_t stream;
  REQUIRE(hipStreamCreate(&stream) == hipSuccess);
  queue q(stream);
  const std::size_t m = n / 2, n_sig = 2, frames = 7, avg = 3, rows = 3, hop = n / 4 + 1, lead = m - 1;
  // reflection admits (frames - 1) * hop + n <= length + 2 * lead; zeros then see the last frame run past the end
  const std::size_t length = (frames - 1) * hop + n - 2 * lead + 1, ip = length + 2, rp = m + 2, op = rows * rp + 3;
  const T pad = static_cast<T>(-7);
  std::vector<T> x(n_sig * ip, pad), w(n);
  for (std::size_t i = 0; i < n_sig; ++i) {
    for (std::size_t t = 0; t < length; ++t) x[i * ip + t] = static_cast<T>(std::sin(0.37 * static_cast<double>(i * length + t) + 0.1) + 0.25);
  }
  for (std::size_t j = 0; j < n; ++j) w[j] = static_cast<T>(0.5 + 0.4 * std::sin(0.13 * static_cast<double>(j)));
  T *dx, *dw, *dout;
  REQUIRE(hipMalloc(&dx, x.size() * sizeof(T)) == hipSuccess);
  REQUIRE(hipMalloc(&dw, w.size() * sizeof(T)) == hipSuccess);
  REQUIRE(hipMalloc(&dout, n_sig * op * sizeof(T)) == hipSuccess);
  REQUIRE(hipMemcpy(dx, x.data(), x.size() * sizeof(T), hipMemcpyHostToDevice) == hipSuccess);
  REQUIRE(hipMemcpy(dw, w.data(), w.size() * sizeof(T), hipMemcpyHostToDevice) == hipSuccess);
  amd::real_descriptor<T> desc(n);
  desc.forward_scale = static_cast<T>(0.5);
  auto plan = desc.commit(q);
  REQUIRE(throws_invalid([&] { plan.periodogram(dx, dout, n_sig, length, ip, hop, lead, PFFT_PAD_ZERO, frames, avg, rp, op); }));  // no window yet
  plan.set_window(dw);
  REQUIRE(throws_invalid([&] { plan.periodogram(dx, dout, n_sig, length, ip, hop, lead, PFFT_PAD_ZERO, frames, avg, rp, op); }));  // the STFT's window is another
  plan.set_periodogram_window(dw);
  // what the C ABI refuses, the facade throws
  REQUIRE(throws_invalid([&] { plan.periodogram(dx, dout, n_sig, length, ip, hop, n, PFFT_PAD_ZERO, frames, avg, rp, op); }));         // lead N
  REQUIRE(throws_invalid([&] { plan.periodogram(dx, dout, n_sig, length, ip, hop, lead, PFFT_PAD_ZERO, frames, 0, rp, op); }));        // avg 0
  REQUIRE(throws_invalid([&] { plan.periodogram(dx, dout, n_sig, length, ip, hop, lead, PFFT_PAD_ZERO, frames, frames + 1, rp, op); }));  // avg > F
  REQUIRE(throws_invalid([&] { plan.periodogram(dx, dout, n_sig, length, ip, hop, lead, PFFT_PAD_ZERO, frames, avg, m, op); }));       // row_pitch
  REQUIRE(throws_invalid([&] { plan.periodogram(dx, dout, n_sig, length, ip, hop, lead, PFFT_PAD_ZERO, frames, avg, rp, rows * rp - 1); }));  // out_pitch
  REQUIRE(throws_invalid([&] { plan.periodogram(dx, dx, 1, length, ip, hop, lead, PFFT_PAD_ZERO, 1, 1, rp, rp); }));                   // in place
  for (int32_t mode : {PFFT_PAD_ZERO, PFFT_PAD_REFLECT}) {
    std::vector<T> first;
    for (int rep = 0; rep < 2; ++rep) {
      std::vector<T> got(n_sig * op, pad);
      REQUIRE(hipMemcpy(dout, got.data(), got.size() * sizeof(T), hipMemcpyHostToDevice) == hipSuccess);
      plan.periodogram(dx, dout, n_sig, length, ip, hop, lead, mode, frames, avg, rp, op).wait();
      REQUIRE(hipMemcpy(got.data(), dout, got.size() * sizeof(T), hipMemcpyDeviceToHost) == hipSuccess);
      if (rep == 1) {
        REQUIRE(std::memcmp(first.data(), got.data(), got.size() * sizeof(T)) == 0);  // bit for bit
        break;
      }
      first = got;
      double worst = 0;
      for (std::size_t i = 0; i < n_sig; ++i) {
        for (std::size_t c = 0; c < rows; ++c) {
          double num = 0, den = 0;
          for (std::size_t k = 0; k <= m; ++k) {
            double want = 0;
            for (std::size_t f = c * avg; f < std::min((c + 1) * avg, frames); ++f) {  // ascending f
              double re = 0, im = 0;
              for (std::size_t j = 0; j < n; ++j) {
                long long p = static_cast<long long>(f * hop + j) - static_cast<long long>(lead);
                const long long last = static_cast<long long>(length) - 1;
                double v = 0;
                if (mode == PFFT_PAD_REFLECT) {
                  p = p < 0 ? -p : (p > last ? 2 * last - p : p);
                  v = static_cast<double>(x[i * ip + static_cast<std::size_t>(p)]);
                } else if (p >= 0 && p <= last) {
                  v = static_cast<double>(x[i * ip + static_cast<std::size_t>(p)]);
                }
                v *= static_cast<double>(w[j]);
                const double a = 2.0 * pi * static_cast<double>((k * j) % n) / static_cast<double>(n);
                re += v * std::cos(a);
                im -= v * std::sin(a);
              }
              want += 0.25 * (re * re + im * im);  // forward_scale squared
            }
            num += std::fabs(want - static_cast<double>(got[i * op + c * rp + k]));
            den += want;
          }
          for (std::size_t k = m + 1; k < rp; ++k) REQUIRE(got[i * op + c * rp + k] == pad);
          worst = std::max(worst, num / den);
        }
        for (std::size_t t = rows * rp; t < op; ++t) REQUIRE(got[i * op + t] == pad);
      }
      std::printf("N=%zu %s periodogram pad %d: %zu signals x %zu frames in rows of %zu, worst rel-L1 of a row %.3e\n", n,
                  sizeof(T) == 4 ? "f32" : "f64", static_cast<int>(mode), n_sig, frames, avg, worst);
      REQUIRE(worst <= 2 * tau + tau * tau + static_cast<double>(avg + 2) * u);
    }
  }
  // the signals are what they were
  {
    std::vector<T> after(x.size());
    REQUIRE(hipMemcpy(after.data(), dx, after.size() * sizeof(T), hipMemcpyDeviceToHost) == hipSuccess);
    REQUIRE(std::memcmp(after.data(), x.data(), after.size() * sizeof(T)) == 0);
  }
  // a plan of the COMPLEX domain refuses both verbs
  {
    descriptor<T, domain::COMPLEX> cd({n});
    auto cp = cd.commit(q);
    REQUIRE(throws_invalid([&] { cp.set_periodogram_window(nullptr); }));
    REQUIRE(throws_invalid([&] { cp.periodogram(dx, dout, 1, length, ip, hop, lead, PFFT_PAD_ZERO, 1, 1, rp, rp); }));
  }
  (void)hipFree(dx);
  (void)hipFree(dw);
  (void)hipFree(dout);
  (void)hipStreamDestroy(stream);
  return 0;
}

int main(int argc, char** argv) {
  if (host_checks() != 0) return 1;
  if (argc > 1 && std::strcmp(argv[1], "host") == 0) return 0;
  // (helpers.REL_L2_TOL of the Python suite: 2e-6 / 5e-15; u = 2^-24 / 2^-53)
  if (device_checks<float>(64, 2e-6, std::ldexp(1.0, -24)) != 0) return 1;
  if (device_checks<double>(64, 5e-15, std::ldexp(1.0, -53)) != 0) return 1;
  std::printf("periodogram facade OK\n");
  return 0;
}
