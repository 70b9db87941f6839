// C++ user-code test of the pair verbs through the facade: portfft::amd::real_descriptor<float> and <double> -> commit ->
// prepare_pairs -> convolve_pairs / correlate_pairs, against the direct sums in the program itself, in double precision,
//   convolve   r[l] = c N sum_n xe[n] ye[(l - n) mod N],   correlate   r[l] = c N sum_n xe[(n + l) mod N] ye[n],
//   c = forward_scale^2 backward_scale,
// at N = 64: 5 rows, x of N - 1 scalars and y of N / 2 + 1 (both extended with zeros by the kernel), N - 1 result scalars,
// odd and pairwise different pitches (the scalars between the rows must stay untouched), forward_scale 0.5 and
// backward_scale 1 / N.  The yardstick is the Python suite's: relative L2 per row <= REL_L2_TOL.  With the phase
// transform a row rotated by d against itself gives its peak at d.  A second call gives the same bits.  The verbs before
// prepare_pairs, the refusals of the C ABI and the verbs on a plan of the COMPLEX domain throw invalid_configuration.
//   hipcc -std=c++17 -I include tests/cpp/pairs_facade_test.cpp -L portfft_amd -lportfft_amd -o build/pairs_facade_test
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
  static_assert(std::is_same_v<decltype(std::declval<committed&>().prepare_pairs()), void>, "prepare_pairs takes no data");
  static_assert(std::is_same_v<decltype(std::declval<committed&>().convolve_pairs(
                                   std::declval<const float*>(), std::declval<const float*>(), std::declval<float*>(),
                                   std::size_t{5}, std::size_t{63}, std::size_t{65}, std::size_t{33}, std::size_t{67},
                                   std::size_t{63}, std::size_t{69}, std::vector<event>{})),
                               event>,
                "convolve_pairs reads two real buffers, writes one and returns the event");
  static_assert(std::is_same_v<decltype(std::declval<committed&>().correlate_pairs(
                                   std::declval<const float*>(), std::declval<const float*>(), std::declval<float*>(),
                                   std::size_t{5}, std::size_t{63}, std::size_t{65}, std::size_t{33}, std::size_t{67},
                                   std::size_t{63}, std::size_t{69}, std::vector<event>{}, 1e-3)),
                               event>,
                "correlate_pairs takes the floor of the phase transform last");
  // the convolving real plan has the same verbs; dependencies and floor are optional
  using rc = decltype(std::declval<amd::real_convolution_descriptor<double>&>().commit(std::declval<queue&>()));
  static_assert(std::is_same_v<decltype(std::declval<rc&>().correlate_pairs(std::declval<const double*>(), std::declval<const double*>(),
                                                                            std::declval<double*>(), std::size_t{1}, std::size_t{64},
                                                                            std::size_t{64}, std::size_t{64}, std::size_t{64},
                                                                            std::size_t{64}, std::size_t{64})),
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
  REQUIRE(pfft_plan_prepare_pairs(nullptr) == PFFT_INVALID_CONFIGURATION);
  REQUIRE(std::strstr(pfft_last_error(), "null plan") != nullptr);
  REQUIRE(pfft_execute_pairs(nullptr, PFFT_CORRELATE, nullptr, nullptr, nullptr, 1, 64, 64, 64, 64, 64, 64, 0.0) ==
          PFFT_INVALID_CONFIGURATION);
  REQUIRE(std::strstr(pfft_last_error(), "null plan") != nullptr);
  REQUIRE(pfft_execute_pairs_ex(nullptr, PFFT_CORRELATE, nullptr, nullptr, nullptr, 1, 64, 64, 64, 64, 64, 64, 0.0, 0, nullptr,
                                &ev) == PFFT_INVALID_CONFIGURATION);
  REQUIRE(std::strstr(pfft_last_error(), "null plan") != nullptr);
  REQUIRE(ev == nullptr);
  std::printf("pairs host checks OK\n");
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
int device_checks(std::size_t n, double tau) {
  using namespace portfft;
  hipStream_t stream;
  REQUIRE(hipStreamCreate(&stream) == hipSuccess);
  queue q(stream);
  const std::size_t rows = 5, xl = n - 1, yl = n / 2 + 1, ol = n - 1, xp = n + 1, yp = n + 3, op = n + 5;
  const T pad = static_cast<T>(-7);
  std::vector<T> x(rows * xp, pad), y(rows * yp, pad);
  for (std::size_t t = 0; t < rows; ++t) {
    for (std::size_t j = 0; j < xl; ++j) x[t * xp + j] = static_cast<T>(std::sin(0.37 * static_cast<double>(t * xl + j) + 0.1) + 0.25);
    for (std::size_t j = 0; j < yl; ++j) y[t * yp + j] = static_cast<T>(std::cos(0.23 * static_cast<double>(t * yl + j)) + 0.5);
  }
  T *dx, *dy, *dout;
  REQUIRE(hipMalloc(&dx, x.size() * sizeof(T)) == hipSuccess);
  REQUIRE(hipMalloc(&dy, y.size() * sizeof(T)) == hipSuccess);
  REQUIRE(hipMalloc(&dout, rows * op * sizeof(T)) == hipSuccess);
  REQUIRE(hipMemcpy(dx, x.data(), x.size() * sizeof(T), hipMemcpyHostToDevice) == hipSuccess);
  REQUIRE(hipMemcpy(dy, y.data(), y.size() * sizeof(T), hipMemcpyHostToDevice) == hipSuccess);
  amd::real_descriptor<T> desc(n);
  desc.forward_scale = static_cast<T>(0.5);
  desc.backward_scale = static_cast<T>(1.0 / static_cast<double>(n));
  auto plan = desc.commit(q);
  REQUIRE(throws_invalid([&] { plan.correlate_pairs(dx, dy, dout, rows, xl, xp, yl, yp, ol, op); }));  // not prepared
  REQUIRE(throws_invalid([&] { plan.convolve_pairs(dx, dy, dout, rows, xl, xp, yl, yp, ol, op); }));
  plan.prepare_pairs();
  plan.prepare_pairs();  // a second call does nothing
  // what the C ABI refuses, the facade throws
  REQUIRE(throws_invalid([&] { plan.correlate_pairs(dx, dy, dout, rows, n + 1, n + 1, yl, yp, ol, op); }));   // x_length above N
  REQUIRE(throws_invalid([&] { plan.correlate_pairs(dx, dy, dout, rows, xl, xl - 1, yl, yp, ol, op); }));     // x_pitch
  REQUIRE(throws_invalid([&] { plan.correlate_pairs(dx, dy, dout, 0, xl, xp, yl, yp, ol, op); }));            // no rows
  REQUIRE(throws_invalid([&] { plan.correlate_pairs(dx, dy, dx, rows, xl, xp, yl, yp, ol, xp); }));           // out == x
  REQUIRE(throws_invalid([&] { plan.correlate_pairs(dx, dy, dy, rows, xl, xp, yl, yp, ol, yp); }));           // out == y
  REQUIRE(throws_invalid([&] { plan.correlate_pairs(dx, dy, dout, rows, xl, xp, yl, yp, ol, op, {}, -1.0); }));  // floor
  REQUIRE(throws_invalid([&] { plan.correlate_pairs(nullptr, dy, dout, rows, xl, xp, yl, yp, ol, op); }));
  const double c = 0.25 / static_cast<double>(n) * static_cast<double>(n);  // forward_scale^2 backward_scale N
  for (int corr = 0; corr < 2; ++corr) {
    std::vector<T> first;
    for (int rep = 0; rep < 2; ++rep) {
      std::vector<T> got(rows * op, pad);
      REQUIRE(hipMemcpy(dout, got.data(), got.size() * sizeof(T), hipMemcpyHostToDevice) == hipSuccess);
      if (corr) {
        plan.correlate_pairs(dx, dy, dout, rows, xl, xp, yl, yp, ol, op).wait();
      } else {
        plan.convolve_pairs(dx, dy, dout, rows, xl, xp, yl, yp, ol, op).wait();
      }
      REQUIRE(hipMemcpy(got.data(), dout, got.size() * sizeof(T), hipMemcpyDeviceToHost) == hipSuccess);
      if (rep == 1) {
        REQUIRE(std::memcmp(first.data(), got.data(), got.size() * sizeof(T)) == 0);  // bit for bit
        break;
      }
      first = got;
      double worst = 0;
      for (std::size_t t = 0; t < rows; ++t) {
        double num = 0, den = 0;
        for (std::size_t l = 0; l < ol; ++l) {
          double want = 0;
          for (std::size_t j = 0; j < n; ++j) {  // xe, ye: zeros behind the lengths
            const std::size_t ix = corr ? (j + l) % n : j, iy = corr ? j : (l + n - j) % n;
            if (ix < xl && iy < yl) want += static_cast<double>(x[t * xp + ix]) * static_cast<double>(y[t * yp + iy]);
          }
          want *= c;
          const double d = want - static_cast<double>(got[t * op + l]);
          num += d * d;
          den += want * want;
        }
        for (std::size_t l = ol; l < op; ++l) REQUIRE(got[t * op + l] == pad);
        worst = std::max(worst, std::sqrt(num / den));
      }
      std::printf("N=%zu %s %s: %zu rows, worst rel-L2 of a row %.3e\n", n, sizeof(T) == 4 ? "f32" : "f64",
                  corr ? "correlate_pairs" : "convolve_pairs", rows, worst);
      REQUIRE(worst <= tau);
    }
  }
  // the phase transform: x = y rotated by d (full rows) has its peak at lag d, of height backward_scale * N = 1 at most
  {
    const std::size_t d = 5;
    std::vector<T> a(n), b(n), r(n);
    for (std::size_t j = 0; j < n; ++j) b[j] = static_cast<T>(std::sin(1.7 * static_cast<double>(j * j % 31)) + 0.3 * std::cos(0.9 * static_cast<double>(j)));
    for (std::size_t j = 0; j < n; ++j) a[(j + d) % n] = b[j];
    REQUIRE(hipMemcpy(dx, a.data(), n * sizeof(T), hipMemcpyHostToDevice) == hipSuccess);
    REQUIRE(hipMemcpy(dy, b.data(), n * sizeof(T), hipMemcpyHostToDevice) == hipSuccess);
    plan.correlate_pairs(dx, dy, dout, 1, n, n, n, n, n, n, {}, 1e-6).wait();
    REQUIRE(hipMemcpy(r.data(), dout, n * sizeof(T), hipMemcpyDeviceToHost) == hipSuccess);
    std::size_t at = 0;
    for (std::size_t j = 1; j < n; ++j) at = r[j] > r[at] ? j : at;
    std::printf("N=%zu %s phase transform: peak %.6f at lag %zu\n", n, sizeof(T) == 4 ? "f32" : "f64", static_cast<double>(r[at]), at);
    REQUIRE(at == d);
    REQUIRE(static_cast<double>(r[at]) > 0.9 && static_cast<double>(r[at]) < 1.0 + 1e-3);
    REQUIRE(hipMemcpy(dx, x.data(), x.size() * sizeof(T), hipMemcpyHostToDevice) == hipSuccess);
    REQUIRE(hipMemcpy(dy, y.data(), y.size() * sizeof(T), hipMemcpyHostToDevice) == hipSuccess);
  }
  // a copy shares the preparation; the inputs are what they were
  {
    auto twin = plan;
    twin.correlate_pairs(dx, dy, dout, rows, xl, xp, yl, yp, ol, op).wait();
    std::vector<T> after(x.size()), after_y(y.size());
    REQUIRE(hipMemcpy(after.data(), dx, after.size() * sizeof(T), hipMemcpyDeviceToHost) == hipSuccess);
    REQUIRE(hipMemcpy(after_y.data(), dy, after_y.size() * sizeof(T), hipMemcpyDeviceToHost) == hipSuccess);
    REQUIRE(std::memcmp(after.data(), x.data(), after.size() * sizeof(T)) == 0);
    REQUIRE(std::memcmp(after_y.data(), y.data(), after_y.size() * sizeof(T)) == 0);
  }
  // a plan of the COMPLEX domain refuses the verbs
  {
    descriptor<T, domain::COMPLEX> cd({n});
    auto cp = cd.commit(q);
    REQUIRE(throws_invalid([&] { cp.prepare_pairs(); }));
    REQUIRE(throws_invalid([&] { cp.convolve_pairs(dx, dy, dout, 1, n, n, n, n, n, n); }));
    REQUIRE(throws_invalid([&] { cp.correlate_pairs(dx, dy, dout, 1, n, n, n, n, n, n); }));
  }
  (void)hipFree(dx);
  (void)hipFree(dy);
  (void)hipFree(dout);
  (void)hipStreamDestroy(stream);
  return 0;
}

int main(int argc, char** argv) {
  if (host_checks() != 0) return 1;
  if (argc > 1 && std::strcmp(argv[1], "host") == 0) return 0;
  // (helpers.REL_L2_TOL of the Python suite: 2e-6 / 5e-15)
  if (device_checks<float>(64, 2e-6) != 0) return 1;
  if (device_checks<double>(64, 5e-15) != 0) return 1;
  std::printf("pairs facade OK\n");
  return 0;
}
