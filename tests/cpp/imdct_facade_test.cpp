// C++ user-code test of the inverse MDCT through the facade: portfft::amd::real_descriptor<float> and <double> -> commit ->
// set_imdct_window -> imdct, against the direct sum
//   y[i][t] = backward_scale * sum_f w[u - f N] * 2 * sum_k X[i][f][k] cos(pi (2 (u - f N) + 1 + N)(2k + 1) / (4N)),  u = t + lead
// over the frames with 0 <= u - f N < 2N, in double precision with the argument reduced mod 8N in integers, at N = 64:
// 2 signals of 5 frames with odd pitches (the scalars between the frames and behind the signals must stay untouched),
// lead N and a window off symmetry, the plan's own chunk and chunks of 2 frames, which must agree bit for bit.  The verbs
// before their window, the refusals of the C ABI (lead 2N, a frame pitch below N, overlapping buffers) and the three verbs
// on a plan of the COMPLEX domain throw invalid_configuration.
//   hipcc -std=c++17 -I include tests/cpp/imdct_facade_test.cpp -L portfft_amd -lportfft_amd -o build/imdct_facade_test
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
  static_assert(std::is_same_v<decltype(std::declval<committed&>().set_imdct_window(std::declval<const float*>())), void>,
                "set_imdct_window takes the window");
  static_assert(std::is_same_v<decltype(std::declval<const committed&>().imdct_chunk_frames(std::size_t{2}, std::size_t{8})), std::size_t>,
                "imdct_chunk_frames answers a count, on a const plan");
  static_assert(std::is_same_v<decltype(std::declval<committed&>().imdct(std::declval<const float*>(), std::declval<float*>(),
                                                                         std::size_t{2}, std::size_t{5}, std::size_t{67},
                                                                         std::size_t{341}, std::size_t{64}, std::size_t{300},
                                                                         std::size_t{303}, std::size_t{2}, std::vector<event>{})),
                               event>,
                "imdct returns the event, like istft");
  // the convolving real plan has the same verbs; chunk_frames and the dependencies are optional
  using rc = decltype(std::declval<amd::real_convolution_descriptor<double>&>().commit(std::declval<queue&>()));
  static_assert(std::is_same_v<decltype(std::declval<rc&>().imdct(std::declval<const double*>(), std::declval<double*>(),
                                                                  std::size_t{1}, std::size_t{4}, std::size_t{64}, std::size_t{256},
                                                                  std::size_t{64}, std::size_t{256}, std::size_t{256})),
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
  uint64_t chunk = 7;
  REQUIRE(pfft_plan_set_imdct_window(nullptr, nullptr) == PFFT_INVALID_CONFIGURATION);
  REQUIRE(std::strstr(pfft_last_error(), "null plan") != nullptr);
  REQUIRE(pfft_plan_imdct_chunk_frames(nullptr, 2, 8, &chunk) == PFFT_INVALID_CONFIGURATION);
  REQUIRE(std::strstr(pfft_last_error(), "null argument") != nullptr && chunk == 7);
  REQUIRE(pfft_execute_imdct(nullptr, nullptr, nullptr, 1, 4, 64, 256, 64, 256, 256, 0) == PFFT_INVALID_CONFIGURATION);
  REQUIRE(std::strstr(pfft_last_error(), "null plan") != nullptr);
  REQUIRE(pfft_execute_imdct_ex(nullptr, nullptr, nullptr, 1, 4, 64, 256, 64, 256, 256, 0, 0, nullptr, &ev) == PFFT_INVALID_CONFIGURATION);
  REQUIRE(std::strstr(pfft_last_error(), "null plan") != nullptr);
  REQUIRE(ev == nullptr);
  std::printf("imdct host checks OK\n");
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
int device_checks(std::size_t n, double tol) {
  using namespace portfft;
  const double pi = std::acos(-1.0);
  hipStream_t stream;
  REQUIRE(hipStreamCreate(&stream) == hipSuccess);
  queue q(stream);
  const std::size_t n_sig = 2, frames = 5, fp = n + 3, ip = frames * fp + 1, lead = n, length = 4 * n + n / 2 + 1, op = length + 2;
  const T pad = static_cast<T>(-7);
  std::vector<T> coeff(n_sig * ip, pad), w(2 * n);
  for (std::size_t i = 0; i < n_sig; ++i) {
    for (std::size_t f = 0; f < frames; ++f) {
      for (std::size_t k = 0; k < n; ++k) coeff[i * ip + f * fp + k] = static_cast<T>(std::sin(0.37 * ((i * frames + f) * n + k) + 0.1));
    }
  }
  for (std::size_t j = 0; j < 2 * n; ++j) w[j] = static_cast<T>(0.5 + 0.4 * std::sin(0.13 * j));
  T *dc, *dw, *dout;
  REQUIRE(hipMalloc(&dc, coeff.size() * sizeof(T)) == hipSuccess);
  REQUIRE(hipMalloc(&dw, w.size() * sizeof(T)) == hipSuccess);
  REQUIRE(hipMalloc(&dout, n_sig * op * sizeof(T)) == hipSuccess);
  REQUIRE(hipMemcpy(dc, coeff.data(), coeff.size() * sizeof(T), hipMemcpyHostToDevice) == hipSuccess);
  REQUIRE(hipMemcpy(dw, w.data(), w.size() * sizeof(T), hipMemcpyHostToDevice) == hipSuccess);
  amd::real_descriptor<T> desc(n);
  desc.forward_scale = static_cast<T>(0.5);
  desc.backward_scale = static_cast<T>(0.25);
  auto plan = desc.commit(q);
  REQUIRE(throws_invalid([&] { plan.imdct(dc, dout, n_sig, frames, fp, ip, lead, length, op); }));  // no window yet
  REQUIRE(throws_invalid([&] { plan.imdct_chunk_frames(n_sig, frames); }));
  plan.set_mdct_window(dw);
  REQUIRE(throws_invalid([&] { plan.imdct(dc, dout, n_sig, frames, fp, ip, lead, length, op); }));  // the analysis window is another
  plan.set_imdct_window(dw);
  const std::size_t own = plan.imdct_chunk_frames(n_sig, frames);
  REQUIRE(own >= 1 && own <= frames);
  // what the C ABI refuses, the facade throws
  REQUIRE(throws_invalid([&] { plan.imdct(dc, dout, n_sig, frames, fp, ip, 2 * n, length, op); }));     // lead 2N
  REQUIRE(throws_invalid([&] { plan.imdct(dc, dout, n_sig, frames, n - 1, ip, lead, length, op); }));   // frame_pitch
  REQUIRE(throws_invalid([&] { plan.imdct(dc, dout, n_sig, frames, fp, ip, lead, 5 * n + 1, op); }));   // uncovered samples
  REQUIRE(throws_invalid([&] { plan.imdct(dc, dc, 1, 1, n, n, lead, n, n); }));                         // in place
  std::vector<T> first;
  for (std::size_t chunk : {std::size_t{0}, std::size_t{2}}) {
    std::vector<T> got(n_sig * op, pad);
    REQUIRE(hipMemcpy(dout, got.data(), got.size() * sizeof(T), hipMemcpyHostToDevice) == hipSuccess);
    plan.imdct(dc, dout, n_sig, frames, fp, ip, lead, length, op, chunk).wait();
    REQUIRE(hipMemcpy(got.data(), dout, got.size() * sizeof(T), hipMemcpyDeviceToHost) == hipSuccess);
    double worst = 0;
    for (std::size_t i = 0; i < n_sig; ++i) {
      double num = 0, den = 0;
      for (std::size_t t = 0; t < length; ++t) {
        const std::size_t u = t + lead;
        double want = 0;
        for (std::size_t f = 0; f < frames; ++f) {  // ascending f
          if (u < f * n || u - f * n >= 2 * n) continue;
          const std::size_t j = u - f * n;
          double s = 0;
          for (std::size_t k = 0; k < n; ++k) {
            const double c = std::cos(pi * static_cast<double>(((2 * k + 1) * (2 * j + 1 + n)) % (8 * n)) / static_cast<double>(4 * n));
            s += 2.0 * static_cast<double>(coeff[i * ip + f * fp + k]) * c;
          }
          want += static_cast<double>(w[j]) * s;
        }
        want *= 0.25;
        const double d = want - static_cast<double>(got[i * op + t]);
        num += d * d;
        den += want * want;
      }
      for (std::size_t t = length; t < op; ++t) REQUIRE(got[i * op + t] == pad);
      worst = std::max(worst, std::sqrt(num / den));
    }
    std::printf("N=%zu %s imdct %zu signals x %zu frames chunk %zu rel-L2 %.3e\n", n, sizeof(T) == 4 ? "f32" : "f64", n_sig, frames,
                chunk, worst);
    REQUIRE(worst < tol);
    if (first.empty()) {
      first = got;
    } else {
      REQUIRE(std::memcmp(first.data(), got.data(), got.size() * sizeof(T)) == 0);  // bit for bit
    }
  }
  // the coefficients are what they were
  {
    std::vector<T> after(coeff.size());
    REQUIRE(hipMemcpy(after.data(), dc, after.size() * sizeof(T), hipMemcpyDeviceToHost) == hipSuccess);
    REQUIRE(std::memcmp(after.data(), coeff.data(), after.size() * sizeof(T)) == 0);
  }
  // a plan of the COMPLEX domain refuses the three verbs
  {
    descriptor<T, domain::COMPLEX> cd({n});
    auto cp = cd.commit(q);
    REQUIRE(throws_invalid([&] { cp.set_imdct_window(nullptr); }));
    REQUIRE(throws_invalid([&] { cp.imdct_chunk_frames(2, 8); }));
    REQUIRE(throws_invalid([&] { cp.imdct(dc, dout, 1, 4, n, 4 * n, n, 4 * n, 4 * n); }));
  }
  (void)hipFree(dc);
  (void)hipFree(dw);
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
  std::printf("imdct facade OK\n");
  return 0;
}
