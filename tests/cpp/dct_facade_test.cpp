// C++ user-code test of the discrete cosine transforms through the facade: portfft::amd::real_descriptor<float> and
// <double> -> commit -> prepare_dct -> dct of type 2 and 3 against the direct sums
//   type 2:  y[k] = forward_scale  * 2 * sum_n x[n] cos(pi k (2n + 1) / (2N))
//   type 3:  y[n] = backward_scale * (x[0] + 2 * sum_{k >= 1} x[k] cos(pi k (2n + 1) / (2N)))
// in double precision with the argument reduced mod 4N in integers, at N = 64, 5 rows with odd pitches (the scalars between
// the rows must stay untouched) and in place; dct before prepare_dct and both verbs on a plan of the COMPLEX domain throw
// invalid_configuration.
//   hipcc -std=c++17 -I include tests/cpp/dct_facade_test.cpp -L portfft_amd -lportfft_amd -o build/dct_facade_test
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
  static_assert(std::is_same_v<decltype(std::declval<committed&>().prepare_dct()), void>, "prepare_dct takes no data");
  static_assert(std::is_same_v<decltype(std::declval<committed&>().dct(std::declval<const float*>(), std::declval<float*>(),
                                                                       PFFT_DCT_II, std::size_t{5}, std::size_t{67},
                                                                       std::size_t{71}, std::vector<event>{})),
                               event>,
                "the verb returns the event, like stft");
  // the convolving real plan has the same verbs; the dependencies are optional
  using rc = decltype(std::declval<amd::real_convolution_descriptor<double>&>().commit(std::declval<queue&>()));
  static_assert(std::is_same_v<decltype(std::declval<rc&>().dct(std::declval<const double*>(), std::declval<double*>(),
                                                                PFFT_DCT_III, std::size_t{1}, std::size_t{64}, std::size_t{64})),
                               event>,
                "on a real_convolution_descriptor's plan too");
  REQUIRE(PFFT_DCT_II == 2 && PFFT_DCT_III == 3);
  // no extension bit: 32 stays invalid
  pfft_desc_t c;
  REQUIRE(pfft_desc_init_real(&c, PFFT_PRECISION_F32, 64) == PFFT_OK);
  REQUIRE(c.extensions == PFFT_EXT_REAL_TRANSFORMS && pfft_desc_validate(&c) == PFFT_OK);
  c.extensions = 32;
  REQUIRE(pfft_desc_validate(&c) == PFFT_INVALID_CONFIGURATION);
  // the C entry points answer a null plan
  REQUIRE(pfft_plan_prepare_dct(nullptr) == PFFT_INVALID_CONFIGURATION);
  REQUIRE(std::strstr(pfft_last_error(), "null plan") != nullptr);
  REQUIRE(pfft_execute_dct(nullptr, PFFT_DCT_II, nullptr, nullptr, 1, 64, 64) == PFFT_INVALID_CONFIGURATION);
  REQUIRE(std::strstr(pfft_last_error(), "null plan") != nullptr);
  void* ev = nullptr;
  REQUIRE(pfft_execute_dct_ex(nullptr, PFFT_DCT_III, nullptr, nullptr, 1, 64, 64, 0, nullptr, &ev) == PFFT_INVALID_CONFIGURATION);
  REQUIRE(ev == nullptr);
  std::printf("dct host checks OK\n");
  return 0;
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
  {
    bool threw = false;
    try {
      plan.dct(din, dout, PFFT_DCT_II, rows, in_pitch, out_pitch);
    } catch (const invalid_configuration&) {
      threw = true;  // not prepared yet
    }
    REQUIRE(threw);
  }
  plan.prepare_dct();
  plan.prepare_dct();  // (idempotent)
  for (int type = PFFT_DCT_II; type <= PFFT_DCT_III; ++type) {
    for (int in_place = 0; in_place < 2; ++in_place) {
      const std::size_t op = in_place ? in_pitch : out_pitch;
      std::vector<T> got(rows * op, pad);
      T* dst = dout;
      if (in_place) {
        dst = din;
      } else {
        REQUIRE(hipMemcpy(dout, got.data(), got.size() * sizeof(T), hipMemcpyHostToDevice) == hipSuccess);
      }
      plan.dct(din, dst, type, rows, in_pitch, op).wait();
      REQUIRE(hipMemcpy(got.data(), dst, got.size() * sizeof(T), hipMemcpyDeviceToHost) == hipSuccess);
      if (in_place) REQUIRE(hipMemcpy(din, x.data(), x.size() * sizeof(T), hipMemcpyHostToDevice) == hipSuccess);
      double worst = 0;
      for (std::size_t r = 0; r < rows; ++r) {
        double num = 0, den = 0;
        for (std::size_t o = 0; o < n; ++o) {
          double s = 0;
          for (std::size_t i = 0; i < n; ++i) {
            // type 2: output k = o, input n = i; type 3: output n = o, input k = i
            const std::size_t k = type == PFFT_DCT_II ? o : i, j = type == PFFT_DCT_II ? i : o;
            const double c = std::cos(pi * static_cast<double>((k * (2 * j + 1)) % (4 * n)) / static_cast<double>(2 * n));
            const double a = (type == PFFT_DCT_III && i == 0) ? 1.0 : 2.0;
            s += a * static_cast<double>(x[r * in_pitch + i]) * c;
          }
          const double want = (type == PFFT_DCT_II ? 0.5 : 0.25) * s;
          const double d = want - static_cast<double>(got[r * op + o]);
          num += d * d;
          den += want * want;
        }
        for (std::size_t t = n; t < op; ++t) REQUIRE(got[r * op + t] == pad);
        worst = std::max(worst, std::sqrt(num / den));
      }
      std::printf("N=%zu rows=%zu %s type %d %s rel-L2 %.3e\n", n, rows, sizeof(T) == 4 ? "f32" : "f64", type,
                  in_place ? "in place" : "out of place", worst);
      REQUIRE(worst < tol);
    }
  }
  // a plan of the COMPLEX domain refuses both verbs
  {
    descriptor<T, domain::COMPLEX> cd({n});
    auto cp = cd.commit(q);
    int threw = 0;
    try {
      cp.prepare_dct();
    } catch (const invalid_configuration&) {
      ++threw;
    }
    try {
      cp.dct(din, dout, PFFT_DCT_II, 1, n, n);
    } catch (const invalid_configuration&) {
      ++threw;
    }
    REQUIRE(threw == 2);
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
  std::printf("dct facade OK\n");
  return 0;
}
