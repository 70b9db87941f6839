// C++ user-code test of real transforms through the facade: portfft::amd::real_descriptor<float> and <double> ->
// commit -> forward against a double-precision DFT of the real input, backward round trip (out of place and in place
// on padded rows); a plain REAL descriptor is still refused and a COMPLEX plan's real overloads still throw.
//   hipcc -std=c++17 -I include tests/cpp/real_facade_test.cpp -L portfft_amd -lportfft_amd -o build/real_facade_test
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
  amd::real_descriptor<float> desc(4096);
  desc.number_of_transforms = 3;
  REQUIRE(desc.forward_distance == 4096 && desc.backward_distance == 2049);
  REQUIRE(desc.get_input_count(direction::FORWARD) == 3 * 4096);
  REQUIRE(desc.get_output_count(direction::FORWARD) == 3 * 2049);
  static_assert(std::is_same_v<decltype(desc.commit(std::declval<queue&>())), committed_descriptor<float, domain::REAL>>,
                "a REAL plan");
  queue q;
  bool threw = false;
  try {
    amd::real_descriptor<double> odd(63);
    odd.commit(q);
  } catch (const unsupported_configuration&) {
    threw = true;
  }
  REQUIRE(threw);
  threw = false;
  try {
    descriptor<float, domain::REAL> plain({64});
    plain.commit(q);
  } catch (const unsupported_configuration&) {
    threw = true;
  }
  REQUIRE(threw);
  std::printf("real host checks OK\n");
  return 0;
}

template <typename T>
int device_checks(std::size_t n, std::size_t batch, double tol) {
  using namespace portfft;
  using C = std::complex<T>;
  const std::size_t bins = n / 2 + 1;
  std::vector<T> h(n * batch), back(n * batch);
  for (std::size_t i = 0; i < h.size(); ++i) h[i] = static_cast<T>(std::sin(0.37 * i + 0.1) + 0.5 * std::cos(1.7 * i));
  std::vector<C> r(bins * batch);
  T* din;
  C* dout;
  T* dback;
  REQUIRE(hipMalloc(&din, h.size() * sizeof(T)) == hipSuccess);
  REQUIRE(hipMalloc(&dout, r.size() * sizeof(C)) == hipSuccess);
  REQUIRE(hipMalloc(&dback, h.size() * sizeof(T)) == hipSuccess);
  REQUIRE(hipMemcpy(din, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice) == hipSuccess);
  hipStream_t stream;
  REQUIRE(hipStreamCreate(&stream) == hipSuccess);
  queue q(stream);
  amd::real_descriptor<T> desc(n);
  desc.number_of_transforms = batch;
  desc.backward_scale = static_cast<T>(1.0 / static_cast<double>(n));
  auto committed = desc.commit(q);
  committed.compute_forward(static_cast<const T*>(din), dout).wait();
  REQUIRE(hipMemcpy(r.data(), dout, r.size() * sizeof(C), hipMemcpyDeviceToHost) == hipSuccess);
  double worst = 0;
  for (std::size_t b = 0; b < batch; ++b) {
    double num = 0, den = 0;
    for (std::size_t k = 0; k < bins; ++k) {
      std::complex<double> s = 0;
      for (std::size_t i = 0; i < n; ++i) {
        s += static_cast<double>(h[b * n + i]) * std::polar(1.0, -2 * M_PI * double((i * k) % n) / double(n));
      }
      num += std::norm(s - std::complex<double>(r[b * bins + k]));
      den += std::norm(s);
    }
    worst = std::max(worst, std::sqrt(num / den));
  }
  std::printf("N=%zu batch=%zu %s forward rel-L2 %.3e\n", n, batch, sizeof(T) == 4 ? "f32" : "f64", worst);
  REQUIRE(worst < tol);
  committed.compute_backward(static_cast<const C*>(dout), dback).wait();
  REQUIRE(hipMemcpy(back.data(), dback, back.size() * sizeof(T), hipMemcpyDeviceToHost) == hipSuccess);
  double num = 0, den = 0;
  for (std::size_t i = 0; i < h.size(); ++i) {
    num += (double(back[i]) - double(h[i])) * (double(back[i]) - double(h[i]));
    den += double(h[i]) * double(h[i]);
  }
  std::printf("N=%zu batch=%zu round trip rel-L2 %.3e\n", n, batch, std::sqrt(num / den));
  REQUIRE(std::sqrt(num / den) < tol);
  // in place on padded rows: N scalars in N/2 + 1 complex slots
  amd::real_descriptor<T> ip(n);
  ip.number_of_transforms = batch;
  ip.placement = placement::IN_PLACE;
  ip.forward_distance = 2 * bins;
  auto cip = ip.commit(q);
  std::vector<T> padded(2 * bins * batch, T(0));
  for (std::size_t b = 0; b < batch; ++b) std::memcpy(&padded[b * 2 * bins], &h[b * n], n * sizeof(T));
  C* dip;
  REQUIRE(hipMalloc(&dip, bins * batch * sizeof(C)) == hipSuccess);
  REQUIRE(hipMemcpy(dip, padded.data(), padded.size() * sizeof(T), hipMemcpyHostToDevice) == hipSuccess);
  cip.compute_forward(reinterpret_cast<const T*>(dip), dip).wait();
  std::vector<C> r2(bins * batch);
  REQUIRE(hipMemcpy(r2.data(), dip, r2.size() * sizeof(C), hipMemcpyDeviceToHost) == hipSuccess);
  REQUIRE(std::memcmp(r2.data(), r.data(), r.size() * sizeof(C)) == 0);  // the same kernel on the same values
  // a COMPLEX plan's real overloads keep throwing
  descriptor<T, domain::COMPLEX> cd({n});
  auto cc = cd.commit(q);
  bool threw = false;
  try {
    cc.compute_forward(static_cast<const T*>(din), dout);
  } catch (const unsupported_configuration& e) {
    threw = std::strstr(e.what(), "Real to complex FFTs not yet implemented.") != nullptr;
  }
  REQUIRE(threw);
  threw = false;
  try {
    cc.compute_backward(static_cast<const C*>(dout), dback);
  } catch (const unsupported_configuration& e) {
    threw = std::strstr(e.what(), "Complex to real FFTs not yet implemented.") != nullptr;
  }
  REQUIRE(threw);
  (void)hipFree(din);
  (void)hipFree(dout);
  (void)hipFree(dback);
  (void)hipFree(dip);
  (void)hipStreamDestroy(stream);
  return 0;
}

int main(int argc, char** argv) {
  if (host_checks() != 0) return 1;
  if (argc > 1 && std::strcmp(argv[1], "host") == 0) return 0;
  if (device_checks<float>(64, 3, 2e-6) != 0) return 1;
  if (device_checks<float>(4096, 2, 2e-6) != 0) return 1;
  if (device_checks<double>(1000, 2, 5e-15) != 0) return 1;
  std::printf("real facade OK\n");
  return 0;
}
