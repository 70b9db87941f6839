// portfft/portfft.hpp -- header-only C++17 facade over the C ABI of portfft_amd.h.
//
// Gives C++ callers the reference's plan-and-commit interface unchanged in spirit:
//   portfft::descriptor<Scalar, Domain>           (/root/reference/src/portfft/descriptor.hpp:43-271)
//   portfft::committed_descriptor<Scalar, Domain> (/root/reference/src/portfft/committed_descriptor.hpp:46-315)
//   enums                                          (/root/reference/src/portfft/enums.hpp:25-38)
//   exceptions                                     (/root/reference/src/portfft/common/exceptions.hpp:32-77)
// with these substitutions: sycl::queue -> portfft::queue (a HIP stream), sycl::event -> portfft::event (a hipEvent_t
// recorded behind the submission: per-call completion, usable as a dependency of later calls), USM pointers -> HIP
// device pointers.  sycl::buffer overloads do not exist
// (HIP has no buffer/accessor model).  Link with -lportfft_amd.
#ifndef PORTFFT_PORTFFT_HPP
#define PORTFFT_PORTFFT_HPP

#include <complex>
#include <cstddef>
#include <functional>
#include <memory>
#include <numeric>
#include <sstream>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <vector>

#include "../portfft_amd.h"

namespace portfft {

enum class domain { REAL = PFFT_DOMAIN_REAL, COMPLEX = PFFT_DOMAIN_COMPLEX };
enum class complex_storage { INTERLEAVED_COMPLEX = PFFT_INTERLEAVED_COMPLEX, SPLIT_COMPLEX = PFFT_SPLIT_COMPLEX };
enum class placement { IN_PLACE = PFFT_IN_PLACE, OUT_OF_PLACE = PFFT_OUT_OF_PLACE };
enum class direction { FORWARD = PFFT_FORWARD, BACKWARD = PFFT_BACKWARD };
constexpr direction inv(direction dir) { return dir == direction::FORWARD ? direction::BACKWARD : direction::FORWARD; }

class base_error : public std::runtime_error {
 public:
  explicit base_error(const std::string& what) : std::runtime_error(what) {}
};
struct internal_error : public base_error {
  using base_error::base_error;
};
struct invalid_configuration : public base_error {
  using base_error::base_error;
};
struct unsupported_configuration : public base_error {
  using base_error::base_error;
};
struct out_of_local_memory_error : public unsupported_configuration {
  using unsupported_configuration::unsupported_configuration;
};
/// a HIP runtime call failed inside the library (the reference would surface a sycl::exception)
struct device_error : public base_error {
  using base_error::base_error;
};

namespace detail {
inline void check(pfft_status st) {
  if (st == PFFT_OK) return;
  const std::string msg = pfft_last_error();
  switch (st) {
    case PFFT_INVALID_CONFIGURATION:
      throw invalid_configuration(msg);
    case PFFT_UNSUPPORTED_CONFIGURATION:
      throw unsupported_configuration(msg);
    case PFFT_OUT_OF_LOCAL_MEMORY:
      throw out_of_local_memory_error(msg);
    case PFFT_HIP_ERROR:
      throw device_error(msg);
    default:
      throw internal_error(msg);
  }
}

inline std::vector<std::size_t> get_default_strides(const std::vector<std::size_t>& lengths) {
  std::vector<std::size_t> strides(lengths.size());
  std::size_t total = 1;
  for (std::size_t i = lengths.size(); i-- > 0;) {
    strides[i] = total;
    total *= lengths[i];
  }
  return strides;
}

/// the Scalar types a descriptor takes: float, double, and _Float16 -- fp16 storage computed in fp32
/// (PFFT_PRECISION_F16: 1-D PACKED COMPLEX transforms only; std::is_floating_point_v<_Float16> is false)
template <typename Scalar>
inline constexpr bool is_scalar_v =
    std::is_same_v<Scalar, float> || std::is_same_v<Scalar, double> || std::is_same_v<Scalar, _Float16>;
/// type of a descriptor's forward_scale / backward_scale: float for _Float16 (1/24000 as _Float16 is subnormal, about
/// 1e-3 off -- worse than the output rounding), Scalar otherwise
template <typename Scalar>
using scale_type_t = std::conditional_t<std::is_same_v<Scalar, _Float16>, float, Scalar>;
template <typename Scalar>
inline constexpr int32_t precision_v = std::is_same_v<Scalar, double>     ? PFFT_PRECISION_F64
                                       : std::is_same_v<Scalar, _Float16> ? PFFT_PRECISION_F16
                                                                          : PFFT_PRECISION_F32;
}  // namespace detail

template <typename Scalar, domain Domain>
class committed_descriptor;
class queue;

/// Stands where the reference returns a sycl::event: the completion of ONE submission.  Owns a hipEvent_t recorded
/// on the plan's stream behind the last kernel of the compute_* call that returned it; copies share it.  wait()
/// blocks the host until that submission has finished (hipEventSynchronize); passing the event in another call's
/// `dependencies` orders that call behind it on the device (hipStreamWaitEvent), also across streams.  A
/// default-constructed event is already complete.  native() is the hipEvent_t for direct HIP interop.
class event {
 public:
  event() = default;
  void wait() const {
    if (ev_) detail::check(pfft_event_wait(ev_.get()));
  }
  /// sycl::event::wait_and_throw(): errors surface as exceptions from wait() already
  void wait_and_throw() const { wait(); }
  /// true once the submission has finished (info::event_command_status::complete in the reference's world)
  bool is_complete() const {
    int32_t done = 1;
    if (ev_) detail::check(pfft_event_query(ev_.get(), &done));
    return done != 0;
  }
  void* native() const { return ev_.get(); }
  /// sycl::event::wait(const std::vector<event>&)
  static void wait(const std::vector<event>& events) {
    for (const event& e : events) e.wait();
  }

 private:
  template <typename S, domain D>
  friend class committed_descriptor;
  friend class queue;
  explicit event(void* hip_event) : ev_(hip_event, [](void* e) { (void)pfft_event_destroy(e); }) {}
  std::shared_ptr<void> ev_;
};

/// Stands where the reference takes a sycl::queue: an in-order HIP stream (nullptr = the default stream).  copy()
/// and wait() are the two queue members the reference's own callers use around compute_* (test/unit_test/
/// fft_test_utils.hpp:286-333, test/bench/portfft/launch_bench.hpp:96-135).
class queue {
 public:
  queue() = default;
  explicit queue(void* hip_stream) : stream_(hip_stream) {}
  void* native() const { return stream_; }

  /// sycl::queue::copy(src, dest, count, dependencies): asynchronous on this stream, any combination of host and
  /// device pointers; the returned event completes with the copy
  template <typename T>
  event copy(const T* src, T* dest, std::size_t count, const std::vector<event>& dependencies = {}) {
    std::vector<void*> deps;
    deps.reserve(dependencies.size());
    for (const event& e : dependencies) deps.push_back(e.native());
    void* ev = nullptr;
    detail::check(pfft_queue_copy(stream_, src, dest, count * sizeof(T), static_cast<int32_t>(deps.size()), deps.data(),
                                  &ev));
    return event(ev);
  }
  /// sycl::queue::wait() / wait_and_throw()
  void wait() const { detail::check(pfft_queue_wait(stream_)); }
  void wait_and_throw() const { wait(); }

 private:
  void* stream_ = nullptr;
};

template <typename Scalar, domain Domain>
struct descriptor;
namespace amd {
template <typename Scalar>
struct real_descriptor;
template <typename Scalar>
struct any_length_descriptor;
template <typename Scalar>
struct convolution_descriptor;
template <typename Scalar>
struct real_convolution_descriptor;
}

template <typename Scalar, domain Domain>
class committed_descriptor {
  static_assert(detail::is_scalar_v<Scalar>, "Scalar must be float, double or _Float16");
  friend struct descriptor<Scalar, Domain>;
  friend struct amd::real_descriptor<Scalar>;
  friend struct amd::any_length_descriptor<Scalar>;
  friend struct amd::convolution_descriptor<Scalar>;
  friend struct amd::real_convolution_descriptor<Scalar>;
  std::shared_ptr<pfft_plan_t> plan_;

  static std::shared_ptr<pfft_plan_t> own(pfft_plan_t* p) {
    return std::shared_ptr<pfft_plan_t>(p, [](pfft_plan_t* x) { (void)pfft_plan_destroy(x); });
  }

  committed_descriptor(const pfft_desc_t& d, queue& q) {
    pfft_plan_t* p = nullptr;
    detail::check(pfft_plan_create(&d, q.native(), &p));
    plan_ = own(p);
  }

  static std::vector<void*> natives(const std::vector<event>& dependencies) {
    std::vector<void*> deps;
    deps.reserve(dependencies.size());
    for (const event& e : dependencies) deps.push_back(e.native());
    return deps;
  }

  /// convolve_pairs / correlate_pairs: one call of pfft_execute_pairs_ex
  event pairs(int32_t mode, const Scalar* x, const Scalar* y, Scalar* out, std::size_t n_rows,
              std::size_t x_length, std::size_t x_pitch, std::size_t y_length, std::size_t y_pitch, std::size_t out_length,
              std::size_t out_pitch, double phat_floor, const std::vector<event>& dependencies) {
    const std::vector<void*> deps = natives(dependencies);
    void* ev = nullptr;
    detail::check(pfft_execute_pairs_ex(plan_.get(), mode, x, y, out, n_rows, x_length, x_pitch, y_length, y_pitch,
                                        out_length, out_pitch, phat_floor, static_cast<int32_t>(deps.size()), deps.data(),
                                        &ev));
    return event(ev);
  }

  event run(direction dir, const void* in, void* out, const std::vector<event>& dependencies) {
    const std::vector<void*> deps = natives(dependencies);
    void* ev = nullptr;
    detail::check(pfft_execute_ex(plan_.get(), static_cast<int32_t>(dir), in, out, static_cast<int32_t>(deps.size()),
                                  deps.data(), &ev));
    return event(ev);
  }
  event run_conv(int32_t mode, const void* in, void* out, const std::vector<event>& dependencies) {
    const std::vector<void*> deps = natives(dependencies);
    void* ev = nullptr;
    detail::check(pfft_execute_convolve_ex(plan_.get(), mode, in, out, static_cast<int32_t>(deps.size()), deps.data(), &ev));
    return event(ev);
  }
  event run_filter(int32_t mode, const void* in, void* out, std::size_t n_signals, std::size_t in_length,
                   std::size_t in_pitch, std::size_t out_length, std::size_t out_pitch,
                   const std::vector<event>& dependencies) {
    const std::vector<void*> deps = natives(dependencies);
    void* ev = nullptr;
    detail::check(pfft_execute_filter_ex(plan_.get(), mode, in, out, n_signals, in_length, in_pitch, out_length, out_pitch,
                                         static_cast<int32_t>(deps.size()), deps.data(), &ev));
    return event(ev);
  }
  /// the verbs on real scalars belong to plans of the REAL domain (`mode` is handed through)
  static int32_t real_only(int32_t mode) {
    if constexpr (Domain != domain::REAL) {
      throw invalid_configuration("real scalars were handed to a plan of the COMPLEX domain (real_convolution_descriptor)");
    }
    return mode;
  }
  /// set_window / stft / set_synthesis_window / istft / prepare_dct / dct / prepare_dct4 / dct4 / set_mdct_window / mdct /
  /// set_imdct_window / imdct / set_periodogram_window / periodogram / prepare_pairs / convolve_pairs / correlate_pairs
  /// belong to plans of the REAL domain
  static void real_plan_only(const char* verb) {
    if constexpr (Domain != domain::REAL) {
      throw invalid_configuration(std::string(verb) + ": the plan is of the COMPLEX domain (the verb belongs to "
                                  "real_descriptor and real_convolution_descriptor)");
    }
    (void)verb;
  }
  event run_split(direction dir, const void* ir, const void* ii, void* outr, void* outi,
                  const std::vector<event>& dependencies) {
    const std::vector<void*> deps = natives(dependencies);
    void* ev = nullptr;
    detail::check(pfft_execute_split_ex(plan_.get(), static_cast<int32_t>(dir), ir, ii, outr, outi,
                                        static_cast<int32_t>(deps.size()), deps.data(), &ev));
    return event(ev);
  }

 public:
  using complex_type = std::complex<Scalar>;
  using scalar_type = Scalar;

  /// Copies share the kernels and twiddle tables and get scratch memory of their own, like the reference's
  /// (committed_descriptor_impl.hpp:774-817): two copies can execute concurrently on two host threads / streams.
  committed_descriptor(const committed_descriptor& other) {
    pfft_plan_t* p = nullptr;
    detail::check(pfft_plan_clone(other.plan_.get(), &p));
    plan_ = own(p);
  }
  committed_descriptor& operator=(const committed_descriptor& other) {
    if (this != &other) {
      pfft_plan_t* p = nullptr;
      detail::check(pfft_plan_clone(other.plan_.get(), &p));
      plan_ = own(p);
    }
    return *this;
  }
  committed_descriptor(committed_descriptor&&) noexcept = default;
  committed_descriptor& operator=(committed_descriptor&&) noexcept = default;

  // Signatures of the USM overloads follow committed_descriptor.hpp:171-310 argument for argument:
  // `dependencies` are events that must complete before the computation starts; the returned event completes with
  // this computation.

  /// in-place, interleaved (committed_descriptor.hpp:171-176 / 215-218)
  event compute_forward(complex_type* inout, const std::vector<event>& dependencies = {}) {
    return run(direction::FORWARD, inout, inout, dependencies);
  }
  event compute_backward(complex_type* inout, const std::vector<event>& dependencies = {}) {
    return run(direction::BACKWARD, inout, inout, dependencies);
  }
  /// in-place, split (committed_descriptor.hpp:186-192 / 228-232)
  event compute_forward(scalar_type* inout_real, scalar_type* inout_imag,
                        const std::vector<event>& dependencies = {}) {
    return run_split(direction::FORWARD, inout_real, inout_imag, inout_real, inout_imag, dependencies);
  }
  event compute_backward(scalar_type* inout_real, scalar_type* inout_imag,
                         const std::vector<event>& dependencies = {}) {
    return run_split(direction::BACKWARD, inout_real, inout_imag, inout_real, inout_imag, dependencies);
  }
  /// out-of-place, interleaved (committed_descriptor.hpp:242-246 / 288-293)
  event compute_forward(const complex_type* in, complex_type* out, const std::vector<event>& dependencies = {}) {
    return run(direction::FORWARD, in, out, dependencies);
  }
  event compute_backward(const complex_type* in, complex_type* out, const std::vector<event>& dependencies = {}) {
    return run(direction::BACKWARD, in, out, dependencies);
  }
  /// out-of-place, split (committed_descriptor.hpp:258-263 / 305-310)
  event compute_forward(const scalar_type* in_real, const scalar_type* in_imag, scalar_type* out_real,
                        scalar_type* out_imag, const std::vector<event>& dependencies = {}) {
    return run_split(direction::FORWARD, in_real, in_imag, out_real, out_imag, dependencies);
  }
  event compute_backward(const scalar_type* in_real, const scalar_type* in_imag, scalar_type* out_real,
                         scalar_type* out_imag, const std::vector<event>& dependencies = {}) {
    return run_split(direction::BACKWARD, in_real, in_imag, out_real, out_imag, dependencies);
  }
  /// real-to-complex entry points exist in the reference only to throw (committed_descriptor.hpp:134-137,273-278), and
  /// on a COMPLEX plan they still do.  A REAL plan -- committed through portfft::amd::real_descriptor, an extension --
  /// runs the transform: N scalars in, N/2 + 1 bins out, and the reverse.  In place (padded rows): pass the one buffer
  /// through both arguments, compute_forward(reinterpret_cast<const scalar_type*>(p), reinterpret_cast<complex_type*>(p)).
  event compute_forward(const scalar_type* in, complex_type* out, const std::vector<event>& dependencies = {}) {
    if constexpr (Domain == domain::REAL) {
      return run(direction::FORWARD, in, out, dependencies);
    } else {
      throw unsupported_configuration("Real to complex FFTs not yet implemented.");
    }
  }
  event compute_backward(const complex_type* in, scalar_type* out, const std::vector<event>& dependencies = {}) {
    if constexpr (Domain == domain::REAL) {
      return run(direction::BACKWARD, in, out, dependencies);
    } else {
      throw unsupported_configuration("Complex to real FFTs not yet implemented.");
    }
  }

  /// Fused circular convolution (no reference equivalent): the verbs of a plan committed through
  /// portfft::amd::convolution_descriptor; on any other plan they throw invalid_configuration.
  /// set_filter: `spectra` points at n_filters * N elements in device memory, packed, in the frequency domain (what
  /// compute_forward of this plan makes of a filter).  They are copied on the plan's stream into memory the plan owns:
  /// the caller's buffer may be rewritten once the stream has passed the copy, executes submitted earlier keep their
  /// filter.  Row t of an execute uses filter t mod n_filters.  Copies of the plan share the filter until either sets another.
  void set_filter(const complex_type* spectra, std::size_t n_filters = 1) {
    detail::check(pfft_plan_set_filter(plan_.get(), spectra, static_cast<uint64_t>(n_filters)));
  }
  /// out[t] = forward_scale * backward_scale * N * IDFT(DFT(in[t]) . H[t mod n_filters]) in one kernel: what
  /// compute_forward, a multiply and compute_backward produce.  `in` is laid out as the forward domain, `out` as the
  /// backward domain.  Before the first set_filter: invalid_configuration.
  event convolve(complex_type* inout, const std::vector<event>& dependencies = {}) {
    return run_conv(PFFT_CONVOLVE, inout, inout, dependencies);
  }
  event convolve(const complex_type* in, complex_type* out, const std::vector<event>& dependencies = {}) {
    return run_conv(PFFT_CONVOLVE, in, out, dependencies);
  }
  /// the same with conj(H): the adjoint of convolve, what a backward pass through a convolution needs
  event correlate(complex_type* inout, const std::vector<event>& dependencies = {}) {
    return run_conv(PFFT_CORRELATE, inout, inout, dependencies);
  }
  event correlate(const complex_type* in, complex_type* out, const std::vector<event>& dependencies = {}) {
    return run_conv(PFFT_CORRELATE, in, out, dependencies);
  }

  /// Overlap-save FIR filtering of long signals (no reference equivalent; plans of convolution_descriptor).
  /// set_filter_taps: `taps` points at n_filters * n_taps elements in device memory, packed, in the time domain,
  /// 1 <= n_taps <= N.  The plan zero-pads every filter to N and transforms it on the device, unscaled; the spectra
  /// become the plan's filter as with set_filter (convolve / correlate on them: circular convolution with the padded taps).
  void set_filter_taps(const complex_type* taps, std::size_t n_taps, std::size_t n_filters = 1) {
    detail::check(pfft_plan_set_filter_taps(plan_.get(), taps, static_cast<uint64_t>(n_taps), static_cast<uint64_t>(n_filters)));
  }
  /// filter: `mode` PFFT_CONVOLVE: y_i[n] = c * sum_k h_i[k] x_i[n - k], n < out_length <= in_length + n_taps - 1;
  /// PFFT_CORRELATE: y_i[n] = c * sum_k conj(h_i[k]) x_i[n + k], n < out_length <= in_length; c = forward_scale *
  /// backward_scale * N, h_i the taps of filter i mod n_filters, x_i zero outside its in_length samples.  Signal i
  /// starts i * in_pitch (out: i * out_pitch) elements behind `in` (`out`); one kernel launch, the buffers must not
  /// overlap.  Needs set_filter_taps; the descriptor's batch, distances and offsets do not apply.
  event filter(int32_t mode, const complex_type* in, complex_type* out, std::size_t n_signals, std::size_t in_length,
               std::size_t in_pitch, std::size_t out_length, std::size_t out_pitch,
               const std::vector<event>& dependencies = {}) {
    return run_filter(mode, in, out, n_signals, in_length, in_pitch, out_length, out_pitch, dependencies);
  }

  /// The same verbs on REAL data (no reference equivalent): a plan committed through
  /// portfft::amd::real_convolution_descriptor.  set_filter (above) takes n_filters * (N / 2 + 1) bins per filter, what
  /// compute_forward of this plan with scale 1 makes of a real filter of N scalars.  convolve / correlate: out[t] =
  /// forward_scale * backward_scale * N * irfft(rfft(in[t]) . H[t mod n_filters]) (conj(H) for correlate); `in` AND
  /// `out` are rows of N real scalars laid out as the forward domain.  set_filter_taps: n_filters * n_taps real scalars.
  /// filter: the definitions above with real x, h, y; lengths and pitches count scalars, n_taps <= N - 2.  On a plan of
  /// the COMPLEX domain these overloads throw invalid_configuration.
  event convolve(scalar_type* inout, const std::vector<event>& dependencies = {}) {
    return run_conv(real_only(PFFT_CONVOLVE), inout, inout, dependencies);
  }
  event convolve(const scalar_type* in, scalar_type* out, const std::vector<event>& dependencies = {}) {
    return run_conv(real_only(PFFT_CONVOLVE), in, out, dependencies);
  }
  event correlate(scalar_type* inout, const std::vector<event>& dependencies = {}) {
    return run_conv(real_only(PFFT_CORRELATE), inout, inout, dependencies);
  }
  event correlate(const scalar_type* in, scalar_type* out, const std::vector<event>& dependencies = {}) {
    return run_conv(real_only(PFFT_CORRELATE), in, out, dependencies);
  }
  void set_filter_taps(const scalar_type* taps, std::size_t n_taps, std::size_t n_filters = 1) {
    (void)real_only(0);
    detail::check(pfft_plan_set_filter_taps(plan_.get(), taps, static_cast<uint64_t>(n_taps), static_cast<uint64_t>(n_filters)));
  }
  event filter(int32_t mode, const scalar_type* in, scalar_type* out, std::size_t n_signals, std::size_t in_length,
               std::size_t in_pitch, std::size_t out_length, std::size_t out_pitch,
               const std::vector<event>& dependencies = {}) {
    return run_filter(real_only(mode), in, out, n_signals, in_length, in_pitch, out_length, out_pitch, dependencies);
  }

  /// Short-time Fourier transform of long real signals (no reference equivalent): verbs of every committed descriptor
  /// of the REAL domain (amd::real_descriptor, amd::real_convolution_descriptor); on a COMPLEX plan they throw
  /// invalid_configuration.  set_window: `window` points at N real scalars in device memory, nullptr = all ones; copied
  /// on the plan's stream into memory the plan owns (the rules of set_filter); the first call resolves the kernel.
  /// stft: X_i[f][k] = forward_scale * sum_n w[n] xe_i[f * hop - lead + n] exp(-2 pi i k n / N) for f < n_frames, k <= N / 2,
  /// xe_i the signal extended by zeros (PFFT_PAD_ZERO) or by reflection (PFFT_PAD_REFLECT); signal i starts i * in_pitch
  /// scalars behind `in`, bin k of frame f of signal i goes to out + i * out_pitch + f * frame_pitch + k; one kernel
  /// launch, the buffers must not overlap.  The descriptor's batch, distances and offsets do not apply.
  void set_window(const scalar_type* window) {
    real_plan_only("set_window");
    detail::check(pfft_plan_set_window(plan_.get(), window));
  }
  event stft(const scalar_type* in, complex_type* out, std::size_t n_signals, std::size_t in_length, std::size_t in_pitch,
             std::size_t hop, std::size_t lead, int32_t pad_mode, std::size_t n_frames, std::size_t frame_pitch,
             std::size_t out_pitch, const std::vector<event>& dependencies = {}) {
    real_plan_only("stft");
    const std::vector<void*> deps = natives(dependencies);
    void* ev = nullptr;
    detail::check(pfft_execute_stft_ex(plan_.get(), in, out, n_signals, in_length, in_pitch, hop, lead, pad_mode, n_frames,
                                       frame_pitch, out_pitch, static_cast<int32_t>(deps.size()), deps.data(), &ev));
    return event(ev);
  }

  /// Inverse short-time Fourier transform (overlap-add synthesis), the counterpart of set_window / stft on the same
  /// descriptors.  set_synthesis_window: N real scalars in device memory, nullptr = all ones, independent of set_window.
  /// istft: y_i[t] = sum_f w[u - f * hop] * g_i[f][u - f * hop], u = t + lead, g_i[f] = backward_scale * N * irfft of the
  /// N / 2 + 1 bins at in + i * in_pitch + f * frame_pitch; PFFT_ISTFT_NORMALIZE divides by sum_f w[u - f * hop]^2 (0 where
  /// that is not above PFFT_ISTFT_ENV_MIN).  Sample t of signal i goes to out + i * out_pitch + t; one kernel launch, plain
  /// stores, the sums in ascending f whatever chunk_frames is (0: the plan chooses); the buffers must not overlap.
  void set_synthesis_window(const scalar_type* window) {
    real_plan_only("set_synthesis_window");
    detail::check(pfft_plan_set_synthesis_window(plan_.get(), window));
  }
  event istft(const complex_type* in, scalar_type* out, std::size_t n_signals, std::size_t n_frames, std::size_t frame_pitch,
              std::size_t in_pitch, std::size_t hop, std::size_t lead, int32_t mode, std::size_t out_length,
              std::size_t out_pitch, std::size_t chunk_frames = 0, const std::vector<event>& dependencies = {}) {
    real_plan_only("istft");
    const std::vector<void*> deps = natives(dependencies);
    void* ev = nullptr;
    detail::check(pfft_execute_istft_ex(plan_.get(), in, out, n_signals, n_frames, frame_pitch, in_pitch, hop, lead, mode,
                                        out_length, out_pitch, chunk_frames, static_cast<int32_t>(deps.size()), deps.data(),
                                        &ev));
    return event(ev);
  }

  /// Discrete cosine transforms of packed real rows on the same descriptors.  prepare_dct: resolves the kernels and uploads
  /// their twiddles, once; takes no data.  dct: type PFFT_DCT_II (y = forward_scale * scipy.fft.dct(x, 2)) or PFFT_DCT_III
  /// (y = backward_scale * scipy.fft.dct(x, 3)) of n_rows rows of N scalars, row t at in + t * in_pitch and
  /// out + t * out_pitch (pitches in scalars, at least N); one kernel launch; in == out with equal pitches is in place.
  void prepare_dct() {
    real_plan_only("prepare_dct");
    detail::check(pfft_plan_prepare_dct(plan_.get()));
  }
  event dct(const scalar_type* in, scalar_type* out, int32_t type, std::size_t n_rows, std::size_t in_pitch,
            std::size_t out_pitch, const std::vector<event>& dependencies = {}) {
    real_plan_only("dct");
    const std::vector<void*> deps = natives(dependencies);
    void* ev = nullptr;
    detail::check(pfft_execute_dct_ex(plan_.get(), type, in, out, n_rows, in_pitch, out_pitch,
                                      static_cast<int32_t>(deps.size()), deps.data(), &ev));
    return event(ev);
  }

  /// DCT-IV of packed real rows and MDCT of real signals on the same descriptors.  prepare_dct4: resolves the kernels and
  /// uploads their twiddles, once; takes no data.  dct4: y = forward_scale (inverse: backward_scale) * scipy.fft.dct(x, 4)
  /// of n_rows rows of N scalars, row t at in + t * in_pitch and out + t * out_pitch (pitches in scalars, at least N); one
  /// kernel launch; in == out with equal pitches is in place; dct4 of dct4 of x is 2N * x with scales of 1.
  void prepare_dct4() {
    real_plan_only("prepare_dct4");
    detail::check(pfft_plan_prepare_dct4(plan_.get()));
  }
  event dct4(const scalar_type* in, scalar_type* out, bool inverse, std::size_t n_rows, std::size_t in_pitch,
             std::size_t out_pitch, const std::vector<event>& dependencies = {}) {
    real_plan_only("dct4");
    const std::vector<void*> deps = natives(dependencies);
    void* ev = nullptr;
    detail::check(pfft_execute_dct4_ex(plan_.get(), inverse ? 1 : 0, in, out, n_rows, in_pitch, out_pitch,
                                       static_cast<int32_t>(deps.size()), deps.data(), &ev));
    return event(ev);
  }
  /// set_mdct_window: what prepare_dct4 does, then the 2N scalars of `window` (device memory; nullptr: ones) are copied
  /// into memory the plan owns.  mdct: frame f of signal i covers the 2N samples from f * N - lead of the signal extended
  /// by zeros (the hop is N; lead in [0, 2N), usually N); its N coefficients go to out + i * out_pitch + f * frame_pitch
  /// (all in scalars); one kernel launch; not in place.  The inverse is imdct.
  void set_mdct_window(const scalar_type* window) {
    real_plan_only("set_mdct_window");
    detail::check(pfft_plan_set_mdct_window(plan_.get(), window));
  }
  event mdct(const scalar_type* in, scalar_type* out, std::size_t n_signals, std::size_t in_length, std::size_t in_pitch,
             std::size_t lead, std::size_t n_frames, std::size_t frame_pitch, std::size_t out_pitch,
             const std::vector<event>& dependencies = {}) {
    real_plan_only("mdct");
    const std::vector<void*> deps = natives(dependencies);
    void* ev = nullptr;
    detail::check(pfft_execute_mdct_ex(plan_.get(), in, out, n_signals, in_length, in_pitch, lead, n_frames, frame_pitch,
                                       out_pitch, static_cast<int32_t>(deps.size()), deps.data(), &ev));
    return event(ev);
  }

  /// Inverse MDCT on the same descriptors.  set_imdct_window: what prepare_dct4 does, the kernel resolved at the first call,
  /// then the 2N scalars of `window` (device memory; nullptr: ones) copied into memory the plan owns; independent of
  /// set_mdct_window.  imdct: y_i[t] = backward_scale * sum_f w[u - f * N] * g_i[f][u - f * N], u = t + lead, g_i[f] the unfolded
  /// frame [q, -reverse(q), -reverse(p), -p] of [p, q] = the unscaled dct4 of the N coefficients at in + i * in_pitch +
  /// f * frame_pitch.  Sample t of signal i goes to out + i * out_pitch + t (all in scalars); one kernel launch, plain
  /// stores, the two frames of a sample added in ascending f whatever chunk_frames is (0: the plan chooses;
  /// imdct_chunk_frames tells what); the buffers must not overlap.
  void set_imdct_window(const scalar_type* window) {
    real_plan_only("set_imdct_window");
    detail::check(pfft_plan_set_imdct_window(plan_.get(), window));
  }
  std::size_t imdct_chunk_frames(std::size_t n_signals, std::size_t n_frames) const {
    real_plan_only("imdct_chunk_frames");
    uint64_t chunk = 0;
    detail::check(pfft_plan_imdct_chunk_frames(plan_.get(), n_signals, n_frames, &chunk));
    return static_cast<std::size_t>(chunk);
  }
  event imdct(const scalar_type* in, scalar_type* out, std::size_t n_signals, std::size_t n_frames, std::size_t frame_pitch,
              std::size_t in_pitch, std::size_t lead, std::size_t out_length, std::size_t out_pitch,
              std::size_t chunk_frames = 0, const std::vector<event>& dependencies = {}) {
    real_plan_only("imdct");
    const std::vector<void*> deps = natives(dependencies);
    void* ev = nullptr;
    detail::check(pfft_execute_imdct_ex(plan_.get(), in, out, n_signals, n_frames, frame_pitch, in_pitch, lead, out_length,
                                        out_pitch, chunk_frames, static_cast<int32_t>(deps.size()), deps.data(), &ev));
    return event(ev);
  }

  /// Power spectrogram / Welch periodogram on the same descriptors.  set_periodogram_window: N real scalars in device
  /// memory, nullptr = all ones, independent of set_window; the first call resolves the kernel.  periodogram: with X_i[f][k]
  /// what stft computes, P_i[c][k] = sum over the frames f = c * avg_frames ... min((c + 1) * avg_frames, n_frames) - 1 of
  /// |X_i[f][k]|^2 -- a sum, not a mean, no one-sided doubling -- goes to out + i * out_pitch + c * row_pitch + k (scalars),
  /// for c < ceil(n_frames / avg_frames), k <= N / 2; one kernel launch, frames added in ascending f, the buffers must not
  /// overlap.
  void set_periodogram_window(const scalar_type* window) {
    real_plan_only("set_periodogram_window");
    detail::check(pfft_plan_set_periodogram_window(plan_.get(), window));
  }
  event periodogram(const scalar_type* in, scalar_type* out, std::size_t n_signals, std::size_t in_length,
                    std::size_t in_pitch, std::size_t hop, std::size_t lead, int32_t pad_mode, std::size_t n_frames,
                    std::size_t avg_frames, std::size_t row_pitch, std::size_t out_pitch,
                    const std::vector<event>& dependencies = {}) {
    real_plan_only("periodogram");
    const std::vector<void*> deps = natives(dependencies);
    void* ev = nullptr;
    detail::check(pfft_execute_periodogram_ex(plan_.get(), in, out, n_signals, in_length, in_pitch, hop, lead, pad_mode,
                                              n_frames, avg_frames, row_pitch, out_pitch, static_cast<int32_t>(deps.size()),
                                              deps.data(), &ev));
    return event(ev);
  }

  /// Convolution / correlation of pairs of real rows on the same descriptors: both operands are data of the call.
  /// prepare_pairs: resolves the kernels, once; takes no data and uploads nothing.  Row t of x (x_length <= N scalars at x
  /// + t * x_pitch) and row t of y are extended with zeros to N; with X, Y their unscaled half spectra and c =
  /// forward_scale^2 * backward_scale, convolve_pairs stores c * N * irfft(X * Y) and correlate_pairs c * N * irfft(X *
  /// conj(Y)) -- r[l] = c * N * sum_n xe[(n + l) mod N] * ye[n], irfft being NumPy's -- as the first out_length <= N scalars at out + t * out_pitch;
  /// with phat_floor f > 0 (GCC-PHAT) every bin of X * conj(Y) is divided by max(|bin|, f) first, and the scale is
  /// backward_scale.  With x_length + y_length - 1 <= N nothing aliases: the lags 0 ... x_length - 1 are at r[0 ...], the
  /// lags -1 ... -(y_length - 1) at r[N - 1] downwards.  One kernel launch; x == y is autocorrelation; out must overlap
  /// neither.
  void prepare_pairs() {
    real_plan_only("prepare_pairs");
    detail::check(pfft_plan_prepare_pairs(plan_.get()));
  }
  event convolve_pairs(const scalar_type* x, const scalar_type* y, scalar_type* out, std::size_t n_rows,
                       std::size_t x_length, std::size_t x_pitch, std::size_t y_length, std::size_t y_pitch,
                       std::size_t out_length, std::size_t out_pitch, const std::vector<event>& dependencies = {}) {
    real_plan_only("convolve_pairs");
    return pairs(PFFT_CONVOLVE, x, y, out, n_rows, x_length, x_pitch, y_length, y_pitch, out_length, out_pitch, 0.0,
                 dependencies);
  }
  event correlate_pairs(const scalar_type* x, const scalar_type* y, scalar_type* out, std::size_t n_rows,
                        std::size_t x_length, std::size_t x_pitch, std::size_t y_length, std::size_t y_pitch,
                        std::size_t out_length, std::size_t out_pitch, const std::vector<event>& dependencies = {},
                        double phat_floor = 0) {
    real_plan_only("correlate_pairs");
    return pairs(PFFT_CORRELATE, x, y, out, n_rows, x_length, x_pitch, y_length, y_pitch, out_length, out_pitch,
                 phat_floor, dependencies);
  }

  /// queue.wait() of the reference's callers: everything submitted on the plan's stream has finished
  void wait() const { detail::check(pfft_plan_wait(plan_.get())); }


  pfft_plan_info_t info() const {
    pfft_plan_info_t i{};
    detail::check(pfft_plan_get_info(plan_.get(), &i));
    return i;
  }
};

template <typename DescScalar, domain DescDomain>
struct descriptor {
  using Scalar = DescScalar;
  static_assert(detail::is_scalar_v<Scalar>, "Scalar must be float, double or _Float16");
  using scale_type = detail::scale_type_t<Scalar>;
  static constexpr domain Domain = DescDomain;

  std::vector<std::size_t> lengths;
  scale_type forward_scale = 1;
  scale_type backward_scale = 1;
  std::size_t number_of_transforms = 1;
  portfft::complex_storage complex_storage = portfft::complex_storage::INTERLEAVED_COMPLEX;
  portfft::placement placement = portfft::placement::OUT_OF_PLACE;
  std::vector<std::size_t> forward_strides;
  std::vector<std::size_t> backward_strides;
  std::size_t forward_distance = 1;
  std::size_t backward_distance = 1;
  std::size_t forward_offset = 0;
  std::size_t backward_offset = 0;

  explicit descriptor(const std::vector<std::size_t>& lengths)
      : lengths(lengths), forward_strides(detail::get_default_strides(lengths)), backward_strides(forward_strides) {
    const std::size_t total = get_flattened_length();
    forward_distance = total;
    backward_distance = total;
  }

  /// validate, then plan (descriptor.hpp:152-156)
  committed_descriptor<Scalar, Domain> commit(queue& q) {
    const pfft_desc_t d = to_c();
    detail::check(pfft_desc_validate(&d));
    return committed_descriptor<Scalar, Domain>(d, q);
  }

  std::size_t get_flattened_length() const noexcept {
    return std::accumulate(lengths.begin(), lengths.end(), std::size_t{1}, std::multiplies<std::size_t>());
  }
  std::size_t get_input_count(direction dir) const {
    const pfft_desc_t d = to_c();
    return static_cast<std::size_t>(pfft_desc_input_count(&d, static_cast<int32_t>(dir)));
  }
  std::size_t get_output_count(direction dir) const { return get_input_count(inv(dir)); }

  const std::vector<std::size_t>& get_strides(direction dir) const noexcept {
    return dir == direction::FORWARD ? forward_strides : backward_strides;
  }
  std::vector<std::size_t>& get_strides(direction dir) noexcept {
    return dir == direction::FORWARD ? forward_strides : backward_strides;
  }
  std::size_t get_distance(direction dir) const noexcept {
    return dir == direction::FORWARD ? forward_distance : backward_distance;
  }
  std::size_t& get_distance(direction dir) noexcept {
    return dir == direction::FORWARD ? forward_distance : backward_distance;
  }
  std::size_t get_offset(direction dir) const noexcept {
    return dir == direction::FORWARD ? forward_offset : backward_offset;
  }
  std::size_t& get_offset(direction dir) noexcept {
    return dir == direction::FORWARD ? forward_offset : backward_offset;
  }
  scale_type get_scale(direction dir) const noexcept { return dir == direction::FORWARD ? forward_scale : backward_scale; }
  scale_type& get_scale(direction dir) noexcept { return dir == direction::FORWARD ? forward_scale : backward_scale; }

 protected:
  pfft_desc_t to_c() const {
    if (lengths.size() > PFFT_MAX_RANK) {
      throw unsupported_configuration("At most " + std::to_string(PFFT_MAX_RANK) + " dimensions are supported");
    }
    pfft_desc_t d{};
    d.precision = detail::precision_v<Scalar>;
    d.domain = static_cast<int32_t>(Domain);
    d.rank = static_cast<int32_t>(lengths.size());
    d.complex_storage = static_cast<int32_t>(complex_storage);
    d.placement = static_cast<int32_t>(placement);
    d.n_forward_strides = static_cast<int32_t>(forward_strides.size());
    d.n_backward_strides = static_cast<int32_t>(backward_strides.size());
    for (std::size_t i = 0; i < lengths.size(); ++i) d.lengths[i] = lengths[i];
    for (std::size_t i = 0; i < forward_strides.size() && i < PFFT_MAX_RANK; ++i) d.forward_strides[i] = forward_strides[i];
    for (std::size_t i = 0; i < backward_strides.size() && i < PFFT_MAX_RANK; ++i) d.backward_strides[i] = backward_strides[i];
    d.forward_distance = forward_distance;
    d.backward_distance = backward_distance;
    d.forward_offset = forward_offset;
    d.backward_offset = backward_offset;
    d.number_of_transforms = number_of_transforms;
    d.forward_scale = static_cast<double>(forward_scale);
    d.backward_scale = static_cast<double>(backward_scale);
    return d;
  }
};

/// Extensions of this library: what the reference does not offer is asked for by name.
namespace amd {

/// Real-to-complex / complex-to-real 1-D transforms of even length (PFFT_EXT_REAL_TRANSFORMS).  A
/// descriptor<Scalar, domain::REAL> with the extension bit and the real defaults: forward_distance = length scalars,
/// backward_distance = length / 2 + 1 complex elements.  commit() returns a committed_descriptor<Scalar, domain::REAL>
/// whose compute_forward(const Scalar*, std::complex<Scalar>*) / compute_backward(const std::complex<Scalar>*, Scalar*)
/// run the transform.  A plain descriptor<Scalar, domain::REAL> keeps the reference's refusal.
template <typename Scalar>
struct real_descriptor : descriptor<Scalar, domain::REAL> {
  using base = descriptor<Scalar, domain::REAL>;
  explicit real_descriptor(std::size_t length) : base({length}) { this->backward_distance = length / 2 + 1; }

  committed_descriptor<Scalar, domain::REAL> commit(queue& q) {
    const pfft_desc_t d = to_c();
    detail::check(pfft_desc_validate(&d));
    return committed_descriptor<Scalar, domain::REAL>(d, q);
  }
  std::size_t get_input_count(direction dir) const {
    const pfft_desc_t d = to_c();
    return static_cast<std::size_t>(pfft_desc_input_count(&d, static_cast<int32_t>(dir)));
  }
  std::size_t get_output_count(direction dir) const { return get_input_count(inv(dir)); }

 private:
  pfft_desc_t to_c() const {
    pfft_desc_t d = base::to_c();
    d.extensions = PFFT_EXT_REAL_TRANSFORMS;
    return d;
  }
};

/// Real 1-D transforms whose committed descriptor also convolves and filters real data (PFFT_EXT_REAL_CONVOLUTION: the
/// R2C half, the product with a filter's half spectrum and the C2R half in one kernel of length / 2-point passes; float
/// / double, even length >= 4, unit strides).  A real_descriptor in every other respect: the same members, defaults,
/// rules and counts, and compute_forward / compute_backward are the real_descriptor's plan, bit for bit.  The committed
/// descriptor's set_filter (bins) and convolve / correlate / set_filter_taps / filter on Scalar* work.
template <typename Scalar>
struct real_convolution_descriptor : descriptor<Scalar, domain::REAL> {
  using base = descriptor<Scalar, domain::REAL>;
  explicit real_convolution_descriptor(std::size_t length) : base({length}) { this->backward_distance = length / 2 + 1; }

  committed_descriptor<Scalar, domain::REAL> commit(queue& q) {
    const pfft_desc_t d = to_c();
    detail::check(pfft_desc_validate(&d));
    return committed_descriptor<Scalar, domain::REAL>(d, q);
  }
  std::size_t get_input_count(direction dir) const {
    const pfft_desc_t d = to_c();
    return static_cast<std::size_t>(pfft_desc_input_count(&d, static_cast<int32_t>(dir)));
  }
  std::size_t get_output_count(direction dir) const { return get_input_count(inv(dir)); }
  /// the C descriptor that commit() hands to the library (extensions == PFFT_EXT_REAL_CONVOLUTION)
  pfft_desc_t c_descriptor() const { return to_c(); }

 private:
  pfft_desc_t to_c() const {
    pfft_desc_t d = base::to_c();
    d.extensions = PFFT_EXT_REAL_CONVOLUTION;
    return d;
  }
};

/// Complex transforms that may have a 1-D length with a prime factor above 61 (PFFT_EXT_ANY_LENGTH: Bluestein's
/// algorithm in one kernel; fp32 lengths up to 4096, fp64 up to 2048).  A descriptor<Scalar, domain::COMPLEX> with the
/// extension bit: every member and default is the base's, and a length the base can commit gets the same plan.  A plain
/// descriptor keeps the reference's refusal of such lengths.
template <typename Scalar>
struct any_length_descriptor : descriptor<Scalar, domain::COMPLEX> {
  using base = descriptor<Scalar, domain::COMPLEX>;
  explicit any_length_descriptor(const std::vector<std::size_t>& lengths) : base(lengths) {}

  committed_descriptor<Scalar, domain::COMPLEX> commit(queue& q) {
    const pfft_desc_t d = to_c();
    detail::check(pfft_desc_validate(&d));
    return committed_descriptor<Scalar, domain::COMPLEX>(d, q);
  }
  /// the C descriptor that commit() hands to the library (extensions == PFFT_EXT_ANY_LENGTH)
  pfft_desc_t c_descriptor() const { return to_c(); }

 private:
  pfft_desc_t to_c() const {
    pfft_desc_t d = base::to_c();
    d.extensions = PFFT_EXT_ANY_LENGTH;
    return d;
  }
};

/// Complex 1-D transforms whose committed descriptor also convolves (PFFT_EXT_CONVOLUTION: forward transform, product
/// with a filter spectrum and backward transform in one kernel; float / double, interleaved storage, unit strides,
/// lengths with a one-kernel LDS-resident plan).  A descriptor<Scalar, domain::COMPLEX> with the extension bit: every
/// member and default is the base's, compute_forward / compute_backward are the base's plan, bit for bit, and the
/// committed descriptor's set_filter / convolve / correlate work.
template <typename Scalar>
struct convolution_descriptor : descriptor<Scalar, domain::COMPLEX> {
  using base = descriptor<Scalar, domain::COMPLEX>;
  explicit convolution_descriptor(const std::vector<std::size_t>& lengths) : base(lengths) {}

  committed_descriptor<Scalar, domain::COMPLEX> commit(queue& q) {
    const pfft_desc_t d = to_c();
    detail::check(pfft_desc_validate(&d));
    return committed_descriptor<Scalar, domain::COMPLEX>(d, q);
  }
  /// the C descriptor that commit() hands to the library (extensions == PFFT_EXT_CONVOLUTION)
  pfft_desc_t c_descriptor() const { return to_c(); }

 private:
  pfft_desc_t to_c() const {
    pfft_desc_t d = base::to_c();
    d.extensions = PFFT_EXT_CONVOLUTION;
    return d;
  }
};

}  // namespace amd
}  // namespace portfft

#endif  // PORTFFT_PORTFFT_HPP
