/*
 * portfft_amd.h -- C ABI of the MI355X-native batched FFT engine.
 *
 * This is the drop-in boundary for the 1-D / N-D complex-to-complex execute path of portFFT.  Every entry point
 * names the reference interface it replaces (paths relative to /root/reference).  The C++ facade
 * include/portfft/portfft.hpp (namespace portfft: descriptor, committed_descriptor, exceptions) and the Python
 * mirror portfft_amd/ are thin wrappers over exactly these symbols.
 *
 * Conventions
 *   - plain C types only: pointers, sizes, enums as int32_t; no HIP or torch types in signatures
 *     (a HIP stream is passed as void*; NULL = the default stream).
 *   - every function returns a pfft_status; the message of the last failure on the calling thread is
 *     available from pfft_last_error().  No C++ exception crosses this boundary.
 *   - `in`/`out` are device-accessible pointers (hipMalloc / hipMallocManaged), i.e. the USM pointers of the
 *     reference's compute_forward/compute_backward overloads.
 *   - execution is asynchronous and ordered on the plan's stream, like the reference's sycl::event-returning
 *     overloads (src/portfft/committed_descriptor.hpp:171-310).
 */
#ifndef PORTFFT_AMD_H
#define PORTFFT_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PFFT_MAX_RANK 8

/* Error taxonomy: mirrors src/portfft/common/exceptions.hpp:32-77. */
typedef enum pfft_status {
  PFFT_OK = 0,
  PFFT_INVALID_CONFIGURATION = 1,     /* portfft::invalid_configuration      */
  PFFT_UNSUPPORTED_CONFIGURATION = 2, /* portfft::unsupported_configuration  */
  PFFT_OUT_OF_LOCAL_MEMORY = 3,       /* portfft::out_of_local_memory_error  */
  PFFT_INTERNAL_ERROR = 4,            /* portfft::internal_error             */
  PFFT_HIP_ERROR = 5                  /* a HIP runtime call failed (reference: sycl::exception) */
} pfft_status;

/* src/portfft/enums.hpp:25-31 */
enum { PFFT_DOMAIN_REAL = 0, PFFT_DOMAIN_COMPLEX = 1 };
enum { PFFT_INTERLEAVED_COMPLEX = 0, PFFT_SPLIT_COMPLEX = 1 };
enum { PFFT_IN_PLACE = 0, PFFT_OUT_OF_PLACE = 1 };
enum { PFFT_FORWARD = 0, PFFT_BACKWARD = 1 };
/* src/portfft/enums.hpp:44-56 (detail::layout) */
enum { PFFT_LAYOUT_PACKED = 0, PFFT_LAYOUT_UNPACKED = 1, PFFT_LAYOUT_BATCH_INTERLEAVED = 2 };
/* PFFT_PRECISION_F16: IEEE binary16 storage (complex elements of two halves, 4 bytes; split planes of 2-byte values),
 * computed in fp32.  1-D PACKED COMPLEX descriptors whose length has a one-kernel plan; scales stay double. */
enum { PFFT_PRECISION_F32 = 0, PFFT_PRECISION_F64 = 1, PFFT_PRECISION_F16 = 2 };

/*
 * POD mirror of portfft::descriptor<Scalar, Domain> (src/portfft/descriptor.hpp:43-129): same fields, same
 * meaning, same defaults (set by pfft_desc_init).  `n_forward_strides`/`n_backward_strides` carry the vector
 * sizes so that the "mismatching strides length" check of descriptor_validation.hpp:92-99 can be reproduced.
 */
typedef struct pfft_desc_t {
  int32_t precision;       /* PFFT_PRECISION_*: the Scalar template argument */
  int32_t domain;          /* PFFT_DOMAIN_*: the Domain template argument */
  int32_t rank;            /* lengths.size() */
  int32_t complex_storage; /* PFFT_INTERLEAVED_COMPLEX (default) | PFFT_SPLIT_COMPLEX */
  int32_t placement;       /* PFFT_OUT_OF_PLACE (default) | PFFT_IN_PLACE */
  int32_t n_forward_strides;
  int32_t n_backward_strides;
  union {
    int32_t extensions; /* PFFT_EXT_* bits; 0 (pfft_desc_init): the reference's behaviour, nothing else */
    int32_t reserved_;  /* the word's former name (same offset and size), kept for code that mirrors it */
  };
  uint64_t lengths[PFFT_MAX_RANK];
  uint64_t forward_strides[PFFT_MAX_RANK];
  uint64_t backward_strides[PFFT_MAX_RANK];
  uint64_t forward_distance;
  uint64_t backward_distance;
  uint64_t forward_offset;
  uint64_t backward_offset;
  uint64_t number_of_transforms;
  double forward_scale;
  double backward_scale;
} pfft_desc_t;

/* Extensions: what the reference does not offer is asked for by name, one bit of pfft_desc_t::extensions each.  A
 * descriptor without bits behaves like the reference's (a REAL descriptor is refused); unknown bits are invalid.
 * PFFT_EXT_REAL_TRANSFORMS: real-to-complex / complex-to-real 1-D transforms of even length N >= 4 (domain REAL, fp32 /
 * fp64, unit strides).  Forward domain: N real scalars per transform; backward domain: N/2 + 1 complex elements (bins
 * 0 ... N/2).  forward_distance / forward_offset count scalars, backward_distance / backward_offset complex elements;
 * in place needs forward_distance == 2 * backward_distance and forward_offset == 2 * backward_offset (padded rows).
 * Forward is numpy's rfft, backward N * irfft (unnormalised; the imaginary parts of bins 0 and N/2 are ignored).
 * PFFT_EXT_ANY_LENGTH: complex 1-D transforms of lengths with a prime factor above 61, which are otherwise refused
 * (Bluestein's algorithm in one kernel; domain COMPLEX, fp32 N <= 4096 / fp64 N <= 2048, INTERLEAVED_COMPLEX, unit
 * strides, any distances >= N, offsets, scales and batch, in place and out of place).  The bit is a permission: a length
 * that has an ordinary plan keeps it, bit for bit.  It cannot be combined with PFFT_EXT_REAL_TRANSFORMS.
 * PFFT_EXT_CONVOLUTION: circular convolution of every row with a filter given in the frequency domain -- forward
 * transform, pointwise product and backward transform in one kernel (pfft_plan_set_filter, pfft_execute_convolve; domain
 * COMPLEX, fp32 / fp64, rank 1, INTERLEAVED_COMPLEX, unit strides, any distances >= N, offsets, scales and batch, in place
 * and out of place; lengths whose plan is one LDS-resident work-group kernel: the powers of two up to fp32 N = 8192 /
 * fp64 N = 4096 pre-compiled, other lengths with prime factors up to 61 compiled at commit, e.g. fp32 N = 10000).  The
 * bit is a permission plus the new verb:
 * pfft_execute of such a plan is the ordinary transform, same plan and same bits, so the filter spectrum can be made with
 * it.  It cannot be combined with the other two bits; bit value 4 is not assigned and stays invalid.
 * PFFT_EXT_REAL_CONVOLUTION: the same verbs on REAL data -- real rows or signals in, real rows or signals out, in one
 * kernel that runs N / 2-point passes and reads and writes every sample as one scalar.  Valid only alone and only on the
 * REAL domain.  Such a descriptor is a real descriptor in every other respect: the rules of PFFT_EXT_REAL_TRANSFORMS
 * (fp32 / fp64, rank 1, even N >= 4, unit strides, the same counts, distances, offsets and padded in-place pair), and
 * pfft_execute of its plan is the plain R2C / C2R of PFFT_EXT_REAL_TRANSFORMS, same kernels and same bits, so the
 * filter spectrum can be made with it.  Lengths: N / 2 with a one-kernel LDS-resident plan (powers of two up to fp32
 * N = 16384 / fp64 N = 8192 pre-compiled, others with prime factors up to 61 compiled at commit, e.g. fp32 N = 12000). */
enum {
  PFFT_EXT_REAL_TRANSFORMS = 1,
  PFFT_EXT_ANY_LENGTH = 2,
  PFFT_EXT_CONVOLUTION = 8,
  PFFT_EXT_REAL_CONVOLUTION = 16
};
/* mode of pfft_execute_convolve: the filter spectrum H as given, or its conjugate (correlation: the adjoint) */
enum { PFFT_CONVOLVE = 0, PFFT_CORRELATE = 1 };

/* Tier a dimension was planned on; the analogue of detail::level (src/portfft/enums.hpp:42). */
enum {
  PFFT_TIER_REGISTER = 0,  /* one register pass per FFT (reference: WORKITEM) */
  PFFT_TIER_WORKGROUP = 1, /* Stockham passes through LDS, specialised kernel (reference: SUBGROUP + WORKGROUP) */
  PFFT_TIER_GENERIC = 2,   /* runtime-radix LDS kernel, any stride / storage */
  PFFT_TIER_GLOBAL = 3     /* multi-kernel decomposition through HBM scratch (reference: GLOBAL) */
};

#define PFFT_MAX_FACTORS 16
typedef struct pfft_dim_info_t {
  uint64_t length;
  int32_t tier;
  int32_t n_factors;
  int32_t factors[PFFT_MAX_FACTORS]; /* radices of the passes (WORKGROUP/GENERIC) or sub-lengths (GLOBAL) */
  int32_t workgroup_size;
  int32_t ffts_per_workgroup;
  uint64_t lds_bytes;
} pfft_dim_info_t;

typedef struct pfft_plan_info_t {
  int32_t rank;
  int32_t n_compute_units;
  uint64_t twiddle_bytes; /* HBM held by the plan for twiddles */
  uint64_t scratch_bytes; /* HBM held by the plan for intermediate data */
  pfft_dim_info_t dims[PFFT_MAX_RANK];
  int32_t launches[2]; /* kernel launches of one execute [forward, backward]; plans that run chunk by chunk
                          (intermediate sized to the Infinity Cache) count every chunk's launches */
  int32_t xcd_local[2]; /* 1: that direction runs the GLOBAL tier as ONE persistent launch (per-XCD task queues) followed
                           by its recovery launch, which does nothing unless a hand-off wait of the former gave up */
  uint64_t xcd_recoveries; /* executes of this plan (copy) whose persistent launch gave up and were recomputed, in stream
                              order, by the recovery launch: the result was valid whenever the execute's event completed */
  uint64_t knob_mask; /* which PFFT_* environment knobs differed from their defaults when the plan was committed (bit order:
                         plan_knobs::from_env, portfft_amd/csrc/plan_core.cpp); 0 = the product's defaults.  The environment
                         is read at commit only, never at execute */
} pfft_plan_info_t;

typedef struct pfft_plan_t pfft_plan_t; /* opaque: portfft::committed_descriptor */

/* ---- descriptor (host only, no device needed) ------------------------------------------------------------ */

/* descriptor::descriptor(lengths): default strides / distances / scales (src/portfft/descriptor.hpp:131-144). */
pfft_status pfft_desc_init(pfft_desc_t* desc, int32_t precision, int32_t domain, int32_t rank,
                           const uint64_t* lengths);
/* No reference equivalent: a REAL descriptor of `length` scalars with PFFT_EXT_REAL_TRANSFORMS set and the real
 * defaults (out of place, forward_distance = length, backward_distance = length / 2 + 1). */
pfft_status pfft_desc_init_real(pfft_desc_t* desc, int32_t precision, uint64_t length);
/* No reference equivalent: the defaults of pfft_desc_init_real with PFFT_EXT_REAL_CONVOLUTION as the only extension. */
pfft_status pfft_desc_init_real_convolution(pfft_desc_t* desc, int32_t precision, uint64_t length);
/* detail::validate::validate_descriptor (src/portfft/descriptor_validation.hpp:264-281). */
pfft_status pfft_desc_validate(const pfft_desc_t* desc);
/* descriptor::get_flattened_length (src/portfft/descriptor.hpp:161-163). */
uint64_t pfft_desc_flattened_length(const pfft_desc_t* desc);
/* descriptor::get_input_count / get_output_count (src/portfft/descriptor.hpp:172-183). */
uint64_t pfft_desc_input_count(const pfft_desc_t* desc, int32_t direction);
uint64_t pfft_desc_output_count(const pfft_desc_t* desc, int32_t direction);
/* detail::get_layout (src/portfft/utils.hpp:238-246). */
int32_t pfft_desc_layout(const pfft_desc_t* desc, int32_t direction);

/* ---- plan (needs a HIP device) ----------------------------------------------------------------------------- */

/* descriptor::commit(queue) (src/portfft/descriptor.hpp:152-156): validate, plan every dimension, upload
 * twiddles, allocate scratch.  `hip_stream` is a hipStream_t (NULL = default stream) on the current device.
 * Configurations without a pre-compiled kernel are specialised here by hiprtc (0.2-2 s the first time, then cached
 * in the process and on disk; the reference builds its kernels at commit too: committed_descriptor_impl.hpp:448-573);
 * nothing is compiled or allocated at execute.  Thread-safe; the plan itself is not (one plan per host thread). */
pfft_status pfft_plan_create(const pfft_desc_t* desc, void* hip_stream, pfft_plan_t** plan);
/* committed_descriptor_impl::~committed_descriptor_impl (committed_descriptor_impl.hpp:825-828): waits for the
 * stream, frees twiddles and scratch. */
pfft_status pfft_plan_destroy(pfft_plan_t* plan);
/* Planner output for tests / logging (no reference equivalent beyond PORTFFT_LOG_TRACE). */
pfft_status pfft_plan_get_info(const pfft_plan_t* plan, pfft_plan_info_t* info);

/* committed_descriptor::compute_forward / compute_backward, interleaved USM overloads
 * (src/portfft/committed_descriptor.hpp:171-176, 215-218, 242-246, 288-293).  in == out selects the in-place
 * overload.  `direction` is PFFT_FORWARD or PFFT_BACKWARD.  Storage mismatch -> PFFT_INVALID_CONFIGURATION like
 * dispatch_direction (committed_descriptor_impl.hpp:862-871). */
pfft_status pfft_execute(pfft_plan_t* plan, int32_t direction, const void* in, void* out);
/* Split-complex USM overloads (src/portfft/committed_descriptor.hpp:186-192, 228-232, 258-263, 305-310). */
pfft_status pfft_execute_split(pfft_plan_t* plan, int32_t direction, const void* in_real, const void* in_imag,
                               void* out_real, void* out_imag);
/* The same overloads with the reference's `const std::vector<sycl::event>& dependencies` argument and its returned
 * sycl::event (src/portfft/committed_descriptor.hpp:171, 215, 242-246, 288-293; split twins 186-192, 228-232,
 * 258-263, 305-310).  `deps` is an array of `n_deps` hipEvent_t handles (as void*; NULL entries are skipped): the
 * plan's stream waits for each of them (hipStreamWaitEvent) before the first kernel.  When `event_out` is not NULL
 * it receives a fresh hipEvent_t recorded behind the last kernel of THIS submission; the caller owns it
 * (pfft_event_wait / pfft_event_query / pfft_event_destroy, or any HIP call that takes a hipEvent_t). */
pfft_status pfft_execute_ex(pfft_plan_t* plan, int32_t direction, const void* in, void* out, int32_t n_deps,
                            void* const* deps, void** event_out);
pfft_status pfft_execute_split_ex(pfft_plan_t* plan, int32_t direction, const void* in_real, const void* in_imag,
                                  void* out_real, void* out_imag, int32_t n_deps, void* const* deps,
                                  void** event_out);
/* No reference equivalent (plans committed with PFFT_EXT_CONVOLUTION; PFFT_INVALID_CONFIGURATION on any other plan).
 * pfft_plan_set_filter: `spectra` is a device pointer to n_filters * N interleaved complex elements of the descriptor's
 * precision, packed, in the frequency domain (what pfft_execute(PFFT_FORWARD) of this plan makes of a filter).  They
 * are copied on the plan's stream into memory the plan owns: the caller's buffer may be rewritten or freed once the
 * stream has passed the copy, and executes submitted later see the new filter.  Executes already submitted keep the
 * filter they were submitted with (replacing a filter nothing else holds waits for them on the host).  Row t of an
 * execute uses filter t mod n_filters: 1 = one shared filter, number_of_transforms = one per row, a channel count =
 * depthwise.  pfft_plan_clone shares the filter; pfft_plan_set_filter on either copy then detaches that copy.
 * pfft_execute_convolve: out[t] = forward_scale * backward_scale * N * IDFT_N(DFT_N(in[t]) . H[t mod n_filters]), with
 * conj(H) for PFFT_CORRELATE -- what pfft_execute(PFFT_FORWARD), a multiply and pfft_execute(PFFT_BACKWARD) produce.
 * `in` is laid out as the forward domain (forward_distance / forward_offset), `out` as the backward domain; in == out
 * selects in place.  Before the first pfft_plan_set_filter: PFFT_INVALID_CONFIGURATION.  The _ex form takes
 * dependencies and returns an event like pfft_execute_ex. */
pfft_status pfft_plan_set_filter(pfft_plan_t* plan, const void* spectra, uint64_t n_filters);
pfft_status pfft_execute_convolve(pfft_plan_t* plan, int32_t mode, const void* in, void* out);
pfft_status pfft_execute_convolve_ex(pfft_plan_t* plan, int32_t mode, const void* in, void* out, int32_t n_deps,
                                     void* const* deps, void** event_out);
/* Overlap-save FIR filtering of long signals on the same plans (PFFT_EXT_CONVOLUTION; no reference equivalent): linear
 * convolution or correlation with time-domain taps, in one kernel launch that reads every signal N / (N - K + 1) times
 * and writes the result once -- no gather of overlapping segments, no copy of the valid samples.  N = lengths[0].
 * pfft_plan_set_filter_taps: `taps` is a device pointer to n_filters * n_taps packed interleaved complex elements of the
 * plan's precision, 1 <= n_taps <= N.  The plan zero-pads each filter to N and transforms it on the device, on its
 * stream, unscaled: the spectra are what pfft_execute(PFFT_FORWARD) with scale 1 makes of the padded taps.  They become
 * the plan's filter exactly as with pfft_plan_set_filter (ownership, clones, replacement, refused inside a stream
 * capture), so pfft_execute_convolve on them is the circular convolution with the zero-padded taps; the plan also
 * remembers n_taps, which pfft_execute_filter needs (after a plain pfft_plan_set_filter it is refused).
 * pfft_execute_filter: with c = forward_scale * backward_scale * N (the factor of pfft_execute_convolve), h_i the taps of
 * filter i mod n_filters, K = n_taps and x_i zero outside [0, in_length):
 *   PFFT_CONVOLVE   y_i[n] = c * sum_{k<K} h_i[k] * x_i[n - k],        n in [0, out_length), out_length <= in_length + K - 1
 *   PFFT_CORRELATE  y_i[n] = c * sum_{k<K} conj(h_i[k]) * x_i[n + k],  n in [0, out_length), out_length <= in_length
 * `in` and `out` point at sample 0 of signal 0; signal i starts i * in_pitch (i * out_pitch) complex elements on, pitches
 * at least the lengths.  Only the out_length elements of every output signal are written.  The descriptor's
 * number_of_transforms, distances and offsets do not apply; the precision, N and the two scales do.  The byte ranges of
 * input and output must not overlap (in == out included: a segment reads samples its predecessor's outputs would
 * overwrite) -- PFFT_INVALID_CONFIGURATION, like null pointers, zero counts, a bad mode, out_length beyond its bound and
 * pitches below the lengths.  PFFT_UNSUPPORTED_CONFIGURATION: what exceeds the kernel's 32-bit byte offsets -- the
 * signals a work-group's rows touch (at most min(rows per work-group, n_signals) consecutive ones) must span less than
 * 4 GiB, so a single signal of 4 GiB or more is refused -- and 2^31 or more (signal, segment) pairs.  Nothing is compiled
 * or allocated at execute.  With real taps the real and the imaginary part of a signal are filtered independently: two
 * real channels ride in one complex signal.  N >= 4 K keeps the re-read of the input below 1.34 x. */
pfft_status pfft_plan_set_filter_taps(pfft_plan_t* plan, const void* taps, uint64_t n_taps, uint64_t n_filters);
pfft_status pfft_execute_filter(pfft_plan_t* plan, int32_t mode, const void* in, void* out, uint64_t n_signals,
                                uint64_t in_length, uint64_t in_pitch, uint64_t out_length, uint64_t out_pitch);
pfft_status pfft_execute_filter_ex(pfft_plan_t* plan, int32_t mode, const void* in, void* out, uint64_t n_signals,
                                   uint64_t in_length, uint64_t in_pitch, uint64_t out_length, uint64_t out_pitch,
                                   int32_t n_deps, void* const* deps, void** event_out);
/* The same six entry points on a plan committed with PFFT_EXT_REAL_CONVOLUTION (REAL domain, N = lengths[0], M = N / 2):
 * everything that is a complex element above is a real scalar here, except the spectra.
 * pfft_plan_set_filter: n_filters * (M + 1) interleaved complex bins, packed -- what pfft_execute(PFFT_FORWARD) of this
 * plan with scale 1 makes of a real filter of N scalars.  The imaginary parts of bins 0 and M are ignored, as C2R ignores
 * them.  Ownership, clone sharing, replacement and refusal inside a stream capture are as above.
 * pfft_execute_convolve: out[t] = c * N-point circular convolution of in[t] with filter t mod n_filters, c =
 * forward_scale * backward_scale * N, i.e. c * irfft(rfft(in[t]) . H) in NumPy's terms (conj(H) for PFFT_CORRELATE).
 * Input AND output are rows of N real scalars laid out as the forward domain (forward_distance / forward_offset, in
 * scalars); in == out is allowed.
 * pfft_plan_set_filter_taps: n_filters * n_taps real scalars, packed; zero-padded to N and transformed on the device by a
 * short-lived real plan (R2C, scale 1) into M + 1 bins each.  The plan remembers n_taps.
 * pfft_execute_filter: the two definitions above with real x, h, y (no conjugate); lengths and pitches count scalars.
 * The kernel works on scalar pairs, so its geometry is even: lead = K - 1 rounded up and hop = N - lead (convolve), hop =
 * N - K + 1 rounded down (correlate) -- at most one sample of hop lost.  n_taps above N - 2 leaves no hop of a pair and is
 * PFFT_INVALID_CONFIGURATION.  The same things are refused as above; the 32-bit limits count bytes of scalars: the
 * signals a work-group's rows touch must span less than 4 GiB, and fewer than 2^31 (signal, segment) pairs. */
/* Short-time Fourier transform of long real signals (no reference equivalent; no extension bit): a pair of verbs on
 * every plan of the REAL domain -- PFFT_EXT_REAL_TRANSFORMS or PFFT_EXT_REAL_CONVOLUTION, whose commit is unchanged.  One
 * kernel launch reads overlapping frames straight from the signals, multiplies each by the window on the way in and
 * stores its R2C bins: no frame buffer, every sample read about N / hop times through L2, every bin written once.
 * N = lengths[0], M = N / 2.  For frame f < n_frames and bin k = 0 ... M of signal i:
 *   X_i[f][k] = forward_scale * sum_{n<N} w[n] * xe_i[f * hop - lead + n] * exp(-2 pi i k n / N)
 * i.e. forward_scale * rfft(w * frame) in NumPy's terms, with xe_i = x_i extended outside [0, in_length) by zeros
 * (PFFT_PAD_ZERO) or by reflection without repeating the edge sample, xe[-p] = x[p], xe[L - 1 + p] = x[L - 1 - p]
 * (PFFT_PAD_REFLECT: np.pad(mode="reflect")).  torch.stft(x, N, hop, window=w, center=True) is lead = N / 2, reflect,
 * n_frames = 1 + in_length / hop, transposed.  The imaginary parts of bins 0 and M are stored as exactly 0.
 * pfft_plan_set_window: `window` is a device pointer to N real scalars of the plan's precision; NULL = all ones.  The
 * first call resolves the kernel (pre-compiled for the power-of-two lengths of the real kernels, otherwise compiled here
 * by hiprtc and cached like every other kernel); every call copies the window on the plan's stream into memory the plan
 * owns, with the rules of pfft_plan_set_filter: executes already submitted keep their window, pfft_plan_clone shares it,
 * a later call on either copy detaches that copy, refused inside a stream capture.
 * pfft_execute_stft: `in` points at sample 0 of signal 0, signal i starts i * in_pitch scalars on; bin k of frame f of
 * signal i goes to out + i * out_pitch + f * frame_pitch + k, in complex elements (frame-major); only those (M + 1) *
 * n_frames * n_signals elements are written.  The precision, N and forward_scale of the descriptor apply; its
 * number_of_transforms, distances and offsets do not.  hop, lead and in_length may be odd.
 * PFFT_INVALID_CONFIGURATION: a plan that is not REAL, no window set, null pointers, zero counts, hop == 0, lead >= N, a
 * bad pad_mode, in_pitch < in_length, frame_pitch < M + 1, out_pitch < n_frames * frame_pitch, overlapping byte ranges
 * of input and output; PFFT_PAD_ZERO with (n_frames - 1) * hop >= in_length + lead (a frame without a sample);
 * PFFT_PAD_REFLECT with lead > in_length - 1 or (n_frames - 1) * hop + N > in_length + 2 * lead (every frame must lie
 * inside the signal padded by `lead` on both sides, so that an index is reflected at most once).
 * PFFT_UNSUPPORTED_CONFIGURATION: what exceeds the kernel's 32-bit byte offsets -- the signals, and the output rows, that
 * one work-group's rows touch span 4 GiB or more -- and 2^31 or more (signal, frame) rows.  Nothing is compiled or
 * allocated at execute.  The _ex form takes dependencies and returns an event like pfft_execute_ex. */
enum { PFFT_PAD_ZERO = 0, PFFT_PAD_REFLECT = 1 };
pfft_status pfft_plan_set_window(pfft_plan_t* plan, const void* window);
pfft_status pfft_execute_stft(pfft_plan_t* plan, const void* in, void* out, uint64_t n_signals, uint64_t in_length,
                              uint64_t in_pitch, uint64_t hop, uint64_t lead, int32_t pad_mode, uint64_t n_frames,
                              uint64_t frame_pitch, uint64_t out_pitch);
pfft_status pfft_execute_stft_ex(pfft_plan_t* plan, const void* in, void* out, uint64_t n_signals, uint64_t in_length,
                                 uint64_t in_pitch, uint64_t hop, uint64_t lead, int32_t pad_mode, uint64_t n_frames,
                                 uint64_t frame_pitch, uint64_t out_pitch, int32_t n_deps, void* const* deps,
                                 void** event_out);
/* Inverse short-time Fourier transform (overlap-add synthesis) of real signals (no reference equivalent; no extension
 * bit): the second pair of verbs on every plan of the REAL domain, whose commit is unchanged.  One kernel launch reads
 * the frame-major bins pfft_execute_stft writes, transforms every frame back (C2R), multiplies it by the synthesis
 * window and adds the overlapping frames in LDS: no frame buffer, no atomics, no zeroed output -- every bin is read once
 * per chunk that needs it, every sample written once with a plain store.  N = lengths[0], M = N / 2.  Frame f of signal i
 * is g_i[f] = what pfft_execute(PFFT_BACKWARD) of the plan makes of its M + 1 bins, backward_scale * N * irfft(X_i[f]);
 * the imaginary parts of bins 0 and M are dropped.  For t < out_length, with u = t + lead:
 *   ola_i[t] = sum_f w[u - f * hop] * g_i[f][u - f * hop]      over the frames with 0 <= u - f * hop < N
 *   env[t]   = sum_f w[u - f * hop]^2                           over the same frames
 *   PFFT_ISTFT_PLAIN:      y_i[t] = ola_i[t]
 *   PFFT_ISTFT_NORMALIZE:  y_i[t] = ola_i[t] / env[t] where env[t] > PFFT_ISTFT_ENV_MIN, else exactly 0
 * Both sums run in ascending f, one frame after the other, wherever the work is cut: the result does not depend on
 * chunk_frames or on the launch grid, bit for bit.  torch.istft(Y, N, hop, window=w, center=True, length=L) is
 * backward_scale = 1 / N, lead = N / 2, NORMALIZE, out_length = L, with the bins transposed.  PLAIN is the synthesis
 * operator alone, for callers whose analysis and synthesis windows differ and who normalise themselves.
 * pfft_plan_set_synthesis_window: `window` is a device pointer to N real scalars of the plan's precision; NULL = all
 * ones.  Independent of pfft_plan_set_window (pass the same scalars to both for torch's convention).  The first call
 * resolves the kernel (pre-compiled for the power-of-two lengths of the real kernels, otherwise compiled here by hiprtc
 * and cached like every other kernel); every call copies the window on the plan's stream into memory the plan owns, with
 * the rules of pfft_plan_set_filter: pfft_plan_clone shares it until either side sets another, refused inside a stream
 * capture.
 * pfft_execute_istft: bin k of frame f of signal i is read from in + i * in_pitch + f * frame_pitch + k (complex
 * elements), sample t of signal i goes to out + i * out_pitch + t (scalars); only those out_length * n_signals scalars
 * are written.  The work is cut into chunks of chunk_frames frames per signal, each preceded by a recomputed halo of
 * ceil(N / hop) - 1 frames; 0 lets the plan choose (as large as still fills the device, at least four halos).
 * PFFT_INVALID_CONFIGURATION: a plan that is not REAL, no synthesis window set, null pointers, zero counts, hop == 0,
 * hop > N (gaps no frame covers), lead >= N, a bad mode, frame_pitch < M + 1, in_pitch < n_frames * frame_pitch,
 * out_pitch < out_length, overlapping byte ranges of input and output, out_length > (n_frames - 1) * hop + N - lead (a
 * sample no frame covers), (n_frames - 1) * hop >= out_length + lead (a frame that contributes nothing).
 * PFFT_UNSUPPORTED_CONFIGURATION: 2^31 or more (signal, frame) rows; the bins or the samples one work-group touches span
 * 4 GiB or more; at pfft_plan_set_synthesis_window, an accumulator that does not fit into LDS behind the images.  Nothing
 * is compiled or allocated at execute.  The _ex form takes dependencies and returns an event like pfft_execute_ex.
 * pfft_plan_istft_chunk_frames: the chunk length that chunk_frames = 0 stands for in a call with these counts and this
 * hop (a synthesis window must have been set); with H = ceil(N / hop) - 1 the share of frames transformed twice is about
 * H / chunk_frames. */
enum { PFFT_ISTFT_PLAIN = 0, PFFT_ISTFT_NORMALIZE = 1 };
#define PFFT_ISTFT_ENV_MIN 1e-11 /* the envelope threshold of torch.istft */
pfft_status pfft_plan_set_synthesis_window(pfft_plan_t* plan, const void* window);
pfft_status pfft_plan_istft_chunk_frames(const pfft_plan_t* plan, uint64_t n_signals, uint64_t n_frames, uint64_t hop,
                                         uint64_t* chunk_frames);
pfft_status pfft_execute_istft(pfft_plan_t* plan, const void* in, void* out, uint64_t n_signals, uint64_t n_frames,
                               uint64_t frame_pitch, uint64_t in_pitch, uint64_t hop, uint64_t lead, int32_t mode,
                               uint64_t out_length, uint64_t out_pitch, uint64_t chunk_frames);
pfft_status pfft_execute_istft_ex(pfft_plan_t* plan, const void* in, void* out, uint64_t n_signals, uint64_t n_frames,
                                  uint64_t frame_pitch, uint64_t in_pitch, uint64_t hop, uint64_t lead, int32_t mode,
                                  uint64_t out_length, uint64_t out_pitch, uint64_t chunk_frames, int32_t n_deps,
                                  void* const* deps, void** event_out);
/* Discrete cosine transforms of type 2 and type 3 of packed real rows (no reference equivalent; no extension bit): the
 * third pair of verbs on every plan of the REAL domain, whose commit is unchanged.  One kernel launch per call reads
 * every row once and writes it once: the M-point passes of the real kernels (M = N / 2, N = lengths[0]) between
 * Makhoul's permutation and a quarter-wave twiddle step, all in LDS.  The definitions are scipy.fft.dct(x, type,
 * norm=None) times the plan's scale:
 *   PFFT_DCT_II:   y[k] = forward_scale  * 2 * sum_{n=0}^{N-1} x[n] cos(pi k (2n + 1) / (2N))              k = 0 ... N - 1
 *   PFFT_DCT_III:  y[n] = backward_scale * (x[0] + 2 * sum_{k=1}^{N-1} x[k] cos(pi k (2n + 1) / (2N)))    n = 0 ... N - 1
 * With the default scales of 1, type 3 of type 2 of x is 2 * N * x; backward_scale = 1 / (2N) makes type 3 scipy's idct.
 * Orthonormal scaling (norm="ortho") is not offered.  Lengths: those of the real transforms (even N >= 4).
 * pfft_plan_prepare_dct: takes no data.  The first call resolves the kernels (pre-compiled for the power-of-two lengths
 * of the real kernels, otherwise compiled here by hiprtc and cached like every other kernel) and uploads a table of
 * M + 1 twiddles into memory the plan owns, with the rules of pfft_plan_set_filter: pfft_plan_clone shares both, refused
 * inside a stream capture.  Later calls do nothing.  No other call prepares implicitly.
 * pfft_execute_dct: scalar j of row t is read from in + t * in_pitch + j and written to out + t * out_pitch + j (pitches
 * in scalars); only those N * n_rows scalars are written.  In place -- in == out with in_pitch == out_pitch -- is
 * allowed.
 * PFFT_INVALID_CONFIGURATION: a plan that is not REAL, pfft_plan_prepare_dct not called, null pointers, n_rows == 0, a
 * type other than 2 or 3, a pitch below N, in == out with different pitches, byte ranges of input and output that overlap
 * without being identical.
 * PFFT_UNSUPPORTED_CONFIGURATION: 2^31 or more rows; the rows of one work-group spanning 4 GiB or more -- a work-group
 * holds ffts_per_workgroup rows (pfft_plan_get_info) and that count times the pitch in bytes must stay below 2^32 on both
 * sides, however few rows the call has.  Nothing is compiled or allocated at execute.  The _ex form takes dependencies and returns an event like pfft_execute_ex. */
enum { PFFT_DCT_II = 2, PFFT_DCT_III = 3 };
pfft_status pfft_plan_prepare_dct(pfft_plan_t* plan);
pfft_status pfft_execute_dct(pfft_plan_t* plan, int32_t type, const void* in, void* out, uint64_t n_rows,
                             uint64_t in_pitch, uint64_t out_pitch);
pfft_status pfft_execute_dct_ex(pfft_plan_t* plan, int32_t type, const void* in, void* out, uint64_t n_rows,
                                uint64_t in_pitch, uint64_t out_pitch, int32_t n_deps, void* const* deps,
                                void** event_out);
/* Discrete cosine transform of type 4 of packed real rows, and the modified discrete cosine transform (MDCT) of long real
 * signals (no reference equivalent; no extension bit): two more pairs of verbs on every plan of the REAL domain, whose
 * commit is unchanged.  One kernel launch per call: an M-point complex transform (M = N / 2, N = lengths[0]) between two
 * twiddle multiplies, all in LDS; no untangle step.  Lengths: those of the real transforms (even N >= 4).
 *   dct4:  y[k] = scale * 2 * sum_{n=0}^{N-1} x[n] cos(pi (2n + 1)(2k + 1) / (4N))                          k = 0 ... N - 1
 * is scipy.fft.dct(x, 4, norm=None) times forward_scale, or times backward_scale when `inverse` is not 0.  The kernel is
 * the same in both directions: with scales of 1, dct4 of dct4 of x is 2 * N * x.
 *   mdct:  X[i,f,k] = forward_scale * 2 * sum_{n=0}^{2N-1} w[n] xe_i[f * N - lead + n] cos(pi (2n + 1 + N)(2k + 1) / (4N))
 * for frame f < n_frames of signal i < n_signals and k = 0 ... N - 1: a frame covers 2N samples, the hop is N (the
 * transform's definition, not a parameter), xe_i is signal i extended by zeros outside [0, in_length), w is a window of 2N
 * scalars, lead is in [0, 2N) and usually N.  With a window that satisfies the Princen-Bradley condition (the sine window),
 * lead = N and ceil(in_length / N) + 1 frames, dct4 of the coefficient rows, the unfold of a row y = [p, q] (halves of
 * N / 2) to the 2N samples [q, -reverse(q), -reverse(p), -p], the window again and the overlap-add at hop N give 2N * x
 * (time-domain alias cancellation).  pfft_execute_imdct (below) does that unfold, window and overlap-add in one kernel;
 * pfft_execute_dct4 of the coefficient rows plus the caller's own unfold remains possible.
 * pfft_plan_prepare_dct4: takes no data.  The first call resolves the kernels (pre-compiled for the power-of-two lengths
 * of the real kernels, otherwise compiled here by hiprtc and cached like every other kernel) and uploads a table of N
 * twiddles into memory the plan owns, with the rules of pfft_plan_set_filter: pfft_plan_clone shares both, refused inside
 * a stream capture.  Later calls do nothing.  No other call prepares implicitly.
 * pfft_plan_set_mdct_window: does what pfft_plan_prepare_dct4 does, then copies the 2N scalars of `window` (device
 * memory; NULL: ones) on the plan's stream into memory the plan owns; every call uploads again; refused inside a stream
 * capture.
 * pfft_execute_dct4: scalar j of row t is read from in + t * in_pitch + j and written to out + t * out_pitch + j (pitches
 * in scalars); only those N * n_rows scalars are written.  In place -- in == out with in_pitch == out_pitch -- is allowed.
 * pfft_execute_mdct: sample s of signal i is read from in + i * in_pitch + s; coefficient k of frame f of signal i is
 * written to out + i * out_pitch + f * frame_pitch + k (all in scalars); nothing else is written.  Not in place: frames
 * overlap.
 * PFFT_INVALID_CONFIGURATION: a plan that is not REAL, the prepare / window call missing, null pointers, zero counts;
 * dct4: a pitch below N, in == out with different pitches, byte ranges that overlap without being identical; mdct:
 * lead >= 2N, in_pitch < in_length, frame_pitch < N, out_pitch < n_frames * frame_pitch, a last frame that holds no sample
 * ((n_frames - 1) * N >= in_length + lead), overlapping byte ranges.
 * PFFT_UNSUPPORTED_CONFIGURATION: 2^31 or more rows or (signal, frame) pairs; a count or pitch of 2^32 or more; dct4: the
 * rows of one work-group spanning 4 GiB or more -- ffts_per_workgroup rows (pfft_plan_get_info) times the pitch in bytes
 * must stay below 2^32 on both sides, however few rows the call has; mdct: the signals and output rows one work-group
 * touches spanning 4 GiB or more.  Nothing is compiled or allocated at execute.  The _ex forms take dependencies and
 * return an event like pfft_execute_ex. */
pfft_status pfft_plan_prepare_dct4(pfft_plan_t* plan);
pfft_status pfft_execute_dct4(pfft_plan_t* plan, int32_t inverse, const void* in, void* out, uint64_t n_rows,
                              uint64_t in_pitch, uint64_t out_pitch);
pfft_status pfft_execute_dct4_ex(pfft_plan_t* plan, int32_t inverse, const void* in, void* out, uint64_t n_rows,
                                 uint64_t in_pitch, uint64_t out_pitch, int32_t n_deps, void* const* deps,
                                 void** event_out);
pfft_status pfft_plan_set_mdct_window(pfft_plan_t* plan, const void* window);
pfft_status pfft_execute_mdct(pfft_plan_t* plan, const void* in, void* out, uint64_t n_signals, uint64_t in_length,
                              uint64_t in_pitch, uint64_t lead, uint64_t n_frames, uint64_t frame_pitch,
                              uint64_t out_pitch);
pfft_status pfft_execute_mdct_ex(pfft_plan_t* plan, const void* in, void* out, uint64_t n_signals, uint64_t in_length,
                                 uint64_t in_pitch, uint64_t lead, uint64_t n_frames, uint64_t frame_pitch,
                                 uint64_t out_pitch, int32_t n_deps, void* const* deps, void** event_out);
/* Inverse modified discrete cosine transform (windowed overlap-add synthesis with time-domain alias cancellation) of real
 * signals (no reference equivalent; no extension bit): one more pair of verbs on every plan of the REAL domain, whose
 * commit, pfft_plan_prepare_dct4, pfft_execute_dct4, pfft_plan_set_mdct_window and pfft_execute_mdct are unchanged.  One
 * kernel launch reads the frame-major coefficients pfft_execute_mdct writes, runs the type-4 transform of every frame in
 * LDS, unfolds it, multiplies it by the synthesis window and adds the two frames that cover a sample: no frame buffer, no
 * atomics, no zeroed output -- every coefficient is read once per chunk that needs it, every sample written once with a
 * plain store.  N = lengths[0], M = N / 2.  For a coefficient row X let Y[k] = 2 * sum_{n=0}^{N-1} X[n] cos(pi (2n + 1)
 * (2k + 1) / (4N)) (the unscaled dct4), Y = [p, q] in halves of M; the unfolded frame is g = [q, -reverse(q), -reverse(p),
 * -p], 2N scalars, g[n] = 2 * sum_k X[k] cos(pi (2n + 1 + N)(2k + 1) / (4N)).  For t < out_length, with u = t + lead:
 *   y_i[t] = backward_scale * sum_f w[u - f * N] * g_i[f][u - f * N]      over the frames 0 <= f < n_frames with 0 <= u - f * N < 2N
 * At most two frames cover a sample; they are added in ascending f, a frame that does not exist adds +0, wherever the
 * work is cut: the result does not depend on chunk_frames or on the launch grid, bit for bit.  With the sine window on
 * both sides, lead = N, ceil(L / N) + 1 frames, forward_scale = 1 and backward_scale = 1 / (2N), the inverse of
 * pfft_execute_mdct of x is x.
 * pfft_plan_set_imdct_window: `window` is a device pointer to 2N real scalars of the plan's precision; NULL = all ones.
 * Independent of pfft_plan_set_mdct_window.  Does what pfft_plan_prepare_dct4 does; the first call also resolves the
 * kernel (pre-compiled for the power-of-two lengths of the real kernels, otherwise compiled here by hiprtc and cached like
 * every other kernel); every call copies the window on the plan's stream into memory the plan owns, with the rules of
 * pfft_plan_set_filter: pfft_plan_clone shares it until either side sets another, refused inside a stream capture.
 * pfft_execute_imdct: coefficient k of frame f of signal i is read from in + i * in_pitch + f * frame_pitch + k, sample t
 * of signal i goes to out + i * out_pitch + t (all in scalars); only those out_length * n_signals scalars are written.
 * Not in place.  The work is cut into chunks of chunk_frames frames per signal, each preceded by a recomputed halo of one
 * frame; 0 lets the plan choose (as large as still fills the device, at least four frames).
 * PFFT_INVALID_CONFIGURATION: a plan that is not REAL, no window set, null pointers, zero counts, lead >= 2N,
 * frame_pitch < N, in_pitch < n_frames * frame_pitch, out_pitch < out_length, out_length > (n_frames - 1) * N + 2N - lead
 * (a sample no frame covers), (n_frames - 1) * N >= out_length + lead (a frame that contributes nothing), overlapping
 * byte ranges of input and output.
 * PFFT_UNSUPPORTED_CONFIGURATION: a count or pitch of 2^32 or more; 2^31 or more (signal, frame) rows; the coefficients
 * or the samples one work-group touches span 4 GiB or more (a smaller chunk_frames shortens both); at
 * pfft_plan_set_imdct_window, a carry of M scalars that does not fit into LDS behind the images.  Nothing is compiled or
 * allocated at execute.  The _ex form takes dependencies and returns an event like pfft_execute_ex.
 * pfft_plan_imdct_chunk_frames: the chunk length that chunk_frames = 0 stands for in a call with these counts (a window
 * must have been set); about 1 / chunk_frames of the frames are transformed twice. */
pfft_status pfft_plan_set_imdct_window(pfft_plan_t* plan, const void* window);
pfft_status pfft_plan_imdct_chunk_frames(const pfft_plan_t* plan, uint64_t n_signals, uint64_t n_frames,
                                         uint64_t* chunk_frames);
pfft_status pfft_execute_imdct(pfft_plan_t* plan, const void* in, void* out, uint64_t n_signals, uint64_t n_frames,
                               uint64_t frame_pitch, uint64_t in_pitch, uint64_t lead, uint64_t out_length,
                               uint64_t out_pitch, uint64_t chunk_frames);
pfft_status pfft_execute_imdct_ex(pfft_plan_t* plan, const void* in, void* out, uint64_t n_signals, uint64_t n_frames,
                                  uint64_t frame_pitch, uint64_t in_pitch, uint64_t lead, uint64_t out_length,
                                  uint64_t out_pitch, uint64_t chunk_frames, int32_t n_deps, void* const* deps,
                                  void** event_out);
/* Power spectrogram and Welch periodogram of long real signals (no reference equivalent; no extension bit): one more pair
 * of verbs on every plan of the REAL domain, whose commit, pfft_plan_set_window and pfft_execute_stft are unchanged.  One
 * kernel launch computes the frames of pfft_execute_stft, squares every bin in registers and adds avg_frames consecutive
 * frames before it stores: the complex bins never reach memory.  N = lengths[0], M = N / 2.  With X_i[f][k] exactly what
 * pfft_execute_stft defines (window, forward_scale inside, PFFT_PAD_ZERO / PFFT_PAD_REFLECT, any hop and lead), F =
 * n_frames, A = avg_frames and R = ceil(F / A) output rows per signal:
 *   P_i[c][k] = sum over f = c * A ... min((c + 1) * A, F) - 1 of |X_i[f][k]|^2          k = 0 ... M,  c < R
 * A = 1 is the power spectrogram, A = F Welch's sum with one row per signal.  The result is a SUM, not a mean, and bins
 * are not doubled for a one-sided spectrum: the caller normalises, or folds the factor into forward_scale (it enters
 * squared).  Every (i, c, k) has one accumulator that takes its frames in ascending f: the result does not depend on the
 * launch grid or on how many signals share a call, bit for bit; no atomics.  One output row is one work-group's lane-set:
 * at A = F a single signal is one unit on one work-group, so a Welch estimate of ONE long signal should choose A so that
 * n_signals * R is a few thousand and add the R rows afterwards.
 * pfft_plan_set_periodogram_window: `window` is a device pointer to N real scalars of the plan's precision; NULL = all
 * ones.  Independent of pfft_plan_set_window.  The first call resolves the kernel (pre-compiled for the power-of-two
 * lengths of the real kernels, otherwise compiled here by hiprtc and cached like every other kernel); every call copies
 * the window on the plan's stream into memory the plan owns, with the rules of pfft_plan_set_filter: pfft_plan_clone
 * shares it until either side sets another, refused inside a stream capture.
 * pfft_execute_periodogram: signal i starts i * in_pitch scalars behind `in`; bin k of row c of signal i goes to out +
 * i * out_pitch + c * row_pitch + k, in real scalars of the plan's precision; only those (M + 1) * R * n_signals scalars
 * are written.  Not in place.
 * PFFT_INVALID_CONFIGURATION: what pfft_execute_stft refuses (with row_pitch < M + 1 and out_pitch < R * row_pitch for its
 * two output pitches), avg_frames == 0, avg_frames > n_frames, no window set.
 * PFFT_UNSUPPORTED_CONFIGURATION: a count, length or pitch of 2^32 or more; 2^31 or more (signal, row) units; the signals,
 * or the output rows, that one work-group's units touch span 4 GiB or more.  Nothing is compiled or allocated at execute.
 * The _ex form takes dependencies and returns an event like pfft_execute_ex. */
pfft_status pfft_plan_set_periodogram_window(pfft_plan_t* plan, const void* window);
pfft_status pfft_execute_periodogram(pfft_plan_t* plan, const void* in, void* out, uint64_t n_signals, uint64_t in_length,
                                     uint64_t in_pitch, uint64_t hop, uint64_t lead, int32_t pad_mode, uint64_t n_frames,
                                     uint64_t avg_frames, uint64_t row_pitch, uint64_t out_pitch);
pfft_status pfft_execute_periodogram_ex(pfft_plan_t* plan, const void* in, void* out, uint64_t n_signals, uint64_t in_length,
                                        uint64_t in_pitch, uint64_t hop, uint64_t lead, int32_t pad_mode, uint64_t n_frames,
                                        uint64_t avg_frames, uint64_t row_pitch, uint64_t out_pitch, int32_t n_deps,
                                        void* const* deps, void** event_out);
/* Circular convolution and correlation of PAIRS of real rows, with the phase transform of generalised cross-correlation
 * (GCC-PHAT) (no reference equivalent; no extension bit): one more pair of verbs on every plan of the REAL domain, whose
 * commit is unchanged.  Both operands are data of the call -- cross-correlation of two channels, autocorrelation, matched
 * filtering against a template that arrives with the data -- where pfft_execute_convolve multiplies with a filter the
 * plan owns.  One kernel launch per call: row t of x and row t of y are read once, transformed in LDS (M = N / 2 points
 * each, N = lengths[0]), untangled and multiplied there, and one inverse transform stores the result row; the spectra
 * never reach memory.  Row t of x holds x_length <= N scalars, row t of y y_length <= N; the kernel extends both with
 * zeros to N as it loads (xe, ye below), so no padded copy is needed.  With X = rfft(xe), Y = rfft(ye), unscaled:
 *   PFFT_CONVOLVE   r_t[l] = c * N * sum_{n<N} xe_t[n] * ye_t[(l - n) mod N]      = c * N * irfft(X * Y)
 *   PFFT_CORRELATE  r_t[l] = c * N * sum_{n<N} xe_t[(n + l) mod N] * ye_t[n]      = c * N * irfft(X * conj(Y))
 *         c = forward_scale^2 * backward_scale, what two forward transforms, a product and a backward one give; irfft
 *         is NumPy's, which divides by N, and the backward transform is unnormalised as in pfft_execute_convolve:
 *         backward_scale = 1 / N gives the plain sums
 *   PFFT_CORRELATE with phat_floor = f > 0:   P = X * conj(Y),  W[k] = P[k] / max(|P[k]|, f),
 *                   r_t = backward_scale * N * irfft(W)
 * for l = 0 ... out_length - 1, out_length <= N: only those scalars of every result row are written.  With x_length +
 * y_length - 1 <= N nothing aliases: PFFT_CONVOLVE is then c * N times the linear convolution (numpy.convolve(x, y), zeros behind it),
 * and PFFT_CORRELATE holds the lags 0 ... x_length - 1 at r[0 ...] and the lags -1 ... -(y_length - 1) at r[N - 1]
 * downwards.  The sign convention is that of pfft_execute_filter with PFFT_CORRELATE, y in the filter's place.  The phase
 * transform keeps the phase of every bin and sets its magnitude to 1 where it is above the floor; below the floor a bin
 * keeps its magnitude divided by the floor, so a bin of two silent channels stays 0 instead of becoming noise of
 * magnitude 1.  The real bins 0 and M become a sign, or a fraction below the floor.  |P[k]| is formed without squaring
 * numbers of P's magnitude, so the branch is right wherever P[k] itself is a finite, normal number of the plan's type
 * (fp32: about 1e-38 ... 3e38; rows of N = 16384 samples of magnitude 1e8 give |P| near 1e20, inside it); where the
 * product X * conj(Y) overflows or is subnormal in that type the result is what such a product gives.
 * pfft_plan_prepare_pairs: takes no data.  The first call resolves the kernels (pre-compiled for the power-of-two lengths
 * of the real kernels, otherwise compiled here by hiprtc and cached like every other kernel); it reads the plan's own
 * twiddle tables and uploads nothing; pfft_plan_clone shares the result.  Later calls do nothing -- except inside a stream
 * capture, where every call is refused, also one that would do nothing (as pfft_plan_prepare_dct4).  No other call prepares implicitly.  The kernel keeps two images per row in LDS: a length whose two image sets
 * do not fit the device's LDS -- beyond the pre-compiled ones, roughly N above 19000 in fp32 -- is refused here with
 * PFFT_UNSUPPORTED_CONFIGURATION.
 * pfft_execute_pairs: scalar j of row t is read from x + t * x_pitch + j and y + t * y_pitch + j and written to out + t *
 * out_pitch + j (lengths and pitches in scalars).  x and y may be the same buffer: that is autocorrelation.  out must
 * overlap neither.  The descriptor's number_of_transforms, distances and offsets do not apply; the precision, N and the
 * two scales do.
 * PFFT_INVALID_CONFIGURATION: a plan that is not REAL, the prepare call missing, then in this order: a null pointer, a
 * mode that is neither PFFT_CONVOLVE nor PFFT_CORRELATE, n_rows 0, a length of 0 or above N, a pitch below its length, a
 * phat_floor that is negative, not finite, or positive and not a normal number of the plan's scalar type, a phat_floor
 * other than 0 with PFFT_CONVOLVE, byte ranges of out that overlap those of x or y.
 * PFFT_UNSUPPORTED_CONFIGURATION, in this order: 2^31 or more rows; a pitch of 2^32 or more; the rows of one work-group
 * spanning 4 GiB or more -- ffts_per_workgroup rows (pfft_plan_get_info) times the pitch in bytes must stay below 2^32 on
 * all three sides, however few rows the call has.  Nothing is compiled or allocated at execute.  The _ex form takes
 * dependencies and returns an event like pfft_execute_ex. */
pfft_status pfft_plan_prepare_pairs(pfft_plan_t* plan);
pfft_status pfft_execute_pairs(pfft_plan_t* plan, int32_t mode, const void* x, const void* y, void* out, uint64_t n_rows,
                               uint64_t x_length, uint64_t x_pitch, uint64_t y_length, uint64_t y_pitch,
                               uint64_t out_length, uint64_t out_pitch, double phat_floor);
pfft_status pfft_execute_pairs_ex(pfft_plan_t* plan, int32_t mode, const void* x, const void* y, void* out,
                                  uint64_t n_rows, uint64_t x_length, uint64_t x_pitch, uint64_t y_length,
                                  uint64_t y_pitch, uint64_t out_length, uint64_t out_pitch, double phat_floor,
                                  int32_t n_deps, void* const* deps, void** event_out);
/* sycl::event::wait() / get_info<command_execution_status>() / destruction of an event returned by the _ex calls. */
pfft_status pfft_event_wait(void* event);
pfft_status pfft_event_query(void* event, int32_t* done);
pfft_status pfft_event_destroy(void* event);
/* committed_descriptor's copy constructor / copy assignment (committed_descriptor_impl.hpp:774-817): the copy shares
 * the kernels and twiddle tables and gets scratch buffers of its own. */
pfft_status pfft_plan_clone(const pfft_plan_t* plan, pfft_plan_t** copy);
/* sycl::queue::copy(src, dest, count, dependencies) and sycl::queue::wait() as the reference's callers use them around
 * compute_* (test/unit_test/fft_test_utils.hpp:286-333, test/bench/portfft/launch_bench.hpp:96-135): an asynchronous
 * copy of `bytes` bytes on `hip_stream` (host or device pointers) behind `deps`, with its own completion event. */
pfft_status pfft_queue_copy(void* hip_stream, const void* src, void* dst, size_t bytes, int32_t n_deps,
                            void* const* deps, void** event_out);
pfft_status pfft_queue_wait(void* hip_stream);
/* Blocks until everything queued on the plan's stream is done (queue.wait() of the reference's destructor path). */
pfft_status pfft_plan_wait(pfft_plan_t* plan);

/* ---- misc ----------------------------------------------------------------------------------------------------- */
const char* pfft_last_error(void);
const char* pfft_status_string(pfft_status s);
/* "portfft_amd x.y (gfx950)" */
const char* pfft_version(void);

#ifdef __cplusplus
}
#endif
#endif /* PORTFFT_AMD_H */
