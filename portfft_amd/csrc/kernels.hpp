// Registry of the pre-compiled gfx950 kernels (host-visible interface of kernels_f32.hip / kernels_f64.hip).
//
// The reference JIT-specialises its kernels at commit time through SYCL specialization constants
// (/root/reference/src/portfft/committed_descriptor_impl.hpp:448-573).  Here the hand-tuned variants are
// offline-compiled template instantiations that commit only looks up; every other length gets the same templates
// instantiated at commit time by hiprtc (jit.hpp) -- those entries carry module functions instead of host symbols
// (the `mod` half of the kernel_fn cells of their form tables; `jit` is set).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdlib>

#include <cstddef>

#include "generic_args.hpp"
#include "strided_args.hpp"
#include "xcd_args.hpp"

namespace pfa {

/// One launchable kernel: the host symbol of a pre-compiled instantiation or the module function of one compiled at
/// commit (jit.cpp).  any_order: the form honours strided_args::any_order / rows2d_args::any_order (a launch without
/// the in-order barrier).  Empty (both null): the entry does not carry that form.
struct kernel_fn {
  const void* sym;
  hipFunction_t mod;
  bool any_order;
  explicit operator bool() const { return sym != nullptr || mod != nullptr; }
};

/// Launch `f` on `grid` work-groups of `wg` lanes; params: the kernel's arguments (hipLaunchKernel convention).  The
/// armed stop event (take_stop_event) rides the dispatch; any_order (honoured when f.any_order) drops the in-order
/// barrier (hipExtAnyOrderLaunch).  hipErrorInvalidValue for an empty f.
hipError_t launch_fn(const kernel_fn& f, unsigned grid, unsigned wg, size_t lds, hipStream_t stream, void** params,
                     bool any_order = false);
/// work-groups of `f` resident per CU at that LDS
hipError_t fn_occupancy(int* per_cu, const kernel_fn& f, int wg, size_t lds);
/// raise the dynamic-LDS limit of a pre-compiled kernel to `lds` bytes (module functions and empty forms: nothing to do)
hipError_t raise_lds_limit(const kernel_fn& f, size_t lds);

/// The forms of a packed entry (spec_kernel::form): one configuration instantiated for different storages and
/// argument lists.  The stage's form: stage::form; the argument list of each form: plan_t::run_stage.
enum spec_form : int {
  WF_INTERLEAVED,     // stockham_wg[_hx|_xlane|_prefetch][_half]_kernel, stockham_nd_kernel
  WF_SPLIT,           // SPLIT_COMPLEX planes: stockham_wg[_hx][_half]_split_kernel, stockham_nd_split_kernel
  WF_UNPACKED,        // runtime strides and distances: stockham_wg_unpacked_kernel (compiled at commit only)
  WF_UNPACKED_SPLIT,  // ... on split planes
  WF_REAL,            // [0] stockham_wg_r2c_kernel, [1] stockham_wg_c2r_kernel (stockham_wg_real.hpp)
  WF_BLUESTEIN,       // stockham_wg_bluestein_kernel (stockham_wg_bluestein.hpp)
  WF_CONV,            // stockham_wg_conv_kernel (stockham_wg_conv.hpp): [0] convolve, [1] correlate
  WF_OLS,             // stockham_wg_ols_kernel (stockham_wg_ols.hpp): [0] convolve, [1] correlate
  WF_RCONV,           // stockham_wg_rconv_kernel (stockham_wg_rconv.hpp): [0] convolve, [1] correlate, real rows
  WF_ROLS,            // stockham_wg_rols_kernel (stockham_wg_rols.hpp): [0] convolve, [1] correlate, real signals
  WF_STFT,            // stockham_wg_stft_kernel (stockham_wg_stft.hpp): [0] zero extension, [1] reflection, real signals
  N_SPEC_FORMS,
  /// The forms a plan resolves on demand, behind the commit-time ones (N_SPEC_FORMS counts those and stays what it was):
  WF_ISTFT = N_SPEC_FORMS,  // stockham_wg_istft_kernel (stockham_wg_istft.hpp): [0] plain overlap-add, [1] normalised
  N_SPEC_FORMS_ALL,
  /// The late forms: spec_kernel::form is full (its size is pinned), so a form added behind it lives in
  /// spec_kernel::late_form and is numbered on from N_SPEC_FORMS_ALL.  Every reader goes through spec_kernel::cells(form),
  /// which serves both tables; a new on-demand verb adds its form here.
  WF_DCT = N_SPEC_FORMS_ALL,  // stockham_wg_dct_kernel (stockham_wg_dct.hpp): [0] type 2, [1] type 3, real rows
  N_SPEC_FORMS_END,
  N_LATE_FORMS = N_SPEC_FORMS_END - N_SPEC_FORMS_ALL,
  /// The open forms: the size of spec_kernel::late_form is pinned as well, so the forms behind it live in
  /// spec_kernel::open_form, numbered on from N_SPEC_FORMS_END, and nothing pins how many there are: the next on-demand
  /// verb adds a line in front of N_SPEC_FORMS_TOP and needs no fourth table.  cells(form) serves all three tables.
  WF_DCT4 = N_SPEC_FORMS_END,  // stockham_wg_dct4_kernel (stockham_wg_dct4.hpp): [0] DCT-IV of real rows, [1] MDCT of real signals
  WF_IMDCT,  // stockham_wg_imdct_kernel (stockham_wg_imdct.hpp): inverse MDCT of real signals; one kernel, in both cells
  WF_PERIODOGRAM,  // stockham_wg_periodogram_kernel (stockham_wg_periodogram.hpp): sums of squared STFT bins; [0] zero extension, [1] reflection
  WF_PAIRS,  // stockham_wg_pairs_kernel (stockham_wg_pairs.hpp): pairs of real rows; [0] product (convolution), [1] conjugate product (correlation)
  N_SPEC_FORMS_TOP,
  N_OPEN_FORMS = N_SPEC_FORMS_TOP - N_SPEC_FORMS_END
};

/// One specialised work-group kernel: packed FFTs of a fixed length.
struct spec_kernel {
  int precision;  // PFFT_PRECISION_*
  int n;
  int wg;   // threads per work-group
  int fpw;  // FFTs per work-group
  size_t lds_bytes;  // launch LDS of the entry's forms
  int n_radices;
  int radices[8];
  int tw_total;  // complex entries of the twiddle table the kernel expects (layout: radix_list::tw_off)
  int tw_in_regs;  // 1: the kernel keeps its twiddles in VGPRs for its whole lifetime (TW_REGS)
  int groups_per_wg;  // tuned grid rule: FFT groups each work-group handles; 0 = persistent grid of 2x resident
  /// the entry's kernels: form[spec_form][backward]; empty where the entry does not carry the form
  kernel_fn form[N_SPEC_FORMS_ALL][2];
  bool jit;  // compiled at commit (jit.cpp): module functions; false: pre-compiled host symbols
  /// 1: WF_INTERLEAVED is a prefetching kernel (stockham_wg_prefetch[_half]_kernel): the trailing (n_main, main_k)
  /// arguments and the two-tier grid of large launches (plan_exec.cpp: two_tier_grid)
  int two_tier;
  /// the remaining wg_cfg arguments, so that other forms of the same configuration (UNPACKED layouts, real data) can be
  /// instantiated at run time
  int pads, padw, twm, occ, aux, staged, twl;
  /// 1: cross-lane variant of the length (stockham_xlane.hpp); only chosen when PFFT_XLANE is set (measurement:
  /// profiles/r2_notes.md)
  int xlane;
  /// 1: register-resident form (stockham_wg_hx.hpp): the transform does not fit LDS, lds_bytes is its half image; the
  /// wg_cfg fields above do not describe a configuration the other packed forms (UNPACKED layouts) could be built from
  int hx;
  /// the cells of the late forms (WF_DCT ...): late_form[form - N_SPEC_FORMS_ALL][mode]
  kernel_fn late_form[N_LATE_FORMS][2];
  /// the cells of the open forms (WF_DCT4, WF_IMDCT, WF_PERIODOGRAM, WF_PAIRS ...): open_form[form - N_SPEC_FORMS_END][mode]
  kernel_fn open_form[N_OPEN_FORMS][2];
  /// The two cells of `f`, any spec_form: the one accessor for a form that is not a compile-time constant of the first
  /// table (set_spec_form, jit_fused_kernel, push_fused_stage, run_stage and the verbs' launches).  No caller learns which
  /// table a form is in.
  kernel_fn (&cells(int f))[2] {
    return f < N_SPEC_FORMS_ALL ? form[f] : f < N_SPEC_FORMS_END ? late_form[f - N_SPEC_FORMS_ALL] : open_form[f - N_SPEC_FORMS_END];
  }
  const kernel_fn (&cells(int f) const)[2] {
    return f < N_SPEC_FORMS_ALL ? form[f] : f < N_SPEC_FORMS_END ? late_form[f - N_SPEC_FORMS_ALL] : open_form[f - N_SPEC_FORMS_END];
  }
};

/// Launch grid and trailing arguments of form `form` of `k` when the planner's uniform grid is `grid` (k groups per
/// work-group).  Only the WF_INTERLEAVED cell of a two_tier entry is a prefetching kernel: for large launches three
/// quarters of its groups keep the uniform shape (n_main work-groups of main_k groups) and the last quarter goes to
/// work-groups of 2 groups each.  Every other cell, and a small launch, keeps `grid` (n_main = 0).
void two_tier_grid(const spec_kernel& k, int form, long long nfft, unsigned* grid, long long* n_main, int* main_k);

/// The forms of a strided entry (strided_kernel::form): one configuration instantiated for different storages and
/// shapes.  The stage's form: plan_t::strided_form_of.
enum strided_form : int {
  SF_PLAIN,      // interleaved on both sides
  SF_STW,        // ... with the store modifier (tables in LDS behind the kernel's own when stw_mode is 1)
  SF_SPLIT,      // SPLIT_COMPLEX planes on both sides
  SF_SPLIT_STW,  // ... with the store modifier (S1 of the three-stage plan; compiled at commit only)
  SF_MIXED_IN,   // split planes in, interleaved scratch out, store modifier (four-step stage A; compiled at commit only)
  SF_MIXED_OUT,  // interleaved scratch in, split planes out (stage B; compiled at commit only)
  SF_ROW_IN,     // row-staged input (stockham_strided_row_kernel; lds_bytes_row)
  SF_ROW_OUT,    // row-staged output
  SF_ROW_MIXED,  // row-staged input of SF_MIXED_OUT (compiled at commit only)
  SF_TIN,        // tiled input: four-step stage B behind a group-major stage A (pre-compiled only; fs_ltw: LDS tables)
  SF_TIN_W,      // ... for tiles of tin_w = 2 * fpw elements (pre-compiled only)
  SF_MIXED_TIN,  // tiled input of SF_MIXED_OUT (stockham_strided_kernel<Cfg, BWD, 0, 3, TIN = true>; compiled at commit only)
  N_STRIDED_FORMS
};

/// One strided work-group kernel (stockham_strided.hpp): FPW FFTs side by side, any element stride / FFT distance.
struct strided_kernel {
  int precision;
  int n;
  int wg;
  int fpw;
  size_t lds_bytes;
  int n_radices;
  int radices[8];
  int groups_per_wg;  // tuned grid rule (see spec_kernel)
  /// the entry's kernels: form[strided_form][backward]; empty where the entry does not carry the form
  kernel_fn form[N_STRIDED_FORMS][2];
  bool jit;  // compiled at commit (jit.cpp): module functions; false: pre-compiled host symbols
  size_t lds_bytes_row;  // LDS of the row-staged forms
  /// tile width of SF_TIN_W (2 * fpw), 0 when the entry does not carry it
  int tin_w;
  /// cache policy of the entry's HBM accesses (stockham_wg.hpp, aux_of_loads / aux_of_stores): 0 everything streamed
  /// (nt), 1 "writer" (streamed loads, default-policy stores: fills an intermediate that should stay in the
  /// Infinity Cache), 2 "reader" (default-policy loads, streamed stores).  Policy twins carry the interleaved forms only.
  int policy;
  /// 1: alternative entry for the same length, preferred when both sides of the stage are column-shaped
  int wide;
  /// 1: alternative entry preferred when one side of the stage is row-shaped (its `_row` forms pay at this length)
  int rowish;
  /// where the store-modifier forms take their tables from (stockham_strided.hpp, STW): 1 small multi-level tables in
  /// LDS (every pre-compiled entry), 2 two global tables (runtime-specialised entries without LDS headroom)
  int stw_mode;
  /// four-step (GLOBAL tier) stage entries: fs_a = the entry of its length for stage A (store modifier, writes the
  /// group-major intermediate), fs_b = for stage B (tiled-input form, SF_TIN).  A pair (fs_a, fs_b) with equal
  /// group widths replaces the default entries of the two lengths (tools/tune_fourstep.hip, profiles/r3_notes.md:
  /// narrow groups at two to four work-groups per CU beat wide ones at one).  fs_groups_per_wg: grid rule inside
  /// such a pair (0: groups_per_wg).
  int fs_a, fs_b, fs_groups_per_wg;
  int fs_only;  // 1: the entry exists only for such pairs (never the default entry of its length)
  /// 1 (fs_b entries): as stage B of a pair this entry carries the inter-stage twiddles on its LOADS (its tiled-input
  /// form multiplies the inputs of pass 0: strided_pass0_compute LTW) and stage A runs without the store modifier --
  /// fp64 n = 1024 (C3): stage A 120 -> 108 us per chunk, stage B 90 -> 91-94 (tools/tune_fourstep.hip case 120)
  int fs_ltw;
  /// > 0 (runtime-compiled entries): the register-resident form (stockham_strided_hx.hpp) planned as that many work-groups
  /// per CU; lds_bytes is its HALF image (+ TWL copy), the interleaved / split / mixed forms are that kernel's, the
  /// row-staged forms stay those of stockham_strided.hpp and there are no tiled-input forms
  int hx;
  /// 1 (runtime-compiled entries): the BIG forms (strided_io_big: groups that span 4 GiB or more); such an entry serves nothing else
  int big;
};

/// storage forms of a rows-2D entry: interleaved, SPLIT_COMPLEX on both sides (rows2d_args::in_im / out_im)
enum rows2d_form : int { R2_INTERLEAVED, R2_SPLIT, N_ROWS2D_FORMS };

/// First pass of the two-pass 2-D plan (stockham_rows2d.hpp): whole row FFTs of length n + the first radix-rc
/// butterfly of the column FFT, rows {M*a + b} -> rows {rc*b + u}.
struct rows2d_kernel {
  int precision;
  int n;   // row length
  int rc;  // column radix taken in this pass (rows per work-group)
  int wg;
  size_t lds_bytes;
  int n_radices;
  int radices[8];
  int groups_per_wg;
  /// form[rows2d_form][backward]; empty where the entry does not carry the form
  kernel_fn form[N_ROWS2D_FORMS][2];
  bool jit;   // compiled at commit (jit.cpp): module functions, one storage per entry
  int policy;  // see strided_kernel::policy (0 or 1)
};
const rows2d_kernel* rows2d_kernels(int* count);

/// XCD-local four-step kernel (stockham_xcd.hpp): both stages of an n1 x n2 transform in one persistent launch
struct xcd_kernel {
  int precision;
  int n1, n2;
  int wg, fpw;        // lanes of the launch's work-groups; columns (stage A) / rows (stage B) of a group
  int tasks_a, tasks_b;  // tickets of a transform per stage (a task = wg / stage-wg groups side by side)
  /// LDS layout (bytes from the dynamic base, xcd_layout): the leading twiddle tables of the two stages, the
  /// store-modifier tables; the launch adds those tables (16-byte rounded) and XCD_LDS_CTL_BYTES of control words
  unsigned twl_a_off, twl_b_off, stw_off;
  int n_radices_a, n_radices_b;
  int radices_a[8], radices_b[8];
  kernel_fn fn[2];  // [backward]; argument: xcd_args
  /// the recovery launch that follows every launch (stockham_xcd_recover_kernel; arguments: xcd_args, int phase =
  /// XCD_RECOVER_*, xcd_args.hpp)
  kernel_fn fn_recover[2];
  int slots, lag, lookahead;  // tuned schedule (xcd_args)
  int wg_per_cu;              // work-groups per CU the launch is padded to (0: as many as fit)
  int min_mib;                // MiB of data per execute from which the launch beats the two-launch plan
};
const xcd_kernel* xcd_kernels(int* count);
/// XCC ids the device hands to work-groups (0: the census failed)
int xcd_census(hipStream_t stream);

/// AUX template values of the three cache policies (stockham_wg.hpp: loads in bits 0-7, stores + 1 in bits 8-15;
/// hardware bits 1 = sc0, 2 = nt, 16 = sc1).  The writer's stores carry sc1: written through the XCD's L2 instead of
/// left dirty in it until the end of the launch, still allocated in the Infinity Cache (tools/tune_2d_small.hip,
/// TUNE_STORE_POLICY: C5 in 256 MiB chunks 1405 us with plain stores, 1378 with sc1 or sc0|sc1, 1590 with nt).
enum : int { PFA_AUX_NT = 2, PFA_AUX_WRITER = ((16 + 1) << 8) | 2, PFA_AUX_READER = 0x300 };
/// (runtime-specialised kernels, jit.cpp; PFFT_JIT_WRITER_AUX overrides the writer's value for experiments)
inline int aux_of_policy(int policy) {
  if (policy == 1) {
    if (const char* e = getenv("PFFT_JIT_WRITER_AUX")) return static_cast<int>(std::strtol(e, nullptr, 0));
    return PFA_AUX_WRITER;
  }
  if (policy == 0) {
    if (const char* e = getenv("PFFT_JIT_NT_AUX")) return static_cast<int>(std::strtol(e, nullptr, 0));  // (experiments)
  }
  // policy 3 (round 6, kernels compiled at commit only): default policy on loads AND stores -- for stages whose column-shaped
  // side has a row pitch that is no multiple of a 128-byte line: every segment shares its first and last line with the
  // neighbouring group, and only lines that live in the L2 are fetched once and written back whole (with the XCD-contiguous
  // walk the neighbours run on one L2).  Streamed (nt) accesses left batch-interleaved N = 768 at a batch of 174 769 at 0.225
  // of the HBM peak against 0.616 at 174 768; with this policy 0.506 (profiles/r6_bi_unaligned_policies.txt).
  if (policy == 3) return 0;
  // (NOT for the four-step stages of lengths like 68640 = 104 x 660 or 10^6, whose pitches are unaligned too: on default policies
  //  -- both sides, or the user's side only -- they lose 10-26 %, profiles/r6_unaligned_policy.txt / r6_fs_unaligned.txt: there the
  //  streamed user side is what keeps the intermediate in the Infinity Cache)
  return policy == 2 ? PFA_AUX_READER : PFA_AUX_NT;
}

/// Completion event of the submission being enqueued (pfft_execute*_ex with event_out): plan_t::execute arms it in
/// front of its LAST launch, the launch helper (launch_fn) takes it and hands it to
/// hipExtLaunchKernel / hipExtModuleLaunchKernel as the dispatch's stop event -- no separate hipEventRecord packet
/// behind a small transform (tools/latency.py).  Thread-local; whoever armed it records the event the ordinary way
/// when no launch helper took it.
void arm_stop_event(hipEvent_t ev);
hipEvent_t take_stop_event();  // the armed event (and disarms), or nullptr

const strided_kernel* strided_kernels_f32(int* count);
const strided_kernel* strided_kernels_f64(int* count);

const spec_kernel* spec_kernels_f32(int* count);
const spec_kernel* spec_kernels_f64(int* count);
/// fp16 storage (PFFT_PRECISION_F16, kernels_f16.hip): precision F16, the fp32 configurations of the power-of-two lengths
const spec_kernel* spec_kernels_f16(int* count);

/// Real-data forms (stockham_wg_real.hpp) of an LDS-resident packed configuration of M = N / 2 points: WF_REAL only, [0]
/// the real-to-complex kernel (forward), [1] the complex-to-real one (backward); lds_bytes is real_lds_bytes<Cfg>(), an
/// image also for single-pass configurations.  A registry of its own (kernels_real.hip: precision F32 / F64, keyed by
/// n = M), apart from the complex entries of the same lengths; jit_fused_kernel (jit.hpp, JF_REAL) makes the entries of other lengths.
const spec_kernel* real_kernels(int* count);

/// Bluestein form (stockham_wg_bluestein.hpp) of an LDS-resident packed configuration of P points, P a power of two:
/// complex transforms of any length N with 2N - 1 <= P (N is a kernel argument).  WF_BLUESTEIN only; lds_bytes is
/// bluestein_lds_bytes<Cfg>().  A registry of its own (kernels_bluestein.hip: precision F32 / F64, keyed by n = P).
const spec_kernel* bluestein_kernels(int* count);

/// Convolution forms (stockham_wg_conv.hpp) of an LDS-resident packed configuration of N points: WF_CONV only, [0] the
/// convolving kernel, [1] the correlating one (the conjugate spectrum); lds_bytes is conv_lds_bytes<Cfg>(), an image also
/// for single-pass configurations.  A registry of its own (kernels_conv.hip: precision F32 / F64, keyed by n = N), apart
/// from the complex entries of the same lengths; jit_fused_kernel (jit.hpp, JF_CONV) makes the entries of other lengths.
const spec_kernel* conv_kernels(int* count);

/// Overlap-save filter forms (stockham_wg_ols.hpp) of the same configurations: WF_OLS only, [0] / [1] as WF_CONV;
/// lds_bytes is ols_lds_bytes<Cfg>() (the convolution kernel's, and the row windows of a STAGED configuration).  A
/// registry of its own (kernels_ols.hip, the configuration list of wg_fused_cfg.hpp); jit_fused_kernel (jit.hpp, JF_OLS)
/// makes the entries of other lengths.
const spec_kernel* ols_kernels(int* count);

/// Real convolution forms (stockham_wg_rconv.hpp) and real overlap-save filter forms (stockham_wg_rols.hpp) of an
/// LDS-resident packed configuration of M = N / 2 points: WF_RCONV / WF_ROLS only, [0] / [1] as WF_CONV; lds_bytes is
/// real_lds_bytes<Cfg>() / rols_lds_bytes<Cfg>().  Registries of their own (kernels_rconv.hip, kernels_rols.hip: the
/// configuration list of wg_fused_cfg.hpp, keyed by n = M); jit_fused_kernel (jit.hpp, JF_RCONV / JF_ROLS) makes the
/// entries of other lengths.
const spec_kernel* rconv_kernels(int* count);
const spec_kernel* rols_kernels(int* count);

/// Short-time Fourier transform forms (stockham_wg_stft.hpp) of the same configurations: WF_STFT only, [0] the kernel
/// that extends a signal with zeros, [1] the one that reflects it; lds_bytes is stft_lds_bytes<Cfg>().  A registry of
/// its own (kernels_stft.hip: the configuration list of wg_fused_cfg.hpp, keyed by n = M); jit_fused_kernel (jit.hpp,
/// JF_STFT) makes the entries of other lengths.  Looked up at pfft_plan_set_window, not at commit.
const spec_kernel* stft_kernels(int* count);

/// Inverse short-time Fourier transform forms (stockham_wg_istft.hpp) of the same configurations: WF_ISTFT only, [0] the
/// plain overlap-add, [1] the one divided by the window envelope; lds_bytes is istft_lds_bytes<Cfg>() (the accumulator
/// behind the images).  A registry of its own (kernels_istft.hip, keyed by n = M); jit_fused_kernel (jit.hpp, JF_ISTFT)
/// makes the entries of other lengths.  Looked up at pfft_plan_set_synthesis_window, not at commit.
const spec_kernel* istft_kernels(int* count);

/// Discrete cosine transform forms (stockham_wg_dct.hpp) of the same configurations: WF_DCT only (a late form: cells()),
/// [0] type 2, [1] type 3; lds_bytes is dct_lds_bytes<Cfg>(), the real kernels'.  A registry of its own (kernels_dct.hip,
/// keyed by n = M); jit_fused_kernel (jit.hpp, JF_DCT) makes the entries of other lengths.  Looked up at
/// pfft_plan_prepare_dct, not at commit.
const spec_kernel* dct_kernels(int* count);

/// DCT-IV / MDCT forms (stockham_wg_dct4.hpp) of the same configurations: WF_DCT4 only (an open form: cells()), [0] the
/// type-4 transform of rows, [1] the MDCT of signals; lds_bytes is dct4_lds_bytes<Cfg>(), the real kernels'.  A registry
/// of its own (kernels_dct4.hip, keyed by n = M); jit_fused_kernel (jit.hpp, JF_DCT4) makes the entries of other lengths.
/// Looked up at pfft_plan_prepare_dct4 / pfft_plan_set_mdct_window, not at commit.
const spec_kernel* dct4_kernels(int* count);

/// Inverse MDCT form (stockham_wg_imdct.hpp) of the same configurations: WF_IMDCT only (an open form: cells()), one kernel
/// that fills both cells; lds_bytes is imdct_lds_bytes<Cfg>() (the carry of M scalars behind the images).  A registry of
/// its own (kernels_imdct.hip, keyed by n = M); jit_fused_kernel (jit.hpp, JF_IMDCT) makes the entries of other lengths.
/// Looked up at pfft_plan_set_imdct_window, not at commit.
const spec_kernel* imdct_kernels(int* count);

/// Power spectrogram / periodogram forms (stockham_wg_periodogram.hpp) of the same configurations: WF_PERIODOGRAM only (an
/// open form: cells()), [0] the kernel that extends a signal with zeros, [1] the one that reflects it; lds_bytes is
/// periodogram_lds_bytes<Cfg>().  A registry of its own (kernels_periodogram.hip, keyed by n = M); jit_fused_kernel
/// (jit.hpp, JF_PERIODOGRAM) makes the entries of other lengths.  Looked up at pfft_plan_set_periodogram_window, not at commit.
const spec_kernel* periodogram_kernels(int* count);

/// Pair convolution / correlation forms (stockham_wg_pairs.hpp) of the same configurations: WF_PAIRS only (an open form:
/// cells()), [0] the product of the two rows' spectra, [1] the product with the conjugate of the second; lds_bytes is
/// pairs_lds_bytes<Cfg>(), two image sets.  A registry of its own (kernels_pairs.hip, keyed by n = M); jit_fused_kernel
/// (jit.hpp, JF_PAIRS) makes the entries of other lengths.  Looked up at pfft_plan_prepare_pairs, not at commit.
const spec_kernel* pairs_kernels(int* count);

hipError_t launch_generic_f32(hipStream_t stream, unsigned grid, size_t lds_bytes, const generic_args& args);
hipError_t launch_generic_f64(hipStream_t stream, unsigned grid, size_t lds_bytes, const generic_args& args);
const void* generic_kernel_symbol(int precision, bool big_radix = false);

}  // namespace pfa
