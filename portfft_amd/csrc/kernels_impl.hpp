// Shared body of the kernels_*.hip files: turns wg_cfg<...> variants into registry entries.
#pragma once
#include <cstdlib>
#include <vector>

#include "../../include/portfft_amd.h"
#include "generic_kernel.hpp"
#include "kernels.hpp"
#include "stockham_rows2d.hpp"
#include "stockham_strided.hpp"
#include "stockham_wg.hpp"
#include "stockham_wg_hx.hpp"
#include "stockham_wg_conv.hpp"
#include "stockham_wg_dct.hpp"
#include "stockham_wg_dct4.hpp"
#include "stockham_wg_imdct.hpp"
#include "stockham_wg_istft.hpp"
#include "stockham_wg_ols.hpp"
#include "stockham_wg_pairs.hpp"
#include "stockham_wg_periodogram.hpp"
#include "stockham_wg_rconv.hpp"
#include "stockham_wg_real.hpp"
#include "stockham_wg_rols.hpp"
#include "stockham_wg_stft.hpp"
#include "stockham_xlane.hpp"

#include <type_traits>

namespace pfa {

/// the same configuration with another cache policy (AUX)
template <typename Cfg, int AUX2>
struct with_aux;
template <typename T, typename Seq, int WG, int FPW, int PADS, int PADW, int TWM, int OCC, int AUX, int STAGED, int TWL,
          int AUX2>
struct with_aux<wg_cfg<T, Seq, WG, FPW, PADS, PADW, TWM, OCC, AUX, STAGED, TWL>, AUX2> {
  using type = wg_cfg<T, Seq, WG, FPW, PADS, PADW, TWM, OCC, AUX2, STAGED, TWL>;
};
template <typename Cfg, int AUX2>
using with_aux_t = typename with_aux<Cfg, AUX2>::type;

/// one form of a pre-compiled entry: the forward / backward host symbols; any_order: the form honours the stage's
/// any_order (kernel_fn)
template <typename... A>
inline void set_form(kernel_fn (&f)[2], void (*fwd)(A...), void (*bwd)(A...), bool any_order) {
  f[0] = kernel_fn{reinterpret_cast<const void*>(fwd), nullptr, any_order};
  f[1] = kernel_fn{reinterpret_cast<const void*>(bwd), nullptr, any_order};
}

/// Host symbol of a kernel launched with a fixed argument array (generic tier, XCD-local launches): the formal
/// parameters must be exactly Want...
template <typename... Want, typename... A>
inline const void* checked_sym(void (*kernel)(A...)) {
  static_assert(std::is_same<void(std::remove_cv_t<A>...), void(Want...)>::value,
                "the kernel's parameters are not the argument array its launch site packs");
  return reinterpret_cast<const void*>(kernel);
}
template <typename... Want, typename... A>
inline void set_form_of(kernel_fn (&f)[2], void (*fwd)(A...), void (*bwd)(A...)) {
  f[0] = kernel_fn{checked_sym<Want...>(fwd), nullptr, false};
  f[1] = kernel_fn{checked_sym<Want...>(bwd), nullptr, false};
}

/// The argument list plan_t::run_stage packs for each form of a packed entry whose kernels compute in T (TWO_TIER:
/// spec_kernel::two_tier).  run_stage hands the kernel an array of addresses that nothing converts, so set_spec_form
/// compares every registered kernel's parameters with this list: a pointer as a pointer, a scalar by its exact type.
struct any_pointer;
template <typename... A>
struct arg_list;
template <typename T, int FORM, bool TWO_TIER = false>
struct spec_form_args;
template <typename T>
struct spec_form_args<T, WF_INTERLEAVED, false> {  // in, out, tw, nfft, scale
  using type = arg_list<any_pointer, any_pointer, any_pointer, long long, T>;
};
template <typename T>
struct spec_form_args<T, WF_INTERLEAVED, true> {  // ..., n_main, main_k
  using type = arg_list<any_pointer, any_pointer, any_pointer, long long, T, long long, int>;
};
template <typename T>
struct spec_form_args<T, WF_SPLIT, false> {  // in_re, in_im, out_re, out_im, tw, nfft, scale
  using type = arg_list<any_pointer, any_pointer, any_pointer, any_pointer, any_pointer, long long, T>;
};
template <typename T>
struct spec_form_args<T, WF_REAL, false> {  // in, out, tw, nfft, scale, fdist, bdist
  using type = arg_list<any_pointer, any_pointer, any_pointer, long long, T, unsigned, unsigned>;
};
template <typename T>
struct spec_form_args<T, WF_BLUESTEIN, false> {  // in, out, tw, nfft, n, scale, idist, odist
  using type = arg_list<any_pointer, any_pointer, any_pointer, long long, unsigned, T, unsigned, unsigned>;
};
template <typename T>
struct spec_form_args<T, WF_CONV, false> {  // in, out, tw, filt, nfft, n_filters, scale, idist, odist
  using type = arg_list<any_pointer, any_pointer, any_pointer, any_pointer, long long, unsigned, T, unsigned, unsigned>;
};
template <typename T>
struct spec_form_args<T, WF_OLS, false> {  // in, out, tw, filt, n_signals, n_seg, n_filters, scale, lead, hop,
                                           // in_length, out_length, in_pitch, out_pitch
  using type = arg_list<any_pointer, any_pointer, any_pointer, any_pointer, unsigned, unsigned, unsigned, T, unsigned,
                        unsigned, unsigned, unsigned, unsigned, unsigned>;
};
template <typename T>
struct spec_form_args<T, WF_RCONV, false> {  // in, out, tw, filt, nfft, n_filters, scale, dist
  using type = arg_list<any_pointer, any_pointer, any_pointer, any_pointer, long long, unsigned, T, unsigned>;
};
template <typename T>
struct spec_form_args<T, WF_ROLS, false> : spec_form_args<T, WF_OLS, false> {};  // the same list, counted in scalars
template <typename T>
struct spec_form_args<T, WF_STFT, false> {  // in, out, tw, win, n_signals, n_frames, scale, lead, hop, in_length,
                                            // in_pitch, frame_pitch, out_pitch
  using type = arg_list<any_pointer, any_pointer, any_pointer, any_pointer, unsigned, unsigned, T, unsigned, unsigned,
                        unsigned, unsigned, unsigned, unsigned>;
};
template <typename T>
struct spec_form_args<T, WF_ISTFT, false> {  // in, out, tw, win, n_signals, n_frames, scale, lead, hop, out_length,
                                             // frame_pitch, in_pitch, out_pitch, chunk_frames
  using type = arg_list<any_pointer, any_pointer, any_pointer, any_pointer, unsigned, unsigned, T, unsigned, unsigned,
                        unsigned, unsigned, unsigned, unsigned, unsigned>;
};
template <typename T>
struct spec_form_args<T, WF_DCT, false> {  // in, out, tw, ctab, n_rows, scale, in_pitch, out_pitch
  using type = arg_list<any_pointer, any_pointer, any_pointer, any_pointer, long long, T, unsigned, unsigned>;
};
template <typename T>
struct spec_form_args<T, WF_DCT4, false> {  // in, out, tw, tab, win, n_signals, n_frames, scale, lead, in_length, in_pitch,
                                            // frame_pitch, out_pitch ([0] rows: n_signals = n_rows, n_frames = 1)
  using type = arg_list<any_pointer, any_pointer, any_pointer, any_pointer, any_pointer, unsigned, unsigned, T, unsigned,
                        unsigned, unsigned, unsigned, unsigned>;
};
template <typename T>
struct spec_form_args<T, WF_IMDCT, false> {  // in, out, tw, tab, win, n_signals, n_frames, scale, lead, out_length,
                                             // frame_pitch, in_pitch, out_pitch, chunk_frames
  using type = arg_list<any_pointer, any_pointer, any_pointer, any_pointer, any_pointer, unsigned, unsigned, T, unsigned,
                        unsigned, unsigned, unsigned, unsigned, unsigned>;
};
template <typename T>
struct spec_form_args<T, WF_PERIODOGRAM, false> {  // in, out, tw, win, n_signals, n_frames, scale, lead, hop, in_length,
                                                   // in_pitch, row_pitch, out_pitch, avg_frames
  using type = arg_list<any_pointer, any_pointer, any_pointer, any_pointer, unsigned, unsigned, T, unsigned, unsigned,
                        unsigned, unsigned, unsigned, unsigned, unsigned>;
};
template <typename T>
struct spec_form_args<T, WF_PAIRS, false> {  // x, y, out, tw, n_rows, scale, floor, x_length, x_pitch, y_length, y_pitch,
                                             // out_length, out_pitch
  using type = arg_list<any_pointer, any_pointer, any_pointer, any_pointer, unsigned, T, T, unsigned, unsigned, unsigned,
                        unsigned, unsigned, unsigned>;
};
template <typename A>
using arg_kind = std::conditional_t<std::is_pointer<A>::value, any_pointer, std::remove_cv_t<A>>;

/// form FORM of the pre-compiled packed entry `k` (computing in T): the forward / backward host symbols
template <int FORM, typename T, bool TWO_TIER = false, typename... A>
inline void set_spec_form(spec_kernel& k, void (*fwd)(A...), void (*bwd)(A...)) {
  static_assert(std::is_same<arg_list<arg_kind<A>...>, typename spec_form_args<T, FORM, TWO_TIER>::type>::value,
                "the kernel's parameters are not the argument list run_stage packs for this form");
  set_form(k.cells(FORM), fwd, bwd, false);
  if constexpr (TWO_TIER) k.two_tier = 1;
}

/// the fields every form of a packed configuration shares (no kernel is instantiated by this)
template <typename Cfg>
spec_kernel spec_entry_fields(int groups_per_wg) {
  spec_kernel k{};
  k.groups_per_wg = groups_per_wg;
  k.precision = sizeof(typename Cfg::T) == 8 ? PFFT_PRECISION_F64 : PFFT_PRECISION_F32;
  k.n = Cfg::N;
  k.wg = Cfg::WG;
  k.fpw = Cfg::FPW;
  k.lds_bytes = Cfg::LDS_BYTES;
  k.n_radices = Cfg::NP;
  for (int i = 0; i < Cfg::NP; ++i) k.radices[i] = Cfg::Seq::r[i];
  k.tw_total = Cfg::Seq::tw_total;
  k.tw_in_regs = Cfg::TWM == TW_REGS ? 1 : 0;
  k.pads = Cfg::PADS;
  k.padw = Cfg::PADW;
  k.twm = Cfg::TWM;
  k.occ = Cfg::OCC;
  k.aux = Cfg::AUX;
  k.staged = Cfg::STAGED;
  k.twl = Cfg::TWL;
  return k;
}

template <typename Cfg>
spec_kernel make_spec_entry(int groups_per_wg = 1) {
  using T = typename Cfg::T;
  spec_kernel k = spec_entry_fields<Cfg>(groups_per_wg);
  set_spec_form<WF_INTERLEAVED, T>(k, &stockham_wg_kernel<Cfg, false>, &stockham_wg_kernel<Cfg, true>);
  set_spec_form<WF_SPLIT, T>(k, &stockham_wg_split_kernel<Cfg, false>, &stockham_wg_split_kernel<Cfg, true>);
  return k;
}

/// software-pipelined form (stockham_wg_prefetch_kernel) of a direct-I/O multi-pass variant
template <typename Cfg>
spec_kernel make_spec_entry_prefetch(int groups_per_wg = 4) {
  spec_kernel k = make_spec_entry<Cfg>(groups_per_wg);
  set_spec_form<WF_INTERLEAVED, typename Cfg::T, true>(k, &stockham_wg_prefetch_kernel<Cfg, false>,
                                                       &stockham_wg_prefetch_kernel<Cfg, true>);
  return k;
}

/// cross-lane form (stockham_xlane.hpp) of an N = R * R staged variant; interleaved storage (split storage keeps
/// the LDS form of the same configuration)
template <typename Cfg>
spec_kernel make_spec_entry_xlane(int groups_per_wg = 1) {
  spec_kernel k = make_spec_entry<Cfg>(groups_per_wg);
  set_spec_form<WF_INTERLEAVED, typename Cfg::T>(k, &stockham_wg_xlane_kernel<Cfg, false>, &stockham_wg_xlane_kernel<Cfg, true>);
  k.xlane = 1;
  return k;
}

/// register-resident form (stockham_wg_hx.hpp) of a packed length; PF: its software-pipelined form
template <typename Cfg, bool PF = false>
spec_kernel make_spec_entry_hx(int groups_per_wg = 0) {
  // (fields only: the LDS-resident stockham_wg kernels of such a configuration -- fp32 32768 would need a 256 KiB image --
  //  are never instantiated, and every cell of the entry is the register-resident kernel's: ADVICE r5)
  using T = typename Cfg::T;
  spec_kernel k = spec_entry_fields<Cfg>(groups_per_wg);
  k.lds_bytes = wg_hx_lds_bytes<Cfg>();
  set_spec_form<WF_INTERLEAVED, T>(k, &stockham_wg_hx_kernel<Cfg, false, PF>, &stockham_wg_hx_kernel<Cfg, true, PF>);
  set_spec_form<WF_SPLIT, T>(k, &stockham_wg_hx_split_kernel<Cfg, false, PF>, &stockham_wg_hx_split_kernel<Cfg, true, PF>);
  k.hx = 1;
  return k;
}

/// fp16 storage (PFFT_PRECISION_F16) forms of an fp32 configuration: the same kernels behind converting I/O objects
/// (stockham_wg.hpp, packed_io / packed_split_io with S = half_t); the LDS, twiddles and grid rule are the fp32 entry's
template <typename Cfg>
spec_kernel make_spec_entry_half(int groups_per_wg = 1) {
  static_assert(sizeof(typename Cfg::T) == 4, "fp16 storage computes in fp32");
  spec_kernel k = spec_entry_fields<Cfg>(groups_per_wg);
  k.precision = PFFT_PRECISION_F16;
  set_spec_form<WF_INTERLEAVED, float>(k, &stockham_wg_half_kernel<Cfg, false>, &stockham_wg_half_kernel<Cfg, true>);
  set_spec_form<WF_SPLIT, float>(k, &stockham_wg_half_split_kernel<Cfg, false>, &stockham_wg_half_split_kernel<Cfg, true>);
  return k;
}

template <typename Cfg>
spec_kernel make_spec_entry_prefetch_half(int groups_per_wg = 4) {
  spec_kernel k = make_spec_entry_half<Cfg>(groups_per_wg);
  set_spec_form<WF_INTERLEAVED, float, true>(k, &stockham_wg_prefetch_half_kernel<Cfg, false>,
                                             &stockham_wg_prefetch_half_kernel<Cfg, true>);
  return k;
}

template <typename Cfg, bool PF = false>
spec_kernel make_spec_entry_hx_half(int groups_per_wg = 0) {
  static_assert(sizeof(typename Cfg::T) == 4, "fp16 storage computes in fp32");
  spec_kernel k = spec_entry_fields<Cfg>(groups_per_wg);
  k.precision = PFFT_PRECISION_F16;
  k.lds_bytes = wg_hx_lds_bytes<Cfg>();
  set_spec_form<WF_INTERLEAVED, float>(k, &stockham_wg_hx_half_kernel<Cfg, false, PF>, &stockham_wg_hx_half_kernel<Cfg, true, PF>);
  set_spec_form<WF_SPLIT, float>(k, &stockham_wg_hx_half_split_kernel<Cfg, false, PF>,
                                 &stockham_wg_hx_half_split_kernel<Cfg, true, PF>);
  k.hx = 1;
  return k;
}

/// The entry of a fused form (WF_REAL, WF_CONV, WF_OLS, WF_RCONV, WF_ROLS, WF_STFT, WF_ISTFT, WF_DCT, WF_DCT4, WF_IMDCT, WF_PERIODOGRAM, WF_PAIRS, WF_BLUESTEIN) of the
/// LDS-resident configuration Cfg: the configuration's fields, the form's LDS (its <verb>_lds_bytes<Cfg>()) and its two
/// kernels in the only cell the entry carries.
template <int FORM, typename Cfg, typename... A>
spec_kernel make_fused_entry(int groups_per_wg, size_t lds_bytes, void (*k0)(A...), void (*k1)(A...)) {
  static_assert(Cfg::LDS_PER_FFT > 0, "LDS-resident configurations only");
  spec_kernel k = spec_entry_fields<Cfg>(groups_per_wg);
  k.lds_bytes = lds_bytes;
  set_spec_form<FORM, typename Cfg::T>(k, k0, k1);
  return k;
}

template <typename Cfg>
rows2d_kernel make_rows2d_entry(int groups_per_wg);

/// the entry for Cfg (cache policy nt) and its writer twin (default-policy stores)
template <typename Cfg>
void add_rows2d_entries(std::vector<rows2d_kernel>& v, int groups_per_wg) {
  rows2d_kernel k = make_rows2d_entry<Cfg>(groups_per_wg);
  set_form(k.form[R2_SPLIT], &stockham_rows2d_kernel<Cfg, false, true>, &stockham_rows2d_kernel<Cfg, true, true>, false);
  v.push_back(k);
  rows2d_kernel w = make_rows2d_entry<with_aux_t<Cfg, PFA_AUX_WRITER>>(groups_per_wg);
  w.policy = 1;
  // (round 6: the split-storage form of the writer twin too -- the two-pass 2-D plan of SPLIT_COMPLEX data in cache-sized chunks)
  using WCfg = with_aux_t<Cfg, PFA_AUX_WRITER>;
  set_form(w.form[R2_SPLIT], &stockham_rows2d_kernel<WCfg, false, true>, &stockham_rows2d_kernel<WCfg, true, true>, false);
  v.push_back(w);
}

/// Cfg: the row FFT's wg_cfg with FPW = rows per work-group (= the column radix)
template <typename Cfg>
rows2d_kernel make_rows2d_entry(int groups_per_wg) {
  rows2d_kernel k{};
  k.precision = sizeof(typename Cfg::T) == 8 ? PFFT_PRECISION_F64 : PFFT_PRECISION_F32;
  k.n = Cfg::N;
  k.rc = Cfg::FPW;
  k.wg = Cfg::WG;
  k.lds_bytes = Cfg::LDS_BYTES;
  k.n_radices = Cfg::NP;
  for (int i = 0; i < Cfg::NP; ++i) k.radices[i] = Cfg::Seq::r[i];
  k.groups_per_wg = groups_per_wg;
  set_form(k.form[R2_INTERLEAVED], &stockham_rows2d_kernel<Cfg, false>, &stockham_rows2d_kernel<Cfg, true>, true);
  return k;
}

/// mark an entry as the wide-group alternative of its length (strided_kernel::wide)
inline strided_kernel wide(strided_kernel k) {
  k.wide = 1;
  return k;
}

/// mark an entry as the alternative of its length for stages with a row-shaped side (strided_kernel::rowish)
inline strided_kernel rowish(strided_kernel k) {
  k.rowish = 1;
  return k;
}

/// add the row-staged forms to an entry (fp32: a wave covers only 64/FPW * 8 B of a row when addressed f-fastest)
template <typename Cfg>
strided_kernel with_rows(strided_kernel k) {
  set_form(k.form[SF_ROW_IN], &stockham_strided_row_kernel<Cfg, false, true, false>,
           &stockham_strided_row_kernel<Cfg, true, true, false>, false);
  set_form(k.form[SF_ROW_OUT], &stockham_strided_row_kernel<Cfg, false, false, true>,
           &stockham_strided_row_kernel<Cfg, true, false, true>, false);
  k.lds_bytes_row = strided_row_lds_bytes<Cfg>();
  return k;
}

/// add the tiled-input form (four-step stage B reading a group-major intermediate) to an entry
/// (PF: the software-pipelined kernel's tiled-input form; LTW: ... carrying the inter-stage twiddles on its loads, tables
/// in LDS behind the kernel's own: strided_kernel::fs_ltw)
template <typename Cfg, bool PF = false, int LTW = 0>
strided_kernel with_tin(strided_kernel k) {
  static_assert(tin_supported<Cfg>(), "see tin_supported()");
  if constexpr (PF) {
    set_form(k.form[SF_TIN], &stockham_strided_prefetch_kernel<Cfg, false, 0, 0, true, LTW>,
             &stockham_strided_prefetch_kernel<Cfg, true, 0, 0, true, LTW>, true);
  } else {
    static_assert(LTW == 0, "the load-side modifier exists in the software-pipelined kernel only");
    set_form(k.form[SF_TIN], &stockham_strided_kernel<Cfg, false, 0, 0, true>, &stockham_strided_kernel<Cfg, true, 0, 0, true>,
             true);
  }
  return k;
}

/// tiled-input form for tiles twice as wide as the entry's groups (SF_TIN_W)
template <typename Cfg>
strided_kernel with_tin_w(strided_kernel k) {
  static_assert(tin_supported<Cfg, 2 * Cfg::FPW>(), "see tin_supported()");
  set_form(k.form[SF_TIN_W], &stockham_strided_kernel<Cfg, false, 0, 0, 2 * Cfg::FPW>,
           &stockham_strided_kernel<Cfg, true, 0, 0, 2 * Cfg::FPW>, true);
  k.tin_w = 2 * Cfg::FPW;
  return k;
}

/// the plain and store-modifier forms of a pre-compiled entry, in the order [backward * 2 + store_modifier]
template <typename... A>
inline void set_plain_stw(strided_kernel& k, void (*f0)(A...), void (*f1)(A...), void (*b0)(A...), void (*b1)(A...)) {
  set_form(k.form[SF_PLAIN], f0, b0, true);
  set_form(k.form[SF_STW], f1, b1, true);
}

template <typename Cfg>
strided_kernel make_strided_entry(int groups_per_wg = 1);

template <typename Cfg>
strided_kernel make_strided_entry_prefetch(int groups_per_wg = 4) {
  strided_kernel k = make_strided_entry<Cfg>(groups_per_wg);
  set_plain_stw(k, &stockham_strided_prefetch_kernel<Cfg, false, false>, &stockham_strided_prefetch_kernel<Cfg, false, true>,
                &stockham_strided_prefetch_kernel<Cfg, true, false>, &stockham_strided_prefetch_kernel<Cfg, true, true>);
  return k;
}

/// flags of add_strided_entries
/// SE_FS_A / SE_FS_B: the entry of its length for the four-step stage A / stage B (strided_kernel::fs_a / fs_b)
enum : unsigned { SE_ROWS = 1, SE_TIN = 2, SE_WIDE = 4, SE_ROWISH = 8, SE_PREFETCH = 16, SE_FS_A = 32, SE_FS_B = 64, SE_FS_ONLY = 128,
                SE_LTW = 256 /* fs_b entry carrying the modifier on its loads (strided_kernel::fs_ltw) */,
                SE_PLAIN_WRITER = 512 /* the writer twin also carries the forms without store modifier (stage A of an SE_LTW pair) */,
                SE_TIN_W = 1024 /* ... and the tiled-input form for tiles of 2 * FPW elements (SF_TIN_W) */ };

template <typename Cfg, unsigned F>
strided_kernel make_strided_entry_flags(int groups_per_wg) {
  strided_kernel k = (F & SE_PREFETCH) ? make_strided_entry_prefetch<Cfg>(groups_per_wg) : make_strided_entry<Cfg>(groups_per_wg);
  if constexpr ((F & SE_ROWS) != 0) k = with_rows<Cfg>(k);
  if constexpr ((F & SE_TIN) != 0) k = with_tin<Cfg, (F & SE_PREFETCH) != 0, (F & SE_LTW) != 0 ? 1 : 0>(k);
  if constexpr ((F & SE_TIN_W) != 0) k = with_tin_w<Cfg>(k);
  k.fs_ltw = (F & SE_LTW) != 0;
  k.wide = (F & SE_WIDE) != 0;
  k.rowish = (F & SE_ROWISH) != 0;
  k.fs_a = (F & SE_FS_A) != 0;
  k.fs_b = (F & SE_FS_B) != 0;
  k.fs_only = (F & SE_FS_ONLY) != 0;
  static_assert((F & SE_FS_B) == 0 || (F & SE_TIN) != 0, "a four-step stage-B entry needs its tiled-input form");
  return k;
}

/// policy twin of `base` (the nt entry of the same shape): Cfg carries the twin's AUX; only the forms a writer
/// (policy 1: with the store modifier, four-step stage A) or a reader (policy 2: without it, stage B and the second pass
/// of the two-pass 2-D plan) is ever launched in are instantiated, the others stay empty
template <typename Cfg, unsigned F>
strided_kernel make_strided_twin(const strided_kernel& base, int policy) {
  constexpr bool PF = (F & SE_PREFETCH) != 0;
  strided_kernel k = base;
  k.policy = policy;
  for (auto& f : k.form) f[0] = f[1] = kernel_fn{};
  k.tin_w = 0;
  if (policy == 1) {
    if constexpr (PF) {
      set_form(k.form[SF_STW], &stockham_strided_prefetch_kernel<Cfg, false, true>, &stockham_strided_prefetch_kernel<Cfg, true, true>,
               true);
    } else {
      set_form(k.form[SF_STW], &stockham_strided_kernel<Cfg, false, true>, &stockham_strided_kernel<Cfg, true, true>, true);
    }
    if constexpr ((F & SE_PLAIN_WRITER) != 0) {  // stage A of a pair whose stage B carries the modifier: no store modifier
      static_assert(!PF, "plain writer forms: the non-pipelined kernel");
      set_form(k.form[SF_PLAIN], &stockham_strided_kernel<Cfg, false, false>, &stockham_strided_kernel<Cfg, true, false>, true);
    }
  } else {
    if constexpr (PF) {
      set_form(k.form[SF_PLAIN], &stockham_strided_prefetch_kernel<Cfg, false, false>,
               &stockham_strided_prefetch_kernel<Cfg, true, false>, true);
    } else {
      set_form(k.form[SF_PLAIN], &stockham_strided_kernel<Cfg, false, false>, &stockham_strided_kernel<Cfg, true, false>, true);
    }
    if constexpr ((F & SE_ROWS) != 0) {
      set_form(k.form[SF_ROW_IN], &stockham_strided_row_kernel<Cfg, false, true, false>,
               &stockham_strided_row_kernel<Cfg, true, true, false>, false);
    }
    if constexpr ((F & SE_TIN) != 0) k = with_tin<Cfg, PF, (F & SE_LTW) != 0 ? 1 : 0>(k);
    if constexpr ((F & SE_TIN_W) != 0) k = with_tin_w<Cfg>(k);
    // (round 6: the reader twin of a wide entry -- the second pass of the two-pass 2-D plan -- carries its split-storage form)
    if constexpr ((F & SE_WIDE) != 0 && !PF) {
      set_form(k.form[SF_SPLIT], &stockham_strided_kernel<Cfg, false, false, true>, &stockham_strided_kernel<Cfg, true, false, true>,
               false);
    }
  }
  return k;
}

/// the entry for Cfg (cache policy nt) and its writer / reader twins
template <typename Cfg, unsigned F = 0>
void add_strided_entries(std::vector<strided_kernel>& v, int groups_per_wg = 1, int fs_groups_per_wg = 0) {
  strided_kernel base = make_strided_entry_flags<Cfg, F>(groups_per_wg);
  base.fs_groups_per_wg = fs_groups_per_wg;
  v.push_back(base);
  v.push_back(make_strided_twin<with_aux_t<Cfg, PFA_AUX_WRITER>, F>(base, 1));
  v.push_back(make_strided_twin<with_aux_t<Cfg, PFA_AUX_READER>, F>(base, 2));
}

template <typename Cfg>
strided_kernel make_strided_entry(int groups_per_wg) {
  strided_kernel k{};
  k.groups_per_wg = groups_per_wg;
  k.precision = sizeof(typename Cfg::T) == 8 ? PFFT_PRECISION_F64 : PFFT_PRECISION_F32;
  k.n = Cfg::N;
  k.wg = Cfg::WG;
  k.fpw = Cfg::FPW;
  k.lds_bytes = strided_lds_bytes<Cfg>();
  k.stw_mode = 1;
  k.n_radices = Cfg::NP;
  for (int i = 0; i < Cfg::NP; ++i) k.radices[i] = Cfg::Seq::r[i];
  set_plain_stw(k, &stockham_strided_kernel<Cfg, false, false>, &stockham_strided_kernel<Cfg, false, true>,
                &stockham_strided_kernel<Cfg, true, false>, &stockham_strided_kernel<Cfg, true, true>);
  set_form(k.form[SF_SPLIT], &stockham_strided_kernel<Cfg, false, false, true>, &stockham_strided_kernel<Cfg, true, false, true>,
           false);
  return k;
}

}  // namespace pfa
