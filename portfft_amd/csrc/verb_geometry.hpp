// Call geometry of the fused verbs whose shape comes with the call (plan_t::filter_signals, stft, istft, dct, dct4, mdct, imdct, periodogram, pairs): every
// check between the plan-state checks and the launch, and the kernel arguments that follow from the call.  The
// refusals here are what keeps a kernel's 32-bit byte offsets from wrapping.  No HIP: a plan hands in the few facts
// the checks read (verb_facts) and the pointers as integers, so the rules run -- and are tested -- without a device
// (tests/cpp/verb_geometry_test.cpp).  The order of the checks is part of the behaviour: a call that breaks several
// rules gets the first one's message.
#pragma once
#include <algorithm>
#include <cstdint>

#include "common.hpp"

namespace pfa {

/// What the checks read of a plan and of the verb's kernel.
struct verb_facts {
  unsigned long long n = 0;       // the descriptor's length: points of a complex plan, scalars of a real one
  unsigned long long sb = 4;      // bytes of a stored scalar; a complex element is two
  bool real = false;              // a plan of the REAL domain (filter: samples are scalars)
  unsigned long long taps = 0;    // filter: taps of the filter set
  unsigned long long fpw = 1;     // rows of one work-group of the verb's kernel
  unsigned long long resident[2] = {0, 0};  // istft, imdct: work-groups the device holds at once, by mode (stage::grid)
};

/// do [a, a + a_bytes) and [b, b + b_bytes) share a byte?
inline bool byte_ranges_overlap(uintptr_t a, unsigned long long a_bytes, uintptr_t b, unsigned long long b_bytes) {
  return a < b + b_bytes && b < a + a_bytes;
}

inline unsigned u32(unsigned long long v) { return static_cast<unsigned>(v); }

// The kernel arguments below stand in the order of their form's spec_form_args (kernels_impl.hpp); `groups` is what
// grid_of gets.

struct filter_geometry {
  unsigned n_signals, n_seg, lead, hop, in_length, out_length, in_pitch, out_pitch;
  long long groups;
};

/// Overlap-save filtering (stockham_wg_ols.hpp, stockham_wg_rols.hpp); `mode` has been checked.
/// A complex plan: lead = taps - 1 (convolve) or 0, hop = n - taps + 1.  A real plan works on scalar pairs and takes
/// both even: lead rounded up, the correlation's hop rounded down -- at most one sample of hop.
inline filter_geometry filter_geometry_of(const verb_facts& p, int mode, uintptr_t in, uintptr_t out,
                                          unsigned long long n_signals, unsigned long long in_length,
                                          unsigned long long in_pitch, unsigned long long out_length,
                                          unsigned long long out_pitch) {
  if (n_signals == 0 || in_length == 0 || out_length == 0) {
    fail(PFFT_INVALID_CONFIGURATION, "filter: zero count (", n_signals, " signals, in_length ", in_length, ", out_length ",
         out_length, ")");
  }
  const bool real = p.real;
  const unsigned long long n = p.n, taps = p.taps;
  if (real && taps > n - 2) {
    fail(PFFT_INVALID_CONFIGURATION, "filter: ", taps, " taps on a real plan of length ", n, "; the kernel works on scalar "
         "pairs and needs a hop of at least 2 samples, that is at most ", n - 2, " taps");
  }
  const unsigned long long lead_conv = real ? (taps & ~1ull) : taps - 1;  // (taps - 1 rounded up to even)
  const unsigned long long lead_of_mode = mode == PFFT_CONVOLVE ? lead_conv : 0;
  const unsigned long long hop = real ? (mode == PFFT_CONVOLVE ? n - lead_conv : ((n - taps + 1) & ~1ull)) : n - taps + 1;
  const unsigned long long bound = mode == PFFT_CONVOLVE ? in_length + taps - 1 : in_length;
  if (out_length > bound) {
    fail(PFFT_INVALID_CONFIGURATION, "filter: out_length ", out_length, " beyond ", bound,
         mode == PFFT_CONVOLVE ? " (in_length + taps - 1, the full linear convolution)"
                               : " (in_length: the non-negative lags of the correlation)");
  }
  if (in_pitch < in_length || out_pitch < out_length) {
    fail(PFFT_INVALID_CONFIGURATION, "filter: pitches (", in_pitch, ", ", out_pitch, ") below the lengths (", in_length, ", ",
         out_length, ")");
  }
  const unsigned long long eb = real ? p.sb : 2 * p.sb;  // of a sample
  // (what would wrap the 64-bit byte arithmetic below; no buffer is that large)
  if (n_signals >= (1ull << 32) || in_pitch >= (1ull << 32) || out_pitch >= (1ull << 32) ||
      n_signals * std::max(in_pitch, out_pitch) >= (1ull << 56)) {
    fail(PFFT_UNSUPPORTED_CONFIGURATION, "filter: the kernel addresses with 32-bit byte offsets: at most 2^32 - 1 signals "
         "and pitches below 4 GiB");
  }
  // segment s + 1 reads the taps - 1 samples the group of segment s overwrites: in place is a race
  if (byte_ranges_overlap(in, ((n_signals - 1) * in_pitch + in_length) * eb, out,
                          ((n_signals - 1) * out_pitch + out_length) * eb)) {
    fail(PFFT_INVALID_CONFIGURATION, "filter: the input and the output byte ranges overlap; overlap-save filtering "
         "cannot run in place (a segment reads samples its predecessor's outputs would overwrite)");
  }
  // the resource of a group starts at the signal of its first row and spans at most min(fpw, n_signals) signals
  const unsigned long long n_seg = (out_length + hop - 1) / hop;
  const unsigned long long span = std::min(p.fpw, n_signals);
  // (and start `lead` samples in front of it: stockham_wg_ols.hpp, ols_row; the last pair of a real window may sit one
  // scalar further on in the address arithmetic, never dereferenced)
  const unsigned long long reach =
      ((span - 1) * std::max(in_pitch, out_pitch) + std::max(in_length, out_length) + lead_conv + (real ? 1 : 0)) * eb;
  if (reach > 0xFFFFFFFFull) {
    fail(PFFT_UNSUPPORTED_CONFIGURATION, "filter: ", span, " consecutive signals (the rows of one work-group) span ", reach,
         " bytes; the kernel's 32-bit byte offsets end at 4 GiB (a single signal of 4 GiB or more, or as many shorter ones "
         "as a work-group holds rows)");
  }
  if (n_signals * n_seg >= (1ull << 31)) {
    fail(PFFT_UNSUPPORTED_CONFIGURATION, "filter: ", n_signals, " signals of ", n_seg, " segments each: the kernel counts "
         "its rows in 32 bits, at most 2^31 - 1 (signal, segment) pairs per call");
  }
  return {u32(n_signals), u32(n_seg),    u32(lead_of_mode), u32(hop), u32(in_length), u32(out_length),
          u32(in_pitch),  u32(out_pitch), static_cast<long long>((n_signals * n_seg + p.fpw - 1) / p.fpw)};
}

struct stft_geometry {
  unsigned n_signals, n_frames, lead, hop, in_length, in_pitch, frame_pitch, out_pitch;
  long long groups;
};

/// Short-time Fourier transform (stockham_wg_stft.hpp).
inline stft_geometry stft_geometry_of(const verb_facts& p, uintptr_t in, uintptr_t out, unsigned long long n_signals,
                                      unsigned long long in_length, unsigned long long in_pitch, unsigned long long hop,
                                      unsigned long long lead, int pad_mode, unsigned long long n_frames,
                                      unsigned long long frame_pitch, unsigned long long out_pitch) {
  if (in == 0 || out == 0) fail(PFFT_INVALID_CONFIGURATION, "stft: null data pointer");
  if (n_signals == 0 || in_length == 0 || n_frames == 0) {
    fail(PFFT_INVALID_CONFIGURATION, "stft: zero count (", n_signals, " signals, in_length ", in_length, ", ", n_frames,
         " frames)");
  }
  const unsigned long long n = p.n, m = n / 2;
  if (hop == 0) fail(PFFT_INVALID_CONFIGURATION, "stft: hop 0");
  if (lead >= n) fail(PFFT_INVALID_CONFIGURATION, "stft: lead ", lead, " must be below the frame length ", n);
  if (pad_mode != PFFT_PAD_ZERO && pad_mode != PFFT_PAD_REFLECT) fail(PFFT_INVALID_CONFIGURATION, "Invalid stft pad_mode ", pad_mode);
  if (in_pitch < in_length) fail(PFFT_INVALID_CONFIGURATION, "stft: in_pitch ", in_pitch, " below in_length ", in_length);
  if (frame_pitch < m + 1) {
    fail(PFFT_INVALID_CONFIGURATION, "stft: frame_pitch ", frame_pitch, " below the ", m + 1, " bins of a frame");
  }
  // (what would wrap the 64-bit arithmetic below; no buffer is that large)
  if (n_signals >= (1ull << 32) || n_frames >= (1ull << 32) || hop >= (1ull << 32) || in_length >= (1ull << 32) ||
      in_pitch >= (1ull << 32) || frame_pitch >= (1ull << 32) || out_pitch >= (1ull << 32)) {
    fail(PFFT_UNSUPPORTED_CONFIGURATION, "stft: the kernel addresses with 32-bit byte offsets: counts, lengths, hop and "
         "pitches below 2^32");
  }
  if (out_pitch < n_frames * frame_pitch) {
    fail(PFFT_INVALID_CONFIGURATION, "stft: out_pitch ", out_pitch, " below n_frames * frame_pitch = ", n_frames * frame_pitch);
  }
  const unsigned long long last_e0 = (n_frames - 1) * hop;  // first sample of the last frame, in front of `lead`
  if (pad_mode == PFFT_PAD_ZERO) {
    if (last_e0 >= in_length + lead) {
      fail(PFFT_INVALID_CONFIGURATION, "stft: frame ", n_frames - 1, " starts at sample ", last_e0, " - lead ", lead,
           ", beyond the in_length ", in_length, " samples: every frame must hold at least one sample (n_frames, hop)");
    }
  } else {
    if (lead > in_length - 1) {
      fail(PFFT_INVALID_CONFIGURATION, "stft: lead ", lead, " above in_length - 1 = ", in_length - 1,
           ": reflection mirrors an index at most once");
    }
    if (last_e0 + n > in_length + 2 * lead) {
      fail(PFFT_INVALID_CONFIGURATION, "stft: frame ", n_frames - 1, " ends at sample ", last_e0 + n, " - lead ", lead,
           ", beyond the signal of in_length ", in_length, " reflected by lead on both sides (n_frames, hop)");
    }
  }
  const unsigned long long sb = p.sb, eb = 2 * p.sb;
  // frames overlap: in place would overwrite samples a later frame reads
  if (byte_ranges_overlap(in, ((n_signals - 1) * in_pitch + in_length) * sb, out,
                          ((n_signals - 1) * out_pitch + (n_frames - 1) * frame_pitch + m + 1) * eb)) {
    fail(PFFT_INVALID_CONFIGURATION, "stft: the input and the output byte ranges overlap; the transform cannot run in "
         "place (overlapping frames read samples an earlier frame's bins would overwrite)");
  }
  if (n_signals * n_frames >= (1ull << 31)) {
    fail(PFFT_UNSUPPORTED_CONFIGURATION, "stft: ", n_signals, " signals of ", n_frames, " frames each: the kernel counts "
         "its rows in 32 bits, at most 2^31 - 1 (signal, frame) pairs per call");
  }
  // The rows of a group are fpw consecutive (signal, frame) pairs: they cross at most `cross` signal boundaries.  The
  // input resource starts at the first of those signals (`lead` scalars in front of it), the output resource at the
  // group's first row (stockham_wg_stft.hpp, stft_io).
  const unsigned long long fpw = p.fpw;
  const unsigned long long cross = std::min(n_signals - 1, (fpw - 1 + n_frames - 1) / n_frames);
  const unsigned long long reach_in = (cross * in_pitch + in_length + lead + n + 1) * sb;
  const unsigned long long reach_out = (cross * out_pitch + std::min(fpw - 1, n_frames - 1) * frame_pitch + m + 1) * eb;
  if (reach_in > 0xFFFFFFFFull || reach_out > 0xFFFFFFFFull) {
    fail(PFFT_UNSUPPORTED_CONFIGURATION, "stft: the ", cross + 1, " consecutive signals the rows of one work-group touch span ",
         reach_in, " bytes, their output rows ", reach_out, "; the kernel's 32-bit byte offsets end at 4 GiB (a single signal "
         "of 4 GiB or more, or as many shorter ones as a work-group holds rows)");
  }
  return {u32(n_signals),   u32(n_frames),  u32(lead), u32(hop), u32(in_length), u32(in_pitch),
          u32(frame_pitch), u32(out_pitch), static_cast<long long>((n_signals * n_frames + fpw - 1) / fpw)};
}

/// Default chunk length of plan_t::istft: as large as still gives every resident work-group slot two groups, at least
/// four halos (at most a quarter of the frames transformed twice), whole steps of fpw frames, at most the signal.
inline unsigned long long istft_default_chunk(unsigned long long n_signals, unsigned long long n_frames,
                                              unsigned long long halo, unsigned long long fpw, unsigned long long resident) {
  const unsigned long long want = std::max<unsigned long long>(1, (2 * resident + n_signals - 1) / n_signals);  // chunks per signal
  unsigned long long c = (n_frames + want - 1) / want;
  c = std::max(c, std::max(4 * halo, fpw));
  c = (c + fpw - 1) / fpw * fpw;
  return std::min(c, n_frames);
}

struct istft_geometry {
  unsigned n_signals, n_frames, lead, hop, out_length, frame_pitch, in_pitch, out_pitch, chunk;
  long long groups;
};

/// Inverse short-time Fourier transform, overlap-add (stockham_wg_istft.hpp); chunk_frames 0: istft_default_chunk.
inline istft_geometry istft_geometry_of(const verb_facts& p, uintptr_t in, uintptr_t out, unsigned long long n_signals,
                                        unsigned long long n_frames, unsigned long long frame_pitch,
                                        unsigned long long in_pitch, unsigned long long hop, unsigned long long lead,
                                        int mode, unsigned long long out_length, unsigned long long out_pitch,
                                        unsigned long long chunk_frames) {
  if (in == 0 || out == 0) fail(PFFT_INVALID_CONFIGURATION, "istft: null data pointer");
  if (n_signals == 0 || n_frames == 0 || out_length == 0) {
    fail(PFFT_INVALID_CONFIGURATION, "istft: zero count (", n_signals, " signals, ", n_frames, " frames, out_length ",
         out_length, ")");
  }
  const unsigned long long n = p.n, m = n / 2;
  if (hop == 0) fail(PFFT_INVALID_CONFIGURATION, "istft: hop 0");
  if (hop > n) {
    fail(PFFT_INVALID_CONFIGURATION, "istft: hop ", hop, " above the frame length ", n, " leaves gaps that no frame covers");
  }
  if (lead >= n) fail(PFFT_INVALID_CONFIGURATION, "istft: lead ", lead, " must be below the frame length ", n);
  if (mode != PFFT_ISTFT_PLAIN && mode != PFFT_ISTFT_NORMALIZE) fail(PFFT_INVALID_CONFIGURATION, "Invalid istft mode ", mode);
  if (frame_pitch < m + 1) {
    fail(PFFT_INVALID_CONFIGURATION, "istft: frame_pitch ", frame_pitch, " below the ", m + 1, " bins of a frame");
  }
  // (what would wrap the 64-bit arithmetic below; no buffer is that large)
  if (n_signals >= (1ull << 32) || n_frames >= (1ull << 32) || out_length >= (1ull << 32) || in_pitch >= (1ull << 32) ||
      frame_pitch >= (1ull << 32) || out_pitch >= (1ull << 32)) {
    fail(PFFT_UNSUPPORTED_CONFIGURATION, "istft: the kernel addresses with 32-bit byte offsets: counts, lengths and pitches "
         "below 2^32 (4 GiB of bytes)");
  }
  if (in_pitch < n_frames * frame_pitch) {
    fail(PFFT_INVALID_CONFIGURATION, "istft: in_pitch ", in_pitch, " below n_frames * frame_pitch = ", n_frames * frame_pitch);
  }
  if (out_pitch < out_length) fail(PFFT_INVALID_CONFIGURATION, "istft: out_pitch ", out_pitch, " below out_length ", out_length);
  const unsigned long long last_e0 = (n_frames - 1) * hop;  // first position of the last frame, in front of `lead`
  if (out_length + lead > last_e0 + n) {
    fail(PFFT_INVALID_CONFIGURATION, "istft: out_length ", out_length, " above (n_frames - 1) * hop + N - lead = ",
         last_e0 + n - lead, ": the samples behind it are covered by no frame");
  }
  if (last_e0 >= out_length + lead) {
    fail(PFFT_INVALID_CONFIGURATION, "istft: frame ", n_frames - 1, " starts at sample ", last_e0, " - lead ", lead,
         ", beyond the out_length ", out_length, " samples: every frame must contribute at least one sample (n_frames, hop)");
  }
  const unsigned long long sb = p.sb, eb = 2 * p.sb;
  // a chunk reads the frames of its halo after the chunk in front of it has stored: in place is a race
  if (byte_ranges_overlap(in, ((n_signals - 1) * in_pitch + (n_frames - 1) * frame_pitch + m + 1) * eb, out,
                          ((n_signals - 1) * out_pitch + out_length) * sb)) {
    fail(PFFT_INVALID_CONFIGURATION, "istft: the input and the output byte ranges overlap; the transform cannot run in "
         "place (a chunk reads bins another chunk's samples would overwrite)");
  }
  if (n_signals * n_frames >= (1ull << 31)) {
    fail(PFFT_UNSUPPORTED_CONFIGURATION, "istft: ", n_signals, " signals of ", n_frames, " frames each: the kernel counts "
         "its rows in 32 bits, at most 2^31 - 1 (signal, frame) pairs per call");
  }
  const unsigned long long fpw = p.fpw;
  const unsigned long long halo = (n + hop - 1) / hop - 1;
  const unsigned long long chunk = chunk_frames == 0 ? istft_default_chunk(n_signals, n_frames, halo, fpw, p.resident[mode])
                                                       : std::min(chunk_frames, n_frames);
  // One group runs at most halo + chunk frames and owns at most chunk * hop samples (the last chunk of a signal up to
  // N - hop more); its resources start at its first frame and at its first sample (stockham_wg_istft.hpp).
  const unsigned long long run = std::min(n_frames, halo + chunk);
  const unsigned long long reach_in = ((run - 1) * frame_pitch + m + 1) * eb;
  const unsigned long long reach_out = (std::min(out_length, chunk * hop + n) + (halo + fpw) * hop + n + lead) * sb;
  if (reach_in > 0xFFFFFFFFull || reach_out > 0xFFFFFFFFull) {
    fail(PFFT_UNSUPPORTED_CONFIGURATION, "istft: the ", run, " frames one work-group runs span ", reach_in, " bytes, the samples "
         "it covers ", reach_out, "; the kernel's 32-bit byte offsets end at 4 GiB (a smaller chunk_frames shortens both)");
  }
  return {u32(n_signals), u32(n_frames),  u32(lead),  u32(hop), u32(out_length), u32(frame_pitch),
          u32(in_pitch),  u32(out_pitch), u32(chunk), static_cast<long long>(n_signals * ((n_frames + chunk - 1) / chunk))};
}

struct dct_geometry {
  long long n_rows;
  unsigned in_pitch, out_pitch;
  long long groups;
};

/// Discrete cosine transforms of type 2 and 3 (stockham_wg_dct.hpp).
inline dct_geometry dct_geometry_of(const verb_facts& p, int type, uintptr_t in, uintptr_t out, unsigned long long n_rows,
                                    unsigned long long in_pitch, unsigned long long out_pitch) {
  if (in == 0 || out == 0) fail(PFFT_INVALID_CONFIGURATION, "dct: null data pointer");
  if (n_rows == 0) fail(PFFT_INVALID_CONFIGURATION, "dct: zero count (n_rows 0)");
  if (type != PFFT_DCT_II && type != PFFT_DCT_III) {
    fail(PFFT_INVALID_CONFIGURATION, "Invalid dct type ", type, " (PFFT_DCT_II = 2 or PFFT_DCT_III = 3)");
  }
  const unsigned long long n = p.n;
  if (in_pitch < n) fail(PFFT_INVALID_CONFIGURATION, "dct: in_pitch ", in_pitch, " below the row length ", n);
  if (out_pitch < n) fail(PFFT_INVALID_CONFIGURATION, "dct: out_pitch ", out_pitch, " below the row length ", n);
  if (n_rows >= (1ull << 31)) {
    fail(PFFT_UNSUPPORTED_CONFIGURATION, "dct: ", n_rows, " rows: at most 2^31 - 1 rows per call");
  }
  const unsigned long long sb = p.sb, fpw = p.fpw;
  // The lane offsets inside wg_live_rows' resources: row slot f of a group at f * pitch bytes, in 32 bits.  EVERY slot
  // f = 0 ... fpw - 1 computes its offset, also the slots of rows that do not exist (fewer rows than fpw, a ragged last
  // group) -- only the resource's range check drops them, and an offset that wrapped could fall back into range.  So the
  // whole group is bounded, whatever n_rows is.
  const unsigned long long reach_in = fpw * in_pitch * sb, reach_out = fpw * out_pitch * sb;
  if (in_pitch >= (1ull << 32) || out_pitch >= (1ull << 32) || reach_in > 0xFFFFFFFFull || reach_out > 0xFFFFFFFFull) {
    fail(PFFT_UNSUPPORTED_CONFIGURATION, "dct: the ", fpw, " row slots of one work-group span ", reach_in,
         " bytes of the input and ", reach_out, " of the output; the kernel's 32-bit byte offsets end at 4 GiB");
  }
  if (in == out) {
    if (in_pitch != out_pitch) {
      fail(PFFT_INVALID_CONFIGURATION, "dct: in place (in == out) needs equal pitches, not in_pitch ", in_pitch,
           " and out_pitch ", out_pitch);
    }
  } else if (byte_ranges_overlap(in, ((n_rows - 1) * in_pitch + n) * sb, out, ((n_rows - 1) * out_pitch + n) * sb)) {
    // groups store rows other groups have not loaded yet
    fail(PFFT_INVALID_CONFIGURATION, "dct: the input and the output byte ranges overlap without being identical; in place "
         "means in == out with equal pitches");
  }
  return {static_cast<long long>(n_rows), u32(in_pitch), u32(out_pitch), static_cast<long long>((n_rows + fpw - 1) / fpw)};
}

struct dct4_geometry {
  unsigned n_rows, in_pitch, out_pitch;
  long long groups;
};

/// Discrete cosine transform of type 4 (stockham_wg_dct4.hpp, MDCT = false): dct_geometry_of without a type.
inline dct4_geometry dct4_geometry_of(const verb_facts& p, uintptr_t in, uintptr_t out, unsigned long long n_rows,
                                      unsigned long long in_pitch, unsigned long long out_pitch) {
  if (in == 0 || out == 0) fail(PFFT_INVALID_CONFIGURATION, "dct4: null data pointer");
  if (n_rows == 0) fail(PFFT_INVALID_CONFIGURATION, "dct4: zero count (n_rows 0)");
  const unsigned long long n = p.n;
  if (in_pitch < n) fail(PFFT_INVALID_CONFIGURATION, "dct4: in_pitch ", in_pitch, " below the row length ", n);
  if (out_pitch < n) fail(PFFT_INVALID_CONFIGURATION, "dct4: out_pitch ", out_pitch, " below the row length ", n);
  if (n_rows >= (1ull << 31)) {
    fail(PFFT_UNSUPPORTED_CONFIGURATION, "dct4: ", n_rows, " rows: at most 2^31 - 1 rows per call");
  }
  const unsigned long long sb = p.sb, fpw = p.fpw;
  // (dct_geometry_of: every row slot of a group computes its 32-bit offset f * pitch, missing rows included, so the
  // whole group is bounded whatever n_rows is)
  const unsigned long long reach_in = fpw * in_pitch * sb, reach_out = fpw * out_pitch * sb;
  if (in_pitch >= (1ull << 32) || out_pitch >= (1ull << 32) || reach_in > 0xFFFFFFFFull || reach_out > 0xFFFFFFFFull) {
    fail(PFFT_UNSUPPORTED_CONFIGURATION, "dct4: the ", fpw, " row slots of one work-group span ", reach_in,
         " bytes of the input and ", reach_out, " of the output; the kernel's 32-bit byte offsets end at 4 GiB");
  }
  if (in == out) {
    if (in_pitch != out_pitch) {
      fail(PFFT_INVALID_CONFIGURATION, "dct4: in place (in == out) needs equal pitches, not in_pitch ", in_pitch,
           " and out_pitch ", out_pitch);
    }
  } else if (byte_ranges_overlap(in, ((n_rows - 1) * in_pitch + n) * sb, out, ((n_rows - 1) * out_pitch + n) * sb)) {
    // groups store rows other groups have not loaded yet
    fail(PFFT_INVALID_CONFIGURATION, "dct4: the input and the output byte ranges overlap without being identical; in place "
         "means in == out with equal pitches");
  }
  return {u32(n_rows), u32(in_pitch), u32(out_pitch), static_cast<long long>((n_rows + fpw - 1) / fpw)};
}

struct mdct_geometry {
  unsigned n_signals, n_frames, lead, in_length, in_pitch, frame_pitch, out_pitch;
  long long groups;
};

/// Modified discrete cosine transform (stockham_wg_dct4.hpp, MDCT = true): frames of 2n samples at hop n, n
/// coefficients each; stft_geometry_of's checks in its order, counted in scalars on both sides.
inline mdct_geometry mdct_geometry_of(const verb_facts& p, uintptr_t in, uintptr_t out, unsigned long long n_signals,
                                      unsigned long long in_length, unsigned long long in_pitch, unsigned long long lead,
                                      unsigned long long n_frames, unsigned long long frame_pitch,
                                      unsigned long long out_pitch) {
  if (in == 0 || out == 0) fail(PFFT_INVALID_CONFIGURATION, "mdct: null data pointer");
  if (n_signals == 0 || in_length == 0 || n_frames == 0) {
    fail(PFFT_INVALID_CONFIGURATION, "mdct: zero count (", n_signals, " signals, in_length ", in_length, ", ", n_frames,
         " frames)");
  }
  const unsigned long long n = p.n;
  if (lead >= 2 * n) fail(PFFT_INVALID_CONFIGURATION, "mdct: lead ", lead, " must be below the frame length ", 2 * n);
  if (in_pitch < in_length) fail(PFFT_INVALID_CONFIGURATION, "mdct: in_pitch ", in_pitch, " below in_length ", in_length);
  if (frame_pitch < n) {
    fail(PFFT_INVALID_CONFIGURATION, "mdct: frame_pitch ", frame_pitch, " below the ", n, " coefficients of a frame");
  }
  // (what would wrap the 64-bit arithmetic below; no buffer is that large)
  if (n_signals >= (1ull << 32) || n_frames >= (1ull << 32) || in_length >= (1ull << 32) || in_pitch >= (1ull << 32) ||
      frame_pitch >= (1ull << 32) || out_pitch >= (1ull << 32)) {
    fail(PFFT_UNSUPPORTED_CONFIGURATION, "mdct: the kernel addresses with 32-bit byte offsets: counts, lengths and "
         "pitches below 2^32");
  }
  if (out_pitch < n_frames * frame_pitch) {
    fail(PFFT_INVALID_CONFIGURATION, "mdct: out_pitch ", out_pitch, " below n_frames * frame_pitch = ", n_frames * frame_pitch);
  }
  const unsigned long long last_e0 = (n_frames - 1) * n;  // first sample of the last frame, in front of `lead`
  if (last_e0 >= in_length + lead) {
    fail(PFFT_INVALID_CONFIGURATION, "mdct: frame ", n_frames - 1, " starts at sample ", last_e0, " - lead ", lead,
         ", beyond the in_length ", in_length, " samples: every frame must hold at least one sample (n_frames; the hop is ",
         n, ")");
  }
  const unsigned long long sb = p.sb;
  // frames overlap: in place would overwrite samples the next frame reads
  if (byte_ranges_overlap(in, ((n_signals - 1) * in_pitch + in_length) * sb, out,
                          ((n_signals - 1) * out_pitch + (n_frames - 1) * frame_pitch + n) * sb)) {
    fail(PFFT_INVALID_CONFIGURATION, "mdct: the input and the output byte ranges overlap; the transform cannot run in "
         "place (overlapping frames read samples an earlier frame's coefficients would overwrite)");
  }
  if (n_signals * n_frames >= (1ull << 31)) {
    fail(PFFT_UNSUPPORTED_CONFIGURATION, "mdct: ", n_signals, " signals of ", n_frames, " frames each: the kernel counts "
         "its rows in 32 bits, at most 2^31 - 1 (signal, frame) pairs per call");
  }
  // (stft_geometry_of: the fpw consecutive (signal, frame) rows of a group cross at most `cross` signal boundaries; the
  // input resource starts `lead` scalars in front of the first of those signals, the output resource at the group's first
  // row -- stockham_wg_dct4.hpp, mdct_row)
  const unsigned long long fpw = p.fpw;
  const unsigned long long cross = std::min(n_signals - 1, (fpw - 1 + n_frames - 1) / n_frames);
  const unsigned long long reach_in = (cross * in_pitch + in_length + lead + 2 * n + 1) * sb;
  const unsigned long long reach_out = (cross * out_pitch + std::min(fpw - 1, n_frames - 1) * frame_pitch + n) * sb;
  if (reach_in > 0xFFFFFFFFull || reach_out > 0xFFFFFFFFull) {
    fail(PFFT_UNSUPPORTED_CONFIGURATION, "mdct: the ", cross + 1, " consecutive signals the rows of one work-group touch span ",
         reach_in, " bytes, their output rows ", reach_out, "; the kernel's 32-bit byte offsets end at 4 GiB (a single signal "
         "of 4 GiB or more, or as many shorter ones as a work-group holds rows)");
  }
  return {u32(n_signals), u32(n_frames),  u32(lead),      u32(in_length),
          u32(in_pitch),  u32(frame_pitch), u32(out_pitch), static_cast<long long>((n_signals * n_frames + fpw - 1) / fpw)};
}

struct imdct_geometry {
  unsigned n_signals, n_frames, lead, out_length, frame_pitch, in_pitch, out_pitch, chunk;
  long long groups;
};

/// Inverse modified discrete cosine transform, overlap-add at hop n of unfolded frames of 2n (stockham_wg_imdct.hpp):
/// istft_geometry_of's checks in its order with N -> 2n, hop -> n and a halo of one frame, counted in scalars on both
/// sides; chunk_frames 0: istft_default_chunk.
inline imdct_geometry imdct_geometry_of(const verb_facts& p, uintptr_t in, uintptr_t out, unsigned long long n_signals,
                                        unsigned long long n_frames, unsigned long long frame_pitch,
                                        unsigned long long in_pitch, unsigned long long lead,
                                        unsigned long long out_length, unsigned long long out_pitch,
                                        unsigned long long chunk_frames) {
  if (in == 0 || out == 0) fail(PFFT_INVALID_CONFIGURATION, "imdct: null data pointer");
  if (n_signals == 0 || n_frames == 0 || out_length == 0) {
    fail(PFFT_INVALID_CONFIGURATION, "imdct: zero count (", n_signals, " signals, ", n_frames, " frames, out_length ",
         out_length, ")");
  }
  const unsigned long long n = p.n;
  if (lead >= 2 * n) fail(PFFT_INVALID_CONFIGURATION, "imdct: lead ", lead, " must be below the frame length ", 2 * n);
  if (frame_pitch < n) {
    fail(PFFT_INVALID_CONFIGURATION, "imdct: frame_pitch ", frame_pitch, " below the ", n, " coefficients of a frame");
  }
  // (what would wrap the 64-bit arithmetic below; no buffer is that large)
  if (n_signals >= (1ull << 32) || n_frames >= (1ull << 32) || out_length >= (1ull << 32) || in_pitch >= (1ull << 32) ||
      frame_pitch >= (1ull << 32) || out_pitch >= (1ull << 32)) {
    fail(PFFT_UNSUPPORTED_CONFIGURATION, "imdct: the kernel addresses with 32-bit byte offsets: counts, lengths and pitches "
         "below 2^32 (4 GiB of bytes)");
  }
  if (in_pitch < n_frames * frame_pitch) {
    fail(PFFT_INVALID_CONFIGURATION, "imdct: in_pitch ", in_pitch, " below n_frames * frame_pitch = ", n_frames * frame_pitch);
  }
  if (out_pitch < out_length) fail(PFFT_INVALID_CONFIGURATION, "imdct: out_pitch ", out_pitch, " below out_length ", out_length);
  const unsigned long long last_e0 = (n_frames - 1) * n;  // first position of the last frame, in front of `lead`
  if (out_length + lead > last_e0 + 2 * n) {
    fail(PFFT_INVALID_CONFIGURATION, "imdct: out_length ", out_length, " above (n_frames - 1) * N + 2N - lead = ",
         last_e0 + 2 * n - lead, ": the samples behind it are covered by no frame");
  }
  if (last_e0 >= out_length + lead) {
    fail(PFFT_INVALID_CONFIGURATION, "imdct: frame ", n_frames - 1, " starts at sample ", last_e0, " - lead ", lead,
         ", beyond the out_length ", out_length, " samples: every frame must contribute at least one sample (n_frames; the "
         "hop is ", n, ")");
  }
  const unsigned long long sb = p.sb;
  // a chunk reads the frame of its halo after the chunk in front of it has stored: in place is a race
  if (byte_ranges_overlap(in, ((n_signals - 1) * in_pitch + (n_frames - 1) * frame_pitch + n) * sb, out,
                          ((n_signals - 1) * out_pitch + out_length) * sb)) {
    fail(PFFT_INVALID_CONFIGURATION, "imdct: the input and the output byte ranges overlap; the transform cannot run in "
         "place (a chunk reads coefficients another chunk's samples would overwrite)");
  }
  if (n_signals * n_frames >= (1ull << 31)) {
    fail(PFFT_UNSUPPORTED_CONFIGURATION, "imdct: ", n_signals, " signals of ", n_frames, " frames each: the kernel counts "
         "its rows in 32 bits, at most 2^31 - 1 (signal, frame) pairs per call");
  }
  const unsigned long long fpw = p.fpw;
  const unsigned long long chunk = chunk_frames == 0 ? istft_default_chunk(n_signals, n_frames, 1, fpw, p.resident[0])
                                                       : std::min(chunk_frames, n_frames);
  // One group runs at most 1 + chunk frames and owns at most chunk * n samples (the last chunk of a signal up to n more);
  // its resources start at its first frame and at its first sample.  A position of its first step wraps in front of the
  // owned samples by less than 2n + lead and a step reaches (fpw + 1) * n positions (stockham_wg_imdct.hpp).
  const unsigned long long run = std::min(n_frames, 1 + chunk);
  const unsigned long long reach_in = ((run - 1) * frame_pitch + n) * sb;
  const unsigned long long reach_out = (std::min(out_length, chunk * n + 2 * n) + (2 + fpw) * n + 2 * n + lead) * sb;
  if (reach_in > 0xFFFFFFFFull || reach_out > 0xFFFFFFFFull) {
    fail(PFFT_UNSUPPORTED_CONFIGURATION, "imdct: the ", run, " frames one work-group runs span ", reach_in, " bytes, the samples "
         "it covers ", reach_out, "; the kernel's 32-bit byte offsets end at 4 GiB (a smaller chunk_frames shortens both)");
  }
  return {u32(n_signals), u32(n_frames),  u32(lead),  u32(out_length), u32(frame_pitch),
          u32(in_pitch),  u32(out_pitch), u32(chunk), static_cast<long long>(n_signals * ((n_frames + chunk - 1) / chunk))};
}

struct periodogram_geometry {
  unsigned n_signals, n_frames, avg_frames, lead, hop, in_length, in_pitch, row_pitch, out_pitch;
  long long groups;
};

/// Power spectrogram / periodogram, sums of avg_frames consecutive squared STFT frames (stockham_wg_periodogram.hpp):
/// stft_geometry_of's checks in its order, the output counted in scalars and in rows of avg_frames frames.  A unit of the
/// kernel is one output row, R = ceil(n_frames / avg_frames) of them per signal.
inline periodogram_geometry periodogram_geometry_of(const verb_facts& p, uintptr_t in, uintptr_t out,
                                                    unsigned long long n_signals, unsigned long long in_length,
                                                    unsigned long long in_pitch, unsigned long long hop,
                                                    unsigned long long lead, int pad_mode, unsigned long long n_frames,
                                                    unsigned long long avg_frames, unsigned long long row_pitch,
                                                    unsigned long long out_pitch) {
  if (in == 0 || out == 0) fail(PFFT_INVALID_CONFIGURATION, "periodogram: null data pointer");
  if (n_signals == 0 || in_length == 0 || n_frames == 0 || avg_frames == 0) {
    fail(PFFT_INVALID_CONFIGURATION, "periodogram: zero count (", n_signals, " signals, in_length ", in_length, ", ", n_frames,
         " frames, avg_frames ", avg_frames, ")");
  }
  const unsigned long long n = p.n, m = n / 2;
  if (hop == 0) fail(PFFT_INVALID_CONFIGURATION, "periodogram: hop 0");
  if (lead >= n) fail(PFFT_INVALID_CONFIGURATION, "periodogram: lead ", lead, " must be below the frame length ", n);
  if (pad_mode != PFFT_PAD_ZERO && pad_mode != PFFT_PAD_REFLECT) {
    fail(PFFT_INVALID_CONFIGURATION, "Invalid periodogram pad_mode ", pad_mode);
  }
  if (avg_frames > n_frames) {
    fail(PFFT_INVALID_CONFIGURATION, "periodogram: avg_frames ", avg_frames, " above the ", n_frames, " frames of a signal");
  }
  if (in_pitch < in_length) fail(PFFT_INVALID_CONFIGURATION, "periodogram: in_pitch ", in_pitch, " below in_length ", in_length);
  if (row_pitch < m + 1) {
    fail(PFFT_INVALID_CONFIGURATION, "periodogram: row_pitch ", row_pitch, " below the ", m + 1, " bins of a row");
  }
  // (what would wrap the 64-bit arithmetic below; no buffer is that large.  avg_frames <= n_frames)
  if (n_signals >= (1ull << 32) || n_frames >= (1ull << 32) || hop >= (1ull << 32) || in_length >= (1ull << 32) ||
      in_pitch >= (1ull << 32) || row_pitch >= (1ull << 32) || out_pitch >= (1ull << 32)) {
    fail(PFFT_UNSUPPORTED_CONFIGURATION, "periodogram: the kernel addresses with 32-bit byte offsets: counts, lengths, hop "
         "and pitches below 2^32");
  }
  const unsigned long long rows = (n_frames + avg_frames - 1) / avg_frames;
  if (out_pitch < rows * row_pitch) {
    fail(PFFT_INVALID_CONFIGURATION, "periodogram: out_pitch ", out_pitch, " below ceil(n_frames / avg_frames) * row_pitch = ",
         rows * row_pitch);
  }
  const unsigned long long last_e0 = (n_frames - 1) * hop;  // first sample of the last frame, in front of `lead`
  if (pad_mode == PFFT_PAD_ZERO) {
    if (last_e0 >= in_length + lead) {
      fail(PFFT_INVALID_CONFIGURATION, "periodogram: frame ", n_frames - 1, " starts at sample ", last_e0, " - lead ", lead,
           ", beyond the in_length ", in_length, " samples: every frame must hold at least one sample (n_frames, hop)");
    }
  } else {
    if (lead > in_length - 1) {
      fail(PFFT_INVALID_CONFIGURATION, "periodogram: lead ", lead, " above in_length - 1 = ", in_length - 1,
           ": reflection mirrors an index at most once");
    }
    if (last_e0 + n > in_length + 2 * lead) {
      fail(PFFT_INVALID_CONFIGURATION, "periodogram: frame ", n_frames - 1, " ends at sample ", last_e0 + n, " - lead ", lead,
           ", beyond the signal of in_length ", in_length, " reflected by lead on both sides (n_frames, hop)");
    }
  }
  const unsigned long long sb = p.sb;
  // a row is stored while other work-groups still read the samples of theirs
  if (byte_ranges_overlap(in, ((n_signals - 1) * in_pitch + in_length) * sb, out,
                          ((n_signals - 1) * out_pitch + (rows - 1) * row_pitch + m + 1) * sb)) {
    fail(PFFT_INVALID_CONFIGURATION, "periodogram: the input and the output byte ranges overlap; the verb cannot run in "
         "place (a row's sums would overwrite samples another row's frames read)");
  }
  if (n_signals * rows >= (1ull << 31)) {
    fail(PFFT_UNSUPPORTED_CONFIGURATION, "periodogram: ", n_signals, " signals of ", rows, " rows each: the kernel counts "
         "its units in 32 bits, at most 2^31 - 1 (signal, row) pairs per call");
  }
  // The units of a group are fpw consecutive (signal, row) pairs: they cross at most `cross` signal boundaries.  The
  // input resource starts at the first of those signals (`lead` scalars in front of it): whatever avg_frames * hop lies
  // between the frames of neighbouring units, a live frame ends inside the signal extended by lead and n.  The output
  // resource starts at the group's first unit (stockham_wg_periodogram.hpp, periodogram_io).
  const unsigned long long fpw = p.fpw;
  const unsigned long long cross = std::min(n_signals - 1, (fpw - 1 + rows - 1) / rows);
  const unsigned long long reach_in = (cross * in_pitch + in_length + lead + n + 1) * sb;
  const unsigned long long reach_out = (cross * out_pitch + std::min(fpw - 1, rows - 1) * row_pitch + m + 1) * sb;
  if (reach_in > 0xFFFFFFFFull || reach_out > 0xFFFFFFFFull) {
    fail(PFFT_UNSUPPORTED_CONFIGURATION, "periodogram: the ", cross + 1, " consecutive signals the units of one work-group touch "
         "span ", reach_in, " bytes, their output rows ", reach_out, "; the kernel's 32-bit byte offsets end at 4 GiB (a single "
         "signal of 4 GiB or more, or as many shorter ones as a work-group holds rows)");
  }
  return {u32(n_signals), u32(n_frames),  u32(avg_frames), u32(lead),
          u32(hop),       u32(in_length), u32(in_pitch),   u32(row_pitch),
          u32(out_pitch), static_cast<long long>((n_signals * rows + fpw - 1) / fpw)};
}

struct pairs_geometry {
  unsigned n_rows;
  double floor;  // (the kernel takes it in the plan's scalar type, next to the scale: plan_t::pairs)
  unsigned x_length, x_pitch, y_length, y_pitch, out_length, out_pitch;
  long long groups;
};

/// Convolution / correlation of pairs of real rows (stockham_wg_pairs.hpp): row t of x (x_length scalars) with row t of y
/// (y_length) into the first out_length scalars of row t of out, all three with pitches in scalars; `floor`: 0, or the
/// floor of the phase transform (PFFT_CORRELATE only).  x and y may be the same rows; out may share no byte with either.
inline pairs_geometry pairs_geometry_of(const verb_facts& p, int mode, uintptr_t x, uintptr_t y, uintptr_t out,
                                        unsigned long long n_rows, unsigned long long x_length, unsigned long long x_pitch,
                                        unsigned long long y_length, unsigned long long y_pitch,
                                        unsigned long long out_length, unsigned long long out_pitch, double floor) {
  if (x == 0 || y == 0 || out == 0) fail(PFFT_INVALID_CONFIGURATION, "pairs: null data pointer");
  if (mode != PFFT_CONVOLVE && mode != PFFT_CORRELATE) {
    fail(PFFT_INVALID_CONFIGURATION, "pairs: mode ", mode, " is neither PFFT_CONVOLVE nor PFFT_CORRELATE");
  }
  if (n_rows == 0) fail(PFFT_INVALID_CONFIGURATION, "pairs: zero count (n_rows 0)");
  const unsigned long long n = p.n;
  if (x_length == 0 || y_length == 0 || out_length == 0 || x_length > n || y_length > n || out_length > n) {
    fail(PFFT_INVALID_CONFIGURATION, "pairs: lengths (x ", x_length, ", y ", y_length, ", out ", out_length,
         ") must be in 1 ... ", n, ", the plan's length");
  }
  if (x_pitch < x_length || y_pitch < y_length || out_pitch < out_length) {
    fail(PFFT_INVALID_CONFIGURATION, "pairs: pitches (x ", x_pitch, ", y ", y_pitch, ", out ", out_pitch,
         ") below the lengths (", x_length, ", ", y_length, ", ", out_length, ")");
  }
  // (the smallest normal number and the largest finite one of the plan's scalar type)
  const double tiny = p.sb == 8 ? 2.2250738585072014e-308 : 1.17549435082228751e-38;
  const double huge = p.sb == 8 ? 1.7976931348623157e308 : 3.40282346638528860e38;
  if (!(floor >= 0.0) || floor > huge || (floor > 0.0 && floor < tiny)) {  // (a NaN fails the first comparison)
    fail(PFFT_INVALID_CONFIGURATION, "pairs: phat_floor ", floor, " must be 0 (no phase transform) or a positive normal "
         "number of the plan's scalar type (", tiny, " ... ", huge, ")");
  }
  if (floor != 0.0 && mode == PFFT_CONVOLVE) {
    fail(PFFT_INVALID_CONFIGURATION, "pairs: phat_floor ", floor, " with PFFT_CONVOLVE; the phase transform belongs to "
         "PFFT_CORRELATE");
  }
  // groups store rows of out while others still load x and y.  (128 bits: the row count and the pitches are checked
  // below, and a refusal there must not come from a wrapped product here)
  using wide = unsigned __int128;
  const wide sb = p.sb;
  auto extent = [&](unsigned long long pitch, unsigned long long length) { return (wide(n_rows - 1) * pitch + length) * sb; };
  auto overlap = [&](uintptr_t a, wide a_bytes, uintptr_t b, wide b_bytes) { return wide(a) < wide(b) + b_bytes && wide(b) < wide(a) + a_bytes; };
  const wide out_bytes = extent(out_pitch, out_length);
  if (overlap(x, extent(x_pitch, x_length), out, out_bytes) || overlap(y, extent(y_pitch, y_length), out, out_bytes)) {
    fail(PFFT_INVALID_CONFIGURATION, "pairs: the output byte range overlaps an input's; the verb cannot run in place (a "
         "group's stores would overwrite rows another group has not loaded)");
  }
  if (n_rows >= (1ull << 31)) {
    fail(PFFT_UNSUPPORTED_CONFIGURATION, "pairs: ", n_rows, " rows: at most 2^31 - 1 rows per call");
  }
  if (x_pitch >= (1ull << 32) || y_pitch >= (1ull << 32) || out_pitch >= (1ull << 32)) {
    fail(PFFT_UNSUPPORTED_CONFIGURATION, "pairs: pitches (x ", x_pitch, ", y ", y_pitch, ", out ", out_pitch,
         ") must be below 2^32 scalars");
  }
  // (dct_geometry_of: every row slot of a group computes its 32-bit offset f * pitch, missing rows included, so the whole
  // group is bounded whatever n_rows is)
  const unsigned long long fpw = p.fpw;
  const unsigned long long reach_x = fpw * x_pitch * p.sb, reach_y = fpw * y_pitch * p.sb, reach_out = fpw * out_pitch * p.sb;
  if (reach_x > 0xFFFFFFFFull || reach_y > 0xFFFFFFFFull || reach_out > 0xFFFFFFFFull) {
    fail(PFFT_UNSUPPORTED_CONFIGURATION, "pairs: the ", fpw, " row slots of one work-group span ", reach_x, " bytes of x, ",
         reach_y, " of y and ", reach_out, " of the output; the kernel's 32-bit byte offsets end at 4 GiB");
  }
  return {u32(n_rows),  floor,           u32(x_length),   u32(x_pitch),
          u32(y_length), u32(y_pitch),   u32(out_length), u32(out_pitch),
          static_cast<long long>((n_rows + fpw - 1) / fpw)};
}

}  // namespace pfa
