// The call-geometry rules of the fused verbs (portfft_amd/csrc/verb_geometry.hpp) on the CPU: every refusal with its
// status and text, every 32-bit boundary as the pair (largest admitted value, that value + 1), the kernel arguments of
// admitted calls against values worked out by hand (the derivation stands at each case), and the order of the checks.
// Includes the header only; links nothing of the library.
#include <cstdio>
#include <cstring>
#include <string>

#include "../../portfft_amd/csrc/verb_geometry.hpp"

using namespace pfa;
using ull = unsigned long long;

static int failures = 0;
static int cases = 0;

#define CHECK_EQ(what, got, want)                                                                        \
  do {                                                                                                   \
    ++cases;                                                                                             \
    const long long g_ = static_cast<long long>(got), w_ = static_cast<long long>(want);                 \
    if (g_ != w_) {                                                                                      \
      ++failures;                                                                                        \
      std::printf("FAIL %s: %s = %lld, expected %lld\n", what, #got, g_, w_);                           \
    }                                                                                                    \
  } while (0)

/// `f` must be refused with `st` and a message containing `sub`
template <typename F>
static void refused(const char* what, pfft_status st, const char* sub, F&& f) {
  ++cases;
  try {
    f();
    ++failures;
    std::printf("FAIL %s: admitted, expected a refusal with \"%s\"\n", what, sub);
  } catch (const error& e) {
    if (e.status != st || std::strstr(e.what(), sub) == nullptr) {
      ++failures;
      std::printf("FAIL %s: status %d \"%s\", expected status %d with \"%s\"\n", what, static_cast<int>(e.status), e.what(),
                  static_cast<int>(st), sub);
    }
  }
}

/// `f` must be admitted; returns its geometry
template <typename F>
static auto admitted(const char* what, F&& f) -> decltype(f()) {
  ++cases;
  try {
    return f();
  } catch (const error& e) {
    ++failures;
    std::printf("FAIL %s: refused with status %d \"%s\"\n", what, static_cast<int>(e.status), e.what());
    return decltype(f()){};
  }
}

static const pfft_status INVALID = PFFT_INVALID_CONFIGURATION, UNSUPPORTED = PFFT_UNSUPPORTED_CONFIGURATION;
// far apart: no geometry below makes the two byte ranges meet unless a case moves them
static const uintptr_t IN = uintptr_t(1) << 48, OUT = uintptr_t(1) << 52;
static const ull P31 = 1ull << 31, P32 = 1ull << 32;

static verb_facts facts(ull n, ull sb, bool real, ull taps, ull fpw, ull resident = 256) {
  verb_facts p;
  p.n = n;
  p.sb = sb;
  p.real = real;
  p.taps = taps;
  p.fpw = fpw;
  p.resident[0] = p.resident[1] = resident;
  return p;
}

static void test_overlap() {
  CHECK_EQ("touching ranges", byte_ranges_overlap(100, 50, 150, 10), 0);
  CHECK_EQ("one shared byte", byte_ranges_overlap(100, 51, 150, 10), 1);
  CHECK_EQ("touching ranges, swapped", byte_ranges_overlap(150, 10, 100, 50), 0);
  CHECK_EQ("one shared byte, swapped", byte_ranges_overlap(150, 10, 100, 51), 1);
  CHECK_EQ("identical ranges", byte_ranges_overlap(100, 8, 100, 8), 1);
  CHECK_EQ("contained range", byte_ranges_overlap(100, 80, 120, 8), 1);
}

static void test_dct() {
  const verb_facts p = facts(64, 4, true, 0, 4);  // fp32, N = 64, 4 rows per work-group
  auto call = [&](int type, uintptr_t in, uintptr_t out, ull rows, ull ip, ull op) {
    return [=] { return dct_geometry_of(p, type, in, out, rows, ip, op); };
  };
  // refusals, in the order of the checks
  refused("dct null in", INVALID, "dct: null data pointer", call(2, 0, OUT, 1, 64, 64));
  refused("dct null out", INVALID, "dct: null data pointer", call(2, IN, 0, 1, 64, 64));
  refused("dct no rows", INVALID, "zero count (n_rows 0)", call(2, IN, OUT, 0, 64, 64));
  refused("dct type 1", INVALID, "Invalid dct type 1", call(1, IN, OUT, 1, 64, 64));
  refused("dct type 4", INVALID, "Invalid dct type 4", call(4, IN, OUT, 1, 64, 64));
  refused("dct in_pitch", INVALID, "in_pitch 63 below the row length 64", call(2, IN, OUT, 1, 63, 64));
  refused("dct out_pitch", INVALID, "out_pitch 63 below the row length 64", call(3, IN, OUT, 1, 64, 63));
  refused("dct in_pitch 2^32", UNSUPPORTED, "row slots of one work-group span", call(2, IN, OUT, 1, P32, 64));
  refused("dct out_pitch 2^32", UNSUPPORTED, "row slots of one work-group span", call(2, IN, OUT, 1, 64, P32));
  // fpw * pitch * sb <= 2^32 - 1 with fpw = 4, sb = 4: pitch <= floor(4294967295 / 16) = 268435455
  admitted("dct in_pitch 268435455", call(2, IN, OUT, 1, 268435455, 64));
  refused("dct in_pitch 268435456", UNSUPPORTED, "the 4 row slots of one work-group span 4294967296 bytes of the input",
          call(2, IN, OUT, 1, 268435456, 64));
  admitted("dct out_pitch 268435455", call(3, IN, OUT, 1, 64, 268435455));
  refused("dct out_pitch 268435456", UNSUPPORTED, "and 4294967296 of the output", call(3, IN, OUT, 1, 64, 268435456));
  // rows: 2^31 - 1 admitted -- ceil((2^31 - 1) / 4) = 2^29 groups --, 2^31 refused
  const dct_geometry top = admitted("dct 2^31 - 1 rows", call(2, IN, OUT, P31 - 1, 64, 64));
  CHECK_EQ("dct 2^31 - 1 rows", top.n_rows, 2147483647ll);
  CHECK_EQ("dct 2^31 - 1 rows", top.groups, 536870912ll);
  refused("dct 2^31 rows", UNSUPPORTED, "2147483648 rows: at most 2^31 - 1 rows per call", call(2, IN, OUT, P31, 64, 64));
  // overlap: identical with equal pitches is in place; identical with unequal pitches and partial overlap are refused
  const dct_geometry inplace = admitted("dct in place", call(2, IN, IN, 9, 72, 72));
  CHECK_EQ("dct in place", inplace.groups, 3);  // ceil(9 / 4)
  CHECK_EQ("dct in place", inplace.in_pitch, 72);
  CHECK_EQ("dct in place", inplace.out_pitch, 72);
  refused("dct in place, unequal pitches", INVALID, "needs equal pitches, not in_pitch 72 and out_pitch 80", call(2, IN, IN, 9, 72, 80));
  // 9 rows at pitch 72: (8 * 72 + 64) * 4 = 2560 bytes
  refused("dct partial overlap", INVALID, "overlap without being identical", call(2, IN, IN + 2559, 9, 72, 72));
  refused("dct partial overlap, out first", INVALID, "overlap without being identical", call(2, IN + 2559, IN, 9, 72, 72));
  const dct_geometry disjoint = admitted("dct disjoint", call(3, IN, IN + 2560, 9, 72, 72));
  CHECK_EQ("dct disjoint", disjoint.n_rows, 9);
  CHECK_EQ("dct disjoint", disjoint.groups, 3);
  admitted("dct disjoint, out first", call(3, IN + 2560, IN, 9, 72, 72));
  // two rules broken: the pitch is checked before the row count, the row count before the reach
  refused("dct pitch before rows", INVALID, "in_pitch 63 below", call(2, IN, OUT, P31, 63, 64));
  refused("dct rows before reach", UNSUPPORTED, "at most 2^31 - 1 rows", call(2, IN, OUT, P31, 268435456, 64));
}

static void test_filter() {
  auto call = [](const verb_facts& p, int mode, uintptr_t in, uintptr_t out, ull ns, ull il, ull ip, ull ol, ull op) {
    return [=] { return filter_geometry_of(p, mode, in, out, ns, il, ip, ol, op); };
  };
  const int CONV = PFFT_CONVOLVE, CORR = PFFT_CORRELATE;
  const verb_facts c17 = facts(1024, 4, false, 17, 4), c18 = facts(1024, 4, false, 18, 4);
  const verb_facts r17 = facts(1024, 4, true, 17, 4), r18 = facts(1024, 4, true, 18, 4);
  // refusals, in the order of the checks
  refused("filter no signals", INVALID, "filter: zero count (0 signals", call(c17, CONV, IN, OUT, 0, 100, 100, 100, 100));
  refused("filter no input", INVALID, "filter: zero count (1 signals, in_length 0", call(c17, CONV, IN, OUT, 1, 0, 100, 100, 100));
  refused("filter no output", INVALID, "out_length 0)", call(c17, CONV, IN, OUT, 1, 100, 100, 0, 100));
  refused("filter real taps", INVALID, "1023 taps on a real plan of length 1024", call(facts(1024, 4, true, 1023, 4), CONV, IN, OUT, 1, 100, 100, 100, 100));
  admitted("filter real 1022 taps", call(facts(1024, 4, true, 1022, 4), CONV, IN, OUT, 1, 100, 100, 100, 100));
  refused("filter convolve out_length", INVALID, "out_length 117 beyond 116 (in_length + taps - 1", call(c17, CONV, IN, OUT, 1, 100, 100, 117, 117));
  admitted("filter convolve out_length 116", call(c17, CONV, IN, OUT, 1, 100, 100, 116, 116));
  refused("filter correlate out_length", INVALID, "out_length 101 beyond 100 (in_length: the non-negative lags", call(c17, CORR, IN, OUT, 1, 100, 100, 101, 101));
  refused("filter in_pitch", INVALID, "pitches (99, 100) below the lengths (100, 100)", call(c17, CONV, IN, OUT, 2, 100, 99, 100, 100));
  refused("filter out_pitch", INVALID, "pitches (100, 99) below the lengths (100, 100)", call(c17, CONV, IN, OUT, 2, 100, 100, 100, 99));
  refused("filter 2^32 signals", UNSUPPORTED, "at most 2^32 - 1 signals and pitches below 4 GiB", call(c17, CONV, IN, OUT, P32, 8, 8, 8, 8));
  refused("filter in_pitch 2^32", UNSUPPORTED, "at most 2^32 - 1 signals and pitches below 4 GiB", call(c17, CONV, IN, OUT, 1, 8, P32, 8, 8));
  refused("filter out_pitch 2^32", UNSUPPORTED, "at most 2^32 - 1 signals and pitches below 4 GiB", call(c17, CONV, IN, OUT, 1, 8, 8, 8, P32));
  refused("filter 2^56 samples", UNSUPPORTED, "at most 2^32 - 1 signals and pitches below 4 GiB", call(c17, CONV, IN, OUT, 1ull << 28, 8, 1ull << 28, 8, 8));
  // 3 signals of 100 samples at pitch 128, 8 bytes each: (2 * 128 + 100) * 8 = 2848 bytes
  refused("filter in place", INVALID, "byte ranges overlap; overlap-save filtering", call(c17, CONV, IN, IN, 3, 100, 128, 100, 128));
  refused("filter partial overlap", INVALID, "byte ranges overlap; overlap-save filtering", call(c17, CONV, IN, IN + 2847, 3, 100, 128, 100, 128));
  admitted("filter adjacent", call(c17, CONV, IN, IN + 2848, 3, 100, 128, 100, 128));
  // ... of a real plan 4 bytes each: 1424 bytes
  refused("filter real partial overlap", INVALID, "byte ranges overlap", call(r17, CONV, IN + 1423, IN, 3, 100, 128, 100, 128));
  admitted("filter real adjacent", call(r17, CONV, IN + 1424, IN, 3, 100, 128, 100, 128));
  // reach of one complex fp32 signal, 17 taps: (length + 16) * 8 <= 2^32 - 1, length + 16 <= 536870911
  admitted("filter complex reach, 1 signal", call(c17, CONV, IN, OUT, 1, 536870895, 536870895, 536870895, 536870895));
  refused("filter complex reach, 1 signal", UNSUPPORTED, "1 consecutive signals (the rows of one work-group) span 4294967296 bytes",
          call(c17, CONV, IN, OUT, 1, 536870896, 536870896, 536870896, 536870896));
  // correlate reaches as far: lead_conv counts whatever the mode (the output length decides)
  admitted("filter complex reach, correlate", call(c17, CORR, IN, OUT, 1, 536870895, 536870895, 536870895, 536870895));
  refused("filter complex reach, correlate", UNSUPPORTED, "span 4294967296 bytes", call(c17, CORR, IN, OUT, 1, 536870896, 536870896, 536870896, 536870896));
  // ... of span = fpw = 4 short signals: (3 * pitch + 1000 + 16) * 8 <= 2^32 - 1, 3 * pitch <= 536869895, pitch <= 178956631
  admitted("filter complex reach, 4 signals, in", call(c17, CONV, IN, OUT, 4, 1000, 178956631, 1000, 1000));
  refused("filter complex reach, 4 signals, in", UNSUPPORTED, "4 consecutive signals (the rows of one work-group) span 4294967296 bytes",
          call(c17, CONV, IN, OUT, 4, 1000, 178956632, 1000, 1000));
  admitted("filter complex reach, 9 signals, out", call(c17, CORR, IN, OUT, 9, 1000, 1000, 1000, 178956631));
  refused("filter complex reach, 9 signals, out", UNSUPPORTED, "4 consecutive signals", call(c17, CORR, IN, OUT, 9, 1000, 1000, 1000, 178956632));
  // a real fp32 plan, 17 taps: lead_conv 16 and one scalar more: (length + 17) * 4 <= 2^32 - 1, length + 17 <= 1073741823
  admitted("filter real reach, 1 signal", call(r17, CONV, IN, OUT, 1, 1073741806, 1073741806, 1073741806, 1073741806));
  refused("filter real reach, 1 signal", UNSUPPORTED, "1 consecutive signals (the rows of one work-group) span 4294967296 bytes",
          call(r17, CONV, IN, OUT, 1, 1073741807, 1073741807, 1073741807, 1073741807));
  // ... 18 taps: lead_conv 18: length + 19 <= 1073741823
  admitted("filter real reach, 18 taps", call(r18, CONV, IN, OUT, 1, 1073741804, 1073741804, 1073741804, 1073741804));
  refused("filter real reach, 18 taps", UNSUPPORTED, "span 4294967296 bytes", call(r18, CONV, IN, OUT, 1, 1073741805, 1073741805, 1073741805, 1073741805));
  // ... span = 4: (3 * pitch + 1000 + 17) * 4 <= 2^32 - 1, 3 * pitch <= 1073740806 = 3 * 357913602
  admitted("filter real reach, 4 signals", call(r17, CONV, IN, OUT, 4, 1000, 357913602, 1000, 1000));
  refused("filter real reach, 4 signals", UNSUPPORTED, "4 consecutive signals (the rows of one work-group) span 4294967304 bytes",
          call(r17, CONV, IN, OUT, 4, 1000, 357913603, 1000, 1000));
  // rows: 2^31 - 1 signals of one segment admitted -- 2^29 groups of 4 --, 2^31 refused; so are 2^30 signals of 2 segments
  const filter_geometry rows = admitted("filter 2^31 - 1 rows", call(c17, CONV, IN, OUT, P31 - 1, 8, 8, 8, 8));
  CHECK_EQ("filter 2^31 - 1 rows", rows.n_signals, 2147483647ll);
  CHECK_EQ("filter 2^31 - 1 rows", rows.n_seg, 1);
  CHECK_EQ("filter 2^31 - 1 rows", rows.groups, 536870912ll);
  refused("filter 2^31 rows", UNSUPPORTED, "2147483648 signals of 1 segments each", call(c17, CONV, IN, OUT, P31, 8, 8, 8, 8));
  refused("filter 2^30 x 2 rows", UNSUPPORTED, "1073741824 signals of 2 segments each", call(c17, CONV, IN, OUT, 1ull << 30, 1009, 1009, 1009, 1009));
  // admitted calls: 5 signals, out_length 3000.  complex: lead = taps - 1 (convolve) / 0, hop = N - taps + 1
  struct { const verb_facts* p; int mode; unsigned lead, hop, n_seg; const char* what; } want[] = {
      {&c17, CONV, 16, 1008, 3, "complex 17 taps convolve"},  // ceil(3000 / 1008) = 3
      {&c17, CORR, 0, 1008, 3, "complex 17 taps correlate"},
      {&c18, CONV, 17, 1007, 3, "complex 18 taps convolve"},
      {&c18, CORR, 0, 1007, 3, "complex 18 taps correlate"},
      // real: lead = taps - 1 rounded up to even, hop = N - lead (convolve) / N - taps + 1 rounded down to even
      {&r17, CONV, 16, 1008, 3, "real 17 taps convolve"},
      {&r17, CORR, 0, 1008, 3, "real 17 taps correlate"},
      {&r18, CONV, 18, 1006, 3, "real 18 taps convolve"},
      {&r18, CORR, 0, 1006, 3, "real 18 taps correlate"},
  };
  for (const auto& w : want) {
    const filter_geometry g = admitted(w.what, call(*w.p, w.mode, IN, OUT, 5, 3000, 3100, 3000, 3200));
    CHECK_EQ(w.what, g.n_signals, 5);
    CHECK_EQ(w.what, g.n_seg, w.n_seg);
    CHECK_EQ(w.what, g.lead, w.lead);
    CHECK_EQ(w.what, g.hop, w.hop);
    CHECK_EQ(w.what, g.in_length, 3000);
    CHECK_EQ(w.what, g.out_length, 3000);
    CHECK_EQ(w.what, g.in_pitch, 3100);
    CHECK_EQ(w.what, g.out_pitch, 3200);
    CHECK_EQ(w.what, g.groups, 4);  // ceil(5 * 3 / 4)
  }
  // hop 1006: 1006 samples are one segment, 1007 two
  CHECK_EQ("real 18 taps, 1006 samples", admitted("real 18 taps, 1006 samples", call(r18, CORR, IN, OUT, 1, 2000, 2000, 1006, 1006)).n_seg, 1);
  CHECK_EQ("real 18 taps, 1007 samples", admitted("real 18 taps, 1007 samples", call(r18, CORR, IN, OUT, 1, 2000, 2000, 1007, 1007)).n_seg, 2);
  // two rules broken: the output length is checked before the pitches, the pitches before the overlap
  refused("filter out_length before pitches", INVALID, "out_length 117 beyond 116", call(c17, CONV, IN, OUT, 1, 100, 99, 117, 100));
  refused("filter pitches before overlap", INVALID, "pitches (99, 100) below", call(c17, CONV, IN, IN, 1, 100, 99, 100, 100));
  refused("filter overlap before reach", INVALID, "byte ranges overlap", call(c17, CONV, IN, IN, 1, 536870896, 536870896, 536870896, 536870896));
}

static void test_stft() {
  const verb_facts p = facts(1024, 4, true, 0, 4);  // fp32, N = 1024 (513 bins), 4 rows per work-group
  const int ZERO = PFFT_PAD_ZERO, REFLECT = PFFT_PAD_REFLECT;
  auto call = [&](uintptr_t in, uintptr_t out, ull ns, ull il, ull ip, ull hop, ull lead, int pad, ull nf, ull fp, ull op) {
    return [=] { return stft_geometry_of(p, in, out, ns, il, ip, hop, lead, pad, nf, fp, op); };
  };
  // refusals, in the order of the checks
  refused("stft null in", INVALID, "stft: null data pointer", call(0, OUT, 1, 2000, 2000, 256, 0, ZERO, 4, 513, 2052));
  refused("stft null out", INVALID, "stft: null data pointer", call(IN, 0, 1, 2000, 2000, 256, 0, ZERO, 4, 513, 2052));
  refused("stft no signals", INVALID, "stft: zero count (0 signals", call(IN, OUT, 0, 2000, 2000, 256, 0, ZERO, 4, 513, 2052));
  refused("stft no input", INVALID, "in_length 0, 4 frames)", call(IN, OUT, 1, 0, 2000, 256, 0, ZERO, 4, 513, 2052));
  refused("stft no frames", INVALID, "in_length 2000, 0 frames)", call(IN, OUT, 1, 2000, 2000, 256, 0, ZERO, 0, 513, 2052));
  refused("stft hop 0", INVALID, "stft: hop 0", call(IN, OUT, 1, 2000, 2000, 0, 0, ZERO, 4, 513, 2052));
  refused("stft lead", INVALID, "lead 1024 must be below the frame length 1024", call(IN, OUT, 1, 2000, 2000, 256, 1024, ZERO, 4, 513, 2052));
  refused("stft pad_mode", INVALID, "Invalid stft pad_mode 2", call(IN, OUT, 1, 2000, 2000, 256, 0, 2, 4, 513, 2052));
  refused("stft in_pitch", INVALID, "in_pitch 1999 below in_length 2000", call(IN, OUT, 2, 2000, 1999, 256, 0, ZERO, 4, 513, 2052));
  refused("stft frame_pitch", INVALID, "frame_pitch 512 below the 513 bins", call(IN, OUT, 1, 2000, 2000, 256, 0, ZERO, 4, 512, 2052));
  refused("stft 2^32 signals", UNSUPPORTED, "counts, lengths, hop and pitches below 2^32", call(IN, OUT, P32, 2000, 2000, 256, 0, ZERO, 4, 513, 2052));
  refused("stft 2^32 frames", UNSUPPORTED, "counts, lengths, hop and pitches below 2^32", call(IN, OUT, 1, 2000, 2000, 256, 0, ZERO, P32, 513, 2052));
  refused("stft hop 2^32", UNSUPPORTED, "counts, lengths, hop and pitches below 2^32", call(IN, OUT, 1, 2000, 2000, P32, 0, ZERO, 4, 513, 2052));
  refused("stft in_length 2^32", UNSUPPORTED, "counts, lengths, hop and pitches below 2^32", call(IN, OUT, 1, P32, P32, 256, 0, ZERO, 4, 513, 2052));
  refused("stft in_pitch 2^32", UNSUPPORTED, "counts, lengths, hop and pitches below 2^32", call(IN, OUT, 1, 2000, P32, 256, 0, ZERO, 4, 513, 2052));
  refused("stft frame_pitch 2^32", UNSUPPORTED, "counts, lengths, hop and pitches below 2^32", call(IN, OUT, 1, 2000, 2000, 256, 0, ZERO, 4, P32, 2052));
  refused("stft out_pitch 2^32", UNSUPPORTED, "counts, lengths, hop and pitches below 2^32", call(IN, OUT, 1, 2000, 2000, 256, 0, ZERO, 4, 513, P32));
  refused("stft out_pitch", INVALID, "out_pitch 2051 below n_frames * frame_pitch = 2052", call(IN, OUT, 2, 2000, 2000, 256, 0, ZERO, 4, 513, 2051));
  // zero extension: frame 3 starts at 3 * 256 = 768 - lead; 768 samples + lead 0 leave it empty, 769 do not
  refused("stft empty frame", INVALID, "frame 3 starts at sample 768 - lead 0, beyond the in_length 768", call(IN, OUT, 1, 768, 768, 256, 0, ZERO, 4, 513, 2052));
  admitted("stft one sample in the last frame", call(IN, OUT, 1, 769, 769, 256, 0, ZERO, 4, 513, 2052));
  // reflection: lead <= in_length - 1, and the last frame ends at 768 + 1024 = 1792 <= in_length + 2 * lead
  refused("stft reflect lead", INVALID, "lead 512 above in_length - 1 = 511", call(IN, OUT, 1, 512, 512, 256, 512, REFLECT, 1, 513, 513));
  refused("stft reflect end", INVALID, "frame 3 ends at sample 1792 - lead 512, beyond the signal of in_length 767", call(IN, OUT, 1, 767, 767, 256, 512, REFLECT, 4, 513, 2052));
  admitted("stft reflect, torch's centre", call(IN, OUT, 1, 768, 768, 256, 512, REFLECT, 4, 513, 2052));
  // 2 signals of 2000 scalars: (2000 + 2000) * 4 = 16000 bytes in; (2052 + 3 * 513 + 513) * 8 = 32832 bytes out
  refused("stft in place", INVALID, "byte ranges overlap; the transform cannot run in place (overlapping frames", call(IN, IN, 2, 2000, 2000, 256, 0, ZERO, 4, 513, 2052));
  refused("stft partial overlap", INVALID, "byte ranges overlap", call(IN, IN + 15999, 2, 2000, 2000, 256, 0, ZERO, 4, 513, 2052));
  admitted("stft adjacent", call(IN, IN + 16000, 2, 2000, 2000, 256, 0, ZERO, 4, 513, 2052));
  refused("stft partial overlap, out first", INVALID, "byte ranges overlap", call(IN + 32831, IN, 2, 2000, 2000, 256, 0, ZERO, 4, 513, 2052));
  admitted("stft adjacent, out first", call(IN + 32832, IN, 2, 2000, 2000, 256, 0, ZERO, 4, 513, 2052));
  // rows: 2^31 - 1 signals of one frame admitted -- 2^29 groups --, 2^31 refused
  const stft_geometry rows = admitted("stft 2^31 - 1 rows", call(IN, OUT, P31 - 1, 8, 8, 1, 0, ZERO, 1, 513, 513));
  CHECK_EQ("stft 2^31 - 1 rows", rows.groups, 536870912ll);
  refused("stft 2^31 rows", UNSUPPORTED, "2147483648 signals of 1 frames each", call(IN, OUT, P31, 8, 8, 1, 0, ZERO, 1, 513, 513));
  refused("stft 2^16 x 2^15 rows", UNSUPPORTED, "65536 signals of 32768 frames each", call(IN, OUT, 1ull << 16, 40000, 40000, 1, 0, ZERO, 1ull << 15, 513, 513ull << 15));
  // reach_in, one signal (cross = 0): (in_length + lead + 1024 + 1) * 4 <= 2^32 - 1, in_length + lead <= 1073740798
  admitted("stft reach_in, 1 signal", call(IN, OUT, 1, 1073740798, 1073740798, 1, 0, ZERO, 1, 513, 513));
  refused("stft reach_in, 1 signal", UNSUPPORTED, "the 1 consecutive signals the rows of one work-group touch span 4294967296 bytes",
          call(IN, OUT, 1, 1073740799, 1073740799, 1, 0, ZERO, 1, 513, 513));
  admitted("stft reach_in, 1 signal, lead 1023", call(IN, OUT, 1, 1073739775, 1073739775, 1, 1023, ZERO, 1, 513, 513));
  refused("stft reach_in, 1 signal, lead 1023", UNSUPPORTED, "span 4294967296 bytes", call(IN, OUT, 1, 1073739776, 1073739776, 1, 1023, ZERO, 1, 513, 513));
  // reach_out, one signal of 4 frames: (3 * frame_pitch + 513) * 8 <= 2^32 - 1, 3 * frame_pitch <= 536870398, frame_pitch <= 178956799
  admitted("stft reach_out, 1 signal", call(IN, OUT, 1, 2000, 2000, 1, 0, ZERO, 4, 178956799, 4ull * 178956799));
  refused("stft reach_out, 1 signal", UNSUPPORTED, "their output rows 4294967304;", call(IN, OUT, 1, 2000, 2000, 1, 0, ZERO, 4, 178956800, 4ull * 178956800));
  // 9 signals of 1 frame: the 4 rows of a group cross min(8, ceil(3 / 1)) = 3 signal boundaries
  //   in: (3 * in_pitch + 2000 + 1025) * 4 <= 2^32 - 1, 3 * in_pitch <= 1073738798, in_pitch <= 357912932
  admitted("stft reach_in, 1 frame", call(IN, OUT, 9, 2000, 357912932, 1, 0, ZERO, 1, 513, 513));
  refused("stft reach_in, 1 frame", UNSUPPORTED, "the 4 consecutive signals the rows of one work-group touch span 4294967296 bytes",
          call(IN, OUT, 9, 2000, 357912933, 1, 0, ZERO, 1, 513, 513));
  //   out: (3 * out_pitch + 513) * 8 <= 2^32 - 1, out_pitch <= 178956799
  admitted("stft reach_out, 1 frame", call(IN, OUT, 9, 2000, 2000, 1, 0, ZERO, 1, 513, 178956799));
  refused("stft reach_out, 1 frame", UNSUPPORTED, "the 4 consecutive signals", call(IN, OUT, 9, 2000, 2000, 1, 0, ZERO, 1, 513, 178956800));
  // 9 signals of 3 frames: min(8, ceil(3 / 3)) = 1 boundary
  //   in: (in_pitch + 2000 + 1025) * 4 <= 2^32 - 1, in_pitch <= 1073738798
  admitted("stft reach_in, 3 frames", call(IN, OUT, 9, 2000, 1073738798, 1, 0, ZERO, 3, 515, 1545));
  refused("stft reach_in, 3 frames", UNSUPPORTED, "the 2 consecutive signals the rows of one work-group touch span 4294967296 bytes",
          call(IN, OUT, 9, 2000, 1073738799, 1, 0, ZERO, 3, 515, 1545));
  //   out: (out_pitch + 2 * 515 + 513) * 8 <= 2^32 - 1, out_pitch <= 536870911 - 1543 = 536869368
  admitted("stft reach_out, 3 frames", call(IN, OUT, 9, 2000, 2000, 1, 0, ZERO, 3, 515, 536869368));
  refused("stft reach_out, 3 frames", UNSUPPORTED, "the 2 consecutive signals", call(IN, OUT, 9, 2000, 2000, 1, 0, ZERO, 3, 515, 536869369));
  // admitted calls: the arguments pass through, groups = ceil(signals * frames / 4)
  const stft_geometry g = admitted("stft 3 x 7", call(IN, OUT, 3, 3000, 3100, 300, 512, REFLECT, 7, 520, 3700));
  CHECK_EQ("stft 3 x 7", g.n_signals, 3);
  CHECK_EQ("stft 3 x 7", g.n_frames, 7);
  CHECK_EQ("stft 3 x 7", g.lead, 512);
  CHECK_EQ("stft 3 x 7", g.hop, 300);
  CHECK_EQ("stft 3 x 7", g.in_length, 3000);
  CHECK_EQ("stft 3 x 7", g.in_pitch, 3100);
  CHECK_EQ("stft 3 x 7", g.frame_pitch, 520);
  CHECK_EQ("stft 3 x 7", g.out_pitch, 3700);
  CHECK_EQ("stft 3 x 7", g.groups, 6);  // ceil(21 / 4)
  CHECK_EQ("stft 1 x 4", admitted("stft 1 x 4", call(IN, OUT, 1, 2000, 2000, 256, 0, ZERO, 4, 513, 2052)).groups, 1);
  CHECK_EQ("stft 1 x 5", admitted("stft 1 x 5", call(IN, OUT, 1, 2000, 2000, 256, 0, ZERO, 5, 513, 2565)).groups, 2);
  // two rules broken: hop before lead, the pitch before the row count
  refused("stft hop before lead", INVALID, "stft: hop 0", call(IN, OUT, 1, 2000, 2000, 0, 1024, ZERO, 4, 513, 2052));
  refused("stft pitch before rows", INVALID, "in_pitch 7 below in_length 8", call(IN, OUT, P31, 8, 7, 1, 0, ZERO, 1, 513, 513));
  refused("stft overlap before rows", INVALID, "byte ranges overlap", call(IN, IN, P31, 8, 8, 1, 0, ZERO, 1, 513, 513));
}

static void test_istft() {
  const verb_facts p = facts(1024, 4, true, 0, 4);  // fp32, N = 1024 (513 bins), 4 rows per work-group, 256 resident
  const int PLAIN = PFFT_ISTFT_PLAIN, NORM = PFFT_ISTFT_NORMALIZE;
  auto call_p = [](const verb_facts& q, uintptr_t in, uintptr_t out, ull ns, ull nf, ull fp, ull ip, ull hop, ull lead, int mode, ull ol,
                   ull op, ull chunk) {
    return [=] { return istft_geometry_of(q, in, out, ns, nf, fp, ip, hop, lead, mode, ol, op, chunk); };
  };
  auto call = [&](uintptr_t in, uintptr_t out, ull ns, ull nf, ull fp, ull ip, ull hop, ull lead, int mode, ull ol, ull op, ull chunk) {
    return call_p(p, in, out, ns, nf, fp, ip, hop, lead, mode, ol, op, chunk);
  };
  // the base call: 4 frames at hop 256 cover 3 * 256 + 1024 = 1792 samples
  admitted("istft base", call(IN, OUT, 1, 4, 513, 2052, 256, 0, PLAIN, 1792, 1792, 0));
  // refusals, in the order of the checks
  refused("istft null in", INVALID, "istft: null data pointer", call(0, OUT, 1, 4, 513, 2052, 256, 0, PLAIN, 1792, 1792, 0));
  refused("istft null out", INVALID, "istft: null data pointer", call(IN, 0, 1, 4, 513, 2052, 256, 0, PLAIN, 1792, 1792, 0));
  refused("istft no signals", INVALID, "istft: zero count (0 signals", call(IN, OUT, 0, 4, 513, 2052, 256, 0, PLAIN, 1792, 1792, 0));
  refused("istft no frames", INVALID, "1 signals, 0 frames", call(IN, OUT, 1, 0, 513, 2052, 256, 0, PLAIN, 1792, 1792, 0));
  refused("istft no output", INVALID, "out_length 0)", call(IN, OUT, 1, 4, 513, 2052, 256, 0, PLAIN, 0, 1792, 0));
  refused("istft hop 0", INVALID, "istft: hop 0", call(IN, OUT, 1, 4, 513, 2052, 0, 0, PLAIN, 1792, 1792, 0));
  refused("istft hop above N", INVALID, "hop 1025 above the frame length 1024", call(IN, OUT, 1, 4, 513, 2052, 1025, 0, PLAIN, 1792, 1792, 0));
  refused("istft lead", INVALID, "lead 1024 must be below the frame length 1024", call(IN, OUT, 1, 4, 513, 2052, 256, 1024, PLAIN, 1792, 1792, 0));
  refused("istft mode", INVALID, "Invalid istft mode 2", call(IN, OUT, 1, 4, 513, 2052, 256, 0, 2, 1792, 1792, 0));
  refused("istft frame_pitch", INVALID, "frame_pitch 512 below the 513 bins", call(IN, OUT, 1, 4, 512, 2052, 256, 0, PLAIN, 1792, 1792, 0));
  refused("istft 2^32 signals", UNSUPPORTED, "counts, lengths and pitches below 2^32", call(IN, OUT, P32, 4, 513, 2052, 256, 0, PLAIN, 1792, 1792, 0));
  refused("istft 2^32 frames", UNSUPPORTED, "counts, lengths and pitches below 2^32", call(IN, OUT, 1, P32, 513, 2052, 256, 0, PLAIN, 1792, 1792, 0));
  refused("istft out_length 2^32", UNSUPPORTED, "counts, lengths and pitches below 2^32", call(IN, OUT, 1, 4, 513, 2052, 256, 0, PLAIN, P32, P32, 0));
  refused("istft in_pitch 2^32", UNSUPPORTED, "counts, lengths and pitches below 2^32", call(IN, OUT, 1, 4, 513, P32, 256, 0, PLAIN, 1792, 1792, 0));
  refused("istft frame_pitch 2^32", UNSUPPORTED, "counts, lengths and pitches below 2^32", call(IN, OUT, 1, 4, P32, 2052, 256, 0, PLAIN, 1792, 1792, 0));
  refused("istft out_pitch 2^32", UNSUPPORTED, "counts, lengths and pitches below 2^32", call(IN, OUT, 1, 4, 513, 2052, 256, 0, PLAIN, 1792, P32, 0));
  refused("istft in_pitch", INVALID, "in_pitch 2051 below n_frames * frame_pitch = 2052", call(IN, OUT, 2, 4, 513, 2051, 256, 0, PLAIN, 1792, 1792, 0));
  refused("istft out_pitch", INVALID, "out_pitch 1791 below out_length 1792", call(IN, OUT, 2, 4, 513, 2052, 256, 0, PLAIN, 1792, 1791, 0));
  refused("istft uncovered samples", INVALID, "out_length 1793 above (n_frames - 1) * hop + N - lead = 1792", call(IN, OUT, 1, 4, 513, 2052, 256, 0, PLAIN, 1793, 1793, 0));
  refused("istft uncovered samples, lead", INVALID, "out_length 1281 above (n_frames - 1) * hop + N - lead = 1280", call(IN, OUT, 1, 4, 513, 2052, 256, 512, NORM, 1281, 1281, 0));
  // frame 3 starts at 768 - lead: 768 samples + lead 0 get nothing of it, 769 do
  refused("istft idle frame", INVALID, "frame 3 starts at sample 768 - lead 0, beyond the out_length 768", call(IN, OUT, 1, 4, 513, 2052, 256, 0, PLAIN, 768, 768, 0));
  admitted("istft one sample of the last frame", call(IN, OUT, 1, 4, 513, 2052, 256, 0, PLAIN, 769, 769, 0));
  // 2 signals: (2052 + 3 * 513 + 513) * 8 = 32832 bytes in, (1792 + 1792) * 4 = 14336 bytes out
  refused("istft in place", INVALID, "byte ranges overlap; the transform cannot run in place (a chunk reads", call(IN, IN, 2, 4, 513, 2052, 256, 0, PLAIN, 1792, 1792, 0));
  refused("istft partial overlap", INVALID, "byte ranges overlap", call(IN, IN + 32831, 2, 4, 513, 2052, 256, 0, PLAIN, 1792, 1792, 0));
  admitted("istft adjacent", call(IN, IN + 32832, 2, 4, 513, 2052, 256, 0, PLAIN, 1792, 1792, 0));
  refused("istft partial overlap, out first", INVALID, "byte ranges overlap", call(IN + 14335, IN, 2, 4, 513, 2052, 256, 0, PLAIN, 1792, 1792, 0));
  admitted("istft adjacent, out first", call(IN + 14336, IN, 2, 4, 513, 2052, 256, 0, PLAIN, 1792, 1792, 0));
  // rows: 2^31 - 1 signals of one frame admitted, 2^31 refused
  const istft_geometry rows = admitted("istft 2^31 - 1 rows", call(IN, OUT, P31 - 1, 1, 513, 513, 1024, 0, PLAIN, 1024, 1024, 1));
  CHECK_EQ("istft 2^31 - 1 rows", rows.groups, 2147483647ll);  // one chunk per signal
  CHECK_EQ("istft 2^31 - 1 rows", rows.chunk, 1);
  refused("istft 2^31 rows", UNSUPPORTED, "2147483648 signals of 1 frames each", call(IN, OUT, P31, 1, 513, 513, 1024, 0, PLAIN, 1024, 1024, 1));
  // reach_in at chunk_frames 8, hop 256 (halo 3), 12 frames: a group runs min(12, 3 + 8) = 11 frames:
  // (10 * frame_pitch + 513) * 8 <= 2^32 - 1, 10 * frame_pitch <= 536870398, frame_pitch <= 53687039
  admitted("istft reach_in", call(IN, OUT, 1, 12, 53687039, 12ull * 53687039, 256, 0, PLAIN, 3840, 3840, 8));
  refused("istft reach_in", UNSUPPORTED, "the 11 frames one work-group runs span 4294967304 bytes", call(IN, OUT, 1, 12, 53687040, 12ull * 53687040, 256, 0, PLAIN, 3840, 3840, 8));
  // ... a smaller chunk shortens it: chunk_frames 4 runs 7 frames
  admitted("istft reach_in, smaller chunk", call(IN, OUT, 1, 12, 53687040, 12ull * 53687040, 256, 0, PLAIN, 3840, 3840, 4));
  // reach_out: (min(out_length, chunk * hop + N) + (halo + fpw) * hop + N + lead) * 4 <= 2^32 - 1.  The bins of a frame
  // take more bytes than its hop, so at the fpw of a real kernel reach_in trips first; the term is reached through fpw:
  // hop 1024 (halo 0), 4 frames in one chunk, fpw 1048571: out_length + 1048571 * 1024 + 1024 + lead <= 1073741823,
  // out_length + lead <= 4095
  const verb_facts wide = facts(1024, 4, true, 0, 1048571);
  admitted("istft reach_out", call_p(wide, IN, OUT, 1, 4, 513, 2052, 1024, 0, PLAIN, 4095, 4095, 4));
  refused("istft reach_out", UNSUPPORTED, "the samples it covers 4294967296;", call_p(wide, IN, OUT, 1, 4, 513, 2052, 1024, 0, PLAIN, 4096, 4096, 4));
  admitted("istft reach_out, lead", call_p(wide, IN, OUT, 1, 4, 513, 2052, 1024, 95, PLAIN, 4000, 4000, 4));
  refused("istft reach_out, lead", UNSUPPORTED, "the samples it covers 4294967296;", call_p(wide, IN, OUT, 1, 4, 513, 2052, 1024, 96, PLAIN, 4000, 4000, 4));
  // ... chunk_frames 2 caps the first term at 2 * 1024 + 1024 = 3072
  admitted("istft reach_out, smaller chunk", call_p(wide, IN, OUT, 1, 4, 513, 2052, 1024, 0, PLAIN, 4096, 4096, 2));
  // the default chunk: 1 signal, 1000 frames, halo 3, fpw 4, 256 resident: 512 chunks wanted, ceil(1000 / 512) = 2 frames,
  // at least max(4 * 3, 4) = 12, a multiple of 4: 12
  CHECK_EQ("default chunk", istft_default_chunk(1, 1000, 3, 4, 256), 12);
  // 64 signals: 8 chunks each wanted, ceil(1000 / 8) = 125, rounded up to 128
  CHECK_EQ("default chunk, 64 signals", istft_default_chunk(64, 1000, 3, 4, 256), 128);
  // never beyond the signal: 5 frames, at least 12 -> 5
  CHECK_EQ("default chunk, short signal", istft_default_chunk(1, 5, 3, 4, 256), 5);
  // halo 0 (hop = N), fpw 4, 1000 resident, 1 signal of 10000 frames: 2000 chunks wanted, 5 frames -> 8
  CHECK_EQ("default chunk, no halo", istft_default_chunk(1, 10000, 0, 4, 1000), 8);
  // ... through the call: 999 * 256 + 1024 = 256768 samples; ceil(1000 / 12) = 84 groups
  const istft_geometry g = admitted("istft 1 x 1000", call(IN, OUT, 1, 1000, 513, 513000, 256, 0, NORM, 256768, 256768, 0));
  CHECK_EQ("istft 1 x 1000", g.n_signals, 1);
  CHECK_EQ("istft 1 x 1000", g.n_frames, 1000);
  CHECK_EQ("istft 1 x 1000", g.lead, 0);
  CHECK_EQ("istft 1 x 1000", g.hop, 256);
  CHECK_EQ("istft 1 x 1000", g.out_length, 256768);
  CHECK_EQ("istft 1 x 1000", g.frame_pitch, 513);
  CHECK_EQ("istft 1 x 1000", g.in_pitch, 513000);
  CHECK_EQ("istft 1 x 1000", g.out_pitch, 256768);
  CHECK_EQ("istft 1 x 1000", g.chunk, 12);
  CHECK_EQ("istft 1 x 1000", g.groups, 84);
  // the resident capacity is the mode's: 16 resident for NORMALIZE: 32 chunks wanted, ceil(1000 / 32) = 32 frames
  verb_facts two = p;
  two.resident[NORM] = 16;
  CHECK_EQ("istft resident by mode, plain", admitted("istft resident by mode", call_p(two, IN, OUT, 1, 1000, 513, 513000, 256, 0, PLAIN, 256768, 256768, 0)).chunk, 12);
  CHECK_EQ("istft resident by mode, normalize", admitted("istft resident by mode", call_p(two, IN, OUT, 1, 1000, 513, 513000, 256, 0, NORM, 256768, 256768, 0)).chunk, 32);
  // a given chunk: at most the frames; 3 signals of 10 frames in chunks of 4: 3 * 3 groups
  const istft_geometry h = admitted("istft 3 x 10", call(IN, OUT, 3, 10, 520, 5300, 256, 512, PLAIN, 2816, 3000, 4));
  CHECK_EQ("istft 3 x 10", h.chunk, 4);
  CHECK_EQ("istft 3 x 10", h.groups, 9);
  CHECK_EQ("istft 3 x 10", h.lead, 512);
  CHECK_EQ("istft 3 x 10", h.out_pitch, 3000);
  CHECK_EQ("istft 3 x 10", h.in_pitch, 5300);
  CHECK_EQ("istft 3 x 10", h.frame_pitch, 520);
  CHECK_EQ("istft chunk above the frames", admitted("istft chunk above the frames", call(IN, OUT, 3, 10, 520, 5300, 256, 512, PLAIN, 2816, 3000, 99)).chunk, 10);
  // two rules broken: the hop before the mode, the pitch before the overlap, the overlap before the row count
  refused("istft hop before mode", INVALID, "above the frame length", call(IN, OUT, 1, 4, 513, 2052, 1025, 0, 2, 1792, 1792, 0));
  refused("istft pitch before overlap", INVALID, "out_pitch 1791 below", call(IN, IN, 2, 4, 513, 2052, 256, 0, PLAIN, 1792, 1791, 0));
  refused("istft overlap before rows", INVALID, "byte ranges overlap", call(IN, IN, P31, 1, 513, 513, 1024, 0, PLAIN, 1024, 1024, 1));
}

int main() {
  test_overlap();
  test_dct();
  test_filter();
  test_stft();
  test_istft();
  if (failures != 0) {
    std::printf("verb geometry: %d of %d checks FAILED\n", failures, cases);
    return 1;
  }
  std::printf("verb geometry OK (%d checks)\n", cases);
  return 0;
}
