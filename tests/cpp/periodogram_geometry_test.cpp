// The call-geometry rules of periodogram (portfft_amd/csrc/verb_geometry.hpp: periodogram_geometry_of) on the CPU: every
// refusal with its status and text, the order of the checks through calls that break two rules, every 32-bit boundary as
// the pair (largest admitted value, that value + 1), and the kernel arguments and `groups` of admitted calls against
// values worked out by hand (the derivation stands at each case).  Includes the header only; links nothing.
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
static const int Z = PFFT_PAD_ZERO, RF = PFFT_PAD_REFLECT;

int main() {
  verb_facts p;  // fp32, N = 1024: frames of 1024 samples, M + 1 = 513 bins, 4 units per work-group
  p.n = 1024;
  p.sb = 4;
  p.real = true;
  p.fpw = 4;
  auto call = [&](uintptr_t in, uintptr_t out, ull ns, ull len, ull ip, ull hop, ull lead, int pad, ull nf, ull avg, ull rp,
                  ull op) { return [=] { return periodogram_geometry_of(p, in, out, ns, len, ip, hop, lead, pad, nf, avg, rp, op); }; };
  // the base call: 2 signals of 5000 samples, hop 256, lead 512, 10 frames in rows of 3: R = 4 rows of pitch 513
  // refusals, in the order of the checks
  refused("null in", INVALID, "periodogram: null data pointer", call(0, OUT, 2, 5000, 5000, 256, 512, Z, 10, 3, 513, 2052));
  refused("null out", INVALID, "periodogram: null data pointer", call(IN, 0, 2, 5000, 5000, 256, 512, Z, 10, 3, 513, 2052));
  refused("no signals", INVALID, "periodogram: zero count (0 signals", call(IN, OUT, 0, 5000, 5000, 256, 512, Z, 10, 3, 513, 2052));
  refused("no samples", INVALID, "2 signals, in_length 0,", call(IN, OUT, 2, 0, 5000, 256, 512, Z, 10, 3, 513, 2052));
  refused("no frames", INVALID, ", 0 frames, avg_frames 3)", call(IN, OUT, 2, 5000, 5000, 256, 512, Z, 0, 3, 513, 2052));
  refused("no average", INVALID, "10 frames, avg_frames 0)", call(IN, OUT, 2, 5000, 5000, 256, 512, Z, 10, 0, 513, 2052));
  refused("hop 0", INVALID, "periodogram: hop 0", call(IN, OUT, 2, 5000, 5000, 0, 512, Z, 10, 3, 513, 2052));
  refused("lead N", INVALID, "lead 1024 must be below the frame length 1024", call(IN, OUT, 2, 5000, 5000, 256, 1024, Z, 10, 3, 513, 2052));
  admitted("lead N - 1", call(IN, OUT, 2, 5000, 5000, 256, 1023, Z, 10, 3, 513, 2052));
  refused("pad_mode", INVALID, "Invalid periodogram pad_mode 2", call(IN, OUT, 2, 5000, 5000, 256, 512, 2, 10, 3, 513, 2052));
  refused("avg above frames", INVALID, "avg_frames 11 above the 10 frames of a signal", call(IN, OUT, 2, 5000, 5000, 256, 512, Z, 10, 11, 513, 2052));
  admitted("avg = frames", call(IN, OUT, 2, 5000, 5000, 256, 512, Z, 10, 10, 513, 513));
  refused("in_pitch", INVALID, "in_pitch 4999 below in_length 5000", call(IN, OUT, 2, 5000, 4999, 256, 512, Z, 10, 3, 513, 2052));
  refused("row_pitch", INVALID, "row_pitch 512 below the 513 bins of a row", call(IN, OUT, 2, 5000, 5000, 256, 512, Z, 10, 3, 512, 2052));
  const char* k32 = "counts, lengths, hop and pitches below 2^32";
  refused("2^32 signals", UNSUPPORTED, k32, call(IN, OUT, P32, 5000, 5000, 256, 512, Z, 10, 3, 513, 2052));
  refused("2^32 frames", UNSUPPORTED, k32, call(IN, OUT, 2, 5000, 5000, 256, 512, Z, P32, 3, 513, 2052));
  refused("2^32 frames, all averaged", UNSUPPORTED, k32, call(IN, OUT, 2, 5000, 5000, 256, 512, Z, P32, P32, 513, 2052));
  refused("hop 2^32", UNSUPPORTED, k32, call(IN, OUT, 2, 5000, 5000, P32, 512, Z, 10, 3, 513, 2052));
  refused("in_length 2^32", UNSUPPORTED, k32, call(IN, OUT, 2, P32, P32, 256, 512, Z, 10, 3, 513, 2052));
  refused("in_pitch 2^32", UNSUPPORTED, k32, call(IN, OUT, 2, 5000, P32, 256, 512, Z, 10, 3, 513, 2052));
  refused("row_pitch 2^32", UNSUPPORTED, k32, call(IN, OUT, 2, 5000, 5000, 256, 512, Z, 10, 3, P32, 2052));
  refused("out_pitch 2^32", UNSUPPORTED, k32, call(IN, OUT, 2, 5000, 5000, 256, 512, Z, 10, 3, 513, P32));
  admitted("in_pitch and out_pitch 2^32 - 1, one signal", call(IN, OUT, 1, 5000, P32 - 1, 256, 512, Z, 10, 3, 513, P32 - 1));
  admitted("hop 2^32 - 1, one frame", call(IN, OUT, 2, 5000, 5000, P32 - 1, 512, Z, 1, 1, 513, 513));
  // R = ceil(10 / 3) = 4 rows of pitch 513: 2052
  refused("out_pitch", INVALID, "out_pitch 2051 below ceil(n_frames / avg_frames) * row_pitch = 2052",
          call(IN, OUT, 2, 5000, 5000, 256, 512, Z, 10, 3, 513, 2051));
  admitted("out_pitch of R rows", call(IN, OUT, 2, 5000, 5000, 256, 512, Z, 10, 3, 513, 2052));
  // zeros: frame 22 starts at 22 * 256 = 5632 >= 5000 + 512, frame 21 at 5376 < 5512
  refused("a frame without a sample", INVALID, "frame 22 starts at sample 5632 - lead 512, beyond the in_length 5000",
          call(IN, OUT, 2, 5000, 5000, 256, 512, Z, 23, 3, 513, 6000));
  admitted("one sample of the last frame", call(IN, OUT, 2, 5000, 5000, 256, 512, Z, 22, 3, 513, 6000));
  // reflection: lead <= in_length - 1, and the last frame ends inside the signal padded by lead: 20 * 250 + 1024 = 6024
  refused("reflected twice", INVALID, "lead 400 above in_length - 1 = 399", call(IN, OUT, 2, 400, 400, 256, 400, RF, 1, 1, 513, 513));
  admitted("lead = in_length - 1", call(IN, OUT, 2, 400, 400, 256, 399, RF, 1, 1, 513, 513));
  refused("beyond the reflection", INVALID, "frame 21 ends at sample 6274 - lead 512, beyond the signal of in_length 5000",
          call(IN, OUT, 2, 5000, 5000, 250, 512, RF, 22, 3, 513, 6000));
  admitted("ends with the reflection", call(IN, OUT, 2, 5000, 5000, 250, 512, RF, 21, 3, 513, 6000));
  // 2 signals: (5000 + 5000) * 4 = 40000 bytes in; (2052 + 3 * 513 + 513) * 4 = 16416 bytes out (scalars on both sides)
  refused("in place", INVALID, "byte ranges overlap; the verb cannot run in place (a row's sums",
          call(IN, IN, 2, 5000, 5000, 256, 512, Z, 10, 3, 513, 2052));
  refused("partial overlap", INVALID, "byte ranges overlap", call(IN, IN + 39999, 2, 5000, 5000, 256, 512, Z, 10, 3, 513, 2052));
  admitted("adjacent", call(IN, IN + 40000, 2, 5000, 5000, 256, 512, Z, 10, 3, 513, 2052));
  refused("partial overlap, out first", INVALID, "byte ranges overlap", call(IN + 16415, IN, 2, 5000, 5000, 256, 512, Z, 10, 3, 513, 2052));
  admitted("adjacent, out first", call(IN + 16416, IN, 2, 5000, 5000, 256, 512, Z, 10, 3, 513, 2052));
  // the order, by calls that break two rules: the earlier one answers
  refused("null before zero count", INVALID, "null data pointer", call(0, OUT, 0, 5000, 5000, 256, 512, Z, 10, 3, 513, 2052));
  refused("zero count before hop", INVALID, "zero count", call(IN, OUT, 2, 5000, 5000, 0, 512, Z, 0, 3, 513, 2052));
  refused("hop before lead", INVALID, "hop 0", call(IN, OUT, 2, 5000, 5000, 0, 1024, Z, 10, 3, 513, 2052));
  refused("lead before pad_mode", INVALID, "lead 1024", call(IN, OUT, 2, 5000, 5000, 256, 1024, 2, 10, 3, 513, 2052));
  refused("pad_mode before avg_frames", INVALID, "pad_mode 2", call(IN, OUT, 2, 5000, 5000, 256, 512, 2, 10, 11, 513, 2052));
  refused("avg_frames before in_pitch", INVALID, "avg_frames 11", call(IN, OUT, 2, 5000, 4999, 256, 512, Z, 10, 11, 513, 2052));
  refused("in_pitch before row_pitch", INVALID, "in_pitch 4999", call(IN, OUT, 2, 5000, 4999, 256, 512, Z, 10, 3, 512, 2052));
  refused("row_pitch before 2^32", INVALID, "row_pitch 512", call(IN, OUT, P32, 5000, 5000, 256, 512, Z, 10, 3, 512, 2052));
  refused("2^32 before out_pitch", UNSUPPORTED, "below 2^32", call(IN, OUT, P32, 5000, 5000, 256, 512, Z, 10, 3, 513, 2051));
  // 23 frames in rows of 3: R = 8, 8 * 513 = 4104
  refused("out_pitch before the frames", INVALID, "out_pitch 4103", call(IN, OUT, 2, 5000, 5000, 256, 512, Z, 23, 3, 513, 4103));
  refused("frames before overlap", INVALID, "at least one sample", call(IN, IN, 2, 5000, 5000, 256, 512, Z, 23, 3, 513, 6000));
  refused("reflection before overlap", INVALID, "reflected by lead on both sides", call(IN, IN, 2, 5000, 5000, 250, 512, RF, 22, 3, 513, 6000));
  refused("overlap before the unit count", INVALID, "cannot run in place", call(IN, IN, P31, 8, 8, 1, 0, Z, 1, 1, 513, 513));
  // 2^20 signals of 4096 frames in rows of 2: 2^31 units; at in_pitch 2^31 the signals a group crosses span far above
  // 4 GiB -- the unit count answers first (the output in front of the input: 2^20 * 2^31 * 4 bytes of signals)
  refused("unit count before the reach", UNSUPPORTED, "1048576 signals of 2048 rows each",
          call(OUT, IN, 1ull << 20, 5000, P31, 1, 0, Z, 4096, 2, 513, 1050624));
  // units: 2^31 - 1 signals of one row admitted, ceil((2^31 - 1) / 4) = 2^29 groups; 2^31 refused
  const periodogram_geometry units = admitted("2^31 - 1 units", call(IN, OUT, P31 - 1, 8, 8, 1, 0, Z, 1, 1, 513, 513));
  CHECK_EQ("2^31 - 1 units", units.groups, 536870912ll);
  refused("2^31 units", UNSUPPORTED, "2147483648 signals of 1 rows each", call(IN, OUT, P31, 8, 8, 1, 0, Z, 1, 1, 513, 513));
  // ... and through the rows: 2^20 signals of 4096 frames, rows of 2 -> 2048 rows each, 2^31 units; rows of 3 -> 1366
  // rows, 2^20 * 1366 = 1432354816 units, 358088704 groups
  refused("2^31 units by rows", UNSUPPORTED, "1048576 signals of 2048 rows each",
          call(IN, OUT, 1ull << 20, 5000, 5000, 1, 0, Z, 4096, 2, 513, 1050624));
  const periodogram_geometry by_rows = admitted("2^20 x 1366", call(IN, OUT, 1ull << 20, 5000, 5000, 1, 0, Z, 4096, 3, 513, 1050624));
  CHECK_EQ("2^20 x 1366", by_rows.groups, 358088704ll);
  // reach_in, one signal: (in_length + lead + 1024 + 1) * 4 <= 2^32 - 1, in_length + lead <= 1073740798
  admitted("reach_in, one signal", call(IN, OUT, 1, 1073740798, 1073740798, 1, 0, Z, 1, 1, 513, 513));
  refused("reach_in, one signal", UNSUPPORTED, "the 1 consecutive signals the units of one work-group touch span 4294967296 bytes",
          call(IN, OUT, 1, 1073740799, 1073740799, 1, 0, Z, 1, 1, 513, 513));
  refused("reach_in counts the lead", UNSUPPORTED, "span 4294967296 bytes", call(IN, OUT, 1, 1073740798, 1073740798, 1, 1, Z, 1, 1, 513, 513));
  // ... two signals, one row each: the 4 units of a group cross a boundary, (in_pitch + 1000 + 1025) * 4 <= 2^32 - 1
  admitted("reach_in, two signals", call(IN, OUT, 2, 1000, 1073739798, 256, 0, Z, 3, 3, 513, 513));
  refused("reach_in, two signals", UNSUPPORTED, "the 2 consecutive signals the units of one work-group touch span 4294967296 bytes",
          call(IN, OUT, 2, 1000, 1073739799, 256, 0, Z, 3, 3, 513, 513));
  // reach_out, one signal of 4 rows: (3 * row_pitch + 513) * 4 <= 2^32 - 1, row_pitch <= 357913770
  admitted("reach_out, 4 rows", call(IN, OUT, 1, 5000, 5000, 256, 512, Z, 10, 3, 357913770, 1431655080));
  refused("reach_out, 4 rows", UNSUPPORTED, "their output rows 4294967304;",
          call(IN, OUT, 1, 5000, 5000, 256, 512, Z, 10, 3, 357913771, 1431655084));
  // ... one row per signal (avg_frames = n_frames) has no second row to reach
  admitted("reach_out, one row", call(IN, OUT, 1, 5000, 5000, 256, 512, Z, 10, 10, 357913771, 1431655084));
  // ... two signals of one row: (out_pitch + 513) * 4 <= 2^32 - 1, out_pitch <= 1073741310
  admitted("reach_out, two signals", call(IN, OUT, 2, 5000, 5000, 256, 512, Z, 10, 10, 513, 1073741310));
  refused("reach_out, two signals", UNSUPPORTED, "their output rows 4294967296;",
          call(IN, OUT, 2, 5000, 5000, 256, 512, Z, 10, 10, 513, 1073741311));
  // admitted calls: the arguments pass through, groups = ceil(signals * R / 4)
  //   2 signals, 10 frames in rows of 3 (3 does not divide 10): R = 4, 8 units, 2 groups
  const periodogram_geometry base = admitted("2 x 10 / 3", call(IN, OUT, 2, 5000, 5001, 255, 511, RF, 10, 3, 515, 2100));
  CHECK_EQ("2 x 10 / 3", base.groups, 2);
  CHECK_EQ("2 x 10 / 3", base.n_signals, 2);
  CHECK_EQ("2 x 10 / 3", base.n_frames, 10);
  CHECK_EQ("2 x 10 / 3", base.avg_frames, 3);
  CHECK_EQ("2 x 10 / 3", base.lead, 511);
  CHECK_EQ("2 x 10 / 3", base.hop, 255);
  CHECK_EQ("2 x 10 / 3", base.in_length, 5000);
  CHECK_EQ("2 x 10 / 3", base.in_pitch, 5001);
  CHECK_EQ("2 x 10 / 3", base.row_pitch, 515);
  CHECK_EQ("2 x 10 / 3", base.out_pitch, 2100);
  //   avg_frames = n_frames: one row per signal, 2 units, 1 group
  const periodogram_geometry welch = admitted("2 x 10 / 10", call(IN, OUT, 2, 5000, 5001, 255, 511, Z, 10, 10, 515, 515));
  CHECK_EQ("2 x 10 / 10", welch.groups, 1);
  CHECK_EQ("2 x 10 / 10", welch.avg_frames, 10);
  //   3 signals of 7 frames: rows of 1 -> 21 units, 6 groups; of 2 -> R = 4, 12 units, 3 groups; of 3 -> R = 3, 9 units,
  //   3 groups; of 7 -> 3 units, 1 group
  CHECK_EQ("3 x 7 / 1", admitted("3 x 7 / 1", call(IN, OUT, 3, 5000, 5000, 256, 0, Z, 7, 1, 513, 3591)).groups, 6);
  CHECK_EQ("3 x 7 / 2", admitted("3 x 7 / 2", call(IN, OUT, 3, 5000, 5000, 256, 0, Z, 7, 2, 513, 2052)).groups, 3);
  CHECK_EQ("3 x 7 / 3", admitted("3 x 7 / 3", call(IN, OUT, 3, 5000, 5000, 256, 0, Z, 7, 3, 513, 1539)).groups, 3);
  CHECK_EQ("3 x 7 / 7", admitted("3 x 7 / 7", call(IN, OUT, 3, 5000, 5000, 256, 0, Z, 7, 7, 513, 513)).groups, 1);
  //   a kernel of one unit per work-group: as many groups as units
  p.fpw = 1;
  CHECK_EQ("fpw 1", admitted("fpw 1", call(IN, OUT, 3, 5000, 5000, 256, 0, Z, 7, 2, 513, 2052)).groups, 12);
  std::printf("%d checks, %d failures\n", cases, failures);
  std::printf(failures == 0 ? "periodogram geometry OK\n" : "periodogram geometry FAILED\n");
  return failures == 0 ? 0 : 1;
}
