// The call-geometry rules of dct4 and mdct (portfft_amd/csrc/verb_geometry.hpp: dct4_geometry_of, mdct_geometry_of) on the
// CPU: every refusal with its status and text, the order of the checks through calls that break two rules, every 32-bit
// boundary as the pair (largest admitted value, that value + 1), and the kernel arguments of admitted calls against
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

static verb_facts facts(ull n, ull sb, ull fpw) {
  verb_facts p;
  p.n = n;
  p.sb = sb;
  p.real = true;
  p.fpw = fpw;
  return p;
}

static void test_dct4() {
  const verb_facts p = facts(64, 4, 4);  // fp32, N = 64, 4 rows per work-group
  auto call = [&](uintptr_t in, uintptr_t out, ull rows, ull ip, ull op) {
    return [=] { return dct4_geometry_of(p, in, out, rows, ip, op); };
  };
  // refusals, in the order of the checks
  refused("dct4 null in", INVALID, "dct4: null data pointer", call(0, OUT, 1, 64, 64));
  refused("dct4 null out", INVALID, "dct4: null data pointer", call(IN, 0, 1, 64, 64));
  refused("dct4 no rows", INVALID, "dct4: zero count (n_rows 0)", call(IN, OUT, 0, 64, 64));
  refused("dct4 in_pitch", INVALID, "dct4: in_pitch 63 below the row length 64", call(IN, OUT, 1, 63, 64));
  refused("dct4 out_pitch", INVALID, "dct4: out_pitch 63 below the row length 64", call(IN, OUT, 1, 64, 63));
  refused("dct4 in_pitch 2^32", UNSUPPORTED, "row slots of one work-group span", call(IN, OUT, 1, P32, 64));
  refused("dct4 out_pitch 2^32", UNSUPPORTED, "row slots of one work-group span", call(IN, OUT, 1, 64, P32));
  // the order, by calls that break two rules: the earlier one answers
  refused("dct4 null before no rows", INVALID, "null data pointer", call(0, OUT, 0, 64, 64));
  refused("dct4 no rows before pitch", INVALID, "zero count", call(IN, OUT, 0, 63, 64));
  refused("dct4 in_pitch before out_pitch", INVALID, "in_pitch 63", call(IN, OUT, 1, 63, 62));
  refused("dct4 pitch before rows", INVALID, "out_pitch 63", call(IN, OUT, P31, 64, 63));
  refused("dct4 rows before reach", UNSUPPORTED, "at most 2^31 - 1 rows", call(IN, OUT, P31, 268435456, 64));
  refused("dct4 reach before in place", UNSUPPORTED, "4 GiB", call(IN, IN, 1, 268435456, 64));
  refused("dct4 pitches before overlap", INVALID, "needs equal pitches", call(IN, IN, 9, 72, 80));
  // fpw * pitch * sb <= 2^32 - 1 with fpw = 4, sb = 4: pitch <= floor(4294967295 / 16) = 268435455, whatever n_rows is
  for (ull rows : {1ull, 2ull, 4ull, 9ull}) {
    admitted("dct4 in_pitch 268435455", call(IN, OUT, rows, 268435455, 64));
    refused("dct4 in_pitch 268435456", UNSUPPORTED, "the 4 row slots of one work-group span 4294967296 bytes of the input",
            call(IN, OUT, rows, 268435456, 64));
    admitted("dct4 out_pitch 268435455", call(IN, OUT, rows, 64, 268435455));
    refused("dct4 out_pitch 268435456", UNSUPPORTED, "and 4294967296 of the output", call(IN, OUT, rows, 64, 268435456));
  }
  // fp64, 2 rows per work-group: pitch <= floor(4294967295 / 16) = 268435455 as well
  {
    const verb_facts q = facts(128, 8, 2);
    admitted("dct4 f64 pitch", [=] { return dct4_geometry_of(q, IN, OUT, 1, 268435455, 128); });
    refused("dct4 f64 pitch + 1", UNSUPPORTED, "the 2 row slots", [=] { return dct4_geometry_of(q, IN, OUT, 1, 268435456, 128); });
  }
  // rows: 2^31 - 1 admitted -- ceil((2^31 - 1) / 4) = 2^29 groups --, 2^31 refused
  const dct4_geometry top = admitted("dct4 2^31 - 1 rows", call(IN, OUT, P31 - 1, 64, 64));
  CHECK_EQ("dct4 2^31 - 1 rows", top.n_rows, 2147483647ll);
  CHECK_EQ("dct4 2^31 - 1 rows", top.groups, 536870912ll);
  refused("dct4 2^31 rows", UNSUPPORTED, "2147483648 rows: at most 2^31 - 1 rows per call", call(IN, OUT, P31, 64, 64));
  // overlap: identical with equal pitches is in place; identical with unequal pitches and partial overlap are refused
  const dct4_geometry inplace = admitted("dct4 in place", call(IN, IN, 9, 72, 72));
  CHECK_EQ("dct4 in place", inplace.groups, 3);  // ceil(9 / 4)
  CHECK_EQ("dct4 in place", inplace.in_pitch, 72);
  CHECK_EQ("dct4 in place", inplace.out_pitch, 72);
  refused("dct4 in place, unequal pitches", INVALID, "needs equal pitches, not in_pitch 72 and out_pitch 80", call(IN, IN, 9, 72, 80));
  // 9 rows at pitch 72: (8 * 72 + 64) * 4 = 2560 bytes
  refused("dct4 partial overlap", INVALID, "overlap without being identical", call(IN, IN + 2559, 9, 72, 72));
  refused("dct4 partial overlap, out first", INVALID, "overlap without being identical", call(IN + 2559, IN, 9, 72, 72));
  const dct4_geometry disjoint = admitted("dct4 disjoint", call(IN, IN + 2560, 9, 72, 72));
  CHECK_EQ("dct4 disjoint", disjoint.n_rows, 9);
  CHECK_EQ("dct4 disjoint", disjoint.groups, 3);
  admitted("dct4 disjoint, out first", call(IN + 2560, IN, 9, 72, 72));
  const dct4_geometry g = admitted("dct4 5 rows", call(IN, OUT, 5, 67, 71));
  CHECK_EQ("dct4 5 rows", g.n_rows, 5);
  CHECK_EQ("dct4 5 rows", g.in_pitch, 67);
  CHECK_EQ("dct4 5 rows", g.out_pitch, 71);
  CHECK_EQ("dct4 5 rows", g.groups, 2);
}

static void test_mdct() {
  const verb_facts p = facts(1024, 4, 4);  // fp32, N = 1024: frames of 2048 samples at hop 1024, 4 rows per work-group
  auto call = [&](uintptr_t in, uintptr_t out, ull ns, ull il, ull ip, ull lead, ull nf, ull fp, ull op) {
    return [=] { return mdct_geometry_of(p, in, out, ns, il, ip, lead, nf, fp, op); };
  };
  // refusals, in the order of the checks
  refused("mdct null in", INVALID, "mdct: null data pointer", call(0, OUT, 1, 3000, 3000, 1024, 4, 1024, 4096));
  refused("mdct null out", INVALID, "mdct: null data pointer", call(IN, 0, 1, 3000, 3000, 1024, 4, 1024, 4096));
  refused("mdct no signals", INVALID, "mdct: zero count (0 signals", call(IN, OUT, 0, 3000, 3000, 1024, 4, 1024, 4096));
  refused("mdct no input", INVALID, "in_length 0, 4 frames)", call(IN, OUT, 1, 0, 3000, 1024, 4, 1024, 4096));
  refused("mdct no frames", INVALID, "in_length 3000, 0 frames)", call(IN, OUT, 1, 3000, 3000, 1024, 0, 1024, 4096));
  refused("mdct lead 2N", INVALID, "lead 2048 must be below the frame length 2048", call(IN, OUT, 1, 3000, 3000, 2048, 4, 1024, 4096));
  admitted("mdct lead 2N - 1", call(IN, OUT, 1, 3000, 3000, 2047, 4, 1024, 4096));
  refused("mdct in_pitch", INVALID, "in_pitch 2999 below in_length 3000", call(IN, OUT, 2, 3000, 2999, 1024, 4, 1024, 4096));
  refused("mdct frame_pitch", INVALID, "frame_pitch 1023 below the 1024 coefficients", call(IN, OUT, 1, 3000, 3000, 1024, 4, 1023, 4096));
  refused("mdct 2^32 signals", UNSUPPORTED, "counts, lengths and pitches below 2^32", call(IN, OUT, P32, 3000, 3000, 1024, 4, 1024, 4096));
  refused("mdct 2^32 frames", UNSUPPORTED, "counts, lengths and pitches below 2^32", call(IN, OUT, 1, 3000, 3000, 1024, P32, 1024, 4096));
  refused("mdct in_length 2^32", UNSUPPORTED, "counts, lengths and pitches below 2^32", call(IN, OUT, 1, P32, P32, 1024, 4, 1024, 4096));
  refused("mdct in_pitch 2^32", UNSUPPORTED, "counts, lengths and pitches below 2^32", call(IN, OUT, 1, 3000, P32, 1024, 4, 1024, 4096));
  refused("mdct frame_pitch 2^32", UNSUPPORTED, "counts, lengths and pitches below 2^32", call(IN, OUT, 1, 3000, 3000, 1024, 4, P32, 4096));
  refused("mdct out_pitch 2^32", UNSUPPORTED, "counts, lengths and pitches below 2^32", call(IN, OUT, 1, 3000, 3000, 1024, 4, 1024, P32));
  admitted("mdct in_pitch 2^32 - 1, one signal", call(IN, OUT, 1, 3000, P32 - 1, 1024, 4, 1024, 4096));
  refused("mdct out_pitch", INVALID, "out_pitch 4095 below n_frames * frame_pitch = 4096", call(IN, OUT, 2, 3000, 3000, 1024, 4, 1024, 4095));
  // frame 3 starts at 3 * 1024 = 3072 - lead; in_length + lead = 3072 leaves it empty, 3073 gives it one sample
  refused("mdct empty frame", INVALID, "frame 3 starts at sample 3072 - lead 1024, beyond the in_length 2048",
          call(IN, OUT, 1, 2048, 2048, 1024, 4, 1024, 4096));
  admitted("mdct one sample in the last frame", call(IN, OUT, 1, 2049, 2049, 1024, 4, 1024, 4096));
  refused("mdct empty frame, lead 0", INVALID, "frame 3 starts at sample 3072 - lead 0", call(IN, OUT, 1, 3072, 3072, 0, 4, 1024, 4096));
  admitted("mdct one sample, lead 0", call(IN, OUT, 1, 3073, 3073, 0, 4, 1024, 4096));
  // 2 signals of 3000 scalars: (3000 + 3000) * 4 = 24000 bytes in; (4096 + 3 * 1024 + 1024) * 4 = 32768 bytes out
  refused("mdct in place", INVALID, "byte ranges overlap; the transform cannot run in place (overlapping frames",
          call(IN, IN, 2, 3000, 3000, 1024, 4, 1024, 4096));
  refused("mdct partial overlap", INVALID, "byte ranges overlap", call(IN, IN + 23999, 2, 3000, 3000, 1024, 4, 1024, 4096));
  admitted("mdct adjacent", call(IN, IN + 24000, 2, 3000, 3000, 1024, 4, 1024, 4096));
  refused("mdct partial overlap, out first", INVALID, "byte ranges overlap", call(IN + 32767, IN, 2, 3000, 3000, 1024, 4, 1024, 4096));
  admitted("mdct adjacent, out first", call(IN + 32768, IN, 2, 3000, 3000, 1024, 4, 1024, 4096));
  // the order, by calls that break two rules: the earlier one answers
  refused("mdct null before zero count", INVALID, "null data pointer", call(0, OUT, 0, 3000, 3000, 1024, 4, 1024, 4096));
  refused("mdct zero count before lead", INVALID, "zero count", call(IN, OUT, 1, 3000, 3000, 2048, 0, 1024, 4096));
  refused("mdct lead before in_pitch", INVALID, "lead 2048", call(IN, OUT, 1, 3000, 2999, 2048, 4, 1024, 4096));
  refused("mdct in_pitch before frame_pitch", INVALID, "in_pitch 2999", call(IN, OUT, 1, 3000, 2999, 1024, 4, 1023, 4096));
  refused("mdct frame_pitch before 2^32", INVALID, "frame_pitch 1023", call(IN, OUT, P32, 3000, 3000, 1024, 4, 1023, 4096));
  refused("mdct 2^32 before out_pitch", UNSUPPORTED, "below 2^32", call(IN, OUT, P32, 3000, 3000, 1024, 4, 1024, 4095));
  refused("mdct out_pitch before the last frame", INVALID, "out_pitch 4095", call(IN, OUT, 1, 2048, 2048, 1024, 4, 1024, 4095));
  refused("mdct last frame before overlap", INVALID, "at least one sample", call(IN, IN, 1, 2048, 2048, 1024, 4, 1024, 4096));
  refused("mdct overlap before the row count", INVALID, "cannot run in place", call(IN, IN, P31, 8, 8, 0, 1, 1024, 1024));
  refused("mdct row count before the reach", UNSUPPORTED, "2147483648 signals of 1 frames each",
          call(OUT, IN, P31, 8, 1073740798, 0, 1, 1024, 1024));  // (the input behind the output: its 2^63 bytes reach upwards)
  // rows: 2^31 - 1 signals of one frame admitted -- 2^29 groups --, 2^31 refused
  const mdct_geometry rows = admitted("mdct 2^31 - 1 rows", call(IN, OUT, P31 - 1, 8, 8, 0, 1, 1024, 1024));
  CHECK_EQ("mdct 2^31 - 1 rows", rows.groups, 536870912ll);
  refused("mdct 2^31 rows", UNSUPPORTED, "2147483648 signals of 1 frames each", call(IN, OUT, P31, 8, 8, 0, 1, 1024, 1024));
  refused("mdct 2^16 x 2^15 rows", UNSUPPORTED, "65536 signals of 32768 frames each",
          call(IN, OUT, 1ull << 16, 1ull << 25, 1ull << 25, 0, 1ull << 15, 1024, 1024ull << 15));
  // reach_in, one signal (cross = 0): (in_length + lead + 2048 + 1) * 4 <= 2^32 - 1, in_length + lead <= 1073739774
  admitted("mdct reach_in, 1 signal", call(IN, OUT, 1, 1073739774, 1073739774, 0, 1, 1024, 1024));
  refused("mdct reach_in, 1 signal", UNSUPPORTED, "the 1 consecutive signals the rows of one work-group touch span 4294967296 bytes",
          call(IN, OUT, 1, 1073739775, 1073739775, 0, 1, 1024, 1024));
  admitted("mdct reach_in, 1 signal, lead 2047", call(IN, OUT, 1, 1073737727, 1073737727, 2047, 1, 1024, 1024));
  refused("mdct reach_in, 1 signal, lead 2047", UNSUPPORTED, "span 4294967296 bytes",
          call(IN, OUT, 1, 1073737728, 1073737728, 2047, 1, 1024, 1024));
  // reach_out, one signal of 4 frames: (3 * frame_pitch + 1024) * 4 <= 2^32 - 1, 3 * frame_pitch <= 1073740799,
  // frame_pitch <= 357913599
  admitted("mdct reach_out, 1 signal", call(IN, OUT, 1, 3000, 3000, 1024, 4, 357913599, 4ull * 357913599));
  refused("mdct reach_out, 1 signal", UNSUPPORTED, "their output rows 4294967296;",
          call(IN, OUT, 1, 3000, 3000, 1024, 4, 357913600, 4ull * 357913600));
  // 9 signals of 1 frame: the 4 rows of a group cross min(8, ceil(3 / 1)) = 3 signal boundaries
  //   in: (3 * in_pitch + 2000 + 0 + 2049) * 4 <= 2^32 - 1, 3 * in_pitch <= 1073737774, in_pitch <= 357912591
  //   (the next pitch: (3 * 357912592 + 4049) * 4 = 4294967300)
  admitted("mdct reach_in, 1 frame", call(IN, OUT, 9, 2000, 357912591, 0, 1, 1024, 1024));
  refused("mdct reach_in, 1 frame", UNSUPPORTED, "the 4 consecutive signals the rows of one work-group touch span 4294967300 bytes",
          call(IN, OUT, 9, 2000, 357912592, 0, 1, 1024, 1024));
  //   out: (3 * out_pitch + 1024) * 4 <= 2^32 - 1, out_pitch <= 357913599
  admitted("mdct reach_out, 1 frame", call(IN, OUT, 9, 2000, 2000, 0, 1, 1024, 357913599));
  refused("mdct reach_out, 1 frame", UNSUPPORTED, "the 4 consecutive signals", call(IN, OUT, 9, 2000, 2000, 0, 1, 1024, 357913600));
  // 9 signals of 3 frames: min(8, ceil(3 / 3)) = 1 boundary
  //   in: (in_pitch + 2000 + 1024 + 2049) * 4 <= 2^32 - 1, in_pitch <= 1073741823 - 5073 = 1073736750
  admitted("mdct reach_in, 3 frames", call(IN, OUT, 9, 2000, 1073736750, 1024, 3, 1030, 3090));
  refused("mdct reach_in, 3 frames", UNSUPPORTED, "the 2 consecutive signals the rows of one work-group touch span 4294967296 bytes",
          call(IN, OUT, 9, 2000, 1073736751, 1024, 3, 1030, 3090));
  //   out: (out_pitch + 2 * 1030 + 1024) * 4 <= 2^32 - 1, out_pitch <= 1073741823 - 3084 = 1073738739
  admitted("mdct reach_out, 3 frames", call(IN, OUT, 9, 2000, 2000, 1024, 3, 1030, 1073738739));
  refused("mdct reach_out, 3 frames", UNSUPPORTED, "the 2 consecutive signals", call(IN, OUT, 9, 2000, 2000, 1024, 3, 1030, 1073738740));
  // admitted calls: the arguments pass through, groups = ceil(signals * frames / 4)
  const mdct_geometry g = admitted("mdct 3 x 7", call(IN, OUT, 3, 6000, 6100, 1023, 7, 1030, 7300));
  CHECK_EQ("mdct 3 x 7", g.n_signals, 3);
  CHECK_EQ("mdct 3 x 7", g.n_frames, 7);
  CHECK_EQ("mdct 3 x 7", g.lead, 1023);
  CHECK_EQ("mdct 3 x 7", g.in_length, 6000);
  CHECK_EQ("mdct 3 x 7", g.in_pitch, 6100);
  CHECK_EQ("mdct 3 x 7", g.frame_pitch, 1030);
  CHECK_EQ("mdct 3 x 7", g.out_pitch, 7300);
  CHECK_EQ("mdct 3 x 7", g.groups, 6);  // ceil(21 / 4)
}

int main() {
  test_dct4();
  test_mdct();
  std::printf("%d checks, %d failures\n", cases, failures);
  std::printf(failures == 0 ? "dct4 geometry OK\n" : "dct4 geometry FAILED\n");
  return failures == 0 ? 0 : 1;
}
