// The call-geometry rules of convolve_pairs / correlate_pairs (portfft_amd/csrc/verb_geometry.hpp: pairs_geometry_of) on
// the CPU: every refusal with its status and text, in the order of the checks -- a call that breaks two rules gets the
// first one's message --, every 32-bit boundary as the pair (largest admitted value, that value + 1), and the kernel
// arguments and `groups` of admitted calls against values worked out by hand (the derivation stands at each case).
// Includes the header only; links nothing.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
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
// far apart: no geometry below makes two byte ranges meet unless a case moves them
static const uintptr_t X = uintptr_t(1) << 48, Y = uintptr_t(1) << 50, OUT = uintptr_t(1) << 52;
static const ull P31 = 1ull << 31, P32 = 1ull << 32;
static const int CONV = PFFT_CONVOLVE, CORR = PFFT_CORRELATE;

int main() {
  verb_facts p;  // fp32, N = 1024, 4 rows per work-group
  p.n = 1024;
  p.sb = 4;
  p.real = true;
  p.fpw = 4;
  auto call = [&](int mode, uintptr_t x, uintptr_t y, uintptr_t out, ull rows, ull xl, ull xp, ull yl, ull yp, ull ol, ull op,
                  double floor) { return [=] { return pairs_geometry_of(p, mode, x, y, out, rows, xl, xp, yl, yp, ol, op, floor); }; };
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  const double fmin = 1.17549435082228751e-38, fmax = 3.40282346638528860e38;
  // the base call: 3 rows, x of 1000 scalars at pitch 1030, y of 513 at pitch 515, out of 1024 at pitch 1100
  // ---- PFFT_INVALID_CONFIGURATION, in the order of the checks
  refused("null x", INVALID, "pairs: null data pointer", call(CORR, 0, Y, OUT, 3, 1000, 1030, 513, 515, 1024, 1100, 0));
  refused("null y", INVALID, "pairs: null data pointer", call(CORR, X, 0, OUT, 3, 1000, 1030, 513, 515, 1024, 1100, 0));
  refused("null out", INVALID, "pairs: null data pointer", call(CORR, X, Y, 0, 3, 1000, 1030, 513, 515, 1024, 1100, 0));
  refused("mode 2", INVALID, "pairs: mode 2 is neither", call(2, X, Y, OUT, 3, 1000, 1030, 513, 515, 1024, 1100, 0));
  refused("mode -1", INVALID, "pairs: mode -1 is neither", call(-1, X, Y, OUT, 3, 1000, 1030, 513, 515, 1024, 1100, 0));
  refused("no rows", INVALID, "pairs: zero count (n_rows 0)", call(CORR, X, Y, OUT, 0, 1000, 1030, 513, 515, 1024, 1100, 0));
  refused("x_length 0", INVALID, "lengths (x 0, y 513, out 1024) must be in 1 ... 1024", call(CORR, X, Y, OUT, 3, 0, 1030, 513, 515, 1024, 1100, 0));
  refused("y_length 0", INVALID, "lengths (x 1000, y 0, out 1024)", call(CORR, X, Y, OUT, 3, 1000, 1030, 0, 515, 1024, 1100, 0));
  refused("out_length 0", INVALID, "lengths (x 1000, y 513, out 0)", call(CORR, X, Y, OUT, 3, 1000, 1030, 513, 515, 0, 1100, 0));
  refused("x_length N + 1", INVALID, "lengths (x 1025, y 513, out 1024)", call(CORR, X, Y, OUT, 3, 1025, 1030, 513, 515, 1024, 1100, 0));
  refused("y_length N + 1", INVALID, "lengths (x 1000, y 1025, out 1024)", call(CORR, X, Y, OUT, 3, 1000, 1030, 1025, 1030, 1024, 1100, 0));
  refused("out_length N + 1", INVALID, "lengths (x 1000, y 513, out 1025)", call(CORR, X, Y, OUT, 3, 1000, 1030, 513, 515, 1025, 1100, 0));
  admitted("all lengths N", call(CORR, X, Y, OUT, 3, 1024, 1024, 1024, 1024, 1024, 1024, 0));
  admitted("all lengths 1", call(CORR, X, Y, OUT, 3, 1, 1, 1, 1, 1, 1, 0));
  refused("x_pitch", INVALID, "pitches (x 999, y 515, out 1100) below the lengths (1000, 513, 1024)",
          call(CORR, X, Y, OUT, 3, 1000, 999, 513, 515, 1024, 1100, 0));
  refused("y_pitch", INVALID, "pitches (x 1030, y 512, out 1100) below", call(CORR, X, Y, OUT, 3, 1000, 1030, 513, 512, 1024, 1100, 0));
  refused("out_pitch", INVALID, "pitches (x 1030, y 515, out 1023) below", call(CORR, X, Y, OUT, 3, 1000, 1030, 513, 515, 1024, 1023, 0));
  refused("a pitch below its length, one row", INVALID, "below the lengths", call(CORR, X, Y, OUT, 1, 1000, 999, 513, 515, 1024, 1100, 0));
  const char* fl = "must be 0 (no phase transform) or a positive normal number";
  refused("floor -1", INVALID, fl, call(CORR, X, Y, OUT, 3, 1000, 1030, 513, 515, 1024, 1100, -1.0));
  refused("floor -0 - tiny", INVALID, fl, call(CORR, X, Y, OUT, 3, 1000, 1030, 513, 515, 1024, 1100, -1e-300));
  refused("floor nan", INVALID, fl, call(CORR, X, Y, OUT, 3, 1000, 1030, 513, 515, 1024, 1100, nan));
  refused("floor inf", INVALID, fl, call(CORR, X, Y, OUT, 3, 1000, 1030, 513, 515, 1024, 1100, inf));
  refused("floor -inf", INVALID, fl, call(CORR, X, Y, OUT, 3, 1000, 1030, 513, 515, 1024, 1100, -inf));
  refused("floor 1e-50 in fp32", INVALID, fl, call(CORR, X, Y, OUT, 3, 1000, 1030, 513, 515, 1024, 1100, 1e-50));
  refused("floor subnormal in fp32", INVALID, fl, call(CORR, X, Y, OUT, 3, 1000, 1030, 513, 515, 1024, 1100, std::nextafter(fmin, 0.0)));
  admitted("floor FLT_MIN", call(CORR, X, Y, OUT, 3, 1000, 1030, 513, 515, 1024, 1100, fmin));
  admitted("floor FLT_MAX", call(CORR, X, Y, OUT, 3, 1000, 1030, 513, 515, 1024, 1100, fmax));
  refused("floor above FLT_MAX", INVALID, fl, call(CORR, X, Y, OUT, 3, 1000, 1030, 513, 515, 1024, 1100, std::nextafter(fmax, inf)));
  refused("floor with convolve", INVALID, "phat_floor 0.001 with PFFT_CONVOLVE", call(CONV, X, Y, OUT, 3, 1000, 1030, 513, 515, 1024, 1100, 1e-3));
  admitted("convolve without a floor", call(CONV, X, Y, OUT, 3, 1000, 1030, 513, 515, 1024, 1100, 0));
  // x: (2 * 1030 + 1000) * 4 = 12240 bytes, y: (2 * 515 + 513) * 4 = 6172, out: (2 * 1100 + 1024) * 4 = 12896
  const char* ov = "the output byte range overlaps an input's";
  refused("out == x", INVALID, ov, call(CORR, X, Y, X, 3, 1000, 1030, 513, 515, 1024, 1100, 0));
  refused("out == y", INVALID, ov, call(CORR, X, Y, Y, 3, 1000, 1030, 513, 515, 1024, 1100, 0));
  refused("out on the last byte of x", INVALID, ov, call(CORR, X, Y, X + 12239, 3, 1000, 1030, 513, 515, 1024, 1100, 0));
  admitted("out behind x", call(CORR, X, Y, X + 12240, 3, 1000, 1030, 513, 515, 1024, 1100, 0));
  refused("x on the last byte of out", INVALID, ov, call(CORR, OUT + 12895, Y, OUT, 3, 1000, 1030, 513, 515, 1024, 1100, 0));
  admitted("x behind out", call(CORR, OUT + 12896, Y, OUT, 3, 1000, 1030, 513, 515, 1024, 1100, 0));
  refused("out on the last byte of y", INVALID, ov, call(CORR, X, Y, Y + 6171, 3, 1000, 1030, 513, 515, 1024, 1100, 0));
  admitted("out behind y", call(CORR, X, Y, Y + 6172, 3, 1000, 1030, 513, 515, 1024, 1100, 0));
  refused("y on the last byte of out", INVALID, ov, call(CORR, X, OUT + 12895, OUT, 3, 1000, 1030, 513, 515, 1024, 1100, 0));
  admitted("y behind out", call(CORR, X, OUT + 12896, OUT, 3, 1000, 1030, 513, 515, 1024, 1100, 0));
  // x against y is never checked: the same rows (autocorrelation), and rows that overlap partly
  admitted("x == y", call(CORR, X, X, OUT, 3, 1000, 1030, 1000, 1030, 1024, 1100, 0));
  admitted("x and y overlap", call(CORR, X, X + 4, OUT, 3, 1000, 1030, 513, 515, 1024, 1100, 0));
  // ---- PFFT_UNSUPPORTED_CONFIGURATION, in the order of the checks
  // rows: 2^31 - 1 rows at pitch 8 admitted, ceil((2^31 - 1) / 4) = 2^29 groups; 2^31 refused
  const pairs_geometry many = admitted("2^31 - 1 rows", call(CORR, X, Y, OUT, P31 - 1, 8, 8, 8, 8, 8, 8, 0));
  CHECK_EQ("2^31 - 1 rows", many.groups, 536870912ll);
  CHECK_EQ("2^31 - 1 rows", many.n_rows, 2147483647ll);
  refused("2^31 rows", UNSUPPORTED, "pairs: 2147483648 rows: at most 2^31 - 1 rows per call", call(CORR, X, Y, OUT, P31, 8, 8, 8, 8, 8, 8, 0));
  // a pitch of 2^32: each side; 2^32 - 1 passes this rule and meets the next one (4 rows * (2^32 - 1) * 4 bytes)
  const char* pitch = "must be below 2^32 scalars";
  refused("x_pitch 2^32", UNSUPPORTED, pitch, call(CORR, X, Y, OUT, 1, 1000, P32, 513, 515, 1024, 1100, 0));
  refused("y_pitch 2^32", UNSUPPORTED, pitch, call(CORR, X, Y, OUT, 1, 1000, 1030, 513, P32, 1024, 1100, 0));
  refused("out_pitch 2^32", UNSUPPORTED, pitch, call(CORR, X, Y, OUT, 1, 1000, 1030, 513, 515, 1024, P32, 0));
  const char* reach = "row slots of one work-group span";
  refused("x_pitch 2^32 - 1", UNSUPPORTED, reach, call(CORR, X, Y, OUT, 1, 1000, P32 - 1, 513, 515, 1024, 1100, 0));
  refused("y_pitch 2^32 - 1", UNSUPPORTED, reach, call(CORR, X, Y, OUT, 1, 1000, 1030, 513, P32 - 1, 1024, 1100, 0));
  refused("out_pitch 2^32 - 1", UNSUPPORTED, reach, call(CORR, X, Y, OUT, 1, 1000, 1030, 513, 515, 1024, P32 - 1, 0));
  // the rows of one work-group: 4 * pitch * 4 bytes <= 2^32 - 1, pitch <= 268435455 -- however few rows the call has
  admitted("x reach", call(CORR, X, Y, OUT, 1, 1000, 268435455, 513, 515, 1024, 1100, 0));
  refused("x reach", UNSUPPORTED, "the 4 row slots of one work-group span 4294967296 bytes of x,", call(CORR, X, Y, OUT, 1, 1000, 268435456, 513, 515, 1024, 1100, 0));
  admitted("y reach", call(CORR, X, Y, OUT, 1, 1000, 1030, 513, 268435455, 1024, 1100, 0));
  refused("y reach", UNSUPPORTED, "4294967296 of y", call(CORR, X, Y, OUT, 1, 1000, 1030, 513, 268435456, 1024, 1100, 0));
  admitted("out reach", call(CORR, X, Y, OUT, 1, 1000, 1030, 513, 515, 1024, 268435455, 0));
  refused("out reach", UNSUPPORTED, "4294967296 of the output", call(CORR, X, Y, OUT, 1, 1000, 1030, 513, 515, 1024, 268435456, 0));
  // ---- the order, by calls that break two rules: the earlier one answers
  refused("null before mode", INVALID, "null data pointer", call(2, 0, Y, OUT, 3, 1000, 1030, 513, 515, 1024, 1100, 0));
  refused("mode before n_rows", INVALID, "mode 2", call(2, X, Y, OUT, 0, 1000, 1030, 513, 515, 1024, 1100, 0));
  refused("n_rows before lengths", INVALID, "zero count", call(CORR, X, Y, OUT, 0, 0, 1030, 513, 515, 1024, 1100, 0));
  refused("lengths before pitches", INVALID, "must be in 1 ... 1024", call(CORR, X, Y, OUT, 3, 1025, 999, 513, 515, 1024, 1100, 0));
  refused("pitches before the floor", INVALID, "below the lengths", call(CORR, X, Y, OUT, 3, 1000, 999, 513, 515, 1024, 1100, -1.0));
  refused("a bad floor before floor with convolve", INVALID, fl, call(CONV, X, Y, OUT, 3, 1000, 1030, 513, 515, 1024, 1100, nan));
  refused("floor with convolve before overlap", INVALID, "with PFFT_CONVOLVE", call(CONV, X, Y, X, 3, 1000, 1030, 513, 515, 1024, 1100, 1e-3));
  refused("overlap before 2^31 rows", INVALID, ov, call(CORR, X, Y, X, P31, 8, 8, 8, 8, 8, 8, 0));
  refused("overlap before a pitch of 2^32", INVALID, ov, call(CORR, X, Y, X, 2, 1000, P32, 513, 515, 1024, 1100, 0));
  // (the output in front of the inputs: 2^31 rows at a pitch of 2^32 scalars reach beyond every address behind x)
  refused("2^31 rows before a pitch of 2^32", UNSUPPORTED, "at most 2^31 - 1 rows", call(CORR, X, Y, uintptr_t(1) << 40, P31, 8, P32, 8, 8, 8, 8, 0));
  refused("a pitch of 2^32 before the reach", UNSUPPORTED, pitch, call(CORR, X, Y, OUT, 1, 1000, P32, 513, 268435456, 1024, 1100, 0));
  // ---- admitted calls: the arguments pass through in the kernel's order, groups = ceil(rows / 4)
  //   3 rows -> 1 group
  const pairs_geometry a = admitted("3 rows", call(CORR, X, Y, OUT, 3, 1000, 1031, 513, 515, 1023, 1101, 0.25));
  CHECK_EQ("3 rows", a.groups, 1);
  CHECK_EQ("3 rows", a.n_rows, 3);
  CHECK_EQ("3 rows", a.x_length, 1000);
  CHECK_EQ("3 rows", a.x_pitch, 1031);
  CHECK_EQ("3 rows", a.y_length, 513);
  CHECK_EQ("3 rows", a.y_pitch, 515);
  CHECK_EQ("3 rows", a.out_length, 1023);
  CHECK_EQ("3 rows", a.out_pitch, 1101);
  CHECK_EQ("3 rows: floor * 4", a.floor * 4, 1);
  //   9 rows = 2 * 4 + 1 -> 3 groups, the last one ragged; convolution, no floor
  const pairs_geometry b = admitted("9 rows", call(CONV, X, Y, OUT, 9, 1, 1025, 1024, 1027, 1, 1029, 0));
  CHECK_EQ("9 rows", b.groups, 3);
  CHECK_EQ("9 rows", b.n_rows, 9);
  CHECK_EQ("9 rows", b.x_length, 1);
  CHECK_EQ("9 rows", b.x_pitch, 1025);
  CHECK_EQ("9 rows", b.y_length, 1024);
  CHECK_EQ("9 rows", b.y_pitch, 1027);
  CHECK_EQ("9 rows", b.out_length, 1);
  CHECK_EQ("9 rows", b.out_pitch, 1029);
  CHECK_EQ("9 rows: no floor", b.floor == 0.0, 1);
  //   a kernel of one row per work-group, fp64: as many groups as rows; the floor's range is double's; the reach of one
  //   row is pitch * 8 bytes, pitch <= 536870911
  p.fpw = 1;
  p.sb = 8;
  const pairs_geometry c = admitted("fpw 1", call(CORR, X, X, OUT, 7, 512, 512, 512, 512, 512, 512, 1e-50));
  CHECK_EQ("fpw 1", c.groups, 7);
  CHECK_EQ("fpw 1", c.n_rows, 7);
  CHECK_EQ("fpw 1", c.x_pitch, 512);
  admitted("floor above FLT_MAX in fp64", call(CORR, X, Y, OUT, 3, 1000, 1030, 513, 515, 1024, 1100, 1e300));
  refused("floor subnormal in fp64", INVALID, fl, call(CORR, X, Y, OUT, 3, 1000, 1030, 513, 515, 1024, 1100, 1e-310));
  admitted("reach, fp64, one row per group", call(CORR, X, Y, OUT, 1, 1000, 536870911, 513, 515, 1024, 1100, 0));
  refused("reach, fp64, one row per group", UNSUPPORTED, "the 1 row slots of one work-group span 4294967296 bytes of x",
          call(CORR, X, Y, OUT, 1, 1000, 536870912, 513, 515, 1024, 1100, 0));
  std::printf("%d checks, %d failures\n", cases, failures);
  std::printf(failures == 0 ? "pairs geometry OK\n" : "pairs geometry FAILED\n");
  return failures == 0 ? 0 : 1;
}
