// The call-geometry rules of imdct (portfft_amd/csrc/verb_geometry.hpp: imdct_geometry_of) on the CPU: every refusal with
// its status and text, the order of the checks through calls that break two rules, every 32-bit boundary as the pair
// (largest admitted value, that value + 1), and the kernel arguments, `groups` and the default chunk of admitted calls
// against values worked out by hand (the derivation stands at each case).  Includes the header only; links nothing.
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

int main() {
  verb_facts p;  // fp32, N = 1024: unfolded frames of 2048 samples at hop 1024, 4 rows per work-group, 256 resident groups
  p.n = 1024;
  p.sb = 4;
  p.real = true;
  p.fpw = 4;
  p.resident[0] = p.resident[1] = 256;
  auto call = [&](uintptr_t in, uintptr_t out, ull ns, ull nf, ull fp, ull ip, ull lead, ull ol, ull op, ull chunk) {
    return [=] { return imdct_geometry_of(p, in, out, ns, nf, fp, ip, lead, ol, op, chunk); };
  };
  // the base call: 2 signals of 4 frames, lead 1024, 3000 samples: 3000 + 1024 <= 3 * 1024 + 2048 and 3072 < 4024
  // refusals, in the order of the checks
  refused("null in", INVALID, "imdct: null data pointer", call(0, OUT, 2, 4, 1024, 4096, 1024, 3000, 3000, 0));
  refused("null out", INVALID, "imdct: null data pointer", call(IN, 0, 2, 4, 1024, 4096, 1024, 3000, 3000, 0));
  refused("no signals", INVALID, "imdct: zero count (0 signals", call(IN, OUT, 0, 4, 1024, 4096, 1024, 3000, 3000, 0));
  refused("no frames", INVALID, "2 signals, 0 frames, out_length 3000)", call(IN, OUT, 2, 0, 1024, 4096, 1024, 3000, 3000, 0));
  refused("no output", INVALID, "4 frames, out_length 0)", call(IN, OUT, 2, 4, 1024, 4096, 1024, 0, 3000, 0));
  refused("lead 2N", INVALID, "lead 2048 must be below the frame length 2048", call(IN, OUT, 2, 4, 1024, 4096, 2048, 3000, 3000, 0));
  admitted("lead 2N - 1", call(IN, OUT, 2, 4, 1024, 4096, 2047, 3000, 3000, 0));
  refused("frame_pitch", INVALID, "frame_pitch 1023 below the 1024 coefficients", call(IN, OUT, 2, 4, 1023, 4096, 1024, 3000, 3000, 0));
  refused("2^32 signals", UNSUPPORTED, "counts, lengths and pitches below 2^32", call(IN, OUT, P32, 4, 1024, 4096, 1024, 3000, 3000, 0));
  refused("2^32 frames", UNSUPPORTED, "counts, lengths and pitches below 2^32", call(IN, OUT, 2, P32, 1024, 4096, 1024, 3000, 3000, 0));
  refused("out_length 2^32", UNSUPPORTED, "counts, lengths and pitches below 2^32", call(IN, OUT, 2, 4, 1024, 4096, 1024, P32, P32, 0));
  refused("in_pitch 2^32", UNSUPPORTED, "counts, lengths and pitches below 2^32", call(IN, OUT, 2, 4, 1024, P32, 1024, 3000, 3000, 0));
  refused("frame_pitch 2^32", UNSUPPORTED, "counts, lengths and pitches below 2^32", call(IN, OUT, 2, 4, P32, 4096, 1024, 3000, 3000, 0));
  refused("out_pitch 2^32", UNSUPPORTED, "counts, lengths and pitches below 2^32", call(IN, OUT, 2, 4, 1024, 4096, 1024, 3000, P32, 0));
  admitted("in_pitch and out_pitch 2^32 - 1, one signal", call(IN, OUT, 1, 4, 1024, P32 - 1, 1024, 3000, P32 - 1, 0));
  refused("in_pitch", INVALID, "in_pitch 4095 below n_frames * frame_pitch = 4096", call(IN, OUT, 2, 4, 1024, 4095, 1024, 3000, 3000, 0));
  refused("out_pitch", INVALID, "out_pitch 2999 below out_length 3000", call(IN, OUT, 2, 4, 1024, 4096, 1024, 3000, 2999, 0));
  // 4 frames, lead 1024, cover 3 * 1024 + 2048 - 1024 = 4096 samples
  refused("uncovered samples", INVALID, "out_length 4097 above (n_frames - 1) * N + 2N - lead = 4096",
          call(IN, OUT, 2, 4, 1024, 4096, 1024, 4097, 4097, 0));
  admitted("full coverage", call(IN, OUT, 2, 4, 1024, 4096, 1024, 4096, 4096, 0));
  // frame 3 starts at 3072 - lead: out_length + lead = 3072 leaves it nothing, 3073 gives it one sample
  refused("idle frame", INVALID, "frame 3 starts at sample 3072 - lead 1024, beyond the out_length 2048",
          call(IN, OUT, 2, 4, 1024, 4096, 1024, 2048, 2048, 0));
  admitted("one sample of the last frame", call(IN, OUT, 2, 4, 1024, 4096, 1024, 2049, 2049, 0));
  refused("idle frame, lead 0", INVALID, "frame 3 starts at sample 3072 - lead 0", call(IN, OUT, 2, 4, 1024, 4096, 0, 3072, 3072, 0));
  admitted("one sample, lead 0", call(IN, OUT, 2, 4, 1024, 4096, 0, 3073, 3073, 0));
  // 2 signals: (4096 + 3 * 1024 + 1024) * 4 = 32768 bytes in; (3000 + 3000) * 4 = 24000 bytes out
  refused("in place", INVALID, "byte ranges overlap; the transform cannot run in place (a chunk reads coefficients",
          call(IN, IN, 2, 4, 1024, 4096, 1024, 3000, 3000, 0));
  refused("partial overlap", INVALID, "byte ranges overlap", call(IN, IN + 32767, 2, 4, 1024, 4096, 1024, 3000, 3000, 0));
  admitted("adjacent", call(IN, IN + 32768, 2, 4, 1024, 4096, 1024, 3000, 3000, 0));
  refused("partial overlap, out first", INVALID, "byte ranges overlap", call(IN + 23999, IN, 2, 4, 1024, 4096, 1024, 3000, 3000, 0));
  admitted("adjacent, out first", call(IN + 24000, IN, 2, 4, 1024, 4096, 1024, 3000, 3000, 0));
  // the order, by calls that break two rules: the earlier one answers
  refused("null before zero count", INVALID, "null data pointer", call(0, OUT, 0, 4, 1024, 4096, 1024, 3000, 3000, 0));
  refused("zero count before lead", INVALID, "zero count", call(IN, OUT, 1, 0, 1024, 4096, 2048, 3000, 3000, 0));
  refused("lead before frame_pitch", INVALID, "lead 2048", call(IN, OUT, 2, 4, 1023, 4096, 2048, 3000, 3000, 0));
  refused("frame_pitch before 2^32", INVALID, "frame_pitch 1023", call(IN, OUT, P32, 4, 1023, 4096, 1024, 3000, 3000, 0));
  refused("2^32 before in_pitch", UNSUPPORTED, "below 2^32", call(IN, OUT, P32, 4, 1024, 4095, 1024, 3000, 3000, 0));
  refused("in_pitch before out_pitch", INVALID, "in_pitch 4095", call(IN, OUT, 2, 4, 1024, 4095, 1024, 3000, 2999, 0));
  refused("out_pitch before coverage", INVALID, "out_pitch 4096 below out_length 4097", call(IN, OUT, 2, 4, 1024, 4096, 1024, 4097, 4096, 0));
  refused("coverage before overlap", INVALID, "covered by no frame", call(IN, IN, 2, 4, 1024, 4096, 1024, 4097, 4097, 0));
  refused("idle frame before overlap", INVALID, "at least one sample", call(IN, IN, 2, 4, 1024, 4096, 1024, 2048, 2048, 0));
  refused("overlap before the row count", INVALID, "cannot run in place", call(IN, IN, P31, 1, 1024, 1024, 0, 8, 8, 0));
  // 2^16 signals of 2^15 frames at frame_pitch 131071 in one chunk: the run spans (32767 * 131071 + 1024) * 4 bytes, far
  // above 4 GiB -- the row count answers first
  refused("row count before the reach", UNSUPPORTED, "65536 signals of 32768 frames each",
          call(IN, OUT, 1ull << 16, 1ull << 15, 131071, 4294934528ull, 0, 33554432, 33554432, 1ull << 15));
  // rows: 2^31 - 1 signals of one frame admitted -- one chunk each, 2^31 - 1 groups --, 2^31 refused
  const imdct_geometry rows = admitted("2^31 - 1 rows", call(IN, OUT, P31 - 1, 1, 1024, 1024, 0, 8, 8, 0));
  CHECK_EQ("2^31 - 1 rows", rows.groups, 2147483647ll);
  CHECK_EQ("2^31 - 1 rows", rows.chunk, 1);
  refused("2^31 rows", UNSUPPORTED, "2147483648 signals of 1 frames each", call(IN, OUT, P31, 1, 1024, 1024, 0, 8, 8, 0));
  // reach_in, chunk 3 of 4 frames: the run is the halo and the chunk, 4 frames: (3 * frame_pitch + 1024) * 4 <= 2^32 - 1,
  // 3 * frame_pitch <= 1073740799, frame_pitch <= 357913599
  admitted("reach_in, chunk 3", call(IN, OUT, 1, 4, 357913599, 4ull * 357913599, 1024, 3000, 3000, 3));
  refused("reach_in, chunk 3", UNSUPPORTED, "the 4 frames one work-group runs span 4294967296 bytes",
          call(IN, OUT, 1, 4, 357913600, 4ull * 357913600, 1024, 3000, 3000, 3));
  refused("reach_in names the way out", UNSUPPORTED, "a smaller chunk_frames shortens both",
          call(IN, OUT, 1, 4, 357913600, 4ull * 357913600, 1024, 3000, 3000, 3));
  // ... chunk 1: a run of 2 frames, (frame_pitch + 1024) * 4 <= 2^32 - 1, frame_pitch <= 1073740799
  admitted("reach_in, chunk 1", call(IN, OUT, 1, 4, 357913600, 4ull * 357913600, 1024, 3000, 3000, 1));
  admitted("reach_in, chunk 1, top", call(IN, OUT, 1, 4, 1073740799, 4294963196ull, 1024, 3000, 3000, 1));
  refused("reach_in, chunk 1, top + 1", UNSUPPORTED, "the 2 frames one work-group runs span 4294967296 bytes",
          call(IN, OUT, 1, 3, 1073740800, 3221222400ull, 1024, 2000, 2000, 1));
  // reach_out, one chunk of 1048567 frames, lead 0: (out_length + 6 * 1024 + 2048) * 4 <= 2^32 - 1, out_length <=
  // 1073741823 - 8192 = 1073733631; (n_frames + 1) * 1024 = 1073733632 covers both; the run spans 1048567 * 4096 bytes
  admitted("reach_out, one chunk", call(IN, OUT, 1, 1048567, 1024, 1073732608, 0, 1073733631, 1073733631, 1048567));
  refused("reach_out, one chunk", UNSUPPORTED, "the samples it covers 4294967296;",
          call(IN, OUT, 1, 1048567, 1024, 1073732608, 0, 1073733632, 1073733632, 1048567));
  admitted("reach_out, chunks of 1024", call(IN, OUT, 1, 1048567, 1024, 1073732608, 0, 1073733632, 1073733632, 1024));
  // the default chunk (istft_default_chunk with a halo of 1): want = max(1, ceil(2 * 256 / signals)) chunks per signal,
  // ceil(frames / want) frames, at least max(4, fpw) = 4, rounded up to whole steps of 4, at most the frames
  //   2 signals of 4 frames: want 256, 1 -> 4 -> min(4, 4) = 4; one chunk each, 2 groups
  const imdct_geometry base = admitted("2 x 4", call(IN, OUT, 2, 4, 1030, 4200, 1023, 3000, 3001, 0));
  CHECK_EQ("2 x 4", base.chunk, 4);
  CHECK_EQ("2 x 4", base.groups, 2);
  CHECK_EQ("2 x 4", base.n_signals, 2);
  CHECK_EQ("2 x 4", base.n_frames, 4);
  CHECK_EQ("2 x 4", base.lead, 1023);
  CHECK_EQ("2 x 4", base.out_length, 3000);
  CHECK_EQ("2 x 4", base.frame_pitch, 1030);
  CHECK_EQ("2 x 4", base.in_pitch, 4200);
  CHECK_EQ("2 x 4", base.out_pitch, 3001);
  //   64 signals of 4097 frames: want 8, ceil(4097 / 8) = 513 -> 516; ceil(4097 / 516) = 8 chunks, 512 groups
  const imdct_geometry wide = admitted("64 x 4097", call(IN, OUT, 64, 4097, 1024, 4097ull * 1024, 1024, 4097ull * 1024, 4097ull * 1024, 0));
  CHECK_EQ("64 x 4097", wide.chunk, 516);
  CHECK_EQ("64 x 4097", wide.groups, 512);
  CHECK_EQ("64 x 4097 is istft_default_chunk", wide.chunk, istft_default_chunk(64, 4097, 1, 4, 256));
  //   1024 signals of 3 frames: want 1, 3 -> 4 -> min(4, 3) = 3
  const imdct_geometry many = admitted("1024 x 3", call(IN, OUT, 1024, 3, 1024, 3072, 1024, 3000, 3000, 0));
  CHECK_EQ("1024 x 3", many.chunk, 3);
  CHECK_EQ("1024 x 3", many.groups, 1024);
  // a given chunk: 3 signals of 7 frames in chunks of 3 -> 3 chunks each, 9 groups; a chunk above the frames is the frames
  const imdct_geometry given = admitted("3 x 7, chunk 3", call(IN, OUT, 3, 7, 1024, 7168, 1024, 7000, 7000, 3));
  CHECK_EQ("3 x 7, chunk 3", given.chunk, 3);
  CHECK_EQ("3 x 7, chunk 3", given.groups, 9);
  const imdct_geometry above = admitted("3 x 7, chunk 100", call(IN, OUT, 3, 7, 1024, 7168, 1024, 7000, 7000, 100));
  CHECK_EQ("3 x 7, chunk 100", above.chunk, 7);
  CHECK_EQ("3 x 7, chunk 100", above.groups, 3);
  const imdct_geometry one = admitted("3 x 7, chunk 1", call(IN, OUT, 3, 7, 1024, 7168, 1024, 7000, 7000, 1));
  CHECK_EQ("3 x 7, chunk 1", one.groups, 21);
  std::printf("%d checks, %d failures\n", cases, failures);
  std::printf(failures == 0 ? "imdct geometry OK\n" : "imdct geometry FAILED\n");
  return failures == 0 ? 0 : 1;
}
