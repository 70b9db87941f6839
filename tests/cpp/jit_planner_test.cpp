// Runtime-specialisation planner (portfft_amd/csrc/jit_planner.cpp) on the host: invariants of the chosen kernel
// parameters for every length, and hiprtc compilation of a few of them for gfx950 (no device needed).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../include/portfft_amd.h"
#include "../../portfft_amd/csrc/jit.hpp"

static int fails = 0;
#define EXPECT(c, ...)                 \
  do {                                 \
    if (!(c)) {                        \
      ++fails;                         \
      std::printf("FAIL %s: ", #c);    \
      std::printf(__VA_ARGS__);        \
      std::printf("\n");               \
    }                                  \
  } while (0)

/// prime factors up to the wavefront size (jit_planner.cpp: jit_max_prime)
static bool smooth31(long long n) {
  for (int p = 2; p <= 61; ++p) {
    while (n % p == 0) n /= p;
  }
  return n == 1;
}

/// The registries of pre-compiled packed kernels (kernels.hpp): every entry carries exactly its registry's forms, as
/// host symbols; the two-tier entries; the configurations the real and the Bluestein registries share.
static void check_packed_registries() {
  struct registry {
    const char* name;
    const pfa::spec_kernel* k;
    int count;
    unsigned forms;  // bit f: the registry's entries carry form f
  };
  registry regs[5] = {{"f32", nullptr, 0, 1u << pfa::WF_INTERLEAVED | 1u << pfa::WF_SPLIT},
                      {"f64", nullptr, 0, 1u << pfa::WF_INTERLEAVED | 1u << pfa::WF_SPLIT},
                      {"f16", nullptr, 0, 1u << pfa::WF_INTERLEAVED | 1u << pfa::WF_SPLIT},
                      {"real", nullptr, 0, 1u << pfa::WF_REAL},
                      {"bluestein", nullptr, 0, 1u << pfa::WF_BLUESTEIN}};
  regs[0].k = pfa::spec_kernels_f32(&regs[0].count);
  regs[1].k = pfa::spec_kernels_f64(&regs[1].count);
  regs[2].k = pfa::spec_kernels_f16(&regs[2].count);
  regs[3].k = pfa::real_kernels(&regs[3].count);
  regs[4].k = pfa::bluestein_kernels(&regs[4].count);
  int two_tier = 0;
  for (const registry& r : regs) {
    EXPECT(r.count > 0, "registry %s is empty", r.name);
    for (int i = 0; i < r.count; ++i) {
      const pfa::spec_kernel& k = r.k[i];
      for (int f = 0; f < pfa::N_SPEC_FORMS; ++f) {
        for (int d = 0; d < 2; ++d) {
          const pfa::kernel_fn& c = k.form[f][d];
          EXPECT(static_cast<bool>(c) == ((r.forms >> f & 1u) != 0), "%s n=%d: form %d direction %d", r.name, k.n, f, d);
          EXPECT(c.mod == nullptr, "%s n=%d: form %d direction %d holds a module function", r.name, k.n, f, d);
        }
      }
      EXPECT(!k.jit && k.lds_bytes > 0, "%s n=%d: jit %d lds %zu", r.name, k.n, static_cast<int>(k.jit), k.lds_bytes);
      const bool headline = k.n == 4096 && (k.precision == PFFT_PRECISION_F32 || k.precision == PFFT_PRECISION_F16) &&
                            (r.forms >> pfa::WF_INTERLEAVED & 1u) != 0;
      EXPECT((k.two_tier != 0) == headline, "%s n=%d precision %d: two_tier %d", r.name, k.n, k.precision, k.two_tier);
      two_tier += k.two_tier != 0;
    }
  }
  EXPECT(two_tier == 2, "%d two-tier entries (fp32 and fp16 N = 4096)", two_tier);
  // every convolution length P runs the configuration of the real entry of M = P (wg_pow2_cfg.hpp)
  for (int i = 0; i < regs[4].count; ++i) {
    const pfa::spec_kernel& b = regs[4].k[i];
    const pfa::spec_kernel* m = nullptr;
    for (int j = 0; j < regs[3].count && m == nullptr; ++j) {
      if (regs[3].k[j].precision == b.precision && regs[3].k[j].n == b.n) m = &regs[3].k[j];
    }
    EXPECT(m != nullptr, "bluestein P=%d precision %d: no real entry of M = P", b.n, b.precision);
    if (m == nullptr) continue;
    EXPECT(m->n_radices == b.n_radices && std::equal(b.radices, b.radices + b.n_radices, m->radices) && m->wg == b.wg &&
               m->fpw == b.fpw && m->groups_per_wg == b.groups_per_wg,
           "bluestein P=%d precision %d differs from the real entry of M = P", b.n, b.precision);
  }
  // the two-tier grid belongs to the prefetching (interleaved) cell of a two_tier entry alone
  for (const registry& r : regs) {
    for (int i = 0; i < r.count; ++i) {
      const pfa::spec_kernel& k = r.k[i];
      for (int f = 0; f < pfa::N_SPEC_FORMS; ++f) {
        unsigned grid = 4098;  // the uniform grid of 16391 groups at 4 per work-group
        long long n_main = -1;
        int main_k = -1;
        pfa::two_tier_grid(k, f, 16391ll * k.fpw, &grid, &n_main, &main_k);
        if (k.two_tier != 0 && f == pfa::WF_INTERLEAVED) {
          EXPECT(grid == 5124 && n_main == 3072 && main_k == 4, "%s n=%d: two-tier grid %u n_main %lld k %d", r.name, k.n,
                 grid, n_main, main_k);
        } else {
          EXPECT(grid == 4098 && n_main == 0 && main_k == 4, "%s n=%d form %d: grid %u n_main %lld reshaped", r.name, k.n, f,
                 grid, n_main);
        }
        grid = 1001;  // a small launch stays uniform whatever the entry
        pfa::two_tier_grid(k, f, 1001ll * k.fpw, &grid, &n_main, &main_k);
        EXPECT(grid == 1001 && n_main == 0 && main_k == 1, "%s n=%d form %d: small grid %u n_main %lld", r.name, k.n, f, grid,
               n_main);
        grid = 4095;  // below 4096 work-groups: uniform, however many groups each takes
        pfa::two_tier_grid(k, f, 4095ll * 8 * k.fpw, &grid, &n_main, &main_k);
        EXPECT(grid == 4095 && n_main == 0 && main_k == 8, "%s n=%d form %d: grid %u below the threshold", r.name, k.n, f, grid);
      }
    }
  }
  std::printf("packed registries: %d + %d + %d complex, %d real, %d bluestein entries\n", regs[0].count, regs[1].count,
              regs[2].count, regs[3].count, regs[4].count);
}

/// What the runtime compiler hands hiprtc for every form it builds (jit_instantiation): header and name expressions, written
/// out here as jit.cpp spelled them before the forms had names -- they are part of the key of the disk cache, so a change
/// of one character recompiles every user's kernels of that form.
static void check_instantiations() {
  using F = pfa::jit_form;  // {family, split, half, stw, split_mode, tin, big, row_out}
  struct {
    F form;
    const char *header, *fwd, *bwd;
  } rows[] = {
      {F{pfa::JF_PACKED}, "stockham_wg.hpp", "pfa::stockham_wg_kernel<CFG, false>", "pfa::stockham_wg_kernel<CFG, true>"},
      {F{pfa::JF_PACKED, true}, "stockham_wg.hpp", "pfa::stockham_wg_split_kernel<CFG, false>", "pfa::stockham_wg_split_kernel<CFG, true>"},
      {F{pfa::JF_PACKED, false, true}, "stockham_wg.hpp", "pfa::stockham_wg_half_kernel<CFG, false>", "pfa::stockham_wg_half_kernel<CFG, true>"},
      {F{pfa::JF_PACKED, true, true}, "stockham_wg.hpp", "pfa::stockham_wg_half_split_kernel<CFG, false>", "pfa::stockham_wg_half_split_kernel<CFG, true>"},
      {F{pfa::JF_PACKED_HX}, "stockham_wg_hx.hpp", "pfa::stockham_wg_hx_kernel<CFG, false>", "pfa::stockham_wg_hx_kernel<CFG, true>"},
      {F{pfa::JF_PACKED_HX, true}, "stockham_wg_hx.hpp", "pfa::stockham_wg_hx_split_kernel<CFG, false>", "pfa::stockham_wg_hx_split_kernel<CFG, true>"},
      {F{pfa::JF_PACKED_HX, false, true}, "stockham_wg_hx.hpp", "pfa::stockham_wg_hx_half_kernel<CFG, false>", "pfa::stockham_wg_hx_half_kernel<CFG, true>"},
      {F{pfa::JF_PACKED_HX, true, true}, "stockham_wg_hx.hpp", "pfa::stockham_wg_hx_half_split_kernel<CFG, false>", "pfa::stockham_wg_hx_half_split_kernel<CFG, true>"},
      {F{pfa::JF_UNPACKED}, "stockham_wg.hpp", "pfa::stockham_wg_unpacked_kernel<CFG, false, false>", "pfa::stockham_wg_unpacked_kernel<CFG, true, false>"},
      {F{pfa::JF_UNPACKED, true}, "stockham_wg.hpp", "pfa::stockham_wg_unpacked_kernel<CFG, false, true>", "pfa::stockham_wg_unpacked_kernel<CFG, true, true>"},
      {F{pfa::JF_REAL}, "stockham_wg_real.hpp", "pfa::stockham_wg_r2c_kernel<CFG>", "pfa::stockham_wg_c2r_kernel<CFG>"},
      // LDS-resident strided: plain, store modifier from LDS / global tables, split, split + store modifier, mixed in, mixed out
      {F{pfa::JF_STRIDED}, "stockham_strided.hpp", "pfa::stockham_strided_kernel<CFG, false, 0, 0, 0, false, 1>", "pfa::stockham_strided_kernel<CFG, true, 0, 0, 0, false, 1>"},
      {F{pfa::JF_STRIDED, false, false, 1}, "stockham_strided.hpp", "pfa::stockham_strided_kernel<CFG, false, 1, 0, 0, false, 1>", "pfa::stockham_strided_kernel<CFG, true, 1, 0, 0, false, 1>"},
      {F{pfa::JF_STRIDED, false, false, 2}, "stockham_strided.hpp", "pfa::stockham_strided_kernel<CFG, false, 2, 0, 0, false, 1>", "pfa::stockham_strided_kernel<CFG, true, 2, 0, 0, false, 1>"},
      {F{pfa::JF_STRIDED, false, false, 0, 1}, "stockham_strided.hpp", "pfa::stockham_strided_kernel<CFG, false, 0, 1, 0, false, 1>", "pfa::stockham_strided_kernel<CFG, true, 0, 1, 0, false, 1>"},
      {F{pfa::JF_STRIDED, false, false, 1, 1}, "stockham_strided.hpp", "pfa::stockham_strided_kernel<CFG, false, 1, 1, 0, false, 1>", "pfa::stockham_strided_kernel<CFG, true, 1, 1, 0, false, 1>"},
      {F{pfa::JF_STRIDED, false, false, 2, 1}, "stockham_strided.hpp", "pfa::stockham_strided_kernel<CFG, false, 2, 1, 0, false, 1>", "pfa::stockham_strided_kernel<CFG, true, 2, 1, 0, false, 1>"},
      {F{pfa::JF_STRIDED, false, false, 1, 2}, "stockham_strided.hpp", "pfa::stockham_strided_kernel<CFG, false, 1, 2, 0, false, 1>", "pfa::stockham_strided_kernel<CFG, true, 1, 2, 0, false, 1>"},
      {F{pfa::JF_STRIDED, false, false, 2, 2}, "stockham_strided.hpp", "pfa::stockham_strided_kernel<CFG, false, 2, 2, 0, false, 1>", "pfa::stockham_strided_kernel<CFG, true, 2, 2, 0, false, 1>"},
      {F{pfa::JF_STRIDED, false, false, 0, 3}, "stockham_strided.hpp", "pfa::stockham_strided_kernel<CFG, false, 0, 3, 0, false, 1>", "pfa::stockham_strided_kernel<CFG, true, 0, 3, 0, false, 1>"},
      // ... BIG
      {F{pfa::JF_STRIDED, false, false, 0, 0, false, true}, "stockham_strided.hpp", "pfa::stockham_strided_kernel<CFG, false, 0, 0, 0, true, 1>", "pfa::stockham_strided_kernel<CFG, true, 0, 0, 0, true, 1>"},
      {F{pfa::JF_STRIDED, false, false, 1, 0, false, true}, "stockham_strided.hpp", "pfa::stockham_strided_kernel<CFG, false, 1, 0, 0, true, 1>", "pfa::stockham_strided_kernel<CFG, true, 1, 0, 0, true, 1>"},
      {F{pfa::JF_STRIDED, false, false, 2, 1, false, true}, "stockham_strided.hpp", "pfa::stockham_strided_kernel<CFG, false, 2, 1, 0, true, 1>", "pfa::stockham_strided_kernel<CFG, true, 2, 1, 0, true, 1>"},
      // ... tiled input: the mixed stage B, and the compile-check-only interleaved form
      {F{pfa::JF_STRIDED, false, false, 0, 3, true}, "stockham_strided.hpp", "pfa::stockham_strided_kernel<CFG, false, 0, 3, true>", "pfa::stockham_strided_kernel<CFG, true, 0, 3, true>"},
      {F{pfa::JF_STRIDED, false, false, 0, 0, true}, "stockham_strided.hpp", "pfa::stockham_strided_kernel<CFG, false, 0, 0, 1>", "pfa::stockham_strided_kernel<CFG, true, 0, 0, 1>"},
      // register-resident strided
      {F{pfa::JF_STRIDED_HX}, "stockham_strided_hx.hpp", "pfa::stockham_strided_hx_kernel<CFG, false, 0, 0>", "pfa::stockham_strided_hx_kernel<CFG, true, 0, 0>"},
      {F{pfa::JF_STRIDED_HX, false, false, 1}, "stockham_strided_hx.hpp", "pfa::stockham_strided_hx_kernel<CFG, false, 1, 0>", "pfa::stockham_strided_hx_kernel<CFG, true, 1, 0>"},
      {F{pfa::JF_STRIDED_HX, false, false, 2}, "stockham_strided_hx.hpp", "pfa::stockham_strided_hx_kernel<CFG, false, 2, 0>", "pfa::stockham_strided_hx_kernel<CFG, true, 2, 0>"},
      {F{pfa::JF_STRIDED_HX, false, false, 0, 1}, "stockham_strided_hx.hpp", "pfa::stockham_strided_hx_kernel<CFG, false, 0, 1>", "pfa::stockham_strided_hx_kernel<CFG, true, 0, 1>"},
      {F{pfa::JF_STRIDED_HX, false, false, 1, 1}, "stockham_strided_hx.hpp", "pfa::stockham_strided_hx_kernel<CFG, false, 1, 1>", "pfa::stockham_strided_hx_kernel<CFG, true, 1, 1>"},
      {F{pfa::JF_STRIDED_HX, false, false, 2, 2}, "stockham_strided_hx.hpp", "pfa::stockham_strided_hx_kernel<CFG, false, 2, 2>", "pfa::stockham_strided_hx_kernel<CFG, true, 2, 2>"},
      {F{pfa::JF_STRIDED_HX, false, false, 0, 3}, "stockham_strided_hx.hpp", "pfa::stockham_strided_hx_kernel<CFG, false, 0, 3>", "pfa::stockham_strided_hx_kernel<CFG, true, 0, 3>"},
      {F{pfa::JF_STRIDED_HX, false, false, 0, 0, false, true}, "stockham_strided_hx.hpp", "pfa::stockham_strided_hx_kernel<CFG, false, 0, 0, true>", "pfa::stockham_strided_hx_kernel<CFG, true, 0, 0, true>"},
      {F{pfa::JF_STRIDED_HX, false, false, 1, 0, false, true}, "stockham_strided_hx.hpp", "pfa::stockham_strided_hx_kernel<CFG, false, 1, 0, true>", "pfa::stockham_strided_hx_kernel<CFG, true, 1, 0, true>"},
      // row-staged: row in, row out, row in of the mixed stage B
      {F{pfa::JF_STRIDED_ROW}, "stockham_strided.hpp", "pfa::stockham_strided_row_kernel<CFG, false, true, false, 0, 1>", "pfa::stockham_strided_row_kernel<CFG, true, true, false, 0, 1>"},
      {F{pfa::JF_STRIDED_ROW, false, false, 0, 0, false, false, true}, "stockham_strided.hpp", "pfa::stockham_strided_row_kernel<CFG, false, false, true, 0, 1>", "pfa::stockham_strided_row_kernel<CFG, true, false, true, 0, 1>"},
      {F{pfa::JF_STRIDED_ROW, false, false, 0, 3}, "stockham_strided.hpp", "pfa::stockham_strided_row_kernel<CFG, false, true, false, 3, 1>", "pfa::stockham_strided_row_kernel<CFG, true, true, false, 3, 1>"},
      {F{pfa::JF_ROWS2D}, "stockham_rows2d.hpp", "pfa::stockham_rows2d_kernel<CFG, false, false>", "pfa::stockham_rows2d_kernel<CFG, true, false>"},
      {F{pfa::JF_ROWS2D, true}, "stockham_rows2d.hpp", "pfa::stockham_rows2d_kernel<CFG, false, true>", "pfa::stockham_rows2d_kernel<CFG, true, true>"},
      {F{pfa::JF_ND}, "stockham_nd.hpp", "pfa::stockham_nd_kernel<CFG, false>", "pfa::stockham_nd_kernel<CFG, true>"},
      {F{pfa::JF_ND, true}, "stockham_nd.hpp", "pfa::stockham_nd_split_kernel<CFG, false>", "pfa::stockham_nd_split_kernel<CFG, true>"},
  };
  for (const auto& r : rows) {
    const pfa::jit_names got = pfa::jit_instantiation(r.form, "CFG");
    EXPECT(std::string(got.header) == r.header && got.expr[0] == r.fwd && got.expr[1] == r.bwd, "%s: %s / %s / %s", r.fwd,
           got.header, got.expr[0].c_str(), got.expr[1].c_str());
  }
  std::printf("instantiations: %zu forms spelled as before\n", sizeof(rows) / sizeof(rows[0]));
}

int main(int argc, char** argv) {
  const size_t max_lds = 160 * 1024;
  // "plan f32|f64 n ...": the packed planner's choice for each length, one line each (tests/test_odd_radix_classes.py)
  if (argc > 2 && std::string(argv[1]) == "plan") {
    const int prec = std::string(argv[2]) == "f64" ? 1 : 0;
    for (int i = 3; i < argc; ++i) {
      const long long n = std::atoll(argv[i]);
      pfa::wg_params p;
      if (!pfa::choose_spec_params(prec, n, max_lds, &p)) {
        std::printf("plan %s n=%lld none\n", argv[2], n);
        continue;
      }
      std::string rad;
      for (int r : p.radices) rad += (rad.empty() ? "" : "x") + std::to_string(r);
      std::printf("plan %s n=%lld radices=%s lanes=%d fpw=%d wg=%d pads=%d staged=%d regs=%d\n", argv[2], n, rad.c_str(),
                  p.wg / p.fpw, p.fpw, p.wg, p.pads, p.staged, p.regs);
    }
    return 0;
  }
  unsetenv("PFFT_UNIFORM_GRID");  // (the A/B switch two_tier_grid reads once: the grids asserted below are the default's)
  check_packed_registries();
  check_instantiations();
  long long planned[2] = {0, 0};
  for (int prec = 0; prec < 2; ++prec) {
    const int es = prec ? 16 : 8;
    for (long long n = 2; n <= 21000; ++n) {
      pfa::wg_params p;
      const bool ok = pfa::choose_spec_params(prec, n, max_lds, &p);
      if (!smooth31(n) || static_cast<size_t>(n) * es > max_lds) {
        EXPECT(!ok, "n=%lld prec=%d should not be planned", n, prec);
        continue;
      }
      EXPECT(ok, "n=%lld prec=%d not planned", n, prec);
      if (!ok) continue;
      ++planned[prec];
      long long prod = 1;
      for (int r : p.radices) {
        prod *= r;
        EXPECT(r >= 2 && r <= 61 && (r <= 32 || (r % 2 != 0 && r % 3 != 0 && r % 5 != 0 && r % 7 != 0)),
               "n=%lld radix %d", n, r);
      }
      EXPECT(prod == n, "n=%lld product %lld", n, prod);
      EXPECT(p.radices.size() <= 6, "n=%lld passes", n);
      EXPECT(p.wg >= 1 && p.wg <= 1024 && p.fpw >= 1 && p.wg % p.fpw == 0, "n=%lld wg=%d fpw=%d", n, p.wg, p.fpw);
      EXPECT(pfa::spec_lds_bytes(p) <= max_lds, "n=%lld lds=%zu", n, pfa::spec_lds_bytes(p));
      EXPECT(p.regs <= 64, "n=%lld regs=%d", n, p.regs);
      const int tpf = p.wg / p.fpw;
      for (int r : p.radices) {
        const long long bpt = (n / r + tpf - 1) / tpf;
        EXPECT(bpt * r <= p.regs, "n=%lld radix %d bpt %lld regs %d", n, r, bpt, p.regs);
      }
      pfa::wg_params q;
      if (pfa::choose_strided_params(prec, n, 1000, max_lds, &q)) {
        long long pq = 1;
        for (int r : q.radices) pq *= r;
        EXPECT(pq == n && (q.radices.size() >= 2 || n <= 61), "strided n=%lld", n);  // one lane per FFT up to the largest radix
        EXPECT(q.wg >= 64 && q.wg <= 1024 && q.wg % q.fpw == 0, "strided n=%lld wg=%d fpw=%d", n, q.wg, q.fpw);
        // (one FFT per work-group -- lengths beyond the generic tier's two images -- may use all of the LDS)
        EXPECT(static_cast<size_t>(n) * q.fpw * es <= (q.fpw == 1 ? max_lds : 128 * 1024), "strided n=%lld lds", n);
        EXPECT(q.fpw > 1 || static_cast<size_t>(n) * 2 * es > max_lds, "strided n=%lld: one FFT per work-group", n);
      }
      // a requested group width (four-step half pairs, plan_global.cpp) is honoured exactly or refused
      for (int want : {8, 16}) {
        pfa::wg_params w;
        if (n > 32 && pfa::choose_strided_params(prec, n, 1024, max_lds, &w, false, want)) {
          EXPECT(w.fpw == want && w.wg % want == 0 && w.wg >= 64 && w.wg <= 1024, "strided n=%lld want %d: fpw=%d wg=%d",
                 n, want, w.fpw, w.wg);
          EXPECT(static_cast<size_t>(n) * want * es <= 128 * 1024, "strided n=%lld want %d lds", n, want);
        }
      }
    }
  }
  std::printf("planned %lld fp32 and %lld fp64 lengths\n", planned[0], planned[1]);
  // choices the measurements in profiles/r1_notes.md rest on
  pfa::wg_params p;
  pfa::choose_spec_params(0, 243, max_lds, &p);
  EXPECT(p.radices.size() == 3 && p.radices[0] == 9, "243 -> 9,9,3");
  pfa::choose_spec_params(0, 4096, max_lds, &p);
  EXPECT(p.radices.size() == 3 && p.radices[0] == 16 && p.wg == 256 && p.fpw == 1, "4096 -> 16,16,16 / 256 lanes");
  // two-pass 2-D plan, pass 1: the planner's invariants for every row length it accepts
  for (int prec = 0; prec < 2; ++prec) {
    int accepted = 0;
    for (long long n1 = 32; n1 <= 8192; ++n1) {
      for (long long n0 : {64ll, 1000ll, 1026ll}) {
        pfa::wg_params q;
        if (!pfa::choose_rows2d_params(prec, n1, n0, max_lds, &q)) continue;
        ++accepted;
        long long prod = 1;
        for (int r : q.radices) prod *= r;
        const long long nbl = n1 / q.radices.back();
        EXPECT(prod == n1 && q.radices.size() >= 2, "rows2d %lld: radices multiply to n1", n1);
        EXPECT(n0 % q.fpw == 0 && n0 / q.fpw >= 2, "rows2d %lld x %lld: column radix %d divides n0", n1, n0, q.fpw);
        EXPECT(nbl % q.wg == 0 && q.wg % q.fpw == 0 && q.wg <= 1024, "rows2d %lld: lanes %d", n1, q.wg);
        EXPECT(q.regs <= (prec ? 16 : 32), "rows2d %lld: %d elements per lane", n1, q.regs);
        EXPECT(pfa::spec_lds_bytes(q) <= max_lds, "rows2d %lld: LDS", n1);
      }
    }
    EXPECT(accepted > 500, "rows2d planner accepts %d (n1, n0) pairs", accepted);
    // the caller's mask of usable column radices is honoured (3000 x 1000: radix 2 would leave 1500-point columns)
    pfa::wg_params q;
    EXPECT(pfa::choose_rows2d_params(prec, 1000, 3000, max_lds, &q, 4) && q.fpw == 4, "rows2d 3000 x 1000, mask 4");
    EXPECT(!pfa::choose_rows2d_params(prec, 1000, 3000, max_lds, &q, 8), "rows2d 3000 x 1000: no radix-8 plan");
  }
  // register-resident packed kernel (stockham_wg_hx.hpp): lengths beyond the LDS whose transform fits the registers of one
  // work-group -- invariants of every plan the planner hands out
  {
    long long planned_hx[2] = {0, 0};
    pfa::wg_params p0;
    for (int prec = 0; prec < 2; ++prec) {
      const int es = prec ? 16 : 8;
      for (long long n = (prec ? 10241 : 19000); n <= (prec ? 21000 : 42000); ++n) {
        pfa::wg_params p;
        if (!pfa::choose_hx_params(prec, n, max_lds, &p)) continue;
        ++planned_hx[prec];
        long long prod = 1;
        int regs = 0;
        for (int r : p.radices) {
          prod *= r;
          EXPECT(r >= 2 && r <= 32, "hx n=%lld radix %d", n, r);
          regs = std::max<int>(regs, static_cast<int>((n / r + p.wg - 1) / p.wg) * r);
        }
        EXPECT(prod == n && p.radices.size() >= 2 && p.radices.size() <= 4, "hx n=%lld radices", n);
        if (p.hx_pair != 0) continue;  // (checked below)
        EXPECT(p.fpw == 1 && p.staged == 0 && p.wg % 64 == 0 && p.wg >= 512 && p.wg <= 1024, "hx n=%lld lanes %d", n, p.wg);
        EXPECT(pfa::hx_lds_bytes(p) <= max_lds && static_cast<size_t>(n) * es > 152 * 1024, "hx n=%lld LDS", n);
        const int budget = 512 / ((p.wg / 64 + 3) / 4);
        EXPECT(regs * (prec ? 4 : 2) < budget && p.regs == regs, "hx n=%lld: %d elements per lane of %d lanes", n, regs, p.wg);
      }
    }
    std::printf("hx planner: %lld fp32 and %lld fp64 lengths\n", planned_hx[0], planned_hx[1]);
    EXPECT(planned_hx[0] > 300 && planned_hx[1] > 150, "hx planner coverage");
    EXPECT(!pfa::choose_hx_params(0, 40960, max_lds, &p0) , "40960: 80 values per lane do not pay");
    pfa::wg_params p;
    // 80 ... 152 KiB: TWO register-resident work-groups per CU (half the LDS, half the registers each), three passes
    // behind a first radix >= 15 with a conflict-free scatter (odd, or even and padded with its own period) -- or the
    // packed planner's LDS-resident kernel
    long long pairs[2] = {0, 0};
    for (int prec = 0; prec < 2; ++prec) {
      const int es = prec ? 16 : 8;
      for (long long n = 80 * 1024 / es - 100; n <= (prec ? 10240 : 19000); ++n) {
        pfa::wg_params q;
        if (!pfa::choose_hx_params(prec, n, max_lds, &q)) continue;
        ++pairs[prec];
        EXPECT(static_cast<size_t>(n) * es > 80 * 1024 && q.hx_pair == 1, "hx pair n=%lld", n);
        EXPECT(q.radices.size() <= 3 && q.radices[0] >= 15 && q.pads == (q.radices[0] % 2 == 0 ? q.radices[0] : 0),
               "hx pair n=%lld: three passes, an even first radix padded", n);
        EXPECT(q.wg >= 256 && q.wg <= 512 && q.wg % 64 == 0 && 2 * pfa::hx_lds_bytes(q) <= max_lds, "hx pair n=%lld: lanes %d", n, q.wg);
        const int budget = 512 / ((2 * (q.wg / 64) + 3) / 4);
        EXPECT(q.regs * (prec ? 4 : 2) < budget && q.occ == (2 * (q.wg / 64) + 3) / 4, "hx pair n=%lld: %d values per lane", n, q.regs);
      }
    }
    std::printf("hx planner: %lld fp32 and %lld fp64 lengths as pairs\n", pairs[0], pairs[1]);
    EXPECT(pairs[0] > 100 && pairs[1] > 50, "hx pair coverage");
    EXPECT(pfa::choose_hx_params(0, 16384, max_lds, &p) && p.hx_pair == 1 && p.wg == 512, "fp32 16384: two work-groups per CU");
    EXPECT(!pfa::choose_hx_params(0, 18000, max_lds, &p), "fp32 18000: no three-pass pair plan, LDS-resident");
    EXPECT(!pfa::choose_hx_params(0, 8192, max_lds, &p), "fp32 8192: the LDS-resident kernel has two work-groups per CU itself");
    EXPECT(pfa::choose_hx_params(0, 20480, max_lds, &p), "fp32 20480: the top of the LDS range goes register-resident");
    EXPECT(!pfa::choose_hx_params(1, 10240, max_lds, &p), "fp64 10240 stays LDS-resident");
    EXPECT(pfa::choose_hx_params(1, 6144, max_lds, &p) && p.hx_pair == 1 && p.wg == 256, "fp64 6144: two work-groups per CU");
    EXPECT(!pfa::choose_hx_params(0, 65536, max_lds, &p), "65536 does not fit the registers");
    EXPECT(pfa::choose_hx_params(0, 32768, max_lds, &p) && p.radices.size() == 3, "fp32 32768 in three passes");
    EXPECT(pfa::choose_hx_params(1, 16384, max_lds, &p) && p.radices.size() <= 4, "fp64 16384");
  }
  {
    // register-resident strided plans (strided_hx_candidates): only for groups that would sit alone on their CU, a half
    // image that lets the planned number of work-groups share the CU's LDS, lanes inside the register budget
    long long planned[2] = {0, 0};
    for (int prec = 0; prec < 2; ++prec) {
      const int es = prec ? 16 : 8;
      for (long long n : {104LL, 256LL, 512LL, 600LL, 625LL, 660LL, 720LL, 768LL, 800LL, 1000LL, 1024LL, 1100LL, 1536LL, 1944LL, 2000LL, 2048LL}) {
        pfa::wg_params b;
        if (!pfa::choose_strided_params(prec, n, 4096, max_lds, &b, false, prec ? 8 : 16)) continue;
        const std::vector<pfa::wg_params> c = pfa::strided_hx_candidates(b, max_lds);
        const size_t full = static_cast<size_t>(n) * b.fpw * es;
        EXPECT(full > 80 * 1024 || c.empty(), "strided hx n=%lld: a group of %zu bytes has two work-groups per CU already", n, full);
        for (const pfa::wg_params& q : c) {
          ++planned[prec];
          long long prod = 1;
          for (int r : q.radices) prod *= r;
          EXPECT(prod == n && q.fpw == b.fpw && q.hx_strided >= 2 && q.hx_strided <= 4, "strided hx n=%lld: same group, 2 ... 4 per CU", n);
          EXPECT(static_cast<size_t>(q.hx_strided) * pfa::strided_hx_lds_bytes(q) <= max_lds, "strided hx n=%lld: LDS of %d work-groups", n, q.hx_strided);
          EXPECT(pfa::strided_hx_lds_bytes(q) < full * 3 / 4, "strided hx n=%lld: the image is about half of the group", n);
          const int waves = (q.wg + 63) / 64, wps = (q.hx_strided * waves + 3) / 4;
          EXPECT(q.wg <= 1024 && q.wg % q.fpw == 0 && q.occ == wps && q.regs * (prec ? 4 : 2) < 512 / wps,
                 "strided hx n=%lld: %d lanes, %d values per lane", n, q.wg, q.regs);
          EXPECT(prec == 1 || q.hx_strided * waves >= 14, "strided hx n=%lld: fp32 plans keep 14 waves on the CU", n);
        }
      }
    }
    std::printf("strided hx planner: %lld fp32 and %lld fp64 candidate plans\n", planned[0], planned[1]);
    EXPECT(planned[0] >= 4 && planned[1] >= 3, "strided hx coverage");
    {
      pfa::wg_params b;
      EXPECT(pfa::choose_strided_params(0, 1000, 4096, max_lds, &b, false, 16) && pfa::strided_hx_candidates(b, max_lds).empty(),
             "fp32 1000 x 16: 16000 values do not fit two work-groups' registers beside ~62 of overhead -- LDS-resident");
    }
  }
  {
    // WIDE groups (choose_strided_wide_base + strided_hx_candidates(..., wide)): a full-width group of a length beyond the LDS, one
    // work-group per CU on a half image that fits the CU's LDS, values + overhead inside the wave's register budget
    long long planned[2] = {0, 0};
    for (int prec = 0; prec < 2; ++prec) {
      const int es = prec ? 16 : 8, fpw = prec ? 8 : 16;
      for (long long n : {1024LL, 1280LL, 1536LL, 1944LL, 2000LL, 2048LL, 3072LL, 4096LL}) {
        pfa::wg_params b;
        if (!pfa::choose_strided_wide_base(prec, n, fpw, &b)) continue;
        const std::vector<pfa::wg_params> c = pfa::strided_hx_candidates(b, max_lds, true);
        const size_t full = static_cast<size_t>(n) * fpw * es;
        EXPECT(full > 128 * 1024 || c.empty(), "wide strided hx n=%lld: a group of %zu bytes fits the LDS", n, full);
        EXPECT(n <= 2048 || c.empty(), "wide strided hx n=%lld: more than 32 values per lane on 1024 lanes", n);
        for (const pfa::wg_params& q : c) {
          ++planned[prec];
          long long prod = 1;
          for (int r : q.radices) prod *= r;
          EXPECT(prod == n && q.fpw == fpw && q.hx_strided == 1, "wide strided hx n=%lld: the same group, one per CU", n);
          EXPECT(pfa::strided_hx_lds_bytes(q) + 4096 <= max_lds, "wide strided hx n=%lld: LDS", n);
          const int waves = (q.wg + 63) / 64, wps = (waves + 3) / 4;
          EXPECT(q.wg <= 1024 && q.wg % q.fpw == 0 && q.occ == wps && q.regs * (prec ? 4 : 2) < 512 / wps,
                 "wide strided hx n=%lld: %d lanes, %d values per lane", n, q.wg, q.regs);
        }
      }
    }
    {
      // the planner's own radices of 2000 (10.8.5.5) hold 40 values per lane on 64 lanes per transform: the base takes the set with the
      // narrowest widest pass instead (16.5.5.5: 35)
      pfa::wg_params b;
      EXPECT(pfa::choose_strided_wide_base(0, 2000, 16, &b) && b.radices == std::vector<int>({16, 5, 5, 5}), "wide base of 2000: 16.5.5.5");
      const std::vector<pfa::wg_params> c = pfa::strided_hx_candidates(b, max_lds, true);
      EXPECT(!c.empty() && c[0].regs == 35 && c[0].wg >= 960, "wide plan of 2000: 35 values per lane on ~1000 lanes");
      // a group that fits the LDS is no wide group; neither is one of more than 36 values per lane
      EXPECT(pfa::choose_strided_wide_base(0, 1000, 16, &b) && pfa::strided_hx_candidates(b, max_lds, true).empty(), "1000 x 16 fits the LDS");
      EXPECT(pfa::choose_strided_wide_base(0, 4096, 16, &b) && pfa::strided_hx_candidates(b, max_lds, true).empty(), "4096 x 16: 64 values per lane");
    }
    std::printf("wide strided hx planner: %lld fp32 and %lld fp64 candidate plans\n", planned[0], planned[1]);
    EXPECT(planned[0] >= 3 && planned[1] >= 4, "wide strided hx coverage");
  }
  if (argc > 1 && std::string(argv[1]) == "compile") {
    using F = pfa::jit_form;  // {family, split, half, stw, split_mode, tin, big, row_out}
    const F strided_plain{pfa::JF_STRIDED}, strided_big{pfa::JF_STRIDED, false, false, 0, 0, false, true};
    const F hx_plain{pfa::JF_STRIDED_HX}, hx_stw{pfa::JF_STRIDED_HX, false, false, 1};
    const F hx_big{pfa::JF_STRIDED_HX, false, false, 0, 0, false, true};
    auto compiles = [&](const char* what, long long n, const F& form, const pfa::wg_params& q) {
      size_t bytes = 0;
      std::string why;
      const std::string cfg = pfa::wg_cfg_type_name(q);
      const bool built = pfa::jit_compile_only(form, cfg, "gfx950", &bytes, &why);
      const std::string expr = pfa::jit_instantiation(form, "CFG").expr[0];
      EXPECT(built && bytes > 1000, "hiprtc %sn=%lld %s: %s", what, n, expr.c_str(), why.c_str());
      std::printf("hiprtc %sn=%lld %s %s: %zu bytes\n", what, n, expr.c_str(), cfg.c_str(), bytes);
    };
    for (auto c : std::vector<std::pair<int, long long>>{{0, 2048}, {1, 2048}, {0, 1536}}) {
      pfa::wg_params b;
      EXPECT(pfa::choose_strided_wide_base(c.first, c.second, c.first ? 8 : 16, &b), "wide base %lld", c.second);
      const std::vector<pfa::wg_params> cand = pfa::strided_hx_candidates(b, max_lds, true);
      EXPECT(!cand.empty(), "wide strided hx plan %lld", c.second);
      if (!cand.empty()) compiles("wide ", c.second, hx_plain, cand[0]);
    }
    for (auto c : std::vector<std::pair<int, long long>>{{0, 660}, {1, 660}, {0, 768}}) {
      pfa::wg_params b;
      EXPECT(pfa::choose_strided_params(c.first, c.second, 4096, max_lds, &b, false, c.first ? 8 : 16), "strided plan %lld", c.second);
      const std::vector<pfa::wg_params> cand = pfa::strided_hx_candidates(b, max_lds);
      EXPECT(!cand.empty(), "strided hx plan %lld", c.second);
      if (cand.empty()) continue;
      compiles("", c.second, hx_plain, cand[0]);
      compiles("", c.second, hx_stw, cand[0]);
      if (c.first == 0 && c.second == 660) compiles("", c.second, hx_big, cand[0]);  // (BIG: 64-bit butterfly-leg offsets)
    }
    for (auto c : std::vector<std::pair<int, long long>>{{0, 24576}, {0, 30000}, {1, 12000}, {1, 15000}}) {
      pfa::wg_params q;
      EXPECT(pfa::choose_hx_params(c.first, c.second, max_lds, &q), "hx plan %lld", c.second);
      compiles("", c.second, F{pfa::JF_PACKED_HX}, q);
      compiles("", c.second, F{pfa::JF_PACKED_HX, true}, q);
    }
    struct { int prec; long long n; F form; } cases[] = {
        {0, 1200, F{pfa::JF_PACKED}}, {1, 625, F{pfa::JF_PACKED, true}}, {0, 30, F{pfa::JF_PACKED}},
        {0, 30, F{pfa::JF_UNPACKED}}, {0, 30, F{pfa::JF_UNPACKED, true}},
        {0, 120, strided_plain}, {0, 120, strided_big}, {1, 250, F{pfa::JF_STRIDED, false, false, 2, 2}},
        {0, 1000, F{pfa::JF_ROWS2D}}, {1, 768, F{pfa::JF_ROWS2D}},
        // forms of the three-stage / tiled plans that exist only at run time
        {0, 128, F{pfa::JF_STRIDED, false, false, 1, 1}}, {1, 1024, F{pfa::JF_STRIDED, false, false, 0, 3, true}},
        {0, 1024, F{pfa::JF_STRIDED, false, false, 0, 0, true}},
        // row-staged forms (fp32 only; jit_strided_ensure_row): row in, row out, row in of the mixed stage B
        {0, 128, F{pfa::JF_STRIDED_ROW}}, {0, 128, F{pfa::JF_STRIDED_ROW, false, false, 0, 0, false, false, true}},
        {0, 128, F{pfa::JF_STRIDED_ROW, false, false, 0, 3}}};
    for (auto& c : cases) {
      pfa::wg_params q;
      const pfa::jit_family fam = c.form.family;
      const bool ok = fam == pfa::JF_PACKED || fam == pfa::JF_UNPACKED ? pfa::choose_spec_params(c.prec, c.n, max_lds, &q)
                      : fam == pfa::JF_ROWS2D ? pfa::choose_rows2d_params(c.prec, c.n, 1200, max_lds, &q)
                                              : pfa::choose_strided_params(c.prec, c.n, 1024, max_lds, &q, false,
                                                                           c.form.tin ? (c.prec ? 8 : 16) : 0);
      EXPECT(ok, "plan %lld", c.n);
      if (fam == pfa::JF_STRIDED_ROW) q.twl = 0;  // (as jit_strided_ensure_row: the twiddles stay in the global table)
      compiles("", c.n, c.form, q);
    }
  }
  // fused N-D tier: fits-in-LDS rule, pass products, and (with "compile") the nd kernel templates under hiprtc
  {
    struct { int prec; std::vector<long long> dims; bool ok; } shapes[] = {
        {0, {64, 64}, true}, {1, {16, 16, 16}, true}, {0, {30, 50}, true}, {0, {128, 128}, true},
        {1, {128, 128}, false}, {0, {67, 8}, false},  {0, {4, 1, 8}, true}, {0, {256, 128}, false}};
    for (auto& sh : shapes) {
      pfa::nd_kernel nk;
      const bool ok = pfa::choose_nd_params(sh.prec, sh.dims, max_lds, &nk);
      EXPECT(ok == sh.ok, "nd shape %lldx%lld.. planned=%d", sh.dims[0], sh.dims[1], int(ok));
      if (!ok) continue;
      long long tot = 1;
      for (size_t d = 0; d < sh.dims.size(); ++d) {
        long long pd = 1;
        for (int r : nk.radices[d]) pd *= r;
        EXPECT(pd == sh.dims[d], "nd dim product");
        tot *= sh.dims[d];
      }
      EXPECT(nk.k.n == tot && nk.k.wg % nk.k.fpw == 0 && nk.k.wg <= 1024 && nk.k.lds_bytes <= 160 * 1024,
             "nd kernel shape n=%d wg=%d fpw=%d lds=%zu", nk.k.n, nk.k.wg, nk.k.fpw, nk.k.lds_bytes);
      if (argc > 1 && std::string(argv[1]) == "compile" && tot >= 512 && tot <= 4096) {
        size_t bytes = 0;
        std::string why;
        const bool built = pfa::jit_compile_only(pfa::jit_form{pfa::JF_ND, sh.prec == 1}, pfa::nd_cfg_type_name(nk), "gfx950", &bytes, &why);
        EXPECT(built && bytes > 1000, "hiprtc nd: %s", why.c_str());
        std::printf("hiprtc nd %s: %zu bytes\n", pfa::nd_cfg_type_name(nk).c_str(), bytes);
      }
    }
  }
  // measured planning (PFFT_PLAN_MEASURE): the candidates start with the planner's own choice, each is a valid plan of
  // the length, and a recorded choice (process table / cache directory) is found again and honoured by the planner
  {
    for (long long n : {3000ll, 6000ll, 10080ll, 625ll, 15625ll}) {
      pfa::wg_params base;
      EXPECT(pfa::choose_spec_params(0, n, max_lds, &base), "n=%lld planned", n);
      const auto cands = pfa::spec_radix_candidates(0, n, max_lds);
      EXPECT(!cands.empty() && cands[0] == base.radices, "n=%lld first candidate is the static choice", n);
      EXPECT(cands.size() >= 2 && cands.size() <= 14, "n=%lld %zu candidates", n, cands.size());
      for (const auto& r : cands) {
        long long prod = 1;
        for (int x : r) prod *= x;
        pfa::wg_params q;
        EXPECT(prod == n && pfa::choose_spec_params(0, n, max_lds, &q, &r) && q.radices == r &&
                   pfa::spec_lds_bytes(q) <= max_lds,
               "n=%lld candidate", n);
      }
    }
    const std::vector<int> pick = {24, 25, 10};
    EXPECT(pfa::plan_choice_lookup("gfx000", 0, 6000).empty(), "no record yet");
    pfa::plan_choice_store("gfx000", 0, 6000, pick);
    EXPECT(pfa::plan_choice_lookup("gfx000", 0, 6000) == pick, "recorded choice found");
    EXPECT(pfa::plan_choice_lookup("gfx000", 1, 6000).empty() && pfa::plan_choice_lookup("gfx000", 0, 3000).empty(),
           "records are per precision and length");
    pfa::wg_params q;
    EXPECT(pfa::choose_spec_params(0, 6000, max_lds, &q, &pick) && q.radices == pick, "forced radices honoured");
    const std::vector<int> bad = {24, 25, 11};
    EXPECT(pfa::choose_spec_params(0, 6000, max_lds, &q, &bad) && q.radices != bad, "a sequence of another length is ignored");
    {  // lanes per transform behind the radices: "0, lanes"
      const std::vector<int> with_lanes = {16, 61, 0, 16};
      pfa::wg_params w;
      EXPECT(pfa::choose_spec_params(0, 976, max_lds, &w, &with_lanes) && w.radices == std::vector<int>({16, 61}) &&
                 w.wg == 16 * w.fpw,
             "forced lanes honoured: wg %d fpw %d", w.wg, w.fpw);
      pfa::plan_choice_store("gfx000", 0, 976, with_lanes);
      EXPECT(pfa::plan_choice_lookup("gfx000", 0, 976) == with_lanes, "a record with lanes is read back");
      pfa::plan_choice_store("gfx000", 0, 976, {});
    }
    pfa::plan_choice_store("gfx000", 0, 6000, {});  // forget it again: the cache directory may be a shared one
    EXPECT(pfa::plan_choice_lookup("gfx000", 0, 6000).empty(), "record forgotten");
  }
  {  // the tuned table shipped with the library (tuned_gfx950.inc): every entry is a sequence the planner accepts
    int entries = 0;
    for (int prec = 0; prec < 2; ++prec) {
      for (long long n = 2; n <= 1000000; n += (n < 21000 ? 1 : 4)) {
        const std::vector<int> c = pfa::builtin_choice("gfx950", prec, n, false);
        const std::vector<int> sp = pfa::builtin_choice("gfx950", prec, n, true);
        if (!c.empty()) {
          ++entries;
          std::vector<int> rad = c;  // (an entry may end in "0, lanes")
          int lanes = 0;
          if (rad.size() >= 3 && rad[rad.size() - 2] == 0) {
            lanes = rad.back();
            rad.resize(rad.size() - 2);
          }
          long long prod = 1;
          for (int x : rad) prod *= x;
          pfa::wg_params q;
          EXPECT(prod == n && pfa::choose_spec_params(prec, n, max_lds, &q, &c) && q.radices == rad &&
                     (lanes == 0 || q.wg == lanes * q.fpw),
                 "tuned radices of n=%lld prec=%d", n, prec);
        }
        if (!sp.empty()) {
          ++entries;
          EXPECT(sp.size() == 2 && static_cast<long long>(sp[0]) * sp[1] == n, "tuned split of n=%lld", n);
        }
        EXPECT(pfa::builtin_choice("gfx942", prec, n, false).empty() && pfa::builtin_choice("gfx942", prec, n, true).empty(),
               "the table is for gfx950 only");
      }
    }
    setenv("PFFT_NO_TUNED_TABLE", "1", 1);
    EXPECT(pfa::builtin_choice("gfx950", 0, 6000, false).empty() && pfa::builtin_choice("gfx950", 0, 100000, true).empty(),
           "PFFT_NO_TUNED_TABLE=1 turns the table off");
    unsetenv("PFFT_NO_TUNED_TABLE");
    std::printf("tuned table: %d entries checked\n", entries);
  }
  {
    long long compiled = 0, from_disk = 0;
    pfa::jit_stats(&compiled, &from_disk);
    std::printf("jit stats: compiled %lld from_disk %lld\n", compiled, from_disk);
  }
  if (fails == 0) std::printf("jit planner OK\n");
  return fails == 0 ? 0 : 1;
}
