// plan_t: construction, device tables, kernel look-up and the stage builders every planner uses (plan.hpp).
#include "plan.hpp"

#include <hip/hip_ext.h>

namespace pfa {

namespace {
thread_local hipEvent_t g_armed_stop_event = nullptr;
}
void arm_stop_event(hipEvent_t ev) { g_armed_stop_event = ev; }
hipEvent_t take_stop_event() {
  hipEvent_t ev = g_armed_stop_event;
  g_armed_stop_event = nullptr;
  return ev;
}

hipError_t launch_fn(const kernel_fn& f, unsigned grid, unsigned wg, size_t lds, hipStream_t stream, void** params,
                     bool any_order) {
  any_order = any_order && f.any_order;
  if (f.sym != nullptr) {
    hipEvent_t stop = take_stop_event();
    if (stop == nullptr && !any_order) return hipLaunchKernel(f.sym, dim3(grid), dim3(wg), params, lds, stream);
    return hipExtLaunchKernel(f.sym, dim3(grid), dim3(wg), params, lds, stream, nullptr, stop,
                              any_order ? hipExtAnyOrderLaunch : 0);
  }
  if (f.mod == nullptr) return hipErrorInvalidValue;
  // (the Ext entry point takes global sizes in work-items, 32 bits: a larger any-order grid keeps the barrier)
  if (any_order && static_cast<unsigned long long>(grid) * wg >= (1ull << 32)) any_order = false;
  hipEvent_t stop = take_stop_event();
  if (stop == nullptr && !any_order) {
    return hipModuleLaunchKernel(f.mod, grid, 1, 1, wg, 1, 1, static_cast<unsigned>(lds), stream, params, nullptr);
  }
  return hipExtModuleLaunchKernel(f.mod, grid * wg, 1, 1, wg, 1, 1, lds, stream, params, nullptr, nullptr, stop,
                                  any_order ? hipExtAnyOrderLaunch : 0);
}

hipError_t fn_occupancy(int* per_cu, const kernel_fn& f, int wg, size_t lds) {
  if (f.sym != nullptr) return hipOccupancyMaxActiveBlocksPerMultiprocessor(per_cu, f.sym, wg, lds);
  return hipModuleOccupancyMaxActiveBlocksPerMultiprocessor(per_cu, f.mod, wg, lds);
}

hipError_t raise_lds_limit(const kernel_fn& f, size_t lds) {
  if (f.sym == nullptr) return hipSuccess;
  return hipFuncSetAttribute(f.sym, hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds));
}

std::vector<int> tw_offsets(const std::vector<int>& radices) {
  std::vector<int> off(radices.size(), 0);
  long long ns = 1;
  int o = 0;
  for (size_t p = 0; p < radices.size(); ++p) {
    off[p] = o;
    if (p >= 1) o += static_cast<int>(ns) * (radices[p] - 1);
    ns *= radices[p];
  }
  return off;
}

bool generic_radix_ok(int r) {
  switch (r) {
#define PFA_OK(x) case x:
    PFA_GENERIC_RADICES(PFA_OK)
    PFA_GENERIC_RADICES_BIG(PFA_OK)
#undef PFA_OK
    return true;
    default:
      return false;
  }
}

/// Factorise n into radices the generic kernel implements; largest radices first (fewest LDS passes).
/// Returns an empty vector when n has a prime factor that is not a supported radix.
std::vector<int> choose_radices(long long n) {
  std::vector<int> r;
  if (n == 1) return {1};
  long long rem = n;
  while (rem > 1) {
    int best = 0;
    for (int c = 16; c >= 2; --c) {
      if (rem % c == 0) {
        best = c;
        break;
      }
    }
    if (best == 0) {
      // prime factors up to the wavefront size: what a wave64 build of the reference takes as one sub-group DFT
      // (/root/reference/src/portfft/common/subgroup.hpp:226-253)
      for (int c : {17, 19, 23, 29, 31, 37, 41, 43, 47, 53, 59, 61}) {
        if (rem % c == 0) best = c;
      }
    }
    if (best == 0 || !generic_radix_ok(best)) return {};
    // avoid a trailing tiny radix: 16 * 2 -> 8 * 4
    r.push_back(best);
    rem /= best;
  }
  if (r.size() >= 2 && r.back() == 2 && r[r.size() - 2] == 16) {
    r[r.size() - 2] = 8;
    r.back() = 4;
  }
  if (static_cast<int>(r.size()) > GENERIC_MAX_PASSES) return {};
  return r;
}

/// The environment, once per commit (plan.hpp: plan_knobs).  The order of this table is the bit order of `mask`.
plan_knobs plan_knobs::from_env() {
  plan_knobs k;
  int bit = 0;
  auto set = [](const char* name) -> const char* {
    const char* e = getenv(name);
    return e;
  };
  auto mark = [&](bool differs) {
    if (differs) k.mask |= 1ull << bit;
    ++bit;
  };
  auto flag = [&](const char* name, bool* dst) {  // present = the alternative
    *dst = set(name) != nullptr;
    mark(*dst);
  };
  auto onoff = [&](const char* name, bool* dst) {  // default on; "0" switches off
    const char* e = set(name);
    const bool def = *dst;
    if (e != nullptr && e[0] != '\0') *dst = std::atoi(e) != 0;
    mark(*dst != def);
  };
  flag("PFFT_NO_PRECOMPILED", &k.no_precompiled);
  flag("PFFT_XLANE", &k.xlane);
  flag("PFFT_NO_REGRES", &k.no_regres);
  flag("PFFT_NO_LTW", &k.no_ltw);
  flag("PFFT_NO_STW_ROWISH", &k.no_stw_rowish);
  flag("PFFT_JIT_SPEC_RADICES", &k.jit_spec_radices);
  flag("PFFT_NO_MIXED_ROWS", &k.no_mixed_rows);
  flag("PFFT_NO_THREE_STAGE", &k.no_three_stage);
  flag("PFFT_NO_TILED_SCRATCH", &k.no_tiled_scratch);
  flag("PFFT_NO_TILED_LANES", &k.no_tiled_lanes);
  flag("PFFT_TIN_ROWS", &k.tin_rows_gone);  // (no effect any more; keeps the bit order of `mask`)
  flag("PFFT_NO_XCD_LOCAL", &k.no_xcd_local);
  flag("PFFT_ND_TWO_STAGE_COLUMNS", &k.nd_two_stage_columns);
  flag("PFFT_NO_FS_PAIRS", &k.no_fs_pairs);
  flag("PFFT_NO_HALF_PAIRS", &k.no_half_pairs);
  flag("PFFT_NO_SPLIT_RULE", &k.no_split_rule);
  flag("PFFT_NO_SPLIT_TILED", &k.no_split_tiled);
  flag("PFFT_NO_WIDE_TILES", &k.no_wide_tiles);
  onoff("PFFT_SPLIT_CACHED", &k.split_cached);
  onoff("PFFT_PAIR_XCD", &k.pair_xcd);
  onoff("PFFT_STOP_EVENT_ON_LAUNCH", &k.stop_event_on_launch);
  onoff("PFFT_XCD_CHECK", &k.xcd_check);
  if (const char* e = set("PFFT_2D_TWO_PASS")) k.two_pass_2d_off = e[0] == '0';
  mark(k.two_pass_2d_off);
  if (const char* e = set("PFFT_JIT_VERBOSE")) k.jit_verbose = e[0] != '\0' && e[0] != '0';
  mark(k.jit_verbose);
  if (const char* e = set("PFFT_DEBUG_GLOBAL")) {
    k.debug_global_set = true;
    k.debug_global = e;
  }
  mark(k.debug_global_set);
  if (const char* e = set("PFFT_GLOBAL_LAYOUT")) k.global_layout = e;
  mark(!k.global_layout.empty());
  if (const char* e = set("PFFT_GLOBAL_N1")) {
    k.global_n1_set = true;
    k.global_n1 = std::atoll(e);
  }
  mark(k.global_n1_set);
  if (const char* e = set("PFFT_CHUNK_OVERLAP")) {
    if (e[0] != '\0') k.chunk_overlap = std::atoi(e);
  }
  mark(k.chunk_overlap != 2);
  if (const char* e = set("PFFT_JIT_GROUPS_PER_WG")) k.jit_groups_per_wg = std::atoi(e);
  mark(k.jit_groups_per_wg >= 0);
  if (const char* e = set("PFFT_GROUPS_PER_WG")) {
    k.groups_per_wg_set = true;
    k.groups_per_wg = std::atoi(e);
  }
  mark(k.groups_per_wg_set);
  if (const char* e = set("PFFT_GLOBAL_CHUNK_MIB")) {
    k.global_chunk_mib_set = true;
    k.global_chunk_mib = std::atol(e);
  }
  mark(k.global_chunk_mib_set);
  if (const char* e = set("PFFT_CACHE_CHUNK_MIB")) {
    k.cache_chunk_mib_set = true;
    k.cache_chunk_mib = std::atol(e);
  }
  mark(k.cache_chunk_mib_set);
  if (const char* e = set("PFFT_ROW_IN_MAX_N")) k.row_in_max_n = std::atoi(e);
  mark(k.row_in_max_n != 512);
  if (const char* e = set("PFFT_THREE_STAGE_MIN")) k.three_stage_min = std::atoll(e);
  mark(k.three_stage_min > 0);
  if (const char* e = set("PFFT_THREE_STAGE_N3")) k.three_stage_n3 = std::atoll(e);
  mark(k.three_stage_n3 != 0);
  if (const char* e = set("PFFT_XCD_MIN_BATCH")) k.xcd_min_batch = std::atoll(e);
  mark(k.xcd_min_batch >= 0);
  if (const char* e = set("PFFT_XCD_SLOTS")) k.xcd_slots = std::atoi(e);
  mark(k.xcd_slots > 0);
  if (const char* e = set("PFFT_XCD_LAG")) k.xcd_lag = std::atoi(e);
  mark(k.xcd_lag > 0);
  if (const char* e = set("PFFT_XCD_MAX_ITERS")) k.xcd_max_iters = std::atoll(e);
  mark(k.xcd_max_iters >= 0);
  onoff("PFFT_XCD_CONTIG", &k.xcd_contig);
  onoff("PFFT_HX_OVER_REGISTERED", &k.hx_over_registered);
  flag("PFFT_NO_SPLIT_2D_CACHED", &k.no_split_2d_cached);
  if (const char* e = set("PFFT_BI_N1")) k.bi_n1 = std::atoll(e);
  mark(k.bi_n1 > 0);
  flag("PFFT_NO_BI_N1_RULE", &k.no_bi_n1_rule);
  flag("PFFT_NO_BIG_BI", &k.no_big_bi);
  flag("PFFT_NO_BI_WIDE", &k.no_bi_wide);
  flag("PFFT_NO_BI_WIDE_SPLIT2", &k.no_bi_wide_split2);
  if (const char* e = set("PFFT_BI_WIDE_FPW")) k.bi_wide_fpw = std::atoi(e);
  mark(k.bi_wide_fpw > 0);
  flag("PFFT_NO_UNALIGNED_POLICY", &k.no_unaligned_policy);
  flag("PFFT_NO_SPLIT_UNALIGNED_POLICY", &k.no_split_unaligned_policy);
  return k;
}

plan_t::~plan_t() {
  (void)hipStreamSynchronize(stream);
  if (aux_stream != nullptr) {
    (void)hipStreamSynchronize(aux_stream);
    (void)hipStreamDestroy(aux_stream);
  }
  for (hipEvent_t e : chunk_events) (void)hipEventDestroy(e);
  if (scratch != nullptr) (void)hipFree(scratch);
  if (alias_scratch != nullptr) (void)hipFree(alias_scratch);
  if (xcd_ctl != nullptr) (void)hipFree(xcd_ctl);
  if (xcd_tmap != nullptr) (void)hipFree(xcd_tmap);
  if (xcd_report != nullptr) (void)hipHostFree(xcd_report);
}

/// the control block of the XCD-local launch: all zero before its first launch (the kernel keeps it that way)
void plan_t::alloc_xcd_ctl() {
  if (xcd_ctl_bytes == 0 || xcd_ctl != nullptr) return;
  hip_check(hipMalloc(&xcd_ctl, xcd_ctl_bytes), "hipMalloc(control block)");
  // On the plan's own stream and waited for.  hipMemset is not: it returns before the fill has run, the fill sits on
  // the null stream, and a launch on a non-blocking stream does not wait for it -- with more host threads than
  // hardware queues the fill was seen to land in the middle of the plan's first launch
  // (tests/cpp/multi_device_test.cpp with MDT_THREADS=8: counters back at zero, hand-off waits that never end).
  hip_check(hipMemsetAsync(xcd_ctl, 0, xcd_ctl_bytes, stream), "hipMemsetAsync(control block)");
  hip_check(hipMalloc(&xcd_tmap, xcd_tmap_bytes), "hipMalloc(transform records)");
  hip_check(hipMemsetAsync(xcd_tmap, 0, xcd_tmap_bytes, stream), "hipMemsetAsync(transform records)");
  hip_check(hipStreamSynchronize(stream), "hipStreamSynchronize");
  // the copy's host report: what the recovery launch behind a launch that gave up tells the host (pfft_plan_get_info)
  void* r = nullptr;
  hip_check(hipHostMalloc(&r, XCD_REPORT_WORDS * sizeof(unsigned), hipHostMallocPortable | hipHostMallocMapped),
            "hipHostMalloc(report)");
  std::memset(r, 0, XCD_REPORT_WORDS * sizeof(unsigned));
  xcd_report = static_cast<unsigned*>(r);
}

void* plan_t::upload(const void* host, size_t bytes) {
  void* d = nullptr;
  hip_check(hipMalloc(&d, bytes), "hipMalloc(twiddles)");
  tables->ptrs.push_back(d);
  hip_check(hipMemcpy(d, host, bytes, hipMemcpyHostToDevice), "hipMemcpy(twiddles)");
  twiddle_bytes += bytes;
  return d;
}

void* plan_t::upload_twiddles(const std::vector<int>& radices) {
  // (fp16 storage computes in fp32: fp32 tables)
  if (desc.precision == PFFT_PRECISION_F64) {
    auto t = host_twiddles<double>(radices);
    return upload(t.data(), t.size() * sizeof(double));
  }
  auto t = host_twiddles<float>(radices);
  return upload(t.data(), t.size() * sizeof(float));
}

/// fused N-D kernel: the per-dimension tables one after the other, last dimension first (nd_cfg_type_name)
void* plan_t::upload_nd_twiddles(const nd_kernel& nk) {
  auto build = [&](auto tag) {
    using T = decltype(tag);
    std::vector<T> all;
    for (int d = static_cast<int>(nk.dims.size()) - 1; d >= 0; --d) {
      const std::vector<int>& r = nk.radices[static_cast<size_t>(d)];
      if (r.size() < 2) continue;  // a single pass has no twiddles
      const std::vector<T> t = host_twiddles<T>(r);
      all.insert(all.end(), t.begin(), t.end());
    }
    if (all.empty()) all = {T(1), T(0)};
    return upload(all.data(), all.size() * sizeof(T));
  };
  return desc.precision == PFFT_PRECISION_F64 ? build(double{}) : build(float{});
}

/// W_M^m split in two tables (see generic_args::stw_*)
void plan_t::upload_store_twiddles(long long M, int shift, const void** lo, const void** hi) {
  const long long nlo = 1ll << shift;
  const long long nhi = (M + nlo - 1) / nlo + 1;
  auto fill = [&](auto tag, long long count, long long mult) {
    using T = decltype(tag);
    std::vector<T> v(static_cast<size_t>(2 * count));
    for (long long i = 0; i < count; ++i) {
      const long double a = -2.0L * static_cast<long double>(PI_L) * static_cast<long double>((i * mult) % M) /
                            static_cast<long double>(M);
      v[static_cast<size_t>(2 * i)] = static_cast<T>(cosl(a));
      v[static_cast<size_t>(2 * i + 1)] = static_cast<T>(sinl(a));
    }
    return upload(v.data(), v.size() * sizeof(T));
  };
  if (desc.precision == PFFT_PRECISION_F64) {
    *lo = fill(double{}, nlo, 1);
    *hi = fill(double{}, nhi, nlo);
  } else {
    *lo = fill(float{}, nlo, 1);
    *hi = fill(float{}, nhi, nlo);
  }
}

/// levels / shift of the store-modifier tables of an M-point plan behind kernel k's LDS: the fewest levels (fewest
/// multiplies per root) whose tables stay within 16 KiB and do not cost the kernel a resident work-group; failing
/// that the smallest tables (levels of <= 128 entries).  fp32 N <= 2^20: two levels; fp64 N = 2^20: three.
void plan_t::store_table_shape(const strided_kernel* k, long long M, int* levels, int* shift) const {
  int bits = 0;
  while ((1ll << bits) < M) ++bits;
  bits = std::max(bits, 1);
  const size_t cu_lds = 160 * 1024, own = std::max<size_t>(k->lds_bytes, 1);
  const size_t resident = std::min<size_t>(cu_lds / own, 8);
  for (int l = 1; l <= 4; ++l) {
    const int sh = (bits + l - 1) / l;
    const size_t bytes = (static_cast<size_t>(l) << sh) * elem_bytes();
    if (bytes <= 16 * 1024 && k->lds_bytes + bytes <= max_lds && std::min<size_t>(cu_lds / (own + bytes), 8) >= resident) {
      *levels = l;
      *shift = sh;
      return;
    }
  }
  *levels = std::max(1, (bits + 6) / 7);
  *shift = std::max(1, (bits + *levels - 1) / *levels);
}

/// can stage kernel k carry the tables behind its LDS?  (always, for the kernels the planners produce: their own
/// LDS ends at 144 KiB and the smallest tables take at most 8 KiB)
bool plan_t::store_tables_fit(const strided_kernel* k, long long M) const {
  if (k == nullptr) return false;
  if (k->stw_mode != 1) return true;  // two global tables
  int levels = 0, shift = 0;
  store_table_shape(k, M, &levels, &shift);
  return levels <= 4 && k->lds_bytes + (static_cast<size_t>(levels) << shift) * elem_bytes() <= max_lds;
}

/// Store-modifier tables of a strided stage: L tables of 2^shift entries, table l = W_M^(i << (l * shift)), so that
/// W_M^m is the product of one entry per table (stockham_strided.hpp: stw_from_lds).  The kernel copies them behind
/// its own LDS once per work-group (round 1: two L2-resident tables read with scattered gathers).
/// on_loads: the tables of a stage B that carries the modifier on its loads (strided_kernel::fs_ltw; pre-compiled
/// tiled-input form, tables in LDS): the stage keeps store_modifier == 0, its SF_TIN forms get the larger LDS limit.
void plan_t::attach_store_tables(stage& s, long long M, bool on_loads) {
  const strided_kernel* k = s.strided;
  s.store_modifier = on_loads ? 0 : 1;
  if (k->stw_mode != 1 && !on_loads) {  // this kernel's store-modifier forms read two global tables (strided_kernel::stw_mode)
    int sh = 0;
    while ((1ll << (2 * sh)) < M) ++sh;
    upload_store_twiddles(M, sh, &s.sa.stw_lo, &s.sa.stw_hi);
    s.sa.stw_shift = sh;
    return;
  }
  int levels = 0, shift = 0;
  store_table_shape(k, M, &levels, &shift);
  const size_t extra = (static_cast<size_t>(levels) << shift) * elem_bytes();
  s.sa.stw_tab = store_tables_for(M, levels, shift);
  s.sa.stw_levels = levels;
  s.sa.stw_lshift = shift;
  const size_t total = k->lds_bytes + extra;
  finish_store_tables(s, k, total, on_loads);
}

/// device copy of the multi-level tables W_M^(i << (l * shift)), l < levels, i < 2^shift (cached per (M, shift))
const void* plan_t::store_tables_for(long long M, int levels, int shift) {
  auto& slot = store_tables[std::make_pair(M, shift)];
  if (slot == nullptr) {
    const long long per = 1ll << shift;
    auto fill = [&](auto tag) {
      using T = decltype(tag);
      std::vector<T> v(static_cast<size_t>(2 * levels * per));
      for (int l = 0; l < levels; ++l) {
        for (long long i = 0; i < per; ++i) {
          const long long m = static_cast<long long>((static_cast<unsigned long long>(i) << (l * shift)) %
                                                     static_cast<unsigned long long>(M));
          const long double a = -2.0L * static_cast<long double>(PI_L) * static_cast<long double>(m) /
                                static_cast<long double>(M);
          v[static_cast<size_t>(2 * (l * per + i))] = static_cast<T>(cosl(a));
          v[static_cast<size_t>(2 * (l * per + i) + 1)] = static_cast<T>(sinl(a));
        }
      }
      return upload(v.data(), v.size() * sizeof(T));
    };
    slot = desc.precision == PFFT_PRECISION_F64 ? fill(double{}) : fill(float{});
  }
  return slot;
}

void plan_t::finish_store_tables(stage& s, const strided_kernel* k, size_t total, bool on_loads) {
  s.lds_bytes = total;
  // the forms that read the tables get the larger dynamic LDS limit
  for (const kernel_fn& f : k->form[on_loads ? SF_TIN : SF_STW]) {
    if (total > 48 * 1024) hip_check(raise_lds_limit(f, total), "hipFuncSetAttribute");
  }
  if (on_loads) return;
  s.store_modifier = 1;
  // pre-compiled: the grid of the store-modifier form (whatever the stage's storage)
  const kernel_fn& f = k->form[SF_STW][s.backward];
  if (!k->jit && f) s.grid = persistent_grid(f, k->wg, total, strided_groups(s.count, s.sa.inner, k->fpw), k->groups_per_wg);
}

const spec_kernel* plan_t::find_spec(long long n, bool allow_hx) const {
  if (kn.no_precompiled) return nullptr;  // experiments: planner-chosen kernels everywhere
  int count = 0;
  const spec_kernel* k = desc.precision == PFFT_PRECISION_F64   ? spec_kernels_f64(&count)
                         : desc.precision == PFFT_PRECISION_F16 ? spec_kernels_f16(&count)
                                                                : spec_kernels_f32(&count);
  // PFFT_XLANE: prefer the cross-lane variant of a length (measurement / parity of stockham_xlane.hpp; fp16 storage has none)
  const bool want_xlane = kn.xlane && desc.complex_storage == PFFT_INTERLEAVED_COMPLEX;
  const spec_kernel* found = nullptr;
  const bool no_regres = kn.no_regres || !allow_hx;  // A/B twin of the register-resident entries / forms they do not have
  for (int i = 0; i < count; ++i) {
    if (k[i].n != n || k[i].lds_bytes > max_lds || (k[i].hx != 0 && no_regres)) continue;
    if (k[i].xlane != 0) {
      if (want_xlane) return &k[i];
      continue;
    }
    if (found == nullptr) found = &k[i];
  }
  return found;
}

/// column_both: the stage is column-shaped on both sides -> the wide-group entry of the length, when there is one
/// row_side: one side of the stage is row-shaped -> the row-friendly entry of the length, when there is one
/// fs_stage: 1 / 2 = the length's entry for the four-step stage A / B when there is one (strided_kernel::fs_a / fs_b);
/// entries that exist only for such pairs are invisible to every other request
const strided_kernel* plan_t::find_strided(long long n, bool column_both, bool row_side, long long inner_count,
                                           int policy, bool store_modifier, int fs_stage, bool allow_ltw) const {
  int count = 0;
  const strided_kernel* k =
      desc.precision == PFFT_PRECISION_F64 ? strided_kernels_f64(&count) : strided_kernels_f32(&count);
  const strided_kernel* found = nullptr;
  // (stage B: an entry that carries the modifier on its loads first -- PFFT_NO_LTW=1 hides those entries, their
  //  tiled-input form cannot run without the tables)
  const bool ltw_ok = allow_ltw && !kn.no_ltw;
  for (int pass = 0; pass < 2 && fs_stage != 0; ++pass) {
    for (int i = 0; i < count; ++i) {
      if (k[i].n != n || k[i].lds_bytes > max_lds || k[i].policy != policy) continue;
      if (k[i].fs_ltw != 0 && (!ltw_ok || pass == 1)) continue;
      if (pass == 0 && fs_stage == 2 && k[i].fs_ltw == 0) continue;
      if ((fs_stage == 1 && k[i].fs_a != 0) || (fs_stage == 2 && k[i].fs_b != 0)) return &k[i];
    }
  }
  if (fs_stage != 0) return nullptr;
  // (the narrow pair entries are for stages with one contiguous side: with both sides strided -- batch-interleaved
  //  N = 256 -- 16 columns at four work-groups per CU run at 4.3 TB/s against 5.2 for the 64-column entry)
  for (int i = 0; i < count; ++i) {
    if (k[i].n != n || k[i].lds_bytes > max_lds || k[i].policy != policy) continue;
    if (k[i].fs_only != 0) continue;
    if (k[i].wide == 0 && k[i].rowish == 0 && found == nullptr) found = &k[i];
    // wide groups only pay when the stage has that many adjacent columns (surplus lanes would be masked)
    if (k[i].wide != 0 && column_both && (inner_count < 0 || inner_count >= k[i].fpw)) return &k[i];
    // ... which is also the entry for a stage with the store modifier: its last radix is 8 (fp32 n = 1024: 16.8.8
    // against the 32.32 prefetch kernel, whose radix-32 store butterfly holds 32 modifier values next to 32 outputs:
    // four-step N = 2^20 stage A 147 -> 131 us per 256 MiB, 1.128 -> 1.006 ms per GiB)
    if (k[i].rowish != 0 && (row_side || (store_modifier && !kn.no_stw_rowish)) &&
        k[i].lds_bytes_row <= max_lds) {
      return &k[i];
    }
  }
  return found;
}

/// FFTs per work-group of the strided kernel get_strided(n, inner_count, ...) would deliver; 0 when there is none.
/// Cheap: consults the registry and the runtime planner, compiles nothing.
int plan_t::strided_fpw(long long n, long long inner_count) const {
  const strided_kernel* k = find_strided(n);
  if (k != nullptr) return k->fpw;
  wg_params p;
  if (jit_enabled() && choose_strided_params(desc.precision, n, inner_count, max_lds, &p)) return p.fpw;
  return 0;
}

/// the pre-compiled strided kernel when it suits the stage, otherwise a runtime-specialised one (jit.hpp)
/// policy: cache policy of the stage (strided_kernel::policy; 1 writer -- needs store_modifier --, 2 reader)
const strided_kernel* plan_t::get_strided(long long n, long long inner_count, bool store_modifier, bool user_split,
                                          bool column_both, bool row_side, int policy) {
  if (policy == 3 && jit_enabled() && (!user_split || (column_both && !store_modifier && !row_side))) {  // (row-shaped sides too: the row-staged forms are built from this entry)
    // an unaligned row pitch (aux_of_policy): the kernel compiled at commit on default cache policies with the shared group
    // walk, whatever the registry holds for the length (split user planes: batch-interleaved on both sides only)
    std::string why;
    if (const strided_kernel* k = jit_strided_kernel(desc.precision, n, inner_count, store_modifier, user_split ? 1 : 0, max_lds, &why, column_both, policy)) {
      return k;
    }
    jit_note("strided (unaligned pitch)", n, why);
  }
  if (policy == 3) policy = 0;
  // (split user planes: streamed kernels -- unless a registered policy twin carries its split form: the reader of the
  //  two-pass 2-D plan's second pass, the only caller that asks for a policy on user planes)
  if (user_split && policy != 0) {
    const strided_kernel* t = find_strided(n, column_both, false, inner_count, policy, store_modifier);
    if (t == nullptr || !t->form[SF_SPLIT][0]) policy = 0;
  }
  const strided_kernel* k = find_strided(n, column_both, row_side && !user_split, inner_count, policy, store_modifier);
  // A registered entry that sits alone on its CU (128 KiB of LDS) against the register-resident form of the same group, two
  // work-groups per CU (stockham_strided_hx.hpp) -- column-shaped stages without the store modifier.  Measured
  // (profiles/r6_hx_over_registered.txt, r6_bi_two_stage_split.txt): fp64 BI N = 1024 x 8 columns 0.578 -> 0.624, at a batch of
  // 66 000 0.543-0.558 -> 0.586; fp32 BI N = 512 x 32 columns (8.8.8 on 1024 lanes) 0.592 / 0.616 -> 0.660 / 0.685.  NOT fp32 n = 1024:
  // its registered 32.32 software-pipelined kernel on 512 lanes holds 0.60-0.64 against 0.54-0.63.  Hence: fp64, and fp32 where
  // the registered entry is one 16-wave work-group.  Costs that length's first commit one hiprtc compilation (then the disk cache).
  if (k != nullptr && kn.hx_over_registered && (desc.precision == PFFT_PRECISION_F64 || (k->wg >= 1024 && k->n <= 512)) &&
      k->lds_bytes > 80 * 1024 &&
      column_both && !store_modifier && !row_side && !user_split && jit_enabled()) {
    wg_params p;
    if (choose_strided_params(desc.precision, n, inner_count, max_lds, &p, column_both, k->fpw) &&
        !strided_hx_candidates(p, max_lds).empty()) {
      std::string why;
      const strided_kernel* j = jit_strided_kernel(desc.precision, n, inner_count, false, 0, max_lds, &why, column_both, policy, k->fpw);
      if (j != nullptr && j->hx != 0) return j;
    }
  }
  if (k != nullptr) return k;
  if (find_strided(n, column_both, row_side && !user_split, inner_count, 0, store_modifier) != nullptr && policy != 0) {
    return find_strided(n, column_both, row_side && !user_split, inner_count, 0, store_modifier);  // no twin registered
  }
  std::string why;
  k = jit_strided_kernel(desc.precision, n, inner_count, store_modifier, user_split ? 1 : 0, max_lds, &why,
                         column_both, policy);
  if (k == nullptr) jit_note("strided", n, why);
  return k;
}

/// four-step stages on SPLIT_COMPLEX data: split user side, interleaved scratch side (runtime-specialised only)
const strided_kernel* plan_t::get_strided_mixed(long long n, long long inner_count, int split_mode, int policy) {
  std::string why;
  return jit_strided_kernel(desc.precision, n, inner_count, split_mode == 2, split_mode, max_lds, &why, false, policy);
}

/// PFFT_JIT_VERBOSE: say why a configuration stayed on the slower tier
void plan_t::jit_note(const char* what, long long n, const std::string& why) const {
  if (kn.jit_verbose && !why.empty()) {
    std::fprintf(stderr, "[portfft_amd jit] %s n=%lld not specialised: %s\n", what, n, why.c_str());
  }
}

/// the pre-compiled packed kernel, otherwise a runtime-specialised one.  fp16 storage (desc.precision F16) is planned
/// as fp32 -- the planner's rules, the tuned table and the measured choices are the fp32 ones (compute_precision) --
/// while the kernel registries are keyed on F16 (their entries are the converting forms).
const spec_kernel* plan_t::get_spec(long long n) {
  std::string why;
  const int cp = compute_precision();
  const bool split = desc.complex_storage == PFFT_SPLIT_COMPLEX;
  // 80 ... 152 KiB: where the register-resident planner has a two-work-groups-per-CU plan it goes before a registered or
  // tuned LDS-resident kernel of the length (one work-group per CU) -- tools/perf_hx_pairs.py: fp32 12288 0.49 -> 0.62,
  // 13824 0.52 -> 0.64, 14400 0.48 -> 0.60, 15360 0.52 -> 0.66, fp64 6144 0.56 -> 0.72, 6400 0.52 -> 0.67.  (A plan whose kernel
  // does not fit its register budget hands the length back: jit_spec_kernel.)
  if (!kn.no_regres && jit_enabled() && !kn.jit_spec_radices) {
    wg_params q;
    if (choose_hx_params(cp, n, max_lds, &q) && q.hx_pair != 0) {
      const spec_kernel* reg = find_spec(n);
      if (reg != nullptr && reg->hx != 0) return reg;  // a registered register-resident entry is such a plan already
      if (const spec_kernel* k = jit_spec_kernel(desc.precision, n, split, max_lds, &why, false, nullptr, true); k != nullptr && k->hx != 0) {
        return k;
      }
    }
  }
  if (const spec_kernel* k = find_spec(n)) return k;
  if (plan_measure_enabled() && jit_enabled() && !kn.jit_spec_radices) {
    // (fp16: the fp32 record of the length when there is one; nothing is measured on fp16 data)
    const std::vector<int> choice = desc.precision == PFFT_PRECISION_F16 ? plan_choice_lookup(jit_device_arch(), cp, n)
                                                                        : measured_radices(n);
    if (!choice.empty()) {
      if (const spec_kernel* k = jit_spec_kernel(desc.precision, n, split, max_lds, &why, false, &choice)) return k;
    }
  }
  if (jit_enabled() && !kn.jit_spec_radices) {  // the tuned table of this architecture
    const std::vector<int> tuned = builtin_choice(jit_device_arch(), cp, n, false);
    if (!tuned.empty()) {
      if (const spec_kernel* k = jit_spec_kernel(desc.precision, n, split, max_lds, &why, false, &tuned)) return k;
    }
  }
  const spec_kernel* k = jit_spec_kernel(desc.precision, n, split, max_lds, &why, false, nullptr, !kn.no_regres);
  if (k == nullptr) jit_note("packed", n, why);
  return k;
}

/// The entry of a fused form's registry (real_kernels, conv_kernels, ...: kernels.hpp) for `n` points in `precision`
/// whose LDS fits, or nullptr.  A registry holds a (precision, length) once.
static const spec_kernel* find_fused(const spec_kernel* (*registry)(int*), int precision, long long n, size_t max_lds) {
  int count = 0;
  const spec_kernel* r = registry(&count);
  for (int i = 0; i < count; ++i) {
    if (r[i].precision == precision && r[i].n == n && r[i].lds_bytes <= max_lds) return &r[i];
  }
  return nullptr;
}

/// The stage of mode `mode` (stage::backward) of the fused form `form` of `k`: `count` rows of `n` points or scalars (0:
/// the geometry comes with the call); the caller adds the addressing its form has.
static stage fused_stage(const spec_kernel* k, int form, long long n, long long count, int mode, double scale) {
  stage s;
  s.spec = k;
  s.form = form;
  s.n = static_cast<int>(n);
  s.count = count;
  s.backward = mode;
  s.scale = scale;
  return s;
}

/// The real-data kernels of N scalars: the plan the complex planner makes for M = N / 2 points -- registered entry, tuned
/// table, recorded measured choice, static rules, in get_spec's order -- when that plan is an LDS-resident work-group
/// kernel; everything else is refused with the reason.  Nothing complex is compiled on the way (plan_only).
const spec_kernel* plan_t::get_real(long long n) {
  const long long m = n / 2;
  const int cp = compute_precision();
  auto refuse_hx = [&]() {
    fail(PFFT_UNSUPPORTED_CONFIGURATION, "real transform of length ", n, ": its half length ", m,
         " is planned on the register-resident tier (stockham_wg_hx); real transforms need an LDS-resident work-group plan");
  };
  if (!kn.no_regres && jit_enabled() && !kn.jit_spec_radices) {
    wg_params q;
    if (choose_hx_params(cp, m, max_lds, &q) && q.hx_pair != 0) refuse_hx();
  }
  const spec_kernel* like = find_spec(m);
  if (like != nullptr && like->hx != 0) refuse_hx();
  if (like != nullptr) {
    if (const spec_kernel* r = find_fused(real_kernels, cp, m, max_lds)) return r;
  }
  std::string why;
  if (like == nullptr && jit_enabled() && !kn.jit_spec_radices) {
    std::vector<int> choice;
    if (plan_measure_enabled()) choice = plan_choice_lookup(jit_device_arch(), cp, m);
    if (choice.empty()) choice = builtin_choice(jit_device_arch(), cp, m, false);
    if (!choice.empty()) like = jit_spec_kernel(cp, m, false, max_lds, &why, true, &choice);
  }
  if (like == nullptr) like = jit_spec_kernel(cp, m, false, max_lds, &why, true, nullptr, !kn.no_regres);
  if (like == nullptr) {
    fail(PFFT_UNSUPPORTED_CONFIGURATION, "real transform of length ", n, ": its half length ", m,
         " has no one-kernel work-group plan (", why, "); the four-step and generic tiers do not carry real transforms");
  }
  if (like->hx != 0) refuse_hx();
  if (fused_lds_bytes_of(JF_REAL, like) > max_lds) {
    fail(PFFT_UNSUPPORTED_CONFIGURATION, "real transform of length ", n, ": the LDS image of its half length ", m,
         " does not fit");
  }
  const spec_kernel* r = jit_fused_kernel(JF_REAL, like, &why);
  if (r == nullptr) {
    fail(PFFT_UNSUPPORTED_CONFIGURATION, "real transform of length ", n, ": no kernel for its half length ", m, " (", why,
         ")");
  }
  return r;
}

void* plan_t::upload_real_twiddles(const std::vector<int>& radices, long long n) {
  auto build = [&](auto tag) {
    using T = decltype(tag);
    std::vector<T> t = host_twiddles<T>(radices);
    if (radices.size() < 2) t.clear();  // (a single pass has no tables; host_twiddles pads an empty table)
    for (long long k = 0; k <= n / 4; ++k) {
      const long double a = -2.0L * static_cast<long double>(PI_L) * static_cast<long double>(k) / static_cast<long double>(n);
      t.push_back(static_cast<T>(cosl(a)));
      t.push_back(static_cast<T>(sinl(a)));
    }
    return upload(t.data(), t.size() * sizeof(T));
  };
  return desc.precision == PFFT_PRECISION_F64 ? build(double{}) : build(float{});
}

/// Finish the one-kernel fused stage `s` (kernel, form and addressing set) of a real or an any-length plan and append it
/// to `direction`: both directions read the same tables (upload_tables() when the forward stage does not hold them),
/// the LDS limit, the grid, and -- forward -- the plan info of the only dimension.
/// `into` (a convolution stage): the list the stage goes to instead of the direction's -- the plan info stays the ordinary
/// plan's, and upload_tables() decides what is shared.
void plan_t::push_fused_stage(stage s, int direction, const std::function<void*()>& upload_tables,
                              std::vector<stage>* into) {
  const spec_kernel* k = s.spec;
  const kernel_fn& f = k->cells(s.form)[s.backward];
  s.lds_bytes = k->lds_bytes;
  const bool shared = into == nullptr && !stages[0].empty() && stages[0][0].spec == k;
  s.tw = shared ? stages[0][0].tw : upload_tables();
  if (k->lds_bytes > 48 * 1024) hip_check(raise_lds_limit(f, k->lds_bytes), "hipFuncSetAttribute");
  if (s.form == WF_OLS || s.form == WF_ROLS || s.form == WF_STFT || s.form == WF_ISTFT || s.form == WF_DCT || s.form == WF_DCT4 || s.form == WF_IMDCT || s.form == WF_PERIODOGRAM || s.form == WF_PAIRS) {  // the groups come with the call (plan_t::filter_signals, plan_t::stft, plan_t::istft, plan_t::dct, plan_t::dct4, plan_t::mdct, plan_t::imdct, plan_t::periodogram, plan_t::pairs: grid_of); commit keeps the capacity
    s.grid = static_cast<unsigned>(std::min<long long>(resident_groups(f, k->wg, k->lds_bytes), 1ll << 30));
  } else {
    s.grid = persistent_grid(f, k->wg, k->lds_bytes, (s.count + k->fpw - 1) / k->fpw, k->groups_per_wg);
  }
  if (into != nullptr) {
    into->push_back(s);
    return;
  }
  stages[direction].push_back(s);
  if (direction == PFFT_FORWARD) {
    pfft_dim_info_t& di = info.dims[0];
    di.length = static_cast<uint64_t>(s.n);
    record_dim(&di, PFFT_TIER_WORKGROUP, radices_of(k), k->wg, k->fpw, k->lds_bytes);  // (any-length: their product is P, not N)
  }
}

void record_dim(pfft_dim_info_t* info, int tier, const std::vector<int>& factors, int wg, int fpw, size_t lds) {
  if (info == nullptr) return;
  info->tier = tier;
  info->n_factors = static_cast<int>(std::min<size_t>(factors.size(), PFFT_MAX_FACTORS));
  for (int i = 0; i < info->n_factors; ++i) info->factors[i] = factors[static_cast<size_t>(i)];
  info->workgroup_size = wg;
  info->ffts_per_workgroup = fpw;
  info->lds_bytes = lds;
}

/// A REAL descriptor (validated: rank 1, even N, unit strides, PACKED): forward = R2C, backward = C2R, one launch each.
/// Offsets and pitches: the forward domain in scalars, the backward domain in complex elements.
void plan_t::plan_real(int direction) {
  const long long n = static_cast<long long>(desc.lengths[0]);
  const long long count = static_cast<long long>(desc.number_of_transforms);
  if (desc.forward_distance >= (1ull << 30) || count * static_cast<long long>(desc.forward_distance) < 0) {
    fail(PFFT_UNSUPPORTED_CONFIGURATION, "real transform: row pitch beyond the kernels' 32-bit range");
  }
  const spec_kernel* k = get_real(n);
  const int backward = direction == PFFT_BACKWARD ? 1 : 0;
  stage s = fused_stage(k, WF_REAL, n, count, backward, backward ? desc.backward_scale : desc.forward_scale);
  // in_addr: the forward (real) side, out_addr: the backward (complex) side, whatever the direction
  s.in_addr.offset = static_cast<long long>(desc.forward_offset);
  s.in_addr.dist_inner = static_cast<long long>(desc.forward_distance);
  s.out_addr.offset = static_cast<long long>(desc.backward_offset);
  s.out_addr.dist_inner = static_cast<long long>(desc.backward_distance);
  push_fused_stage(s, direction,
                   [&] { return upload_real_twiddles(std::vector<int>(k->radices, k->radices + k->n_radices), n); });
}

/// The convolution kernels of N points: the plan the complex planner makes for N -- registered entry, tuned table,
/// recorded measured choice, static rules, in get_spec's order -- when that plan is an LDS-resident work-group kernel;
/// everything else is refused with the reason.  Nothing complex is compiled on the way (plan_only).
const spec_kernel* plan_t::get_conv(long long n, const spec_kernel** ols) {
  const int cp = compute_precision();
  auto refuse_hx = [&]() {
    fail(PFFT_UNSUPPORTED_CONFIGURATION, "fused convolution of length ", n,
         ": the length is planned on the register-resident tier (stockham_wg_hx); the fused kernel needs an LDS-resident "
         "work-group plan");
  };
  if (has_large_prime_factor(static_cast<uint64_t>(n))) {
    fail(PFFT_UNSUPPORTED_CONFIGURATION, "fused convolution of length ", n,
         ": the length has a prime factor above 61, the largest radix of any kernel");
  }
  if (!kn.no_regres && jit_enabled() && !kn.jit_spec_radices) {
    wg_params q;
    if (choose_hx_params(cp, n, max_lds, &q) && q.hx_pair != 0) refuse_hx();
  }
  const spec_kernel* like = find_spec(n);
  if (like != nullptr && like->hx != 0) refuse_hx();
  if (like != nullptr) {
    if (const spec_kernel* r = find_fused(conv_kernels, cp, n, max_lds)) {
      if (const spec_kernel* o = find_fused(ols_kernels, cp, n, max_lds)) *ols = o;  // (the same configuration lines)
      return r;
    }
  }
  if (!jit_enabled()) {
    fail(PFFT_UNSUPPORTED_CONFIGURATION, "fused convolution of length ", n,
         ": no pre-compiled kernel of this length, and the runtime compiler is off (PFFT_JIT=0)");
  }
  std::string why;
  if (like == nullptr && !kn.jit_spec_radices) {
    std::vector<int> choice;
    if (plan_measure_enabled()) choice = plan_choice_lookup(jit_device_arch(), cp, n);
    if (choice.empty()) choice = builtin_choice(jit_device_arch(), cp, n, false);
    if (!choice.empty()) like = jit_spec_kernel(cp, n, false, max_lds, &why, true, &choice);
  }
  if (like == nullptr) like = jit_spec_kernel(cp, n, false, max_lds, &why, true, nullptr, !kn.no_regres);
  if (like == nullptr) {
    fail(PFFT_UNSUPPORTED_CONFIGURATION, "fused convolution of length ", n, ": the length has no one-kernel work-group plan (",
         why, "); the four-step and generic tiers do not carry the fused kernel");
  }
  if (like->hx != 0) refuse_hx();
  if (fused_lds_bytes_of(JF_CONV, like) > max_lds) {
    fail(PFFT_UNSUPPORTED_CONFIGURATION, "fused convolution of length ", n, ": its LDS image does not fit");
  }
  const spec_kernel* r = jit_fused_kernel(JF_CONV, like, &why);
  if (r == nullptr) {
    fail(PFFT_UNSUPPORTED_CONFIGURATION, "fused convolution of length ", n, ": no kernel (", why, ")");
  }
  // whatever commits for convolve filters: the same configuration, the same compiler (the row windows of a STAGED
  // configuration are 16 bytes per row behind images of at least as many)
  if (fused_lds_bytes_of(JF_OLS, like) <= max_lds) {  // (else pfft_execute_filter refuses; convolve is not affected)
    *ols = jit_fused_kernel(JF_OLS, like, &why);
    if (*ols == nullptr) {
      fail(PFFT_UNSUPPORTED_CONFIGURATION, "fused convolution of length ", n, ": no overlap-save kernel (", why, ")");
    }
  }
  return r;
}

/// PFFT_EXT_CONVOLUTION (validated: fp32 / fp64, rank 1, interleaved, unit strides, distances >= N), behind the ordinary
/// plan: one WF_CONV stage per mode.  in_addr: the forward domain (input), out_addr: the backward domain (output), in
/// complex elements.  The N-point tables are the ordinary plan's when its one stage reads the same ones.
void plan_t::plan_conv(const spec_kernel* k, const spec_kernel* ols) {
  const long long n = static_cast<long long>(desc.lengths[0]);
  const long long count = static_cast<long long>(desc.number_of_transforms);
  const view_t iv = view_of(desc, PFFT_FORWARD), ov = view_of(desc, PFFT_BACKWARD);
  // the kernel's buffer resources cover the fpw rows of a group with 32-bit byte offsets
  const unsigned long long row_limit = (1ull << 32) / (static_cast<unsigned long long>(k->fpw) * elem_bytes());
  if (std::max(iv.distance, ov.distance) >= row_limit) {
    fail(PFFT_UNSUPPORTED_CONFIGURATION, "fused convolution: row pitch beyond the kernel's 32-bit range (the ", k->fpw,
         " rows of one work-group must span less than 4 GiB: distances below ", row_limit, " elements)");
  }
  const void* tables = nullptr;
  if (stages[0].size() == 1 && stages[0][0].spec != nullptr && !stages[0][0].generic && stages[0][0].tw != nullptr) {
    const spec_kernel* o = stages[0][0].spec;
    if (o->n == k->n && o->n_radices == k->n_radices && std::equal(k->radices, k->radices + k->n_radices, o->radices)) {
      tables = stages[0][0].tw;
    }
  }
  for (int mode = 0; mode < 2; ++mode) {
    stage s = fused_stage(k, WF_CONV, n, count, mode, desc.forward_scale * desc.backward_scale);
    s.in_addr.offset = static_cast<long long>(iv.offset);
    s.in_addr.dist_inner = static_cast<long long>(iv.distance);  // (validated: at least n)
    s.out_addr.offset = static_cast<long long>(ov.offset);
    s.out_addr.dist_inner = static_cast<long long>(ov.distance);
    push_fused_stage(s, PFFT_FORWARD, [&]() -> void* {
      if (tables == nullptr) tables = upload_twiddles(std::vector<int>(k->radices, k->radices + k->n_radices));
      return const_cast<void*>(tables);
    }, &conv_stages);
  }
  // pfft_execute_filter: the geometry comes with the call; commit keeps the kernel, the tables and, as `grid`, the
  // number of groups the device holds at once (push_fused_stage); plan_t::filter_signals applies grid_of to the groups
  // of the call
  for (int mode = 0; ols != nullptr && mode < 2; ++mode) {
    push_fused_stage(fused_stage(ols, WF_OLS, n, 0, mode, desc.forward_scale * desc.backward_scale), PFFT_FORWARD,
                     [&]() -> void* { return const_cast<void*>(conv_stages[0].tw); }, &ols_stages);
  }
}

/// PFFT_EXT_REAL_CONVOLUTION (validated as a real descriptor), behind plan_real in both directions: one WF_RCONV stage
/// and one WF_ROLS stage per mode, of the configuration the real plan runs for M = N / 2 -- the pre-compiled entry of the
/// same configuration line, or the forms compiled at commit from the real plan's own entry -- reading the real plan's
/// tables (the M-point twiddles and w_k behind them).  Whatever plan_real refuses never gets here.
void plan_t::plan_rconv() {
  const spec_kernel* real = stages[0][0].spec;
  const long long n = static_cast<long long>(desc.lengths[0]);
  const spec_kernel *k = nullptr, *rols = nullptr;
  if (!real->jit) {  // (kernels_rconv.hip, kernels_rols.hip: the configuration lines of kernels_real.hip)
    k = find_fused(rconv_kernels, real->precision, real->n, max_lds);
    rols = find_fused(rols_kernels, real->precision, real->n, max_lds);
    if (k == nullptr) fail(PFFT_INTERNAL_ERROR, "real convolution of length ", n, ": no pre-compiled kernel next to the real one");
  } else {
    std::string why;
    k = jit_fused_kernel(JF_RCONV, real, &why);
    if (k == nullptr) fail(PFFT_UNSUPPORTED_CONFIGURATION, "real convolution of length ", n, ": no kernel (", why, ")");
    // (a STAGED configuration whose images leave no room for the row windows commits; pfft_execute_filter then refuses)
    if (fused_lds_bytes_of(JF_ROLS, real) <= max_lds) {
      rols = jit_fused_kernel(JF_ROLS, real, &why);
      if (rols == nullptr) {
        fail(PFFT_UNSUPPORTED_CONFIGURATION, "real convolution of length ", n, ": no overlap-save kernel (", why, ")");
      }
    }
  }
  void* tables = const_cast<void*>(stages[0][0].tw);
  for (int mode = 0; mode < 2; ++mode) {
    stage s = fused_stage(k, WF_RCONV, n, static_cast<long long>(desc.number_of_transforms), mode,
                          desc.forward_scale * desc.backward_scale);
    // input and output: the forward domain, in scalars (plan_real has checked the pitch)
    s.in_addr.offset = s.out_addr.offset = static_cast<long long>(desc.forward_offset);
    s.in_addr.dist_inner = s.out_addr.dist_inner = static_cast<long long>(desc.forward_distance);
    push_fused_stage(s, PFFT_FORWARD, [&]() -> void* { return tables; }, &conv_stages);
  }
  for (int mode = 0; rols != nullptr && mode < 2; ++mode) {
    push_fused_stage(fused_stage(rols, WF_ROLS, n, 0, mode, desc.forward_scale * desc.backward_scale), PFFT_FORWARD,
                     [&]() -> void* { return tables; }, &ols_stages);
  }
}

filter_buf::~filter_buf() {
  if (ptr == nullptr) return;
  int cur = -1;
  const bool switched = hipGetDevice(&cur) == hipSuccess && cur != device && hipSetDevice(device) == hipSuccess;
  (void)hipStreamSynchronize(stream);  // executes submitted with this filter read it until they are done
  (void)hipFree(ptr);
  if (switched) (void)hipSetDevice(cur);
}

void plan_t::set_filter(const void* spectra, unsigned long long n_filters) {
  if (conv_stages.empty()) {
    fail(PFFT_INVALID_CONFIGURATION, "set_filter: the plan was not committed with PFFT_EXT_CONVOLUTION or "
         "PFFT_EXT_REAL_CONVOLUTION");
  }
  if (spectra == nullptr) fail(PFFT_INVALID_CONFIGURATION, "set_filter: null filter pointer");
  if (n_filters == 0 || n_filters > 0xFFFFFFFFull) {
    fail(PFFT_INVALID_CONFIGURATION, "set_filter: invalid number of filters ", n_filters, ", must be 1 ... 2^32 - 1");
  }
  device_guard dg(device);
  refuse_in_capture("set_filter");
  // a real plan: the N / 2 + 1 bins of the half spectrum per filter
  const size_t bins = is_real(desc) ? desc.lengths[0] / 2 + 1 : desc.lengths[0];
  const size_t bytes = static_cast<size_t>(n_filters) * bins * elem_bytes();
  auto fb = std::make_shared<filter_buf>();
  fb->n_filters = static_cast<unsigned>(n_filters);
  fb->stream = stream;
  fb->device = device;
  hip_check(hipMalloc(&fb->ptr, bytes), "hipMalloc(filter)");
  hip_check(hipMemcpyAsync(fb->ptr, spectra, bytes, hipMemcpyDeviceToDevice, stream), "hipMemcpyAsync(filter)");
  filter = std::move(fb);  // (the old buffer goes when its last holder does: filter_buf::~filter_buf)
}

/// The taps of each filter go to the front of a zeroed row of N elements of a new filter buffer, and a short-lived
/// ordinary plan of the same length and precision (n_filters packed rows, scale 1, in place, on the plan's stream)
/// transforms the rows where they lie: the spectra are what pfft_execute(PFFT_FORWARD) makes of the padded taps.
void plan_t::set_filter_taps(const void* taps, unsigned long long n_taps, unsigned long long n_filters) {
  if (conv_stages.empty()) {
    fail(PFFT_INVALID_CONFIGURATION, "set_filter_taps: the plan was not committed with PFFT_EXT_CONVOLUTION or "
         "PFFT_EXT_REAL_CONVOLUTION");
  }
  if (taps == nullptr) fail(PFFT_INVALID_CONFIGURATION, "set_filter_taps: null taps pointer");
  const unsigned long long n = desc.lengths[0];
  if (n_taps == 0 || n_taps > n) {
    fail(PFFT_INVALID_CONFIGURATION, "set_filter_taps: invalid number of taps ", n_taps, ", must be 1 ... ", n,
         " (the length of the descriptor)");
  }
  if (n_filters == 0 || n_filters > 0xFFFFFFFFull) {
    fail(PFFT_INVALID_CONFIGURATION, "set_filter_taps: invalid number of filters ", n_filters, ", must be 1 ... 2^32 - 1");
  }
  device_guard dg(device);
  refuse_in_capture("set_filter_taps");
  // a real plan: real taps, R2C in place on padded rows -- N + 2 scalars each, which are the N / 2 + 1 bins of a filter
  const bool real = is_real(desc);
  pfft_desc_t td = desc;  // (precision, domain, rank 1, interleaved, unit strides: validated with the bit)
  td.extensions = real ? PFFT_EXT_REAL_TRANSFORMS : 0;
  td.placement = PFFT_IN_PLACE;
  td.number_of_transforms = n_filters;
  td.forward_distance = real ? n + 2 : n;
  td.backward_distance = real ? n / 2 + 1 : n;
  td.forward_offset = td.backward_offset = 0;
  td.forward_scale = td.backward_scale = 1.0;
  validate(td);
  const size_t eb = real ? static_cast<size_t>(scalar_bytes()) : elem_bytes();  // of a tap
  const size_t bytes = static_cast<size_t>(n_filters) * td.forward_distance * eb;
  auto fb = std::make_shared<filter_buf>();
  fb->n_filters = static_cast<unsigned>(n_filters);
  fb->n_taps = static_cast<unsigned>(n_taps);
  fb->stream = stream;
  fb->device = device;
  hip_check(hipMalloc(&fb->ptr, bytes), "hipMalloc(filter)");
  hip_check(hipMemsetAsync(fb->ptr, 0, bytes, stream), "hipMemsetAsync(filter)");
  hip_check(hipMemcpy2DAsync(fb->ptr, td.forward_distance * eb, taps, n_taps * eb, n_taps * eb, n_filters, hipMemcpyDeviceToDevice, stream),
            "hipMemcpy2DAsync(taps)");
  {
    plan_t transform(td, stream);
    transform.execute(PFFT_FORWARD, fb->ptr, nullptr, fb->ptr, nullptr);
  }  // (its destructor waits for the stream before its tables go)
  filter = std::move(fb);  // (the old buffer goes when its last holder does: filter_buf::~filter_buf)
}

/// The two stages of a fused form that is resolved after commit, next to the real plan (set_window,
/// set_synthesis_window, prepare_dct, prepare_dct4, set_imdct_window, set_periodogram_window, prepare_pairs): the pre-compiled entry of the real plan's configuration line in `registry`, or
/// the form of `family` compiled from the real plan's own entry (cached like every other form), reading the real plan's
/// tables; stage [0] runs mode 0 with scale0, stage [1] mode 1 with scale1.  Their geometry comes with the call, so they go to no direction's list.
/// `refuse`: raises the verb's own refusal -- refuse(nullptr) when `lds_check` finds that the form's LDS does not fit,
/// refuse(&why) when there is no kernel.
std::vector<stage> plan_t::resolve_next_to_real(const spec_kernel* (*registry)(int*), jit_family family, int form,
                                                double scale0, double scale1, bool lds_check,
                                                const std::function<void(const std::string*)>& refuse) {
  const spec_kernel* real = stages[0][0].spec;
  // (kernels_stft.hip, kernels_istft.hip, kernels_dct.hip, kernels_dct4.hip, kernels_imdct.hip, kernels_periodogram.hip, kernels_pairs.hip: the configuration lines of kernels_real.hip)
  const spec_kernel* k = real->jit ? nullptr : find_fused(registry, real->precision, real->n, max_lds);
  if (k == nullptr) {
    if (lds_check && fused_lds_bytes_of(family, real) > max_lds) refuse(nullptr);
    std::string why;
    k = jit_fused_kernel(family, real, &why);
    if (k == nullptr) refuse(&why);
  }
  void* tables = const_cast<void*>(stages[0][0].tw);
  std::vector<stage> resolved;
  for (int mode = 0; mode < 2; ++mode) {
    push_fused_stage(fused_stage(k, form, static_cast<long long>(desc.lengths[0]), 0, mode, mode ? scale1 : scale0),
                     PFFT_FORWARD, [&]() -> void* { return tables; }, &resolved);
  }
  return resolved;
}

/// A window of the plan: the N scalars (`scalars` of them, when given) of `win` in device memory, or ones for nullptr, copied on the plan's stream into
/// a buffer the plan owns (filter_buf's rules).  `label` names it in a HIP error.
std::shared_ptr<filter_buf> plan_t::upload_window(const void* win, const char* label, unsigned long long scalars) {
  const unsigned long long n = scalars != 0 ? scalars : desc.lengths[0];
  const size_t bytes = static_cast<size_t>(n) * static_cast<size_t>(scalar_bytes());
  const std::string malloc_label = std::string("hipMalloc(") + label + ")", copy_label = std::string("hipMemcpyAsync(") + label + ")";
  auto wb = std::make_shared<filter_buf>();
  wb->stream = stream;
  wb->device = device;
  hip_check(hipMalloc(&wb->ptr, bytes), malloc_label.c_str());
  if (win != nullptr) {
    hip_check(hipMemcpyAsync(wb->ptr, win, bytes, hipMemcpyDeviceToDevice, stream), copy_label.c_str());
  } else {
    const std::vector<double> ones_d(desc.precision == PFFT_PRECISION_F64 ? n : 0, 1.0);
    const std::vector<float> ones_f(desc.precision == PFFT_PRECISION_F64 ? 0 : n, 1.0f);
    const void* host = desc.precision == PFFT_PRECISION_F64 ? static_cast<const void*>(ones_d.data()) : ones_f.data();
    hip_check(hipMemcpyAsync(wb->ptr, host, bytes, hipMemcpyHostToDevice, stream), copy_label.c_str());
    hip_check(hipStreamSynchronize(stream), "hipStreamSynchronize");  // (the host block goes with this call)
  }
  return wb;
}

/// The STFT stages of a real plan are resolved here, at the first window (resolve_next_to_real; commit of a real plan
/// is what it was), with forward_scale.  Then the window is copied into a buffer the plan owns (upload_window).
void plan_t::set_window(const void* win) {
  require_real("set_window");
  device_guard dg(device);
  refuse_in_capture("set_window");
  const unsigned long long n = desc.lengths[0];
  if (stft_stages.empty()) {
    stft_stages = resolve_next_to_real(stft_kernels, JF_STFT, WF_STFT, desc.forward_scale, desc.forward_scale, true,
                                       [&](const std::string* why) {
      if (why == nullptr) {
        fail(PFFT_UNSUPPORTED_CONFIGURATION, "set_window: the row windows of the short-time Fourier transform kernel of "
             "length ", n, " do not fit into LDS behind its images");
      }
      fail(PFFT_UNSUPPORTED_CONFIGURATION, "set_window: no short-time Fourier transform kernel of length ", n, " (", *why, ")");
    });
  }
  window = upload_window(win, "window");  // (the old buffer goes when its last holder does: filter_buf::~filter_buf)
}

/// set_window's twin for the inverse: the stages of the two modes are resolved at the first synthesis window, with
/// backward_scale.  The synthesis window is a buffer of its own.
void plan_t::set_synthesis_window(const void* win) {
  require_real("set_synthesis_window");
  device_guard dg(device);
  refuse_in_capture("set_synthesis_window");
  const unsigned long long n = desc.lengths[0];
  if (istft_stages.empty()) {
    istft_stages = resolve_next_to_real(istft_kernels, JF_ISTFT, WF_ISTFT, desc.backward_scale, desc.backward_scale, true,
                                        [&](const std::string* why) {
      if (why == nullptr) {
        fail(PFFT_UNSUPPORTED_CONFIGURATION, "set_synthesis_window: the overlap-add accumulator of the inverse short-time "
             "Fourier transform kernel of length ", n, " (", n, " scalars) does not fit into LDS behind "
             "its images: ", fused_lds_bytes_of(JF_ISTFT, stages[0][0].spec), " bytes of ", max_lds);
      }
      fail(PFFT_UNSUPPORTED_CONFIGURATION, "set_synthesis_window: no inverse short-time Fourier transform kernel of length ",
           n, " (", *why, ")");
    });
  }
  synthesis_window = upload_window(win, "synthesis window");  // (the old buffer goes as `window`'s does)
}

/// set_window's counterpart for the cosine transforms, without data: the stages of the two types are resolved here -- the
/// pre-compiled entry of the real plan's configuration line (kernels_dct.hip), or the form compiled from the real plan's
/// own entry -- on the real plan's tables, type 2 with forward_scale and type 3 with backward_scale; then the quarter-wave
/// table c_k = exp(-i pi k / (2N)), k = 0 ... M, is computed the way the plan's other twiddles are and uploaded into a
/// buffer the plan owns (filter_buf's rules).  A second call finds both and does nothing.
void plan_t::prepare_dct() {
  require_real("prepare_dct");
  device_guard dg(device);
  refuse_in_capture("prepare_dct");
  if (!dct_stages.empty() && dct_table) return;
  const unsigned long long n = desc.lengths[0], m = n / 2;
  if (dct_stages.empty()) {  // (no LDS check: the real form's LDS -- what fits the real plan fits this)
    dct_stages = resolve_next_to_real(dct_kernels, JF_DCT, WF_DCT, desc.forward_scale, desc.backward_scale, false,
                                      [&](const std::string* why) {
      fail(PFFT_UNSUPPORTED_CONFIGURATION, "prepare_dct: no discrete cosine transform kernel of length ", n, " (", *why, ")");
    });
  }
  auto build = [&](auto tag) {
    using T = decltype(tag);
    std::vector<T> t;
    t.reserve(2 * (m + 1));
    for (unsigned long long k = 0; k <= m; ++k) {
      const long double a = -static_cast<long double>(PI_L) * static_cast<long double>(k) / static_cast<long double>(2 * n);
      t.push_back(static_cast<T>(cosl(a)));
      t.push_back(static_cast<T>(sinl(a)));
    }
    auto tb = std::make_shared<filter_buf>();
    tb->stream = stream;
    tb->device = device;
    const size_t bytes = t.size() * sizeof(T);
    hip_check(hipMalloc(&tb->ptr, bytes), "hipMalloc(dct table)");
    hip_check(hipMemcpyAsync(tb->ptr, t.data(), bytes, hipMemcpyHostToDevice, stream), "hipMemcpyAsync(dct table)");
    hip_check(hipStreamSynchronize(stream), "hipStreamSynchronize");  // (the host block goes with this call)
    return tb;
  };
  dct_table = desc.precision == PFFT_PRECISION_F64 ? build(double{}) : build(float{});
}

/// prepare_dct's twin for the type-4 transforms: the stages of the two cells ([0] rows, [1] MDCT) are resolved here -- the
/// pre-compiled entry of the real plan's configuration line (kernels_dct4.hip), or the form compiled from the real plan's
/// own entry -- on the real plan's tables; their scale is an argument of each call.  Then the table a_n = exp(-i pi (4n + 1) /
/// (4N)), n < M, followed by b_k = exp(-i pi k / N), k < M, is computed in long double and uploaded into a buffer the plan
/// owns (filter_buf's rules).  A second call finds both and does nothing.
void plan_t::prepare_dct4() {
  require_real("prepare_dct4");
  device_guard dg(device);
  refuse_in_capture("prepare_dct4");
  if (!dct4_stages.empty() && dct4_table) return;
  const unsigned long long n = desc.lengths[0], m = n / 2;
  if (dct4_stages.empty()) {  // (no LDS check: the real form's LDS -- what fits the real plan fits this)
    dct4_stages = resolve_next_to_real(dct4_kernels, JF_DCT4, WF_DCT4, desc.forward_scale, desc.forward_scale, false,
                                       [&](const std::string* why) {
      fail(PFFT_UNSUPPORTED_CONFIGURATION, "prepare_dct4: no DCT-IV kernel of length ", n, " (", *why, ")");
    });
  }
  auto build = [&](auto tag) {
    using T = decltype(tag);
    std::vector<T> t;
    t.reserve(4 * m);
    for (unsigned long long k = 0; k < m; ++k) {
      const long double a = -static_cast<long double>(PI_L) * static_cast<long double>(4 * k + 1) / static_cast<long double>(4 * n);
      t.push_back(static_cast<T>(cosl(a)));
      t.push_back(static_cast<T>(sinl(a)));
    }
    for (unsigned long long k = 0; k < m; ++k) {
      const long double a = -static_cast<long double>(PI_L) * static_cast<long double>(k) / static_cast<long double>(n);
      t.push_back(static_cast<T>(cosl(a)));
      t.push_back(static_cast<T>(sinl(a)));
    }
    auto tb = std::make_shared<filter_buf>();
    tb->stream = stream;
    tb->device = device;
    const size_t bytes = t.size() * sizeof(T);
    hip_check(hipMalloc(&tb->ptr, bytes), "hipMalloc(dct4 table)");
    hip_check(hipMemcpyAsync(tb->ptr, t.data(), bytes, hipMemcpyHostToDevice, stream), "hipMemcpyAsync(dct4 table)");
    hip_check(hipStreamSynchronize(stream), "hipStreamSynchronize");  // (the host block goes with this call)
    return tb;
  };
  dct4_table = desc.precision == PFFT_PRECISION_F64 ? build(double{}) : build(float{});
}

/// set_window's twin for the MDCT: what prepare_dct4 does, then the 2N scalars of the window into a buffer of its own;
/// every call uploads again.
void plan_t::set_mdct_window(const void* win) {
  require_real("set_mdct_window");
  device_guard dg(device);
  refuse_in_capture("set_mdct_window");
  prepare_dct4();
  mdct_window = upload_window(win, "mdct window", 2 * desc.lengths[0]);  // (the old buffer goes as `window`'s does)
}

/// set_synthesis_window's twin for the inverse MDCT: what prepare_dct4 does (the kernel reads the type-4 table), then the
/// stages of the form are resolved at the first window, with backward_scale -- the form has one kernel, both stages are
/// it -- and the 2N scalars of the window go into a buffer of its own; every call uploads again.
void plan_t::set_imdct_window(const void* win) {
  require_real("set_imdct_window");
  device_guard dg(device);
  refuse_in_capture("set_imdct_window");
  prepare_dct4();
  const unsigned long long n = desc.lengths[0];
  if (imdct_stages.empty()) {
    imdct_stages = resolve_next_to_real(imdct_kernels, JF_IMDCT, WF_IMDCT, desc.backward_scale, desc.backward_scale, true,
                                        [&](const std::string* why) {
      if (why == nullptr) {
        fail(PFFT_UNSUPPORTED_CONFIGURATION, "set_imdct_window: the carry of the inverse MDCT kernel of length ", n, " (", n / 2,
             " scalars) does not fit into LDS behind its images: ", fused_lds_bytes_of(JF_IMDCT, stages[0][0].spec),
             " bytes of ", max_lds);
      }
      fail(PFFT_UNSUPPORTED_CONFIGURATION, "set_imdct_window: no inverse MDCT kernel of length ", n, " (", *why, ")");
    });
  }
  imdct_window = upload_window(win, "imdct window", 2 * n);  // (the old buffer goes as `window`'s does)
}

/// set_window's twin for the power spectrogram / periodogram: the stages of the two extensions are resolved at the first
/// window, with forward_scale (the sums carry forward_scale squared).  The window is a buffer of its own.
void plan_t::set_periodogram_window(const void* win) {
  require_real("set_periodogram_window");
  device_guard dg(device);
  refuse_in_capture("set_periodogram_window");
  const unsigned long long n = desc.lengths[0];
  if (periodogram_stages.empty()) {
    periodogram_stages = resolve_next_to_real(periodogram_kernels, JF_PERIODOGRAM, WF_PERIODOGRAM, desc.forward_scale,
                                              desc.forward_scale, true, [&](const std::string* why) {
      if (why == nullptr) {
        fail(PFFT_UNSUPPORTED_CONFIGURATION, "set_periodogram_window: the row windows of the periodogram kernel of length ", n,
             " do not fit into LDS behind its images");
      }
      fail(PFFT_UNSUPPORTED_CONFIGURATION, "set_periodogram_window: no periodogram kernel of length ", n, " (", *why, ")");
    });
  }
  periodogram_window = upload_window(win, "periodogram window");  // (the old buffer goes as `window`'s does)
}

/// prepare_dct4's twin for the pair verbs: the stages of the two cells ([PFFT_CONVOLVE] product, [PFFT_CORRELATE]
/// conjugate product) are resolved here -- the pre-compiled entry of the real plan's configuration line
/// (kernels_pairs.hip), or the form compiled from the real plan's own entry -- on the real plan's tables, w_k included;
/// scale and floor are arguments of each call.  Nothing is uploaded.  A second call finds the stages and does nothing.
void plan_t::prepare_pairs() {
  require_real("prepare_pairs");
  device_guard dg(device);
  refuse_in_capture("prepare_pairs");
  if (!pairs_stages.empty()) return;
  const unsigned long long n = desc.lengths[0];
  const double c = desc.forward_scale * desc.forward_scale * desc.backward_scale;
  pairs_stages = resolve_next_to_real(pairs_kernels, JF_PAIRS, WF_PAIRS, c, c, true, [&](const std::string* why) {
    if (why == nullptr) {
      fail(PFFT_UNSUPPORTED_CONFIGURATION, "prepare_pairs: the two image sets of the pair kernel of length ", n,
           " do not fit into LDS: ", fused_lds_bytes_of(JF_PAIRS, stages[0][0].spec), " bytes of ", max_lds);
    }
    fail(PFFT_UNSUPPORTED_CONFIGURATION, "prepare_pairs: no pair kernel of length ", n, " (", *why, ")");
  });
}

namespace {
/// in-place radix-2 transform of a power-of-two length in long double (tables only: Bh of the Bluestein plan)
void host_fft_pow2(std::vector<long double>& re, std::vector<long double>& im) {
  const size_t p = re.size();
  const long double pi = acosl(-1.0L);
  for (size_t i = 1, j = 0; i < p; ++i) {
    size_t bit = p >> 1;
    for (; (j & bit) != 0; bit >>= 1) j ^= bit;
    j ^= bit;
    if (i < j) {
      std::swap(re[i], re[j]);
      std::swap(im[i], im[j]);
    }
  }
  for (size_t len = 2; len <= p; len <<= 1) {
    const size_t half = len / 2;
    for (size_t k = 0; k < half; ++k) {  // every twiddle evaluated directly: no recurrence error
      const long double a = -2.0L * pi * static_cast<long double>(k) / static_cast<long double>(len);
      const long double wr = cosl(a), wi = sinl(a);
      for (size_t s = k; s < p; s += len) {
        const long double tr = re[s + half] * wr - im[s + half] * wi, ti = re[s + half] * wi + im[s + half] * wr;
        re[s + half] = re[s] - tr;
        im[s + half] = im[s] - ti;
        re[s] += tr;
        im[s] += ti;
      }
    }
  }
}
}  // namespace

void* plan_t::upload_bluestein_tables(const std::vector<int>& radices, long long n, long long p) {
  // w[j] = exp(-i pi j^2 / N): the angle is reduced as j^2 mod 2N in integers before it meets floating point
  const long double pi = acosl(-1.0L);
  std::vector<long double> wr(static_cast<size_t>(n)), wi(static_cast<size_t>(n));
  for (long long j = 0; j < n; ++j) {
    const long long r = static_cast<long long>((static_cast<unsigned long long>(j) * static_cast<unsigned long long>(j)) %
                                               static_cast<unsigned long long>(2 * n));
    const long double a = -pi * static_cast<long double>(r) / static_cast<long double>(n);
    wr[static_cast<size_t>(j)] = cosl(a);
    wi[static_cast<size_t>(j)] = sinl(a);
  }
  // b[m] = conj(w[|m|]), |m| < N, circularly in P slots; Bh = DFT_P(b) / P
  std::vector<long double> br(static_cast<size_t>(p), 0.0L), bi(static_cast<size_t>(p), 0.0L);
  for (long long j = 0; j < n; ++j) {
    br[static_cast<size_t>(j)] = wr[static_cast<size_t>(j)];
    bi[static_cast<size_t>(j)] = -wi[static_cast<size_t>(j)];
    if (j > 0) {
      br[static_cast<size_t>(p - j)] = wr[static_cast<size_t>(j)];
      bi[static_cast<size_t>(p - j)] = -wi[static_cast<size_t>(j)];
    }
  }
  host_fft_pow2(br, bi);
  auto build = [&](auto tag) {
    using T = decltype(tag);
    std::vector<T> t = host_twiddles<T>(radices);
    for (long long j = 0; j < n; ++j) {
      t.push_back(static_cast<T>(wr[static_cast<size_t>(j)]));
      t.push_back(static_cast<T>(wi[static_cast<size_t>(j)]));
    }
    for (long long k = 0; k < p; ++k) {
      t.push_back(static_cast<T>(br[static_cast<size_t>(k)] / static_cast<long double>(p)));
      t.push_back(static_cast<T>(bi[static_cast<size_t>(k)] / static_cast<long double>(p)));
    }
    return upload(t.data(), t.size() * sizeof(T));
  };
  return desc.precision == PFFT_PRECISION_F64 ? build(double{}) : build(float{});
}

/// PFFT_EXT_ANY_LENGTH on a length with a prime factor above 61 (validated: fp32 / fp64, rank 1, interleaved, unit
/// strides): Bluestein's algorithm in one launch per direction, on the convolution length P = the smallest power of two
/// >= 2N - 1.  in_addr / out_addr: the input / output side of this direction, in complex elements.
void plan_t::plan_bluestein(int direction) {
  const long long n = static_cast<long long>(desc.lengths[0]);
  const long long count = static_cast<long long>(desc.number_of_transforms);
  long long p = 1;
  while (p < 2 * n - 1) p *= 2;
  const int cp = compute_precision();
  const spec_kernel* k = nullptr;
  int n_entries = 0;
  const spec_kernel* all = bluestein_kernels(&n_entries);
  long long longest_p = 0;  // of this precision, among the entries whose LDS the device can give
  for (int i = 0; i < n_entries; ++i) {
    if (all[i].precision != cp) continue;
    if (all[i].n == p && k == nullptr) k = &all[i];
    if (all[i].lds_bytes <= max_lds) longest_p = std::max<long long>(longest_p, all[i].n);
  }
  if (k != nullptr && k->lds_bytes > max_lds) {
    fail(PFFT_OUT_OF_LOCAL_MEMORY, "any-length transform of length ", n, ": its convolution length P = ", p, " needs ",
         k->lds_bytes, " bytes of LDS, device has ", max_lds);
  }
  if (k == nullptr) {
    fail(PFFT_UNSUPPORTED_CONFIGURATION, "any-length transform of length ", n, ": its convolution length P = ", p,
         " has no LDS-resident plan (the longest in this precision is P = ", longest_p, ", for lengths up to ",
         longest_p / 2, ")");
  }
  const int backward = direction == PFFT_BACKWARD ? 1 : 0;
  const view_t iv = view_of(desc, direction), ov = view_of(desc, backward ? PFFT_FORWARD : PFFT_BACKWARD);
  // the kernel's buffer resources cover the fpw rows of a group with 32-bit byte offsets
  const unsigned long long row_limit = (1ull << 32) / (static_cast<unsigned long long>(k->fpw) * elem_bytes());
  if (std::max(iv.distance, ov.distance) >= row_limit) {
    fail(PFFT_UNSUPPORTED_CONFIGURATION, "any-length transform: row pitch beyond the kernel's 32-bit range (the ", k->fpw,
         " rows of one work-group must span less than 4 GiB: distances below ", row_limit, " elements)");
  }
  stage s;
  s.spec = k;
  s.form = WF_BLUESTEIN;
  s.n = static_cast<int>(n);
  s.count = count;
  s.backward = backward;
  s.scale = backward ? desc.backward_scale : desc.forward_scale;
  s.in_addr.offset = static_cast<long long>(iv.offset);
  // (a single transform may carry any distance; the kernel's resources are sized by the pitch, so it gets the row)
  s.in_addr.dist_inner = std::max(static_cast<long long>(iv.distance), n);
  s.out_addr.offset = static_cast<long long>(ov.offset);
  s.out_addr.dist_inner = std::max(static_cast<long long>(ov.distance), n);
  push_fused_stage(s, direction, [&] {
    return upload_bluestein_tables(std::vector<int>(k->radices, k->radices + k->n_radices), n, p);
  });
}

/// work-group loop trips of a strided stage (stockham_strided.hpp: strided_ngroups)
long long plan_t::strided_groups(long long count, long long inner, int fpw) {
  return ((count + inner - 1) / inner) * ((inner + fpw - 1) / fpw);
}

/// can the strided kernel `k` address this stage?  (interleaved data, whole groups, 32-bit byte ranges)
bool plan_t::strided_fits(const strided_kernel* k, long long inner_count, int in_buf, const addressing& ia,
                          int out_buf, const addressing& oa) const {
  if (k == nullptr) return false;
  // split storage: both sides user buffers (split variant), both scratch (interleaved variant), or one of each
  // when the entry carries the mixed forms
  const bool split = desc.complex_storage == PFFT_SPLIT_COMPLEX;
  if (split && ((in_buf == BUF_SCRATCH) != (out_buf == BUF_SCRATCH))) {
    if (!k->form[in_buf == BUF_SCRATCH ? SF_MIXED_OUT : SF_MIXED_IN][0]) return false;
  }
  (void)inner_count;
  auto range_ok = [&](const addressing& a) {
    const unsigned long long elems = static_cast<unsigned long long>(k->fpw - 1) * a.dist_inner +
                                     static_cast<unsigned long long>(k->n - 1) * a.stride + 1;
    return a.stride < (1ll << 31) && a.dist_inner < (1ll << 31) && fits_buffer_range(elems * elem_bytes());
  };
  return range_ok(ia) && range_ok(oa);
}

/// W_n^m for m in [0, n): the inter-pass column twiddles of the two-pass 2-D plan
const void* plan_t::upload_unit_roots(long long n) {
  auto fill = [&](auto tag) {
    using T = decltype(tag);
    std::vector<T> v(static_cast<size_t>(2 * n));
    for (long long i = 0; i < n; ++i) {
      const long double a = -2.0L * static_cast<long double>(PI_L) * static_cast<long double>(i) /
                            static_cast<long double>(n);
      v[static_cast<size_t>(2 * i)] = static_cast<T>(cosl(a));
      v[static_cast<size_t>(2 * i + 1)] = static_cast<T>(sinl(a));
    }
    return upload(v.data(), v.size() * sizeof(T));
  };
  return desc.precision == PFFT_PRECISION_F64 ? fill(double{}) : fill(float{});
}

stage plan_t::make_strided_stage(const strided_kernel* k, long long count, long long inner_count, int in_buf,
                                 const addressing& ia, int out_buf, const addressing& oa, double scale, int backward,
                                 int store_modifier, bool allow_row) {
  stage s;
  s.strided = k;
  s.store_modifier = store_modifier;
  s.n = k->n;
  s.in_buf = in_buf;
  s.out_buf = out_buf;
  s.count = count;
  s.in_addr = ia;
  s.out_addr = oa;
  s.backward = backward;
  strided_args& a = s.sa;
  a.tw = upload_twiddles(std::vector<int>(k->radices, k->radices + k->n_radices));
  a.total = count;
  a.inner = std::max<long long>(inner_count, 1);
  a.in_dist_outer = ia.dist_outer;
  a.out_dist_outer = oa.dist_outer;
  a.in_stride = static_cast<unsigned>(ia.stride);
  a.out_stride = static_cast<unsigned>(oa.stride);
  a.in_fdist = static_cast<unsigned>(ia.dist_inner);
  a.out_fdist = static_cast<unsigned>(oa.dist_inner);
  a.scale = scale;
  a.stw_tab = nullptr;
  a.stw_levels = 0;
  a.stw_lshift = 0;
  a.stw_cdiv = 1;
  a.stw_lo = nullptr;
  a.stw_hi = nullptr;
  a.stw_shift = 0;
  s.lds_bytes = k->lds_bytes;
  // row-shaped side of an interleaved fp32 stage: copy it through LDS with full-line accesses
  const bool user_split =
      desc.complex_storage == PFFT_SPLIT_COMPLEX && in_buf != BUF_SCRATCH && out_buf != BUF_SCRATCH;
  // fp32 row-shaped sides are staged through LDS (`_row` forms).  Measured (tools/perf_global_f32.py): a staged
  // row-shaped INPUT pays up to n = 512 (four-step stage B of N=65536: 2.6 vs 2.0 TB/s; P->BI n=256 5.2 vs 3.2) and
  // loses beyond (N=2^20: 1.76 vs 2.07 with the group-major intermediate; P->BI n=1024 2.7 vs 3.7); a staged
  // row-shaped OUTPUT always pays (BI->P n=1024 4.0 vs 2.0).
  int want_row = 0;
  if (ia.stride == 1 && ia.dist_inner != 1 && oa.dist_inner == 1 && (k->n <= kn.row_in_max_n || k->rowish != 0)) want_row = 1;
  if (oa.stride == 1 && oa.dist_inner != 1 && ia.dist_inner == 1) want_row = 2;
  if (!allow_row) want_row = 0;  // four-step pair: stage B reads the group-major intermediate (tiled-input form)
  const bool mixed = desc.complex_storage == PFFT_SPLIT_COMPLEX && (in_buf == BUF_SCRATCH) != (out_buf == BUF_SCRATCH);
  if (k->jit && want_row != 0 && !user_split && !mixed) {  // runtime-compiled entry: build the row form
    std::string why;
    if (jit_strided_ensure_row(k, want_row - 1, max_lds, &why)) {
      s.row_mode = want_row;
      s.lds_bytes = k->lds_bytes_row;
    }
  }
  // mixed stage B (interleaved scratch rows -> the user's planes): always row-staged when the image fits -- its
  // f-fastest form reads 8 bytes per lane from FPW different rows, and there is no tiled-input form to fall back on
  // (power-of-two rows only: fp32 N = 65536 1.88 -> 0.91 ms per GiB, 2^20 1.61 -> 1.28; with 8000-byte rows
  //  -- N = 10^6 -- the f-fastest form spreads over the channels by itself and the staged form loses, 1.84 -> 2.21)
  if (allow_row && k->jit && mixed && in_buf == BUF_SCRATCH && ia.stride == 1 && ia.dist_inner != 1 &&
      oa.dist_inner == 1 && (k->n & (k->n - 1)) == 0 && !kn.no_mixed_rows) {
    std::string why;
    if (jit_strided_ensure_row(k, 0, max_lds, &why, 3)) {
      s.row_mode = 1;
      s.lds_bytes = k->lds_bytes_row;
    }
  }
  // pre-compiled entries with row forms (policy twins carry the row-shaped-input forms only)
  if (!k->jit && k->form[SF_ROW_IN][0] && !user_split && k->lds_bytes_row <= max_lds &&
      (want_row == 0 || k->form[SF_ROW_IN + want_row - 1][backward])) {
    s.row_mode = want_row;
    if (s.row_mode != 0) {
      s.lds_bytes = k->lds_bytes_row;
      for (int f : {SF_ROW_IN, SF_ROW_OUT}) {
        for (const kernel_fn& fn : k->form[f]) hip_check(raise_lds_limit(fn, k->lds_bytes_row), "hipFuncSetAttribute");
      }
    }
  }
  if (k->lds_bytes > 48 * 1024) {
    for (int f : {SF_PLAIN, SF_STW, SF_SPLIT, SF_TIN_W, SF_TIN}) {
      for (const kernel_fn& fn : k->form[f]) hip_check(raise_lds_limit(fn, k->lds_bytes), "hipFuncSetAttribute");
    }
  }
  // the grid: occupancy of the form each case has always asked -- not always the form the stage launches
  int f = SF_PLAIN;
  size_t lds = k->lds_bytes;
  int gpw = k->groups_per_wg;
  if (s.row_mode != 0) {  // the row form
    f = k->jit && mixed ? SF_ROW_MIXED : SF_ROW_IN + s.row_mode - 1;
    lds = k->lds_bytes_row;
    if (k->jit) gpw = 1;
  } else if (k->jit) {  // interleaved: the plain form even with the store modifier; split / mixed: their own; else SF_STW
    f = user_split ? (store_modifier ? SF_SPLIT_STW : SF_SPLIT) : SF_PLAIN;
    if (mixed) f = in_buf == BUF_SCRATCH ? SF_MIXED_OUT : SF_MIXED_IN;
    if (!k->form[f][backward]) f = SF_STW;
  } else {  // pre-compiled: plain / store modifier (also for a split stage), else whichever of the two a twin carries
    f = store_modifier ? SF_STW : SF_PLAIN;
    if (!k->form[f][backward]) f = k->form[SF_PLAIN][backward] ? SF_PLAIN : SF_STW;
  }
  s.grid = persistent_grid(k->form[f][backward], k->wg, lds, strided_groups(count, a.inner, k->fpw), gpw);
  return s;
}

/// the launch grid of a chunked stage is sized for ONE chunk (`count` FFTs / `nmat` matrices), not for the whole
/// batch: the per-kernel rule "groups_per_wg groups per work-group" must hold inside a chunk
void plan_t::regrid_for_chunk(stage& s, long long count) {
  if (s.strided != nullptr) {
    const strided_kernel* k = s.strided;
    const long long groups = strided_groups(count, s.sa.inner, k->fpw);
    if (k->jit) {  // runtime-compiled entries: one group per work-group unless asked otherwise
      int gpw = s.gpw;
      if (kn.jit_groups_per_wg >= 0) gpw = kn.jit_groups_per_wg;  // experiments
      if (gpw > 1 && s.row_mode == 0) {
        // the first forward form the entry carries of plain, store modifier, mixed in, mixed out -- whatever the stage's
        // (the backward plain / store-modifier forms come between: an entry that has the one has the other)
        kernel_fn f{};
        for (const kernel_fn& c : {k->form[SF_PLAIN][0], k->form[SF_STW][0], k->form[SF_PLAIN][1], k->form[SF_STW][1],
                                   k->form[SF_MIXED_IN][0], k->form[SF_MIXED_OUT][0]}) {
          if (!f) f = c;
        }
        if (f) s.grid = persistent_grid(f, k->wg, std::max(k->lds_bytes, s.lds_bytes), groups, gpw);
      }
      return;
    }
    // pre-compiled: the row / tiled-input / plain or store-modifier form (a split stage asks the plain form, a row
    // stage with the store modifier its row form)
    const int f = s.row_mode != 0 ? SF_ROW_IN + s.row_mode - 1
                  : s.tiled_in == 2 ? SF_TIN_W
                  : s.tiled_in != 0 ? SF_TIN
                  : s.store_modifier ? SF_STW : SF_PLAIN;
    if (!k->form[f][s.backward]) return;
    const size_t lds = s.row_mode != 0 ? k->lds_bytes_row : std::max(k->lds_bytes, s.lds_bytes);
    s.grid = persistent_grid(k->form[f][s.backward], k->wg, lds, groups, s.gpw > 0 ? s.gpw : k->groups_per_wg);
  } else if (s.rows2d != nullptr) {
    const rows2d_kernel* k = s.rows2d;
    const bool split = desc.complex_storage == PFFT_SPLIT_COMPLEX;
    s.grid = persistent_grid(k->form[split ? R2_SPLIT : R2_INTERLEAVED][s.backward], k->wg, k->lds_bytes,
                             count / std::max<long long>(1, s.ra.n0) * (s.ra.n0 / k->rc), k->groups_per_wg);
  }
}

/// `count` transforms in chunks of AT MOST `chunk` (the cap is the caller's: the scratch allocation, the Infinity Cache):
/// the same number of chunks, equally filled.  N = 40000 x 3355 in 256 MiB chunks was 4 chunks of 838 transforms + one of 3
/// -- two launches of an almost empty grid per execute; now five chunks of 671.  (Round 4 dropped a sliver chunk and let
/// the others grow past the cap by up to an eighth: 288 MiB "cache-sized" chunks fall off the Infinity Cache -- ADVICE r4.)
long long plan_t::even_chunks(long long chunk, long long count) {
  if (chunk >= count) return count;
  const long long n = (count + chunk - 1) / chunk;
  return (count + n - 1) / n;
}

/// bytes of intermediate data per chunk of the GLOBAL tier = cap of the scratch allocation
/// (PFFT_GLOBAL_CHUNK_MIB overrides; 0 = unbounded)
size_t plan_t::global_chunk_bytes() const {
  if (kn.global_chunk_mib_set) {
    if (kn.global_chunk_mib <= 0) return ~size_t{0} >> 1;
    return static_cast<size_t>(kn.global_chunk_mib) << 20;
  }
  return size_t{4} << 30;
}

/// Two-launch plans (four-step tier, two-pass 2-D plan) run chunk by chunk with the intermediate of a chunk sized
/// to the 256 MiB Infinity Cache: the first launch writes it with default-policy stores (streamed loads), the second
/// reads it with default-policy loads (streamed stores), so the intermediate's read is served on-die.  Measured on
/// C5 (tools/tune_2d_small.hip): 256 matrices as 8 chunks of 256 MiB 1.274 ms against 1.421 ms unchunked with
/// streamed accesses; chunks of 288 MiB and more fall off the cliff (1.60 ms), smaller ones pay launch tails.
/// PFFT_CACHE_CHUNK_MIB overrides (0: no cache-sized chunks, everything streamed as in round 1).
size_t plan_t::cache_chunk_bytes() const {
  if (kn.cache_chunk_mib_set) return kn.cache_chunk_mib <= 0 ? 0 : static_cast<size_t>(kn.cache_chunk_mib) << 20;
  return size_t{256} << 20;
}

/// Grid of a persistent kernel.  Measured on the N=4096 kernel (tools/probes/proto_c2.hip, interleaved rounds): a grid of
/// 1-2x the resident work-groups keeps every work-group in lock-step (all load, then all compute) and loses ~5 %
/// against a grid where each work-group handles only `groups_per_wg` groups (4-5 is the optimum when the kernel
/// pre-loads its twiddles into registers, 1 when it re-reads them per FFT): staggered work-group start times smooth
/// the HBM demand.
long long plan_t::resident_groups(const kernel_fn& f, int wg, size_t lds) {
  int per_cu = 0;
  hip_check(fn_occupancy(&per_cu, f, wg, lds), "occupancy query");
  return static_cast<long long>(std::max(per_cu, 1)) * n_cus;
}

unsigned plan_t::persistent_grid(const kernel_fn& f, int wg, size_t lds, long long groups, int groups_per_wg) {
  return grid_of(resident_groups(f, wg, lds), groups, groups_per_wg);
}

unsigned plan_t::grid_of(long long resident, long long groups, int groups_per_wg) const {
  if (kn.groups_per_wg_set) groups_per_wg = kn.groups_per_wg;  // grid-rule experiments
  // groups_per_wg comes from the per-kernel tuning (tools/tune.hip, profiles/r1_notes.md); 0 selects the long
  // persistent loop, which only the one-work-group-per-CU kernels (f32 N=16384) prefer
  long long grid = groups_per_wg <= 0 ? 2 * resident : (groups + groups_per_wg - 1) / groups_per_wg;
  grid = std::min(groups, std::max(grid, std::min<long long>(groups, 2 * resident)));
  grid = std::min<long long>(grid, 1ll << 30);
  return static_cast<unsigned>(std::max<long long>(1, grid));
}

stage plan_t::make_spec_stage(const spec_kernel* k, long long count, int in_buf, long long in_off, int out_buf,
                              long long out_off, double scale, int backward, const void* twiddles, bool unpacked) {
  const bool split = desc.complex_storage == PFFT_SPLIT_COMPLEX;
  stage s;
  s.generic = false;
  s.spec = k;
  s.form = unpacked ? (split ? WF_UNPACKED_SPLIT : WF_UNPACKED) : (split ? WF_SPLIT : WF_INTERLEAVED);
  s.n = k->n;
  s.in_buf = in_buf;
  s.out_buf = out_buf;
  s.in_offset = in_off;
  s.out_offset = out_off;
  s.count = count;
  s.scale = scale;
  s.backward = backward;
  s.tw = twiddles != nullptr ? twiddles
                             : upload_twiddles(std::vector<int>(k->radices, k->radices + k->n_radices));
  // (both storages of a pre-compiled entry, whichever this stage launches; module functions need no raise)
  for (int d = 0; d < 2 && k->lds_bytes > 48 * 1024; ++d) {
    hip_check(raise_lds_limit(k->form[WF_INTERLEAVED][d], k->lds_bytes), "hipFuncSetAttribute");
    hip_check(raise_lds_limit(k->form[WF_SPLIT][d], k->lds_bytes), "hipFuncSetAttribute");
  }
  // The occupancy behind the grid: the stage's own kernel for an entry compiled at commit; for a pre-compiled entry
  // the INTERLEAVED symbol also when the stage runs the split form (as ever since the split forms exist: asking the
  // split symbol could change a tuned grid).
  const int asked = k->jit ? s.form : WF_INTERLEAVED;
  s.grid = persistent_grid(k->form[asked][backward], k->wg, k->lds_bytes, (count + k->fpw - 1) / k->fpw, k->groups_per_wg);
  return s;
}

stage plan_t::make_generic_stage(long long n, long long count, long long inner_count, int in_buf, const addressing& ia,
                                 int out_buf, const addressing& oa, double scale, int conj_in, int conj_out) {
  const std::vector<int> radices = choose_radices(n);
  if (radices.empty()) {
    fail(PFFT_UNSUPPORTED_CONFIGURATION, "FFT size ", n, " : Large Prime sized FFT currently is unsupported");
  }
  stage s;
  s.generic = true;
  s.n = static_cast<int>(n);
  s.in_buf = in_buf;
  s.out_buf = out_buf;
  s.count = count;
  s.in_addr = ia;
  s.out_addr = oa;
  generic_args& g = s.ga;
  g.n = static_cast<int>(n);
  g.n_passes = (n == 1) ? 0 : static_cast<int>(radices.size());
  const std::vector<int> offs = tw_offsets(radices);
  for (int p = 0; p < g.n_passes; ++p) {
    g.radix[p] = radices[static_cast<size_t>(p)];
    g.tw_off[p] = offs[static_cast<size_t>(p)];
  }
  g.tw = upload_twiddles(radices);
  g.in_stride = ia.stride;
  g.out_stride = oa.stride;
  g.in_dist_inner = ia.dist_inner;
  g.in_dist_outer = ia.dist_outer;
  g.out_dist_inner = oa.dist_inner;
  g.out_dist_outer = oa.dist_outer;
  g.inner_count = std::max<long long>(inner_count, 1);
  g.total_count = count;
  g.conj_in = conj_in;
  g.conj_out = conj_out;
  g.scale = scale;
  g.stw_lo = nullptr;
  g.stw_hi = nullptr;
  g.stw_shift = 0;
  // FFTs per work-group: fill ~64 KiB of LDS (two images), at least one FFT, at most what the stage has
  const size_t per_fft = 2 * static_cast<size_t>(n) * elem_bytes();
  long long fpw = std::max<long long>(1, static_cast<long long>((64 * 1024) / per_fft));
  fpw = std::min<long long>(fpw, std::max<long long>(1, count));
  fpw = std::min<long long>(fpw, 256);
  g.fpw = static_cast<int>(fpw);
  s.lds_bytes = per_fft * static_cast<size_t>(fpw);
  if (s.lds_bytes > max_lds) {
    fail(PFFT_OUT_OF_LOCAL_MEMORY, "FFT size ", n, " needs ", s.lds_bytes, " bytes of LDS, device has ", max_lds);
  }
  // lane order: walk whichever index is contiguous in memory
  g.magic_n = generic_magic(static_cast<unsigned>(n));
  g.magic_fpw = generic_magic(static_cast<unsigned>(fpw));
  {
    unsigned ns = 1;
    for (int p = 0; p < g.n_passes; ++p) {
      g.magic_nb[p] = generic_magic(static_cast<unsigned>(n / g.radix[p]));
      g.magic_ns[p] = generic_magic(ns);
      ns *= static_cast<unsigned>(g.radix[p]);
    }
  }
  g.in_f_fast = (fpw > 1 && ia.dist_inner < ia.stride) ? 1 : 0;
  g.out_f_fast = (fpw > 1 && oa.dist_inner < oa.stride) ? 1 : 0;
  bool big_radix = false;  // a prime radix 37 ... 61: the kernel's "big radix" instantiation (generic_args.hpp)
  for (int p = 0; p < g.n_passes; ++p) big_radix = big_radix || g.radix[p] > GENERIC_MAX_SMALL_RADIX;
  const void* fn = generic_kernel_symbol(desc.precision, big_radix);
  if (s.lds_bytes > 48 * 1024) {
    hip_check(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(max_lds)),
              "hipFuncSetAttribute");
  }
  s.grid = persistent_grid(kernel_fn{fn, nullptr, false}, GENERIC_WG, s.lds_bytes, (count + fpw - 1) / fpw, 1);
  return s;
}

/// `forced_n1`: the first factor of the four-step split (measured_split's candidates; 0: the planner's rules)
plan_t::plan_t(const pfft_desc_t& d, hipStream_t s, long long forced_n1_) : desc(d), stream(s), forced_n1(forced_n1_) {
  validate(desc);
  hip_check(hipGetDevice(&device), "hipGetDevice");
  hipDeviceProp_t prop;
  hip_check(hipGetDeviceProperties(&prop, device), "hipGetDeviceProperties");
  n_cus = prop.multiProcessorCount;
  max_lds = prop.sharedMemPerBlock;
  info.rank = desc.rank;
  info.n_compute_units = n_cus;
  info.knob_mask = kn.mask;
  // (a convolution the kernels do not carry is refused before anything is planned or allocated)
  const spec_kernel* ols = nullptr;
  const spec_kernel* conv = has_convolution(desc) ? get_conv(static_cast<long long>(desc.lengths[0]), &ols) : nullptr;
  if (is_real(desc)) {
    plan_real(PFFT_FORWARD);
    plan_real(PFFT_BACKWARD);
  } else if (is_any_length(desc)) {
    plan_bluestein(PFFT_FORWARD);
    plan_bluestein(PFFT_BACKWARD);
  } else {
    build_direction(PFFT_FORWARD);
    build_direction(PFFT_BACKWARD);
  }
  if (scratch_bytes > 0) {
    hip_check(hipMalloc(&scratch, scratch_bytes), "hipMalloc(scratch)");
  }
  alloc_xcd_ctl();
  if (alias_scratch_bytes > 0) ensure_alias_scratch();
  info.twiddle_bytes = twiddle_bytes;
  info.scratch_bytes = scratch_bytes + alias_scratch_bytes;
  // (behind the plan info, which is the ordinary plan's: the bit is a permission)
  if (conv != nullptr) plan_conv(conv, ols);
  if (has_real_convolution(desc)) plan_rconv();
  for (int d = 0; d < 2; ++d) {
    long long n = 0;
    for (const stage& st : stages[d]) {
      const long long batches = st.chunk_group < 0 ? 1 : st.count / std::max<long long>(1, st.ffts_per_batch);
      const long long per = std::max<long long>(1, st.chunk_batches);
      n += st.chunk_group < 0 ? 1 : (batches + per - 1) / per;
      if (st.xcd != nullptr) ++n;  // its recovery launch (two when the execute's buffers alias)
    }
    info.launches[d] = static_cast<int32_t>(std::min<long long>(n, 0x7fffffff));
  }
}

/// Copy of a committed plan (committed_descriptor_impl.hpp:774-817): the kernels and the twiddle tables are shared,
/// the scratch buffers are allocated again, so two copies can execute concurrently on two streams.
plan_t::plan_t(const plan_t& o) : kn(o.kn), desc(o.desc), stream(o.stream), device(o.device), n_cus(o.n_cus), max_lds(o.max_lds),
               tables(o.tables), scratch_bytes(o.scratch_bytes), twiddle_bytes(o.twiddle_bytes),
               alias_scratch_bytes(o.alias_scratch_bytes), two_pass_chunk_bytes(o.two_pass_chunk_bytes),
               n_chunk_groups(o.n_chunk_groups), info(o.info), overlap_scratch_half(o.overlap_scratch_half),
               overlap_mode(o.overlap_mode) {
  stages[0] = o.stages[0];
  stages[1] = o.stages[1];
  conv_stages = o.conv_stages;
  ols_stages = o.ols_stages;
  filter = o.filter;
  stft_stages = o.stft_stages;
  window = o.window;
  istft_stages = o.istft_stages;
  synthesis_window = o.synthesis_window;
  dct_stages = o.dct_stages;
  dct_table = o.dct_table;
  dct4_stages = o.dct4_stages;
  dct4_table = o.dct4_table;
  mdct_window = o.mdct_window;
  imdct_stages = o.imdct_stages;
  imdct_window = o.imdct_window;
  periodogram_stages = o.periodogram_stages;
  periodogram_window = o.periodogram_window;
  pairs_stages = o.pairs_stages;
  xcd_ctl_bytes = o.xcd_ctl_bytes;
  xcd_tmap_bytes = o.xcd_tmap_bytes;
  device_guard dg(device);
  if (scratch_bytes > 0) hip_check(hipMalloc(&scratch, scratch_bytes), "hipMalloc(scratch)");
  alloc_xcd_ctl();
  if (o.alias_scratch != nullptr) ensure_alias_scratch();
}

}  // namespace pfa
