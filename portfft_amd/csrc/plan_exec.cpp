// plan_t: execute -- binding the user's pointers, chunked and overlapped launches -- and the C ABI on top of it
// (include/portfft_amd.h).
#include "plan.hpp"

#include <cstdio>

namespace pfa {

/// intermediate of the two-pass 2-D plan when the caller's buffers alias: allocated at commit for IN_PLACE
/// descriptors, on first use when an OUT_OF_PLACE plan is executed with in == out
/// (the lazy path is serialised, refuses to allocate inside a stream capture -- hipMalloc is not capturable: run the
///  aliasing execute once before capturing, or commit the descriptor IN_PLACE)
void plan_t::ensure_alias_scratch() {
  if (alias_scratch != nullptr) return;
  static std::mutex m;
  std::lock_guard<std::mutex> lock(m);
  if (alias_scratch != nullptr) return;
  hipStreamCaptureStatus capturing = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(stream, &capturing) == hipSuccess && capturing != hipStreamCaptureStatusNone) {
    fail(PFFT_INVALID_CONFIGURATION,
         "an OUT_OF_PLACE plan executed with aliasing buffers needs an intermediate that cannot be allocated during "
         "stream capture: execute it once before capturing, or commit the descriptor IN_PLACE");
  }
  if (alias_scratch_bytes == 0) alias_scratch_bytes = two_pass_chunk_bytes;
  hip_check(hipMalloc(&alias_scratch, alias_scratch_bytes), "hipMalloc(2-D intermediate)");
}

int plan_t::strided_form_of(const stage& s) const {
  const bool split = desc.complex_storage == PFFT_SPLIT_COMPLEX;
  const bool in_user = s.in_buf != BUF_SCRATCH, out_user = s.out_buf != BUF_SCRATCH;
  if (split && in_user != out_user) {  // mixed storage (four-step stages): split planes on the user's side
    if (in_user) return SF_MIXED_IN;
    if (s.tiled_in != 0) return SF_MIXED_TIN;
    return s.row_mode == 1 ? SF_ROW_MIXED : SF_MIXED_OUT;
  }
  if (split && in_user) return s.store_modifier ? SF_SPLIT_STW : SF_SPLIT;
  if (s.row_mode != 0 && s.store_modifier == 0) return s.row_mode == 1 ? SF_ROW_IN : SF_ROW_OUT;
  if (s.tiled_in != 0) return s.tiled_in == 2 ? SF_TIN_W : SF_TIN;
  return s.store_modifier ? SF_STW : SF_PLAIN;
}

namespace {
/// launch LDS of form `form` of `k`: its image (the row-staged image for the row forms), then the store- or load-modifier
/// tables (strided_args::stw_tab) when the form reads them from LDS; a register-resident entry's kernel, whose image is
/// a half one, is told where its own LDS ends (strided_args::stw_lds_off)
size_t strided_form_lds(const strided_kernel* k, int form, strided_args& a) {
  const bool row = form == SF_ROW_IN || form == SF_ROW_OUT || form == SF_ROW_MIXED;
  const bool tables =
      form == SF_STW || form == SF_SPLIT_STW || form == SF_MIXED_IN || (form == SF_TIN && k->fs_ltw != 0);
  size_t lds = row ? k->lds_bytes_row : k->lds_bytes;
  if (tables && k->stw_mode == 1) {
    if (k->hx != 0) a.stw_lds_off = static_cast<unsigned>(k->lds_bytes);
    lds += (static_cast<size_t>(a.stw_levels) << a.stw_lshift) * 2 * (k->precision == PFFT_PRECISION_F64 ? 8 : 4);
  }
  return lds;
}

}  // namespace

void two_tier_grid(const spec_kernel& e, int form, long long nfft, unsigned* grid_io, long long* n_main_out,
                   int* main_k_out) {
  unsigned grid = *grid_io;
  const long long ngroups = (nfft + e.fpw - 1) / e.fpw;
  const long long k = grid > 0 ? (ngroups + grid - 1) / grid : 1;
  long long n_main = 0;
  static const bool uniform_only = getenv("PFFT_UNIFORM_GRID") != nullptr;  // A/B switch (profiles/r2_notes.md)
  if (e.two_tier != 0 && form == WF_INTERLEAVED && k >= 4 && grid >= 4096 && !uniform_only) {
    n_main = (static_cast<long long>(grid) * 3 / 4) & ~255ll;
    const long long rest = ngroups - k * n_main;
    grid = static_cast<unsigned>(n_main + (rest + 1) / 2);
  }
  *grid_io = grid;
  *n_main_out = n_main;
  *main_k_out = static_cast<int>(k);
}

/// run stage `s` for the user transforms [b0, b0 + nb) (chunked stages) or entirely (nb < 0)
void plan_t::run_stage(const stage& s, const void* in_re, const void* in_im, void* out_re, void* out_im, long long b0,
                       long long nb, const launch_ctx& lc) {
  const bool on_aux = lc.on_aux, any_order = lc.any_order;
  const size_t scratch_shift = lc.scratch_shift;
  const long long in_shift = nb < 0 ? 0 : b0 * s.in_batch_dist;    // elements
  const long long out_shift = nb < 0 ? 0 : b0 * s.out_batch_dist;  // elements
  const long long count = nb < 0 ? s.count : nb * s.ffts_per_batch;
  const size_t sb = static_cast<size_t>(scalar_bytes());
  const bool split = desc.complex_storage == PFFT_SPLIT_COMPLEX;
  hipStream_t stream = on_aux ? aux_stream : this->stream;
  char* const scratch = this->scratch == nullptr ? nullptr : static_cast<char*>(this->scratch) + scratch_shift;
  // resolve buffers: user buffers follow the descriptor's storage, scratch is always interleaved
  auto base_re = [&](int buf, bool is_in) -> const char* {
    if (buf == BUF_SCRATCH) return static_cast<const char*>(scratch);
    if (buf == BUF_IN) return static_cast<const char*>(in_re);
    (void)is_in;
    return static_cast<const char*>(out_re);
  };
  auto base_im = [&](int buf) -> const char* {
    if (buf == BUF_SCRATCH) return static_cast<const char*>(scratch) + sb;
    if (buf == BUF_IN) return split ? static_cast<const char*>(in_im) : static_cast<const char*>(in_re) + sb;
    return split ? static_cast<const char*>(out_im) : static_cast<const char*>(out_re) + sb;
  };
  auto step_of = [&](int buf) { return (buf == BUF_SCRATCH || !split) ? 2 : 1; };
  // (split storage: either pair of planes aliasing means the pass cannot write its output over its input)
  const bool aliased = s.alias_scratch != 0 && (in_re == out_re || (split && in_im != nullptr && in_im == out_im));
  if (aliased) ensure_alias_scratch();
  if (s.xcd != nullptr) {  // one launch for the whole batch: stage A and stage B tasks from per-XCD queues
    xcd_args x = s.xa;
    x.a.in = static_cast<const char*>(in_re) + static_cast<size_t>(s.in_addr.offset) * elem_bytes();
    x.a.out = scratch;
    x.b.in = scratch;
    x.b.out = static_cast<char*>(out_re) + static_cast<size_t>(s.out_addr.offset) * elem_bytes();
    x.ctl = static_cast<unsigned*>(xcd_ctl);
    x.tmap = static_cast<unsigned*>(xcd_tmap);
    x.report = xcd_report;
    // The persistent launch, then its recovery launch: every work-group of the latter reads one word and leaves unless a
    // hand-off wait of the former gave up, in which case it recomputes what is missing IN STREAM ORDER -- the
    // submission's event (the stop event of the last launch) and everything queued behind the execute see valid data.
    // Aliasing buffers: stage B from the slot rings first (the input of those transforms is already overwritten).
    // A launch that gave up is recomputed silently in stream order -- but it first stalled the stream for seconds (2^24
    // polls of the waiting wave, stockham_xcd.hpp XCD_SPIN_LIMIT).  The report word lives in pinned host memory: look at it
    // WITHOUT synchronising, here, on the next execute, and say so once (latency spikes without a diagnostic).
    if (!xcd_recovery_warned && xcd_report != nullptr && __atomic_load_n(xcd_report, __ATOMIC_RELAXED) != 0) {
      xcd_recovery_warned = true;
      std::fprintf(stderr,
                   "[portfft_amd] an XCD-local four-step launch of this plan gave up a hand-off wait and was recomputed by its "
                   "recovery launch (%u so far; the results are valid, the execute stalled for up to ~3 s). "
                   "pfft_plan_info_t::xcd_recoveries counts them, PFFT_XCD_CHECK=1 turns them into errors, "
                   "PFFT_NO_XCD_LOCAL=1 keeps the two-launch plan.\n",
                   __atomic_load_n(xcd_report, __ATOMIC_RELAXED));
    }
    const hipEvent_t stop = take_stop_event();
    const unsigned wg = static_cast<unsigned>(s.xcd->wg);
    int phase = XCD_RECOVER_STAGE_B;
    void* params[] = {&x, &phase};  // (the four-step kernel takes the first only)
    hip_check(launch_fn(s.xcd->fn[s.backward], s.grid, wg, s.lds_bytes, stream, params), "kernel launch");
    const bool aliasing = in_re == out_re;
    if (aliasing) {
      hip_check(launch_fn(s.xcd->fn_recover[s.backward], s.recover_grid, wg, s.lds_bytes, stream, params), "kernel launch");
    }
    if (stop != nullptr) arm_stop_event(stop);
    phase = aliasing ? XCD_RECOVER_REST : XCD_RECOVER_ALL;
    hip_check(launch_fn(s.xcd->fn_recover[s.backward], s.recover_grid, wg, s.lds_bytes, stream, params), "kernel launch");
    if (kn.xcd_check) check_xcd_recoveries();
    return;
  }
  if (s.rows2d != nullptr) {
    rows2d_args a = s.ra;
    a.any_order = any_order ? 1 : 0;
    if (nb >= 0) a.nmat = nb;  // chunked: matrices [b0, b0 + nb)
    const size_t unit = split ? sb : elem_bytes();
    const size_t io = static_cast<size_t>(s.in_offset + in_shift) * unit;
    const size_t oo = static_cast<size_t>(s.out_offset + out_shift) * unit;
    a.in = static_cast<const char*>(in_re) + io;
    a.out = aliased ? static_cast<char*>(alias_scratch)  // one chunk at a time goes through the scratch
                    : static_cast<char*>(out_re) + oo;
    if (split) {  // the scratch of an in-place execute holds the two planes one after the other
      a.in_im = static_cast<const char*>(in_im) + io;
      a.out_im = aliased ? static_cast<char*>(alias_scratch) + alias_scratch_bytes / 2 : static_cast<char*>(out_im) + oo;
    }
    const long long groups = a.nmat * (a.n0 / s.rows2d->rc);
    unsigned grid = static_cast<unsigned>(std::min<long long>(s.grid, std::max<long long>(groups, 1)));
    void* params[] = {&a};
    hip_check(launch_fn(s.rows2d->form[split ? R2_SPLIT : R2_INTERLEAVED][s.backward], grid,
                        static_cast<unsigned>(s.rows2d->wg), s.rows2d->lds_bytes, stream, params, a.any_order != 0),
              "kernel launch");
    return;
  }
  if (s.strided != nullptr) {
    strided_args a = s.sa;
    a.any_order = any_order ? 1 : 0;
    a.total = count;
    const long long groups = strided_groups(count, a.inner, s.strided->fpw);
    unsigned grid = static_cast<unsigned>(std::min<long long>(s.grid, std::max<long long>(groups, 1)));
    // column-shaped input in segments narrower than a 128-byte line (fp32 n = 2048 stages: 8 columns; the planes of
    // SPLIT_COMPLEX data at 16 fp32 / 8 fp64 columns): neighbouring groups on one XCD (strided_args::pair_xcd).
    // Only the plain strided kernel forms honour it; the grid becomes a multiple of 16.
    {
      const bool in_user_split = split && s.in_buf != BUF_SCRATCH;
      const size_t seg = static_cast<size_t>(s.strided->fpw) * (in_user_split ? sb : elem_bytes());
      const bool column_in = a.in_fdist == 1 && a.in_gdist == 0 && a.in_stride > 1;
      if (column_in && seg < 128 && s.row_mode == 0 && s.tiled_in == 0 && s.strided->fpw > 1 && grid >= 32 &&
          groups >= 32 && kn.pair_xcd) {
        a.pair_xcd = 1;
        grid &= ~15u;
      }
      // ... and a row pitch that is no multiple of a line (68640 = 104 x 660: 5280-byte rows; the columns of a 1000 x 1000
      // matrix): every segment straddles one line more than it fills and shares it with the neighbour group -- the blocks
      // of an XCD walk neighbouring groups (strided_group_walk, pair_xcd 2) so that the shared line is fetched once
      const size_t pitch = static_cast<size_t>(a.in_stride) * (in_user_split ? sb : elem_bytes());
      // ... or a column-shaped OUTPUT at such a pitch (the four-step stage B of 68640 = 104 x 660 writes 128-byte segments at a
      // pitch of 832 bytes): the partial lines of two neighbouring groups meet in one L2
      const bool out_user_split = split && s.out_buf != BUF_SCRATCH;
      const bool column_out = a.out_fdist == 1 && a.out_gdist == 0 && a.out_stride > 1 && a.out_tile_shift == 0;
      const size_t opitch = static_cast<size_t>(a.out_stride) * (out_user_split ? sb : elem_bytes());
      // (kernels compiled at commit only: the pre-compiled instantiations keep the loop of rounds 1-5)
      // (the row-staged forms of such entries walk the same way)
      if (a.pair_xcd == 0 && ((column_in && a.in_tile_shift == 0 && pitch % 128 != 0) || (column_out && opitch % 128 != 0)) &&
          s.tiled_in == 0 && s.strided->jit && s.strided->fpw > 1 && grid >= 64 && kn.xcd_contig) {
        a.pair_xcd = 2;
      }
    }
    if (split && (s.in_buf == BUF_SCRATCH) != (s.out_buf == BUF_SCRATCH)) {  // mixed storage (four-step stages)
      const bool in_user = s.in_buf != BUF_SCRATCH;
      const size_t iu = in_user ? sb : elem_bytes(), ou = in_user ? elem_bytes() : sb;
      const size_t io = static_cast<size_t>(s.in_addr.offset + in_shift) * iu;
      const size_t oo = static_cast<size_t>(s.out_addr.offset + out_shift) * ou;
      a.in = base_re(s.in_buf, true) + io;
      a.in_im = in_user ? base_im(s.in_buf) + io : nullptr;
      a.out = const_cast<char*>(base_re(s.out_buf, false)) + oo;
      a.out_im = in_user ? nullptr : const_cast<char*>(base_im(s.out_buf)) + oo;
    } else if (split && s.in_buf != BUF_SCRATCH) {  // both sides are user buffers
      const size_t io = static_cast<size_t>(s.in_addr.offset + in_shift) * sb;
      const size_t oo = static_cast<size_t>(s.out_addr.offset + out_shift) * sb;
      a.in = base_re(s.in_buf, true) + io;
      a.in_im = base_im(s.in_buf) + io;
      if (aliased && s.alias_scratch == 2) {  // two-pass 2-D plan, in-place execute: pass 1 left planes in the scratch
        a.in = alias_scratch;
        a.in_im = static_cast<const char*>(alias_scratch) + alias_scratch_bytes / 2;
      }
      a.out = const_cast<char*>(base_re(s.out_buf, false)) + oo;
      a.out_im = const_cast<char*>(base_im(s.out_buf)) + oo;
    } else {
      a.in = base_re(s.in_buf, true) + static_cast<size_t>(s.in_addr.offset + in_shift) * elem_bytes();
      if (aliased && s.alias_scratch == 2) a.in = alias_scratch;  // two-pass 2-D plan, in-place execute
      a.out = const_cast<char*>(base_re(s.out_buf, false)) +
              static_cast<size_t>(s.out_addr.offset + out_shift) * elem_bytes();
    }
    const int form = strided_form_of(s);
    const size_t lds = strided_form_lds(s.strided, form, a);
    void* params[] = {&a};
    hip_check(launch_fn(s.strided->form[form][s.backward], grid, static_cast<unsigned>(s.strided->wg), lds, stream, params,
                        a.any_order != 0),
              "kernel launch");
    return;
  }
  if (!s.generic) {  // a packed work-group kernel in its form s.form: resolve the pointers, pack that form's arguments
    const spec_kernel* k = s.spec;
    const int f = s.form;
    const void *i0 = nullptr, *i1 = nullptr;
    void *o0 = nullptr, *o1 = nullptr;
    if (f == WF_REAL || f == WF_BLUESTEIN || f == WF_CONV) {  // user buffers, interleaved; offsets and row pitches in in_addr / out_addr
      const size_t io = static_cast<size_t>(s.in_addr.offset) * (f == WF_REAL ? sb : elem_bytes());
      const size_t oo = static_cast<size_t>(s.out_addr.offset) * elem_bytes();
      const bool swap = f == WF_REAL && s.backward != 0;  // C2R: in_addr is the real side, which is the output
      i0 = static_cast<const char*>(in_re) + (swap ? oo : io);
      o0 = static_cast<char*>(out_re) + (swap ? io : oo);
    } else if (f == WF_RCONV) {  // user buffers of real rows on both sides: the forward domain's offset, in scalars
      i0 = static_cast<const char*>(in_re) + static_cast<size_t>(s.in_addr.offset) * sb;
      o0 = static_cast<char*>(out_re) + static_cast<size_t>(s.out_addr.offset) * sb;
    } else {  // offsets in scalars on split planes (user buffers only: plan_1d), in complex elements otherwise
      const size_t unit = (f == WF_SPLIT || f == WF_UNPACKED_SPLIT) ? sb : elem_bytes();
      const size_t io = static_cast<size_t>(s.in_offset) * unit, oo = static_cast<size_t>(s.out_offset) * unit;
      i0 = base_re(s.in_buf, true) + io;
      i1 = base_im(s.in_buf) + io;
      o0 = const_cast<char*>(base_re(s.out_buf, false)) + oo;
      o1 = const_cast<char*>(base_im(s.out_buf)) + oo;
    }
    const void* tw = s.tw;
    const void* filt = filter ? filter->ptr : nullptr;  // (WF_CONV only; plan_t::convolve has checked it)
    unsigned n_filters = filter ? filter->n_filters : 0;
    long long nfft = s.count;
    scale_arg scale_of(s.scale, desc.precision);
    void* const scale = scale_of.ptr();
    unsigned n = static_cast<unsigned>(s.n);
    unsigned in_stride = static_cast<unsigned>(s.in_addr.stride), in_dist = static_cast<unsigned>(s.in_addr.dist_inner);
    unsigned out_stride = static_cast<unsigned>(s.out_addr.stride), out_dist = static_cast<unsigned>(s.out_addr.dist_inner);
    unsigned grid = s.grid;
    long long n_main = 0;
    int main_k = 0;
    two_tier_grid(*k, f, nfft, &grid, &n_main, &main_k);
    // (the formal parameter types of each form: kernels_impl.hpp, spec_form_args)
    void* params[11];
    auto pack = [&](std::initializer_list<void*> l) { std::copy(l.begin(), l.end(), params); };
    switch (f) {
      case WF_INTERLEAVED: pack({&i0, &o0, &tw, &nfft, scale, &n_main, &main_k}); break;  // (the last two: two_tier only)
      case WF_SPLIT: pack({&i0, &i1, &o0, &o1, &tw, &nfft, scale}); break;
      case WF_UNPACKED:
      case WF_UNPACKED_SPLIT:
        pack({&i0, &i1, &o0, &o1, &tw, &nfft, scale, &in_stride, &in_dist, &out_stride, &out_dist});
        break;
      case WF_REAL: pack({&i0, &o0, &tw, &nfft, scale, &in_dist, &out_dist}); break;
      case WF_BLUESTEIN: pack({&i0, &o0, &tw, &nfft, &n, scale, &in_dist, &out_dist}); break;
      case WF_CONV: pack({&i0, &o0, &tw, &filt, &nfft, &n_filters, scale, &in_dist, &out_dist}); break;
      case WF_RCONV: pack({&i0, &o0, &tw, &filt, &nfft, &n_filters, scale, &in_dist}); break;
      default: fail(PFFT_INTERNAL_ERROR, "packed stage without a form");  // (stage::form was never set)
    }
    hip_check(launch_fn(k->cells(f)[s.backward], grid, static_cast<unsigned>(k->wg), k->lds_bytes, stream, params),
              "kernel launch");
    return;
  }
  generic_args g = s.ga;
  g.total_count = count;
  g.in_step = step_of(s.in_buf);
  g.out_step = step_of(s.out_buf);
  const size_t ioff = static_cast<size_t>(s.in_addr.offset + in_shift);
  const size_t ooff = static_cast<size_t>(s.out_addr.offset + out_shift);
  g.in_re = base_re(s.in_buf, true) + ioff * sb * static_cast<size_t>(g.in_step);
  g.in_im = base_im(s.in_buf) + ioff * sb * static_cast<size_t>(g.in_step);
  g.out_re = const_cast<char*>(base_re(s.out_buf, false)) + ooff * sb * static_cast<size_t>(g.out_step);
  g.out_im = const_cast<char*>(base_im(s.out_buf)) + ooff * sb * static_cast<size_t>(g.out_step);
  const hipError_t e = desc.precision == PFFT_PRECISION_F64 ? launch_generic_f64(stream, s.grid, s.lds_bytes, g)
                                                            : launch_generic_f32(stream, s.grid, s.lds_bytes, g);
  hip_check(e, "kernel launch");
}

/// a two-launch chunk group with several chunks whose chunks do not share an intermediate buffer
bool plan_t::overlappable(const std::vector<stage>& st, size_t i, size_t j, bool several_chunks, bool aliased) const {
  if (!chunk_overlap_enabled() || j - i != 2 || !several_chunks) return false;
  hipStreamCaptureStatus capturing = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(stream, &capturing) != hipSuccess || capturing != hipStreamCaptureStatusNone) {
    return false;  // a captured execute is a plain chain of kernel nodes
  }
  const stage& a = st[i];
  const stage& b = st[i + 1];
  if (aliased && (a.alias_scratch != 0 || b.alias_scratch != 0)) return false;  // one scratch chunk for all chunks
  const bool uses_scratch = a.in_buf == BUF_SCRATCH || a.out_buf == BUF_SCRATCH || b.in_buf == BUF_SCRATCH ||
                            b.out_buf == BUF_SCRATCH;
  return !uses_scratch || overlap_scratch_half > 0;
}

/// chunk c: first launch on the plan's stream, second launch on aux_stream behind an event; the plan's stream joins
/// at the end.  The scratch (four-step plans) alternates between its two halves.
void plan_t::run_chunks_overlapped(const stage& a, const stage& b, long long batches, long long chunk_batches,
                                   const void* in_re, const void* in_im, void* out_re, void* out_im) {
  if (overlap_mode == 2) {
    // Every second launch keeps its barrier, so when the barrier-free first launch of chunk c starts, only the
    // second launch of chunk c - 1 can still be running: other matrices, the other half of the scratch.
    size_t c = 0;
    for (long long b0 = 0; b0 < batches; b0 += chunk_batches, ++c) {
      const long long nb = std::min(chunk_batches, batches - b0);
      launch_ctx lc;
      lc.scratch_shift = (c & 1) * overlap_scratch_half;
      lc.any_order = c > 0;
      run_stage(a, in_re, in_im, out_re, out_im, b0, nb, lc);
      lc.any_order = false;
      run_stage(b, in_re, in_im, out_re, out_im, b0, nb, lc);
    }
    return;
  }
  if (aux_stream == nullptr) {
    hip_check(hipStreamCreateWithFlags(&aux_stream, hipStreamNonBlocking), "hipStreamCreate");
  }
  const size_t n_chunks = static_cast<size_t>((batches + chunk_batches - 1) / chunk_batches);
  while (chunk_events.size() < 2 * n_chunks) {  // [c]: first launch of chunk c done, [n_chunks + c]: second launch
    hipEvent_t ev = nullptr;
    hip_check(hipEventCreateWithFlags(&ev, hipEventDisableTiming), "hipEventCreate");
    chunk_events.push_back(ev);
  }
  size_t c = 0;
  for (long long b0 = 0; b0 < batches; b0 += chunk_batches, ++c) {
    const long long nb = std::min(chunk_batches, batches - b0);
    launch_ctx lc;
    lc.scratch_shift = (c & 1) * overlap_scratch_half;
    if (c >= 2 && overlap_scratch_half > 0) {  // this half of the scratch was last read by chunk c - 2
      hip_check(hipStreamWaitEvent(stream, chunk_events[n_chunks + c - 2], 0), "hipStreamWaitEvent");
    }
    run_stage(a, in_re, in_im, out_re, out_im, b0, nb, lc);
    hip_check(hipEventRecord(chunk_events[c], stream), "hipEventRecord");
    hip_check(hipStreamWaitEvent(aux_stream, chunk_events[c], 0), "hipStreamWaitEvent");
    lc.on_aux = true;
    run_stage(b, in_re, in_im, out_re, out_im, b0, nb, lc);
    if (c + 1 == n_chunks || overlap_scratch_half > 0) {
      hip_check(hipEventRecord(chunk_events[n_chunks + c], aux_stream), "hipEventRecord");
    }
  }
  hip_check(hipStreamWaitEvent(stream, chunk_events[2 * n_chunks - 1], 0), "hipStreamWaitEvent");
}

/// `completion`: the submission's completion event.  Returns true when it rode on the last launch as that dispatch's
/// stop event (kernels.hpp: arm_stop_event); otherwise the caller records it behind the launches.
bool plan_t::execute(int direction, const void* in_re, const void* in_im, void* out_re, void* out_im,
                     hipEvent_t completion) {
  if (direction != PFFT_FORWARD && direction != PFFT_BACKWARD) {
    fail(PFFT_INVALID_CONFIGURATION, "Invalid direction ", direction);
  }
  if (in_re == nullptr || out_re == nullptr) fail(PFFT_INVALID_CONFIGURATION, "null data pointer");
  device_guard dg(device);  // launches go to the device the plan was committed on, whatever is current
  const std::vector<stage>& st = stages[direction];
  bool rode = false;
  if (completion != nullptr && !st.empty() && st.back().chunk_group < 0 && kn.stop_event_on_launch) {
    hipStreamCaptureStatus capturing = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(stream, &capturing) != hipSuccess || capturing != hipStreamCaptureStatusNone) {
      completion = nullptr;  // a captured execute records its event as a node of its own
    }
  } else {
    completion = nullptr;
  }
  for (size_t i = 0; i < st.size();) {
    if (st[i].chunk_group < 0) {
      if (completion != nullptr && i + 1 == st.size()) {
        arm_stop_event(completion);
        struct disarm {  // also when the launch throws
          bool* rode;
          ~disarm() { *rode = take_stop_event() == nullptr; }
        } guard{&rode};
        run_stage(st[i], in_re, in_im, out_re, out_im);
      } else {
        run_stage(st[i], in_re, in_im, out_re, out_im);
      }
      ++i;
      continue;
    }
    size_t j = i;
    while (j < st.size() && st[j].chunk_group == st[i].chunk_group) ++j;
    const long long batches = st[i].count / st[i].ffts_per_batch;
    const long long chunk_batches = std::max<long long>(1, st[i].chunk_batches);
    if (overlappable(st, i, j, batches > chunk_batches, in_re == out_re || (in_im != nullptr && in_im == out_im))) {
      run_chunks_overlapped(st[i], st[i + 1], batches, chunk_batches, in_re, in_im, out_re, out_im);
      i = j;
      continue;
    }
    for (long long b0 = 0; b0 < batches; b0 += chunk_batches) {
      const long long nb = std::min(chunk_batches, batches - b0);
      for (size_t k = i; k < j; ++k) run_stage(st[k], in_re, in_im, out_re, out_im, b0, nb);
    }
    i = j;
  }
  return rode;
}

/// One launch of the call-geometry stage `s` (form s.form, mode s.backward) for `groups` groups of this call:
/// persistent_grid's rule on them -- s.grid is the kernel's resident capacity from when the stage was resolved -- and the
/// completion event riding the launch.  `params`: that form's arguments (kernels_impl.hpp, spec_form_args).
bool plan_t::launch_fused(const stage& s, long long groups, void** params, hipEvent_t completion) {
  const spec_kernel* k = s.spec;
  const unsigned grid = grid_of(s.grid, groups, k->groups_per_wg);
  return launch_riding(completion, [&] {
    hip_check(launch_fn(k->cells(s.form)[s.backward], grid, static_cast<unsigned>(k->wg), k->lds_bytes, stream, params),
              "kernel launch");
  });
}

verb_facts plan_t::facts_of(const std::vector<stage>& st) const {
  verb_facts p;
  p.n = desc.lengths[0];
  p.sb = static_cast<unsigned long long>(scalar_bytes());
  p.real = is_real(desc);
  p.taps = filter ? filter->n_taps : 0;
  p.fpw = static_cast<unsigned long long>(st[0].spec->fpw);  // (the stages of a verb's modes are one kernel entry's)
  p.resident[0] = st[0].grid;
  p.resident[1] = st[1].grid;
  return p;
}

/// The fused stage of `mode` on the user's buffers; the completion event rides the launch as in execute.
bool plan_t::convolve(int mode, const void* in, void* out, hipEvent_t completion) {
  if (conv_stages.empty()) {
    fail(PFFT_INVALID_CONFIGURATION, "convolve: the plan was not committed with PFFT_EXT_CONVOLUTION or "
         "PFFT_EXT_REAL_CONVOLUTION");
  }
  if (mode != PFFT_CONVOLVE && mode != PFFT_CORRELATE) fail(PFFT_INVALID_CONFIGURATION, "Invalid convolution mode ", mode);
  if (in == nullptr || out == nullptr) fail(PFFT_INVALID_CONFIGURATION, "null data pointer");
  if (!filter) fail(PFFT_INVALID_CONFIGURATION, "convolve: no filter has been set (pfft_plan_set_filter)");
  device_guard dg(device);
  const stage& s = conv_stages[static_cast<size_t>(mode)];
  return launch_riding(completion, [&] { run_stage(s, in, nullptr, out, nullptr); });
}

/// Overlap-save filtering of the user's signals with the taps of pfft_plan_set_filter_taps: one launch of the WF_OLS
/// (a real plan: WF_ROLS) stage of `mode`, whose geometry is this call's (verb_geometry.hpp).  Nothing is compiled or
/// allocated here.
bool plan_t::filter_signals(int mode, const void* in, void* out, unsigned long long n_signals, unsigned long long in_length,
                            unsigned long long in_pitch, unsigned long long out_length, unsigned long long out_pitch,
                            hipEvent_t completion) {
  if (conv_stages.empty()) {
    fail(PFFT_INVALID_CONFIGURATION, "filter: the plan was not committed with PFFT_EXT_CONVOLUTION or "
         "PFFT_EXT_REAL_CONVOLUTION");
  }
  if (ols_stages.empty()) {  // (a STAGED configuration whose images fill the LDS to the last 16 bytes per row)
    fail(PFFT_UNSUPPORTED_CONFIGURATION, "filter: the row windows of the overlap-save kernel of length ", desc.lengths[0],
         " do not fit into LDS behind its images");
  }
  // (the mode and the pointers: checked here because they go before the filter's state)
  if (mode != PFFT_CONVOLVE && mode != PFFT_CORRELATE) fail(PFFT_INVALID_CONFIGURATION, "Invalid filter mode ", mode);
  if (in == nullptr || out == nullptr) fail(PFFT_INVALID_CONFIGURATION, "filter: null data pointer");
  if (!filter) fail(PFFT_INVALID_CONFIGURATION, "filter: no filter has been set (needs pfft_plan_set_filter_taps)");
  if (filter->n_taps == 0) {
    fail(PFFT_INVALID_CONFIGURATION,
         "filter: the filter was given as spectra (pfft_plan_set_filter); overlap-save filtering needs "
         "pfft_plan_set_filter_taps, which knows the number of taps");
  }
  filter_geometry g = filter_geometry_of(facts_of(ols_stages), mode, reinterpret_cast<uintptr_t>(in),
                                         reinterpret_cast<uintptr_t>(out), n_signals, in_length, in_pitch, out_length, out_pitch);
  device_guard dg(device);
  const stage& s = ols_stages[static_cast<size_t>(mode)];
  const void* tw = s.tw;
  const void* filt = filter->ptr;
  unsigned n_filters = filter->n_filters;
  scale_arg scale(s.scale, desc.precision);
  void* params[] = {&in,         &out,    &tw,    &filt,        &g.n_signals,  &g.n_seg,    &n_filters,
                    scale.ptr(), &g.lead, &g.hop, &g.in_length, &g.out_length, &g.in_pitch, &g.out_pitch};
  return launch_fused(s, g.groups, params, completion);
}

unsigned long long plan_t::istft_chunk_frames(unsigned long long n_signals, unsigned long long n_frames, unsigned long long hop) const {
  require_real("istft_chunk_frames");
  if (istft_stages.empty()) {
    fail(PFFT_INVALID_CONFIGURATION, "istft_chunk_frames: no synthesis window has been set (pfft_plan_set_synthesis_window)");
  }
  const unsigned long long n = desc.lengths[0];
  if (n_signals == 0 || n_frames == 0 || hop == 0 || hop > n) {
    fail(PFFT_INVALID_CONFIGURATION, "istft_chunk_frames: ", n_signals, " signals, ", n_frames, " frames, hop ", hop,
         ": counts of at least 1 and a hop of 1 ... ", n);
  }
  const stage& s = istft_stages[0];
  return istft_default_chunk(n_signals, n_frames, (n + hop - 1) / hop - 1, static_cast<unsigned long long>(s.spec->fpw), s.grid);
}

/// Inverse short-time Fourier transform of the user's bins with the window of pfft_plan_set_synthesis_window: one launch
/// of the WF_ISTFT stage of `mode` (stockham_wg_istft.hpp), whose geometry is this call's (verb_geometry.hpp).  Nothing
/// is compiled or allocated here.
bool plan_t::istft(const void* in, void* out, unsigned long long n_signals, unsigned long long n_frames,
                   unsigned long long frame_pitch, unsigned long long in_pitch, unsigned long long hop,
                   unsigned long long lead, int mode, unsigned long long out_length, unsigned long long out_pitch,
                   unsigned long long chunk_frames, hipEvent_t completion) {
  require_real("istft");
  if (!synthesis_window || istft_stages.empty()) {
    fail(PFFT_INVALID_CONFIGURATION, "istft: no synthesis window has been set (pfft_plan_set_synthesis_window)");
  }
  istft_geometry g = istft_geometry_of(facts_of(istft_stages), reinterpret_cast<uintptr_t>(in), reinterpret_cast<uintptr_t>(out),
                                       n_signals, n_frames, frame_pitch, in_pitch, hop, lead, mode, out_length, out_pitch,
                                       chunk_frames);
  device_guard dg(device);
  const stage& s = istft_stages[static_cast<size_t>(mode)];
  const void* tw = s.tw;
  const void* win = synthesis_window->ptr;
  scale_arg scale(s.scale, desc.precision);
  void* params[] = {&in,     &out,   &tw,           &win,           &g.n_signals, &g.n_frames,  scale.ptr(),
                    &g.lead, &g.hop, &g.out_length, &g.frame_pitch, &g.in_pitch,  &g.out_pitch, &g.chunk};
  return launch_fused(s, g.groups, params, completion);
}

/// Short-time Fourier transform of the user's signals with the window of pfft_plan_set_window: one launch of the WF_STFT
/// stage of `pad_mode` (stockham_wg_stft.hpp), whose geometry is this call's (verb_geometry.hpp).  Nothing is compiled
/// or allocated here.
bool plan_t::stft(const void* in, void* out, unsigned long long n_signals, unsigned long long in_length,
                  unsigned long long in_pitch, unsigned long long hop, unsigned long long lead, int pad_mode,
                  unsigned long long n_frames, unsigned long long frame_pitch, unsigned long long out_pitch,
                  hipEvent_t completion) {
  require_real("stft");
  if (!window || stft_stages.empty()) fail(PFFT_INVALID_CONFIGURATION, "stft: no window has been set (pfft_plan_set_window)");
  stft_geometry g = stft_geometry_of(facts_of(stft_stages), reinterpret_cast<uintptr_t>(in), reinterpret_cast<uintptr_t>(out),
                                     n_signals, in_length, in_pitch, hop, lead, pad_mode, n_frames, frame_pitch, out_pitch);
  device_guard dg(device);
  const stage& s = stft_stages[static_cast<size_t>(pad_mode)];
  const void* tw = s.tw;
  const void* win = window->ptr;
  scale_arg scale(s.scale, desc.precision);
  void* params[] = {&in,     &out,   &tw,          &win,        &g.n_signals,   &g.n_frames, scale.ptr(),
                    &g.lead, &g.hop, &g.in_length, &g.in_pitch, &g.frame_pitch, &g.out_pitch};
  return launch_fused(s, g.groups, params, completion);
}

/// Discrete cosine transform of type 2 or 3 of the user's packed real rows: one launch of the WF_DCT stage of the type
/// (stockham_wg_dct.hpp) on the rows of this call (verb_geometry.hpp).  Nothing is compiled or allocated here.
bool plan_t::dct(int type, const void* in, void* out, unsigned long long n_rows, unsigned long long in_pitch,
                 unsigned long long out_pitch, hipEvent_t completion) {
  require_real("dct");
  if (!dct_table || dct_stages.empty()) {
    fail(PFFT_INVALID_CONFIGURATION, "dct: the plan was not prepared for cosine transforms (pfft_plan_prepare_dct)");
  }
  dct_geometry g = dct_geometry_of(facts_of(dct_stages), type, reinterpret_cast<uintptr_t>(in), reinterpret_cast<uintptr_t>(out),
                                   n_rows, in_pitch, out_pitch);
  device_guard dg(device);
  const stage& s = dct_stages[type == PFFT_DCT_III ? 1 : 0];
  const void* tw = s.tw;
  const void* ctab = dct_table->ptr;
  scale_arg scale(s.scale, desc.precision);
  void* params[] = {&in, &out, &tw, &ctab, &g.n_rows, scale.ptr(), &g.in_pitch, &g.out_pitch};
  return launch_fused(s, g.groups, params, completion);
}

/// Discrete cosine transform of type 4 of the user's packed real rows: one launch of cell [0] of the WF_DCT4 stages
/// (stockham_wg_dct4.hpp) on the rows of this call (verb_geometry.hpp), with forward_scale or -- `inverse` -- backward_scale.
/// Nothing is compiled or allocated here.
bool plan_t::dct4(bool inverse, const void* in, void* out, unsigned long long n_rows, unsigned long long in_pitch,
                  unsigned long long out_pitch, hipEvent_t completion) {
  require_real("dct4");
  if (!dct4_table || dct4_stages.empty()) {
    fail(PFFT_INVALID_CONFIGURATION, "dct4: the plan was not prepared for type-4 cosine transforms (pfft_plan_prepare_dct4)");
  }
  dct4_geometry g = dct4_geometry_of(facts_of(dct4_stages), reinterpret_cast<uintptr_t>(in), reinterpret_cast<uintptr_t>(out),
                                     n_rows, in_pitch, out_pitch);
  device_guard dg(device);
  const stage& s = dct4_stages[0];
  const void* tw = s.tw;
  const void* tab = dct4_table->ptr;
  const void* win = nullptr;
  unsigned one = 1, zero = 0;
  scale_arg scale(inverse ? desc.backward_scale : desc.forward_scale, desc.precision);
  void* params[] = {&in,   &out,  &tw,         &tab,  &win,         &g.n_rows, &one,
                    scale.ptr(), &zero, &zero, &g.in_pitch, &zero, &g.out_pitch};
  return launch_fused(s, g.groups, params, completion);
}

/// Modified discrete cosine transform of the user's signals with the window of pfft_plan_set_mdct_window: one launch of
/// cell [1] of the WF_DCT4 stages, whose geometry is this call's (verb_geometry.hpp), with forward_scale.  Nothing is
/// compiled or allocated here.
bool plan_t::mdct(const void* in, void* out, unsigned long long n_signals, unsigned long long in_length,
                  unsigned long long in_pitch, unsigned long long lead, unsigned long long n_frames,
                  unsigned long long frame_pitch, unsigned long long out_pitch, hipEvent_t completion) {
  require_real("mdct");
  if (!mdct_window || !dct4_table || dct4_stages.empty()) {
    fail(PFFT_INVALID_CONFIGURATION, "mdct: no window has been set (pfft_plan_set_mdct_window)");
  }
  mdct_geometry g = mdct_geometry_of(facts_of(dct4_stages), reinterpret_cast<uintptr_t>(in), reinterpret_cast<uintptr_t>(out),
                                     n_signals, in_length, in_pitch, lead, n_frames, frame_pitch, out_pitch);
  device_guard dg(device);
  const stage& s = dct4_stages[1];
  const void* tw = s.tw;
  const void* tab = dct4_table->ptr;
  const void* win = mdct_window->ptr;
  scale_arg scale(desc.forward_scale, desc.precision);
  void* params[] = {&in,     &out,         &tw,         &tab,           &win,        &g.n_signals, &g.n_frames, scale.ptr(),
                    &g.lead, &g.in_length, &g.in_pitch, &g.frame_pitch, &g.out_pitch};
  return launch_fused(s, g.groups, params, completion);
}

unsigned long long plan_t::imdct_chunk_frames(unsigned long long n_signals, unsigned long long n_frames) const {
  require_real("imdct_chunk_frames");
  if (imdct_stages.empty()) {
    fail(PFFT_INVALID_CONFIGURATION, "imdct_chunk_frames: no window has been set (pfft_plan_set_imdct_window)");
  }
  if (n_signals == 0 || n_frames == 0) {
    fail(PFFT_INVALID_CONFIGURATION, "imdct_chunk_frames: ", n_signals, " signals, ", n_frames, " frames: counts of at least 1");
  }
  const stage& s = imdct_stages[0];
  return istft_default_chunk(n_signals, n_frames, 1, static_cast<unsigned long long>(s.spec->fpw), s.grid);
}

/// Inverse modified discrete cosine transform of the user's coefficient frames with the window of
/// pfft_plan_set_imdct_window: one launch of the WF_IMDCT stage (stockham_wg_imdct.hpp), whose geometry is this call's
/// (verb_geometry.hpp), with backward_scale.  Nothing is compiled or allocated here.
bool plan_t::imdct(const void* in, void* out, unsigned long long n_signals, unsigned long long n_frames,
                   unsigned long long frame_pitch, unsigned long long in_pitch, unsigned long long lead,
                   unsigned long long out_length, unsigned long long out_pitch, unsigned long long chunk_frames,
                   hipEvent_t completion) {
  require_real("imdct");
  if (!imdct_window || !dct4_table || imdct_stages.empty()) {
    fail(PFFT_INVALID_CONFIGURATION, "imdct: no window has been set (pfft_plan_set_imdct_window)");
  }
  imdct_geometry g = imdct_geometry_of(facts_of(imdct_stages), reinterpret_cast<uintptr_t>(in), reinterpret_cast<uintptr_t>(out),
                                       n_signals, n_frames, frame_pitch, in_pitch, lead, out_length, out_pitch, chunk_frames);
  device_guard dg(device);
  const stage& s = imdct_stages[0];
  const void* tw = s.tw;
  const void* tab = dct4_table->ptr;
  const void* win = imdct_window->ptr;
  scale_arg scale(s.scale, desc.precision);
  void* params[] = {&in,     &out,          &tw,            &tab,        &win,         &g.n_signals, &g.n_frames, scale.ptr(),
                    &g.lead, &g.out_length, &g.frame_pitch, &g.in_pitch, &g.out_pitch, &g.chunk};
  return launch_fused(s, g.groups, params, completion);
}

/// Power spectrogram / periodogram of the user's signals with the window of pfft_plan_set_periodogram_window: one launch
/// of the WF_PERIODOGRAM stage of `pad_mode` (stockham_wg_periodogram.hpp), whose geometry is this call's
/// (verb_geometry.hpp).  Nothing is compiled or allocated here.
bool plan_t::periodogram(const void* in, void* out, unsigned long long n_signals, unsigned long long in_length,
                         unsigned long long in_pitch, unsigned long long hop, unsigned long long lead, int pad_mode,
                         unsigned long long n_frames, unsigned long long avg_frames, unsigned long long row_pitch,
                         unsigned long long out_pitch, hipEvent_t completion) {
  require_real("periodogram");
  if (!periodogram_window || periodogram_stages.empty()) {
    fail(PFFT_INVALID_CONFIGURATION, "periodogram: no window has been set (pfft_plan_set_periodogram_window)");
  }
  periodogram_geometry g =
      periodogram_geometry_of(facts_of(periodogram_stages), reinterpret_cast<uintptr_t>(in), reinterpret_cast<uintptr_t>(out),
                              n_signals, in_length, in_pitch, hop, lead, pad_mode, n_frames, avg_frames, row_pitch, out_pitch);
  device_guard dg(device);
  const stage& s = periodogram_stages[static_cast<size_t>(pad_mode)];
  const void* tw = s.tw;
  const void* win = periodogram_window->ptr;
  scale_arg scale(s.scale, desc.precision);
  void* params[] = {&in,     &out,   &tw,          &win,        &g.n_signals, &g.n_frames,  scale.ptr(),
                    &g.lead, &g.hop, &g.in_length, &g.in_pitch, &g.row_pitch, &g.out_pitch, &g.avg_frames};
  return launch_fused(s, g.groups, params, completion);
}

/// Convolution or correlation of the user's pairs of real rows: one launch of the WF_PAIRS stage of `mode`
/// (stockham_wg_pairs.hpp), whose geometry is this call's (verb_geometry.hpp).  The scale is forward_scale^2 *
/// backward_scale -- what two forward transforms, a product and a backward one give -- or, with the phase transform, whose
/// weights have unit magnitude, backward_scale alone.  Nothing is compiled or allocated here.
bool plan_t::pairs(int mode, const void* x, const void* y, void* out, unsigned long long n_rows,
                   unsigned long long x_length, unsigned long long x_pitch, unsigned long long y_length,
                   unsigned long long y_pitch, unsigned long long out_length, unsigned long long out_pitch,
                   double phat_floor, hipEvent_t completion) {
  require_real("pairs");
  if (pairs_stages.empty()) {
    fail(PFFT_INVALID_CONFIGURATION, "pairs: prepare_pairs missing: the plan was not prepared for pairs of rows "
         "(pfft_plan_prepare_pairs)");
  }
  pairs_geometry g = pairs_geometry_of(facts_of(pairs_stages), mode, reinterpret_cast<uintptr_t>(x),
                                       reinterpret_cast<uintptr_t>(y), reinterpret_cast<uintptr_t>(out), n_rows, x_length,
                                       x_pitch, y_length, y_pitch, out_length, out_pitch, phat_floor);
  device_guard dg(device);
  const stage& s = pairs_stages[mode == PFFT_CORRELATE ? 1 : 0];
  const void* tw = s.tw;
  scale_arg scale(g.floor > 0.0 ? desc.backward_scale : s.scale, desc.precision);
  scale_arg floor(g.floor, desc.precision);
  void* params[] = {&x,          &y,         &out,        &tw,        &g.n_rows,    scale.ptr(), floor.ptr(),
                    &g.x_length, &g.x_pitch, &g.y_length, &g.y_pitch, &g.out_length, &g.out_pitch};
  return launch_fused(s, g.groups, params, completion);
}

void plan_t::check_xcd_recoveries() {
  hipStreamCaptureStatus capturing = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(stream, &capturing) != hipSuccess || capturing != hipStreamCaptureStatusNone) return;
  hip_check(hipStreamSynchronize(stream), "hipStreamSynchronize");
  const unsigned n = __atomic_load_n(xcd_report, __ATOMIC_RELAXED);
  if (n != xcd_recoveries_seen) {
    xcd_recoveries_seen = n;
    fail(PFFT_INTERNAL_ERROR, "XCD-local four-step launch: ", xcd_report[1], " hand-off waits gave up (first: site ",
         xcd_report[2], ", local transform ", xcd_report[3], ", wanted ", xcd_report[4], ", saw ", xcd_report[5],
         "); the execute was recomputed by its recovery launch (PFFT_XCD_CHECK=1 reports this as an error)");
  }
}

}  // namespace pfa


struct pfft_plan_t {
  std::unique_ptr<pfa::plan_t> impl;
};

namespace {
/// Completion events are recycled: creating and destroying a hipEvent_t per submission costs more than the launch
/// of a small transform.  pfft_event_destroy returns the event to this pool (per device), new events come from it.
struct event_pool {
  std::mutex m;
  std::vector<std::pair<int, hipEvent_t>> free_list;  // (device, event)
  hipEvent_t get(int device) {
    {
      std::lock_guard<std::mutex> lock(m);
      for (size_t i = free_list.size(); i-- > 0;) {
        if (free_list[i].first == device) {
          hipEvent_t ev = free_list[i].second;
          free_list[i] = free_list.back();
          free_list.pop_back();
          return ev;
        }
      }
    }
    hipEvent_t ev = nullptr;
    const hipError_t e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
    if (e != hipSuccess) pfa::fail(PFFT_HIP_ERROR, "hipEventCreate: ", hipGetErrorString(e));
    std::lock_guard<std::mutex> lock(m);
    owner[ev] = device;
    return ev;
  }
  /// true when the event was taken back (events not created here are destroyed by the caller)
  bool put(hipEvent_t ev) {
    std::lock_guard<std::mutex> lock(m);
    const auto it = owner.find(ev);
    if (it == owner.end()) return false;
    if (free_list.size() >= 1024) {
      owner.erase(it);
      return false;
    }
    free_list.emplace_back(it->second, ev);
    return true;
  }
  std::map<hipEvent_t, int> owner;
};
event_pool& events() {
  static event_pool* p = new event_pool();  // never destroyed: events may outlive static destruction order
  return *p;
}

/// dependencies in, completion event out (shared by the two _ex entry points)
template <typename Run>
void execute_with_events(pfft_plan_t* plan, int32_t n_deps, void* const* deps, void** event_out, Run&& run) {
  pfa::plan_t& p = *plan->impl;
  pfa::device_guard dg(p.device);
  if (n_deps < 0 || (n_deps > 0 && deps == nullptr)) pfa::fail(PFFT_INVALID_CONFIGURATION, "invalid dependency list");
  for (int32_t i = 0; i < n_deps; ++i) {
    if (deps[i] == nullptr) continue;  // a default-constructed event: nothing to wait for
    const hipError_t e = hipStreamWaitEvent(p.stream, static_cast<hipEvent_t>(deps[i]), 0);
    if (e != hipSuccess) pfa::fail(PFFT_HIP_ERROR, "hipStreamWaitEvent: ", hipGetErrorString(e));
  }
  if (event_out == nullptr) {
    (void)run(nullptr);
    return;
  }
  *event_out = nullptr;
  hipEvent_t ev = events().get(p.device);
  bool rode = false;
  try {
    rode = run(ev);  // true: the event is the stop event of the last dispatch, no packet of its own
  } catch (...) {
    (void)events().put(ev);
    throw;
  }
  if (!rode) {
    const hipError_t e = hipEventRecord(ev, p.stream);
    if (e != hipSuccess) {
      (void)events().put(ev);
      pfa::fail(PFFT_HIP_ERROR, "hipEventRecord: ", hipGetErrorString(e));
    }
  }
  *event_out = ev;
}
}  // namespace

extern "C" {

pfft_status pfft_plan_create(const pfft_desc_t* desc, void* hip_stream, pfft_plan_t** plan) {
  return pfa::guarded([&] {
    if (desc == nullptr || plan == nullptr) pfa::fail(PFFT_INVALID_CONFIGURATION, "null argument");
    *plan = nullptr;
    auto p = std::make_unique<pfft_plan_t>();
    p->impl = std::make_unique<pfa::plan_t>(*desc, static_cast<hipStream_t>(hip_stream));
    *plan = p.release();
  });
}

pfft_status pfft_plan_destroy(pfft_plan_t* plan) {
  return pfa::guarded([&] { delete plan; });
}

pfft_status pfft_plan_get_info(const pfft_plan_t* plan, pfft_plan_info_t* info) {
  return pfa::guarded([&] {
    if (plan == nullptr || info == nullptr) pfa::fail(PFFT_INVALID_CONFIGURATION, "null argument");
    *info = plan->impl->info;
    if (plan->impl->xcd_report != nullptr) info->xcd_recoveries = __atomic_load_n(plan->impl->xcd_report, __ATOMIC_RELAXED);
  });
}

pfft_status pfft_execute(pfft_plan_t* plan, int32_t direction, const void* in, void* out) {
  return pfa::guarded([&] {
    if (plan == nullptr) pfa::fail(PFFT_INVALID_CONFIGURATION, "null plan");
    if (plan->impl->desc.complex_storage != PFFT_INTERLEAVED_COMPLEX) {
      // committed_descriptor_impl.hpp:862-871
      pfa::fail(PFFT_INVALID_CONFIGURATION,
                "To use interleaved data layout, the descriptor.complex_storage must be INTERLEAVED_COMPLEX");
    }
    plan->impl->execute(direction, in, nullptr, out, nullptr);
  });
}

pfft_status pfft_execute_split(pfft_plan_t* plan, int32_t direction, const void* in_real, const void* in_imag,
                               void* out_real, void* out_imag) {
  return pfa::guarded([&] {
    if (plan == nullptr) pfa::fail(PFFT_INVALID_CONFIGURATION, "null plan");
    if (plan->impl->desc.complex_storage != PFFT_SPLIT_COMPLEX) {
      pfa::fail(PFFT_INVALID_CONFIGURATION,
                "To use split data layout, the descriptor.complex_storage must be SPLIT_COMPLEX");
    }
    if (in_imag == nullptr || out_imag == nullptr) pfa::fail(PFFT_INVALID_CONFIGURATION, "null imaginary pointer");
    plan->impl->execute(direction, in_real, in_imag, out_real, out_imag);
  });
}

pfft_status pfft_execute_ex(pfft_plan_t* plan, int32_t direction, const void* in, void* out, int32_t n_deps,
                            void* const* deps, void** event_out) {
  return pfa::guarded([&] {
    if (plan == nullptr) pfa::fail(PFFT_INVALID_CONFIGURATION, "null plan");
    if (plan->impl->desc.complex_storage != PFFT_INTERLEAVED_COMPLEX) {
      pfa::fail(PFFT_INVALID_CONFIGURATION,
                "To use interleaved data layout, the descriptor.complex_storage must be INTERLEAVED_COMPLEX");
    }
    execute_with_events(plan, n_deps, deps, event_out,
                        [&](hipEvent_t ev) { return plan->impl->execute(direction, in, nullptr, out, nullptr, ev); });
  });
}

pfft_status pfft_execute_split_ex(pfft_plan_t* plan, int32_t direction, const void* in_real, const void* in_imag,
                                  void* out_real, void* out_imag, int32_t n_deps, void* const* deps,
                                  void** event_out) {
  return pfa::guarded([&] {
    if (plan == nullptr) pfa::fail(PFFT_INVALID_CONFIGURATION, "null plan");
    if (plan->impl->desc.complex_storage != PFFT_SPLIT_COMPLEX) {
      pfa::fail(PFFT_INVALID_CONFIGURATION,
                "To use split data layout, the descriptor.complex_storage must be SPLIT_COMPLEX");
    }
    if (in_imag == nullptr || out_imag == nullptr) pfa::fail(PFFT_INVALID_CONFIGURATION, "null imaginary pointer");
    execute_with_events(plan, n_deps, deps, event_out,
                        [&](hipEvent_t ev) {
                          return plan->impl->execute(direction, in_real, in_imag, out_real, out_imag, ev);
                        });
  });
}

pfft_status pfft_plan_set_filter(pfft_plan_t* plan, const void* spectra, uint64_t n_filters) {
  return pfa::guarded([&] {
    if (plan == nullptr) pfa::fail(PFFT_INVALID_CONFIGURATION, "null plan");
    plan->impl->set_filter(spectra, n_filters);
  });
}

pfft_status pfft_execute_convolve(pfft_plan_t* plan, int32_t mode, const void* in, void* out) {
  return pfa::guarded([&] {
    if (plan == nullptr) pfa::fail(PFFT_INVALID_CONFIGURATION, "null plan");
    plan->impl->convolve(mode, in, out);
  });
}

pfft_status pfft_execute_convolve_ex(pfft_plan_t* plan, int32_t mode, const void* in, void* out, int32_t n_deps,
                                     void* const* deps, void** event_out) {
  return pfa::guarded([&] {
    if (plan == nullptr) pfa::fail(PFFT_INVALID_CONFIGURATION, "null plan");
    execute_with_events(plan, n_deps, deps, event_out,
                        [&](hipEvent_t ev) { return plan->impl->convolve(mode, in, out, ev); });
  });
}

pfft_status pfft_plan_set_filter_taps(pfft_plan_t* plan, const void* taps, uint64_t n_taps, uint64_t n_filters) {
  return pfa::guarded([&] {
    if (plan == nullptr) pfa::fail(PFFT_INVALID_CONFIGURATION, "null plan");
    plan->impl->set_filter_taps(taps, n_taps, n_filters);
  });
}

pfft_status pfft_execute_filter(pfft_plan_t* plan, int32_t mode, const void* in, void* out, uint64_t n_signals,
                                uint64_t in_length, uint64_t in_pitch, uint64_t out_length, uint64_t out_pitch) {
  return pfa::guarded([&] {
    if (plan == nullptr) pfa::fail(PFFT_INVALID_CONFIGURATION, "null plan");
    plan->impl->filter_signals(mode, in, out, n_signals, in_length, in_pitch, out_length, out_pitch);
  });
}

pfft_status pfft_execute_filter_ex(pfft_plan_t* plan, int32_t mode, const void* in, void* out, uint64_t n_signals,
                                   uint64_t in_length, uint64_t in_pitch, uint64_t out_length, uint64_t out_pitch,
                                   int32_t n_deps, void* const* deps, void** event_out) {
  return pfa::guarded([&] {
    if (plan == nullptr) pfa::fail(PFFT_INVALID_CONFIGURATION, "null plan");
    execute_with_events(plan, n_deps, deps, event_out, [&](hipEvent_t ev) {
      return plan->impl->filter_signals(mode, in, out, n_signals, in_length, in_pitch, out_length, out_pitch, ev);
    });
  });
}

pfft_status pfft_plan_set_window(pfft_plan_t* plan, const void* window) {
  return pfa::guarded([&] {
    if (plan == nullptr) pfa::fail(PFFT_INVALID_CONFIGURATION, "null plan");
    plan->impl->set_window(window);
  });
}

pfft_status pfft_execute_stft(pfft_plan_t* plan, const void* in, void* out, uint64_t n_signals, uint64_t in_length,
                              uint64_t in_pitch, uint64_t hop, uint64_t lead, int32_t pad_mode, uint64_t n_frames,
                              uint64_t frame_pitch, uint64_t out_pitch) {
  return pfa::guarded([&] {
    if (plan == nullptr) pfa::fail(PFFT_INVALID_CONFIGURATION, "null plan");
    plan->impl->stft(in, out, n_signals, in_length, in_pitch, hop, lead, pad_mode, n_frames, frame_pitch, out_pitch);
  });
}

pfft_status pfft_execute_stft_ex(pfft_plan_t* plan, const void* in, void* out, uint64_t n_signals, uint64_t in_length,
                                 uint64_t in_pitch, uint64_t hop, uint64_t lead, int32_t pad_mode, uint64_t n_frames,
                                 uint64_t frame_pitch, uint64_t out_pitch, int32_t n_deps, void* const* deps,
                                 void** event_out) {
  return pfa::guarded([&] {
    if (plan == nullptr) pfa::fail(PFFT_INVALID_CONFIGURATION, "null plan");
    execute_with_events(plan, n_deps, deps, event_out, [&](hipEvent_t ev) {
      return plan->impl->stft(in, out, n_signals, in_length, in_pitch, hop, lead, pad_mode, n_frames, frame_pitch, out_pitch, ev);
    });
  });
}

pfft_status pfft_plan_set_synthesis_window(pfft_plan_t* plan, const void* window) {
  return pfa::guarded([&] {
    if (plan == nullptr) pfa::fail(PFFT_INVALID_CONFIGURATION, "null plan");
    plan->impl->set_synthesis_window(window);
  });
}

pfft_status pfft_plan_istft_chunk_frames(const pfft_plan_t* plan, uint64_t n_signals, uint64_t n_frames, uint64_t hop,
                                         uint64_t* chunk_frames) {
  return pfa::guarded([&] {
    if (plan == nullptr || chunk_frames == nullptr) pfa::fail(PFFT_INVALID_CONFIGURATION, "null argument");
    *chunk_frames = plan->impl->istft_chunk_frames(n_signals, n_frames, hop);
  });
}

pfft_status pfft_execute_istft(pfft_plan_t* plan, const void* in, void* out, uint64_t n_signals, uint64_t n_frames,
                               uint64_t frame_pitch, uint64_t in_pitch, uint64_t hop, uint64_t lead, int32_t mode,
                               uint64_t out_length, uint64_t out_pitch, uint64_t chunk_frames) {
  return pfa::guarded([&] {
    if (plan == nullptr) pfa::fail(PFFT_INVALID_CONFIGURATION, "null plan");
    plan->impl->istft(in, out, n_signals, n_frames, frame_pitch, in_pitch, hop, lead, mode, out_length, out_pitch, chunk_frames);
  });
}

pfft_status pfft_execute_istft_ex(pfft_plan_t* plan, const void* in, void* out, uint64_t n_signals, uint64_t n_frames,
                                  uint64_t frame_pitch, uint64_t in_pitch, uint64_t hop, uint64_t lead, int32_t mode,
                                  uint64_t out_length, uint64_t out_pitch, uint64_t chunk_frames, int32_t n_deps,
                                  void* const* deps, void** event_out) {
  return pfa::guarded([&] {
    if (plan == nullptr) pfa::fail(PFFT_INVALID_CONFIGURATION, "null plan");
    execute_with_events(plan, n_deps, deps, event_out, [&](hipEvent_t ev) {
      return plan->impl->istft(in, out, n_signals, n_frames, frame_pitch, in_pitch, hop, lead, mode, out_length, out_pitch,
                               chunk_frames, ev);
    });
  });
}

pfft_status pfft_plan_prepare_dct(pfft_plan_t* plan) {
  return pfa::guarded([&] {
    if (plan == nullptr) pfa::fail(PFFT_INVALID_CONFIGURATION, "null plan");
    plan->impl->prepare_dct();
  });
}

pfft_status pfft_execute_dct(pfft_plan_t* plan, int32_t type, const void* in, void* out, uint64_t n_rows, uint64_t in_pitch,
                             uint64_t out_pitch) {
  return pfa::guarded([&] {
    if (plan == nullptr) pfa::fail(PFFT_INVALID_CONFIGURATION, "null plan");
    plan->impl->dct(type, in, out, n_rows, in_pitch, out_pitch);
  });
}

pfft_status pfft_execute_dct_ex(pfft_plan_t* plan, int32_t type, const void* in, void* out, uint64_t n_rows, uint64_t in_pitch,
                                uint64_t out_pitch, int32_t n_deps, void* const* deps, void** event_out) {
  return pfa::guarded([&] {
    if (plan == nullptr) pfa::fail(PFFT_INVALID_CONFIGURATION, "null plan");
    execute_with_events(plan, n_deps, deps, event_out,
                        [&](hipEvent_t ev) { return plan->impl->dct(type, in, out, n_rows, in_pitch, out_pitch, ev); });
  });
}

pfft_status pfft_plan_prepare_dct4(pfft_plan_t* plan) {
  return pfa::guarded([&] {
    if (plan == nullptr) pfa::fail(PFFT_INVALID_CONFIGURATION, "null plan");
    plan->impl->prepare_dct4();
  });
}

pfft_status pfft_execute_dct4(pfft_plan_t* plan, int32_t inverse, const void* in, void* out, uint64_t n_rows,
                              uint64_t in_pitch, uint64_t out_pitch) {
  return pfa::guarded([&] {
    if (plan == nullptr) pfa::fail(PFFT_INVALID_CONFIGURATION, "null plan");
    plan->impl->dct4(inverse != 0, in, out, n_rows, in_pitch, out_pitch);
  });
}

pfft_status pfft_execute_dct4_ex(pfft_plan_t* plan, int32_t inverse, const void* in, void* out, uint64_t n_rows,
                                 uint64_t in_pitch, uint64_t out_pitch, int32_t n_deps, void* const* deps, void** event_out) {
  return pfa::guarded([&] {
    if (plan == nullptr) pfa::fail(PFFT_INVALID_CONFIGURATION, "null plan");
    execute_with_events(plan, n_deps, deps, event_out,
                        [&](hipEvent_t ev) { return plan->impl->dct4(inverse != 0, in, out, n_rows, in_pitch, out_pitch, ev); });
  });
}

pfft_status pfft_plan_set_mdct_window(pfft_plan_t* plan, const void* window) {
  return pfa::guarded([&] {
    if (plan == nullptr) pfa::fail(PFFT_INVALID_CONFIGURATION, "null plan");
    plan->impl->set_mdct_window(window);
  });
}

pfft_status pfft_execute_mdct(pfft_plan_t* plan, const void* in, void* out, uint64_t n_signals, uint64_t in_length,
                              uint64_t in_pitch, uint64_t lead, uint64_t n_frames, uint64_t frame_pitch, uint64_t out_pitch) {
  return pfa::guarded([&] {
    if (plan == nullptr) pfa::fail(PFFT_INVALID_CONFIGURATION, "null plan");
    plan->impl->mdct(in, out, n_signals, in_length, in_pitch, lead, n_frames, frame_pitch, out_pitch);
  });
}

pfft_status pfft_execute_mdct_ex(pfft_plan_t* plan, const void* in, void* out, uint64_t n_signals, uint64_t in_length,
                                 uint64_t in_pitch, uint64_t lead, uint64_t n_frames, uint64_t frame_pitch,
                                 uint64_t out_pitch, int32_t n_deps, void* const* deps, void** event_out) {
  return pfa::guarded([&] {
    if (plan == nullptr) pfa::fail(PFFT_INVALID_CONFIGURATION, "null plan");
    execute_with_events(plan, n_deps, deps, event_out, [&](hipEvent_t ev) {
      return plan->impl->mdct(in, out, n_signals, in_length, in_pitch, lead, n_frames, frame_pitch, out_pitch, ev);
    });
  });
}

pfft_status pfft_plan_set_imdct_window(pfft_plan_t* plan, const void* window) {
  return pfa::guarded([&] {
    if (plan == nullptr) pfa::fail(PFFT_INVALID_CONFIGURATION, "null plan");
    plan->impl->set_imdct_window(window);
  });
}

pfft_status pfft_plan_imdct_chunk_frames(const pfft_plan_t* plan, uint64_t n_signals, uint64_t n_frames, uint64_t* chunk_frames) {
  return pfa::guarded([&] {
    if (plan == nullptr || chunk_frames == nullptr) pfa::fail(PFFT_INVALID_CONFIGURATION, "null argument");
    *chunk_frames = plan->impl->imdct_chunk_frames(n_signals, n_frames);
  });
}

pfft_status pfft_execute_imdct(pfft_plan_t* plan, const void* in, void* out, uint64_t n_signals, uint64_t n_frames,
                               uint64_t frame_pitch, uint64_t in_pitch, uint64_t lead, uint64_t out_length, uint64_t out_pitch,
                               uint64_t chunk_frames) {
  return pfa::guarded([&] {
    if (plan == nullptr) pfa::fail(PFFT_INVALID_CONFIGURATION, "null plan");
    plan->impl->imdct(in, out, n_signals, n_frames, frame_pitch, in_pitch, lead, out_length, out_pitch, chunk_frames);
  });
}

pfft_status pfft_execute_imdct_ex(pfft_plan_t* plan, const void* in, void* out, uint64_t n_signals, uint64_t n_frames,
                                  uint64_t frame_pitch, uint64_t in_pitch, uint64_t lead, uint64_t out_length,
                                  uint64_t out_pitch, uint64_t chunk_frames, int32_t n_deps, void* const* deps,
                                  void** event_out) {
  return pfa::guarded([&] {
    if (plan == nullptr) pfa::fail(PFFT_INVALID_CONFIGURATION, "null plan");
    execute_with_events(plan, n_deps, deps, event_out, [&](hipEvent_t ev) {
      return plan->impl->imdct(in, out, n_signals, n_frames, frame_pitch, in_pitch, lead, out_length, out_pitch, chunk_frames,
                               ev);
    });
  });
}

pfft_status pfft_plan_set_periodogram_window(pfft_plan_t* plan, const void* window) {
  return pfa::guarded([&] {
    if (plan == nullptr) pfa::fail(PFFT_INVALID_CONFIGURATION, "null plan");
    plan->impl->set_periodogram_window(window);
  });
}

pfft_status pfft_execute_periodogram(pfft_plan_t* plan, const void* in, void* out, uint64_t n_signals, uint64_t in_length,
                                     uint64_t in_pitch, uint64_t hop, uint64_t lead, int32_t pad_mode, uint64_t n_frames,
                                     uint64_t avg_frames, uint64_t row_pitch, uint64_t out_pitch) {
  return pfa::guarded([&] {
    if (plan == nullptr) pfa::fail(PFFT_INVALID_CONFIGURATION, "null plan");
    plan->impl->periodogram(in, out, n_signals, in_length, in_pitch, hop, lead, pad_mode, n_frames, avg_frames, row_pitch,
                            out_pitch);
  });
}

pfft_status pfft_execute_periodogram_ex(pfft_plan_t* plan, const void* in, void* out, uint64_t n_signals, uint64_t in_length,
                                        uint64_t in_pitch, uint64_t hop, uint64_t lead, int32_t pad_mode, uint64_t n_frames,
                                        uint64_t avg_frames, uint64_t row_pitch, uint64_t out_pitch, int32_t n_deps,
                                        void* const* deps, void** event_out) {
  return pfa::guarded([&] {
    if (plan == nullptr) pfa::fail(PFFT_INVALID_CONFIGURATION, "null plan");
    execute_with_events(plan, n_deps, deps, event_out, [&](hipEvent_t ev) {
      return plan->impl->periodogram(in, out, n_signals, in_length, in_pitch, hop, lead, pad_mode, n_frames, avg_frames,
                                     row_pitch, out_pitch, ev);
    });
  });
}

pfft_status pfft_plan_prepare_pairs(pfft_plan_t* plan) {
  return pfa::guarded([&] {
    if (plan == nullptr) pfa::fail(PFFT_INVALID_CONFIGURATION, "null plan");
    plan->impl->prepare_pairs();
  });
}

pfft_status pfft_execute_pairs(pfft_plan_t* plan, int32_t mode, const void* x, const void* y, void* out, uint64_t n_rows,
                               uint64_t x_length, uint64_t x_pitch, uint64_t y_length, uint64_t y_pitch,
                               uint64_t out_length, uint64_t out_pitch, double phat_floor) {
  return pfa::guarded([&] {
    if (plan == nullptr) pfa::fail(PFFT_INVALID_CONFIGURATION, "null plan");
    plan->impl->pairs(mode, x, y, out, n_rows, x_length, x_pitch, y_length, y_pitch, out_length, out_pitch, phat_floor);
  });
}

pfft_status pfft_execute_pairs_ex(pfft_plan_t* plan, int32_t mode, const void* x, const void* y, void* out,
                                  uint64_t n_rows, uint64_t x_length, uint64_t x_pitch, uint64_t y_length,
                                  uint64_t y_pitch, uint64_t out_length, uint64_t out_pitch, double phat_floor,
                                  int32_t n_deps, void* const* deps, void** event_out) {
  return pfa::guarded([&] {
    if (plan == nullptr) pfa::fail(PFFT_INVALID_CONFIGURATION, "null plan");
    execute_with_events(plan, n_deps, deps, event_out, [&](hipEvent_t ev) {
      return plan->impl->pairs(mode, x, y, out, n_rows, x_length, x_pitch, y_length, y_pitch, out_length, out_pitch,
                               phat_floor, ev);
    });
  });
}

pfft_status pfft_event_wait(void* event) {
  return pfa::guarded([&] {
    if (event == nullptr) return;
    const hipError_t e = hipEventSynchronize(static_cast<hipEvent_t>(event));
    if (e != hipSuccess) pfa::fail(PFFT_HIP_ERROR, "hipEventSynchronize: ", hipGetErrorString(e));
  });
}

pfft_status pfft_event_query(void* event, int32_t* done) {
  return pfa::guarded([&] {
    if (done == nullptr) pfa::fail(PFFT_INVALID_CONFIGURATION, "null argument");
    *done = 1;
    if (event == nullptr) return;
    const hipError_t e = hipEventQuery(static_cast<hipEvent_t>(event));
    if (e == hipErrorNotReady) {
      *done = 0;
    } else if (e != hipSuccess) {
      pfa::fail(PFFT_HIP_ERROR, "hipEventQuery: ", hipGetErrorString(e));
    }
  });
}

pfft_status pfft_event_destroy(void* event) {
  return pfa::guarded([&] {
    if (event == nullptr) return;
    if (events().put(static_cast<hipEvent_t>(event))) return;  // recycled
    const hipError_t e = hipEventDestroy(static_cast<hipEvent_t>(event));
    if (e != hipSuccess) pfa::fail(PFFT_HIP_ERROR, "hipEventDestroy: ", hipGetErrorString(e));
  });
}

pfft_status pfft_queue_copy(void* hip_stream, const void* src, void* dst, size_t bytes, int32_t n_deps,
                            void* const* deps, void** event_out) {
  return pfa::guarded([&] {
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    if (n_deps < 0 || (n_deps > 0 && deps == nullptr)) pfa::fail(PFFT_INVALID_CONFIGURATION, "invalid dependency list");
    for (int32_t i = 0; i < n_deps; ++i) {
      if (deps[i] == nullptr) continue;
      const hipError_t e = hipStreamWaitEvent(st, static_cast<hipEvent_t>(deps[i]), 0);
      if (e != hipSuccess) pfa::fail(PFFT_HIP_ERROR, "hipStreamWaitEvent: ", hipGetErrorString(e));
    }
    if (bytes > 0) {
      const hipError_t e = hipMemcpyAsync(dst, src, bytes, hipMemcpyDefault, st);
      if (e != hipSuccess) pfa::fail(PFFT_HIP_ERROR, "hipMemcpyAsync: ", hipGetErrorString(e));
    }
    if (event_out != nullptr) {
      *event_out = nullptr;
      int device = 0;
      (void)hipGetDevice(&device);
      hipEvent_t ev = events().get(device);
      const hipError_t e = hipEventRecord(ev, st);
      if (e != hipSuccess) {
        (void)events().put(ev);
        pfa::fail(PFFT_HIP_ERROR, "hipEventRecord: ", hipGetErrorString(e));
      }
      *event_out = ev;
    }
  });
}

pfft_status pfft_queue_wait(void* hip_stream) {
  return pfa::guarded([&] {
    const hipError_t e = hipStreamSynchronize(static_cast<hipStream_t>(hip_stream));
    if (e != hipSuccess) pfa::fail(PFFT_HIP_ERROR, "hipStreamSynchronize: ", hipGetErrorString(e));
  });
}

pfft_status pfft_plan_clone(const pfft_plan_t* plan, pfft_plan_t** copy) {
  return pfa::guarded([&] {
    if (plan == nullptr || copy == nullptr) pfa::fail(PFFT_INVALID_CONFIGURATION, "null argument");
    *copy = nullptr;
    auto p = std::make_unique<pfft_plan_t>();
    p->impl = std::make_unique<pfa::plan_t>(*plan->impl);
    *copy = p.release();
  });
}

pfft_status pfft_plan_wait(pfft_plan_t* plan) {
  return pfa::guarded([&] {
    if (plan == nullptr) pfa::fail(PFFT_INVALID_CONFIGURATION, "null plan");
    const hipError_t e = hipStreamSynchronize(plan->impl->stream);
    if (e != hipSuccess) pfa::fail(PFFT_HIP_ERROR, "hipStreamSynchronize: ", hipGetErrorString(e));
  });
}

}  // extern "C"
