"""Power spectrogram / Welch periodogram of REAL signals on the GPU (plan.set_periodogram_window / plan.periodogram of a plan
of the REAL domain: stockham_wg_periodogram_kernel): every output row of every case against NumPy in double precision,
    test_gpu_stft._reference (pad by mode -> frames -> forward_scale * rfft(w * frame)) -> abs() ** 2 -> sums of A frames

Yardsticks.  Relative L1 error per output row <= 2 tau + tau^2 + (A + 2) u, with tau = helpers.REL_L2_TOL of the plan's
complex type and u = 2^-24 (fp32) / 2^-53 (fp64).  Derived, not measured: if the bins of a frame meet tau in relative L2,
| |a|^2 - |b|^2 | <= |a - b| (2 |b| + |a - b|) and Cauchy-Schwarz give ||P^ - P||_1 <= (2 tau + tau^2) ||P||_1; sums of
non-negative rows keep that bound; A + 2 roundings cover the square (two products and their sum, the bound of one bin
being relative) and the A - 1 additions.  And helpers.check_reference_rule(sqrt(got), sqrt(ref), N) per element, with the
tolerance of the plan's complex type.  Signals are uniform in [-1, 1].

One length per kernel shape (M = 2, single-pass STAGED, TWL two-pass, FPW 16 / 4 / 2 / 1 with TW_REGS, 32.16.16, lengths
compiled when the window is set; every registered line runs in test_gpu_periodogram_registry.py).  Per length and pad mode
the smallest geometries that can go wrong: hop in {1 (N <= 128), N/4 + 1 made odd, N, N + 3} x lead in {0, N/2, N - 1},
three signals of F = 7 frames, and for each of them A in {1, 2, 3, F}: 7 = 3 * 2 + 1 = 2 * 3 + 1, so at A = 2 and A = 3 the
last row of every signal holds ONE frame and dead frames sit beside live lane-sets; counts that put S * R at 2 FPW - 1 and
2 FPW + 1 units, as signals of one row (every unit another signal: a group straddles signal boundaries) and as rows of one
signal given as 1-D tensors (A = 2, F = 2 R - 1: a ragged last group and a ragged last row).  The windows rotate through
periodic Hann, a random window in [-1, 1] and None; every third scenario runs on the scaled plan of the length
(forward_scale = 0.5, which enters squared).

Every launch reads from and writes into gpu_utils.Guarded buffers with an ODD in_pitch, row_pitch = M + 2 or M + 3 and
out_pitch above R * row_pitch: the guards, every scalar between the rows and between the signals and the whole input must
be unchanged, bit for bit.

Bit identity (helpers.check_same_bits): a second call against the first, and the three signals in one call against three
one-signal calls, for every A -- one accumulator per (signal, row, bin) that takes its frames in ascending f.  Whether
A = 1 equals |plan.stft|^2 computed by torch bit for bit is printed, not asserted (the kernel may contract re * re + im * im
into a fused multiply-add; torch does not).

Measured on the MI355X (worst row of every case of a length, both pad modes, all windows, relative L1): see DESIGN 3.1o.

No case is skipped."""
import numpy as np
import pytest

import helpers as H
from test_gpu_stft import _odd, _reference, _types, _windows

pytestmark = pytest.mark.gpu

LENGTHS = {"f32": [4, 8, 64, 128, 1024, 4096, 16384, 2000], "f64": [128, 1024, 8192, 6000]}
CASES = [(p, n, pad) for p in ("f32", "f64") for n in LENGTHS[p] for pad in ("zero", "reflect")]
UNIT = {"f32": 2.0 ** -24, "f64": 2.0 ** -53}
FRAMES = 7


def _mods():
    import gpu_utils as G
    import portfft_amd as pf
    return G, pf, G.torch_mod()


_plans = {}


def _plan(pf, n, prec, scaled=False):
    """(plan, forward_scale, fpw) of a length: committed once per process, the window is set per launch"""
    key = (n, prec, scaled)
    if key not in _plans:
        d = pf.real_descriptor(n, prec)
        if scaled:
            d.forward_scale = 0.5
        plan = d.commit()
        _plans[key] = (plan, d.forward_scale, max(1, plan.info().dims[0].ffts_per_workgroup))
    return _plans[key]


def bound(prec, avg):
    """2 tau + tau^2 + (A + 2) u (the module's docstring)"""
    tau = H.REL_L2_TOL[np.dtype(_types(prec)[1])]
    return 2 * tau + tau * tau + (avg + 2) * UNIT[prec]


def rows_of(power, avg):
    """(signals, frames, bins) -> (signals, ceil(frames / avg), bins): sums of avg consecutive frames, the last row ragged"""
    ns, frames, bins = power.shape
    n_rows = -(-frames // avg)
    padded = np.zeros((ns, n_rows * avg, bins))
    padded[:, :frames] = power
    return padded.reshape(ns, n_rows, avg, bins).sum(axis=2)


_worst = {}


def check_rows(got, ref, prec, n, avg, what):
    """got, ref: (signals, rows, bins)"""
    ct = _types(prec)[1]
    g, r = np.asarray(got).astype(np.float64), np.asarray(ref)
    assert np.all(g >= 0), (what, "a negative sum of squares")
    err = np.abs(g - r).sum(axis=2) / np.maximum(r.sum(axis=2), 1e-300)
    worst = float(err.max())
    _worst[(prec, n)] = max(_worst.get((prec, n), 0.0), worst)
    print("%s: worst rel-L1 of a row %.3e (bound %.3e)" % (what, worst, bound(prec, avg)))
    assert worst <= bound(prec, avg), (what, "row", np.unravel_index(int(np.argmax(err)), err.shape), worst, bound(prec, avg))
    assert H.check_reference_rule(np.sqrt(g), np.sqrt(r).astype(ct), n), (what, "per-element reference rule")


def run(G, torch, plan, n, x, hop, lead, pad, frames, avg, what, extra=2, guard=None, one_d=False):
    """plan.periodogram of the signals x (numpy, (signals, in_length)) with the window already set: buffers with an odd
    in_pitch, row_pitch = M + extra and an out_pitch above the rows; write set, guards, unchanged input.  Returns (the sums
    as numpy (signals, rows, M + 1), the Guarded output)."""
    ns, in_length = x.shape
    m = n // 2
    n_rows = -(-frames // avg)
    in_pitch, row_pitch = _odd(in_length + 3), m + extra
    out_pitch = n_rows * row_pitch + 3
    guard = G.GUARD if guard is None else guard
    dtype = torch.from_numpy(x[:0]).dtype
    gin = G.Guarded(ns * in_pitch, dtype, guard)
    gout = G.Guarded(ns * out_pitch, dtype, guard)
    xin = gin.buf.view(ns, in_pitch)
    xin[:, :in_length].copy_(torch.from_numpy(x))
    before = gin.buf.cpu().numpy()
    xv = xin[:, :in_length]
    pv = gout.buf.view(ns, out_pitch)[:, :n_rows * row_pitch].view(ns, n_rows, row_pitch)[:, :, :m + 1]
    if one_d:
        assert ns == 1
        xv, pv = xv[0], pv[0]
    plan.periodogram(xv, pv, hop, frames, frames_per_row=avg, lead=lead, pad=pad)
    plan.wait()
    gin.check(str(what) + ": input")
    gout.check(str(what) + ": output")
    H.check_unchanged(before, gin.buf.cpu().numpy(), what=str(what) + ": the input")
    raw = gout.buf.cpu().numpy()
    idx = (np.arange(ns)[:, None, None] * out_pitch + np.arange(n_rows)[None, :, None] * row_pitch +
           np.arange(m + 1)[None, None, :]).ravel()
    H.check_write_set(raw, idx, what=str(what) + ": output buffer")
    return raw[idx].reshape(ns, n_rows, m + 1), gout


def in_length_for(n, hop, lead, pad, frames, shift=0):
    """a signal that `frames` frames fit, whose last frame runs past its end (zeros) or ends with the reflection"""
    if pad == "zero":
        return max((frames - 1) * hop - lead + n // 2 + 1 + shift, 2)
    return max((frames - 1) * hop + n - 2 * lead + shift, lead + 1)


def scenarios(n, fpw):
    """(name, signals, hop, lead, frames, [A ...], one_d)"""
    m = n // 2
    hops = ([1] if n <= 128 else []) + [_odd(n // 4 + 1), n, n + 3]
    out = [("hop %d lead %d" % (hop, lead), 3, hop, lead, FRAMES, (1, 2, 3, FRAMES), False) for hop in hops for lead in (0, m, n - 1)]
    lead = m - 1 if (m - 1) % 2 else m + 1
    hop = _odd(n // 4 + 1)
    for units in (2 * fpw - 1, 2 * fpw + 1):
        out.append(("%d signals of one row" % units, units, hop, lead, 2, (2,), False))
        out.append(("%d rows of one signal" % units, 1, hop, lead, 2 * units - 1, (min(2, 2 * units - 1),), True))
    return out


@pytest.mark.parametrize("prec,n,pad", CASES)
def test_periodogram_against_numpy(prec, n, pad):
    G, pf, torch = _mods()
    rt, ct = _types(prec)
    rng = np.random.Generator(np.random.SFC64(2000 * n + len(pad)))
    fpw = _plan(pf, n, prec)[2]
    windows = _windows(n, rt, rng)
    print("N=%d %s %s: fpw %d" % (n, prec, pad, fpw))
    seen = set()
    for i, (name, ns, hop, lead, frames, avgs, one_d) in enumerate(scenarios(n, fpw)):
        plan, scale, _ = _plan(pf, n, prec, scaled=i % 3 == 2)
        wname, w = windows[i % 3] if i % 9 < 6 else windows[(i + 1) % 3]  # (every window meets both plans)
        plan.set_periodogram_window(None if w is None else torch.from_numpy(w).cuda())
        length = in_length_for(n, hop, lead, pad, frames, shift=i % 2)
        x = rng.uniform(-1, 1, (ns, length)).astype(rt)
        power = np.abs(_reference(scale, x, w, n, hop, lead, pad, frames)) ** 2  # once per scenario, shared by every A
        for j, avg in enumerate(avgs):
            what = (prec, n, pad, name, wname, "signals", ns, "frames", frames, "A", avg, "scale", scale)
            got, _ = run(G, torch, plan, n, x, hop, lead, pad, frames, avg, what, extra=2 + (i + j) % 2,
                         guard=(65, 63) if i == 0 and j == 0 else None, one_d=one_d)
            check_rows(got, rows_of(power, avg), prec, n, avg, what)
        seen.add(wname)
    assert seen == {"hann", "random", "none"}, seen
    print("periodogram N=%d %s: worst rel-L1 of a row so far %.3e" % (n, prec, _worst[(prec, n)]))


@pytest.mark.parametrize("prec,n,pad", CASES)
def test_the_sums_do_not_depend_on_the_call(prec, n, pad):
    """a second call, and one call per signal: the same bits; A = 1 against |stft|^2 by torch: printed"""
    G, pf, torch = _mods()
    rt, ct = _types(prec)
    m = n // 2
    plan, scale, _ = _plan(pf, n, prec)
    rng = np.random.Generator(np.random.SFC64(31 * n + len(pad)))
    w = rng.uniform(-1, 1, n).astype(rt)
    wd = torch.from_numpy(w).cuda()
    plan.set_periodogram_window(wd)
    hop, lead = _odd(n // 4 + 1), m
    length = in_length_for(n, hop, lead, pad, FRAMES, shift=1)
    x = rng.uniform(-1, 1, (3, length)).astype(rt)
    power = np.abs(_reference(scale, x, w, n, hop, lead, pad, FRAMES)) ** 2
    for avg in (1, 2, 3, FRAMES):
        what = (prec, n, pad, "A", avg)
        got, first = run(G, torch, plan, n, x, hop, lead, pad, FRAMES, avg, what + ("first call",))
        check_rows(got, rows_of(power, avg), prec, n, avg, what)
        again, second = run(G, torch, plan, n, x, hop, lead, pad, FRAMES, avg, what + ("second call",))
        H.check_same_bits(first.buf, second.buf, what=str(what) + ": a second call")
        for i in range(3):
            alone, _ = run(G, torch, plan, n, x[i:i + 1], hop, lead, pad, FRAMES, avg, what + ("signal", i, "alone"))
            H.check_same_bits(torch.from_numpy(np.ascontiguousarray(got[i]).reshape(-1)),
                              torch.from_numpy(np.ascontiguousarray(alone[0]).reshape(-1)),
                              what=str(what) + ": signal %d in a call of its own" % i)
        if avg == 1:
            plan.set_window(wd)
            y = torch.empty(3, FRAMES, m + 1, dtype=torch.from_numpy(np.zeros(0, dtype=ct)).dtype, device="cuda")
            plan.stft(torch.from_numpy(x).cuda(), y, hop, lead=lead, pad=pad).wait()
            composed = (y.real ** 2 + y.imag ** 2).cpu().numpy()
            print("N=%d %s %s: A = 1 equals |stft|^2 by torch bit for bit: %s" % (n, prec, pad, bool(np.array_equal(composed, got))))


def test_refusals_name_the_cause():
    G, pf, torch = _mods()
    from portfft_amd import _lib
    lib = _lib.lib
    n, m = 256, 128
    plan = pf.real_descriptor(n).commit()
    x = torch.zeros(3, 1000, dtype=torch.float32, device="cuda")
    p = torch.zeros(3, 2, m + 1, dtype=torch.float32, device="cuda")
    rp, op = m + 1, 2 * (m + 1)

    def status(call, code, text):
        assert call == code, (call, lib.pfft_last_error())
        assert text in lib.pfft_last_error().decode(), lib.pfft_last_error()

    def run_c(i=x.data_ptr(), o=p.data_ptr(), ns=3, il=1000, ip=1000, hop=64, lead=0, pad=0, nf=5, avg=3, rp=rp, op=op, pl=None):
        return lib.pfft_execute_periodogram(plan._plan if pl is None else pl, i, o, ns, il, ip, hop, lead, pad, nf, avg, rp, op)

    INVALID, UNSUPPORTED = 1, 2
    # no window yet -- the STFT's window is another; a plan that is not REAL
    status(run_c(), INVALID, "no window has been set (pfft_plan_set_periodogram_window)")
    with pytest.raises(pf.invalid_configuration, match="no window has been set"):
        plan.periodogram(x, p, 64, 5, frames_per_row=3)
    plan.set_window(None)
    status(run_c(), INVALID, "no window has been set (pfft_plan_set_periodogram_window)")
    cplx = pf.descriptor([n]).commit()
    status(run_c(pl=cplx._plan), INVALID, "not of the REAL domain")
    status(lib.pfft_plan_set_periodogram_window(cplx._plan, None), INVALID, "not of the REAL domain")
    with pytest.raises(pf.invalid_configuration, match="not of the REAL domain"):
        cplx.periodogram(x, p, 64, 5, frames_per_row=3)
    with pytest.raises(pf.invalid_configuration, match="not of the REAL domain"):
        cplx.set_periodogram_window(None)
    info_before = bytes(plan.info())
    plan.set_periodogram_window(None)
    assert bytes(plan.info()) == info_before  # the plan info is the real plan's
    status(run_c(i=None), INVALID, "null data pointer")
    status(run_c(avg=0), INVALID, "zero count")
    status(run_c(hop=0), INVALID, "hop 0")
    status(run_c(lead=n), INVALID, "lead 256")
    status(run_c(pad=2), INVALID, "pad_mode 2")
    status(run_c(avg=6), INVALID, "avg_frames 6 above the 5 frames")
    status(run_c(rp=m), INVALID, "row_pitch 128 below")
    status(run_c(op=op - 1), INVALID, "out_pitch 257 below")
    status(run_c(avg=2), INVALID, "out_pitch 258 below")  # R = 3
    status(run_c(hop=250), INVALID, "frame 4 starts at sample 1000")
    assert run_c(hop=249) == 0
    status(run_c(hop=187, pad=1), INVALID, "frame 4 ends at sample 1004")
    assert run_c(hop=186, pad=1) == 0
    status(run_c(o=x.data_ptr()), INVALID, "overlap")
    far = x.data_ptr() + (1 << 44)
    status(run_c(ns=1, il=1 << 30, ip=1 << 30, o=far), UNSUPPORTED, "4 GiB")
    status(run_c(ns=1 << 20, il=2048 * 64, ip=2048 * 64, nf=2048, avg=1, op=2048 * rp, o=far), UNSUPPORTED, "2^31")
    plan.wait()
    plan.periodogram(x, p, 64, 5, frames_per_row=3).wait()
    assert float(p.abs().max()) == 0.0


def test_a_copy_keeps_its_window_and_events_order_the_call():
    G, pf, torch = _mods()
    n, prec = 1024, "f32"
    rt, ct = _types(prec)
    rng = np.random.Generator(np.random.SFC64(5))
    (_, hann), (_, rand), _ = _windows(n, rt, rng)
    plan = pf.real_descriptor(n, prec).commit()
    hop, lead, avg = 257, 512, 3
    x = rng.uniform(-1, 1, (3, in_length_for(n, hop, lead, "zero", FRAMES))).astype(rt)
    plan.set_periodogram_window(torch.from_numpy(hann).cuda())
    ref = rows_of(np.abs(_reference(1.0, x, hann, n, hop, lead, "zero", FRAMES)) ** 2, avg)
    bits, _ = run(G, torch, plan, n, x, hop, lead, "zero", FRAMES, avg, "original, hann")
    check_rows(bits, ref, prec, n, avg, "original, hann")
    clone = plan.copy()  # shares the window
    plan.set_periodogram_window(torch.from_numpy(rand).cuda())
    other, _ = run(G, torch, plan, n, x, hop, lead, "zero", FRAMES, avg, "original, second window")
    assert not np.array_equal(bits, other)
    kept, _ = run(G, torch, clone, n, x, hop, lead, "zero", FRAMES, avg, "clone afterwards")
    H.check_unchanged(bits, kept, what="the clone keeps its window")
    # a dependency and a returned event: the input is written by another stream
    xd = torch.zeros(3, x.shape[1], dtype=torch.float32, device="cuda")
    out = torch.zeros(3, 3, n // 2 + 1, dtype=torch.float32, device="cuda")
    staged = torch.from_numpy(x).cuda()
    torch.cuda.current_stream().synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        xd.copy_(staged)
        dep = torch.cuda.Event()
        dep.record(side)
    ev = clone.periodogram(xd, out, hop, FRAMES, frames_per_row=avg, lead=lead, dependencies=[dep])
    assert ev.native
    ev.wait()
    assert ev.is_complete()
    H.check_unchanged(bits, out.cpu().numpy(), what="periodogram with a dependency and a returned event")
    ev = clone.periodogram(xd, out, hop, FRAMES, frames_per_row=avg, lead=lead, want_event=False)
    assert not ev.native
    ev.wait()


@pytest.mark.parametrize("prec,n,groups", [("f32", 512, 1500), ("f64", 6000, 1500), ("f32", 16384, 600)])
def test_many_trips_of_the_persistent_loop(prec, n, groups):
    """more units than the grid holds work-groups (N = 16384: two work-groups per CU, 512), in rows of 2 frames with a ragged
    last row, on a plan that also convolves: a work-group starts its accumulators again for every group it runs"""
    G, pf, torch = _mods()
    rt, ct = _types(prec)
    m = n // 2
    plan = pf.real_convolution_descriptor(n, prec).commit()
    fpw = max(1, plan.info().dims[0].ffts_per_workgroup)
    rng = np.random.Generator(np.random.SFC64(7 * n))
    w = rng.uniform(-1, 1, n).astype(rt)
    plan.set_periodogram_window(torch.from_numpy(w).cuda())
    ns, hop, lead, avg = 5, _odd(n // 4 + 1), m, 2
    n_rows = (groups * fpw) // ns + 1
    frames = avg * (n_rows - 1) + 1
    length = in_length_for(n, hop, lead, "reflect", frames, shift=3)
    x = rng.uniform(-1, 1, (ns, length)).astype(rt)
    gout = G.Guarded(ns * n_rows * (m + 1), torch.from_numpy(x[:0]).dtype)
    plan.periodogram(torch.from_numpy(x).cuda(), gout.buf.view(ns, n_rows, m + 1), hop, frames, frames_per_row=avg, lead=lead,
                     pad="reflect")
    plan.wait()
    gout.check("many trips: output")
    ref = rows_of(np.abs(_reference(1.0, x, w, n, hop, lead, "reflect", frames)) ** 2, avg)
    check_rows(gout.buf.cpu().numpy().reshape(ns, n_rows, m + 1), ref, prec, n, avg, (prec, n, "many trips"))
