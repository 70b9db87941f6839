"""Overlap-save FIR filtering on the GPU (plan.set_filter_taps / plan.filter: stockham_wg_ols_kernel): every signal of
every case against NumPy in double precision,
    convolve   c * np.convolve(x, h)[:out_length]
    correlate  c * np.correlate(concatenate(x, zeros(K - 1)), h, "valid")[:out_length]
with c = forward_scale * backward_scale * N, and the project's two yardsticks unchanged: relative L2 per signal within
helpers.REL_L2_TOL and helpers.check_reference_rule with n = N.  Signals are uniform in [-1, 1] per component, taps
uniform in [-1, 1] / sqrt(K).

One length per kernel shape (single-pass STAGED, TWL two-pass, STAGED FPW 16, FPW 4, FPW 2, TW_REGS, 32.16.16, lengths
compiled at commit; every registered line of the kernel runs in test_gpu_fused_registry.py), and per length the tap counts K = 1, 2, ceil(N/4) + 1, floor(5N/8) (hop < K - 1: several segments
of a signal start in front of its sample 0) and, up to N = 64, K = N (hop 1).  Per (N, K), both modes, the scenarios of
_scenarios(): one segment, exact multiples of the hop, ragged last segments, outputs at their bound and shorter than
the input, 1 and 3 signals and counts that put the number of (signal, segment) rows at or next to 2 * FPW - 1 and
2 * FPW + 1 -- rows of different signals in one work-group, and rows behind the last signal --, one filter and one per
signal.  Apart from the single-signal one-segment case, every output has at least K samples (see _scenarios).

Every launch writes into a gpu_utils.Guarded buffer whose signals are pitched wider than their lengths: the guards, every
element between the signals and the whole input must be unchanged, bit for bit.  Once per case the base pointers are one
element off 128-byte alignment.

Measured on the MI355X (worst signal of every case of a length, both modes): fp32 rel-L2 2.0e-7 (N = 256) ... 3.9e-7
(N = 16), fp64 4.9e-16 (N = 512) ... 9.8e-16 (N = 64).

No case is skipped."""
import numpy as np
import pytest

import helpers as H

pytestmark = pytest.mark.gpu

LENGTHS = {"f32": [16, 32, 256, 512, 2048, 4096, 8192, 1000, 6000], "f64": [64, 512, 4096, 3000]}


def _taps_of(n):
    ks = [1, 2, -(-n // 4) + 1, (5 * n) // 8]
    if n <= 64:
        ks.append(n)
    return sorted(set(ks))


CASES = [(p, n, k) for p in ("f32", "f64") for n in LENGTHS[p] for k in _taps_of(n)]
SCALED = (0.5, 0.25)  # forward_scale, backward_scale * N of the second plan of a length


def _mods():
    import gpu_utils as G
    import portfft_amd as pf
    return G, pf, G.torch_mod()


def _ct(prec):
    return np.complex64 if prec == "f32" else np.complex128


_plans = {}


def _plan(pf, n, prec, scaled=False):
    """(plan, c, fpw) of a length: committed once per process, the filter is set per case"""
    key = (n, prec, scaled)
    if key not in _plans:
        d = pf.convolution_descriptor([n], prec)
        if scaled:
            d.forward_scale, d.backward_scale = SCALED[0], SCALED[1] / n
        plan = d.commit()
        dim = plan.info().dims[0]
        _plans[key] = (plan, d.forward_scale * d.backward_scale * n, max(1, dim.ffts_per_workgroup))
    return _plans[key]


def _data(rng, rows, n, ct, amp=1.0):
    return ((rng.uniform(-1, 1, (rows, n)) + 1j * rng.uniform(-1, 1, (rows, n))) * amp).astype(ct)


def _reference(c, x, h, out_length, correlate):
    """NumPy in double, signal by signal; filter i mod F"""
    k = h.shape[1]
    ref = np.empty((x.shape[0], out_length), dtype=np.complex128)
    for i in range(x.shape[0]):
        xi, hi = x[i].astype(np.complex128), h[i % h.shape[0]].astype(np.complex128)
        if correlate:
            # (np.correlate conjugates its second argument: sum_k x[n + k] conj(h[k]))
            full = np.correlate(np.concatenate([xi, np.zeros(k - 1, dtype=np.complex128)]), hi, "valid")
        else:
            full = np.convolve(xi, hi)
        ref[i] = c * full[:out_length]
    return ref


_worst = {}


def _check(got, ref, ct, n, what):
    err = np.linalg.norm(got - ref, axis=1) / np.maximum(np.linalg.norm(ref, axis=1), 1e-300)
    key = np.dtype(ct).name
    _worst[key] = max(_worst.get(key, 0.0), float(err.max()))
    print("%s: worst rel-L2 %.3e (signal %d)" % (what, float(err.max()), int(np.argmax(err))))
    assert np.all(err <= H.REL_L2_TOL[np.dtype(ct)]), (what, "signal", int(np.argmax(err)), float(err.max()))
    assert H.check_reference_rule(got, ref.astype(ct), n), (what, "per-element reference rule")


def _filter(G, torch, plan, c, n, x, h, out_length, correlate, what, pads=(3, 5), guard=None, verb=None):
    """plan.filter of the signals x (numpy, (signals, in_length)) with the taps h already set: pitched buffers, write set,
    guards, unchanged input, every signal against the reference.  Returns the output signals (numpy)."""
    ns, in_length = x.shape
    ct = x.dtype.type
    in_pitch, out_pitch = in_length + pads[0], out_length + pads[1]
    guard = G.GUARD if guard is None else guard
    dtype = torch.from_numpy(x[:0]).dtype
    gin = G.Guarded(ns * in_pitch, dtype, guard)
    gout = G.Guarded(ns * out_pitch, dtype, guard)
    xin = gin.buf.view(ns, in_pitch)
    xin[:, :in_length].copy_(torch.from_numpy(x))
    before = gin.buf.cpu().numpy()
    xv, yv = xin[:, :in_length], gout.buf.view(ns, out_pitch)[:, :out_length]
    if ns == 1 and verb is None:  # (a single signal may come as a 1-D tensor)
        xv, yv = xv[0], yv[0]
    if verb is None:
        plan.filter(xv, yv, correlate=correlate)
        plan.wait()
    else:
        verb(xv, yv)
    gin.check(str(what) + ": input")
    gout.check(str(what) + ": output")
    H.check_unchanged(before, gin.buf.cpu().numpy(), what=str(what) + ": the input")
    raw = gout.buf.cpu().numpy()
    idx = (np.arange(ns)[:, None] * out_pitch + np.arange(out_length)[None, :]).ravel()
    H.check_write_set(raw, idx, what=str(what) + ": output buffer")
    got = raw.reshape(ns, out_pitch)[:, :out_length].astype(np.complex128)
    _check(got, _reference(c, x, h, out_length, correlate), ct, n, what)
    return raw.reshape(ns, out_pitch)[:, :out_length]


def _scenarios(n, k, fpw, correlate):
    """(name, signals, filters, in_length, out_length, scaled plan, guard): see the head of the file"""
    hop = n - k + 1
    extra = 0 if correlate else k - 1  # out_length <= in_length + extra
    out = []
    # One segment, at the bound where the bound allows one.  With hop < K such an output is a partial sum over the first
    # taps alone (at hop 1 the one product h[0] x[0]): its relative measure is the rounding of any FFT method times
    # ||h|| / |h[0..]|, one draw per case here, fixed by the seed (accuracy).
    l1 = max(1, hop - extra)
    o1 = min(hop, l1 + extra)
    out.append(("one segment", 1, 1, l1, o1, False, None))
    # Short signals, 2 FPW - 1 of them with one filter and 2 FPW + 1 with a filter each: one segment where a segment holds
    # K outputs (hop >= K), otherwise the fewest that do -- over many signals and filters the ratio above is unbounded,
    # while with K outputs the norm of an output is of the size of ||h|| ||x||, as the measure assumes.
    ls, os_ = max(l1, k if correlate else 1), max(o1, k)
    out.append(("short signals, 2 fpw - 1 of them", 2 * fpw - 1, 1, ls, os_, False, None))
    out.append(("short signals, 2 fpw + 1 of them", 2 * fpw + 1, 2 * fpw + 1, ls, os_, False, None))
    # an exact multiple of the hop (correlate: at its bound): two hops, or as many as hold K outputs
    whole = max(2, -(-k // hop)) * hop
    out.append(("whole hops", 3, 3, whole, whole, False, (65, 63)))
    # ragged last segment, the output at its bound
    lr = 2 * hop + hop // 2 + 1
    out.append(("ragged, at the bound", 3, 1, lr, lr + extra, False, None))
    # the output shorter than the input, ragged, n_signals * S just above and just below 2 FPW + 1 / 2 FPW - 1 rows
    o_short = max(2 * hop + (hop + 1) // 2, k)  # S = 3, or as many segments as hold K outputs
    l_short = o_short + 3
    seg = -(-o_short // hop)
    many = -(-(2 * fpw + 1) // seg)
    out.append(("shorter than the input, %d rows" % (many * seg), many, many, l_short, o_short, True, None))
    few = max(1, (2 * fpw - 1) // seg)
    out.append(("shorter than the input, %d rows" % (few * seg), few, 1, l_short, o_short, False, None))
    return out


@pytest.mark.parametrize("prec,n,k", CASES)
def test_filter_against_numpy(prec, n, k):
    G, pf, torch = _mods()
    ct = _ct(prec)
    rng = np.random.Generator(np.random.SFC64(1000 * n + k))
    fpw = _plan(pf, n, prec)[2]
    print("N=%d K=%d %s: hop %d fpw %d" % (n, k, prec, n - k + 1, fpw))
    for correlate in (False, True):
        for name, ns, nf, in_length, out_length, scaled, guard in _scenarios(n, k, fpw, correlate):
            plan, c, _ = _plan(pf, n, prec, scaled)
            x = _data(rng, ns, in_length, ct)
            h = _data(rng, nf, k, ct, 1.0 / np.sqrt(k))
            plan.set_filter_taps(torch.from_numpy(h).cuda())
            _filter(G, torch, plan, c, n, x, h, out_length, correlate,
                    (prec, n, k, "corr" if correlate else "conv", name, ns, nf, in_length, out_length), guard=guard)
    print("worst rel-L2 so far: %s" % _worst)


@pytest.mark.parametrize("prec,n,k", [("f32", 256, 9), ("f64", 3000, 17), ("f32", 4096, 17)])
def test_many_trips_of_the_persistent_loop(prec, n, k):
    """more (signal, segment) rows than the grid holds work-groups"""
    G, pf, torch = _mods()
    ct = _ct(prec)
    plan, c, fpw = _plan(pf, n, prec)
    hop = n - k + 1
    rng = np.random.Generator(np.random.SFC64(7 * n + k))
    ns = 5
    segs = (3000 * fpw) // ns + 1
    in_length = segs * hop - 7
    x = _data(rng, ns, in_length, ct)
    h = _data(rng, 2, k, ct, 1.0 / np.sqrt(k))
    plan.set_filter_taps(torch.from_numpy(h).cuda())
    ref = _reference(c, x, h, in_length, False)
    dtype = torch.from_numpy(x[:0]).dtype
    gout = G.Guarded(ns * in_length, dtype)
    xd = torch.from_numpy(x).cuda()
    plan.filter(xd, gout.buf.view(ns, in_length))
    plan.wait()
    gout.check("many trips: output")
    _check(gout.buf.cpu().numpy().reshape(ns, in_length).astype(np.complex128), ref, ct, n, (prec, n, k, "many trips"))


@pytest.mark.parametrize("prec,n,k", [("f32", 512, 100), ("f64", 3000, 700)])
def test_taps_are_a_filter_like_any_other(prec, n, k):
    G, pf, torch = _mods()
    ct = _ct(prec)
    rng = np.random.Generator(np.random.SFC64(13 * n))
    batch = 5
    d = pf.convolution_descriptor([n], prec)
    d.number_of_transforms = batch
    plan = d.commit()
    c = float(n)
    rows = _data(rng, batch, n, ct)
    xs = _data(rng, 2, 3 * n + 5, ct)
    h1, h2 = _data(rng, 2, k, ct, 1.0 / np.sqrt(k)), _data(rng, 1, k // 2, ct, 1.0 / np.sqrt(k // 2))
    rd = torch.from_numpy(rows.ravel()).cuda()

    def circular(p, h, correlate):
        """convolve / correlate of the plan against circular convolution with the zero-padded taps"""
        y = torch.empty_like(rd)
        (p.correlate if correlate else p.convolve)(rd, y).wait()
        hp = np.zeros((h.shape[0], n), dtype=np.complex128)
        hp[:, :h.shape[1]] = h
        spec = np.fft.fft(hp, axis=1)[np.arange(batch) % h.shape[0]]
        ref = n * np.fft.ifft(np.fft.fft(rows.astype(np.complex128), axis=1) * (np.conj(spec) if correlate else spec), axis=1)
        _check(y.cpu().numpy().reshape(batch, n).astype(np.complex128), ref, ct, n, (prec, n, "circular", correlate))

    def linear(p, h, what):
        return _filter(G, torch, p, c, n, xs, h, xs.shape[1], False, (prec, n, what))

    # a plain set_filter gives spectra: filter() is refused, with the way out
    plan.set_filter(torch.from_numpy(_data(rng, 1, n, ct)).cuda())
    y = torch.empty(2, xs.shape[1], dtype=rd.dtype, device="cuda")
    with pytest.raises(pf.invalid_configuration, match="needs pfft_plan_set_filter_taps"):
        plan.filter(torch.from_numpy(xs).cuda(), y)
    plan.set_filter_taps(torch.from_numpy(h1).cuda())
    circular(plan, h1, False)
    circular(plan, h1, True)
    bits1 = linear(plan, h1, "first taps")
    clone = plan.copy()  # shares the taps
    H.check_unchanged(bits1, linear(clone, h1, "clone, shared taps"), what="a clone filters with the shared taps")
    plan.set_filter_taps(torch.from_numpy(h2.ravel()).cuda())  # another K, shape (K,): takes effect, for this plan
    linear(plan, h2, "second taps, another K")
    circular(plan, h2, False)
    H.check_unchanged(bits1, linear(clone, h1, "clone after the original's second taps"), what="the clone keeps its taps")
    plan.set_filter(torch.from_numpy(_data(rng, 1, n, ct)).cuda())  # spectra again: the taps are forgotten
    with pytest.raises(pf.invalid_configuration, match="needs pfft_plan_set_filter_taps"):
        plan.filter(torch.from_numpy(xs).cuda(), y)


def test_refusals_name_the_cause():
    G, pf, torch = _mods()
    from portfft_amd import _lib
    lib = _lib.lib
    n, k = 256, 17
    plan = pf.convolution_descriptor([n]).commit()
    x = torch.zeros(3, 1000, dtype=torch.complex64, device="cuda")
    y = torch.zeros(3, 1016, dtype=torch.complex64, device="cuda")
    taps = torch.ones(2, k, dtype=torch.complex64, device="cuda")

    def status(call, code, text):
        assert call == code, (call, lib.pfft_last_error())
        assert text in lib.pfft_last_error().decode(), lib.pfft_last_error()

    def run(mode=0, i=x.data_ptr(), o=y.data_ptr(), ns=3, il=1000, ip=1000, ol=1016, op=1016, p=None):
        return lib.pfft_execute_filter(plan._plan if p is None else p, mode, i, o, ns, il, ip, ol, op)

    INVALID, UNSUPPORTED = 1, 2
    # no filter yet; a plan without the bit
    status(run(), INVALID, "needs pfft_plan_set_filter_taps")
    plain = G.make_descriptor([n], "f32").commit()
    status(run(p=plain._plan), INVALID, "PFFT_EXT_CONVOLUTION")
    status(lib.pfft_plan_set_filter_taps(plain._plan, taps.data_ptr(), k, 2), INVALID, "PFFT_EXT_CONVOLUTION")
    with pytest.raises(pf.invalid_configuration, match="convolution_descriptor"):
        plain.filter(x, y)
    with pytest.raises(pf.invalid_configuration, match="convolution_descriptor"):
        plain.set_filter_taps(taps)
    # set_filter_taps
    status(lib.pfft_plan_set_filter_taps(plan._plan, None, k, 2), INVALID, "null taps pointer")
    status(lib.pfft_plan_set_filter_taps(plan._plan, taps.data_ptr(), 0, 2), INVALID, "number of taps 0")
    status(lib.pfft_plan_set_filter_taps(plan._plan, taps.data_ptr(), n + 1, 2), INVALID, "number of taps %d" % (n + 1))
    status(lib.pfft_plan_set_filter_taps(plan._plan, taps.data_ptr(), k, 0), INVALID, "number of filters 0")
    status(lib.pfft_plan_set_filter_taps(plan._plan, taps.data_ptr(), k, 1 << 32), INVALID, "number of filters")
    status(run(), INVALID, "needs pfft_plan_set_filter_taps")  # none of them became the filter
    plan.set_filter_taps(taps)
    # execute_filter
    status(run(mode=2), INVALID, "Invalid filter mode 2")
    status(run(i=None), INVALID, "null data pointer")
    status(run(o=None), INVALID, "null data pointer")
    status(run(ns=0), INVALID, "zero count")
    status(run(il=0, ip=0), INVALID, "zero count")
    status(run(ol=0), INVALID, "zero count")
    status(run(ol=1017, op=1017), INVALID, "out_length 1017 beyond 1016")
    status(run(mode=1, ol=1001), INVALID, "out_length 1001 beyond 1000")
    status(run(ip=999), INVALID, "below the lengths")
    status(run(ol=1000, op=999), INVALID, "below the lengths")
    status(run(o=x.data_ptr(), ol=1000, op=1000), INVALID, "overlap")  # in == out
    status(run(o=x.data_ptr() + 8 * 2999), INVALID, "overlap")  # the last input element is the first output
    assert run(ns=1, i=x.data_ptr(), o=x.data_ptr() + 8 * 1000, ol=1000, op=1000) == 0  # adjacent is not overlapping
    # beyond the kernel's 32-bit byte offsets (nothing is launched: the pointers are never followed)
    status(run(ns=1, il=1 << 29, ip=1 << 29, ol=1 << 29, op=1 << 29, o=x.data_ptr() + (1 << 40)), UNSUPPORTED, "4 GiB")
    status(run(ns=16, il=1000, ip=1 << 26, ol=1000, op=1000, o=x.data_ptr() + (1 << 40)), UNSUPPORTED, "4 GiB")
    status(run(ns=1 << 31, il=10, ip=10, ol=10, op=10, o=x.data_ptr() + (1 << 40)), UNSUPPORTED, "2^31")
    plan.wait()
    # the binding: shapes, types and strides before the library is called
    for bad_x, bad_y in ((x.to(torch.complex128), y), (x, y.real.contiguous()), (x[:2], y), (x, y[:, ::2]), (x.cpu(), y),
                         (x.reshape(3, 10, 100), y), (x[:, :0], y), (x.cpu().numpy(), y)):
        with pytest.raises(pf.invalid_configuration):
            plan.filter(bad_x, bad_y)
    for bad in (taps.to(torch.complex128), taps.real.contiguous(), torch.ones(2, n + 1, dtype=torch.complex64, device="cuda"),
                torch.ones(2, 0, dtype=torch.complex64, device="cuda"), taps.cpu(), taps.cpu().numpy(),
                torch.ones(2, 2 * k, dtype=torch.complex64, device="cuda")[:, ::2]):
        with pytest.raises(pf.invalid_configuration):
            plan.set_filter_taps(bad)
    with pytest.raises(pf.invalid_configuration, match="overlap"):
        plan.filter(x, x)
    plan.filter(x, y).wait()
    assert float(y.abs().max()) == 0.0


@pytest.mark.parametrize("prec,n,k", [("f32", 2048, 300), ("f64", 3000, 41)])
def test_dependencies_and_events(prec, n, k):
    G, pf, torch = _mods()
    ct = _ct(prec)
    plan, c, _ = _plan(pf, n, prec)
    rng = np.random.Generator(np.random.SFC64(5 * n))
    x = _data(rng, 4, 2 * n + 11, ct)
    h = _data(rng, 2, k, ct, 1.0 / np.sqrt(k))
    plan.set_filter_taps(torch.from_numpy(h).cuda())
    bits = _filter(G, torch, plan, c, n, x, h, x.shape[1], False, (prec, n, k, "plain call"))
    seen = {}

    def with_events(xv, yv):
        # the input is written by another stream; the execute is ordered behind it by the event alone
        side = torch.cuda.Stream()
        staged = xv.clone()
        xv.zero_()
        torch.cuda.current_stream().synchronize()
        with torch.cuda.stream(side):
            xv.copy_(staged)
            dep = torch.cuda.Event()
            dep.record(side)
        ev = plan.filter(xv, yv, dependencies=[dep])
        assert ev.native
        ev.wait()
        assert ev.is_complete()
        seen["bits"] = yv.cpu().numpy().copy()  # read right behind the event, before any other wait

    ebits = _filter(G, torch, plan, c, n, x, h, x.shape[1], False, (prec, n, k, "with events"), verb=with_events)
    H.check_unchanged(bits, ebits, what="filter with a dependency and a returned event")
    H.check_unchanged(bits, seen["bits"], what="the output behind the returned event")
    xd = torch.from_numpy(x).cuda()
    y = torch.empty(4, x.shape[1], dtype=xd.dtype, device="cuda")
    ev = plan.filter(xd, y, correlate=True, want_event=False)
    assert not ev.native
    ev.wait()
    _check(y.cpu().numpy().astype(np.complex128), _reference(c, x, h, x.shape[1], True), ct, n, (prec, n, "want_event=False"))
