"""Overlap-save FIR filtering of REAL signals on the GPU (plan.set_filter_taps / plan.filter of a
pf.real_convolution_descriptor: stockham_wg_rols_kernel): every signal of every case against NumPy in double precision,
    convolve   c * np.convolve(x, h)[:out_length]
    correlate  c * np.correlate(concatenate(x, zeros(K - 1)), h, "valid")[:out_length]
with c = forward_scale * backward_scale * N, and the project's two yardsticks unchanged: relative L2 per signal within
helpers.REL_L2_TOL and helpers.check_reference_rule with n = N (real arrays cast to complex, as test_gpu_real.py does).
Signals are uniform in [-1, 1], taps uniform in [-1, 1] / sqrt(K).

The kernel works on scalar pairs with an even geometry: convolve lead = K - 1 rounded up to even and hop = N - lead,
correlate hop = N - K + 1 rounded down to even (_hop below restates the host's choice; the scenarios are built on it).

One length per kernel shape (M = 2, single-pass STAGED, TWL two-pass, FPW 16 / 4 / 2 / 1 with TW_REGS, 32.16.16,
lengths compiled at commit; every registered line of the kernel runs in test_gpu_fused_registry.py), and per length the tap counts K = 1, 2, ceil(N/4) + 1, floor(5N/8) and, up to N = 128,
K = N - 2 (hop 2).  Per (N, K), both modes, the scenarios of test_gpu_filter.py::_scenarios: one segment, exact multiples
of the hop, ragged last segments, outputs at their bound and shorter than the input, 1 and 3 signals and counts that
put the number of (signal, segment) rows at or next to 2 FPW - 1 and 2 FPW + 1, one filter and one per signal -- and,
new here, the ragged scenarios once more with in_length and out_length one longer, so that odd and even lengths both
occur: the per-scalar edge of a pair at the end of a signal.  Apart from the single-signal one-segment case, every
output has at least K samples (test_gpu_filter.py's rule: shorter outputs make the relative measure ill-conditioned).

Every launch writes into a gpu_utils.Guarded buffer whose signals are pitched wider than their lengths, with ODD
pitches: the guards, every scalar between the signals and the whole input must be unchanged, bit for bit.  Once per
case the base pointers are one scalar off 128-byte alignment.

Measured on the MI355X (worst signal of every case of a length, both modes): fp32 rel-L2 2.2e-7 (N = 1024) ... 4.8e-7
(N = 8) and 1.99e-6 at N = 4, fp64 5.1e-16 (N = 1024) ... 6.4e-16 (N = 6000).  The N = 4 figure is one of the 513
two-sample signals of K = 2, correlate (2 FPW + 1 signals at FPW = 256): x = (0.994, 0.011), h = (0.0013, 0.324) give
||y|| = 0.015 c ||x|| ||h||, so a single rounding of 2^-24 relative to c ||x|| ||h|| is 3.9e-6 of ||y|| -- the conditioning of
the measure at the smallest shape, not the kernel (accuracy).

No case is skipped."""
import numpy as np
import pytest

import helpers as H

pytestmark = pytest.mark.gpu

LENGTHS = {"f32": [4, 8, 32, 64, 128, 512, 1024, 4096, 8192, 16384, 2000, 12000], "f64": [128, 1024, 8192, 6000]}


def _taps_of(n):
    ks = [1, 2, -(-n // 4) + 1, (5 * n) // 8]
    if n <= 128:
        ks.append(n - 2)
    return sorted({k for k in ks if k <= n - 2})


CASES = [(p, n, k) for p in ("f32", "f64") for n in LENGTHS[p] for k in _taps_of(n)]
SCALED = (0.5, 0.25)  # forward_scale, backward_scale * N of the second plan of a length


def _mods():
    import gpu_utils as G
    import portfft_amd as pf
    return G, pf, G.torch_mod()


def _types(prec):
    return (np.float32, np.complex64) if prec == "f32" else (np.float64, np.complex128)


def _hop(n, k, correlate):
    """the even geometry the host chooses (include/portfft_amd.h)"""
    return (n - k + 1) & ~1 if correlate else n - ((k - 1 + 1) & ~1)


_plans = {}


def _plan(pf, n, prec, scaled=False):
    """(plan, c, fpw) of a length: committed once per process, the filter is set per case"""
    key = (n, prec, scaled)
    if key not in _plans:
        d = pf.real_convolution_descriptor(n, prec)
        if scaled:
            d.forward_scale, d.backward_scale = SCALED[0], SCALED[1] / n
        plan = d.commit()
        dim = plan.info().dims[0]
        _plans[key] = (plan, d.forward_scale * d.backward_scale * n, max(1, dim.ffts_per_workgroup))
    return _plans[key]


def _reference(c, x, h, out_length, correlate):
    """NumPy in double, signal by signal; filter i mod F"""
    k = h.shape[1]
    ref = np.empty((x.shape[0], out_length), dtype=np.float64)
    for i in range(x.shape[0]):
        xi, hi = x[i].astype(np.float64), h[i % h.shape[0]].astype(np.float64)
        if correlate:
            full = np.correlate(np.concatenate([xi, np.zeros(k - 1)]), hi, "valid")
        else:
            full = np.convolve(xi, hi)
        ref[i] = c * full[:out_length]
    return ref


_worst = {}


def _check(got, ref, ct, n, what):
    got = np.asarray(got).astype(np.complex128)
    ref = np.asarray(ref).astype(np.complex128)
    err = np.linalg.norm(got - ref, axis=1) / np.maximum(np.linalg.norm(ref, axis=1), 1e-300)
    key = np.dtype(ct).name
    _worst[key] = max(_worst.get(key, 0.0), float(err.max()))
    print("%s: worst rel-L2 %.3e (signal %d)" % (what, float(err.max()), int(np.argmax(err))))
    assert np.all(err <= H.REL_L2_TOL[np.dtype(ct)]), (what, "signal", int(np.argmax(err)), float(err.max()))
    assert H.check_reference_rule(got, ref.astype(ct), n), (what, "per-element reference rule")


def _odd(v):
    return v | 1


def _filter(G, torch, plan, c, n, x, h, out_length, correlate, what, pads=(3, 5), guard=None, verb=None):
    """plan.filter of the signals x (numpy, (signals, in_length)) with the taps h already set: buffers with odd pitches
    above the lengths, write set, guards, unchanged input, every signal against the reference.  Returns the output
    signals (numpy)."""
    ns, in_length = x.shape
    ct = np.complex64 if x.dtype == np.float32 else np.complex128
    in_pitch, out_pitch = _odd(in_length + pads[0]), _odd(out_length + pads[1])
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
    got = raw.reshape(ns, out_pitch)[:, :out_length]
    _check(got, _reference(c, x, h, out_length, correlate), ct, n, what)
    return got


def _scenarios(n, k, fpw, correlate):
    """(name, signals, filters, in_length, out_length, scaled plan, guard): test_gpu_filter.py::_scenarios on the even
    hop of this kernel, and the ragged ones in both parities"""
    hop = _hop(n, k, correlate)
    extra = 0 if correlate else k - 1  # out_length <= in_length + extra
    out = []
    # one segment, at the bound where the bound allows one (its output may be shorter than K: one signal, one filter)
    l1 = max(1, hop - extra)
    o1 = min(hop, l1 + extra)
    out.append(("one segment", 1, 1, l1, o1, False, None))
    # short signals, 2 FPW - 1 of them with one filter and 2 FPW + 1 with a filter each: the fewest segments that hold K
    # outputs
    ls, os_ = max(l1, k if correlate else 1), max(o1, k)
    out.append(("short signals, 2 fpw - 1 of them", 2 * fpw - 1, 1, ls, os_, False, None))
    out.append(("short signals, 2 fpw + 1 of them", 2 * fpw + 1, 2 * fpw + 1, ls, os_, False, None))
    # an exact multiple of the hop (correlate: at its bound): two hops, or as many as hold K outputs; base pointers one
    # scalar off 128-byte alignment
    whole = max(2, -(-k // hop)) * hop
    out.append(("whole hops", 3, 3, whole, whole, False, (65, 63)))
    # ragged last segment, the output at its bound; odd and even lengths
    lr = max(2 * hop + hop // 2 + 1, k)
    for more in (0, 1):
        out.append(("ragged, at the bound, in %d" % (lr + more), 3, 1, lr + more, lr + more + extra, False, None))
    # the output shorter than the input, ragged, n_signals * S just above and just below 2 FPW + 1 / 2 FPW - 1 rows
    o_short = max(2 * hop + (hop + 1) // 2, k)  # S = 3, or as many segments as hold K outputs
    seg = -(-o_short // hop)
    many = -(-(2 * fpw + 1) // seg)
    few = max(1, (2 * fpw - 1) // seg)
    for more in (0, 1):
        o, l_ = o_short + more, o_short + more + 3 - more  # (in_length of the other parity than out_length, then the same)
        out.append(("shorter than the input, %d rows, out %d" % (many * -(-o // hop), o), many, many, l_, o, True, None))
    out.append(("shorter than the input, %d rows" % (few * seg), few, 1, o_short + 3, o_short, False, None))
    return out


@pytest.mark.parametrize("prec,n,k", CASES)
def test_filter_against_numpy(prec, n, k):
    G, pf, torch = _mods()
    rt, ct = _types(prec)
    rng = np.random.Generator(np.random.SFC64(1000 * n + k))
    fpw = _plan(pf, n, prec)[2]
    print("N=%d K=%d %s: hops %d / %d fpw %d" % (n, k, prec, _hop(n, k, False), _hop(n, k, True), fpw))
    parities = set()
    for correlate in (False, True):
        for name, ns, nf, in_length, out_length, scaled, guard in _scenarios(n, k, fpw, correlate):
            plan, c, _ = _plan(pf, n, prec, scaled)
            x = rng.uniform(-1, 1, (ns, in_length)).astype(rt)
            h = (rng.uniform(-1, 1, (nf, k)) / np.sqrt(k)).astype(rt)
            plan.set_filter_taps(torch.from_numpy(h).cuda())
            _filter(G, torch, plan, c, n, x, h, out_length, correlate,
                    (prec, n, k, "corr" if correlate else "conv", name, ns, nf, in_length, out_length), guard=guard)
            parities.add((correlate, in_length % 2, out_length % 2))
    for correlate in (False, True):  # odd and even in_length and out_length, in both modes
        for side in (1, 2):
            assert {p[side] for p in parities if p[0] == correlate} == {0, 1}, (correlate, side, parities)
    print("worst rel-L2 so far: %s" % _worst)


@pytest.mark.parametrize("prec,n,k", [("f32", 512, 9), ("f64", 6000, 17), ("f32", 8192, 17)])
def test_many_trips_of_the_persistent_loop(prec, n, k):
    """more (signal, segment) rows than the grid holds work-groups"""
    G, pf, torch = _mods()
    rt, ct = _types(prec)
    plan, c, fpw = _plan(pf, n, prec)
    hop = _hop(n, k, False)
    rng = np.random.Generator(np.random.SFC64(7 * n + k))
    ns = 5
    segs = (1500 * fpw) // ns + 1
    in_length = segs * hop - 7
    x = rng.uniform(-1, 1, (ns, in_length)).astype(rt)
    h = (rng.uniform(-1, 1, (2, k)) / np.sqrt(k)).astype(rt)
    plan.set_filter_taps(torch.from_numpy(h).cuda())
    ref = _reference(c, x, h, in_length, False)
    gout = G.Guarded(ns * in_length, torch.from_numpy(x[:0]).dtype)
    xd = torch.from_numpy(x).cuda()
    plan.filter(xd, gout.buf.view(ns, in_length))
    plan.wait()
    gout.check("many trips: output")
    _check(gout.buf.cpu().numpy().reshape(ns, in_length), ref, ct, n, (prec, n, k, "many trips"))


@pytest.mark.parametrize("prec,n,k", [("f32", 1024, 100), ("f64", 6000, 700)])
def test_taps_are_a_filter_like_any_other(prec, n, k):
    G, pf, torch = _mods()
    rt, ct = _types(prec)
    rng = np.random.Generator(np.random.SFC64(13 * n))
    batch = 5
    d = pf.real_convolution_descriptor(n, prec)
    d.number_of_transforms = batch
    plan = d.commit()
    c = float(n)
    rows = rng.uniform(-1, 1, (batch, n)).astype(rt)
    xs = rng.uniform(-1, 1, (2, 3 * n + 5)).astype(rt)
    h1 = (rng.uniform(-1, 1, (2, k)) / np.sqrt(k)).astype(rt)
    h2 = (rng.uniform(-1, 1, (1, k // 2)) / np.sqrt(k // 2)).astype(rt)
    rd = torch.from_numpy(rows.ravel()).cuda()

    def circular(p, h, correlate):
        """convolve / correlate of the plan against circular convolution with the zero-padded taps"""
        y = torch.empty_like(rd)
        (p.correlate if correlate else p.convolve)(rd, y).wait()
        hp = np.zeros((h.shape[0], n))
        hp[:, :h.shape[1]] = h
        spec = np.fft.rfft(hp, axis=1)[np.arange(batch) % h.shape[0]]
        ref = n * np.fft.irfft(np.fft.rfft(rows.astype(np.float64), axis=1) * (np.conj(spec) if correlate else spec), n, axis=1)
        _check(y.cpu().numpy().reshape(batch, n), ref, ct, n, (prec, n, "circular", correlate))

    def linear(p, h, what):
        return _filter(G, torch, p, c, n, xs, h, xs.shape[1], False, (prec, n, what))

    # a plain set_filter gives spectra: filter() is refused, with the way out
    bins = n // 2 + 1
    spectra = (rng.uniform(-1, 1, (1, bins)) + 1j * rng.uniform(-1, 1, (1, bins))).astype(ct)
    plan.set_filter(torch.from_numpy(spectra).cuda())
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
    plan.set_filter(torch.from_numpy(spectra).cuda())  # spectra again: the taps are forgotten
    with pytest.raises(pf.invalid_configuration, match="needs pfft_plan_set_filter_taps"):
        plan.filter(torch.from_numpy(xs).cuda(), y)


def test_refusals_name_the_cause():
    G, pf, torch = _mods()
    from portfft_amd import _lib
    lib = _lib.lib
    n, k = 256, 17
    plan = pf.real_convolution_descriptor(n).commit()
    x = torch.zeros(3, 1000, dtype=torch.float32, device="cuda")
    y = torch.zeros(3, 1016, dtype=torch.float32, device="cuda")
    taps = torch.ones(2, k, dtype=torch.float32, device="cuda")

    def status(call, code, text):
        assert call == code, (call, lib.pfft_last_error())
        assert text in lib.pfft_last_error().decode(), lib.pfft_last_error()

    def run(mode=0, i=x.data_ptr(), o=y.data_ptr(), ns=3, il=1000, ip=1000, ol=1016, op=1016, p=None):
        return lib.pfft_execute_filter(plan._plan if p is None else p, mode, i, o, ns, il, ip, ol, op)

    INVALID, UNSUPPORTED = 1, 2
    # no filter yet; a plan without the bit
    status(run(), INVALID, "needs pfft_plan_set_filter_taps")
    plain = pf.real_descriptor(n).commit()
    status(run(p=plain._plan), INVALID, "PFFT_EXT_REAL_CONVOLUTION")
    status(lib.pfft_plan_set_filter_taps(plain._plan, taps.data_ptr(), k, 2), INVALID, "PFFT_EXT_REAL_CONVOLUTION")
    with pytest.raises(pf.invalid_configuration, match="convolution_descriptor"):
        plain.filter(x, y)
    with pytest.raises(pf.invalid_configuration, match="convolution_descriptor"):
        plain.set_filter_taps(taps)
    # spectra instead of taps
    plan.set_filter(torch.ones(n // 2 + 1, dtype=torch.complex64, device="cuda"))
    status(run(), INVALID, "needs pfft_plan_set_filter_taps")
    # set_filter_taps
    status(lib.pfft_plan_set_filter_taps(plan._plan, None, k, 2), INVALID, "null taps pointer")
    status(lib.pfft_plan_set_filter_taps(plan._plan, taps.data_ptr(), 0, 2), INVALID, "number of taps 0")
    status(lib.pfft_plan_set_filter_taps(plan._plan, taps.data_ptr(), n + 1, 2), INVALID, "number of taps %d" % (n + 1))
    status(lib.pfft_plan_set_filter_taps(plan._plan, taps.data_ptr(), k, 0), INVALID, "number of filters 0")
    status(lib.pfft_plan_set_filter_taps(plan._plan, taps.data_ptr(), k, 1 << 32), INVALID, "number of filters")
    status(run(), INVALID, "needs pfft_plan_set_filter_taps")  # none of them became the filter
    # more than N - 2 taps: a filter for convolve / correlate, refused by filter with the reason
    long_taps = torch.ones(1, n - 1, dtype=torch.float32, device="cuda")
    plan.set_filter_taps(long_taps)
    for mode in (0, 1):
        status(run(mode=mode, ol=1000, op=1000), INVALID, "at most %d taps" % (n - 2))
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
    status(run(o=x.data_ptr() + 4 * 2999), INVALID, "overlap")  # the last input scalar is the first output
    assert run(ns=1, i=x.data_ptr(), o=x.data_ptr() + 4 * 1000, ol=1000, op=1000) == 0  # adjacent is not overlapping
    # beyond the kernel's 32-bit byte offsets, in bytes of scalars (nothing is launched: the pointers are never followed)
    status(run(ns=1, il=1 << 30, ip=1 << 30, ol=1 << 30, op=1 << 30, o=x.data_ptr() + (1 << 40)), UNSUPPORTED, "4 GiB")
    status(run(ns=16, il=1000, ip=1 << 27, ol=1000, op=1000, o=x.data_ptr() + (1 << 40)), UNSUPPORTED, "4 GiB")
    status(run(ns=1 << 31, il=10, ip=10, ol=10, op=10, o=x.data_ptr() + (1 << 40)), UNSUPPORTED, "2^31")
    plan.wait()
    # the binding: shapes, types and strides before the library is called
    for bad_x, bad_y in ((x.to(torch.float64), y), (x, y.to(torch.complex64)), (x[:2], y), (x, y[:, ::2]), (x.cpu(), y),
                         (x.reshape(3, 10, 100), y), (x[:, :0], y), (x.cpu().numpy(), y)):
        with pytest.raises(pf.invalid_configuration):
            plan.filter(bad_x, bad_y)
    for bad in (taps.to(torch.float64), taps.to(torch.complex64), torch.ones(2, n + 1, dtype=torch.float32, device="cuda"),
                torch.ones(2, 0, dtype=torch.float32, device="cuda"), taps.cpu(), taps.cpu().numpy(),
                torch.ones(2, 2 * k, dtype=torch.float32, device="cuda")[:, ::2]):
        with pytest.raises(pf.invalid_configuration):
            plan.set_filter_taps(bad)
    with pytest.raises(pf.invalid_configuration, match="overlap"):
        plan.filter(x, x)
    plan.filter(x, y).wait()
    assert float(y.abs().max()) == 0.0


@pytest.mark.parametrize("prec,n,k", [("f32", 4096, 300), ("f64", 6000, 41)])
def test_dependencies_and_events(prec, n, k):
    G, pf, torch = _mods()
    rt, ct = _types(prec)
    plan, c, _ = _plan(pf, n, prec)
    rng = np.random.Generator(np.random.SFC64(5 * n))
    x = rng.uniform(-1, 1, (4, 2 * n + 11)).astype(rt)
    h = (rng.uniform(-1, 1, (2, k)) / np.sqrt(k)).astype(rt)
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
    _check(y.cpu().numpy(), _reference(c, x, h, x.shape[1], True), ct, n, (prec, n, "want_event=False"))
