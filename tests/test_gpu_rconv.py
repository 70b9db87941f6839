"""Fused circular convolution of REAL rows on the GPU (pf.real_convolution_descriptor: stockham_wg_rconv_kernel): every row
of every case against NumPy in double precision -- forward_scale * backward_scale * N * irfft(rfft(x) * H[t % F]), with
conj(H) for correlate -- with the project's two yardsticks unchanged (per-row relative L2 within helpers.REL_L2_TOL,
helpers.check_reference_rule with n = N; real arrays cast to complex, as test_gpu_real.py does).  Rows are uniform in
[-1, 1], spectra uniform in [-1, 1] per component (the imaginary parts of bins 0 and N/2 are garbage the kernel must
ignore, as C2R does).

Every launch runs on gpu_utils.Guarded buffers: the guards, every scalar in front of the offset and between the rows and
the whole input of an out-of-place call must be unchanged, bit for bit.  A real descriptor's rows are PACKED (pitch N)
or the padded in-place pair (pitch N + 2): those are the two pitches the descriptor's rules allow, so an odd pitch
cannot occur here (tests/test_gpu_rfilter.py has them); offsets are odd out of place, and once per case the base
pointers are one scalar off 128-byte alignment.

One length per kernel shape: M = 2, single-pass STAGED, TWL two-pass, FPW 16 / 4 / 2 / 1 with TW_REGS, 32.16.16, and
lengths compiled at commit (every registered line of the kernel runs in test_gpu_fused_registry.py).  Batches 1,
2 FPW - 1 and 2 FPW + 1; one filter and one per row; out of place and
in == out; both modes.

Measured on the MI355X (worst row of every case of a length, both modes): fp32 rel-L2 1.7e-7 (N = 128) ... 2.7e-7
(N = 64), fp64 4.9e-16 (N = 1024) ... 6.5e-16 (N = 6000).

No case is skipped: a commit that answers unsupported_configuration inside the supported set fails the test."""
import numpy as np
import pytest

import helpers as H

pytestmark = pytest.mark.gpu

LENGTHS = {"f32": [4, 8, 32, 64, 128, 512, 1024, 4096, 8192, 16384, 2000, 12000], "f64": [128, 1024, 8192, 6000]}
CASES = [(p, n) for p in ("f32", "f64") for n in LENGTHS[p]]


def _mods():
    import gpu_utils as G
    import portfft_amd as pf
    return G, pf, G.torch_mod()


def _types(prec):
    return (np.float32, np.complex64) if prec == "f32" else (np.float64, np.complex128)


def _desc(pf, n, prec, batch=1, padded=False, offset=0, scales=(1.0, 1.0), make=None):
    d = (make or pf.real_convolution_descriptor)(n, prec)
    d.number_of_transforms = batch
    d.forward_scale, d.backward_scale = scales
    if padded:  # the padded in-place pair: rows of N + 2 scalars
        d.placement = pf.placement.IN_PLACE
        d.forward_distance = 2 * d.backward_distance
        d.forward_offset, d.backward_offset = 2 * offset, offset
    else:
        d.forward_offset = offset
    return d


def _spectra(rng, count, n, ct):
    bins = n // 2 + 1
    return (rng.uniform(-1, 1, (count, bins)) + 1j * rng.uniform(-1, 1, (count, bins))).astype(ct)


def _reference(d, x, h, correlate):
    """NumPy in double: fs * bs * N * irfft(rfft(x) * H[t % F]), conj(H) for correlate"""
    n = x.shape[1]
    hh = h.astype(np.complex128)[np.arange(x.shape[0]) % h.shape[0]]
    hh[:, 0] = hh[:, 0].real  # (what C2R ignores)
    hh[:, n // 2] = hh[:, n // 2].real
    if correlate:
        hh = np.conj(hh)
    return d.forward_scale * d.backward_scale * n * np.fft.irfft(np.fft.rfft(x.astype(np.float64), axis=1) * hh, n, axis=1)


_worst = {}


def _check(got, ref, ct, n, what):
    got = np.asarray(got).astype(np.complex128)
    ref = np.asarray(ref).astype(np.complex128)
    err = np.linalg.norm(got - ref, axis=1) / np.maximum(np.linalg.norm(ref, axis=1), 1e-300)
    key = np.dtype(ct).name
    _worst[key] = max(_worst.get(key, 0.0), float(err.max()))
    print("%s: worst rel-L2 %.3e (row %d)" % (what, float(err.max()), int(np.argmax(err))))
    assert np.all(err <= H.REL_L2_TOL[np.dtype(ct)]), (what, "row", int(np.argmax(err)), float(err.max()))
    assert H.check_reference_rule(got, ref.astype(ct), n), (what, "per-element reference rule")


def _run(G, pf, torch, d, x, h, plan, correlate, what, same_buffer=False, guard=None, verb=None):
    """one verb of `plan` (committed from d, filter h set) on the rows x through d's forward layout, which is the layout
    of the input and of the output; every row checked.  Returns the raw output scalars of the rows (bits)."""
    rt, ct = _types(d.scalar)
    n, batch = d.lengths[0], d.number_of_transforms
    guard = G.GUARD if guard is None else guard
    count = d.get_input_count(pf.direction.FORWARD)
    idx = (d.forward_offset + np.arange(batch)[:, None] * d.forward_distance + np.arange(n)[None, :]).astype(np.int64)
    host = np.full(count, H.PADDING_VALUE, rt)
    host[idx.ravel()] = x.astype(rt).ravel()
    dtype = torch.from_numpy(host[:0]).dtype
    gin = G.Guarded(count, dtype, guard)
    gin.buf.copy_(torch.from_numpy(host))
    gout = gin if same_buffer else G.Guarded(count, dtype, guard)
    fn = verb or (plan.correlate if correlate else plan.convolve)
    if same_buffer:
        fn(gin.buf)
    else:
        fn(gin.buf, gout.buf)
    plan.wait()
    what = what + ("corr" if correlate else "conv", "in == out" if same_buffer else "oop")
    gin.check(str(what) + ": input")
    gout.check(str(what) + ": output")
    if not same_buffer:
        H.check_unchanged(host, gin.buf.cpu().numpy(), what=str(what) + ": the input")
    raw = gout.buf.cpu().numpy()
    H.check_write_set(raw, idx, what=str(what) + ": output buffer")
    _check(raw[idx], _reference(d, x, h, correlate), ct, n, what)
    return raw[idx]


def _commit(pf, torch, d, h):
    plan = d.commit()
    plan.set_filter(torch.from_numpy(h).cuda())
    return plan


def _fpw(pf, n, prec):
    info = _desc(pf, n, prec).commit().info()
    dim = info.dims[0]
    assert dim.length == n and dim.tier == 1 and tuple(info.launches) == (1, 1)
    assert int(np.prod(dim.factors[:dim.n_factors])) == n // 2
    return max(1, dim.ffts_per_workgroup), dim


@pytest.mark.parametrize("prec,n", CASES)
def test_convolve_and_correlate_against_numpy(prec, n):
    G, pf, torch = _mods()
    rt, ct = _types(prec)
    fpw, dim = _fpw(pf, n, prec)
    print("N=%d %s: factors %s fpw %d lds %d" % (n, prec, list(dim.factors[:dim.n_factors]), fpw, dim.lds_bytes))
    rng = np.random.Generator(np.random.SFC64(n))
    for batch in sorted({1, 2 * fpw - 1, 2 * fpw + 1}):
        x = rng.uniform(-1, 1, (batch, n)).astype(rt)
        for nf in sorted({1, batch}):
            h = _spectra(rng, nf, n, ct)
            d = _desc(pf, n, prec, batch)
            plan = _commit(pf, torch, d, h)
            for correlate in (False, True):
                for same in (False, True):
                    _run(G, pf, torch, d, x, h, plan, correlate, (prec, n, batch, nf), same)
        # offsets and scales off their defaults: an odd offset on packed rows (base one scalar off 128 bytes), and the
        # padded in-place pair (rows of N + 2 scalars), in == out and out of place
        scales = (0.5, 0.25 / n)
        h = _spectra(rng, min(batch, 3), n, ct)
        for padded, offset, guard, name in ((False, 5, (65, 63), "packed, odd offset"), (True, 3, (63, 65), "padded rows")):
            d = _desc(pf, n, prec, batch, padded, offset, scales)
            plan = _commit(pf, torch, d, h)
            for correlate in (False, True):
                for same in (False, True):
                    _run(G, pf, torch, d, x, h, plan, correlate, (prec, n, batch, name), same, guard)
    print("worst rel-L2 so far: %s" % _worst)


@pytest.mark.parametrize("prec,n", [("f32", 64), ("f32", 4096), ("f32", 2000), ("f64", 1024)])
def test_many_trips_of_the_persistent_loop(prec, n):
    G, pf, torch = _mods()
    rt, ct = _types(prec)
    fpw, _ = _fpw(pf, n, prec)
    batch = 1000 * fpw + 1
    rng = np.random.Generator(np.random.SFC64(3 * n + 1))
    x = rng.uniform(-1, 1, (batch, n)).astype(rt)
    h = _spectra(rng, 3, n, ct)
    d = _desc(pf, n, prec, batch)
    _run(G, pf, torch, d, x, h, _commit(pf, torch, d, h), False, (prec, n, batch, 3))


@pytest.mark.parametrize("prec,n", [("f32", 2000), ("f32", 4096), ("f64", 128)])
def test_the_plain_transforms_are_the_real_descriptors(prec, n):
    """compute_forward / compute_backward of a plan with the bit: the plan info and the output bits of a real_descriptor
    plan; and a spectrum made with the plan itself is the filter the verb expects"""
    G, pf, torch = _mods()
    rt, ct = _types(prec)
    batch, bins = 7, n // 2 + 1
    rng = np.random.Generator(np.random.SFC64(n))
    x = rng.uniform(-1, 1, (batch, n)).astype(rt)
    spec = _spectra(rng, batch, n, ct)
    plain, withbit = _desc(pf, n, prec, batch, make=pf.real_descriptor), _desc(pf, n, prec, batch)
    pp, wp = plain.commit(), withbit.commit()
    assert bytes(pp.info()) == bytes(wp.info()), "the plan info of a descriptor with PFFT_EXT_REAL_CONVOLUTION is the real one's"
    rdt, cdt = torch.from_numpy(x[:0]).dtype, torch.from_numpy(spec[:0]).dtype
    xd, sd = torch.from_numpy(x.ravel()).cuda(), torch.from_numpy(spec.ravel()).cuda()
    outs = []
    for p in (pp, wp):
        y = torch.full((batch * bins,), H.PADDING_VALUE, dtype=cdt, device="cuda")
        back = torch.full((batch * n,), H.PADDING_VALUE, dtype=rdt, device="cuda")
        p.compute_forward(xd, y).wait()
        p.compute_backward(sd, back).wait()
        outs.append((y.cpu().numpy(), back.cpu().numpy()))
    H.check_unchanged(outs[0][0], outs[1][0], what="compute_forward with PFFT_EXT_REAL_CONVOLUTION")
    H.check_unchanged(outs[0][1], outs[1][1], what="compute_backward with PFFT_EXT_REAL_CONVOLUTION")
    _check(outs[1][0].reshape(batch, bins), np.fft.rfft(x.astype(np.float64), axis=1), ct, n, (prec, n, "forward is rfft"))
    # the filter made by the plan: circular convolution with a real filter g
    g = rng.uniform(-1, 1, (1, n)).astype(rt)
    one = _desc(pf, n, prec, 1).commit()
    hd = torch.empty(bins, dtype=cdt, device="cuda")
    one.compute_forward(torch.from_numpy(g.ravel()).cuda(), hd).wait()
    wp.set_filter(hd)
    got = _run(G, pf, torch, withbit, x, hd.cpu().numpy().reshape(1, bins), wp, False, (prec, n, "spectrum by the same plan"))
    direct = np.fft.irfft(np.fft.rfft(x.astype(np.float64), axis=1) * np.fft.rfft(g.astype(np.float64), axis=1), n, axis=1) * n
    _check(got, direct, ct, n, (prec, n, "against the filter in the time domain"))


@pytest.mark.parametrize("prec,n", [("f32", 512), ("f64", 6000)])
def test_filter_lifetime_and_clones(prec, n):
    G, pf, torch = _mods()
    rt, ct = _types(prec)
    batch = 9
    rng = np.random.Generator(np.random.SFC64(11 * n))
    x = rng.uniform(-1, 1, (batch, n)).astype(rt)
    h1, h2, h3 = _spectra(rng, 3, n, ct), _spectra(rng, batch, n, ct), _spectra(rng, 1, n, ct)
    d = _desc(pf, n, prec, batch)
    plan = d.commit()
    t1 = torch.from_numpy(h1).cuda()
    plan.set_filter(t1)
    plan.wait()
    t1.fill_(7.0)  # the caller's tensor is the caller's again
    torch.cuda.synchronize()
    bits1 = _run(G, pf, torch, d, x, h1, plan, False, (prec, n, "after overwriting the caller's tensor"))
    clone = plan.copy()
    H.check_unchanged(bits1, _run(G, pf, torch, d, x, h1, clone, False, (prec, n, "clone, shared filter")),
                      what="a clone convolves with the shared filter")
    clone.set_filter(torch.from_numpy(h2).cuda())  # detaches the clone
    _run(G, pf, torch, d, x, h2, clone, True, (prec, n, "clone, its own filter"))
    H.check_unchanged(bits1, _run(G, pf, torch, d, x, h1, plan, False, (prec, n, "original after the clone's set_filter")),
                      what="the original's results after set_filter on the clone")
    plan.set_filter(torch.from_numpy(h3.ravel()).cuda())  # shape (N/2 + 1,): one shared filter, for later executes
    _run(G, pf, torch, d, x, h3, plan, False, (prec, n, "second set_filter"))
    _run(G, pf, torch, d, x, h2, clone, False, (prec, n, "clone after the original's set_filter"))


@pytest.mark.parametrize("prec,n", [("f32", 4096), ("f64", 6000)])
def test_dependencies_and_events(prec, n):
    G, pf, torch = _mods()
    rt, ct = _types(prec)
    batch = 5
    rng = np.random.Generator(np.random.SFC64(7 * n))
    x, h = rng.uniform(-1, 1, (batch, n)).astype(rt), _spectra(rng, 2, n, ct)
    d = _desc(pf, n, prec, batch)
    plan = _commit(pf, torch, d, h)
    bits = _run(G, pf, torch, d, x, h, plan, False, (prec, n, "plain call"))
    seen = {}

    def with_events(*bufs):
        # the input is written by another stream; the execute is ordered behind it by the event alone
        side = torch.cuda.Stream()
        staged = bufs[0].clone()
        bufs[0].zero_()
        torch.cuda.current_stream().synchronize()
        with torch.cuda.stream(side):
            bufs[0].copy_(staged)
            dep = torch.cuda.Event()
            dep.record(side)
        ev = plan.convolve(*bufs, dependencies=[dep])
        assert ev.native
        ev.wait()
        assert ev.is_complete()
        seen["bits"] = bufs[-1].cpu().numpy().copy()  # read right behind the event, before any other wait

    ebits = _run(G, pf, torch, d, x, h, plan, False, (prec, n, "with events"), verb=with_events)
    H.check_unchanged(bits, ebits, what="convolve with a dependency and a returned event")
    H.check_unchanged(bits.ravel(), seen["bits"][:bits.size], what="the output behind the returned event")
    y = torch.empty(batch * n, dtype=torch.from_numpy(x[:0]).dtype, device="cuda")
    ev = plan.correlate(torch.from_numpy(x.ravel()).cuda(), y, want_event=False)
    assert not ev.native
    ev.wait()
    _check(y.cpu().numpy().reshape(batch, n), _reference(d, x, h, True), ct, n, (prec, n, "want_event=False"))


def test_verbs_and_filters_that_are_invalid():
    G, pf, torch = _mods()
    from portfft_amd import _lib
    lib = _lib.lib
    n, batch, bins = 256, 4, 129
    d = _desc(pf, n, "f32", batch)
    plan = d.commit()
    x = torch.zeros(batch * n, dtype=torch.float32, device="cuda")
    y = torch.empty_like(x)
    for verb in (plan.convolve, plan.correlate):
        with pytest.raises(pf.invalid_configuration, match="no filter"):
            verb(x, y)
        with pytest.raises(pf.invalid_configuration, match="no filter"):
            verb(x)
    good = torch.ones(2, bins, dtype=torch.complex64, device="cuda")
    for bad in (good.to(torch.complex128), good.real.contiguous(), torch.ones(2, n, dtype=torch.complex64, device="cuda"),
                torch.ones(bins - 1, dtype=torch.complex64, device="cuda"), torch.ones(0, bins, dtype=torch.complex64, device="cuda"),
                good.cpu(), torch.ones(2, 2 * bins, dtype=torch.complex64, device="cuda")[:, ::2], good.cpu().numpy()):
        with pytest.raises(pf.invalid_configuration):
            plan.set_filter(bad)
    with pytest.raises(pf.invalid_configuration, match="no filter"):
        plan.convolve(x, y)  # none of them became the filter
    plan.set_filter(good)
    for bad in (x[:-1], x.to(torch.float64), x.cpu()):
        with pytest.raises(pf.invalid_configuration):
            plan.convolve(bad, y)
        with pytest.raises(pf.invalid_configuration):
            plan.convolve(x, bad)
    with pytest.raises(pf.invalid_configuration):
        plan.convolve(x, y, y)
    assert lib.pfft_execute_convolve(plan._plan, 2, x.data_ptr(), y.data_ptr()) == 1
    assert b"Invalid convolution mode 2" in lib.pfft_last_error()
    plan.convolve(x, y).wait()
    assert float(y.abs().max()) == 0.0
    # a real_descriptor's plan has no such verbs: status and message of the C ABI, and the binding
    plain = _desc(pf, n, "f32", batch, make=pf.real_descriptor).commit()
    assert lib.pfft_plan_set_filter(plain._plan, good.data_ptr(), 2) == 1
    assert b"PFFT_EXT_REAL_CONVOLUTION" in lib.pfft_last_error()
    assert lib.pfft_execute_convolve(plain._plan, 0, x.data_ptr(), y.data_ptr()) == 1
    assert b"PFFT_EXT_REAL_CONVOLUTION" in lib.pfft_last_error()
    with pytest.raises(pf.invalid_configuration):
        plain.set_filter(good)
    with pytest.raises(pf.invalid_configuration):
        plain.convolve(x, y)


@pytest.mark.parametrize("prec,n,reason", [("f32", 32768, "register-resident"), ("f32", 1 << 21, "work-group plan"),
                                           ("f32", 67 * 16, "work-group plan"), ("f64", 16384, "register-resident")])
def test_refusals_at_commit_are_the_real_plans(prec, n, reason):
    """what plan_real refuses is refused with its reason, and with the same one as for a real_descriptor"""
    G, pf, torch = _mods()
    msgs = []
    for make in (pf.real_convolution_descriptor, pf.real_descriptor):
        d = _desc(pf, n, prec, 2, make=make)
        d.validate()
        with pytest.raises(pf.unsupported_configuration) as e:
            d.commit()
        msgs.append(str(e.value))
    assert msgs[0] == msgs[1], msgs
    assert "real transform of length %d" % n in msgs[0], msgs[0]
    print(msgs[0])
    assert reason in msgs[0], msgs[0]
