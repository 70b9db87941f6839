"""Fused circular convolution on the GPU (pf.convolution_descriptor: stockham_wg_conv_kernel): every row of every case
against NumPy in double precision -- forward_scale * backward_scale * N * ifft(fft(x) * H[t % F]), with conj(H) for
correlate -- with the project's two yardsticks unchanged (per-transform relative L2 within helpers.REL_L2_TOL,
helpers.check_reference_rule with n = N), through gpu_utils.transform_packed: guard bands, the unchanged input of an
out-of-place execute and the write set (padded distances, offsets, in place, a base pointer one element off 128-byte
alignment).  Inputs and spectra are uniform in [-1, 1] per component.

One length per kernel shape: single pass, TWL two-pass, FPW 4, TW_REGS, 32.16.16, and lengths compiled at commit.
Every registered line of the kernel runs in test_gpu_fused_registry.py.

Measured on the MI355X (worst row of every case of a length, both modes):
fp32 rel-L2 1.4e-7 (N = 2) ... 2.3e-7 (N = 10000), fp64 3.7e-16 ... 5.4e-16 (N = 3000).

No case is skipped: a commit that answers unsupported_configuration inside the supported set fails the test."""
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers as H

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS = {"f32": [2, 16, 64, 256, 512, 2048, 4096, 8192, 1000, 1920, 6000, 10000],
           "f64": [16, 64, 512, 2048, 4096, 1000, 3000]}
CASES = [(p, n) for p in ("f32", "f64") for n in LENGTHS[p]]


def _mods():
    import gpu_utils as G
    import portfft_amd as pf
    return G, pf, G.torch_mod()


def _ct(prec):
    return np.complex64 if prec == "f32" else np.complex128


def _desc(pf, n, prec, batch=1, in_place=False, distances=None, offsets=(0, 0), scales=(1.0, 1.0)):
    d = pf.convolution_descriptor([n], prec)
    d.number_of_transforms = batch
    d.forward_scale, d.backward_scale = scales
    d.forward_offset, d.backward_offset = offsets
    if distances is not None:
        d.forward_distance, d.backward_distance = distances
    if in_place:
        d.placement = pf.placement.IN_PLACE
    return d


def _data(rng, batch, n, ct):
    return (rng.uniform(-1, 1, (batch, n)) + 1j * rng.uniform(-1, 1, (batch, n))).astype(ct)


def _reference(d, x, h, correlate):
    """NumPy in double: fs * bs * N * ifft(fft(x) * H[t % F]), conj(H) for correlate"""
    n = x.shape[1]
    hh = h.astype(np.complex128)[np.arange(x.shape[0]) % h.shape[0]]
    if correlate:
        hh = np.conj(hh)
    return d.forward_scale * d.backward_scale * n * np.fft.ifft(np.fft.fft(x.astype(np.complex128), axis=1) * hh, axis=1)


def _check(got, ref, ct, n, what):
    got = np.asarray(got).astype(np.complex128)
    ref = np.asarray(ref).astype(np.complex128)
    err = np.linalg.norm(got - ref, axis=1) / np.maximum(np.linalg.norm(ref, axis=1), 1e-300)
    print("%s: worst rel-L2 %.3e (transform %d)" % (what, float(err.max()), int(np.argmax(err))))
    assert np.all(err <= H.REL_L2_TOL[np.dtype(ct)]), (what, "transform", int(np.argmax(err)), float(err.max()))
    assert H.check_reference_rule(got, ref.astype(ct), n), (what, "per-element reference rule")


class _verb:
    """the plan as gpu_utils.execute drives it: its forward execute is the fused verb (input: the forward domain,
    output: the backward domain, as compute_forward)"""

    def __init__(self, plan, correlate):
        self.wait = plan.wait
        self.compute_forward = plan.correlate if correlate else plan.convolve


def _run(G, pf, torch, d, x, h, plan, correlate, what, guard=None):
    """one verb of `plan` (committed from d, filter h set) on the packed rows x through d's layout, every row checked"""
    guard = G.GUARD if guard is None else guard
    y, bits = G.transform_packed(d, pf.direction.FORWARD, x, _verb(plan, correlate), guard)
    _check(y, _reference(d, x, h, correlate), x.dtype.type, x.shape[1], what + ("corr" if correlate else "conv",))
    return bits


def _commit(pf, torch, d, h):
    plan = d.commit()
    plan.set_filter(torch.from_numpy(h).cuda())
    return plan


def _fpw(pf, n, prec):
    info = _desc(pf, n, prec).commit().info()
    dim = info.dims[0]
    assert dim.length == n and dim.tier in (0, 1) and tuple(info.launches) == (1, 1)  # (a single pass: the register tier)
    assert int(np.prod(dim.factors[:dim.n_factors])) == n
    return max(1, dim.ffts_per_workgroup), dim


@pytest.mark.parametrize("prec,n", CASES)
def test_convolve_and_correlate_against_numpy(prec, n):
    G, pf, torch = _mods()
    ct = _ct(prec)
    fpw, dim = _fpw(pf, n, prec)
    print("N=%d %s: factors %s fpw %d lds %d" % (n, prec, list(dim.factors[:dim.n_factors]), fpw, dim.lds_bytes))
    rng = np.random.Generator(np.random.SFC64(n))
    for batch in sorted({1, 3, 2 * fpw - 1, 2 * fpw + 1}):
        x = _data(rng, batch, n, ct)
        for nf in sorted({1, 3, batch}):
            h = _data(rng, nf, n, ct)
            for in_place in (False, True):
                d = _desc(pf, n, prec, batch, in_place)
                plan = _commit(pf, torch, d, h)
                for correlate in (False, True):
                    _run(G, pf, torch, d, x, h, plan, correlate, (prec, n, batch, nf, "ip" if in_place else "oop"))
        if batch in (3, 2 * fpw + 1):
            scales = (0.5, 0.25 / n)
            h = _data(rng, 3, n, ct)
            # padded rows on one side, packed rows on the other, different offsets; base one element off 128 bytes
            for dist, off, ip, guard, name in (((n + 5, n), (5, 2), False, (65, 63), "oop padded input"),
                                               ((n, n + 5), (0, 3), False, None, "oop padded output"),
                                               ((n + 5, n + 5), (3, 3), True, (63, 65), "ip padded")):
                d = _desc(pf, n, prec, batch, ip, dist, off, scales)
                plan = _commit(pf, torch, d, h)
                for correlate in (False, True):
                    _run(G, pf, torch, d, x, h, plan, correlate, (prec, n, batch, name), guard)


@pytest.mark.parametrize("prec,n", CASES)
def test_many_trips_of_the_persistent_loop(prec, n):
    G, pf, torch = _mods()
    ct = _ct(prec)
    fpw, _ = _fpw(pf, n, prec)
    batch = 4000 * fpw + 1
    rng = np.random.Generator(np.random.SFC64(3 * n + 1))
    x = _data(rng, batch, n, ct)
    h = _data(rng, 3, n, ct)
    d = _desc(pf, n, prec, batch)
    _run(G, pf, torch, d, x, h, _commit(pf, torch, d, h), False, (prec, n, batch, 3, "oop"))


@pytest.mark.parametrize("prec,n", [("f32", 1000), ("f32", 4096)])
def test_the_bit_is_a_permission(prec, n):
    G, pf, torch = _mods()
    ct = _ct(prec)
    batch = 7
    x = _data(np.random.Generator(np.random.SFC64(n)), batch, n, ct)
    plain = G.make_descriptor([n], prec, batch=batch)
    withbit = _desc(pf, n, prec, batch)
    pi, wi = plain.commit().info(), withbit.commit().info()
    assert bytes(pi) == bytes(wi), "the plan info of a descriptor with PFFT_EXT_CONVOLUTION is the plain one's"
    for direction in (pf.direction.FORWARD, pf.direction.BACKWARD):
        _, a = G.transform_packed(plain, direction, x)
        _, b = G.transform_packed(withbit, direction, x)
        H.check_unchanged(a, b, what="length %d with PFFT_EXT_CONVOLUTION" % n)
    # the spectrum made with the same plan: the three steps composed are what the fused verb computes
    hplan = _desc(pf, n, prec, 1).commit()
    g = _data(np.random.Generator(np.random.SFC64(5)), 1, n, ct)
    hd = torch.empty(n, dtype=torch.from_numpy(g).dtype, device="cuda")
    hplan.compute_forward(torch.from_numpy(g.ravel()).cuda(), hd).wait()
    plan = withbit.commit()
    plan.set_filter(hd)
    _run(G, pf, torch, withbit, x, hd.cpu().numpy().reshape(1, n), plan, False, (prec, n, "spectrum by the same plan"))


@pytest.mark.parametrize("prec,n", [("f32", 512), ("f64", 1000)])
def test_filter_lifetime(prec, n):
    G, pf, torch = _mods()
    ct = _ct(prec)
    batch = 9
    rng = np.random.Generator(np.random.SFC64(11 * n))
    x = _data(rng, batch, n, ct)
    h1, h2, h3 = _data(rng, 3, n, ct), _data(rng, batch, n, ct), _data(rng, 1, n, ct)
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
    plan.set_filter(torch.from_numpy(h3.ravel()).cuda())  # shape (N,): one shared filter, for later executes
    _run(G, pf, torch, d, x, h3, plan, False, (prec, n, "second set_filter"))
    _run(G, pf, torch, d, x, h2, clone, False, (prec, n, "clone after the original's set_filter"))


def test_verbs_and_filters_that_are_invalid():
    G, pf, torch = _mods()
    n, batch = 256, 4
    d = _desc(pf, n, "f32", batch)
    plan = d.commit()
    x = torch.zeros(batch * n, dtype=torch.complex64, device="cuda")
    y = torch.empty_like(x)
    for verb in (plan.convolve, plan.correlate):
        with pytest.raises(pf.invalid_configuration, match="no filter"):
            verb(x, y)
        with pytest.raises(pf.invalid_configuration, match="no filter"):
            verb(x)
    good = torch.ones(2, n, dtype=torch.complex64, device="cuda")
    for bad in (good.to(torch.complex128), good.real.contiguous(), torch.ones(2, n + 1, dtype=torch.complex64, device="cuda"),
                torch.ones(n - 1, dtype=torch.complex64, device="cuda"), torch.ones(0, n, dtype=torch.complex64, device="cuda"),
                good.cpu(), torch.ones(2, 2 * n, dtype=torch.complex64, device="cuda")[:, ::2], good.cpu().numpy()):
        with pytest.raises(pf.invalid_configuration):
            plan.set_filter(bad)
    with pytest.raises(pf.invalid_configuration, match="no filter"):
        plan.convolve(x, y)  # none of them became the filter
    plan.set_filter(good)
    for bad in (x[:-1], x.to(torch.complex128), x.cpu()):
        with pytest.raises(pf.invalid_configuration):
            plan.convolve(bad, y)
        with pytest.raises(pf.invalid_configuration):
            plan.convolve(x, bad)
    with pytest.raises(pf.invalid_configuration):
        plan.convolve(x, y, y)
    plan.convolve(x, y).wait()
    assert float(y.abs().max()) == 0.0
    # a plain plan has no such verbs
    plain = G.make_descriptor([n], "f32", batch=batch).commit()
    with pytest.raises(pf.invalid_configuration):
        plain.set_filter(good)
    with pytest.raises(pf.invalid_configuration):
        plain.convolve(x, y)


@pytest.mark.parametrize("prec,n", [("f32", 2048), ("f64", 1000)])
def test_dependencies_and_events(prec, n):
    G, pf, torch = _mods()
    ct = _ct(prec)
    batch = 5
    rng = np.random.Generator(np.random.SFC64(7 * n))
    x, h = _data(rng, batch, n, ct), _data(rng, 2, n, ct)
    d = _desc(pf, n, prec, batch)
    plan = _commit(pf, torch, d, h)
    bits = _run(G, pf, torch, d, x, h, plan, False, (prec, n, "plain call"))
    seen = {}

    class with_events:
        wait = staticmethod(plan.wait)

        @staticmethod
        def compute_forward(*bufs):
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

    _, ebits = G.transform_packed(d, pf.direction.FORWARD, x, with_events)
    H.check_unchanged(bits, ebits, what="convolve with a dependency and a returned event")
    H.check_unchanged(bits, seen["bits"][:bits.size], what="the output behind the returned event")
    y = torch.empty(batch * n, dtype=torch.from_numpy(x).dtype, device="cuda")
    ev = plan.correlate(torch.from_numpy(x.ravel()).cuda(), y, want_event=False)
    assert not ev.native
    ev.wait()
    _check(y.cpu().numpy().reshape(batch, n), _reference(d, x, h, True), ct, n, (prec, n, "want_event=False"))


@pytest.mark.parametrize("prec,n,reason", [("f32", 16384, "register-resident"), ("f32", 1 << 20, "four-step"),
                                           ("f32", 67 * 8, "prime factor above 61"),
                                           ("f64", 8192, "register-resident")])
def test_refusals_at_commit_name_the_cause(prec, n, reason):
    G, pf, torch = _mods()
    d = _desc(pf, n, prec, 2)
    d.validate()
    with pytest.raises(pf.unsupported_configuration) as e:
        d.commit()
    assert reason in str(e.value) and "fused convolution" in str(e.value), str(e.value)


def test_row_pitch_beyond_the_32_bit_range_is_refused():
    G, pf, torch = _mods()
    d = _desc(pf, 4096, "f32", 1, distances=(1 << 30, 4096))
    with pytest.raises(pf.unsupported_configuration, match="32-bit range"):
        d.commit()


def test_without_runtime_specialisation():
    """PFFT_JIT=0 (fresh child process): the registered N = 4096 convolves, an unregistered length is refused at commit"""
    code = (
        "import numpy as np, torch, portfft_amd as pf\n"
        "d = pf.convolution_descriptor([4096], 'f32')\n"
        "p = d.commit()\n"
        "p.set_filter(torch.ones(4096, dtype=torch.complex64, device='cuda'))\n"
        "x = torch.zeros(4096, dtype=torch.complex64, device='cuda'); x[1] = 1\n"
        "y = torch.empty_like(x)\n"
        "p.convolve(x, y).wait()\n"
        "assert abs(complex(y[1]) - 4096) < 1e-2 and float(y.abs().sum()) < 4096.5, y[:4]\n"
        "try:\n"
        "    pf.convolution_descriptor([1000], 'f32').commit()\n"
        "    raise SystemExit('1000 committed without the runtime compiler')\n"
        "except pf.unsupported_configuration as e:\n"
        "    assert 'PFFT_JIT=0' in str(e) and 'fused convolution' in str(e), e\n"
        "print('jit0 OK')\n")
    env = dict(os.environ, PFFT_JIT="0", PYTHONPATH=ROOT)
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "jit0 OK" in p.stdout
