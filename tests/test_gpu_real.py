"""Real transforms on the GPU (pf.real_descriptor: stockham_wg_r2c_kernel / stockham_wg_c2r_kernel): every transform of
every case against NumPy in double precision -- forward np.fft.rfft, backward N * np.fft.irfft -- with the project's two
yardsticks (per-transform relative L2 within helpers.REL_L2_TOL, helpers.check_reference_rule with n = N), the exactly
real bins 0 and N/2, the ignored imaginary parts of those bins on the way back, and the write sets: every scalar in
front of the offset, between and behind the rows keeps the padding bit pattern, out of place and in place.

In place, row t of the one buffer holds N scalars (forward domain) in N/2 + 1 complex slots (backward domain).  After a
backward transform the two pad scalars at the end of each row may hold anything; nothing else outside the rows changes.

The lengths below are one per kernel shape; every registered line of the kernels runs in test_gpu_fused_registry.py.

No case is skipped: a commit that answers unsupported_configuration inside the supported set fails the test."""
import numpy as np
import pytest

import helpers as H

pytestmark = pytest.mark.gpu

GUARD = 64  # scalars / complex elements in front of and behind every buffer
# pre-compiled powers of two, lengths only hiprtc serves (6, 30, 1000 -> M = 3, 15, 500), a prime factor 37 in M (592),
# the longest LDS-resident length per precision and one hiprtc length near it
LENGTHS = {"f32": [4, 6, 8, 16, 30, 64, 256, 592, 1000, 1024, 4096, 8192, 16384, 20000],
           "f64": [4, 6, 8, 16, 30, 64, 256, 592, 1000, 1024, 4096, 6000, 8192]}
CASES = [(p, n) for p in ("f32", "f64") for n in LENGTHS[p]]


def _mods():
    import gpu_utils as G
    import portfft_amd as pf
    return G, pf, G.torch_mod()


def _types(prec):
    return (np.float32, np.complex64) if prec == "f32" else (np.float64, np.complex128)


def _desc(pf, n, prec, batch, in_place, offsets, scales):
    d = pf.real_descriptor(n, prec)
    d.number_of_transforms = batch
    d.forward_scale, d.backward_scale = scales
    d.forward_offset, d.backward_offset = offsets
    if in_place:
        d.placement = pf.placement.IN_PLACE
        d.forward_distance = 2 * d.backward_distance
    return d


def _rows(offset, dist, batch, width):
    return (offset + np.arange(batch)[:, None] * dist + np.arange(width)[None, :]).astype(np.int64)


def _alloc(torch, count, np_dtype):
    t = torch.full((GUARD + count + GUARD,), H.PADDING_VALUE, dtype=torch.from_numpy(np.zeros(0, np_dtype)).dtype, device="cuda")
    return t, t[GUARD:GUARD + count]


def _execute(pf, torch, d, plan, direction, packed, call=None):
    """packed [batch, N] reals (forward) or [batch, N/2 + 1] bins (backward) through the descriptor's layout.  Checks the
    guards, the input of an out-of-place execute and the write set; returns the packed output and the raw output
    scalars (bits)."""
    rt, ct = _types(d.scalar)
    n, batch = d.lengths[0], d.number_of_transforms
    bins = n // 2 + 1
    fwd = direction == pf.direction.FORWARD
    in_place = d.placement == pf.placement.IN_PLACE
    fo, fd, bo, bd = d.forward_offset, d.forward_distance, d.backward_offset, d.backward_distance
    n_real, n_cplx = d.get_input_count(pf.direction.FORWARD), d.get_output_count(pf.direction.FORWARD)
    ridx, cidx = _rows(fo, fd, batch, n), _rows(bo, bd, batch, bins)
    fn = call or (plan.compute_forward if fwd else plan.compute_backward)
    if in_place:
        count = max(n_real, 2 * n_cplx)  # scalars
        alloc, buf = _alloc(torch, count, rt)
        host = np.full(count, H.PADDING_VALUE, rt)
        if fwd:
            host[ridx.ravel()] = packed.astype(rt).ravel()
        else:
            host.view(ct)[cidx.ravel()] = packed.astype(ct).ravel()
        buf.copy_(torch.from_numpy(host))
        fn(buf)
        plan.wait()
        res = alloc.cpu().numpy()
        H.check_guards(res, GUARD, count, what="in place")
        out = res[GUARD:GUARD + count]
        # the row slots: 2 * bins scalars from 2 * bo + t * 2 * bd; everything else keeps the padding
        H.check_write_set(out, _rows(2 * bo, 2 * bd, batch, 2 * bins), what="in place buffer")
        if fwd:
            return out.view(ct)[cidx], out
        # backward: the pad scalars of each row may hold anything; return the rows only
        return out[ridx], out[ridx]
    in_count, out_count = (n_real, n_cplx) if fwd else (n_cplx, n_real)
    it, ot = (rt, ct) if fwd else (ct, rt)
    ialloc, ibuf = _alloc(torch, in_count, it)
    oalloc, obuf = _alloc(torch, out_count, ot)
    host = np.full(in_count, H.PADDING_VALUE, it)
    host[(ridx if fwd else cidx).ravel()] = packed.astype(it).ravel()
    ibuf.copy_(torch.from_numpy(host))
    fn(ibuf, obuf)
    plan.wait()
    ires, ores = ialloc.cpu().numpy(), oalloc.cpu().numpy()
    H.check_guards(ires, GUARD, in_count, what="out of place input")
    H.check_unchanged(host, ires[GUARD:GUARD + in_count], what="the input of an out-of-place execute")
    H.check_guards(ores, GUARD, out_count, what="out of place output")
    out = ores[GUARD:GUARD + out_count]
    H.check_write_set(out, cidx if fwd else ridx, what="output buffer")
    return out[cidx if fwd else ridx], out


def _check(got, ref, ct, n, what):
    got = np.asarray(got).astype(np.complex128)
    ref = np.asarray(ref).astype(np.complex128)
    err = np.linalg.norm(got - ref, axis=1) / np.maximum(np.linalg.norm(ref, axis=1), 1e-300)
    print("%s: worst rel-L2 %.3e (transform %d)" % (what, float(err.max()), int(np.argmax(err))))
    assert np.all(err <= H.REL_L2_TOL[np.dtype(ct)]), (what, "transform", int(np.argmax(err)), float(err.max()))
    assert H.check_reference_rule(got, ref.astype(ct), n), (what, "per-element reference rule")


@pytest.mark.parametrize("prec,n", CASES)
def test_real_transforms_against_numpy(prec, n):
    G, pf, torch = _mods()
    rt, ct = _types(prec)
    m = n // 2
    info = _desc(pf, n, prec, 1, False, (0, 0), (1.0, 1.0)).commit().info()
    assert info.dims[0].length == n and info.dims[0].tier == 1 and tuple(info.launches) == (1, 1)
    assert int(np.prod(info.dims[0].factors[:info.dims[0].n_factors])) == m
    fpw = max(1, info.dims[0].ffts_per_workgroup)
    rng = np.random.Generator(np.random.SFC64(n))
    for batch in sorted({1, 3, 33, fpw + 1}):
        x = rng.uniform(-1, 1, (batch, n)).astype(rt)
        X = np.fft.rfft(x.astype(np.float64), axis=1)
        Xin = X.astype(ct)
        Xclean = Xin.astype(np.complex128)
        Xclean[:, 0] = Xclean[:, 0].real
        Xclean[:, m] = Xclean[:, m].real
        xback = n * np.fft.irfft(Xclean, n, axis=1)
        for in_place in (False, True):
            variants = [((0, 0), (1.0, 1.0))]
            if batch in (3, 33):
                variants.append(((6, 3) if in_place else (5, 2), (0.5, 1.0 / n)))
            for offsets, scales in variants:
                what = (prec, n, batch, "ip" if in_place else "oop", offsets)
                d = _desc(pf, n, prec, batch, in_place, offsets, scales)
                plan = d.commit()
                y, _ = _execute(pf, torch, d, plan, pf.direction.FORWARD, x)
                _check(y, scales[0] * X, ct, n, what + ("fwd",))
                assert np.all(y[:, 0].imag == 0) and np.all(y[:, m].imag == 0), (what, "bins 0 and N/2 must be real")
                back, bits = _execute(pf, torch, d, plan, pf.direction.BACKWARD, Xin)
                _check(back, scales[1] * xback, ct, n, what + ("bwd",))
                # garbage in the imaginary parts of bins 0 and N/2: the same output, bit for bit
                Xg = Xin.copy()
                Xg[:, 0] = Xg[:, 0].real + 1j * 123.25
                Xg[:, m] = Xg[:, m].real - 1j * 7.5
                _, bits_g = _execute(pf, torch, d, plan, pf.direction.BACKWARD, Xg)
                H.check_unchanged(bits, bits_g, what="backward with garbage in Im X[0], Im X[N/2]")


@pytest.mark.parametrize("prec,n", [("f32", 1024), ("f32", 1000), ("f64", 4096), ("f32", 16384)])
def test_round_trip_clone_and_events(prec, n):
    G, pf, torch = _mods()
    rt, ct = _types(prec)
    batch = 5
    x = np.random.Generator(np.random.SFC64(7 * n)).uniform(-1, 1, (batch, n)).astype(rt)
    d = _desc(pf, n, prec, batch, False, (0, 0), (1.0, 1.0))
    plan = d.commit()
    y, ybits = _execute(pf, torch, d, plan, pf.direction.FORWARD, x)
    back, _ = _execute(pf, torch, d, plan, pf.direction.BACKWARD, y)
    _check(back, n * x.astype(np.float64), ct, n, (prec, n, "round trip"))
    # a cloned plan and the dependency / event path give the same bits as the plain call
    clone = plan.copy()
    _, cbits = _execute(pf, torch, d, clone, pf.direction.FORWARD, x)
    H.check_unchanged(ybits, cbits, what="cloned plan")
    seen = {}

    def with_events(*bufs):
        dep = torch.cuda.Event()
        dep.record(torch.cuda.current_stream())
        ev = plan.compute_forward(*bufs, dependencies=[dep])
        assert ev.native
        ev.wait()
        assert ev.is_complete()
        seen["event"] = True

    _, ebits = _execute(pf, torch, d, plan, pf.direction.FORWARD, x, call=with_events)
    H.check_unchanged(ybits, ebits, what="execute with a dependency and a returned event")
    assert seen["event"]


def test_split_entry_point_refuses_a_real_plan():
    import ctypes as C
    G, pf, torch = _mods()
    from portfft_amd import _lib
    plan = pf.real_descriptor(64).commit()
    t = torch.zeros(128, device="cuda")
    p = C.c_void_p(t.data_ptr())
    assert _lib.lib.pfft_execute_split(plan._plan, 0, p, p, p, p) == 1  # PFFT_INVALID_CONFIGURATION


def test_lengths_outside_the_supported_set_are_refused_at_commit():
    G, pf, torch = _mods()
    with pytest.raises(pf.unsupported_configuration) as e:
        pf.real_descriptor(32768, "f32").commit()  # M = 16384 runs on the register-resident kernel
    assert "register-resident" in str(e.value)
    with pytest.raises(pf.unsupported_configuration) as e:
        pf.real_descriptor(16384, "f64").commit()  # fp64 M = 8192 likewise
    assert "register-resident" in str(e.value)
    with pytest.raises(pf.unsupported_configuration):
        pf.real_descriptor(2 * 67 * 8, "f32").commit()  # a prime factor above 61 in M
    with pytest.raises(pf.unsupported_configuration):
        pf.real_descriptor(1 << 20, "f32").commit()  # M on the four-step tier
