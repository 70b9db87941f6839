"""Fused inverse MDCT (set_imdct_window / imdct of a plan of the REAL domain) on the GPU against NumPy in double
(imdct_ref.py: the bins 2n + 1 + N of a zero-stuffed FFT of 8N points, frames added in ascending f; it knows neither the
unfold nor the twiddles the kernel uses).

The lengths of test_gpu_dct4.py, one per kernel shape (every registered line runs in test_gpu_imdct_registry.py): fp32
N = 4, 8, 32, 64, 128, 512, 1024, 4096, 16384 pre-compiled, 30 (odd M: a middle item), 2000 and 12000 through the runtime
compiler; fp64 N = 128, 1024, 8192 and 6000.

Per length: three signals with lead N (the default), a random non-symmetric window and an out_length that is no multiple
of N and shorter than the frames cover; lead 0 without a window over the full coverage (F + 1) N; lead 2N - 1, the first
frame contributing one sample; one signal of 2 FPW + 1 frames with lead 1 (a ragged last step); lead N - 2; every third
scenario on the scaled plan.  Odd pitches of the frames, the signals' coefficients and the output rows in guarded
buffers.  Every signal: relative L2 within helpers.REL_L2_TOL and helpers.check_reference_rule(n=N); the write set; the
guards; the input unchanged.  Every geometry runs with chunk_frames 0, 1, 2 FPW + 1 and n_frames + 3, and the four whole
guarded output allocations hold the same bits.

The round trip imdct(mdct(x)) with the sine window on both sides, lead N, ceil(L / N) + 1 frames and backward_scale
1 / (2N) against x within 2 REL_L2_TOL (the bound of the dct4 and istft round trips), at every length.

mdct, dct4 and R2C of a plan are bit-identical before and after set_imdct_window; a copy shares the window until either
side sets another.

Worst relative L2 per length (MI355X; every scenario; the tests print them): see DESIGN.md 3.1n.

No case is skipped."""
import numpy as np
import pytest

import helpers as H
from imdct_ref import imdct_reference

pytestmark = pytest.mark.gpu

LENGTHS = {"f32": [4, 8, 32, 64, 128, 512, 1024, 4096, 16384, 30, 2000, 12000], "f64": [128, 1024, 8192, 6000]}
CASES = [(p, n) for p in ("f32", "f64") for n in LENGTHS[p]]
SCALES = (0.5, 0.25)  # forward_scale, backward_scale of the scaled plan


def _mods():
    import gpu_utils as G
    import portfft_amd as pf
    return G, pf, G.torch_mod()


def _types(prec):
    return (np.float32, np.complex64) if prec == "f32" else (np.float64, np.complex128)


_plans = {}


def _plan(pf, n, prec, kind="plain"):
    """(plan, backward_scale, fpw) of a length: committed once per process; kind: plain, scaled (SCALES) or trip
    (backward_scale 1 / (2N))"""
    key = (n, prec, kind)
    if key not in _plans:
        d = pf.real_descriptor(n, prec)
        if kind == "scaled":
            d.forward_scale, d.backward_scale = SCALES
        elif kind == "trip":
            d.backward_scale = 1.0 / (2 * n)
        plan = d.commit()
        plan.set_imdct_window(None)
        _plans[key] = (plan, d.backward_scale, max(1, plan.info().dims[0].ffts_per_workgroup))
    return _plans[key]


_worst = {}


def _check(got, ref, ct, n, what, tol_factor=1.0):
    g = np.asarray(got).astype(np.float64)
    r = np.asarray(ref).astype(np.float64)
    err = np.linalg.norm(g - r, axis=1) / np.maximum(np.linalg.norm(r, axis=1), 1e-300)
    key = (np.dtype(ct).name, n)
    _worst[key] = max(_worst.get(key, 0.0), float(err.max()))
    print("%s: worst rel-L2 %.3e (signal %d)" % (what, float(err.max()), int(np.argmax(err))))
    assert np.all(err <= tol_factor * H.REL_L2_TOL[np.dtype(ct)]), (what, "signal", int(np.argmax(err)), float(err.max()))
    if tol_factor == 1.0:
        assert H.check_reference_rule(g, r.astype(ct), n), (what, "per-element reference rule")


def _odd(v):
    return v | 1


def _imdct(G, torch, plan, coeff, n, lead, length, chunk, what, lead_arg="given", gin=None):
    """plan.imdct of the coefficients coeff (numpy, (S, F, N)) into a guarded buffer with an odd pitch: the guards, the
    write set, the input unchanged.  Returns (samples (S, L), the whole output allocation, the guarded input)."""
    n_sig, n_frames, _ = coeff.shape
    tt = torch.from_numpy(coeff[:0]).dtype
    frame_pitch = _odd(n + 3)
    in_pitch = _odd(n_frames * frame_pitch + 5)
    out_pitch = _odd(length + 3)
    if gin is None:
        gin = G.Guarded(n_sig * in_pitch, tt)
        gin.buf.as_strided((n_sig, n_frames, n), (in_pitch, frame_pitch, 1)).copy_(torch.from_numpy(coeff))
    gout = G.Guarded(n_sig * out_pitch, tt)
    before = gin.buf.cpu().numpy()
    yv = gin.buf.as_strided((n_sig, n_frames, n), (in_pitch, frame_pitch, 1))
    xv = gout.buf.view(n_sig, out_pitch)[:, :length]
    if n_sig == 1:  # (a single signal comes as a 2-D input and a 1-D output)
        yv, xv = yv[0], xv[0]
    if lead_arg == "default":
        plan.imdct(yv, xv, chunk_frames=chunk)
    else:
        plan.imdct(yv, xv, lead=lead, chunk_frames=chunk)
    plan.wait()
    gin.check(str(what) + ": input")
    gout.check(str(what) + ": output")
    H.check_unchanged(before, gin.buf.cpu().numpy(), what=str(what) + ": the input")
    raw = gout.buf.cpu().numpy()
    idx = (np.arange(n_sig)[:, None] * out_pitch + np.arange(length)[None, :]).ravel()
    H.check_write_set(raw, idx, what=str(what) + ": output buffer")
    return raw[idx].reshape(n_sig, length), gout.alloc, gin


def _scenarios(n, fpw):
    """(signals, frames, lead, out_length, windowed, how lead is passed)"""
    return [
        (3, 4, n, 3 * n + n // 2 + 1, True, "default"),               # lead N; shorter than the 4N the frames cover
        (3, 3, 0, 4 * n, False, "given"),                             # no window; the full coverage (F + 1) N
        (3, 4, 2 * n - 1, 2 * n + 3, True, "given"),                  # the first frame contributes its last sample alone
        (1, 2 * fpw + 1, 1, (2 * fpw + 2) * n - 1, True, "given"),    # 2 FPW + 1 frames: a ragged last step
        (3, 3, n - 2, 3 * n + 1, True, "given"),                      # even lead
    ]


@pytest.mark.parametrize("prec,n", CASES)
def test_imdct_against_numpy_and_across_chunks(prec, n):
    G, pf, torch = _mods()
    rt, ct = _types(prec)
    rng = np.random.default_rng(n * 17 + (prec == "f64"))
    fpw = _plan(pf, n, prec)[2]
    for i, (n_sig, n_frames, lead, length, windowed, lead_arg) in enumerate(_scenarios(n, fpw)):
        plan, bs, _ = _plan(pf, n, prec, "scaled" if i % 3 == 2 else "plain")
        coeff = rng.uniform(-1, 1, (n_sig, n_frames, n)).astype(rt)
        w = rng.uniform(0.25, 1.0, 2 * n).astype(rt) if windowed else None  # (not symmetric)
        plan.set_imdct_window(None if w is None else torch.from_numpy(w).cuda())
        what = "%s N=%d imdct S=%d F=%d lead=%d L=%d%s%s" % (prec, n, n_sig, n_frames, lead, length,
                                                             " windowed" if windowed else "", " scaled" if i % 3 == 2 else "")
        ref = bs * imdct_reference(coeff, w, n, lead, length)
        first, gin = None, None
        for chunk in (0, 1, 2 * fpw + 1, n_frames + 3):
            got, alloc, gin = _imdct(G, torch, plan, coeff, n, lead, length, chunk, "%s chunk=%d" % (what, chunk), lead_arg, gin)
            if first is None:
                first = alloc
                _check(got, ref, ct, n, what)
            else:
                H.check_same_bits(first, alloc, what=what + ": chunk_frames %d against 0" % chunk)
    print("worst rel-L2 imdct %s N=%d: %.3e" % (prec, n, _worst[(np.dtype(ct).name, n)]))


@pytest.mark.parametrize("prec,n", CASES)
def test_imdct_of_mdct_reconstructs_the_signal(prec, n):
    """sine window on both sides, lead N, ceil(L / N) + 1 frames, forward_scale 1, backward_scale 1 / (2N)"""
    G, pf, torch = _mods()
    rt, ct = _types(prec)
    plan = _plan(pf, n, prec, "trip")[0]
    rng = np.random.default_rng(n * 19 + (prec == "f64"))
    n_sig, length = 2, 3 * n + n // 2 + 1
    n_frames = -(-length // n) + 1
    x = rng.uniform(-1, 1, (n_sig, length)).astype(rt)
    w = torch.from_numpy(np.sin(np.pi * (np.arange(2 * n) + 0.5) / (2 * n)).astype(rt)).cuda()
    plan.set_mdct_window(w)
    plan.set_imdct_window(w)
    xd = torch.from_numpy(x).cuda()
    coeff = torch.empty(n_sig, n_frames, n, dtype=xd.dtype, device="cuda")
    back = torch.full((n_sig, length), H.PADDING_VALUE, dtype=xd.dtype, device="cuda")
    plan.mdct(xd, coeff)
    plan.imdct(coeff, back)
    plan.wait()
    _check(back.cpu().numpy(), x, ct, n, "%s N=%d imdct(mdct(x))" % (prec, n), tol_factor=2.0)


@pytest.mark.parametrize("prec,n", [("f32", 512), ("f32", 2000), ("f64", 1024)])
def test_set_imdct_window_leaves_the_other_verbs_bit_stable(prec, n):
    """mdct, dct4 and R2C of a plan are what they were before the first set_imdct_window"""
    G, pf, torch = _mods()
    rt, ct = _types(prec)
    rng = np.random.default_rng(n)
    rows = 5
    d = pf.real_descriptor(n, prec)
    d.number_of_transforms = rows
    plan = d.commit()
    x = torch.from_numpy(rng.uniform(-1, 1, (rows, n)).astype(rt)).cuda()
    sig = torch.from_numpy(rng.uniform(-1, 1, (2, 3 * n + 5)).astype(rt)).cuda()
    w = torch.from_numpy(rng.uniform(0.25, 1.0, 2 * n).astype(rt)).cuda()
    ctt = torch.from_numpy(np.zeros(0, dtype=ct)).dtype
    plan.set_mdct_window(w)
    outs = []
    for step in range(2):
        bins = torch.empty(rows, n // 2 + 1, dtype=ctt, device="cuda")
        y = torch.empty_like(x)
        coeff = torch.empty(2, 4, n, dtype=x.dtype, device="cuda")
        plan.compute_forward(x.reshape(-1), bins.reshape(-1))
        plan.dct4(x, y)
        plan.mdct(sig, coeff)
        plan.wait()
        outs.append((bins, y, coeff))
        if step == 0:
            plan.set_imdct_window(w)
            back = torch.empty(2, 3 * n, dtype=x.dtype, device="cuda")
            plan.imdct(coeff, back)
            plan.wait()
    for name, a, b in zip(("R2C", "dct4", "mdct"), outs[0], outs[1]):
        H.check_same_bits(torch.view_as_real(a).reshape(-1) if a.is_complex() else a.reshape(-1),
                          torch.view_as_real(b).reshape(-1) if b.is_complex() else b.reshape(-1),
                          what=name + " before and after set_imdct_window")


def test_a_copy_shares_the_window_until_either_side_sets_another():
    G, pf, torch = _mods()
    n, n_sig, n_frames = 64, 2, 4
    length = (n_frames + 1) * n - n
    rng = np.random.default_rng(7)
    coeff_h = rng.uniform(-1, 1, (n_sig, n_frames, n)).astype(np.float32)
    coeff = torch.from_numpy(coeff_h).cuda()
    ws = [rng.uniform(0.25, 1.0, 2 * n).astype(np.float32) for _ in range(3)]

    def run(p):
        out = torch.empty(n_sig, length, device="cuda")
        p.imdct(coeff, out)
        p.wait()
        return out

    plan = pf.real_descriptor(n).commit()
    plan.set_imdct_window(torch.from_numpy(ws[0]).cuda())
    copy = plan.copy()
    a, b = run(plan), run(copy)
    H.check_same_bits(a.reshape(-1), b.reshape(-1), what="a copy runs with the plan's window")
    _check(b.cpu().numpy(), imdct_reference(coeff_h, ws[0], n, n, length), np.complex64, n, "copy, shared window")
    copy.set_imdct_window(torch.from_numpy(ws[1]).cuda())
    H.check_same_bits(a.reshape(-1), run(plan).reshape(-1), what="the plan keeps its window when the copy sets another")
    _check(run(copy).cpu().numpy(), imdct_reference(coeff_h, ws[1], n, n, length), np.complex64, n, "copy, own window")
    c = run(copy)
    plan.set_imdct_window(torch.from_numpy(ws[2]).cuda())
    H.check_same_bits(c.reshape(-1), run(copy).reshape(-1), what="the copy keeps its window when the plan sets another")
    _check(run(plan).cpu().numpy(), imdct_reference(coeff_h, ws[2], n, n, length), np.complex64, n, "plan, third window")


def test_the_verbs_need_a_window_and_a_real_plan():
    G, pf, torch = _mods()
    n = 64
    plan = pf.real_descriptor(n).commit()
    coeff = torch.zeros(3, n, device="cuda")
    out = torch.empty(3 * n, device="cuda")
    with pytest.raises(pf.invalid_configuration, match="pfft_plan_set_imdct_window"):
        plan.imdct(coeff, out)
    with pytest.raises(pf.invalid_configuration, match="pfft_plan_set_imdct_window"):
        plan.imdct_chunk_frames(2, 8)
    plan.set_mdct_window(None)
    with pytest.raises(pf.invalid_configuration, match="pfft_plan_set_imdct_window"):  # (the analysis window is another)
        plan.imdct(coeff, out)
    cplx = pf.descriptor([n]).commit()
    for call in (lambda: cplx.set_imdct_window(None), lambda: cplx.imdct(coeff, out), lambda: cplx.imdct_chunk_frames(2, 8)):
        with pytest.raises(pf.invalid_configuration, match="not of the REAL domain"):
            call()
    plan.set_imdct_window(None)
    assert 1 <= plan.imdct_chunk_frames(2, 8) <= 8
    both = torch.zeros(4 * n, device="cuda")
    with pytest.raises(pf.invalid_configuration, match="cannot run in place"):
        plan.imdct(both[:3 * n].view(3, n), both[n:4 * n])
    plan.imdct(coeff, out)  # set_imdct_window prepared the type-4 table: dct4 runs too
    y = torch.empty_like(coeff)
    plan.dct4(coeff, y)
    plan.wait()
