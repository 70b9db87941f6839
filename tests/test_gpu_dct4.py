"""Fused DCT-IV of real rows and MDCT of real signals (prepare_dct4 / dct4 / set_mdct_window / mdct of a plan of the REAL
domain) on the GPU against NumPy in double (dct4_ref.py: the odd bins of a zero-stuffed FFT of 8N points, which knows
neither the fold identity nor the twiddles the kernel uses).

The lengths of test_gpu_dct.py, one per kernel shape (every registered line runs in test_gpu_dct4_registry.py): fp32
N = 4, 8, 32, 64, 128, 512, 1024, 4096, 16384 pre-compiled, 30 (odd M: a middle item), 2000 and 12000 through the runtime
compiler; fp64 N = 128, 1024, 8192 and 6000.

dct4: 1 (1-D tensors), 3, 2 FPW - 1, 2 FPW + 1 (a ragged last group) and 8 rows; out of place with two different odd pitches
in guarded buffers, in place with one odd pitch; once per placement the base pointers are one scalar off their alignment;
uniform, constant and impulse rows; every third scenario on the scaled plan (forward_scale 0.5, backward_scale 0.25);
`inverse` off and on.  Every row: relative L2 within helpers.REL_L2_TOL and helpers.check_reference_rule(n=N); the write
set; the guards; the input unchanged out of place; and, in addition, dct4(inverse) of dct4 of x over 2N and the scales
against x within 2 REL_L2_TOL.

mdct, per length: three signals with lead N, an in_length that is no multiple of N and frames cut at both ends; lead 0
without a window; lead 2N - 1 with a first and a last frame that hold a single sample each; one signal of 2 FPW + 1 frames
with lead 1; lead N - 2.  Odd pitches of the signals, the frames and the output rows; a random, non-symmetric window or
None.  Every frame against mdct_reference of the windowed, zero-extended frame with the same yardsticks; the write set;
the guards; the input unchanged.

Worst relative L2 per length (MI355X; dct4 forward, inverse and round trip and every mdct scenario; the tests print them):
fp32 N=4 2.2e-07, 8 1.8e-07, 32 1.8e-07, 64 2.0e-07, 128 1.6e-07, 512 1.8e-07, 1024 1.7e-07, 4096 1.9e-07, 16384 2.1e-07, 30
1.8e-07, 2000 2.1e-07, 12000 2.2e-07; fp64 N=128 3.9e-16, 1024 4.1e-16, 8192 4.8e-16, 6000 5.3e-16: a factor 9 inside
REL_L2_TOL (2e-6 / 5e-15), no length within a factor 2 of it.

No case is skipped."""
import re

import numpy as np
import pytest

import helpers as H
from dct4_ref import dct4_reference, frames_of, mdct_reference, overlap_add, tdac_unfold

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


def _plan(pf, n, prec, scaled=False):
    """(plan, (forward_scale, backward_scale), fpw) of a length: committed and prepared once per process"""
    key = (n, prec, scaled)
    if key not in _plans:
        d = pf.real_descriptor(n, prec)
        if scaled:
            d.forward_scale, d.backward_scale = SCALES
        plan = d.commit()
        plan.prepare_dct4()
        _plans[key] = (plan, (d.forward_scale, d.backward_scale), max(1, plan.info().dims[0].ffts_per_workgroup))
    return _plans[key]


def _data(n, rows, rt, rng):
    """rows cycling through the data kinds: uniform, constant, impulses at 0, 1, M - 1, M, N - 2, N - 1"""
    m = n // 2
    x = np.zeros((rows, n), dtype=rt)
    for r in range(rows):
        kind = r % 8
        if kind == 0:
            x[r] = rng.uniform(-1, 1, n).astype(rt)
        elif kind == 1:
            x[r] = rt(0.75)
        else:
            x[r, (0, 1, m - 1, m, n - 2, n - 1)[kind - 2]] = 1
    return x


_worst = {}


def _check(got, ref, ct, n, what, tol_factor=1.0):
    g = np.asarray(got).astype(np.float64)
    r = np.asarray(ref).astype(np.float64)
    err = np.linalg.norm(g - r, axis=1) / np.maximum(np.linalg.norm(r, axis=1), 1e-300)
    key = (np.dtype(ct).name, n)
    _worst[key] = max(_worst.get(key, 0.0), float(err.max()))
    print("%s: worst rel-L2 %.3e (row %d)" % (what, float(err.max()), int(np.argmax(err))))
    assert np.all(err <= tol_factor * H.REL_L2_TOL[np.dtype(ct)]), (what, "row", int(np.argmax(err)), float(err.max()))
    if tol_factor == 1.0:
        assert H.check_reference_rule(g, r.astype(ct), n), (what, "per-element reference rule")


def _odd(v):
    return v | 1


def _dct4(G, torch, plan, inverse, x, in_place, what, guard=None):
    """plan.dct4 of the rows x (numpy, (rows, N)): guarded buffers with odd pitches, the write set, the guards, the input
    unchanged out of place.  Returns the output rows (numpy)."""
    rows, n = x.shape
    tt = torch.from_numpy(x[:0]).dtype
    in_pitch = _odd(n + 3)
    out_pitch = in_pitch if in_place else _odd(n + 7)
    guard = G.GUARD if guard is None else guard
    gin = G.Guarded(rows * in_pitch, tt, guard)
    gin.buf.view(rows, in_pitch)[:, :n].copy_(torch.from_numpy(x))
    gout = gin if in_place else G.Guarded(rows * out_pitch, tt, guard)
    before = gin.buf.cpu().numpy()
    xv = gin.buf.view(rows, in_pitch)[:, :n]
    yv = xv if in_place else gout.buf.view(rows, out_pitch)[:, :n]
    if rows == 1:  # (a single row comes as 1-D tensors)
        xv = xv[0]
        yv = xv if in_place else yv[0]
    plan.dct4(xv, yv, inverse=inverse)
    plan.wait()
    gin.check(str(what) + ": input")
    gout.check(str(what) + ": output")
    if not in_place:
        H.check_unchanged(before, gin.buf.cpu().numpy(), what=str(what) + ": the input")
    raw = gout.buf.cpu().numpy()
    idx = (np.arange(rows)[:, None] * out_pitch + np.arange(n)[None, :]).ravel()
    H.check_write_set(raw, idx, what=str(what) + ": output buffer")
    return raw[idx].reshape(rows, n)


def _scenarios(fpw):
    """(rows, in_place, guard): every row count out of place and in place; one scenario of each placement has a guard of
    65 scalars in front, which puts its base pointers one scalar off their 256-byte alignment"""
    out = []
    counts = []
    for c in (1, 3, 2 * fpw - 1, 2 * fpw + 1, 8):
        if c not in counts:
            counts.append(c)
    for i, c in enumerate(counts):
        out.append((c, False, (65, 64) if i == 1 else None))
        out.append((c, True, (65, 63) if i == 2 else None))
    return out


@pytest.mark.parametrize("prec,n", CASES)
def test_dct4_against_numpy(prec, n):
    G, pf, torch = _mods()
    rt, ct = _types(prec)
    rng = np.random.default_rng(n * 11 + (prec == "f64"))
    fpw = _plan(pf, n, prec)[2]
    for i, (rows, in_place, guard) in enumerate(_scenarios(fpw)):
        plan, (fs, bs), _ = _plan(pf, n, prec, scaled=i % 3 == 2)
        x = _data(n, rows, rt, rng)
        what = "%s N=%d rows=%d %s%s" % (prec, n, rows, "in place" if in_place else "out of place",
                                         " scaled" if i % 3 == 2 else "")
        ref = dct4_reference(x)
        yf = _dct4(G, torch, plan, False, x, in_place, what + " forward", guard)
        _check(yf, fs * ref, ct, n, what + " forward")
        yb = _dct4(G, torch, plan, True, x, in_place, what + " inverse", guard)
        _check(yb, bs * ref, ct, n, what + " inverse")
        back = _dct4(G, torch, plan, True, yf, in_place, what + " round trip", guard)
        _check(back / (2 * n * fs * bs), x, ct, n, what + " round trip", tol_factor=2.0)
    print("worst rel-L2 dct4 %s N=%d: %.3e" % (prec, n, _worst[(np.dtype(ct).name, n)]))


def _mdct(G, torch, plan, x, n, lead, n_frames, what, lead_arg="given"):
    """plan.mdct of the signals x (numpy, (S, L)) into guarded buffers with odd pitches: the guards, the write set, the
    input unchanged.  Returns the coefficients (numpy, (S, F, N))."""
    n_sig, length = x.shape
    tt = torch.from_numpy(x[:0]).dtype
    in_pitch = _odd(length + 3)
    frame_pitch = _odd(n + 3)
    out_pitch = _odd(n_frames * frame_pitch + 5)
    gin = G.Guarded(n_sig * in_pitch, tt)
    gin.buf.view(n_sig, in_pitch)[:, :length].copy_(torch.from_numpy(x))
    gout = G.Guarded(n_sig * out_pitch, tt)
    before = gin.buf.cpu().numpy()
    xv = gin.buf.view(n_sig, in_pitch)[:, :length]
    yv = gout.buf.as_strided((n_sig, n_frames, n), (out_pitch, frame_pitch, 1))
    if n_sig == 1:  # (a single signal comes as a 1-D tensor and a 2-D output)
        xv, yv = xv[0], yv[0]
    if lead_arg == "default":
        plan.mdct(xv, yv)
    else:
        plan.mdct(xv, yv, lead=lead)
    plan.wait()
    gin.check(str(what) + ": input")
    gout.check(str(what) + ": output")
    H.check_unchanged(before, gin.buf.cpu().numpy(), what=str(what) + ": the input")
    raw = gout.buf.cpu().numpy()
    idx = (np.arange(n_sig)[:, None, None] * out_pitch + np.arange(n_frames)[None, :, None] * frame_pitch
           + np.arange(n)[None, None, :]).ravel()
    H.check_write_set(raw, idx, what=str(what) + ": output buffer")
    return raw[idx].reshape(n_sig, n_frames, n)


def _mdct_scenarios(n, fpw):
    """(signals, in_length, lead, frames, windowed, how lead is passed)"""
    return [
        (3, 2 * n + n // 2 + 1, n, 4, True, "default"),          # lead N: the first frame starts at -N, the last ends behind L
        (3, 2 * n + n // 2 + 1, 0, 3, False, "given"),           # no window; the last frame is cut
        (3, 2 * n + 2, 2 * n - 1, 5, True, "given"),             # odd lead: frame 0 holds x[0] alone, frame 4 x[L - 1] alone
        (1, 2 * fpw * n + 3, 1, 2 * fpw + 1, True, "given"),     # 2 FPW + 1 rows: a ragged last group
        (3, 3 * n + 1, n - 2, 3, True, "given"),                 # even lead
    ]


@pytest.mark.parametrize("prec,n", CASES)
def test_mdct_against_numpy(prec, n):
    G, pf, torch = _mods()
    rt, ct = _types(prec)
    rng = np.random.default_rng(n * 13 + (prec == "f64"))
    fpw = _plan(pf, n, prec)[2]
    for i, (n_sig, length, lead, n_frames, windowed, lead_arg) in enumerate(_mdct_scenarios(n, fpw)):
        plan, (fs, _), _ = _plan(pf, n, prec, scaled=i % 3 == 2)
        x = rng.uniform(-1, 1, (n_sig, length)).astype(rt)
        w = rng.uniform(0.25, 1.0, 2 * n).astype(rt) if windowed else None  # (not symmetric)
        plan.set_mdct_window(None if w is None else torch.from_numpy(w).cuda())
        what = "%s N=%d mdct S=%d L=%d lead=%d F=%d%s%s" % (prec, n, n_sig, length, lead, n_frames,
                                                            " windowed" if windowed else "", " scaled" if i % 3 == 2 else "")
        got = _mdct(G, torch, plan, x, n, lead, n_frames, what, lead_arg)
        ref = fs * mdct_reference(frames_of(x, n, lead, n_frames, w))
        _check(got.reshape(-1, n), ref.reshape(-1, n), ct, n, what)
    print("worst rel-L2 dct4+mdct %s N=%d: %.3e" % (prec, n, _worst[(np.dtype(ct).name, n)]))


def test_mdct_then_dct4_reconstructs_the_signal():
    """time-domain alias cancellation end to end at N = 64: sine window, lead N, ceil(L / N) + 1 frames, mdct, dct4(inverse)
    of the coefficient rows, NumPy unfold, window and overlap-add give x times 2N forward_scale backward_scale"""
    G, pf, torch = _mods()
    n, length, n_sig = 64, 5 * 64 + 3, 2
    plan, (fs, bs), _ = _plan(pf, n, "f32", scaled=True)
    rng = np.random.default_rng(64)
    x = rng.uniform(-1, 1, (n_sig, length)).astype(np.float32)
    w = np.sin(np.pi * (np.arange(2 * n) + 0.5) / (2 * n))
    n_frames = -(-length // n) + 1
    plan.set_mdct_window(torch.from_numpy(w.astype(np.float32)).cuda())
    coeff = torch.empty(n_sig, n_frames, n, device="cuda")
    plan.mdct(torch.from_numpy(x).cuda(), coeff)
    rows = coeff.view(n_sig * n_frames, n)
    plan.dct4(rows, rows, inverse=True)
    plan.wait()
    y = rows.cpu().numpy().astype(np.float64).reshape(n_sig, n_frames, n)
    back = overlap_add(tdac_unfold(y) * w, n, n, length) / (2 * n * fs * bs)
    _check(back, x, np.complex64, n, "mdct -> dct4 -> unfold and overlap-add", tol_factor=2.0)


def test_the_verbs_need_their_prepare_and_a_real_plan():
    G, pf, torch = _mods()
    n = 64
    plan = pf.real_descriptor(n).commit()
    x = torch.zeros(3, n, device="cuda")
    y = torch.empty_like(x)
    sig = torch.zeros(3 * n, device="cuda")
    coeff = torch.empty(3, n, device="cuda")
    with pytest.raises(pf.invalid_configuration, match="pfft_plan_prepare_dct4"):
        plan.dct4(x, y)
    with pytest.raises(pf.invalid_configuration, match="pfft_plan_set_mdct_window"):
        plan.mdct(sig, coeff)
    plan.prepare_dct4()
    with pytest.raises(pf.invalid_configuration, match="pfft_plan_set_mdct_window"):  # (prepared, but no window)
        plan.mdct(sig, coeff)
    cplx = pf.descriptor([n]).commit()
    for call in (cplx.prepare_dct4, lambda: cplx.dct4(x, y), lambda: cplx.set_mdct_window(None), lambda: cplx.mdct(sig, coeff)):
        with pytest.raises(pf.invalid_configuration, match="not of the REAL domain"):
            call()
    # the library's own refusal of byte ranges that overlap without being identical (the Python verb passes the strides on)
    wide = torch.zeros(3, n + 5, device="cuda")
    with pytest.raises(pf.invalid_configuration, match="overlap"):
        plan.dct4(wide[:, :n], wide[:, 3:n + 3])
    plan.set_mdct_window(None)
    both = torch.zeros(4 * n, device="cuda")
    with pytest.raises(pf.invalid_configuration, match="cannot run in place"):
        plan.mdct(both[:3 * n], both[n:4 * n].view(3, n))
    # set_mdct_window on an unprepared plan prepares: dct4 runs on it
    other = pf.real_descriptor(n).commit()
    other.set_mdct_window(None)
    other.dct4(x, y)
    other.wait()


@pytest.mark.parametrize("prec,n", [("f32", 512), ("f32", 2000), ("f64", 1024)])
def test_prepare_twice_and_r2c_are_bit_stable(prec, n):
    """a second prepare_dct4 changes no output bit, and R2C of the same plan is what it was before the first"""
    G, pf, torch = _mods()
    rt, ct = _types(prec)
    rng = np.random.default_rng(n)
    rows = 5
    d = pf.real_descriptor(n, prec)
    d.number_of_transforms = rows
    plan = d.commit()
    x = torch.from_numpy(rng.uniform(-1, 1, (rows, n)).astype(rt)).cuda()
    bins = [torch.empty(rows, n // 2 + 1, dtype=torch.from_numpy(np.zeros(0, dtype=ct)).dtype, device="cuda") for _ in range(2)]
    plan.compute_forward(x.reshape(-1), bins[0].reshape(-1))
    plan.wait()
    plan.prepare_dct4()
    outs = []
    for _ in range(2):
        y = torch.empty_like(x)
        plan.dct4(x, y)
        plan.wait()
        outs.append(y)
        plan.prepare_dct4()
    H.check_same_bits(outs[0].reshape(-1), outs[1].reshape(-1), what="dct4 after a second prepare_dct4")
    plan.compute_forward(x.reshape(-1), bins[1].reshape(-1))
    plan.wait()
    H.check_same_bits(bins[0].reshape(-1), bins[1].reshape(-1), what="R2C before and after prepare_dct4")
    copy = plan.copy()
    y = torch.empty_like(x)
    copy.dct4(x, y)
    copy.wait()
    H.check_same_bits(outs[0].reshape(-1), y.reshape(-1), what="dct4 of a copy of the plan")


def _raw(pf, plan, inverse, x, y, n_rows, in_pitch, out_pitch):
    """pfft_execute_dct4 itself: (status, message) -- geometries no tensor has (the refusals come before any launch)"""
    from portfft_amd import _lib
    st = _lib.lib.pfft_execute_dct4(plan._plan, inverse, x.data_ptr(), y.data_ptr(), n_rows, in_pitch, out_pitch)
    return st, _lib.lib.pfft_last_error().decode() if st != 0 else ""


def _raw_mdct(pf, plan, x, y, *geometry):
    from portfft_amd import _lib
    st = _lib.lib.pfft_execute_mdct(plan._plan, x.data_ptr(), y.data_ptr(), *geometry)
    return st, _lib.lib.pfft_last_error().decode() if st != 0 else ""


RANGE_CASES = [("f32", 64, 3), ("f32", 8, 2), ("f32", 4096, 1), ("f32", 16384, 1), ("f64", 1024, 1), ("f32", 2000, 1)]


@pytest.mark.parametrize("prec,n,rows", RANGE_CASES)
def test_the_row_slots_of_a_group_end_below_4_gib(prec, n, rows):
    """The rows kernel addresses row slot f of a group at f * pitch bytes in 32 bits, also the slots of rows that do not
    exist, so FPW * pitch * sizeof(T) must stay below 2^32 whatever n_rows is.  The largest pitch the rule admits runs and
    is right (every row against the reference, the scalars between the rows and the guards untouched); one scalar more is
    refused naming "4 GiB" at every row count, 1 and 2 included (fewer rows than a group holds)."""
    G, pf, torch = _mods()
    rt, ct = _types(prec)
    sb = np.dtype(rt).itemsize
    plan, (fs, bs), fpw = _plan(pf, n, prec)
    top = (2 ** 32 - 1) // (fpw * sb)  # the largest pitch in scalars
    assert top >= n
    tt = torch.from_numpy(np.zeros(0, dtype=rt)).dtype
    small = torch.zeros(2 * n, dtype=tt, device="cuda")
    for inverse in (0, 1):
        for n_rows in (1, 2, fpw, 2 * fpw + 1):
            for ip, op in ((top + 1, n), (n, top + 1), (top + 1, top + 1)):
                st, msg = _raw(pf, plan, inverse, small, small[n:], n_rows, ip, op)
                assert st == 2 and "4 GiB" in msg, (inverse, n_rows, ip, op, st, msg)
    rng = np.random.default_rng(n)
    x = rng.uniform(-1, 1, (rows, n)).astype(rt)
    count = (rows - 1) * top + n
    for in_place in (False, True):
        gin = G.Guarded(count, tt)
        for r in range(rows):
            gin.buf[r * top:r * top + n].copy_(torch.from_numpy(x[r]))
        gout = gin if in_place else G.Guarded(count, tt)
        st, msg = _raw(pf, plan, 0, gin.buf, gout.buf, rows, top, top)
        assert st == 0, msg
        plan.wait()
        what = "%s N=%d rows=%d pitch %d %s" % (prec, n, rows, top, "in place" if in_place else "out of place")
        gin.check(what + ": input")
        gout.check(what + ": output")
        got = np.stack([gout.buf[r * top:r * top + n].cpu().numpy() for r in range(rows)])
        _check(got, fs * dct4_reference(x), ct, n, what)
        for r in range(rows - 1):  # the scalars between the rows, on the device
            gap = gout.buf[r * top + n:(r + 1) * top]
            assert bool((gap == H.PADDING_VALUE).all()), (what, "written between rows", r)
        if not in_place:
            for r in range(rows):
                H.check_unchanged(x[r], gin.buf[r * top:r * top + n].cpu().numpy(), what=what + ": the input")
        del gin, gout
    torch.cuda.empty_cache()


def test_refusals_of_the_library_name_the_cause():
    """what no tensor can express: in == out with different pitches, 2^31 rows, null pointers, no rows; and the MDCT's
    geometry rules through the C call"""
    G, pf, torch = _mods()
    n = 64
    plan = _plan(pf, n, "f32")[0]
    buf = torch.zeros(4 * (n + 8), device="cuda")
    other = torch.zeros(4 * (n + 8), device="cuda")
    for args, status, text in (
            ((0, buf, buf, 3, n, n + 1), 1, "equal pitches"), ((1, buf, buf, 3, n + 2, n), 1, "equal pitches"),
            ((0, buf, other, 2 ** 31, n, n), 2, r"2\^31"), ((1, buf, other, 2 ** 40, n, n), 2, r"2\^31"),
            ((0, buf, other, 0, n, n), 1, "n_rows 0"),
            ((0, buf, other, 3, n - 1, n), 1, "in_pitch 63"), ((0, buf, other, 3, n, n - 2), 1, "out_pitch 62")):
        st, msg = _raw(pf, plan, *args)
        assert st == status and re.search(text, msg), (args[0], args[3:], st, msg)
    from portfft_amd import _lib
    assert _lib.lib.pfft_execute_dct4(plan._plan, 0, None, other.data_ptr(), 1, n, n) == 1
    assert b"null data pointer" in _lib.lib.pfft_last_error()
    st, msg = _raw(pf, plan, 0, buf, other, 3, n + 8, n + 8)
    assert st == 0, msg
    plan.wait()
    plan.set_mdct_window(None)
    sig = torch.zeros(4 * n, device="cuda")
    out = torch.zeros(8 * n, device="cuda")
    # (n_signals, in_length, in_pitch, lead, n_frames, frame_pitch, out_pitch)
    for geometry, status, text in (
            ((0, 3 * n, 3 * n, n, 4, n, 4 * n), 1, "zero count"), ((1, 3 * n, 3 * n, n, 0, n, 4 * n), 1, "zero count"),
            ((1, 3 * n, 3 * n, 2 * n, 4, n, 4 * n), 1, "lead 128"), ((1, 3 * n, 3 * n - 1, n, 4, n, 4 * n), 1, "in_pitch 191"),
            ((1, 3 * n, 3 * n, n, 4, n - 1, 4 * n), 1, "frame_pitch 63"), ((1, 3 * n, 3 * n, n, 2 ** 32, n, 4 * n), 2, r"2\^32"),
            ((1, 3 * n, 3 * n, n, 4, n, 4 * n - 1), 1, "out_pitch 255"), ((1, 3 * n, 3 * n, n, 6, n, 6 * n), 1, "at least one sample")):
        st, msg = _raw_mdct(pf, plan, sig, out, *geometry)
        assert st == status and re.search(text, msg), (geometry, st, msg)
    assert _lib.lib.pfft_execute_mdct(plan._plan, None, out.data_ptr(), 1, 3 * n, 3 * n, n, 4, n, 4 * n) == 1
    assert b"null data pointer" in _lib.lib.pfft_last_error()
    st, msg = _raw_mdct(pf, plan, sig, out, 1, 3 * n, 3 * n, n, 4, n, 4 * n)
    assert st == 0, msg
    plan.wait()
