"""Fused discrete cosine transforms of type 2 and 3 (prepare_dct / dct of a plan of the REAL domain) on the GPU against
NumPy in double (dct_ref.py: scipy.fft.dct(x, type, norm=None) times the plan's scale, from NumPy's FFT alone).

One length per kernel shape, as test_gpu_stft.py (every registered line of the kernels runs in
test_gpu_fused_registry.py): fp32 N = 4 (both special items and nothing else), 8, 32, 64, 128, 512,
1024, 4096, 16384 pre-compiled, 30 (odd M: no 2k = M item), 2000 (even M, no power of two) and 12000 through the runtime
compiler; fp64 N = 128, 1024, 8192 and 6000.  Row counts: 1 (1-D tensors), 3, 2 FPW - 1 and 2 FPW + 1 (a ragged last
group) and the eight rows of the data kinds.  Placement: out of place with two different odd pitches in guarded buffers,
in place with one odd pitch; once per case the base pointers are one scalar off their alignment.  Data: uniform in
[-1, 1], a constant row, unit impulses at 0, 1, M - 1, M, N - 2 and N - 1 (an index-map error shows as a whole wrong row).
Every third scenario runs on the scaled plan (forward_scale = 0.5, backward_scale = 0.25).

Both types, every row: relative L2 within helpers.REL_L2_TOL of the precision's complex dtype and
helpers.check_reference_rule(n=N); the write set (guards and every scalar between the rows bit-identical); the input
unchanged out of place; type 3 of type 2 of x over 2N (and the scales) against x within 2 REL_L2_TOL.

Worst relative L2 per length (MI355X, both types and the round trip, all scenarios; the test prints them): fp32 N=4
1.6e-07, 8 1.8e-07, 32 1.8e-07, 64 1.6e-07, 128 1.6e-07, 512 1.8e-07, 1024 1.8e-07, 4096 1.9e-07, 16384 2.1e-07, 30 1.9e-07,
2000 2.3e-07, 12000 2.1e-07; fp64 N=128 3.4e-16, 1024 3.6e-16, 8192 4.1e-16, 6000 4.7e-16: a factor 8 and 10 inside
REL_L2_TOL (2e-6 / 5e-15), no length within a factor 2 of it.

Address range: a work-group addresses its FPW row slots at f * pitch bytes in 32 bits, also the slots of missing rows, so
FPW * pitch * sizeof(T) stays below 2^32; the largest pitch the rule admits runs (both types, both placements, gaps and
guards untouched) and one scalar more is refused naming "4 GiB" at 1, 2, FPW and 2 FPW + 1 rows.  The refusals no tensor
can express (in == out with different pitches, 2^31 rows, a bad type, no rows, null pointers) go through the C call.

No case is skipped."""
import re

import numpy as np
import pytest

import helpers as H
from dct_ref import dct_reference

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
        plan.prepare_dct()
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


def _dct(G, torch, plan, kind, x, in_place, what, guard=None):
    """plan.dct of the rows x (numpy, (rows, N)): guarded buffers with odd pitches, the write set, the guards, the input
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
    plan.dct(xv, yv, type=kind)
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
def test_dct_against_numpy(prec, n):
    G, pf, torch = _mods()
    rt, ct = _types(prec)
    rng = np.random.default_rng(n * 7 + (prec == "f64"))
    fpw = _plan(pf, n, prec)[2]
    for i, (rows, in_place, guard) in enumerate(_scenarios(fpw)):
        plan, (fs, bs), _ = _plan(pf, n, prec, scaled=i % 3 == 2)
        x = _data(n, rows, rt, rng)
        what = "%s N=%d rows=%d %s%s" % (prec, n, rows, "in place" if in_place else "out of place",
                                         " scaled" if i % 3 == 2 else "")
        y2 = _dct(G, torch, plan, 2, x, in_place, what + " type 2", guard)
        _check(y2, fs * dct_reference(x, 2), ct, n, what + " type 2")
        y3 = _dct(G, torch, plan, 3, x, in_place, what + " type 3", guard)
        _check(y3, bs * dct_reference(x, 3), ct, n, what + " type 3")
        back = _dct(G, torch, plan, 3, y2, in_place, what + " round trip", guard)
        _check(back / (2 * n * fs * bs), x, ct, n, what + " round trip", tol_factor=2.0)
    print("worst rel-L2 %s N=%d: %.3e" % (prec, n, _worst[(np.dtype(ct).name, n)]))


def test_dct_needs_prepare_and_a_real_plan():
    G, pf, torch = _mods()
    n = 64
    plan = pf.real_descriptor(n).commit()
    x = torch.zeros(3, n, device="cuda")
    y = torch.empty_like(x)
    with pytest.raises(pf.invalid_configuration, match="pfft_plan_prepare_dct"):
        plan.dct(x, y)
    with pytest.raises(pf.invalid_configuration, match="pfft_plan_prepare_dct"):
        plan.dct(x, y, type=3)
    cplx = pf.descriptor([n]).commit()
    with pytest.raises(pf.invalid_configuration, match="not of the REAL domain"):
        cplx.prepare_dct()
    with pytest.raises(pf.invalid_configuration, match="not of the REAL domain"):
        cplx.dct(x, y)
    plan.prepare_dct()
    # the library's own refusal of byte ranges that overlap without being identical (the Python verb passes the strides on)
    wide = torch.zeros(3, n + 5, device="cuda")
    with pytest.raises(pf.invalid_configuration, match="overlap"):
        plan.dct(wide[:, :n], wide[:, 3:n + 3])
    with pytest.raises(pf.invalid_configuration, match="overlap"):
        plan.dct(x.reshape(-1)[:2 * n].view(2, n), x.reshape(-1)[n:3 * n].view(2, n))


@pytest.mark.parametrize("prec,n", [("f32", 512), ("f32", 2000), ("f64", 1024)])
def test_prepare_twice_and_r2c_are_bit_stable(prec, n):
    """a second prepare_dct changes no output bit, and R2C of the same plan is what it was before the first"""
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
    plan.prepare_dct()
    outs = []
    for _ in range(2):
        y = torch.empty_like(x)
        plan.dct(x, y, type=2)
        z = torch.empty_like(x)
        plan.dct(x, z, type=3)
        plan.wait()
        outs.append((y, z))
        plan.prepare_dct()
    H.check_same_bits(outs[0][0].reshape(-1), outs[1][0].reshape(-1), what="type 2 after a second prepare_dct")
    H.check_same_bits(outs[0][1].reshape(-1), outs[1][1].reshape(-1), what="type 3 after a second prepare_dct")
    plan.compute_forward(x.reshape(-1), bins[1].reshape(-1))
    plan.wait()
    H.check_same_bits(bins[0].reshape(-1), bins[1].reshape(-1), what="R2C before and after prepare_dct")
    copy = plan.copy()
    y = torch.empty_like(x)
    copy.dct(x, y, type=2)
    copy.wait()
    H.check_same_bits(outs[0][0].reshape(-1), y.reshape(-1), what="type 2 of a copy of the plan")


def _raw(pf, plan, kind, x, y, n_rows, in_pitch, out_pitch):
    """pfft_execute_dct itself: (status, message) -- geometries no tensor has (the refusals come before any launch)"""
    from portfft_amd import _lib
    st = _lib.lib.pfft_execute_dct(plan._plan, kind, x.data_ptr(), y.data_ptr(), n_rows, in_pitch, out_pitch)
    return st, _lib.lib.pfft_last_error().decode() if st != 0 else ""


RANGE_CASES = [("f32", 64, 3), ("f32", 8, 2), ("f32", 4096, 1), ("f32", 16384, 1), ("f64", 1024, 1), ("f32", 2000, 1)]


@pytest.mark.parametrize("prec,n,rows", RANGE_CASES)
def test_the_row_slots_of_a_group_end_below_4_gib(prec, n, rows):
    """The kernel addresses row slot f of a group at f * pitch bytes in 32 bits, also the slots of rows that do not exist,
    so FPW * pitch * sizeof(T) must stay below 2^32 whatever n_rows is.  The largest pitch the rule admits runs and is
    right (every row against the reference, the scalars between the rows and the guards untouched); one scalar more is
    refused naming "4 GiB" at every row count, 1 and 2 included (fewer rows than a group holds)."""
    G, pf, torch = _mods()
    rt, ct = _types(prec)
    sb = np.dtype(rt).itemsize
    plan, (fs, bs), fpw = _plan(pf, n, prec)
    top = (2 ** 32 - 1) // (fpw * sb)  # the largest pitch in scalars
    assert top >= n
    tt = torch.from_numpy(np.zeros(0, dtype=rt)).dtype
    small = torch.zeros(2 * n, dtype=tt, device="cuda")
    for kind in (2, 3):
        for n_rows in (1, 2, fpw, 2 * fpw + 1):
            for ip, op in ((top + 1, n), (n, top + 1), (top + 1, top + 1)):
                st, msg = _raw(pf, plan, kind, small, small[n:], n_rows, ip, op)
                assert st == 2 and "4 GiB" in msg, (kind, n_rows, ip, op, st, msg)
    rng = np.random.default_rng(n)
    x = rng.uniform(-1, 1, (rows, n)).astype(rt)
    count = (rows - 1) * top + n
    for kind, scale in ((2, fs), (3, bs)):
        for in_place in (False, True):
            gin = G.Guarded(count, tt)
            for r in range(rows):
                gin.buf[r * top:r * top + n].copy_(torch.from_numpy(x[r]))
            gout = gin if in_place else G.Guarded(count, tt)
            st, msg = _raw(pf, plan, kind, gin.buf, gout.buf, rows, top, top)
            assert st == 0, msg
            plan.wait()
            what = "%s N=%d rows=%d pitch %d type %d %s" % (prec, n, rows, top, kind, "in place" if in_place else "out of place")
            gin.check(what + ": input")
            gout.check(what + ": output")
            got = np.stack([gout.buf[r * top:r * top + n].cpu().numpy() for r in range(rows)])
            _check(got, scale * dct_reference(x, kind), ct, n, what)
            for r in range(rows - 1):  # the scalars between the rows, on the device
                gap = gout.buf[r * top + n:(r + 1) * top]
                assert bool((gap == H.PADDING_VALUE).all()), (what, "written between rows", r)
            if not in_place:
                for r in range(rows):
                    H.check_unchanged(x[r], gin.buf[r * top:r * top + n].cpu().numpy(), what=what + ": the input")
            del gin, gout
    torch.cuda.empty_cache()


def test_refusals_of_the_library_name_the_cause():
    """what no tensor can express: in == out with different pitches, 2^31 rows, null pointers, a bad type, no rows"""
    G, pf, torch = _mods()
    n = 64
    plan = _plan(pf, n, "f32")[0]
    buf = torch.zeros(4 * (n + 8), device="cuda")
    other = torch.zeros(4 * (n + 8), device="cuda")
    for args, status, text in (
            ((2, buf, buf, 3, n, n + 1), 1, "equal pitches"), ((3, buf, buf, 3, n + 2, n), 1, "equal pitches"),
            ((2, buf, other, 2 ** 31, n, n), 2, r"2\^31"), ((3, buf, other, 2 ** 40, n, n), 2, r"2\^31"),
            ((4, buf, other, 3, n, n), 1, "type 4"), ((2, buf, other, 0, n, n), 1, "n_rows 0"),
            ((2, buf, other, 3, n - 1, n), 1, "in_pitch 63"), ((2, buf, other, 3, n, n - 2), 1, "out_pitch 62")):
        st, msg = _raw(pf, plan, *args)
        assert st == status and re.search(text, msg), (args[0], args[3:], st, msg)
    from portfft_amd import _lib
    assert _lib.lib.pfft_execute_dct(plan._plan, 2, None, other.data_ptr(), 1, n, n) == 1
    assert b"null data pointer" in _lib.lib.pfft_last_error()
    # the same rows, accepted: 2^31 - 1 rows would pass the count (not launched here), 3 rows run
    st, msg = _raw(pf, plan, 2, buf, other, 3, n + 8, n + 8)
    assert st == 0, msg
    plan.wait()
