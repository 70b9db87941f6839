"""convolve_pairs / correlate_pairs on the GPU (stockham_wg_pairs_kernel): every row of every case against the reference in
double precision (tests/pairs_ref.py, itself held against the O(N^2) sums by test_pairs_reference.py).

One length per kernel shape: fp32 N = 4, 8 (single pass, STAGED), 64, 128 (TWL two-pass), 1024, 4096, 16384 (TW_REGS, FPW 4 /
2 / 1; 16384 is the 139 KiB case), 2000 (compiled at prepare_pairs); fp64 N = 128, 1024, 8192, 6000.  Per length the whole
product of: modes convolve / correlate / correlate with a floor; (x_length, y_length) in (N, N), (N - 1, N / 2 + 1), (1, N),
(N / 2, N / 2) -- the last is alias-free and also goes against np.convolve / np.correlate directly --; out_length N, N - 1,
1; rows 3, 2 FPW - 1, 2 FPW + 1 (ragged last groups).  The three pitches are odd and pairwise different, the base pointers
sit one scalar off 128 bytes, and every third scenario runs on a plan with forward_scale 0.5 and backward_scale 1 / N.

Write set: every launch runs on gpu_utils.Guarded buffers; the guards, every scalar between the rows and behind
out_length, and both inputs must be unchanged, bit for bit.

Yardstick of the plain modes: per-row relative L2 within helpers.REL_L2_TOL of the plan's complex type, the stored row
against the stored part of the reference row, and the per-element rule helpers.check_reference_rule with n = N, as
test_gpu_rconv.py applies them -- one forward depth, one product, one inverse, the chain of the real convolution.  Inputs
are uniform in [-1, 1] from fixed seeds.  Two thirds of the scenarios run on the default scales, where a row is N times
the sum of the definition (the backward transform is unnormalised).
  cancellation   A relative L2 only means something where the row is no cancellation case (the real convolution's finding
                 at N = 4), so the test asserts on its own reference ||r_ref|| >= 1/4 c N ||x|| ||y|| for the stored part
                 of every row at out_length N and N - 1, and |r_ref[0]| >= 1/4 c ||x|| ||y|| for the scalar of out_length 1
                 (cancellation()).  The rows are made on the CPU so that this holds: a row that misses it is drawn again
                 from the same generator (at N = 4, of 513 uniform rows some always have disjoint spectra), never skipped.
  out_length 1   The stored scalar is one element of a transform's result; its error scales with the row, not with itself.
                 It is held to |e_0| <= tau ||r_ref||, which the row's bound implies for every single element, and to the
                 per-element rule (check_plain).
  the rule       Its absolute tolerance 2 eps N log2 N is not scale-free: it was set for N irfft(X H) with a filter of
                 unit-order bins.  A pair row is that with H = c Y, bins of RMS magnitude c ||y||, sqrt(N / 3) at default
                 scales: there 1 of 18 432 elements misses the unchanged rule at N = 1024 (2.4 times the tolerance, next to
                 a zero crossing).  So the absolute branch is multiplied per row by max(1, c min(||x||, ||y||) / sqrt(2 /
                 3)), derived in rule_gain(); with a gain of 1 -- the scaled plan, x of one scalar -- it is the unchanged
                 function.  Every stored scalar of every plain launch is asserted.

Yardstick of the phase transform: |d(P / |P|)| <= |dP| / |P|, so the relative L2 of W is at most kappa times that of P,
and the inverse adds one tau: (kappa + 1) tau with tau = REL_L2_TOL, kappa from the reference spectra of the rounded inputs.
  delta          y from a Hermitian spectrum of constant magnitude and random phases, x = y rotated by d: kappa = max |P| /
                 min |P| (asserted <= 2); the row meets the bound and argmax(r) == d for d in (0, 1, N / 2, N - 1)
  both branches  uniform rows, floor = median |P| of the row (one row per call: the floor is the call's): kappa = sqrt(2)
                 max |P| / floor, with ||W|| >= sqrt(bins / 2)
  huge floor     floor 1e30 (fp64: 1e300): floor * r is the plain correlate row within 2 tau
The worst observed ratio to the bound is printed per length.  In the product of shapes the third mode takes
the median of |P| over the data set as its floor, and kappa of a row from the same inequality without an assumption on the
row: |dW| <= |dP| / max(|P|, floor) <= |dP| / floor gives kappa = ||P|| / (floor ||W||), norms over the whole spectrum.

Also: an all-zero x row gives an exactly zero result row in all three modes; the same tensor as x and y equals a separate
copy, bit for bit; a second call and three one-row calls equal the first call, bit for bit; with NaN in every gap, behind
every row's length and all over the output buffer before the call the results are bit-identical, and NaN in one scalar of
x row i (of y row i) makes exactly output row i non-finite.  What the library refuses on a plan stands at the end.

No case is skipped."""
import numpy as np
import pytest

import helpers as H
import pairs_ref as R

pytestmark = pytest.mark.gpu

LENGTHS = {"f32": [4, 8, 64, 128, 1024, 4096, 16384, 2000], "f64": [128, 1024, 8192, 6000]}
CASES = [(p, n) for p in ("f32", "f64") for n in LENGTHS[p]]
MODES = ("convolve", "correlate", "phat")
HUGE = {"f32": 1e30, "f64": 1e300}


def _mods():
    import gpu_utils as G
    import portfft_amd as pf
    return G, pf, G.torch_mod()


def _types(prec):
    return (np.float32, np.complex64) if prec == "f32" else (np.float64, np.complex128)


def plan_of(pf, n, prec, scales=(1.0, 1.0)):
    d = pf.real_descriptor(n, prec)
    d.forward_scale, d.backward_scale = scales
    plan = d.commit()
    plan.prepare_pairs()
    return plan


def fpw_of(plan, n):
    dim = plan.info().dims[0]
    assert dim.length == n and dim.tier == 1
    return max(1, dim.ffts_per_workgroup)


def pitches_of(n, shift=0):
    """odd, pairwise different, at least N: x, y, out"""
    base = (n | 1) + 2 * shift
    return base + 2, base + 6, base + 4


def run(G, torch, plan, x, y, mode, out_length, pitches, what, floor=None, pad=H.PADDING_VALUE, same=False, poison=()):
    """One launch on guarded buffers whose gaps and guards hold `pad`: rows x (rows, lx) and y (rows, ly) at their pitches,
    base pointers one scalar off 128 bytes; the guards, the gaps, the scalars behind out_length and both inputs are held
    to their bits.  same: y is the tensor of x.  poison: (name, flat index) scalars overwritten with POISON before the
    call.  Returns (the stored rows, the whole output buffer) as numpy."""
    rows = x.shape[0]
    xp, yp, op = pitches
    bufs, hosts = {}, {}
    for name, a, pitch, guard in (("x", x, xp, (65, 63)), ("y", y, yp, (33, 95))):
        host = H.full(rows * pitch, pad, a.dtype)
        idx = (np.arange(rows)[:, None] * pitch + np.arange(a.shape[1])[None, :]).ravel()
        host[idx] = a.ravel()
        for who, at in poison:
            if who == name:
                H.poison_numpy(host, [at])
        g = G.Guarded(rows * pitch, torch.from_numpy(host[:0]).dtype, guard, pad=pad)
        g.buf.copy_(torch.from_numpy(host))
        bufs[name], hosts[name] = g, host
    gout = G.Guarded(rows * op, bufs["x"].buf.dtype, (97, 31), pad=pad)
    xv = bufs["x"].buf.as_strided((rows, x.shape[1]), (xp, 1))
    yv = xv if same else bufs["y"].buf.as_strided((rows, y.shape[1]), (yp, 1))
    ov = gout.buf.as_strided((rows, out_length), (op, 1))
    if mode == "convolve":
        plan.convolve_pairs(xv, yv, ov)
    else:
        plan.correlate_pairs(xv, yv, ov, phat_floor=floor)
    plan.wait()
    for name, g in list(bufs.items()) + [("out", gout)]:
        g.check("%s: %s" % (what, name))
    for name in ("x", "y"):
        H.check_unchanged(hosts[name], bufs[name].buf.cpu().numpy(), what="%s: the input %s" % (what, name))
    raw = gout.buf.cpu().numpy()
    oidx = np.arange(rows)[:, None] * op + np.arange(out_length)[None, :]
    H.check_write_set(raw, oidx, pad=pad, what="%s: output buffer" % (what,))
    return raw[oidx], raw


_worst = {}


def rule_gain(x, y, c):
    """By how much the absolute tolerance of the per-element rule grows with the row's scale.  test_gpu_rconv.py applies
    the rule to N irfft(X H) with the components of H uniform in [-1, 1]: a filter whose bins have the RMS magnitude
    sqrt(2 / 3).  A pair row c N irfft(X Y) is that convolution with the filter H = c Y, whose bins have the RMS magnitude
    c ||y|| (Parseval: sum |Y_k|^2 = N ||y||^2); either operand may stand for the filter, so the smaller one does.  The
    absolute tolerance 2 eps N log2 N is multiplied by max(1, c min(||x||, ||y||) / sqrt(2 / 3)) per row: the rule
    unchanged wherever a row is no larger than the real convolution's, never a tighter one; the relative branch of the
    rule is scale-free and stays what it is."""
    nx, ny = np.linalg.norm(x.astype(np.float64), axis=1), np.linalg.norm(y.astype(np.float64), axis=1)
    return np.maximum(1.0, c * np.minimum(nx, ny) / np.sqrt(2.0 / 3.0))


def check_rule(got, ref, ct, n, gain, what):
    """helpers.check_reference_rule as test_gpu_rconv.py applies it (every element within tol absolutely OR relatively, tol
    = helpers.reference_tolerance, the reference rounded to the plan's type), the absolute branch times gain[row]
    (rule_gain); with a gain of 1 in every row it is that function itself"""
    if np.all(gain == 1.0):
        assert H.check_reference_rule(got, ref.astype(ct), n), (what, "per-element reference rule")
        return
    tol = H.reference_tolerance(ct, n)
    r = ref.astype(ct).real.astype(np.float64)
    a = np.abs(got.astype(np.float64) - r)
    bad = (a > tol * gain[:, None]) & (a > tol * np.maximum(np.abs(r), 1e-300))
    assert not bad.any(), (what, "per-element reference rule", int(bad.sum()), "of", bad.size, "worst over its tolerance",
                           float((a / (tol * gain[:, None]))[bad].max()))


def check_plain(got, ref_full, ct, n, what, gain):
    """The stored rows against the reference.  out_length > 1: the relative L2 of every stored row, against the stored part
    of the reference row, within REL_L2_TOL.  out_length 1: the stored scalar r[0] is one element of a transform's result,
    and the error of one element is not relative to that element but to the row: what the row's bound ||e|| <= tau ||r||
    says about any single element is |e_0| <= tau ||r||, and that is asserted (a relative bound on r[0] alone would need
    |r[0]| several times the row's RMS, which uniform rows do not give).  The per-element rule is asserted on every stored
    scalar in both cases (check_rule).  Returns the worst relative L2."""
    length = got.shape[1]
    ref = ref_full[:, :length]
    scale = np.linalg.norm(ref if length > 1 else ref_full, axis=1)
    err = np.linalg.norm(got.astype(np.float64) - ref, axis=1) / scale
    assert np.all(err <= H.REL_L2_TOL[np.dtype(ct)]), (what, "row", int(np.argmax(err)), float(err.max()))
    check_rule(got, ref, ct, n, gain, what)
    return float(err.max())


def cancellation(x, y, n):
    """rows that are a cancellation case for a stored length, scales of 1 (a row is N times the sum): the stored part of
    the reference row of either mode below 1/4 N ||x|| ||y|| for out_length N or N - 1 -- N times the bound of the
    definition without the factor N of the unnormalised transform, so it implies that one --, or the single stored
    scalar of out_length 1 below 1/4 ||x|| ||y||"""
    nxy = np.linalg.norm(x.astype(np.float64), axis=1) * np.linalg.norm(y.astype(np.float64), axis=1)
    bad = np.zeros(x.shape[0], dtype=bool)
    for correlate in (False, True):
        r = R.pairs(x, y, n, correlate)
        bad |= np.linalg.norm(r, axis=1) < 0.25 * n * nxy
        bad |= np.linalg.norm(r[:, :n - 1], axis=1) < 0.25 * n * nxy
        bad |= np.abs(r[:, 0]) < 0.25 * nxy
    return bad


def draw_rows(rng, rows, lx, ly, n, rt):
    """uniform rows in [-1, 1] of which none is a cancellation case (cancellation()); a row that is one is drawn again from
    the same generator, on the CPU"""
    x = rng.uniform(-1, 1, (rows, lx)).astype(rt)
    y = rng.uniform(-1, 1, (rows, ly)).astype(rt)
    for _ in range(200):
        bad = cancellation(x, y, n)
        if not bad.any():
            return x, y
        x[bad] = rng.uniform(-1, 1, (int(bad.sum()), lx)).astype(rt)
        y[bad] = rng.uniform(-1, 1, (int(bad.sum()), ly)).astype(rt)
    raise AssertionError("no rows without cancellation after 200 draws")


def shapes_of(n):
    return ((n, n), (n - 1, n // 2 + 1), (1, n), (n // 2, n // 2))


def spectrum_norm(p, n):
    """the 2-norm over the whole spectrum of a row given by its half: bins 1 ... N / 2 - 1 count twice"""
    w = np.full(p.shape[-1], 2.0)
    w[0] = w[n // 2] = 1.0
    return np.sqrt((w * np.abs(p) ** 2).sum(axis=-1))


def check_phat(got, ref_full, kappa, ct, n, what):
    """rows with the phase transform: relative L2 of the stored row against the stored part of the reference row (a single
    stored scalar: against the whole row, see check_plain) within (kappa + 1) tau, kappa per row; returns the worst ratio to
    the bound"""
    length = got.shape[1]
    scale = np.linalg.norm(ref_full[:, :length] if length > 1 else ref_full, axis=1)
    err = np.linalg.norm(got.astype(np.float64) - ref_full[:, :length], axis=1) / scale
    bound = (np.asarray(kappa) + 1.0) * H.REL_L2_TOL[np.dtype(ct)]
    assert np.all(err <= bound), (what, "row", int(np.argmax(err / bound)), float(err.max()), float(np.max(err / bound)))
    return float(np.max(err / bound))


@pytest.mark.parametrize("prec,n", CASES)
def test_every_shape_against_the_reference(prec, n):
    G, pf, torch = _mods()
    rt, ct = _types(prec)
    # the plans of the product: the default scales, and every third scenario forward_scale 0.5 and backward_scale 1 / N
    plain, scaled = (1.0, 1.0), (0.5, 1.0 / n)
    plans = {plain: plan_of(pf, n, prec, plain), scaled: plan_of(pf, n, prec, scaled)}
    fpw = fpw_of(plans[plain], n)
    dim = plans[plain].info().dims[0]
    print("N=%d %s: factors %s fpw %d" % (n, prec, list(dim.factors[:dim.n_factors]), fpw))
    rng = np.random.Generator(np.random.SFC64(1000003 * n + (prec == "f64")))
    row_counts = sorted({3, max(1, 2 * fpw - 1), 2 * fpw + 1})
    scenario, worst, worst_phat = 0, 0.0, 0.0
    for lx, ly in shapes_of(n):
        x, y = draw_rows(rng, row_counts[-1], lx, ly, n, rt)
        nx, ny = np.linalg.norm(x.astype(np.float64), axis=1), np.linalg.norm(y.astype(np.float64), axis=1)
        # the floor of this data set: the median of |P| over all its bins, so that both branches are live; kappa of a row
        # from |dW| <= |dP| / max(|P|, floor) <= |dP| / floor: ||dW|| / ||W|| <= (||P|| / (floor ||W||)) ||dP|| / ||P||
        p = R.cross_spectrum(x, y, n, True)
        floor = float(rt(np.median(np.abs(p))))
        kappa = spectrum_norm(p, n) / (floor * spectrum_norm(R.phat_weight(p, floor), n))
        refs, gains = {}, {}
        assert not cancellation(x, y, n).any(), (prec, n, lx, ly, "a cancellation case")  # the precondition, once more
        for scales in plans:
            c = scales[0] * scales[0] * scales[1]
            gains[scales] = rule_gain(x, y, c)
            for mode in MODES:
                refs[scales, mode] = R.pairs(x, y, n, mode != "convolve", None, scales[0], scales[1],
                                             floor if mode == "phat" else None)
            for mode in ("convolve", "correlate"):  # ... and on the references the launches are held to
                assert np.all(np.linalg.norm(refs[scales, mode], axis=1) >= 0.25 * c * n * nx * ny), (prec, n, lx, ly, mode,
                                                                                                       "a cancellation case")
                assert np.all(np.abs(refs[scales, mode][:, 0]) >= 0.25 * c * nx * ny), (prec, n, lx, ly, mode, "r[0] cancels")
            if lx + ly - 1 <= n:  # nothing aliases: NumPy's linear convolution and correlation, directly
                for t in (0, x.shape[0] - 1):
                    a, b = x[t].astype(np.float64), y[t].astype(np.float64)
                    lags = np.correlate(a, b, "full")  # lags -(ly - 1) ... lx - 1
                    lin = np.concatenate([lags[ly - 1:], np.zeros(n - lx - ly + 1), lags[:ly - 1]])
                    assert np.abs(refs[scales, "correlate"][t] - c * n * lin).max() <= 1e-12 * c * n * n
                    conv = np.concatenate([np.convolve(a, b), np.zeros(n - lx - ly + 1)])
                    assert np.abs(refs[scales, "convolve"][t] - c * n * conv).max() <= 1e-12 * c * n * n
        for mode in MODES:
            for out_length in (n, n - 1, 1):
                for rows in row_counts:
                    scales = scaled if scenario % 3 == 2 else plain
                    what = (prec, n, mode, "x %d y %d out %d" % (lx, ly, out_length), "rows %d" % rows, "scales %s" % (scales,))
                    got, _ = run(G, torch, plans[scales], x[:rows], y[:rows], mode, out_length, pitches_of(n, scenario % 4), what,
                                 floor=floor if mode == "phat" else None)
                    if mode == "phat":
                        worst_phat = max(worst_phat, check_phat(got, refs[scales, mode][:rows], kappa[:rows], ct, n, what))
                    else:
                        worst = max(worst, check_plain(got, refs[scales, mode][:rows], ct, n, what, gains[scales][:rows]))
                    scenario += 1
    print("pairs %s N=%d: %d launches, worst rel-L2 of a row %.3e (%.1f times inside the bound); with a floor, worst ratio to "
          "(kappa + 1) tau %.3f" % (prec, n, scenario, worst, H.REL_L2_TOL[np.dtype(ct)] / max(worst, 1e-300), worst_phat))


@pytest.mark.parametrize("prec,n", CASES)
def test_the_phase_transform(prec, n):
    G, pf, torch = _mods()
    rt, ct = _types(prec)
    tau = H.REL_L2_TOL[np.dtype(ct)]
    plan = plan_of(pf, n, prec)
    rng = np.random.Generator(np.random.SFC64(7000003 * n + (prec == "f64")))
    m, pitches = n // 2, pitches_of(n, 1)
    # 1. delta: a Hermitian spectrum of constant magnitude sqrt(N) (samples of order 1) and random phases, bins 0 and M real
    delays = sorted({0, 1, n // 2, n - 1})
    spec = np.sqrt(n) * np.exp(2j * np.pi * rng.uniform(0, 1, m + 1))
    spec[0], spec[m] = np.sqrt(n), -np.sqrt(n)
    y1 = np.fft.irfft(spec, n).astype(rt)
    x = np.stack([np.roll(y1, d) for d in delays])  # x[t, j] = y[j - d]: the rounded row itself, rotated
    y = np.stack([y1] * len(delays))
    p = np.abs(R.cross_spectrum(x, y, n, True))
    kappa = p.max(axis=1) / p.min(axis=1)
    kappa_delta = float(kappa.max())
    assert kappa_delta <= 2.0, (prec, n, "the delta's precondition", kappa_delta)
    floor = float(rt(0.5 * p.min()))
    ref = R.pairs(x, y, n, True, phat_floor=floor)
    got, _ = run(G, torch, plan, x, y, "phat", n, pitches, (prec, n, "delta"), floor=floor)
    ratio_delta = check_phat(got, ref, kappa, ct, n, (prec, n, "delta"))
    assert [int(v) for v in np.argmax(got, axis=1)] == delays, (prec, n, "the peak is the delay")
    # 2. both branches: uniform rows, the floor of a call is the median |P| of its row
    ratio_both = 0.0
    for t in range(3):
        x, y = rng.uniform(-1, 1, (1, n)).astype(rt), rng.uniform(-1, 1, (1, n)).astype(rt)
        p = np.abs(R.cross_spectrum(x, y, n, True))
        floor = float(rt(np.median(p)))
        assert (p > floor).any() and (p < floor).any(), "both branches are live"
        kappa = np.sqrt(2.0) * p.max(axis=1) / floor
        got, _ = run(G, torch, plan, x, y, "phat", n, pitches, (prec, n, "both branches", t), floor=floor)
        ratio_both = max(ratio_both, check_phat(got, R.pairs(x, y, n, True, phat_floor=floor), kappa, ct, n, (prec, n, "both", t)))
    # 3. a huge floor: every bin is P / floor, and floor * r is the plain correlation
    x, y = draw_rows(rng, 3, n, n, n, rt)
    huge = float(rt(HUGE[prec]))
    got, _ = run(G, torch, plan, x, y, "phat", n, pitches, (prec, n, "huge floor"), floor=huge)
    plain = R.pairs(x, y, n, True)
    err = np.linalg.norm(huge * got.astype(np.float64) - plain, axis=1) / np.linalg.norm(plain, axis=1)
    assert np.all(err <= 2 * tau), (prec, n, "huge floor", float(err.max()))
    print("pairs %s N=%d phase transform: worst ratio to the bound: delta %.3f (kappa %.3f), both branches %.3f, huge floor "
          "%.3f" % (prec, n, ratio_delta, kappa_delta, ratio_both, float(err.max() / (2 * tau))))


SMALL = [("f32", 8), ("f32", 128), ("f32", 4096), ("f32", 16384), ("f32", 2000), ("f64", 1024), ("f64", 6000)]


@pytest.mark.parametrize("prec,n", SMALL)
def test_zero_rows_autocorrelation_and_bit_identity(prec, n):
    G, pf, torch = _mods()
    rt, ct = _types(prec)
    plan = plan_of(pf, n, prec)
    fpw = fpw_of(plan, n)
    rows = max(2 * fpw + 1, 5)
    rng = np.random.Generator(np.random.SFC64(9000011 * n + (prec == "f64")))
    x, y = rng.uniform(-1, 1, (rows, n - 1)).astype(rt), rng.uniform(-1, 1, (rows, n // 2 + 1)).astype(rt)
    zero = sorted({0, rows // 2, rows - 1})
    x[zero] = 0
    pitches = pitches_of(n, 2)
    for mode in MODES:
        floor = 1e-3 if mode == "phat" else None
        got, raw = run(G, torch, plan, x, y, mode, n, pitches, (prec, n, mode, "zero rows"), floor=floor)
        assert np.isfinite(got).all(), (prec, n, mode)
        assert not got[zero].any(), (prec, n, mode, "an all-zero x row gives an exactly zero row")
        assert got[[t for t in range(rows) if t not in zero]].any(axis=1).all()
        # a second call
        again, raw2 = run(G, torch, plan, x, y, mode, n, pitches, (prec, n, mode, "second call"), floor=floor)
        H.check_unchanged(raw, raw2, what="%s N=%d %s: a second call" % (prec, n, mode))
        # three rows in one call against three one-row calls
        three, _ = run(G, torch, plan, x[1:4], y[1:4], mode, n, pitches, (prec, n, mode, "three rows"), floor=floor)
        for t in range(3):
            one, _ = run(G, torch, plan, x[1 + t:2 + t], y[1 + t:2 + t], mode, n, pitches, (prec, n, mode, "one row", t), floor=floor)
            H.check_unchanged(three[t], one[0], what="%s N=%d %s: row %d alone" % (prec, n, mode, t))
    # autocorrelation: the same tensor twice against a separate copy of it
    full = rng.uniform(-1, 1, (rows, n)).astype(rt)
    for mode in MODES:
        floor = 1e-3 if mode == "phat" else None
        apart, _ = run(G, torch, plan, full, full.copy(), mode, n, pitches, (prec, n, mode, "x and a copy"), floor=floor)
        same, _ = run(G, torch, plan, full, full, mode, n, pitches, (prec, n, mode, "x twice"), floor=floor, same=True)
        H.check_unchanged(apart, same, what="%s N=%d %s: the same tensor as x and y" % (prec, n, mode))
        if mode == "correlate":  # (an autocorrelation peaks at lag 0: no cancellation case)
            check_plain(same, R.pairs(full, full, n, True), ct, n, (prec, n, "autocorrelation"), rule_gain(full, full, 1.0))


@pytest.mark.parametrize("prec,n", SMALL)
def test_what_a_row_reads(prec, n):
    """the NaN-poison idiom: two runs that differ only in values that must not matter agree bit for bit, and a poisoned
    value that must matter reaches every scalar of its row and no other"""
    G, pf, torch = _mods()
    rt, ct = _types(prec)
    plan = plan_of(pf, n, prec)
    fpw = fpw_of(plan, n)
    rows = 2 * fpw + 1
    rng = np.random.Generator(np.random.SFC64(11000027 * n + (prec == "f64")))
    lx, ly, lo = n - 1, n // 2 + 1, n - 1
    x, y = rng.uniform(-1, 1, (rows, lx)).astype(rt), rng.uniform(-1, 1, (rows, ly)).astype(rt)
    pitches = pitches_of(n, 3)
    xp, yp, op = pitches
    oidx = np.arange(rows)[:, None] * op + np.arange(lo)[None, :]
    victim = sorted({1, rows - 2})
    for mode in MODES:
        floor = 1e-3 if mode == "phat" else None
        what = "%s N=%d %s" % (prec, n, mode)
        _, clean = run(G, torch, plan, x, y, mode, lo, pitches, (what, "clean"), floor=floor)
        # the gaps between the rows, the scalars of a row behind its length, the guards and the output before the call
        _, gaps = run(G, torch, plan, x, y, mode, lo, pitches, (what, "poisoned gaps"), floor=floor, pad=H.POISON)
        H.check_isolated(clean, gaps, oidx.ravel(), [], what + ": poisoned gaps and output", locate=H.rows_of(op))
        # one scalar of x row i, and separately of y row i: exactly output row i
        for name, at in (("x", lambda i: i * xp + lx // 2), ("x", lambda i: i * xp + lx - 1), ("y", lambda i: i * yp + ly - 1),
                         ("y", lambda i: i * yp)):
            _, hit = run(G, torch, plan, x, y, mode, lo, pitches, (what, "poisoned", name), floor=floor,
                         poison=[(name, at(i)) for i in victim])
            others = [t for t in range(rows) if t not in victim]
            H.check_isolated(clean, hit, oidx[others].ravel(), oidx[victim].ravel(), what + ": a poisoned scalar of " + name,
                             locate=H.rows_of(op))


def test_what_the_library_refuses_on_a_plan():
    G, pf, torch = _mods()
    from portfft_amd import _lib
    lib = _lib.lib
    n = 256
    plan = pf.real_descriptor(n, "f32").commit()
    x = torch.zeros(3, n, dtype=torch.float32, device="cuda")
    y, out = torch.ones_like(x), torch.empty_like(x)

    def c_call(p, mode, xa, ya, oa, rows, xl, xp, yl, yp, ol, op, floor):
        return lib.pfft_execute_pairs(p._plan, mode, xa, ya, oa, rows, xl, xp, yl, yp, ol, op, floor)

    # not prepared: the library's own answer, under the binding's
    assert c_call(plan, 1, x.data_ptr(), y.data_ptr(), out.data_ptr(), 3, n, n, n, n, n, n, 0.0) == 1
    assert b"prepare_pairs missing" in lib.pfft_last_error()
    with pytest.raises(pf.invalid_configuration, match="prepare_pairs missing"):
        plan.correlate_pairs(x, y, out)
    plan.prepare_pairs()
    plan.prepare_pairs()
    twin = plan.copy()  # shares the preparation
    twin.correlate_pairs(x, y, out).wait()
    assert float(out.abs().max()) == 0.0
    for args, text in (((2, x.data_ptr(), y.data_ptr(), out.data_ptr(), 3, n, n, n, n, n, n, 0.0), b"mode 2"),
                       ((1, x.data_ptr(), y.data_ptr(), x.data_ptr(), 3, n, n, n, n, n, n, 0.0), b"overlaps an input"),
                       ((1, x.data_ptr(), y.data_ptr(), y.data_ptr(), 3, n, n, n, n, n, n, 0.0), b"overlaps an input"),
                       ((0, x.data_ptr(), y.data_ptr(), out.data_ptr(), 3, n, n, n, n, n, n, 1e-3), b"with PFFT_CONVOLVE"),
                       ((1, x.data_ptr(), y.data_ptr(), out.data_ptr(), 3, n + 1, n + 1, n, n, n, n, 0.0), b"must be in 1 ... 256"),
                       ((1, x.data_ptr(), y.data_ptr(), out.data_ptr(), 3, n, n, n, n, n, n, 1e-42), b"positive normal number")):
        assert c_call(plan, *args) == 1, args
        assert text in lib.pfft_last_error(), (args, lib.pfft_last_error())
    with pytest.raises(pf.invalid_configuration, match="overlaps an input"):
        plan.correlate_pairs(x, y, x)
    # x against y is never checked; overlapping rows of the output of a Python caller are
    plan.correlate_pairs(x, x, out).wait()
    # a plan of the COMPLEX domain
    cplan = pf.descriptor([n], "f32").commit()
    assert lib.pfft_plan_prepare_pairs(cplan._plan) == 1
    assert c_call(cplan, 1, x.data_ptr(), y.data_ptr(), out.data_ptr(), 3, n, n, n, n, n, n, 0.0) == 1
    # a length whose two image sets do not fit the LDS: the real plan commits, prepare_pairs refuses with the reason
    # (M = 10290 = 15 * 14 * 7 * 7 stays an LDS-resident plan; two image sets are at least 2 * 82 320 of 163 840 bytes,
    # however the images are padded)
    big = pf.real_descriptor(20580, "f32").commit()
    with pytest.raises(pf.unsupported_configuration, match="two image sets .* do not fit into LDS"):
        big.prepare_pairs()
    with pytest.raises(pf.invalid_configuration, match="prepare_pairs missing"):
        big.correlate_pairs(torch.zeros(20580, device="cuda"), torch.zeros(20580, device="cuda"), torch.zeros(20580, device="cuda"))
