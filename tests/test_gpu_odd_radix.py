"""Every fused verb on the odd-radix and ragged configurations of the runtime planner (helpers.ODD_RADIX_LENGTHS: one M per
configuration class and precision; test_odd_radix_classes.py holds the table to the host planner).  The real verbs run at
N = 2M, the complex convolution and filter at N = M.  None of these lengths has a pre-compiled line: every case commits
(or prepares) once, which compiles the verb's kernel for that configuration, and runs a handful of rows.

What a case checks is what the verb's own module and test_gpu_isolation.py / test_gpu_basis.py check -- their runners are
imported, nothing is restated and no yardstick is new:
  R2C, C2R, DCT-II / III, DCT-IV   check_basis_rows on ALL N impulses (bound 3.3 u P(N/2) + ..., test_gpu_basis.py), out of
                                   place, in place and scaled with offsets; and one clean-versus-poisoned pair of runs
  every other verb                 the NumPy / long-double reference with REL_L2_TOL and the per-element rule on the clean
                                   run, guards, write set and unchanged input on every launch, and helpers.check_isolated
                                   with gaps, guards, the output before the call and a neighbouring row / signal / frame /
                                   sample poisoned: an idle lane of a ragged pass that loads or stores shows here
Shapes: 2 FPW + 1 rows (513 in the work-item form), rows 1 and batch - 2 poisoned, so every group but the last is full and
the last holds one row; three signals whose frame counts leave a ragged last group.  stft / periodogram / istft: the hop is
helpers.odd_radix_hop (odd, coprime to N), the lead N/2 +- 1; mdct / imdct: lead N + 1.  periodogram: frames_per_row 1, 3
and n_frames.  istft and imdct: chunk_frames 0, 1 and 2 FPW + 1.  Filters: 1 tap, an odd count near N/2, and the largest the
verb takes -- N (complex), N - 2 (real: include/portfft_amd.h refuses more) --, convolve and correlate.  Pairs: x_length
N - 1, y_length N/2 + 1, out_length N - 1 (odd), FPW + 1 rows against pairs_ref, plain and with a floor at the median |P|;
then test_gpu_pairs.test_what_a_row_reads.

Every case first asserts on plan.info() that the plan is the one-launch LDS-resident work-group plan (tier 1) whose radices,
lanes per transform and transforms per group have the property of the row's class (helpers.odd_radix_class_miss): a
fall-back to another tier or a planner that moved the length fails before anything is compared.

Filter taps are uniform in [-1, 1] / sqrt(K), as test_gpu_filter.py and test_gpu_rfilter.py draw them (_filter_case says
what unscaled taps measured).  Radix 61 (976 = 16 x 61) runs for R2C / C2R and the DCT-IV only: helpers.ODD_RADIX_61.

Measured on the MI355X, worst over all rows (fp32 / fp64; records, not inputs to any bound).  Ratio to the basis bound: R2C
0.11 / 0.13, C2R 0.10 / 0.13, DCT-II 0.11 / 0.12, DCT-III 0.10 / 0.14, DCT-IV 0.10 / 0.14.  Rel-L2 over REL_L2_TOL: R2C 0.07 /
0.08, C2R 0.07 / 0.08, DCT-II 0.08 / 0.08, DCT-III 0.08 / 0.09, DCT-IV 0.08 / 0.08, mdct and imdct 0.10 / 0.09, stft and istft
0.08 / 0.08, real and complex convolve / correlate and the plain pairs 0.14 / 0.16, real filter 0.15 / 0.16, complex filter
0.17 / 0.12; periodogram rel-L1 over its bound 0.05 / 0.05; pairs with a floor 0.05 / 0.06 of (kappa + 1) tau.  Every class
check on plan.info() held; no kernel, geometry or table was found wrong on these configurations.
398 cases: 310 s from an empty code-object cache (the commit-time compiles), 14 s warm.  Cold, a case takes 0.1 - 2 s
without a prime radix and 2 - 9 s with radix 37; the exceptions are the commits that compile four kernels or radix 61:
complex convolve at 592 = 16 x 37 13.9 s, R2C / C2R at 976 = 16 x 61 9.9 s.  Warm, the slowest case takes 2.1 s.

No case is skipped."""
import numpy as np
import pytest

import helpers as H

pytestmark = pytest.mark.gpu

ROWS = [(p, m, cls) for p in ("f32", "f64") for m, cls in H.ODD_RADIX_LENGTHS[p]]
ROWS_61 = ROWS + [(p, m, cls) for p in ("f32", "f64") for m, cls in H.ODD_RADIX_61[p]]


def _ids(table):
    return ["%s-M%d-%s" % (p, m, cls.replace(" ", "_").replace(",", "").replace("/", "over")) for p, m, cls in table]


rows = pytest.mark.parametrize("prec,m,cls", ROWS, ids=_ids(ROWS))
rows_and_radix_61 = pytest.mark.parametrize("prec,m,cls", ROWS_61, ids=_ids(ROWS_61))  # (helpers.ODD_RADIX_61 says which verbs)


def _mods():
    import gpu_utils as G
    import portfft_amd as pf
    return G, pf, G.torch_mod()


def _iso():
    import test_gpu_isolation as ISO
    return ISO


def _basis():
    import test_gpu_basis as BASIS
    return BASIS


def _assert_class(info, n, m, cls, what):
    """the plan behind `info` is the one-launch work-group plan of an M-point transform in the row's class"""
    dim = info.dims[0]
    radices = [int(v) for v in dim.factors[:dim.n_factors]]
    # (a complex plan of a single radix reports the register tier: the same one-launch kernel, one lane per transform)
    tiers = (0, 1) if cls.startswith("work-item") and n == m else (1,)
    assert dim.length == n and dim.tier in tiers and tuple(info.launches) == (1, 1), (what, dim.length, dim.tier, tuple(info.launches))
    assert 0 < dim.lds_bytes <= 160 * 1024 and dim.workgroup_size % max(1, dim.ffts_per_workgroup) == 0, (what, dim.lds_bytes)
    fpw = max(1, dim.ffts_per_workgroup)
    miss = H.odd_radix_class_miss(cls, m, radices, dim.workgroup_size // fpw, fpw)
    assert miss is None, (what, miss)
    print("%s: radices %s, %d lanes, %d per group, %d bytes of LDS" % (what, radices, dim.workgroup_size // fpw, fpw, dim.lds_bytes))


def _real(prec, m, cls):
    """N of the real verbs, after the class check on the real plan"""
    G, pf, torch = _mods()
    n = 2 * m
    _assert_class(_iso()._real_plan(pf, n, prec).info(), n, m, cls, "real plan %s N=%d" % (prec, n))
    return n


@pytest.fixture(autouse=True)
def _all_rows_and_figures(monkeypatch):
    """every impulse in the basis runners (they sample above N = 1024); the hop of the table in the analysis geometry; and
    the rel-L2 figures of the runners that assert without printing"""
    ISO, BASIS = _iso(), _basis()
    monkeypatch.setattr(BASIS, "_real_rows", lambda pf, n, prec, dct_plan=None: np.arange(n))
    geometry = ISO._analysis_geometry

    def analysis_geometry(n, fpw, pad):
        hop, lead, frames, length = geometry(n, fpw, pad)
        mine = H.odd_radix_hop(n)
        return mine, lead, frames, length + (frames - 1) * (mine - hop)

    monkeypatch.setattr(ISO, "_analysis_geometry", analysis_geometry)
    asserted = ISO._rel_l2_rows

    def rel_l2_rows(got, ref, ct, n, what):
        g = np.asarray(got).astype(np.complex128).reshape(len(ref), -1)
        r = np.asarray(ref).astype(np.complex128).reshape(len(ref), -1)
        err = np.linalg.norm(g - r, axis=1) / np.maximum(np.linalg.norm(r, axis=1), 1e-300)
        print("%s: worst rel-L2 %.3e (row %d)" % (what, float(err.max()), int(np.argmax(err))))
        asserted(got, ref, ct, n, what)

    monkeypatch.setattr(ISO, "_rel_l2_rows", rel_l2_rows)


# ---------------------------------------------------------------------------------------------------------------------
# rows: R2C / C2R, the DCTs

@rows_and_radix_61
def test_r2c_and_c2r_of_every_impulse(prec, m, cls):
    _basis().test_real_transforms_of_basis_vectors(prec, _real(prec, m, cls))


@rows
def test_r2c_and_c2r_with_poisoned_neighbours(prec, m, cls):
    _iso().test_real_transforms_with_poisoned_neighbours(prec, _real(prec, m, cls))


@rows
def test_dct_2_and_3_of_every_impulse(prec, m, cls):
    _basis().test_dct_2_and_3_of_basis_vectors(prec, _real(prec, m, cls))


@rows_and_radix_61
def test_dct_4_of_every_impulse(prec, m, cls):
    _basis().test_dct_4_of_basis_vectors(prec, _real(prec, m, cls))


@rows
def test_dcts_with_poisoned_gaps_and_neighbours(prec, m, cls):
    _iso().test_dcts_with_poisoned_gaps_and_neighbours(prec, _real(prec, m, cls))


# ---------------------------------------------------------------------------------------------------------------------
# long signals

@rows
def test_mdct(prec, m, cls):
    _iso().test_mdct_reads_its_frames_only(prec, _real(prec, m, cls))


@rows
def test_imdct(prec, m, cls):
    _iso().test_imdct_spreads_a_frame_over_its_samples_only(prec, _real(prec, m, cls))


@pytest.mark.parametrize("pad", ["zero", "reflect"])
@rows
def test_stft(prec, m, cls, pad):
    _iso().test_stft_reads_its_frames_only(prec, _real(prec, m, cls), pad)


@pytest.mark.parametrize("normalize", [False, True], ids=["plain", "normalized"])
@rows
def test_istft(prec, m, cls, normalize):
    import test_gpu_istft as I
    n = _real(prec, m, cls)
    hop = H.odd_radix_hop(n)

    def reference(y, w, lead, olen):
        ola, env = I._reference(1.0, y, w, n, hop, lead, olen)
        assert env.min() >= 0.25
        return ola / env if normalize else ola

    _iso()._synthesis(prec, n, "istft normalize" if normalize else "istft plain", n, n // 2 + 1, hop,
                      lambda plan, w: plan.set_synthesis_window(w),
                      lambda plan, a, b, lead, chunk: plan.istft(a, b, hop, lead=lead, normalize=normalize, chunk_frames=chunk),
                      reference, I._check)


@rows
def test_periodogram(prec, m, cls):
    _iso().test_periodogram_reads_its_frames_only(prec, _real(prec, m, cls), "reflect")


# ---------------------------------------------------------------------------------------------------------------------
# convolutions and filters

def _tap_counts(n, largest):
    return sorted({1, min((n // 2) | 1, largest), largest})


def _filter_case(monkeypatch, kind, prec, n, k, correlate):
    """test_gpu_isolation's filter case with the taps drawn as the verb's own module draws them, uniform in [-1, 1] /
    sqrt(K) (test_gpu_filter.py, test_gpu_rfilter.py): the absolute branch of the per-element rule is not scale-free, and
    K near N / 2 unscaled puts c sqrt(K) / 3 -- 2e4 at N = 2002 -- into every output.  (Measured with unscaled taps at the
    middle K of N = 486, 2002, 2738 and 4736, fp32 and fp64: every signal inside REL_L2_TOL, and a few elements next to a
    zero crossing outside the rule; K = 1 and K = N - 2 inside both.)"""
    ISO = _iso()
    uniform = ISO._uniform

    def scaled(rng, shape, dtype):
        a = uniform(rng, shape, dtype)
        return (a / np.sqrt(k)).astype(a.dtype) if tuple(shape) == (1, k) else a

    monkeypatch.setattr(ISO, "_uniform", scaled)
    ISO.test_filter_outputs_between_the_cone_and_the_segments(kind, prec, n, k, correlate)
    monkeypatch.setattr(ISO, "_uniform", uniform)


@rows
def test_real_convolve_and_correlate(prec, m, cls):
    _iso().test_real_convolution_with_a_poisoned_filter_rows_and_ignored_parts(prec, _real(prec, m, cls))


@rows
def test_real_filter(prec, m, cls, monkeypatch):
    n = _real(prec, m, cls)
    for k in _tap_counts(n, n - 2):
        for correlate in (False, True):
            _filter_case(monkeypatch, "real", prec, n, k, correlate)


@rows
def test_complex_convolve_and_correlate(prec, m, cls):
    import test_gpu_conv as C
    G, pf, torch = _mods()
    _assert_class(C._desc(pf, m, prec).commit().info(), m, m, cls, "convolution plan %s N=%d" % (prec, m))
    _iso().test_complex_convolution_with_a_poisoned_filter_and_rows(prec, m)


@rows
def test_complex_filter(prec, m, cls, monkeypatch):
    import test_gpu_filter as FC
    G, pf, torch = _mods()
    _assert_class(FC._plan(pf, m, prec)[0].info(), m, m, cls, "convolution plan %s N=%d" % (prec, m))
    for k in _tap_counts(m, m):
        for correlate in (False, True):
            _filter_case(monkeypatch, "complex", prec, m, k, correlate)


# ---------------------------------------------------------------------------------------------------------------------
# pairs

@rows
def test_pairs_against_the_reference(prec, m, cls):
    """x_length N - 1, y_length N / 2 + 1, out_length N - 1 (odd), FPW + 1 rows: convolve, correlate, correlate with a floor
    at the median of |P| (both branches live), with the yardsticks of test_gpu_pairs.py"""
    import pairs_ref as R
    import test_gpu_pairs as PR
    G, pf, torch = _mods()
    n = _real(prec, m, cls)
    rt, ct = PR._types(prec)
    plan = PR.plan_of(pf, n, prec)
    _assert_class(plan.info(), n, m, cls, "prepared plan %s N=%d" % (prec, n))
    count = PR.fpw_of(plan, n) + 1
    lx, ly, lo = n - 1, n // 2 + 1, n - 1
    x, y = PR.draw_rows(np.random.Generator(np.random.SFC64(13000039 * n + (prec == "f64"))), count, lx, ly, n, rt)
    p = R.cross_spectrum(x, y, n, True)
    floor = float(rt(np.median(np.abs(p))))
    assert (np.abs(p) > floor).any() and (np.abs(p) < floor).any()
    kappa = PR.spectrum_norm(p, n) / (floor * PR.spectrum_norm(R.phat_weight(p, floor), n))
    gain = PR.rule_gain(x, y, 1.0)
    for mode in PR.MODES:
        what = (prec, n, mode, "x %d y %d out %d" % (lx, ly, lo), "rows %d" % count)
        got, _ = PR.run(G, torch, plan, x, y, mode, lo, PR.pitches_of(n, 1), what, floor=floor if mode == "phat" else None)
        if mode == "phat":
            ratio = PR.check_phat(got, R.pairs(x, y, n, True, phat_floor=floor), kappa, ct, n, what)
            print("%s: worst ratio to (kappa + 1) tau %.3f" % (what, ratio))
        else:
            worst = PR.check_plain(got, R.pairs(x, y, n, mode != "convolve"), ct, n, what, gain)
            print("%s: worst rel-L2 %.3e" % (what, worst))


@rows
def test_pairs_with_poisoned_gaps_and_rows(prec, m, cls):
    import test_gpu_pairs as PR
    PR.test_what_a_row_reads(prec, _real(prec, m, cls))
