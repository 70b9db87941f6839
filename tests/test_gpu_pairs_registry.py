"""EVERY pre-compiled pair kernel on the GPU against its reference: the registry of kernels_pairs.hip is built from the
configuration list of csrc/wg_fused_cfg.hpp as the other eleven are (test_gpu_fused_registry.py) -- 13 fp32 lines, M = 2 ...
8192 points, and 12 fp64 lines, M = 2 ... 4096; a line of M points serves N = 2 M.  Both cells of a line run: [0] the
product (convolve_pairs), [1] the conjugate product (correlate_pairs), and the latter once more with a floor.

The pre-compiled kernel is the one that ran: the plan is committed, and prepare_pairs called, inside an in-process
PFFT_JIT=0 block.  The list is tied to the code: the next power of two above it (fp32 M = 16384, fp64 M = 8192) is refused
as "register-resident" and M = 96 is refused naming PFFT_JIT=0, in the same block.

Nothing here is a second reference: the runner, the reference (tests/pairs_ref.py) and the yardsticks of
test_gpu_pairs.py are imported and run unchanged -- guard bands, the write set, the unchanged inputs, relative L2 per row
within REL_L2_TOL and helpers.check_reference_rule, (kappa + 1) tau with a floor.  One reduced scenario per case: 2 FPW + 1
rows, x of N - 1 scalars and y of N / 2 + 1, all N result scalars, odd pitches, scales off their defaults, one seed per
case.

The commit-compiled form, with the runtime compiler on: the same scenario at the two planner shapes M = 3 (one odd pass)
and M = 296 = 8 * 37, in both precisions.

No case is skipped."""
import contextlib

import numpy as np
import pytest

import helpers as H
import pairs_ref as R
import test_gpu_pairs as P
from test_gpu_fused_registry import BEYOND, LINES, _env, _fpw, _mods

pytestmark = pytest.mark.gpu

NOT_A_POWER_OF_TWO = 96
JIT_SHAPES = [3, 296]


def _case(prec, m, env, seed):
    G, pf, torch = _mods()
    rt, ct = P._types(prec)
    n = 2 * m
    scales = (0.5, 2.0 / n)
    with env:
        plan = P.plan_of(pf, n, prec, scales)
    fpw = _fpw(plan, n, m)
    rows, lx, ly = 2 * fpw + 1, n - 1, n // 2 + 1
    rng = np.random.Generator(np.random.SFC64(seed))
    x, y = P.draw_rows(rng, rows, lx, ly, n, rt)
    p = R.cross_spectrum(x, y, n, True)
    floor = float(rt(np.median(np.abs(p))))
    kappa = P.spectrum_norm(p, n) / (floor * P.spectrum_norm(R.phat_weight(p, floor), n))
    worst = []
    for mode in P.MODES:
        what = ("registry", prec, n, mode, "rows %d" % rows)
        ref = R.pairs(x, y, n, mode != "convolve", None, scales[0], scales[1], floor if mode == "phat" else None)
        got, _ = P.run(G, torch, plan, x, y, mode, n, P.pitches_of(n, m % 3), what, floor=floor if mode == "phat" else None)
        if mode == "phat":
            worst.append(P.check_phat(got, ref, kappa, ct, n, what) * (float(kappa.max()) + 1) * H.REL_L2_TOL[np.dtype(ct)])
        else:
            worst.append(P.check_plain(got, ref, ct, n, what, P.rule_gain(x, y, scales[0] * scales[0] * scales[1])))
    print("fused pairs %s N=%d fpw %d: worst rel-L2 of a row: convolve %.3e, correlate %.3e (%.1f times inside the bound); "
          "with a floor at most %.3e" % (prec, n, fpw, worst[0], worst[1], H.REL_L2_TOL[np.dtype(ct)] / max(worst[:2]), worst[2]))


REGISTRY_CASES = [(p, m) for p in ("f32", "f64") for m in LINES[p]]
JIT_CASES = [(p, m) for p in ("f32", "f64") for m in JIT_SHAPES]


@pytest.mark.parametrize("prec,m", REGISTRY_CASES)
def test_every_registered_line_against_its_reference(prec, m):
    """the pre-compiled kernels of (precision, line): committed and prepared with the runtime compiler off"""
    _case(prec, m, _env(PFFT_JIT="0"), 100019 * m + 11)


@pytest.mark.parametrize("prec,m", JIT_CASES)
def test_commit_compiled_shapes_against_their_reference(prec, m):
    """M = 3 (one odd pass) and M = 296 = 8 * 37: the form compiled at prepare_pairs"""
    _case(prec, m, contextlib.nullcontext(), 100019 * m + 12)


def test_nothing_outside_the_list_resolves_without_the_compiler():
    """with the runtime compiler off, nothing behind or between the lines of the list commits or resolves"""
    G, pf, torch = _mods()

    def run(prec, n):
        pf.real_descriptor(n, prec).commit().prepare_pairs()

    with _env(PFFT_JIT="0"):
        for prec in ("f32", "f64"):
            for m, reason in ((BEYOND[prec], "register-resident"), (NOT_A_POWER_OF_TWO, "PFFT_JIT=0")):
                with pytest.raises(pf.unsupported_configuration) as e:
                    run(prec, 2 * m)
                assert reason in str(e.value), (prec, 2 * m, str(e.value))
            run(prec, 2 * LINES[prec][-1])  # (the last line of the list does: the refusals are not the block's doing)
