"""EVERY pre-compiled DCT-IV / MDCT kernel on the GPU against its reference: the registry of kernels_dct4.hip is built
from the configuration list of csrc/wg_fused_cfg.hpp as the other eight are (test_gpu_fused_registry.py) -- 13 fp32
lines, M = 2 ... 8192 points, and 12 fp64 lines, M = 2 ... 4096; a line of M points serves N = 2 M -- and every entry
carries two cells: 25 lines x {dct4, mdct}.

The pre-compiled kernel is the one that ran: the plan is committed, and prepare_dct4 / set_mdct_window called, inside an
in-process PFFT_JIT=0 block.  The list is tied to the code: the next power of two above it (fp32 M = 16384, fp64 M = 8192)
is refused as "register-resident" and M = 96 is refused naming PFFT_JIT=0, in the same block.

Nothing here is a second reference: the runners (_dct4, _mdct), the NumPy references of dct4_ref.py and the _check of
test_gpu_dct4.py are imported and run unchanged -- guard bands, the write set, the unchanged input, every row with
helpers.REL_L2_TOL and helpers.check_reference_rule(n = N).  One reduced scenario per case, scales off their defaults,
uniform data in [-1, 1), one seed per case:
  dct4   2 FPW + 1 rows (two full groups and a ragged one), forward out of place (base pointers one scalar off their
         alignment) and inverse in place, odd pitches
  mdct   three signals whose (signal, frame) rows number just above 2 FPW + 1, an odd lead, an in_length that is no
         multiple of N, frames cut at both ends, a random window in [0.25, 1] (not symmetric), odd pitches

The commit-compiled forms, with the runtime compiler on: the same scenarios at the two planner shapes M = 3 (one odd pass:
the middle item) and M = 296 = 8 * 37, in both precisions.

Measured on the MI355X, relative L2 of the worst row of a case (the test prints one line per case), smallest ... largest
over the lines and the two commit-compiled shapes of a cell and precision:
  dct4   fp32 1.1e-07 (N = 8) ... 2.0e-07 (N = 6),   fp64 3.5e-16 (N = 64) ... 4.5e-16 (N = 16)
  mdct   fp32 1.2e-07 (N = 64) ... 2.3e-07 (N = 4),  fp64 3.4e-16 (N = 32) ... 9.5e-16 (N = 4)
Per line, dct4 | mdct: fp32 N=4 1.5e-07 | 2.3e-07, 8 1.1e-07 | 1.4e-07, 16 1.3e-07 | 1.7e-07, 32 1.3e-07 | 1.5e-07, 64 1.3e-07 |
1.2e-07, 128 1.1e-07 | 1.2e-07, 256 1.2e-07 | 1.3e-07, 512 1.2e-07 | 1.3e-07, 1024 1.2e-07 | 1.3e-07, 2048 1.2e-07 | 1.3e-07, 4096
1.3e-07 | 1.3e-07, 8192 1.3e-07 | 1.4e-07, 16384 1.4e-07 | 1.4e-07, 6 2.0e-07 | 1.7e-07, 592 1.3e-07 | 1.4e-07; fp64 N=4 3.9e-16 |
9.5e-16, 8 3.7e-16 | 5.1e-16, 16 4.5e-16 | 3.9e-16, 32 3.7e-16 | 3.4e-16, 64 3.5e-16 | 3.6e-16, 128 3.6e-16 | 3.6e-16, 256 3.5e-16 |
3.7e-16, 512 3.6e-16 | 4.0e-16, 1024 3.9e-16 | 4.1e-16, 2048 3.9e-16 | 4.0e-16, 4096 4.2e-16 | 4.2e-16, 8192 4.4e-16 | 4.5e-16, 6
4.1e-16 | 7.1e-16, 592 3.9e-16 | 3.9e-16.  The closest case is 5.3 times inside REL_L2_TOL (mdct, fp64, N = 4; fp32: 8.6 times,
mdct, N = 4): no line within a factor 2 of it.

No case is skipped."""
import contextlib
import re

import numpy as np
import pytest

import helpers as H
import test_gpu_dct4 as D4
from dct4_ref import dct4_reference, frames_of, mdct_reference
from test_gpu_fused_registry import BEYOND, LINES, _env, _fpw, _mods

pytestmark = pytest.mark.gpu

NOT_A_POWER_OF_TWO = 96
JIT_SHAPES = [3, 296]
SCALES = (0.5, 0.25)


def _plan(pf, prec, n):
    d = pf.real_descriptor(n, prec)
    d.forward_scale, d.backward_scale = SCALES
    return d.commit()


def _dct4(G, pf, torch, prec, n, rng, what):
    rt, ct = D4._types(prec)
    plan = _plan(pf, prec, n)
    plan.prepare_dct4()
    fpw = _fpw(plan, n, n // 2)
    rows = 2 * fpw + 1
    x = rng.uniform(-1, 1, (rows, n)).astype(rt)
    ref = dct4_reference(x)
    for inverse, in_place, guard in ((False, False, (65, 64)), (True, True, None)):
        tag = "%s rows=%d %s %s" % (what, rows, "in place" if in_place else "out of place", "inverse" if inverse else "forward")
        y = D4._dct4(G, torch, plan, inverse, x, in_place, tag, guard)
        D4._check(y, SCALES[1 if inverse else 0] * ref, ct, n, tag)


def _mdct(G, pf, torch, prec, n, rng, what):
    rt, ct = D4._types(prec)
    plan = _plan(pf, prec, n)
    w = rng.uniform(0.25, 1.0, 2 * n).astype(rt)
    plan.set_mdct_window(torch.from_numpy(w).cuda())
    fpw = _fpw(plan, n, n // 2)
    n_sig, lead = 3, n + 1
    frames = max(3, -(-(2 * fpw + 2) // n_sig))
    length = (frames - 1) * n - lead + n // 2 + 1  # the last frame holds N / 2 + 1 samples, the first starts at -lead
    x = rng.uniform(-1, 1, (n_sig, length)).astype(rt)
    tag = "%s S=%d L=%d lead=%d F=%d" % (what, n_sig, length, lead, frames)
    got = D4._mdct(G, torch, plan, x, n, lead, frames, tag)
    ref = SCALES[0] * mdct_reference(frames_of(x, n, lead, frames, w))
    D4._check(got.reshape(-1, n), ref.reshape(-1, n), ct, n, tag)


VERBS = {"dct4": _dct4, "mdct": _mdct}
_REL = re.compile(r"worst rel-L2 ([0-9]\.[0-9]+e[-+][0-9]+)")


def _case(capsys, verb, prec, m, env, seed):
    G, pf, torch = _mods()
    n = 2 * m
    with env:
        VERBS[verb](G, pf, torch, prec, n, np.random.Generator(np.random.SFC64(seed)), "%s %s N=%d" % (verb, prec, n))
    text = capsys.readouterr().out
    print(text, end="")
    errs = [float(v) for v in _REL.findall(text)]
    assert errs, (verb, prec, n, "no row was measured")
    tol = H.REL_L2_TOL[np.dtype(np.complex64 if prec == "f32" else np.complex128)]
    print("fused %s %s N=%d: worst rel-L2 %.3e, %.1f times inside REL_L2_TOL" % (verb, prec, n, max(errs), tol / max(errs)))


REGISTRY_CASES = [(v, p, m) for v in VERBS for p in ("f32", "f64") for m in LINES[p]]
JIT_CASES = [(v, p, m) for v in VERBS for p in ("f32", "f64") for m in JIT_SHAPES]


@pytest.mark.parametrize("verb,prec,m", REGISTRY_CASES)
def test_every_registered_line_against_its_reference(verb, prec, m, capsys):
    """the pre-compiled kernel of (cell, precision, line): committed and prepared with the runtime compiler off"""
    _case(capsys, verb, prec, m, _env(PFFT_JIT="0"), 100019 * m + len(verb))


@pytest.mark.parametrize("verb,prec,m", JIT_CASES)
def test_commit_compiled_shapes_against_their_reference(verb, prec, m, capsys):
    """M = 3 (one odd pass) and M = 296 = 8 * 37 (a prime's pass decides the lanes): the forms compiled at prepare"""
    _case(capsys, verb, prec, m, contextlib.nullcontext(), 100019 * m + len(verb) + 1)


@pytest.mark.parametrize("prepare", ("prepare_dct4", "set_mdct_window"))
def test_nothing_outside_the_list_prepares_without_the_compiler(prepare):
    """with the runtime compiler off, nothing behind or between the lines of the list commits or prepares"""
    G, pf, torch = _mods()

    def run(prec, n):
        plan = pf.real_descriptor(n, prec).commit()
        plan.prepare_dct4() if prepare == "prepare_dct4" else plan.set_mdct_window(None)

    with _env(PFFT_JIT="0"):
        for prec in ("f32", "f64"):
            for m, reason in ((BEYOND[prec], "register-resident"), (NOT_A_POWER_OF_TWO, "PFFT_JIT=0")):
                with pytest.raises(pf.unsupported_configuration) as e:
                    run(prec, 2 * m)
                assert reason in str(e.value), (prepare, prec, 2 * m, str(e.value))
            run(prec, 2 * LINES[prec][-1])  # (the last line of the list does: the refusals are not the block's doing)
