"""EVERY pre-compiled inverse MDCT kernel on the GPU against its reference: the registry of kernels_imdct.hip is built from
the configuration list of csrc/wg_fused_cfg.hpp as the other nine are (test_gpu_fused_registry.py) -- 13 fp32 lines,
M = 2 ... 8192 points, and 12 fp64 lines, M = 2 ... 4096; a line of M points serves N = 2 M.

The pre-compiled kernel is the one that ran: the plan is committed, and set_imdct_window called, inside an in-process
PFFT_JIT=0 block.  The list is tied to the code: the next power of two above it (fp32 M = 16384, fp64 M = 8192) is refused
as "register-resident" and M = 96 is refused naming PFFT_JIT=0, in the same block.

Nothing here is a second reference: the runner (_imdct), the NumPy reference of imdct_ref.py and the _check of
test_gpu_imdct.py are imported and run unchanged -- guard bands, the write set, the unchanged input, every signal with
helpers.REL_L2_TOL and helpers.check_reference_rule(n = N).  One reduced scenario per case, scales off their defaults,
uniform coefficients in [-1, 1), one seed per case: three signals of just above (2 FPW + 1) / 3 frames each (a halo, two
full steps and a ragged one per chunk cut), an odd lead, an out_length that is no multiple of N, a random window in
[0.25, 1] (not symmetric), odd pitches, the plan's own chunk and a chunk of 2 frames, whose outputs hold the same bits.

The commit-compiled form, with the runtime compiler on: the same scenario at the two planner shapes M = 3 (one odd pass:
the middle item) and M = 296 = 8 * 37, in both precisions.

The test prints one line per case; the worst per precision stand in DESIGN.md 3.1n.

No case is skipped."""
import contextlib
import re

import numpy as np
import pytest

import helpers as H
import test_gpu_imdct as IM
from imdct_ref import imdct_reference
from test_gpu_fused_registry import BEYOND, LINES, _env, _fpw, _mods

pytestmark = pytest.mark.gpu

NOT_A_POWER_OF_TWO = 96
JIT_SHAPES = [3, 296]
SCALES = (0.5, 0.25)
_REL = re.compile(r"worst rel-L2 ([0-9]\.[0-9]+e[-+][0-9]+)")


def _run(G, pf, torch, prec, n, rng, what):
    rt, ct = IM._types(prec)
    d = pf.real_descriptor(n, prec)
    d.forward_scale, d.backward_scale = SCALES
    plan = d.commit()
    w = rng.uniform(0.25, 1.0, 2 * n).astype(rt)
    plan.set_imdct_window(torch.from_numpy(w).cuda())
    fpw = _fpw(plan, n, n // 2)
    n_sig, lead = 3, n + 1
    frames = max(3, -(-(2 * fpw + 2) // n_sig))
    length = (frames - 1) * n - lead + n // 2 + 1  # the last frame contributes N / 2 + 1 samples, the first starts at -lead
    coeff = rng.uniform(-1, 1, (n_sig, frames, n)).astype(rt)
    tag = "%s S=%d F=%d lead=%d L=%d" % (what, n_sig, frames, lead, length)
    ref = SCALES[1] * imdct_reference(coeff, w, n, lead, length)
    got, first, gin = IM._imdct(G, torch, plan, coeff, n, lead, length, 0, tag)
    IM._check(got, ref, ct, n, tag)
    _, other, _ = IM._imdct(G, torch, plan, coeff, n, lead, length, 2, tag + " chunk=2", gin=gin)
    H.check_same_bits(first, other, what=tag + ": chunk_frames 2 against 0")


def _case(capsys, prec, m, env, seed):
    G, pf, torch = _mods()
    n = 2 * m
    with env:
        _run(G, pf, torch, prec, n, np.random.Generator(np.random.SFC64(seed)), "imdct %s N=%d" % (prec, n))
    text = capsys.readouterr().out
    print(text, end="")
    errs = [float(v) for v in _REL.findall(text)]
    assert errs, (prec, n, "no signal was measured")
    tol = H.REL_L2_TOL[np.dtype(np.complex64 if prec == "f32" else np.complex128)]
    print("fused imdct %s N=%d: worst rel-L2 %.3e, %.1f times inside REL_L2_TOL" % (prec, n, max(errs), tol / max(errs)))


REGISTRY_CASES = [(p, m) for p in ("f32", "f64") for m in LINES[p]]
JIT_CASES = [(p, m) for p in ("f32", "f64") for m in JIT_SHAPES]


@pytest.mark.parametrize("prec,m", REGISTRY_CASES)
def test_every_registered_line_against_its_reference(prec, m, capsys):
    """the pre-compiled kernel of (precision, line): committed and its window set with the runtime compiler off"""
    _case(capsys, prec, m, _env(PFFT_JIT="0"), 100019 * m + 5)


@pytest.mark.parametrize("prec,m", JIT_CASES)
def test_commit_compiled_shapes_against_their_reference(prec, m, capsys):
    """M = 3 (one odd pass) and M = 296 = 8 * 37 (a prime's pass decides the lanes): the form compiled at set_imdct_window"""
    _case(capsys, prec, m, contextlib.nullcontext(), 100019 * m + 6)


def test_nothing_outside_the_list_resolves_without_the_compiler():
    """with the runtime compiler off, nothing behind or between the lines of the list commits or resolves"""
    G, pf, torch = _mods()

    def run(prec, n):
        pf.real_descriptor(n, prec).commit().set_imdct_window(None)

    with _env(PFFT_JIT="0"):
        for prec in ("f32", "f64"):
            for m, reason in ((BEYOND[prec], "register-resident"), (NOT_A_POWER_OF_TWO, "PFFT_JIT=0")):
                with pytest.raises(pf.unsupported_configuration) as e:
                    run(prec, 2 * m)
                assert reason in str(e.value), (prec, 2 * m, str(e.value))
            run(prec, 2 * LINES[prec][-1])  # (the last line of the list does: the refusals are not the block's doing)
