"""EVERY pre-compiled periodogram kernel on the GPU against its reference: the registry of kernels_periodogram.hip is built
from the configuration list of csrc/wg_fused_cfg.hpp as the other ten are (test_gpu_fused_registry.py) -- 13 fp32 lines,
M = 2 ... 8192 points, and 12 fp64 lines, M = 2 ... 4096; a line of M points serves N = 2 M.

The pre-compiled kernel is the one that ran: the plan is committed, and set_periodogram_window called, inside an in-process
PFFT_JIT=0 block.  The list is tied to the code: the next power of two above it (fp32 M = 16384, fp64 M = 8192) is refused
as "register-resident" and M = 96 is refused naming PFFT_JIT=0, in the same block.

Nothing here is a second reference: the runner, the reference (test_gpu_stft._reference -> abs() ** 2 -> sums) and the
yardsticks of test_gpu_periodogram.py are imported and run unchanged -- guard bands, the write set, the unchanged input,
relative L1 per row within 2 tau + tau^2 + (A + 2) u, helpers.check_reference_rule on the square roots.  One reduced
scenario per case and BOTH extensions (the two cells of a line are two kernels), forward_scale off its default, uniform
signals in [-1, 1), one seed per case: three signals in rows of A = 3 frames, as many rows as put 3 R just above 2 FPW + 1
units, F = 3 (R - 1) + 1 so that the last row of every signal holds one frame, an odd hop near N / 4, an odd lead, a random
window, odd pitches.

The commit-compiled form, with the runtime compiler on: the same scenario at the two planner shapes M = 3 (one odd pass)
and M = 296 = 8 * 37, in both precisions.

The test prints one line per case; the worst per precision stand in DESIGN.md 3.1o.

No case is skipped."""
import contextlib
import re

import numpy as np
import pytest

import helpers as H
import test_gpu_periodogram as PG
from test_gpu_fused_registry import BEYOND, LINES, _env, _fpw, _mods, _odd, _odd_lead
from test_gpu_stft import _reference, _types

pytestmark = pytest.mark.gpu

NOT_A_POWER_OF_TWO = 96
JIT_SHAPES = [3, 296]
SCALE = 0.5
AVG = 3
_REL = re.compile(r"worst rel-L1 of a row ([0-9]\.[0-9]+e[-+][0-9]+)")


def _run(G, pf, torch, prec, n, rng, what):
    rt, ct = _types(prec)
    d = pf.real_descriptor(n, prec)
    d.forward_scale = SCALE
    plan = d.commit()
    w = rng.uniform(-1, 1, n).astype(rt)
    plan.set_periodogram_window(torch.from_numpy(w).cuda())
    fpw = _fpw(plan, n, n // 2)
    n_sig, hop, lead = 3, _odd(n // 4 + 1), min(_odd_lead(n), n - 1)
    n_rows = max(2, -(-(2 * fpw + 2) // n_sig))
    frames = AVG * (n_rows - 1) + 1
    for i, pad in enumerate(("zero", "reflect")):
        length = PG.in_length_for(n, hop, lead, pad, frames, shift=i)
        x = rng.uniform(-1, 1, (n_sig, length)).astype(rt)
        tag = "%s %s S=%d F=%d A=%d hop=%d lead=%d L=%d" % (what, pad, n_sig, frames, AVG, hop, lead, length)
        ref = PG.rows_of(np.abs(_reference(SCALE, x, w, n, hop, lead, pad, frames)) ** 2, AVG)
        got, _ = PG.run(G, torch, plan, n, x, hop, lead, pad, frames, AVG, tag, extra=2 + i)
        PG.check_rows(got, ref, prec, n, AVG, tag)


def _case(capsys, prec, m, env, seed):
    G, pf, torch = _mods()
    n = 2 * m
    with env:
        _run(G, pf, torch, prec, n, np.random.Generator(np.random.SFC64(seed)), "periodogram %s N=%d" % (prec, n))
    text = capsys.readouterr().out
    print(text, end="")
    errs = [float(v) for v in _REL.findall(text)]
    assert len(errs) == 2, (prec, n, "both extensions are measured")
    print("fused periodogram %s N=%d: worst rel-L1 of a row %.3e, %.1f times inside the bound" % (
        prec, n, max(errs), PG.bound(prec, AVG) / max(errs)))


REGISTRY_CASES = [(p, m) for p in ("f32", "f64") for m in LINES[p]]
JIT_CASES = [(p, m) for p in ("f32", "f64") for m in JIT_SHAPES]


@pytest.mark.parametrize("prec,m", REGISTRY_CASES)
def test_every_registered_line_against_its_reference(prec, m, capsys):
    """the pre-compiled kernels of (precision, line): committed and their window set with the runtime compiler off"""
    _case(capsys, prec, m, _env(PFFT_JIT="0"), 100019 * m + 7)


@pytest.mark.parametrize("prec,m", JIT_CASES)
def test_commit_compiled_shapes_against_their_reference(prec, m, capsys):
    """M = 3 (one odd pass) and M = 296 = 8 * 37: the form compiled at set_periodogram_window"""
    _case(capsys, prec, m, contextlib.nullcontext(), 100019 * m + 8)


def test_nothing_outside_the_list_resolves_without_the_compiler():
    """with the runtime compiler off, nothing behind or between the lines of the list commits or resolves"""
    G, pf, torch = _mods()

    def run(prec, n):
        pf.real_descriptor(n, prec).commit().set_periodogram_window(None)

    with _env(PFFT_JIT="0"):
        for prec in ("f32", "f64"):
            for m, reason in ((BEYOND[prec], "register-resident"), (NOT_A_POWER_OF_TWO, "PFFT_JIT=0")):
                with pytest.raises(pf.unsupported_configuration) as e:
                    run(prec, 2 * m)
                assert reason in str(e.value), (prec, 2 * m, str(e.value))
            run(prec, 2 * LINES[prec][-1])  # (the last line of the list does: the refusals are not the block's doing)
