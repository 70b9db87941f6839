"""EVERY pre-compiled fused kernel on the GPU against its reference: the eight registries of the fused verbs -- R2C / C2R
(kernels_real.hip), complex convolve / correlate (_conv) and filter (_ols), real convolve / correlate (_rconv) and filter
(_rols), stft, istft and dct -- are built from the one configuration list of csrc/wg_fused_cfg.hpp: 13 fp32 lines,
M = 2 ... 8192 points, and 12 fp64 lines, M = 2 ... 4096 (a line of M points serves N = 2 M of the real-data verbs).  The
per-verb modules run one length per kernel shape; this one runs every line of every registry, 200 entries, so that a
verb body that is wrong at one combination of TPF, FPW, STAGED, NP, TWM and the LDS padding cannot go unseen.

The pre-compiled kernel is the one that ran: every plan is committed, and every preparing call (set_filter,
set_filter_taps, set_window, set_synthesis_window, prepare_dct) made, inside an in-process PFFT_JIT=0 block
(test_gpu_write_sets._env; the library reads the environment at those calls, and the fused kernel is chosen there).  With
the runtime compiler off a call that succeeds can only have taken the registry entry, and a refusal fails the test.
The list is tied to the code: per verb, the next power of two above it (fp32 M = 16384, fp64 M = 8192) is refused as
"register-resident" and M = 96 is refused naming PFFT_JIT=0, in the same block.  No verb's limits exclude a listed line:
the complex filter runs at N = 2 with K = 2 taps (hop 1), the real filter at N = 4 with K = N - 2 = 2 (hop 2).

Nothing here is a second reference: the runners (_execute, _run, _filter, _stft, _istft, _dct), the double-precision
NumPy references and the _check of every verb's own module are imported and run unchanged -- guard bands, the write
set, the unchanged input, every row with the project's two yardsticks (relative L2 within helpers.REL_L2_TOL,
helpers.check_reference_rule with n = N).  One reduced scenario per case: 2 FPW + 1 rows (two full groups and a ragged
one), odd pitches or offsets, scales off their defaults, uniform data in [-1, 1), one seed per case:
  real     forward and backward, out of place (offsets 5 / 2) and in place (the padded pair, offsets 6 / 3); a real
           descriptor admits the pitches N and N + 2 only, so odd offsets stand in for odd pitches here and in rconv
  conv     convolve and correlate, a filter per row, out of place (pitches N + 5 / N + 3, made odd) and in place
  filter   K = ceil(N / 4) + 1 taps (at most N; the real one at most N - 2), several signals whose (signal, segment)
           rows number just above 2 FPW + 1, a filter each, a ragged last segment, the output shorter than the input,
           both modes, odd pitches
  rconv    convolve and correlate, a filter per row, packed rows at an odd offset and the padded pair, out of place
           and in == out
  stft     zeros and reflection, three signals, odd hop, odd lead, a random window in [-1, 1] (not symmetric)
  istft    plain (random window) and envelope-normalised (random window in [0.5, 1]), hop N / 4, odd lead, two signals
           of FPW + 1 frames, all chunk lengths of test_gpu_istft._istft compared bit for bit
  dct      types 2 and 3, out of place and in place, odd pitches

The commit-compiled forms, with the runtime compiler on: the same scenarios at the two planner shapes that reached only
R2C / C2R so far -- a one-pass odd length (M = 3: N = 6 real, N = 3 complex) and a half length with a prime factor 37
(M = 296 = 8 * 37: "as many lanes as the prime's pass has butterflies") -- in both precisions, the plan asserted to be
the one-kernel work-group tier through plan.info().

Measured on the MI355X, relative L2 of the worst row of a case (the test prints one line per case), smallest ... largest
over the lines and the two commit-compiled shapes of a verb and precision, N in the verb's own count:
  real     fp32 9.4e-08 (N = 4) ... 1.6e-07 (N = 6),     fp64 1.0e-16 (N = 4) ... 3.6e-16 (N = 8192)
  conv     fp32 1.2e-07 (N = 2) ... 2.0e-07 (N = 8192),  fp64 2.5e-16 (N = 2) ... 4.7e-16 (N = 4096)
  filter   fp32 1.1e-07 (N = 4) ... 2.4e-07 (N = 8192),  fp64 2.4e-16 (N = 4) ... 5.7e-16 (N = 4096)
  rconv    fp32 1.7e-07 (N = 256) ... 2.4e-07 (N = 6),   fp64 3.2e-16 (N = 4) ... 5.5e-16 (N = 16)
  rfilter  fp32 1.2e-07 (N = 4) ... 2.6e-07 (N = 16384), fp64 3.1e-16 (N = 4) ... 5.8e-16 (N = 6)
  stft     fp32 4.5e-08 (N = 4) ... 1.4e-07 (N = 16384), fp64 3.5e-17 (N = 4) ... 3.7e-16 (N = 8192)
  istft    fp32 6.6e-08 (N = 4) ... 1.5e-07 (N = 16384), fp64 6.1e-17 (N = 4) ... 3.8e-16 (N = 8192)
  dct      fp32 1.2e-07 (N = 128) ... 1.9e-07 (N = 6),   fp64 3.1e-16 (N = 4) ... 4.2e-16 (N = 6)
The line no per-verb module ran, fp32 M = 1024: real 1.2e-07, conv 1.7e-07, filter 1.9e-07, rconv 1.8e-07, rfilter 2.2e-07,
stft 1.2e-07, istft 1.3e-07, dct 1.3e-07.  The closest case is 7.8 times inside REL_L2_TOL (rfilter, fp32, N = 16384; fp64:
8.6 times, rfilter, N = 6): no line within a factor 2 of it, the margin of the per-verb modules.

No case is skipped."""
import contextlib
import re

import numpy as np
import pytest

import helpers as H
import test_gpu_conv as CONV
import test_gpu_dct as DCT
import test_gpu_filter as OLS
import test_gpu_istft as ISTFT
import test_gpu_rconv as RCONV
import test_gpu_real as REAL
import test_gpu_rfilter as ROLS
import test_gpu_stft as STFT
from dct_ref import dct_reference
from test_gpu_write_sets import _env

pytestmark = pytest.mark.gpu

# the configuration list of csrc/wg_fused_cfg.hpp in points M, and the first power of two behind it
LINES = {"f32": [2 << i for i in range(13)], "f64": [2 << i for i in range(12)]}
BEYOND = {"f32": 16384, "f64": 8192}
NOT_A_POWER_OF_TWO = 96
# the planner shapes of the commit-compiled forms, in points M
JIT_SHAPES = [3, 296]
SCALES = (0.5, 0.25)  # forward_scale, backward_scale (* N where the verb's result carries a factor N)


def _mods():
    import gpu_utils as G
    import portfft_amd as pf
    return G, pf, G.torch_mod()


def _odd(v):
    return v | 1


def _fpw(plan, n, points, tiers=(1,)):
    """the plan is one kernel of the work-group tier for `points` points; returns its transforms per work-group"""
    info = plan.info()
    dim = info.dims[0]
    assert dim.length == n and dim.tier in tiers and tuple(info.launches) == (1, 1), (n, dim.length, dim.tier, tuple(info.launches))
    assert int(np.prod(dim.factors[:dim.n_factors])) == points, (n, list(dim.factors[:dim.n_factors]))
    return max(1, dim.ffts_per_workgroup)


def _odd_lead(n):
    m = n // 2
    return m - 1 if (m - 1) % 2 else m + 1


# ---------------------------------------------------------------------------------------------------------------------
# one reduced scenario per verb.  Each function is entered inside the PFFT_JIT=0 block (or with the compiler on) and
# commits, prepares and launches there; `what` names the case in every message.

def _real(G, pf, torch, prec, n, rng, what):
    rt, ct = REAL._types(prec)
    m = n // 2
    fpw = _fpw(REAL._desc(pf, n, prec, 1, False, (0, 0), (1.0, 1.0)).commit(), n, m)
    batch = 2 * fpw + 1
    x = rng.uniform(-1, 1, (batch, n)).astype(rt)
    X = np.fft.rfft(x.astype(np.float64), axis=1)
    Xin = X.astype(ct)
    Xclean = Xin.astype(np.complex128)
    Xclean[:, 0] = Xclean[:, 0].real
    Xclean[:, m] = Xclean[:, m].real
    xback = n * np.fft.irfft(Xclean, n, axis=1)
    scales = (SCALES[0], SCALES[1] / n)
    for in_place, offsets in ((False, (5, 2)), (True, (6, 3))):
        d = REAL._desc(pf, n, prec, batch, in_place, offsets, scales)
        plan = d.commit()
        tag = what + (batch, "ip" if in_place else "oop", offsets)
        y, _ = REAL._execute(pf, torch, d, plan, pf.direction.FORWARD, x)
        REAL._check(y, scales[0] * X, ct, n, tag + ("fwd",))
        assert np.all(y[:, 0].imag == 0) and np.all(y[:, m].imag == 0), (tag, "bins 0 and N/2 must be real")
        back, _ = REAL._execute(pf, torch, d, plan, pf.direction.BACKWARD, Xin)
        REAL._check(back, scales[1] * xback, ct, n, tag + ("bwd",))


def _conv(G, pf, torch, prec, n, rng, what):
    ct = CONV._ct(prec)
    fpw = _fpw(CONV._desc(pf, n, prec).commit(), n, n, tiers=(0, 1))
    batch = 2 * fpw + 1
    x, h = CONV._data(rng, batch, n, ct), CONV._data(rng, batch, n, ct)
    scales = (SCALES[0], SCALES[1] / n)
    for dist, off, in_place, guard in (((_odd(n + 4), _odd(n + 2)), (5, 2), False, (65, 63)),
                                       ((_odd(n + 4), _odd(n + 4)), (3, 3), True, None)):
        d = CONV._desc(pf, n, prec, batch, in_place, dist, off, scales)
        plan = CONV._commit(pf, torch, d, h)
        for correlate in (False, True):
            CONV._run(G, pf, torch, d, x, h, plan, correlate, what + (batch, "ip" if in_place else "oop", dist), guard)


def _rconv(G, pf, torch, prec, n, rng, what):
    rt, ct = RCONV._types(prec)
    fpw = _fpw(RCONV._desc(pf, n, prec).commit(), n, n // 2)
    batch = 2 * fpw + 1
    x = rng.uniform(-1, 1, (batch, n)).astype(rt)
    h = RCONV._spectra(rng, batch, n, ct)
    scales = (SCALES[0], SCALES[1] / n)
    for padded, offset, guard, name in ((False, 5, (65, 63), "packed, odd offset"), (True, 3, None, "padded rows")):
        d = RCONV._desc(pf, n, prec, batch, padded, offset, scales)
        plan = RCONV._commit(pf, torch, d, h)
        for correlate in (False, True):
            for same in (False, True):
                RCONV._run(G, pf, torch, d, x, h, plan, correlate, what + (batch, name), same, guard)


def _filter_geometry(hop, k, fpw):
    """(signals, in_length, out_length): three segments (or as many as hold K outputs), the last one ragged, the output
    three samples shorter than the input, and (signal, segment) rows just above 2 FPW + 1"""
    out_length = max(2 * hop + (hop + 1) // 2, k)
    segments = -(-out_length // hop)
    return max(2, -(-(2 * fpw + 2) // segments)), out_length + 3, out_length


def _ols(G, pf, torch, prec, n, rng, what):
    ct = OLS._ct(prec)
    d = pf.convolution_descriptor([n], prec)
    d.forward_scale, d.backward_scale = SCALES[0], SCALES[1] / n
    plan = d.commit()
    fpw = _fpw(plan, n, n, tiers=(0, 1))
    c = d.forward_scale * d.backward_scale * n
    k = min(-(-n // 4) + 1, n)
    for correlate in (False, True):
        ns, in_length, out_length = _filter_geometry(n - k + 1, k, fpw)
        x = OLS._data(rng, ns, in_length, ct)
        h = OLS._data(rng, ns, k, ct, 1.0 / np.sqrt(k))
        plan.set_filter_taps(torch.from_numpy(h).cuda())
        OLS._filter(G, torch, plan, c, n, x, h, out_length, correlate,
                    what + (k, "corr" if correlate else "conv", ns, in_length, out_length),
                    pads=(3 + in_length % 2, 5 + out_length % 2), guard=(65, 63) if correlate else None)


def _rols(G, pf, torch, prec, n, rng, what):
    rt, ct = ROLS._types(prec)
    d = pf.real_convolution_descriptor(n, prec)
    d.forward_scale, d.backward_scale = SCALES[0], SCALES[1] / n
    plan = d.commit()
    fpw = _fpw(plan, n, n // 2)
    c = d.forward_scale * d.backward_scale * n
    k = min(-(-n // 4) + 1, n - 2)
    for correlate in (False, True):
        ns, in_length, out_length = _filter_geometry(ROLS._hop(n, k, correlate), k, fpw)
        x = rng.uniform(-1, 1, (ns, in_length)).astype(rt)
        h = (rng.uniform(-1, 1, (ns, k)) / np.sqrt(k)).astype(rt)
        plan.set_filter_taps(torch.from_numpy(h).cuda())
        ROLS._filter(G, torch, plan, c, n, x, h, out_length, correlate,
                     what + (k, "corr" if correlate else "conv", ns, in_length, out_length),
                     guard=(65, 63) if correlate else None)


def _stft(G, pf, torch, prec, n, rng, what):
    rt, ct = STFT._types(prec)
    m = n // 2
    d = pf.real_descriptor(n, prec)
    d.forward_scale = SCALES[0]
    plan = d.commit()
    fpw = _fpw(plan, n, m)
    w = rng.uniform(-1, 1, n).astype(rt)
    plan.set_window(torch.from_numpy(w).cuda())
    ns, hop, lead = 3, _odd(n // 4 + 1), _odd_lead(n)
    frames = max(2, -(-(2 * fpw + 1) // ns))
    for i, pad in enumerate(("zero", "reflect")):
        if pad == "zero":  # the first frames reach in front of the signal, the last one holds M + 1 samples of it
            length = max((frames - 1) * hop - lead + m + 1, 1)
        else:  # the last frame ends at the mirror image of sample L - 1 - lead, or the signal is as short as lead admits
            length = max((frames - 1) * hop + n - 2 * lead, lead + 1)
        assert STFT._max_frames(n, length, hop, lead, pad) >= frames, (n, length, hop, lead, pad, frames)
        x = rng.uniform(-1, 1, (ns, length)).astype(rt)
        STFT._stft(G, torch, plan, d.forward_scale, n, x, w, hop, lead, pad, frames,
                   what + (pad, "hop", hop, "lead", lead, "in", length, "frames", frames),
                   guard=(65, 63) if i else None, extra=2 + i)


def _istft(G, pf, torch, prec, n, rng, what):
    rt, ct = ISTFT._types(prec)
    m = n // 2
    d = pf.real_descriptor(n, prec)
    d.backward_scale = SCALES[1]
    plan = d.commit()
    fpw = _fpw(plan, n, m)
    ns, frames, hop, lead = 2, fpw + 1, max(1, n // 4), _odd_lead(n)
    top = (frames - 1) * hop + n - lead
    olen = top - 3 if top - 3 >= 1 and top - 3 + lead > (frames - 1) * hop else top
    y = ISTFT._bins(rng, ns, frames, m, ct)
    tag = what + ("hop", hop, "lead", lead, "frames", frames, "out", olen)
    w = rng.uniform(-1, 1, n).astype(rt)
    ISTFT._set(plan, torch, w)
    ISTFT._istft(G, torch, plan, d.backward_scale, fpw, n, y, w, hop, lead, False, olen, tag + ("plain",), (65, 63), 2)
    positive = rng.uniform(0.5, 1, n).astype(rt)
    ISTFT._set(plan, torch, positive)
    ISTFT._istft(G, torch, plan, d.backward_scale, fpw, n, y, positive, hop, lead, True, olen, tag + ("normalize",), None, 3)


def _dct(G, pf, torch, prec, n, rng, what):
    rt, ct = DCT._types(prec)
    d = pf.real_descriptor(n, prec)
    d.forward_scale, d.backward_scale = SCALES
    plan = d.commit()
    plan.prepare_dct()
    fpw = _fpw(plan, n, n // 2)
    rows = 2 * fpw + 1
    x = rng.uniform(-1, 1, (rows, n)).astype(rt)
    for in_place, guard in ((False, (65, 64)), (True, None)):
        for kind, scale in ((2, d.forward_scale), (3, d.backward_scale)):
            tag = "%s rows=%d %s type %d" % (what, rows, "in place" if in_place else "out of place", kind)
            y = DCT._dct(G, torch, plan, kind, x, in_place, tag, guard)
            DCT._check(y, scale * dct_reference(x, kind), ct, n, tag)


# verb -> (scenario, real-data verb: a line of M points serves N = 2 M)
VERBS = {"real": (_real, True), "conv": (_conv, False), "filter": (_ols, False), "rconv": (_rconv, True),
         "rfilter": (_rols, True), "stft": (_stft, True), "istft": (_istft, True), "dct": (_dct, True)}

_REL = re.compile(r"worst rel-L2 ([0-9]\.[0-9]+e[-+][0-9]+)")


def _case(capsys, verb, prec, m, env, seed):
    G, pf, torch = _mods()
    scenario, real = VERBS[verb]
    n = 2 * m if real else m
    with env:
        scenario(G, pf, torch, prec, n, np.random.Generator(np.random.SFC64(seed)), (verb, prec, n))
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
    """the pre-compiled kernel of (verb, precision, line): committed and prepared with the runtime compiler off"""
    _case(capsys, verb, prec, m, _env(PFFT_JIT="0"), 100003 * m + len(verb))


@pytest.mark.parametrize("verb,prec,m", JIT_CASES)
def test_commit_compiled_shapes_against_their_reference(verb, prec, m, capsys):
    """M = 3 (one odd pass) and M = 296 = 8 * 37 (a prime's pass decides the lanes): the forms compiled at commit"""
    _case(capsys, verb, prec, m, contextlib.nullcontext(), 100003 * m + len(verb) + 1)


def _commit_and_prepare(pf, verb, prec, n):
    if verb in ("conv", "filter"):
        return pf.convolution_descriptor([n], prec).commit()
    if verb in ("rconv", "rfilter"):
        return pf.real_convolution_descriptor(n, prec).commit()
    plan = pf.real_descriptor(n, prec).commit()
    if verb == "stft":
        plan.set_window(None)
    elif verb == "istft":
        plan.set_synthesis_window(None)
    elif verb == "dct":
        plan.prepare_dct()
    return plan


@pytest.mark.parametrize("verb", list(VERBS))
def test_nothing_outside_the_list_commits_without_the_compiler(verb):
    """with the runtime compiler off, nothing behind or between the lines of the list commits: the next power of two is
    the register-resident tier's, a length that is no power of two has no pre-compiled fused kernel"""
    G, pf, torch = _mods()
    real = VERBS[verb][1]
    with _env(PFFT_JIT="0"):
        for prec in ("f32", "f64"):
            for m, reason in ((BEYOND[prec], "register-resident"), (NOT_A_POWER_OF_TWO, "PFFT_JIT=0")):
                n = 2 * m if real else m
                with pytest.raises(pf.unsupported_configuration) as e:
                    _commit_and_prepare(pf, verb, prec, n)
                assert reason in str(e.value), (verb, prec, n, str(e.value))
            # (and the last line of the list does: the refusals above are not the block's doing)
            m = LINES[prec][-1]
            _commit_and_prepare(pf, verb, prec, 2 * m if real else m)
