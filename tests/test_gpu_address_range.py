"""The fused verbs at the top of their 32-bit range and past 4 GiB.  The kernels behind real, any-length and fp16
transforms, convolve / correlate, filter and stft address the rows of one work-group with 32-bit byte offsets from a
64-bit base computed per group, and the host refuses what would not fit.  Here the accepted side of that contract runs:

Part A  geometries derived from the host's own rule (the derivation is the comment at each case), the largest it accepts:
        the highest byte offset one group forms is well past 2^31 and within 1 MiB of 2^32, and the same geometry one
        element larger is refused with unsupported_configuration naming "4 GiB" (that call launches nothing).
Part B  packed rows in buffers of 4.5 ... 10 GiB: the 64-bit group bases, at batch counts that are no multiple of FPW.

Every launch is checked in EVERY output element, on the device (helpers.check_rows): the input is periodic -- row b holds
base[b mod 61], a long signal base[(t + i) mod 61] -- so that a small fp64 reference (NumPy, the formulas of the
per-verb test files) covers gigabytes; the criterion is the project's own, per work-group row: relative L2 within
helpers.REL_L2_TOL and helpers.check_reference_rule's per-element rule with n = N (fp16: test_gpu_half.py's criterion).
A displacement by a multiple of 61 rows or samples is invisible to such an input (never a 32-bit wrap: a power of two);
so every case runs a second time on device-generated random data, checked at marked rows -- the first and last, and
those on either side of byte offsets 2^31 and 2^32 (and element 2^31) of each buffer -- against NumPy on slices copied
to the host.  Write sets, on the device: every buffer is a gpu_utils.Guarded allocation; both guards, every element
outside the output rows (the gaps between pitched signals and frames included) hold the padding bit pattern, and the
input equals its generator bit for bit.

What is not here: part A.6 for real plans.  A real descriptor (a real convolution descriptor too) takes packed rows only,
so the pitch arithmetic of real_io / rconv_io cannot be driven above N + 2 scalars per row;
test_real_plans_take_packed_rows_only pins that refusal, which is what keeps that arithmetic in range.

Measured on the MI355X (worst row of every launch of a verb, periodic and random data, relative L2):
  filter convolve / correlate     fp32 2.4e-07 / 2.3e-07, fp64 4.0e-16 / 4.1e-16; real plans fp32 2.4e-07 / 2.4e-07, fp64 4.5e-16 / 4.5e-16
  stft                            fp32 1.4e-07, fp64 3.9e-16
  convolve / correlate            fp32 1.9e-07 / 1.6e-07, fp64 3.9e-16 / 4.0e-16; real plan fp32 1.9e-07
  R2C / C2R                       fp32 1.3e-07 / 1.3e-07, fp64 3.3e-16 / 3.4e-16
  any-length                      fp32 2.1e-07
  fp16                            2.1e-04 (of the order of the rounding to fp16 itself; the limit is 1.5 times that rounding per row, plus 1e-6)
Nothing failed: no wrong value and no stray write, in 54 cases.  Peak device memory of the module 45.3 GiB (torch's
max_memory_allocated; the 9 signals of 4 GiB of test_stft_rows_of_one_group_cross_signals_at_the_limit[3-in_pitch] and the
mask of their write-set check).  pytest --durations=0, the whole module in one process: 31 s for 54 tests; the slowest
are test_any_length_rows_at_the_limit[True] 3.8 s, test_filter_one_signal_at_the_limit[False-f32-4096-False] 3.4 s (the first
test: the first allocations), test_stft_one_signal_at_the_limit[f64-1024-reflect] 2.9 s, test_stft_rows_of_one_group_cross_
signals_at_the_limit[3-in_pitch] 2.0 s, the short-signal filters 0.8 ... 1.9 s; every other test takes 0.05 ... 1 s, two
launches and their checks each.  test_gpu_fullsize.py::test_buffers_beyond_4gib, which moves the same volume per launch,
takes 8.1 s for its 15 launches in the same session, 0.54 s per launch.

No case is skipped."""
import numpy as np
import pytest

import helpers as H

pytestmark = pytest.mark.gpu

P = 61                 # distinct rows / the period of a long signal: an odd prime that divides no hop or pitch used here
K = 17                 # taps: the segment count stays small
TOP = (1 << 32) - 1    # the highest value a 32-bit byte offset takes
MIB = 1 << 20
UNSUPPORTED = 2


def _mods():
    import gpu_utils as G
    import portfft_amd as pf
    return G, pf, G.torch_mod()


def _types(prec):
    import torch
    if prec == "f64":
        return np.float64, np.complex128, torch.float64, torch.complex128
    return np.float32, np.complex64, torch.float32, torch.complex64


def _draw(rng, shape, dtype):
    if np.dtype(dtype).kind == "c":
        return (rng.uniform(-1, 1, shape) + 1j * rng.uniform(-1, 1, shape)).astype(dtype)
    return rng.uniform(-1, 1, shape).astype(dtype)


_worst = {}


def _note(verb, prec, err):
    _worst[(verb, prec)] = max(_worst.get((verb, prec), 0.0), float(err))


def _done(torch, what):
    torch.cuda.empty_cache()
    print("%s: done; peak device memory so far %.1f GiB; worst rel-L2 so far %s" % (
        what, torch.cuda.max_memory_allocated() / 2.0 ** 30, {"%s %s" % k: "%.2e" % v for k, v in sorted(_worst.items())}))


def _marks(offsets, rows, extra=()):
    """rows to compare on the host: the first and last two, and those on either side of 2^31 and 2^32 bytes in each of the
    monotone byte-offset arrays `offsets` (and of the values `extra` in the same arrays)"""
    marks = {0, 1, rows - 2, rows - 1}
    for off in offsets:
        for b in (1 << 31, 1 << 32) + tuple(extra):
            j = int(np.searchsorted(off, b))
            marks.update((j - 2, j - 1, j, j + 1))
    return sorted(r for r in marks if 0 <= r < rows)


def _compare(got, exp, ct, n, tol, what):
    err = H.rel_l2(got, exp)
    assert err <= tol, (what, err, tol)
    assert H.check_reference_rule(np.asarray(got).astype(ct), np.asarray(exp).astype(ct), n), (what, "per-element rule")
    return err


# ---------------------------------------------------------------------------------------------------------------------
# filter (stockham_wg_ols.hpp, stockham_wg_rols.hpp)

_fplans = {}


def _fplan(pf, real, n, prec):
    key = (real, n, prec)
    if key not in _fplans:
        d = pf.real_convolution_descriptor(n, prec) if real else pf.convolution_descriptor([n], prec)
        plan = d.commit()
        _fplans[key] = (plan, float(n), max(1, plan.info().dims[0].ffts_per_workgroup))
    return _fplans[key]


def _hop(real, n, k, correlate):
    """the host's choice (verb_geometry.hpp: filter_geometry_of)"""
    if not real:
        return n - k + 1
    return (n - k + 1) & ~1 if correlate else n - (k & ~1)


def _lead_conv(real, k):
    return (k & ~1) if real else k - 1


def _filter_reach(real, fpw, ns, in_length, in_pitch, out_length, out_pitch, k, es):
    """verb_geometry.hpp, filter_geometry_of: the bytes the rows of one work-group span"""
    span = min(fpw, ns)
    return ((span - 1) * max(in_pitch, out_pitch) + max(in_length, out_length) + _lead_conv(real, k) + (1 if real else 0)) * es


def _filter_case(real, prec, n, ns, in_length, in_pitch, out_length, out_pitch, nf, correlate, what, refused=None,
                 top=True, seed=1):
    """one geometry of plan.filter: the refused neighbour (a dict of the arguments that differ), a launch on the periodic
    input checked in every row, a launch on random data checked at the marked rows; write sets of both"""
    G, pf, torch = _mods()
    from portfft_amd import _lib
    rt, ct, trt, tct = _types(prec)
    snp, sdt = (rt, trt) if real else (ct, tct)
    es = np.dtype(snp).itemsize
    plan, c, fpw = _fplan(pf, real, n, prec)
    tol = H.REL_L2_TOL[np.dtype(ct)]
    rng = np.random.Generator(np.random.SFC64(1000 * n + ns + seed))
    taps = (_draw(rng, (nf, K), snp) / np.sqrt(K)).astype(snp)
    base = _draw(rng, (P,), snp)
    plan.set_filter_taps(torch.from_numpy(taps).cuda())
    hop = _hop(real, n, K, correlate)
    n_seg = -(-out_length // hop)
    reach = _filter_reach(real, fpw, ns, in_length, in_pitch, out_length, out_pitch, K, es)
    verb = "%sfilter %s" % ("real " if real else "", "correlate" if correlate else "convolve")
    print("%s: %s %s N=%d fpw %d: %d signal(s), in %d pitch %d, out %d pitch %d, hop %d, %d segments; one group spans %d "
          "bytes = 2^32 - %d" % (what, verb, prec, n, fpw, ns, in_length, in_pitch, out_length, out_pitch, hop, n_seg, reach,
                                 (1 << 32) - reach))
    assert reach <= TOP
    assert hop % P and in_pitch % P and out_pitch % P
    if top:
        assert reach > TOP - MIB and reach > (1 << 31) + (1 << 30), (what, reach)
    gin, gout = G.Guarded(ns * in_pitch, sdt), G.Guarded(ns * out_pitch, sdt)
    geo = dict(il=in_length, ip=in_pitch, ol=out_length, op=out_pitch)
    if refused is not None:  # nothing is launched: the rule answers first
        g2 = dict(geo, **refused)
        st = _lib.lib.pfft_execute_filter(plan._plan, int(correlate), gin.buf.data_ptr(), gout.buf.data_ptr(), ns, g2["il"],
                                          g2["ip"], g2["ol"], g2["op"])
        msg = _lib.lib.pfft_last_error().decode()
        print("%s: the neighbour %s is refused: %s" % (what, refused, msg))
        assert st == UNSUPPORTED and "4 GiB" in msg, (what, st, msg)
    xv = gin.buf.view(ns, in_pitch)[:, :in_length]
    yv = gout.buf.view(ns, out_pitch)[:, :out_length]
    if ns == 1:
        xv, yv = xv[0], yv[0]
    # 1. the periodic input: every row
    base_t = torch.from_numpy(base).cuda()
    H.fill_periodic(gin.buf, base_t, ns, in_length, in_pitch, torch)
    plan.filter(xv, yv, correlate=correlate)
    plan.wait()
    gin.check(what + ": input")
    gout.check(what + ": output")
    sig0, sig_len = np.arange(ns, dtype=np.int64) * in_pitch, np.full(ns, in_length, dtype=np.int64)
    H.check_periodic(gin.buf, base_t, ns, in_length, in_pitch, torch, what=what + ": the input")
    H.check_untouched(gin.buf, sig0, sig_len, what=what + ": input buffer")
    start, valid, key, ref = H.filter_rows(base, taps, c, ns, in_length, out_length, out_pitch, hop, correlate)
    _note(verb, prec, H.check_rows(gout.buf, start, valid, key, ref, tol, what + ": periodic", rule_n=n))
    H.check_untouched(gout.buf, start, valid, what=what + ": output buffer")
    # 2. random data: marked rows against NumPy on slices
    G.fill_random(gin.buf, seed)
    gout.buf.fill_(H.PADDING_VALUE)
    plan.filter(xv, yv, correlate=correlate)
    plan.wait()
    gin.check(what + ": input (random)")
    gout.check(what + ": output (random)")
    G.check_random(gin.buf, seed, what + ": the input (random)")
    H.check_untouched(gout.buf, start, valid, what=what + ": output buffer (random)")
    i_of, s_of = np.repeat(np.arange(ns, dtype=np.int64), n_seg), np.tile(np.arange(n_seg, dtype=np.int64), ns)
    worst = 0.0
    for r in _marks([(i_of * in_pitch + s_of * hop) * es, start * es], ns * n_seg):
        i, first, v = int(i_of[r]), int(s_of[r]) * hop, int(valid[r])
        a, b = (first, first + hop + K - 1) if correlate else (first - (K - 1), first + hop)
        lo, hi = max(a, 0), min(b, in_length)
        x = np.zeros(b - a, dtype=np.float64 if real else np.complex128)
        if hi > lo:
            x[lo - a:hi - a] = gin.buf[i * in_pitch + lo:i * in_pitch + hi].cpu().numpy()
        h = taps[i % nf].astype(x.dtype)
        exp = c * (np.correlate(x, h, "valid") if correlate else np.convolve(x, h, "valid"))[:v]
        got = gout.buf[int(start[r]):int(start[r]) + v].cpu().numpy()
        worst = max(worst, _compare(got, exp, ct, n, tol, (what, "random", "row", r, "signal", i, "sample", first)))
    print("%s: random data, marked rows: worst rel-L2 %.3e" % (what, worst))
    _note(verb, prec, worst)
    del gin, gout, xv, yv, base_t
    _done(torch, what)


# (real, precision, N): an FPW = 1 shape whose window lives in SGPRs, a STAGED one (windows in LDS), fp64 -- the shape
# table of test_gpu_filter.py / test_gpu_rfilter.py; a real plan of N scalars runs the N / 2-point configuration
ONE_SIGNAL = [(False, "f32", 4096), (False, "f32", 256), (False, "f64", 4096), (True, "f32", 8192), (True, "f64", 8192)]


@pytest.mark.parametrize("correlate", [False, True])
@pytest.mark.parametrize("real,prec,n", ONE_SIGNAL)
def test_filter_one_signal_at_the_limit(real, prec, n, correlate):
    """A.1 / A.3: one signal.  span = 1, so the rule is (max(in_length, out_length) + lead_conv + [real: 1]) * es <= 2^32 - 1
    with lead_conv = K - 1 (real: K rounded down to even, 16).  Convolve at its bound out_length = in_length + K - 1 gives
    in_length <= E - (K - 1) - lead_conv - [1], E = floor((2^32 - 1) / es); correlate at its bound out_length = in_length
    gives in_length <= E - lead_conv - [1].  A real plan takes the largest ODD in_length (K - 1 is even: out_length is odd
    too), so that the per-scalar edge of the last pair sits at the top; the refused neighbour is the rule's own maximum + 1."""
    G, pf, torch = _mods()
    assert (_fplan(pf, real, n, prec)[2] == 1) == (n != 256)  # (N = 256: the STAGED shape, FPW = 16)
    es = np.dtype(_types(prec)[0 if real else 1]).itemsize
    e = TOP // es
    most = e - _lead_conv(real, K) - (1 if real else 0) - (0 if correlate else K - 1)
    in_length = most if not real or most % 2 else most - 1
    out_length = in_length if correlate else in_length + K - 1
    over = most + 1
    _filter_case(real, prec, n, 1, in_length, in_length, out_length, out_length, 1, correlate,
                 "A one signal %s%s N=%d %s" % ("real " if real else "", prec, n, "corr" if correlate else "conv"),
                 refused=dict(il=over, ip=over, ol=over if correlate else over + K - 1, op=over if correlate else over + K - 1))


@pytest.mark.parametrize("correlate", [False, True])
@pytest.mark.parametrize("real,prec,n", [(False, "f32", 512), (False, "f64", 512), (True, "f32", 1024), (True, "f64", 1024)])
def test_filter_short_signals_at_the_limit(real, prec, n, correlate):
    """A.2 / A.3: 2 fpw + 1 one-segment signals on an FPW = 4 shape, a filter per signal.  span = fpw, so the rule is
    ((fpw - 1) * max(in_pitch, out_pitch) + max(in_length, out_length) + lead_conv + [real: 1]) * es <= 2^32 - 1: the larger
    pitch is floor((E - max(lengths) - lead_conv - [1]) / (fpw - 1)), made odd (one less where it is even), the other one two
    less; convolve gives the larger one to the input, correlate to the output.  The row di = fpw - 1 of a group then starts
    just under 4 GiB.  One segment: out_length = hop (real: odd, hop - 1), in_length = out_length - (K - 1)."""
    G, pf, torch = _mods()
    fpw = _fplan(pf, real, n, prec)[2]
    assert fpw > 1, fpw
    es = np.dtype(_types(prec)[0 if real else 1]).itemsize
    hop = _hop(real, n, K, correlate)
    out_length = hop - 1 if real else hop
    in_length = out_length if correlate else out_length - (K - 1)
    most = (TOP // es - max(in_length, out_length) - _lead_conv(real, K) - (1 if real else 0)) // (fpw - 1)
    big = most if most % 2 else most - 1
    in_pitch, out_pitch = (big - 2, big) if correlate else (big, big - 2)
    _filter_case(real, prec, n, 2 * fpw + 1, in_length, in_pitch, out_length, out_pitch, 2 * fpw + 1, correlate,
                 "A short signals %s%s N=%d %s" % ("real " if real else "", prec, n, "corr" if correlate else "conv"),
                 refused={"op" if correlate else "ip": most + 1})


def test_filter_many_ragged_signals_beyond_4gib():
    """B: 70001 signals (no multiple of FPW) of 3 ragged segments each, 5.3 GiB per buffer, a filter of 3 per signal"""
    n = 4096
    hop = n - K + 1
    out_length = 2 * hop + hop // 2 + 1
    for correlate in (False, True):
        in_length = out_length + 3 if correlate else out_length - (K - 1)
        _filter_case(False, "f32", n, 70001, in_length, in_length + 3, out_length, out_length + 5, 3, correlate,
                     "B filter %s" % ("corr" if correlate else "conv"), top=False)


# ---------------------------------------------------------------------------------------------------------------------
# stft (stockham_wg_stft.hpp)

_splans = {}


def _splan(pf, n, prec):
    if (n, prec) not in _splans:
        d = pf.real_descriptor(n, prec)
        d.number_of_transforms = 6
        plan = d.commit()
        _splans[(n, prec)] = (plan, max(1, plan.info().dims[0].ffts_per_workgroup))
    return _splans[(n, prec)]


def _max_frames(n, length, hop, lead, pad):
    if pad == "zero":
        return (length + lead - 1) // hop + 1
    return (length + 2 * lead - n) // hop + 1


def _stft_reach(n, fpw, ns, in_length, in_pitch, lead, frames, frame_pitch, out_pitch, sb):
    """verb_geometry.hpp, stft_geometry_of: (reach_in, reach_out)"""
    cross = min(ns - 1, (fpw - 1 + frames - 1) // frames)
    return ((cross * in_pitch + in_length + lead + n + 1) * sb,
            (cross * out_pitch + min(fpw - 1, frames - 1) * frame_pitch + n // 2 + 1) * 2 * sb)


def _stft_case(prec, n, ns, in_length, in_pitch, hop, lead, pad, frames, frame_pitch, out_pitch, what, refused=None,
               top="in", seed=2):
    G, pf, torch = _mods()
    from portfft_amd import _lib
    rt, ct, trt, tct = _types(prec)
    sb, m = np.dtype(rt).itemsize, n // 2
    plan, fpw = _splan(pf, n, prec)
    tol = H.REL_L2_TOL[np.dtype(ct)]
    rng = np.random.Generator(np.random.SFC64(1000 * n + ns + seed))
    w = _draw(rng, (n,), rt)
    base = _draw(rng, (P,), rt)
    plan.set_window(torch.from_numpy(w).cuda())
    reach = _stft_reach(n, fpw, ns, in_length, in_pitch, lead, frames, frame_pitch, out_pitch, sb)
    print("%s: stft %s N=%d fpw %d pad %s: %d signal(s), in %d pitch %d, hop %d lead %d, %d frames, frame pitch %d, out pitch "
          "%d; one group spans %d bytes of input = 2^32 - %d, %d of output = 2^32 - %d" % (
              what, prec, n, fpw, pad, ns, in_length, in_pitch, hop, lead, frames, frame_pitch, out_pitch, reach[0],
              (1 << 32) - reach[0], reach[1], (1 << 32) - reach[1]))
    assert max(reach) <= TOP
    assert hop % P and in_pitch % P and out_pitch % P and frame_pitch % P
    if top is not None:
        r = reach[0 if top == "in" else 1]
        assert r > TOP - MIB and r > (1 << 31) + (1 << 30), (what, reach)
    gin, gout = G.Guarded(ns * in_pitch, trt), G.Guarded(ns * out_pitch, tct)
    geo = dict(il=in_length, ip=in_pitch, fp=frame_pitch, op=out_pitch)
    if refused is not None:  # nothing is launched: the rule answers first
        g2 = dict(geo, **refused)
        st = _lib.lib.pfft_execute_stft(plan._plan, gin.buf.data_ptr(), gout.buf.data_ptr(), ns, g2["il"], g2["ip"], hop, lead,
                                        1 if pad == "reflect" else 0, frames, g2["fp"], g2["op"])
        msg = _lib.lib.pfft_last_error().decode()
        print("%s: the neighbour %s is refused: %s" % (what, refused, msg))
        assert st == UNSUPPORTED and "4 GiB" in msg, (what, st, msg)
    xv = gin.buf.view(ns, in_pitch)[:, :in_length]
    yv = gout.buf.view(ns, out_pitch)[:, :frames * frame_pitch].view(ns, frames, frame_pitch)[:, :, :m + 1]
    if ns == 1:
        xv, yv = xv[0], yv[0]
    # 1. the periodic input: every frame
    base_t = torch.from_numpy(base).cuda()
    H.fill_periodic(gin.buf, base_t, ns, in_length, in_pitch, torch)
    plan.stft(xv, yv, hop, lead=lead, pad=pad)
    plan.wait()
    gin.check(what + ": input")
    gout.check(what + ": output")
    sig0, sig_len = np.arange(ns, dtype=np.int64) * in_pitch, np.full(ns, in_length, dtype=np.int64)
    H.check_periodic(gin.buf, base_t, ns, in_length, in_pitch, torch, what=what + ": the input")
    H.check_untouched(gin.buf, sig0, sig_len, what=what + ": input buffer")
    start, valid, key, ref = H.stft_rows(base, w, 1.0, n, ns, in_length, hop, lead, pad, frames, frame_pitch, out_pitch)
    _note("stft", prec, H.check_rows(gout.buf, start, valid, key, ref, tol, what + ": periodic", rule_n=n))
    H.check_untouched(gout.buf, start, valid, what=what + ": output buffer")
    # 2. random data: marked frames against NumPy on slices
    G.fill_random(gin.buf, seed)
    gout.buf.fill_(H.PADDING_VALUE)
    plan.stft(xv, yv, hop, lead=lead, pad=pad)
    plan.wait()
    gin.check(what + ": input (random)")
    gout.check(what + ": output (random)")
    G.check_random(gin.buf, seed, what + ": the input (random)")
    H.check_untouched(gout.buf, start, valid, what=what + ": output buffer (random)")
    i_of, f_of = np.repeat(np.arange(ns, dtype=np.int64), frames), np.tile(np.arange(frames, dtype=np.int64), ns)
    in_off = (i_of * in_pitch + np.maximum(f_of * hop - lead, 0)) * sb
    worst = 0.0
    wd = w.astype(np.float64)
    for r in _marks([in_off, start * 2 * sb], ns * frames):
        i, f = int(i_of[r]), int(f_of[r])
        exp = H.stft_frame(lambda a, b: gin.buf[i * in_pitch + a:i * in_pitch + b].cpu().numpy(), wd, 1.0, n, f * hop - lead,
                           in_length, pad)
        got = gout.buf[int(start[r]):int(start[r]) + m + 1].cpu().numpy()
        assert got[0].imag == 0 and got[m].imag == 0, (what, "imaginary parts of bins 0 and M", r)
        worst = max(worst, _compare(got, exp, ct, n, tol, (what, "random", "row", r, "signal", i, "frame", f)))
    print("%s: random data, marked frames: worst rel-L2 %.3e" % (what, worst))
    _note("stft", prec, worst)
    del gin, gout, xv, yv, base_t
    _done(torch, what)


@pytest.mark.parametrize("pad", ["zero", "reflect"])
@pytest.mark.parametrize("prec,n", [("f32", 8192), ("f32", 1024), ("f64", 8192), ("f64", 1024)])
def test_stft_one_signal_at_the_limit(prec, n, pad):
    """A.4: one signal, hop = N, on an FPW = 1 shape (N = 8192: 4096 points) and an FPW = 4 one (N = 1024).  cross = 0, so
    reach_in = (in_length + lead + N + 1) * sb <= 2^32 - 1 gives in_length = floor((2^32 - 1) / sb) - lead - N - 1, with as
    many frames as the mode admits: zeros with lead = N - 1, and reflection with lead = N / 2, whose last frame mirrors
    2 * last - p at the top of the `int` range (fp32: last just under 2^30 scalars).  frame_pitch = M + 3."""
    G, pf, torch = _mods()
    fpw = _splan(pf, n, prec)[1]
    assert (fpw == 1) == (n == 8192), fpw
    sb = np.dtype(_types(prec)[0]).itemsize
    lead = n - 1 if pad == "zero" else n // 2
    in_length = TOP // sb - lead - n - 1
    frames = _max_frames(n, in_length, n, lead, pad)
    fp = n // 2 + 3
    _stft_case(prec, n, 1, in_length, in_length, n, lead, pad, frames, fp, frames * fp, "A stft one signal %s N=%d %s" % (prec, n, pad),
               refused=dict(il=in_length + 1, ip=in_length + 1))


@pytest.mark.parametrize("which", ["in_pitch", "out_pitch"])
@pytest.mark.parametrize("frames", [1, 3])
def test_stft_rows_of_one_group_cross_signals_at_the_limit(frames, which):
    """A.5: fp32 N = 1024 (FPW = 4), 2 fpw + 1 signals of 1 or 3 frames, frame_pitch = M + 3.  The rows of a group cross
    `cross` = min(S - 1, ceil((fpw - 1) / frames)) signal boundaries.  in_pitch: the largest with (cross * in_pitch +
    in_length + lead + N + 1) * sb <= 2^32 - 1; out_pitch: the largest with (cross * out_pitch + min(fpw - 1, frames - 1) *
    frame_pitch + M + 1) * eb <= 2^32 - 1; the other pitch stays small.  Reflection with lead = N / 2 on signals of N + 1
    scalars: hop = N + 3 admits one frame, hop = N / 2 - 1 three."""
    G, pf, torch = _mods()
    prec, n = "f32", 1024
    fpw = _splan(pf, n, prec)[1]
    assert fpw > 1
    m, sb, ns = n // 2, 4, 2 * fpw + 1
    hop, lead, fp = (n + 3 if frames == 1 else m - 1), m, m + 3
    in_length = n + 1
    assert _max_frames(n, in_length, hop, lead, "reflect") == frames
    cross = min(ns - 1, (fpw - 1 + frames - 1) // frames)
    if which == "in_pitch":
        in_pitch = (TOP // sb - in_length - lead - n - 1) // cross
        out_pitch = frames * fp + 3
        refused = dict(ip=in_pitch + 1)
    else:
        in_pitch = in_length + 2
        out_pitch = (TOP // (2 * sb) - min(fpw - 1, frames - 1) * fp - (m + 1)) // cross
        refused = dict(op=out_pitch + 1)
    _stft_case(prec, n, ns, in_length, in_pitch, hop, lead, "reflect", frames, fp, out_pitch,
               "A stft %d signals of %d frame(s), %s at the limit" % (ns, frames, which), refused=refused,
               top="in" if which == "in_pitch" else "out")


def test_stft_many_signals_beyond_4gib():
    """B: 400001 signals (no multiple of FPW) of 5 frames each: 5.4 GiB of input, 7.7 GiB of output"""
    n = 1024
    hop, lead = n + 3, n // 2
    in_length = 4 * hop - lead + 7
    assert _max_frames(n, in_length, hop, lead, "zero") == 5
    fp = n // 2 + 3
    _stft_case("f32", n, 400001, in_length, in_length + 2, hop, lead, "zero", 5, fp, 5 * fp + 1, "B stft", top=None)


# ---------------------------------------------------------------------------------------------------------------------
# rows: compute_forward / compute_backward of real, any-length and fp16 plans, convolve / correlate

def _round16(y):
    return y.real.astype(np.float16).astype(np.float64) + 1j * y.imag.astype(np.float16).astype(np.float64)


class _Side:
    """one side of a rows case: a flat device tensor, rows of `width` elements every `dist` (pairs: the tensor holds
    interleaved (re, im) scalars and width / dist count complex elements)"""

    def __init__(self, buf, width, dist, pairs=False):
        self.buf, self.width, self.dist, self.pairs = buf, width, dist, pairs
        self.es = buf.element_size() * (2 if pairs else 1)

    def elems(self):
        return self.buf.view(-1, 2) if self.pairs else self.buf

    def row(self, b):
        r = self.elems()[b * self.dist:b * self.dist + self.width].cpu().numpy()
        return r[:, 0].astype(np.float64) + 1j * r[:, 1].astype(np.float64) if self.pairs else r

    def fill_rows(self, base_t, batch, torch, chunk=1 << 24):
        ev = self.elems()
        per = max(1, chunk // self.width)
        cols = torch.arange(self.width, dtype=torch.int64, device="cuda")[None, :]
        for b0 in range(0, batch, per):
            b = torch.arange(b0, min(batch, b0 + per), dtype=torch.int64, device="cuda")
            ev[(b[:, None] * self.dist + cols).reshape(-1)] = base_t[b % P].reshape((-1,) + tuple(base_t.shape[2:]))

    def check_rows_unchanged(self, base_t, batch, torch, what, chunk=1 << 24):
        ev = self.elems()
        per = max(1, chunk // self.width)
        cols = torch.arange(self.width, dtype=torch.int64, device="cuda")[None, :]
        for b0 in range(0, batch, per):
            b = torch.arange(b0, min(batch, b0 + per), dtype=torch.int64, device="cuda")
            got = ev[(b[:, None] * self.dist + cols).reshape(-1)]
            want = base_t[b % P].reshape((-1,) + tuple(base_t.shape[2:]))
            same = H._bit_rows(got.reshape(-1), torch) == H._bit_rows(want.reshape(-1), torch)
            assert bool(same.all()), "%s changed in rows %d .. %d" % (what, b0, int(b[-1]))


def _rows_case(what, verb, prec, n, batch, launch, gbufs, xin, yout, base, ref, keys, row_ref, in_place=False, fp16=False,
               write_set=True, seed=3):
    """launch(): the execute.  xin / yout: _Side; base: (P, width) rows of the input's storage type (fp16: (P, width, 2));
    ref: the fp64 reference rows, keys(b) their index for row b; row_ref(b, x): NumPy's row for the input row x"""
    G, pf, torch = _mods()
    rt, ct, trt, tct = _types("f32" if prec == "f16" else prec)
    pad = H.PADDING_VALUE  # (exact in fp16 too)
    if fp16:  # test_gpu_half.py: rel-L2 <= 1.5 e_round + 1e-6 per transform, |out - Y| <= ulp16(Y) + 1e-6 max|Y| per component
        tol = 1.5 * np.linalg.norm(_round16(ref) - ref, axis=1) / np.linalg.norm(ref, axis=1) + 1e-6
    else:
        tol = H.REL_L2_TOL[np.dtype(ct)]
    b_all = np.arange(batch, dtype=np.int64)
    start, valid = b_all * yout.dist, np.full(batch, yout.width, dtype=np.int64)
    unit = 2 if yout.pairs else 1
    print("%s: %s %s N=%d: %d rows, in %d every %d (%.2f GiB), out %d every %d (%.2f GiB)%s" % (
        what, verb, prec, n, batch, xin.width, xin.dist, xin.buf.numel() * xin.buf.element_size() / 2.0 ** 30, yout.width,
        yout.dist, yout.buf.numel() * yout.buf.element_size() / 2.0 ** 30, ", in place" if in_place else ""))
    base_t = torch.from_numpy(base).cuda()
    # 1. periodic rows: every row
    xin.fill_rows(base_t, batch, torch)
    launch()
    for i, g in enumerate(gbufs):
        g.check("%s: buffer %d" % (what, i))
    _note(verb, prec, H.check_rows(yout.buf, start, valid, keys(b_all), ref, tol, what + ": periodic",
                                   rule_n=None if fp16 else n, pairs=yout.pairs, fp16=fp16))
    if not in_place:
        xin.check_rows_unchanged(base_t, batch, torch, what + ": the input")
        H.check_untouched(xin.buf, b_all * xin.dist, np.full(batch, xin.width), pad=pad, what=what + ": input buffer",
                          unit=2 if xin.pairs else 1)
        if write_set:
            H.check_untouched(yout.buf, start, valid, pad=pad, what=what + ": output buffer", unit=unit)
    # 2. random data: marked rows against NumPy
    marks = _marks([b_all * xin.dist * xin.es, b_all * yout.dist * yout.es], batch,
                   extra=((1 << 31) * xin.es, (1 << 31) * yout.es))
    whole_in = gbufs[0].buf
    G.fill_random(whole_in, seed)
    rows_in = {b: xin.row(b) for b in marks}
    if not in_place:
        yout.buf.fill_(pad)
    launch()
    for i, g in enumerate(gbufs):
        g.check("%s: buffer %d (random)" % (what, i))
    if not in_place:
        G.check_random(whole_in, seed, what + ": the input (random)")
        if write_set:
            H.check_untouched(yout.buf, start, valid, pad=pad, what=what + ": output buffer (random)", unit=unit)
    worst = 0.0
    for b in marks:
        exp, got = row_ref(b, rows_in[b]), yout.row(b)
        if fp16:
            import test_gpu_half
            test_gpu_half.check_accuracy(np.asarray(got)[None, :], exp[None, :], (what, "random", "row", b))
            worst = max(worst, H.rel_l2(got, exp))
        else:
            worst = max(worst, _compare(got, exp, ct, n, tol, (what, "random", "row", b)))
    print("%s: random data, %d marked rows: worst rel-L2 %.3e" % (what, len(marks), worst))
    _note(verb, prec, worst)


def _limit_refused(pf, make, what):
    """commit of the descriptor make() returns is refused, naming the 4 GiB span"""
    with pytest.raises(pf.unsupported_configuration, match="4 GiB") as e:
        make().commit()
    print("%s: the neighbour is refused: %s" % (what, e.value))


def _real_desc(pf, n, prec, batch, fdist=None, bdist=None, conv=False, in_place=False):
    d = (pf.real_convolution_descriptor if conv else pf.real_descriptor)(n, prec)
    d.number_of_transforms = batch
    if fdist is not None:
        d.forward_distance = fdist
    if bdist is not None:
        d.backward_distance = bdist
    if in_place:
        d.placement = pf.placement.IN_PLACE
        d.forward_distance = 2 * d.backward_distance
    return d


def _real_sides(G, torch, prec, n, batch, fdist, bdist, in_place):
    """(guarded buffers, the real side, the complex side) of a real plan"""
    rt, ct, trt, tct = _types(prec)
    m = n // 2
    if in_place:  # one buffer: row t holds N scalars in M + 1 complex slots
        g = G.Guarded(batch * (m + 1), tct)
        return [g], _Side(torch.view_as_real(g.buf).reshape(-1), n, 2 * (m + 1)), _Side(g.buf, m + 1, m + 1)
    gr, gc = G.Guarded(batch * fdist, trt), G.Guarded(batch * bdist, tct)
    return [gr, gc], _Side(gr.buf, n, fdist), _Side(gc.buf, m + 1, bdist)


def _real_case(what, prec, n, batch, fdist, bdist, backward, in_place=False, plan=None):
    """R2C (compute_forward) or C2R (compute_backward) of a real plan"""
    G, pf, torch = _mods()
    rt, ct, trt, tct = _types(prec)
    m = n // 2
    if in_place:
        fdist, bdist = 2 * (m + 1), m + 1
    plan = plan or _real_desc(pf, n, prec, batch, fdist, bdist, in_place=in_place).commit()
    gbufs, rside, cside = _real_sides(G, torch, prec, n, batch, fdist, bdist, in_place)
    rng = np.random.Generator(np.random.SFC64(n + batch))

    def bins(x):  # what C2R reads: the imaginary parts of bins 0 and M are ignored
        x = np.array(x, dtype=np.complex128)
        x[..., 0], x[..., m] = x[..., 0].real, x[..., m].real
        return x

    if backward:
        base = _draw(rng, (P, m + 1), ct)
        ref = n * np.fft.irfft(bins(base), n, axis=1)
        xin, yout = cside, rside
        if not in_place:
            gbufs = gbufs[::-1]

        def launch():
            (plan.compute_backward(gbufs[0].buf) if in_place else plan.compute_backward(cside.buf, rside.buf)).wait()

        def row_ref(b, x):
            return n * np.fft.irfft(bins(x), n)
    else:
        base = _draw(rng, (P, n), rt)
        ref = np.fft.rfft(base.astype(np.float64), axis=1)
        xin, yout = rside, cside

        def launch():
            (plan.compute_forward(gbufs[0].buf) if in_place else plan.compute_forward(rside.buf, cside.buf)).wait()

        def row_ref(b, x):
            return np.fft.rfft(x.astype(np.float64))
    _rows_case(what, "C2R" if backward else "R2C", prec, n, batch, launch, gbufs, xin, yout, base, ref, lambda b: b % P, row_ref,
               in_place=in_place)
    del gbufs, rside, cside, xin, yout
    _done(torch, what)


@pytest.mark.parametrize("conv", [False, True])
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_real_plans_take_packed_rows_only(prec, conv):
    """A.6 has no real case: real_io / rconv_io form rp = forward_distance * sizeof(T), f * rp and the resource size
    live * rp in `unsigned`, and plan_real's own backstop is forward_distance < 2^30 scalars whatever FPW and precision --
    which an fp64 pitch of 2^29, or an fp32 one with FPW >= 2, would wrap.  What keeps that arithmetic in range is
    validate(): a real descriptor (a real convolution descriptor too) is PACKED, forward_distance = N and backward_distance
    = N / 2 + 1 -- the padded in-place pair aside -- so fpw rows span fpw * (N + 2) scalars.  This pins that refusal: whoever
    lifts it has to give plan_real the row_limit rule of plan_conv first."""
    G, pf, torch = _mods()
    n = 1024
    for fdist, bdist in ((n + 2, None), (None, n // 2 + 2), ((1 << 28) - 1, None), ((1 << 30) - 1, (1 << 29) - 1)):
        with pytest.raises(pf.unsupported_configuration, match="PACKED layout only"):
            _real_desc(pf, n, prec, 9, fdist, bdist, conv=conv).commit()


def _conv_case(what, real, prec, n, batch, dist, correlate, nf=3, plan=None):
    """convolve / correlate of a complex or a real plan, out of place, both sides at pitch `dist`"""
    G, pf, torch = _mods()
    rt, ct, trt, tct = _types(prec)
    snp, sdt = (rt, trt) if real else (ct, tct)
    m = n // 2
    rng = np.random.Generator(np.random.SFC64(n + batch + nf))
    spectra = _draw(rng, (nf, m + 1 if real else n), ct)
    plan.set_filter(torch.from_numpy(spectra).cuda())
    hh = spectra.astype(np.complex128)
    if real:
        hh[:, 0], hh[:, m] = hh[:, 0].real, hh[:, m].real
    if correlate:
        hh = np.conj(hh)

    def rows(x, f):
        if real:
            return n * np.fft.irfft(np.fft.rfft(x.astype(np.float64), axis=-1) * hh[f], n, axis=-1)
        return n * np.fft.ifft(np.fft.fft(x.astype(np.complex128), axis=-1) * hh[f], axis=-1)

    base = _draw(rng, (P, n), snp)
    ref = np.concatenate([rows(base, f) for f in range(nf)])
    gin, gout = G.Guarded(batch * dist, sdt), G.Guarded(batch * dist, sdt)
    xin, yout = _Side(gin.buf, n, dist), _Side(gout.buf, n, dist)

    def launch():
        (plan.correlate if correlate else plan.convolve)(gin.buf, gout.buf).wait()

    verb = "%s%s" % ("real " if real else "", "correlate" if correlate else "convolve")
    _rows_case(what, verb, prec, n, batch, launch, [gin, gout], xin, yout, base, ref, lambda b: (b % nf) * P + b % P,
               lambda b, x: rows(x, b % nf))
    del gin, gout, xin, yout
    _done(torch, what)


@pytest.mark.parametrize("correlate", [False, True])
@pytest.mark.parametrize("prec,n", [("f32", 512), ("f64", 512)])
def test_convolve_rows_at_the_limit(prec, n, correlate):
    """A.6, convolve / correlate of a complex plan: FPW = 4 shapes, batch 2 fpw + 1, 3 filters.  plan_core.cpp: distances
    below row_limit = 2^32 / (fpw * elem_bytes); the largest accepted is row_limit - 1 on both sides, row_limit is
    refused.  (A real plan takes packed rows only: test_real_plans_take_packed_rows_only.)"""
    G, pf, torch = _mods()
    real = False
    es = 2 * (4 if prec == "f32" else 8)

    def desc(dist, batch):
        d = pf.convolution_descriptor([n], prec)
        d.number_of_transforms, d.forward_distance, d.backward_distance = batch, dist, dist
        return d

    fpw = max(1, desc(n, 1).commit().info().dims[0].ffts_per_workgroup)
    assert fpw > 1
    dist, batch = (1 << 32) // (fpw * es) - 1, 2 * fpw + 1
    what = "A %sconv rows %s %s" % ("real " if real else "", prec, "corr" if correlate else "conv")
    print("%s: fpw %d, distance %d: the %d rows of a group span %d bytes = 2^32 - %d" % (
        what, fpw, dist, fpw, fpw * dist * es, (1 << 32) - fpw * dist * es))
    assert fpw * dist * es > TOP - MIB
    _limit_refused(pf, lambda: desc(dist + 1, batch), what + " distance + 1")
    _conv_case(what, real, prec, n, batch, dist, correlate, plan=desc(dist, batch).commit())


def _complex_case(what, verb, prec, n, batch, dist, plan, backward=False, fp16=False):
    """compute_forward / compute_backward of a complex plan (any-length, fp16), out of place, both sides at pitch `dist`"""
    G, pf, torch = _mods()
    rt, ct, trt, tct = _types("f32" if fp16 else prec)
    rng = np.random.Generator(np.random.SFC64(n + batch))

    def rows(x):
        x = np.asarray(x, dtype=np.complex128)
        return n * np.fft.ifft(x, axis=-1) if backward else np.fft.fft(x, axis=-1)

    if fp16:
        pair = rng.uniform(-1, 1, (P, n, 2)).astype(np.float16)
        base, based = pair, pair[..., 0].astype(np.float64) + 1j * pair[..., 1].astype(np.float64)
        gin, gout = G.Guarded(2 * batch * dist, torch.float16), G.Guarded(2 * batch * dist, torch.float16)
    else:
        base = based = _draw(rng, (P, n), ct)
        gin, gout = G.Guarded(batch * dist, tct), G.Guarded(batch * dist, tct)
    xin, yout = _Side(gin.buf, n, dist, pairs=fp16), _Side(gout.buf, n, dist, pairs=fp16)

    def launch():
        (plan.compute_backward if backward else plan.compute_forward)(gin.buf, gout.buf).wait()

    _rows_case(what, verb, prec, n, batch, launch, [gin, gout], xin, yout, base, rows(based), lambda b: b % P,
               lambda b, x: rows(x), fp16=fp16)
    del gin, gout, xin, yout
    _done(torch, what)


@pytest.mark.parametrize("backward", [False, True])
def test_any_length_rows_at_the_limit(backward):
    """A.6, any-length: fp32 N = 251 (convolution length 512), batch 2 fpw + 1, distances row_limit - 1 = 2^32 / (fpw *
    elem_bytes) - 1 on both sides; row_limit is refused"""
    G, pf, torch = _mods()
    n, prec, es = 251, "f32", 8

    def desc(dist, batch):
        d = pf.any_length_descriptor([n], prec)
        d.number_of_transforms, d.forward_distance, d.backward_distance = batch, dist, dist
        return d

    fpw = max(1, desc(n, 1).commit().info().dims[0].ffts_per_workgroup)
    dist, batch = (1 << 32) // (fpw * es) - 1, 2 * fpw + 1
    what = "A any-length rows %s" % ("backward" if backward else "forward")
    print("%s: fpw %d, distance %d: the %d rows of a group span %d bytes = 2^32 - %d" % (
        what, fpw, dist, fpw, fpw * dist * es, (1 << 32) - fpw * dist * es))
    assert fpw * dist * es > TOP - MIB
    _limit_refused(pf, lambda: desc(dist + 1, batch), what + " distance + 1")
    _complex_case(what, "any-length", prec, n, batch, dist, desc(dist, batch).commit(), backward=backward)


@pytest.mark.parametrize("in_place", [False, True])
@pytest.mark.parametrize("backward", [False, True])
@pytest.mark.parametrize("prec,n,batch", [("f32", 4096, 540001), ("f64", 1024, 600001)])
def test_real_rows_beyond_4gib(prec, n, batch, backward, in_place):
    """B: packed rows of real plans, 8.2 ... 8.3 GiB (fp32: past 2^31 scalars) and 4.6 GiB (fp64) per buffer"""
    _real_case("B real %s N=%d %s%s" % (prec, n, "C2R" if backward else "R2C", " in place" if in_place else ""), prec, n, batch,
               n, n // 2 + 1, backward, in_place=in_place)


def test_any_length_rows_beyond_4gib():
    """B: N = 4093 fp32, 150001 packed rows, 4.6 GiB per buffer"""
    G, pf, torch = _mods()
    d = pf.any_length_descriptor([4093], "f32")
    d.number_of_transforms = 150001
    _complex_case("B any-length", "any-length", "f32", 4093, 150001, 4093, d.commit())


def test_half_rows_beyond_4gib():
    """B: fp16 N = 4096, 540001 packed rows, 8.2 GiB per buffer: past 2^32 bytes and 2^31 elements"""
    G, pf, torch = _mods()
    d = pf.descriptor([4096], "f16")
    d.number_of_transforms = 540001
    _complex_case("B fp16", "fp16", "f16", 4096, 540001, 4096, d.commit(), fp16=True)


@pytest.mark.parametrize("real,batch", [(False, 150001), (True, 540001)])
def test_convolve_rows_beyond_4gib(real, batch):
    """B: convolve with 3 filters on packed rows, N = 4096 fp32: a complex plan (4.6 GiB per buffer) and a real plan (8.2 GiB:
    past 2^31 scalars); the filter row cycles through the 3 filters across the groups"""
    G, pf, torch = _mods()
    n = 4096
    if real:
        d = _real_desc(pf, n, "f32", batch, conv=True)
    else:
        d = pf.convolution_descriptor([n], "f32")
        d.number_of_transforms = batch
    _conv_case("B %sconvolve" % ("real " if real else ""), real, "f32", n, batch, n, False, plan=d.commit())
