"""Inverse short-time Fourier transform (overlap-add) of REAL signals on the GPU (plan.set_synthesis_window / plan.istft of
a plan of the REAL domain: stockham_wg_istft_kernel): every signal of every case against NumPy in double precision,
    g[i, f] = backward_scale * N * np.fft.irfft(bins[i, f], N);  a loop over the frames adds w * g[i, f] at f * hop and
    w ** 2 into the envelope;  samples lead ... lead + out_length;  NORMALIZE divides by the envelope
and the project's two yardsticks unchanged: relative L2 per signal within helpers.REL_L2_TOL, and
helpers.check_reference_rule with n = N.  Bins are uniform in [-1, 1] in both parts, the imaginary parts of bins 0 and M
included (they must have no effect: np.fft.irfft drops them too).

One length per kernel shape, as in test_gpu_stft.py (every registered line of the kernel runs in
test_gpu_fused_registry.py).  Per length the smallest geometries that can go wrong: hop in {1
(N <= 128), N/4 + 1 made odd, N/2, N} x lead in {0, N/2, the odd one of N/2 - 1 and N/2 + 1, N - 1} x out_length at its
maximum and 3 below it (one odd, one even), three signals of 4 FPW + 3 frames; 1 signal (1-D tensors) of 2 FPW - 1 and of
2 FPW + 1 frames.  PLAIN rotates through periodic Hann, a random window in [-1, 1] and None; every third scenario runs on
the scaled plan of the length (backward_scale = 0.5).  NORMALIZE only runs where the double-precision envelope is at least
0.25 at every written sample -- asserted on the reference envelope itself -- so that the threshold cannot decide
differently in the two precisions: a random window in [0.5, 1] at every geometry, and periodic Hann with hop <= N/2,
lead = N/2 and out_length <= (n_frames - 1) * hop.  One extra case at N = 64: periodic Hann with hop = N, whose envelope
at the frame starts is exactly 0 (w[0] = 0) and whose output there must be exactly 0.0.

EVERY geometry runs with chunk_frames in {0, 1, 2 FPW + 1, >= n_frames} (at least three chunks at the middle value) AND
THE OUTPUTS OF ALL CHUNK LENGTHS ARE COMPARED BIT FOR BIT (helpers.check_same_bits): that is what checks the halo and the
summation order.

Every launch reads from and writes into gpu_utils.Guarded buffers with an ODD out_pitch, frame_pitch = M + 2 or M + 3 and
an in_pitch above the frames: the guards, the gaps between the signals, the tail behind out_length and the whole input
must be unchanged, bit for bit.  Once per case the base pointers are one scalar off 128-byte alignment.

Anchor: with window None, hop = N, lead = 0, PLAIN and out_length = F * N the result is compute_backward of the same plan
on the bins as F rows: checked with the two yardsticks; whether it is also bit-identical is printed.
Round trip: istft(stft(x)) against x on a plan with backward_scale = 1 / N, periodic Hann, hop = N/4, reflection,
lead = N/2, NORMALIZE, out_length = (F - 1) * hop, within 2 * REL_L2_TOL -- one tolerance per verb, the normalised
overlap-add is a weighted average of the frames and does not amplify; the double-precision NumPy composite is first
asserted to reproduce x to 1e-12.

Measured on the MI355X (worst signal of every case of a length, both modes, all windows and chunk lengths, relative L2):
fp32 N=4 6.5e-08, 8 1.2e-07, 32 1.7e-07, 64 2.8e-07, 128 2.7e-07, 512 1.3e-07, 1024 1.3e-07, 4096 1.4e-07, 16384 1.5e-07,
2000 1.5e-07, 12000 1.5e-07; fp64 N=128 5.1e-16, 1024 3.6e-16, 8192 3.9e-16, 6000 4.7e-16; the round trip fp32 5.3e-08 ...
1.8e-07, fp64 2.0e-16 ... 2.7e-16.  The anchor is bit-identical to compute_backward at every length but fp32 N = 8 and 32.

No case is skipped."""
import numpy as np
import pytest

import helpers as H

pytestmark = pytest.mark.gpu

LENGTHS = {"f32": [4, 8, 32, 64, 128, 512, 1024, 4096, 16384, 2000, 12000], "f64": [128, 1024, 8192, 6000]}
CASES = [(p, n) for p in ("f32", "f64") for n in LENGTHS[p]]
BATCH = (2, 3)  # signals x frames of the plan's own number_of_transforms (compute_backward in the anchor test)


def _mods():
    import gpu_utils as G
    import portfft_amd as pf
    return G, pf, G.torch_mod()


def _types(prec):
    return (np.float32, np.complex64) if prec == "f32" else (np.float64, np.complex128)


_plans = {}


def _plan(pf, n, prec, scale=1.0):
    """(plan, backward_scale, fpw) of a length: committed once per process, the window is set per launch"""
    key = (n, prec, scale)
    if key not in _plans:
        d = pf.real_descriptor(n, prec)
        d.number_of_transforms = BATCH[0] * BATCH[1]
        d.backward_scale = scale
        plan = d.commit()
        _plans[key] = (plan, d.backward_scale, max(1, plan.info().dims[0].ffts_per_workgroup))
    return _plans[key]


def _hann(n, rt):
    return (0.5 - 0.5 * np.cos(2 * np.pi * np.arange(n) / n)).astype(rt)  # periodic


def _reference(scale, y, w, n, hop, lead, olen):
    """NumPy in double: irfft, window, overlap-add with a loop; returns (ola, envelope) of samples lead ... lead + olen"""
    ns, frames = y.shape[:2]
    g = scale * n * np.fft.irfft(y.astype(np.complex128), n, axis=-1)
    wd = np.ones(n) if w is None else w.astype(np.float64)
    total = (frames - 1) * hop + n
    ola, env = np.zeros((ns, total)), np.zeros(total)
    for f in range(frames):
        ola[:, f * hop:f * hop + n] += wd * g[:, f]
        env[f * hop:f * hop + n] += wd * wd
    return ola[:, lead:lead + olen], env[lead:lead + olen]


_worst = {}


def _check(got, ref, ct, n, what):
    """got, ref: (signals, samples)"""
    g = np.asarray(got).astype(np.complex128)
    r = np.asarray(ref).astype(np.complex128)
    err = np.linalg.norm(g - r, axis=1) / np.maximum(np.linalg.norm(r, axis=1), 1e-300)
    key = (np.dtype(ct).name, n)
    _worst[key] = max(_worst.get(key, 0.0), float(err.max()))
    print("%s: worst rel-L2 %.3e (signal %d)" % (what, float(err.max()), int(np.argmax(err))))
    assert np.all(err <= H.REL_L2_TOL[np.dtype(ct)]), (what, "signal", int(np.argmax(err)), float(err.max()))
    assert H.check_reference_rule(g, r.astype(ct), n), (what, "per-element reference rule")


def _odd(v):
    return v | 1


def _launch(G, torch, plan, n, y, hop, lead, normalize, olen, chunk, what, guard=None, extra=2, verb=None):
    """plan.istft of the bins y (numpy, (signals, frames, M + 1)) with the window already set: buffers with an odd
    out_pitch, frame_pitch = M + extra and an in_pitch above the frames; write set, guards, unchanged input.  Returns
    (samples as numpy (signals, olen), the whole output allocation as a device tensor)."""
    ns, frames, _ = y.shape
    m = n // 2
    rt = np.float32 if y.dtype == np.complex64 else np.float64
    frame_pitch = m + extra
    in_pitch, out_pitch = frames * frame_pitch + 3, _odd(olen + 4)
    guard = G.GUARD if guard is None else guard
    gin = G.Guarded(ns * in_pitch, torch.from_numpy(y[:0]).dtype, guard)
    gout = G.Guarded(ns * out_pitch, torch.from_numpy(np.zeros(0, dtype=rt)).dtype, guard)
    yv = gin.buf.view(ns, in_pitch)[:, :frames * frame_pitch].view(ns, frames, frame_pitch)[:, :, :m + 1]
    yv.copy_(torch.from_numpy(y))
    before = gin.buf.cpu().numpy()
    xv = gout.buf.view(ns, out_pitch)[:, :olen]
    if ns == 1 and verb is None:  # (a single signal may come as 1-D / 2-D tensors)
        xv, yv = xv[0], yv[0]
    if verb is None:
        plan.istft(yv, xv, hop, lead=lead, normalize=normalize, chunk_frames=chunk)
        plan.wait()
    else:
        verb(yv, xv)
    gin.check(str(what) + ": input")
    gout.check(str(what) + ": output")
    H.check_unchanged(before, gin.buf.cpu().numpy(), what=str(what) + ": the input")
    raw = gout.buf.cpu().numpy()
    idx = (np.arange(ns)[:, None] * out_pitch + np.arange(olen)[None, :]).ravel()
    H.check_write_set(raw, idx, what=str(what) + ": output buffer")
    return raw[idx].reshape(ns, olen), gout.alloc


def _istft(G, torch, plan, scale, fpw, n, y, w, hop, lead, normalize, olen, what, guard=None, extra=2, exact_zero=False):
    """every chunk length of one geometry: chunk_frames = 0 against the reference, the others against its bits"""
    frames = y.shape[1]
    ct = y.dtype
    ola, env = _reference(scale, y, w, n, hop, lead, olen)
    if normalize and not exact_zero:
        assert env.min() >= 0.25, (what, "the reference envelope", float(env.min()))
    if normalize:
        ref = np.where(env > 1e-11, ola / np.where(env > 1e-11, env, 1.0), 0.0)
    else:
        ref = ola
    first = None
    for chunk in (0, 1, 2 * fpw + 1, frames + 2):
        got, alloc = _launch(G, torch, plan, n, y, hop, lead, normalize, olen, chunk, what + ("chunk", chunk), guard, extra)
        if first is None:
            _check(got, ref, ct, n, what)
            first = (got, alloc)
        else:
            H.check_same_bits(first[1], alloc, what=str(what + ("chunk_frames", chunk, "against 0")))
    return first[0], env


def _geometries(n, fpw):
    """(name, signals, frames, hop, lead, out_length, guard)"""
    m = n // 2
    hops = ([1] if n <= 128 else []) + sorted({min(_odd(n // 4 + 1), n), m, n})
    leads = sorted({0, m, m - 1 if (m - 1) % 2 else m + 1, n - 1})
    frames = 4 * fpw + 3  # at least three chunks of 2 fpw + 1 frames
    out = []
    first = True
    for hop in hops:
        for lead in leads:
            top = (frames - 1) * hop + n - lead
            for olen in (top, top - 3):
                out.append(("hop %d lead %d out %d" % (hop, lead, olen), 3, frames, hop, lead, olen, (65, 63) if first else None))
                first = False
    # 1 signal (1-D tensors) of 2 fpw - 1 and 2 fpw + 1 frames
    hop, lead = min(_odd(n // 4 + 1), n), m - 1 if (m - 1) % 2 else m + 1
    for rows in (2 * fpw - 1, 2 * fpw + 1):
        out.append(("%d frames of one signal" % rows, 1, rows, hop, lead, (rows - 1) * hop + n - lead - 1, None))
    return out


def _bins(rng, ns, frames, m, ct):
    rt = np.float32 if ct == np.complex64 else np.float64
    y = np.empty((ns, frames, m + 1), dtype=ct)
    y.real = rng.uniform(-1, 1, y.shape).astype(rt)
    y.imag = rng.uniform(-1, 1, y.shape).astype(rt)
    return y


def _set(plan, torch, w):
    plan.set_synthesis_window(None if w is None else torch.from_numpy(w).cuda())


@pytest.mark.parametrize("prec,n", CASES)
def test_istft_against_numpy(prec, n):
    G, pf, torch = _mods()
    rt, ct = _types(prec)
    m = n // 2
    rng = np.random.Generator(np.random.SFC64(1000 * n + 7))
    fpw = _plan(pf, n, prec)[2]
    plain = [("hann", _hann(n, rt)), ("random", rng.uniform(-1, 1, n).astype(rt)), ("none", None)]
    positive = rng.uniform(0.5, 1, n).astype(rt)
    print("N=%d %s: fpw %d" % (n, prec, fpw))
    seen = set()
    for i, (name, ns, frames, hop, lead, olen, guard) in enumerate(_geometries(n, fpw)):
        plan, scale, _ = _plan(pf, n, prec, 0.5 if i % 3 == 2 else 1.0)
        y = _bins(rng, ns, frames, m, ct)
        wname, w = plain[i % 3] if i % 9 < 6 else plain[(i + 1) % 3]  # (every window meets both plans)
        tag = (prec, n, name, "signals", ns, "frames", frames, "scale", scale)
        _set(plan, torch, w)
        _istft(G, torch, plan, scale, fpw, n, y, w, hop, lead, False, olen, tag + ("plain", wname), guard, 2 + i % 2)
        _set(plan, torch, positive)
        _istft(G, torch, plan, scale, fpw, n, y, positive, hop, lead, True, olen, tag + ("normalize", "positive"), guard, 3 - i % 2)
        if hop <= m and lead == m:  # periodic Hann: some frame covers every sample below (F - 1) hop where w >= 0.5
            _set(plan, torch, plain[0][1])
            cut = (frames - 1) * hop - (3 if olen % 2 else 0)
            if cut >= 1 and (frames - 1) * hop < cut + lead:
                _istft(G, torch, plan, scale, fpw, n, y, plain[0][1], hop, lead, True, cut, tag + ("normalize", "hann", cut), guard)
                seen.add(("hann-normalize", cut % 2))
        seen.add((olen % 2, wname))
    assert {p for p, _ in seen if p in (0, 1)} == {0, 1} and {w for _, w in seen} >= {"hann", "random", "none"}, seen
    assert any(k[0] == "hann-normalize" for k in seen), seen
    print("worst rel-L2 so far: %s" % _worst)


def test_an_empty_envelope_gives_exact_zeros():
    """N = 64, periodic Hann, hop = N: w[0] = 0, so the envelope at the frame starts is exactly 0"""
    G, pf, torch = _mods()
    n, prec = 64, "f32"
    rt, ct = _types(prec)
    plan, scale, fpw = _plan(pf, n, prec)
    rng = np.random.Generator(np.random.SFC64(64))
    w = _hann(n, rt)
    assert w[0] == 0.0
    frames = 4 * fpw + 3
    y = _bins(rng, 3, frames, n // 2, ct)
    _set(plan, torch, w)
    olen = frames * n
    got, env = _istft(G, torch, plan, scale, fpw, n, y, w, n, 0, True, olen, (prec, n, "hann, hop = N"), exact_zero=True)
    starts = np.arange(frames) * n
    # (the neighbours: w[1] ** 2 = sin(pi / 64) ** 4 = 5.8e-6, far from the threshold of 1e-11)
    assert np.all(env[starts] == 0.0) and np.delete(env, starts).min() >= 0.999 * np.sin(np.pi / n) ** 4, env[:3]
    assert np.all(got[:, starts] == 0.0) and not np.any(np.signbit(got[:, starts])), "the samples without envelope"


@pytest.mark.parametrize("prec,n", CASES)
def test_window_none_is_compute_backward(prec, n):
    """hop = N, lead = 0, out_length = F * N, all ones, PLAIN: the rows of the plan's own C2R transform"""
    G, pf, torch = _mods()
    rt, ct = _types(prec)
    m = n // 2
    ns, frames = BATCH
    rng = np.random.Generator(np.random.SFC64(17 * n))
    y = _bins(rng, ns, frames, m, ct)
    same = []
    for scale in (1.0, 0.5):
        plan, scale, fpw = _plan(pf, n, prec, scale)
        _set(plan, torch, None)
        yd = torch.from_numpy(y).cuda()
        x = torch.full((ns * frames * n,), H.PADDING_VALUE, dtype=torch.from_numpy(np.zeros(0, dtype=rt)).dtype, device="cuda")
        plan.compute_backward(yd.reshape(-1), x).wait()
        rows = x.cpu().numpy().reshape(ns, frames * n)
        got, _ = _istft(G, torch, plan, scale, fpw, n, y, None, n, 0, False, frames * n, (prec, n, "window None, whole frames", scale))
        _check(got, rows, ct, n, (prec, n, "against compute_backward"))
        same.append(bool(np.array_equal(got, rows)))
    print("N=%d %s: bit-identical to compute_backward: %s" % (n, prec, same))  # (recorded in DESIGN 3.1j, not a bound)


@pytest.mark.parametrize("prec,n", CASES)
def test_round_trip_through_stft(prec, n):
    G, pf, torch = _mods()
    rt, ct = _types(prec)
    m = n // 2
    plan, scale, fpw = _plan(pf, n, prec, 1.0 / n)
    hop, lead = max(1, n // 4), m
    frames = 4 * fpw + 3
    length = (frames - 1) * hop
    ns = 3
    rng = np.random.Generator(np.random.SFC64(29 * n))
    x = rng.uniform(-1, 1, (ns, length)).astype(rt)
    w = _hann(n, rt)
    # the composite in double reproduces x: the tolerance below is the two verbs' own
    xe = np.pad(x.astype(np.float64), ((0, 0), (lead, lead)), mode="reflect")
    idx = np.arange(frames)[:, None] * hop + np.arange(n)[None, :]
    bins = np.fft.rfft(xe[:, idx] * w.astype(np.float64), axis=-1)
    ola, env = _reference(1.0 / n, bins, w, n, hop, lead, length)
    assert env.min() >= 0.25
    assert np.abs(ola / env - x).max() <= 1e-12
    wd = torch.from_numpy(w).cuda()
    plan.set_window(wd)
    plan.set_synthesis_window(wd)
    xd = torch.from_numpy(x).cuda()
    y = torch.empty(ns, frames, m + 1, dtype=torch.from_numpy(np.zeros(0, dtype=ct)).dtype, device="cuda")
    back = torch.full((ns, length), H.PADDING_VALUE, dtype=xd.dtype, device="cuda")
    plan.stft(xd, y, hop, lead=lead, pad="reflect")
    plan.istft(y, back, hop, lead=lead, normalize=True).wait()
    got = back.cpu().numpy().astype(np.float64)
    err = np.linalg.norm(got - x, axis=1) / np.linalg.norm(x.astype(np.float64), axis=1)
    print("N=%d %s: round trip worst rel-L2 %.3e" % (n, prec, float(err.max())))
    assert np.all(err <= 2 * H.REL_L2_TOL[np.dtype(ct)]), (prec, n, float(err.max()))


@pytest.mark.parametrize("prec,n", [("f32", 512), ("f64", 6000), ("f32", 16384)])
def test_many_trips_of_the_persistent_loop(prec, n):
    """more (signal, chunk) groups than the grid holds work-groups, on a plan that also convolves"""
    G, pf, torch = _mods()
    rt, ct = _types(prec)
    m = n // 2
    plan = pf.real_convolution_descriptor(n, prec).commit()
    fpw = max(1, plan.info().dims[0].ffts_per_workgroup)
    rng = np.random.Generator(np.random.SFC64(7 * n))
    w = rng.uniform(0.5, 1, n).astype(rt)
    _set(plan, torch, w)
    ns, hop, lead = 4, m, m
    frames = 400 * fpw
    olen = (frames - 1) * hop + n - lead - 1
    y = _bins(rng, ns, frames, m, ct)
    ola, env = _reference(1.0, y, w, n, hop, lead, olen)
    assert env.min() >= 0.25
    bits = None
    for chunk in (fpw, 0):
        got, alloc = _launch(G, torch, plan, n, y, hop, lead, True, olen, chunk, (prec, n, "many trips", chunk))
        _check(got, ola / env, ct, n, (prec, n, "many trips", chunk))
        if bits is None:
            bits = alloc
        else:
            H.check_same_bits(bits, alloc, what="many trips: chunk_frames fpw against 0")
    print("N=%d %s: chunk_frames chosen %d of %d frames" % (n, prec, plan.istft_chunk_frames(ns, frames, hop), frames))


def test_the_window_is_replaced_and_a_copy_keeps_its_own():
    G, pf, torch = _mods()
    n, prec = 1024, "f32"
    rt, ct = _types(prec)
    m = n // 2
    rng = np.random.Generator(np.random.SFC64(5))
    hann, rand = _hann(n, rt), rng.uniform(-1, 1, n).astype(rt)
    plan = pf.real_descriptor(n, prec).commit()
    fpw = max(1, plan.info().dims[0].ffts_per_workgroup)
    frames, hop, lead = 9, 257, 512
    olen = (frames - 1) * hop + n - lead
    y = _bins(rng, 3, frames, m, ct)
    fresh = plan.copy()  # made before any window: resolves the kernel itself, shares nothing
    wd = torch.from_numpy(hann).cuda()
    plan.set_synthesis_window(wd)
    wd.fill_(7)  # the plan owns a copy: later writes do not matter
    a, _ = _istft(G, torch, plan, 1.0, fpw, n, y, hann, hop, lead, False, olen, ("original, hann",))
    clone = plan.copy()  # shares the window
    b, _ = _istft(G, torch, clone, 1.0, fpw, n, y, hann, hop, lead, False, olen, ("clone, shared window",))
    H.check_unchanged(a, b, what="a clone transforms with the shared window")
    plan.set_synthesis_window(torch.from_numpy(rand).cuda())
    c, _ = _istft(G, torch, plan, 1.0, fpw, n, y, rand, hop, lead, False, olen, ("original, second window",))
    assert not np.array_equal(a, c)
    b, _ = _istft(G, torch, clone, 1.0, fpw, n, y, hann, hop, lead, False, olen, ("clone afterwards",))
    H.check_unchanged(a, b, what="the clone keeps its window")
    yd = torch.from_numpy(y).cuda()
    xd = torch.zeros(3, olen, dtype=torch.float32, device="cuda")
    with pytest.raises(pf.invalid_configuration, match="no synthesis window has been set"):
        fresh.istft(yd, xd, hop, lead=lead)
    fresh.set_window(None)  # the analysis window is another one
    with pytest.raises(pf.invalid_configuration, match="no synthesis window has been set"):
        fresh.istft(yd, xd, hop, lead=lead)
    fresh.set_synthesis_window(None)
    _istft(G, torch, fresh, 1.0, fpw, n, y, None, hop, lead, False, olen, ("a copy made before any window",))


def test_refusals_name_the_cause():
    G, pf, torch = _mods()
    from portfft_amd import _lib
    lib = _lib.lib
    n, m = 256, 128
    plan = pf.real_descriptor(n).commit()
    fp, ip = m + 1, 5 * (m + 1)
    y = torch.zeros(3, 5, m + 1, dtype=torch.complex64, device="cuda")
    x = torch.zeros(3, 512, dtype=torch.float32, device="cuda")
    big = torch.zeros(3, 1200, dtype=torch.float32, device="cuda")

    def status(call, code, text):
        assert call == code, (call, lib.pfft_last_error())
        assert text in lib.pfft_last_error().decode(), lib.pfft_last_error()

    def run(i=y.data_ptr(), o=x.data_ptr(), ns=3, nf=5, fp=fp, ip=ip, hop=64, lead=0, mode=0, ol=512, op=512, chunk=0, p=None):
        return lib.pfft_execute_istft(plan._plan if p is None else p, i, o, ns, nf, fp, ip, hop, lead, mode, ol, op, chunk)

    INVALID, UNSUPPORTED = 1, 2
    status(run(), INVALID, "no synthesis window has been set")
    cplx = pf.descriptor([n]).commit()
    status(run(p=cplx._plan), INVALID, "not of the REAL domain")
    status(lib.pfft_plan_set_synthesis_window(cplx._plan, None), INVALID, "not of the REAL domain")
    with pytest.raises(pf.invalid_configuration, match="not of the REAL domain"):
        cplx.istft(y, x, 64)
    with pytest.raises(pf.invalid_configuration, match="not of the REAL domain"):
        cplx.set_synthesis_window(None)
    info_before = bytes(plan.info())
    plan.set_synthesis_window(None)
    assert bytes(plan.info()) == info_before  # the plan info is the real plan's
    with pytest.raises(pf.invalid_configuration, match="no window has been set"):  # stft's window is another one
        plan.stft(x, y, 64)
    # frames of 256 at hop 64, 5 frames: positions 0 ... 512; lead 0: out_length 257 ... 512
    assert run() == 0
    status(run(i=None), INVALID, "null data pointer")
    status(run(o=None), INVALID, "null data pointer")
    status(run(ns=0), INVALID, "zero count")
    status(run(nf=0), INVALID, "zero count")
    status(run(ol=0), INVALID, "zero count")
    status(run(hop=0), INVALID, "hop 0")
    status(run(hop=257, ol=1200, op=1200), INVALID, "hop 257 above the frame length 256")
    assert run(hop=256, ol=1200, op=1200, o=big.data_ptr()) == 0
    status(run(lead=n), INVALID, "lead 256")
    status(run(mode=2), INVALID, "mode 2")
    status(run(fp=m), INVALID, "frame_pitch 128 below")
    status(run(ip=ip - 1), INVALID, "in_pitch 644 below")
    status(run(op=511), INVALID, "out_pitch 511 below out_length 512")
    status(run(ol=513, op=513), INVALID, "out_length 513 above (n_frames - 1) * hop + N - lead = 512")
    status(run(lead=1), INVALID, "out_length 512 above (n_frames - 1) * hop + N - lead = 511")
    assert run(lead=1, ol=511) == 0
    status(run(ol=256), INVALID, "frame 4 starts at sample 256")  # (F - 1) hop >= out_length + lead
    assert run(ol=257) == 0
    status(run(ol=156, lead=100), INVALID, "frame 4 starts at sample 256")
    assert run(ol=157, lead=100) == 0
    status(run(o=y.data_ptr()), INVALID, "overlap")  # in == out
    status(run(o=y.data_ptr() + 8 * (2 * ip + 4 * fp + m)), INVALID, "overlap")  # the last bin is the first sample
    # beyond the kernel's 32-bit byte offsets (nothing is launched: the pointers are never followed)
    far = y.data_ptr() + (1 << 44)
    status(run(ns=1, nf=64, fp=1 << 27, ip=1 << 33, hop=256, ol=64 * 256, op=64 * 256, o=far), UNSUPPORTED, "below 2^32")
    status(run(ns=1, nf=64, fp=1 << 24, ip=1 << 30, hop=256, ol=64 * 256, op=64 * 256, chunk=64, o=far), UNSUPPORTED, "4 GiB")
    status(run(ns=1, nf=1 << 23, ip=(1 << 23) * fp, hop=256, ol=1 << 31, op=1 << 31, chunk=1 << 23, o=far), UNSUPPORTED, "4 GiB")
    status(run(ns=1 << 20, nf=2048, ip=2048 * fp, ol=2048 * 64, op=2048 * 64, o=far), UNSUPPORTED, "2^31")
    plan.wait()
    # the binding: geometry bounds and overlapping tensors, before the library is called
    with pytest.raises(pf.invalid_configuration, match="frame 4 starts at sample 256"):
        plan.istft(y, x[:, :256], 64)
    with pytest.raises(pf.invalid_configuration, match="out_length 512 above"):
        plan.istft(y, x, 64, lead=1)
    both = torch.zeros(2 * 3 * 5 * 129 + 3 * 512, dtype=torch.float32, device="cuda")
    yb = torch.view_as_complex(both[:2 * 3 * 5 * 129].view(-1, 2)).view(3, 5, 129)
    with pytest.raises(pf.invalid_configuration, match="overlap"):
        plan.istft(yb, both[1000:1000 + 3 * 512].view(3, 512), 64)
    plan.istft(y, x, 64).wait()
    assert float(x.abs().max()) == 0.0
    assert plan.istft_chunk_frames(3, 5, 64) == 5


@pytest.mark.parametrize("prec,n", [("f32", 4096), ("f64", 6000)])
def test_dependencies_and_events(prec, n):
    G, pf, torch = _mods()
    rt, ct = _types(prec)
    m = n // 2
    plan, scale, fpw = _plan(pf, n, prec)
    rng = np.random.Generator(np.random.SFC64(5 * n))
    w = rng.uniform(0.5, 1, n).astype(rt)
    _set(plan, torch, w)
    hop, lead, frames = m, m, 7
    olen = (frames - 1) * hop + n - lead
    y = _bins(rng, 4, frames, m, ct)
    bits, _ = _launch(G, torch, plan, n, y, hop, lead, True, olen, 0, (prec, n, "plain call"))
    seen = {}

    def with_events(yv, xv):
        # the bins are written by another stream; the execute is ordered behind it by the event alone
        side = torch.cuda.Stream()
        staged = yv.clone()
        yv.zero_()
        torch.cuda.current_stream().synchronize()
        with torch.cuda.stream(side):
            yv.copy_(staged)
            dep = torch.cuda.Event()
            dep.record(side)
        ev = plan.istft(yv, xv, hop, lead=lead, normalize=True, dependencies=[dep])
        assert ev.native
        ev.wait()
        assert ev.is_complete()
        seen["bits"] = xv.cpu().numpy().copy()  # read right behind the event, before any other wait

    ebits, _ = _launch(G, torch, plan, n, y, hop, lead, True, olen, 0, (prec, n, "with events"), verb=with_events)
    H.check_unchanged(bits, ebits, what="istft with a dependency and a returned event")
    H.check_unchanged(bits, seen["bits"], what="the output behind the returned event")
    ola, env = _reference(scale, y, w, n, hop, lead, olen)
    _check(bits, ola / env, ct, n, (prec, n, "events"))
    yd = torch.from_numpy(y).cuda()
    x = torch.empty(4, olen, dtype=torch.from_numpy(np.zeros(0, dtype=rt)).dtype, device="cuda")
    ev = plan.istft(yd, x, hop, lead=lead, normalize=True, want_event=False)
    assert not ev.native
    ev.wait()
    H.check_unchanged(bits, x.cpu().numpy(), what="want_event=False")
