"""Short-time Fourier transform of REAL signals on the GPU (plan.set_window / plan.stft of a plan of the REAL domain:
stockham_wg_stft_kernel): every signal of every case against NumPy in double precision,
    np.pad(x, mode by pad) -> frames of N scalars every hop -> forward_scale * np.fft.rfft(w * frame)
and the project's two yardsticks unchanged: relative L2 per signal, all its frames together, within helpers.REL_L2_TOL, and
helpers.check_reference_rule with n = N.  Signals are uniform in [-1, 1].

One length per kernel shape, as in test_gpu_rfilter.py (M = 2, single-pass STAGED, TWL two-pass, FPW 16 / 4 / 2 / 1 with
TW_REGS, 32.16.16, lengths compiled when the window is set; every registered line of the kernel runs in
test_gpu_fused_registry.py).  Per length and pad mode the smallest geometries that can go
wrong: hop in {1 (N <= 128), N/4 + 1 made odd, N/2, N, N + 3} x lead in {0, N/2, the odd one of N/2 - 1 and N/2 + 1,
N - 1} x in_length odd and even, three signals and as many frames as the mode admits; a signal shorter than N and a last
frame whose only sample is x[L-1] (zeros); lead = in_length - 1 with in_length < N, so that both ends reflect inside one
frame (reflection); 1 signal (1-D tensors) and counts that put S * n_frames at 2 FPW - 1 and 2 FPW + 1 rows, as signals
of one frame and as frames of one signal.  The windows rotate through periodic Hann, a random window in [-1, 1] and None;
every third scenario runs on the scaled plan of the length (forward_scale = 0.5).

Every launch reads from and writes into gpu_utils.Guarded buffers with an ODD in_pitch, frame_pitch = M + 2 or M + 3 and
out_pitch above n_frames * frame_pitch: the guards, every element between the frames and between the signals and the
whole input must be unchanged, bit for bit, and the imaginary parts of bins 0 and M exactly 0.  Once per case the base
pointers are one scalar off 128-byte alignment.

With window None, hop = N, lead = 0 and in_length = F * N the transform is compute_forward of the same plan on the
reshaped signal: checked with the two yardsticks; whether it is also bit-identical is printed and recorded in DESIGN
3.1i (the same passes, the same untangle step; the multiplication by 1 is exact).

Measured on the MI355X (worst signal of every case of a length, both pad modes, all windows, relative L2): fp32 N=4
8.6e-08, 8 1.1e-07, 32 1.3e-07, 64 1.2e-07, 128 1.2e-07, 512 1.2e-07, 1024 1.2e-07, 4096 1.3e-07, 16384 1.4e-07, 2000
1.4e-07, 12000 1.4e-07; fp64 N=128 3.1e-16, 1024 3.4e-16, 8192 3.7e-16, 6000 4.5e-16.  No shape comes near REL_L2_TOL: by
Parseval the half spectrum carries at least half of N * ||w * frame||^2, so the measure is relative to the windowed data
itself, also for a frame that holds a single sample (accuracy).

No case is skipped."""
import numpy as np
import pytest

import helpers as H

pytestmark = pytest.mark.gpu

LENGTHS = {"f32": [4, 8, 32, 64, 128, 512, 1024, 4096, 16384, 2000, 12000], "f64": [128, 1024, 8192, 6000]}
CASES = [(p, n, pad) for p in ("f32", "f64") for n in LENGTHS[p] for pad in ("zero", "reflect")]
BATCH = (2, 3)  # signals x frames of the plan's own number_of_transforms (compute_forward in the None-window test)


def _mods():
    import gpu_utils as G
    import portfft_amd as pf
    return G, pf, G.torch_mod()


def _types(prec):
    return (np.float32, np.complex64) if prec == "f32" else (np.float64, np.complex128)


_plans = {}


def _plan(pf, n, prec, scaled=False):
    """(plan, forward_scale, fpw) of a length: committed once per process, the window is set per launch"""
    key = (n, prec, scaled)
    if key not in _plans:
        d = pf.real_descriptor(n, prec)
        d.number_of_transforms = BATCH[0] * BATCH[1]
        if scaled:
            d.forward_scale = 0.5
        plan = d.commit()
        _plans[key] = (plan, d.forward_scale, max(1, plan.info().dims[0].ffts_per_workgroup))
    return _plans[key]


def _windows(n, rt, rng):
    hann = (0.5 - 0.5 * np.cos(2 * np.pi * np.arange(n) / n)).astype(rt)  # periodic
    return [("hann", hann), ("random", rng.uniform(-1, 1, n).astype(rt)), ("none", None)]


def _reference(scale, x, w, n, hop, lead, pad, frames):
    """NumPy in double: pad by mode, frames, rfft of the windowed frames"""
    xd = x.astype(np.float64)
    length = x.shape[1]
    if pad == "zero":
        xe = np.pad(xd, ((0, 0), (lead, max(0, (frames - 1) * hop + n - lead - length))))
    else:
        xe = np.pad(xd, ((0, 0), (lead, lead)), mode="reflect")
    idx = np.arange(frames)[:, None] * hop + np.arange(n)[None, :]
    wd = np.ones(n) if w is None else w.astype(np.float64)
    return scale * np.fft.rfft(xe[:, idx] * wd, axis=-1)


_worst = {}


def _check(got, ref, ct, n, what):
    """got, ref: (signals, frames, bins)"""
    ns = got.shape[0]
    g = np.asarray(got).astype(np.complex128).reshape(ns, -1)
    r = np.asarray(ref).astype(np.complex128).reshape(ns, -1)
    err = np.linalg.norm(g - r, axis=1) / np.maximum(np.linalg.norm(r, axis=1), 1e-300)
    key = (np.dtype(ct).name, n)
    _worst[key] = max(_worst.get(key, 0.0), float(err.max()))
    print("%s: worst rel-L2 %.3e (signal %d)" % (what, float(err.max()), int(np.argmax(err))))
    assert np.all(err <= H.REL_L2_TOL[np.dtype(ct)]), (what, "signal", int(np.argmax(err)), float(err.max()))
    assert H.check_reference_rule(g, r.astype(ct), n), (what, "per-element reference rule")


def _odd(v):
    return v | 1


def _stft(G, torch, plan, scale, n, x, w, hop, lead, pad, frames, what, guard=None, verb=None, extra=2):
    """plan.stft of the signals x (numpy, (signals, in_length)) with the window w already set: buffers with an odd
    in_pitch, frame_pitch = M + extra and an out_pitch above the frames; write set, guards, unchanged input, exact zeros,
    every signal against the reference.  Returns the bins (numpy, (signals, frames, M + 1))."""
    ns, in_length = x.shape
    m = n // 2
    ct = np.complex64 if x.dtype == np.float32 else np.complex128
    in_pitch, frame_pitch = _odd(in_length + 3), m + extra
    out_pitch = frames * frame_pitch + 3
    guard = G.GUARD if guard is None else guard
    gin = G.Guarded(ns * in_pitch, torch.from_numpy(x[:0]).dtype, guard)
    gout = G.Guarded(ns * out_pitch, torch.from_numpy(np.zeros(0, dtype=ct)).dtype, guard)
    xin = gin.buf.view(ns, in_pitch)
    xin[:, :in_length].copy_(torch.from_numpy(x))
    before = gin.buf.cpu().numpy()
    xv = xin[:, :in_length]
    yv = gout.buf.view(ns, out_pitch)[:, :frames * frame_pitch].view(ns, frames, frame_pitch)[:, :, :m + 1]
    if ns == 1 and verb is None:  # (a single signal may come as a 1-D tensor)
        xv, yv = xv[0], yv[0]
    if verb is None:
        plan.stft(xv, yv, hop, lead=lead, pad=pad)
        plan.wait()
    else:
        verb(xv, yv)
    gin.check(str(what) + ": input")
    gout.check(str(what) + ": output")
    H.check_unchanged(before, gin.buf.cpu().numpy(), what=str(what) + ": the input")
    raw = gout.buf.cpu().numpy()
    idx = (np.arange(ns)[:, None, None] * out_pitch + np.arange(frames)[None, :, None] * frame_pitch +
           np.arange(m + 1)[None, None, :]).ravel()
    H.check_write_set(raw, idx, what=str(what) + ": output buffer")
    got = raw[idx].reshape(ns, frames, m + 1)
    assert np.all(got[:, :, 0].imag == 0) and np.all(got[:, :, m].imag == 0), (what, "imaginary parts of bins 0 and M")
    _check(got, _reference(scale, x, w, n, hop, lead, pad, frames), ct, n, what)
    return got


def _max_frames(n, length, hop, lead, pad):
    """the most frames the mode admits (include/portfft_amd.h)"""
    if pad == "zero":
        return (length + lead - 1) // hop + 1
    return (length + 2 * lead - n) // hop + 1


def _scenarios(n, fpw, pad):
    """(name, signals, in_length, hop, lead, frames, guard)"""
    m = n // 2
    hops = ([1] if n <= 128 else []) + [_odd(n // 4 + 1), m, n, n + 3]
    leads = sorted({0, m, m - 1 if (m - 1) % 2 else m + 1, n - 1})
    out = []
    first = True
    for hop in hops:
        for lead in leads:
            for parity in (1, 0):
                length = n + m + 3 + (1 - parity)  # n + m + 3 is odd for even m, so make the parity explicit
                length += (length % 2) != parity
                frames = _max_frames(n, length, hop, lead, pad)
                if hop == 1:
                    frames = min(frames, 2 * n)
                out.append(("hop %d lead %d in %d" % (hop, lead, length), 3, length, hop, lead, frames,
                            (65, 63) if first else None))
                first = False
    if pad == "zero":
        # a signal shorter than a frame; a last frame whose only sample is x[L-1]
        out.append(("shorter than a frame", 3, max(1, m - 1), n, 0, 1, None))
        hop = _odd(n // 4 + 1)
        for lead in (0, m):
            length = 2 * hop - lead + 1
            if length >= 1:
                out.append(("last frame holds x[L-1] only, lead %d" % lead, 3, length, hop, lead, 3, None))
    else:
        # lead = in_length - 1 with in_length < N: both ends reflect inside one frame
        out.append(("both ends reflect in one frame", 3, m, n, m - 1, 1, None))
        if n >= 8:
            out.append(("both ends reflect, two frames", 1, m, 1, m - 1, 2, None))
    # 1 signal (1-D tensors), and S * frames at 2 fpw - 1 and 2 fpw + 1 rows: signals of one frame, frames of one signal
    lead = m - 1 if (m - 1) % 2 else m + 1
    hop = _odd(n // 4 + 1)
    for rows in (2 * fpw - 1, 2 * fpw + 1):
        out.append(("%d signals of one frame" % rows, rows, n + 1, n, lead, 1, None))
        length = (rows - 1) * hop + n - 2 * lead + 1 if pad == "reflect" else (rows - 1) * hop - lead + 2
        length = max(length, lead + 1, 1)
        assert _max_frames(n, length, hop, lead, pad) >= rows
        out.append(("%d frames of one signal" % rows, 1, length, hop, lead, rows, None))
    return out


@pytest.mark.parametrize("prec,n,pad", CASES)
def test_stft_against_numpy(prec, n, pad):
    G, pf, torch = _mods()
    rt, ct = _types(prec)
    rng = np.random.Generator(np.random.SFC64(1000 * n + len(pad)))
    fpw = _plan(pf, n, prec)[2]
    windows = _windows(n, rt, rng)
    print("N=%d %s %s: fpw %d" % (n, prec, pad, fpw))
    seen = set()
    for i, (name, ns, length, hop, lead, frames, guard) in enumerate(_scenarios(n, fpw, pad)):
        plan, scale, _ = _plan(pf, n, prec, scaled=i % 3 == 2)
        wname, w = windows[i % 3] if i % 9 < 6 else windows[(i + 1) % 3]  # (every window meets both plans)
        plan.set_window(None if w is None else torch.from_numpy(w).cuda())
        x = rng.uniform(-1, 1, (ns, length)).astype(rt)
        _stft(G, torch, plan, scale, n, x, w, hop, lead, pad, frames,
              (prec, n, pad, name, wname, "signals", ns, "frames", frames, "scale", scale), guard=guard, extra=2 + i % 2)
        seen.add((length % 2, wname))
    assert {p for p, _ in seen} == {0, 1} and {w for _, w in seen} == {"hann", "random", "none"}, seen
    print("worst rel-L2 so far: %s" % _worst)


@pytest.mark.parametrize("prec,n", [(p, n) for p in ("f32", "f64") for n in LENGTHS[p]])
def test_window_none_is_compute_forward(prec, n):
    """hop = N, lead = 0, in_length = F * N, all ones: the rows of the plan's own R2C transform"""
    G, pf, torch = _mods()
    rt, ct = _types(prec)
    m = n // 2
    ns, frames = BATCH
    rng = np.random.Generator(np.random.SFC64(17 * n))
    x = rng.uniform(-1, 1, (ns, frames * n)).astype(rt)
    same = []
    for scaled in (False, True):
        plan, scale, _ = _plan(pf, n, prec, scaled)
        plan.set_window(None)
        xd = torch.from_numpy(x).cuda()
        y = torch.full((ns * frames * (m + 1),), H.PADDING_VALUE, dtype=torch.from_numpy(np.zeros(0, dtype=ct)).dtype, device="cuda")
        plan.compute_forward(xd.reshape(-1), y).wait()
        rows = y.cpu().numpy().reshape(ns, frames, m + 1)
        for pad in ("zero", "reflect"):
            got = _stft(G, torch, plan, scale, n, x, None, n, 0, pad, frames, (prec, n, pad, "window None, whole frames", scale))
            _check(got, rows, ct, n, (prec, n, pad, "against compute_forward"))
            same.append(bool(np.array_equal(got.view(rt), rows.view(rt))))
    print("N=%d %s: bit-identical to compute_forward: %s" % (n, prec, same))  # (recorded in DESIGN 3.1i, not a bound)


@pytest.mark.parametrize("prec,n", [(p, n) for p in ("f32", "f64") for n in LENGTHS[p]])
def test_the_window_is_replaced_between_executes(prec, n):
    G, pf, torch = _mods()
    rt, ct = _types(prec)
    m = n // 2
    plan, scale, _ = _plan(pf, n, prec)
    rng = np.random.Generator(np.random.SFC64(23 * n))
    (_, hann), (_, rand), _ = _windows(n, rt, rng)
    x = rng.uniform(-1, 1, (2, 2 * n + 5)).astype(rt)
    hop, lead = _odd(n // 4 + 1), m
    frames = _max_frames(n, x.shape[1], hop, lead, "reflect")
    wd = torch.from_numpy(hann).cuda()
    plan.set_window(wd)
    wd.fill_(7)  # the plan owns a copy: later writes do not matter
    a = _stft(G, torch, plan, scale, n, x, hann, hop, lead, "reflect", frames, (prec, n, "first window"))
    plan.set_window(torch.from_numpy(rand).cuda())
    b = _stft(G, torch, plan, scale, n, x, rand, hop, lead, "reflect", frames, (prec, n, "second window"))
    assert not np.array_equal(a, b)


def test_a_copy_keeps_its_window():
    G, pf, torch = _mods()
    n, prec = 1024, "f32"
    rt, ct = _types(prec)
    rng = np.random.Generator(np.random.SFC64(5))
    (_, hann), (_, rand), _ = _windows(n, rt, rng)
    plan = pf.real_descriptor(n, prec).commit()
    x = rng.uniform(-1, 1, (3, 3 * n + 1)).astype(rt)
    hop, lead = 257, 512
    frames = _max_frames(n, x.shape[1], hop, lead, "zero")
    fresh = plan.copy()  # made before any window: resolves the kernel itself, shares nothing
    plan.set_window(torch.from_numpy(hann).cuda())
    bits = _stft(G, torch, plan, 1.0, n, x, hann, hop, lead, "zero", frames, "original, hann")
    clone = plan.copy()  # shares the window
    H.check_unchanged(bits, _stft(G, torch, clone, 1.0, n, x, hann, hop, lead, "zero", frames, "clone, shared window"),
                      what="a clone transforms with the shared window")
    plan.set_window(torch.from_numpy(rand).cuda())
    _stft(G, torch, plan, 1.0, n, x, rand, hop, lead, "zero", frames, "original, second window")
    H.check_unchanged(bits, _stft(G, torch, clone, 1.0, n, x, hann, hop, lead, "zero", frames, "clone afterwards"),
                      what="the clone keeps its window")
    with pytest.raises(pf.invalid_configuration, match="no window has been set"):
        fresh.stft(torch.from_numpy(x).cuda(), torch.zeros(3, frames, n // 2 + 1, dtype=torch.complex64, device="cuda"), hop, lead=lead)
    fresh.set_window(None)
    _stft(G, torch, fresh, 1.0, n, x, None, hop, lead, "zero", frames, "a copy made before any window")


@pytest.mark.parametrize("prec,n", [("f32", 512), ("f64", 6000), ("f32", 16384)])
def test_many_trips_of_the_persistent_loop(prec, n):
    """more (signal, frame) rows than the grid holds work-groups, on a plan that also convolves"""
    G, pf, torch = _mods()
    rt, ct = _types(prec)
    m = n // 2
    plan = pf.real_convolution_descriptor(n, prec).commit()
    fpw = max(1, plan.info().dims[0].ffts_per_workgroup)
    rng = np.random.Generator(np.random.SFC64(7 * n))
    w = rng.uniform(-1, 1, n).astype(rt)
    plan.set_window(torch.from_numpy(w).cuda())
    ns, hop, lead = 5, _odd(n // 4 + 1), m
    frames = (1500 * fpw) // ns + 1
    length = (frames - 1) * hop + n - 2 * lead + 3
    x = rng.uniform(-1, 1, (ns, length)).astype(rt)
    gout = G.Guarded(ns * frames * (m + 1), torch.from_numpy(np.zeros(0, dtype=ct)).dtype)
    plan.stft(torch.from_numpy(x).cuda(), gout.buf.view(ns, frames, m + 1), hop, lead=lead, pad="reflect")
    plan.wait()
    gout.check("many trips: output")
    _check(gout.buf.cpu().numpy().reshape(ns, frames, m + 1), _reference(1.0, x, w, n, hop, lead, "reflect", frames), ct, n,
           (prec, n, "many trips"))


def test_refusals_name_the_cause():
    G, pf, torch = _mods()
    from portfft_amd import _lib
    lib = _lib.lib
    n, m = 256, 128
    plan = pf.real_descriptor(n).commit()
    x = torch.zeros(3, 1000, dtype=torch.float32, device="cuda")
    y = torch.zeros(3, 5, m + 1, dtype=torch.complex64, device="cuda")
    fp, op = m + 1, 5 * (m + 1)

    def status(call, code, text):
        assert call == code, (call, lib.pfft_last_error())
        assert text in lib.pfft_last_error().decode(), lib.pfft_last_error()

    def run(i=x.data_ptr(), o=y.data_ptr(), ns=3, il=1000, ip=1000, hop=64, lead=0, pad=0, nf=5, fp=fp, op=op, p=None):
        return lib.pfft_execute_stft(plan._plan if p is None else p, i, o, ns, il, ip, hop, lead, pad, nf, fp, op)

    INVALID, UNSUPPORTED = 1, 2
    # no window yet; a plan that is not REAL
    status(run(), INVALID, "no window has been set")
    with pytest.raises(pf.invalid_configuration, match="no window has been set"):
        plan.stft(x, y, 64)
    cplx = pf.descriptor([n]).commit()
    status(run(p=cplx._plan), INVALID, "not of the REAL domain")
    status(lib.pfft_plan_set_window(cplx._plan, None), INVALID, "not of the REAL domain")
    with pytest.raises(pf.invalid_configuration, match="not of the REAL domain"):
        cplx.stft(x, y, 64)
    with pytest.raises(pf.invalid_configuration, match="not of the REAL domain"):
        cplx.set_window(None)
    info_before = bytes(plan.info())
    plan.set_window(None)
    assert bytes(plan.info()) == info_before  # the plan info is the real plan's
    # execute_stft: what the C entry point refuses, each bound at its first refused value
    status(run(i=None), INVALID, "null data pointer")
    status(run(o=None), INVALID, "null data pointer")
    status(run(ns=0), INVALID, "zero count")
    status(run(il=0, ip=0), INVALID, "zero count")
    status(run(nf=0), INVALID, "zero count")
    status(run(hop=0), INVALID, "hop 0")
    status(run(lead=n), INVALID, "lead 256")
    status(run(pad=2), INVALID, "pad_mode 2")
    status(run(ip=999), INVALID, "in_pitch 999 below in_length 1000")
    status(run(fp=m), INVALID, "frame_pitch 128 below")
    status(run(op=op - 1), INVALID, "out_pitch 644 below")
    status(run(hop=250), INVALID, "frame 4 starts at sample 1000")  # zeros: (F - 1) hop >= L + lead
    assert run(hop=249) == 0
    status(run(hop=282, lead=128), INVALID, "frame 4 starts at sample 1128")
    assert run(hop=281, lead=128) == 0
    status(run(il=100, ip=100, lead=100, pad=1, nf=1), INVALID, "lead 100 above in_length - 1 = 99")  # reflection
    assert run(il=100, ip=100, lead=99, pad=1, nf=1) == 0
    status(run(hop=187, pad=1), INVALID, "frame 4 ends at sample 1004")  # (F - 1) hop + N > L + 2 lead
    assert run(hop=186, pad=1) == 0
    status(run(hop=251, lead=128, pad=1), INVALID, "frame 4 ends at sample 1260")
    assert run(hop=250, lead=128, pad=1) == 0
    status(run(o=x.data_ptr()), INVALID, "overlap")  # in == out
    status(run(o=x.data_ptr() + 4 * 2999), INVALID, "overlap")  # the last input scalar is the first output
    # beyond the kernel's 32-bit byte offsets (nothing is launched: the pointers are never followed)
    far = x.data_ptr() + (1 << 44)
    status(run(ns=1, il=1 << 30, ip=1 << 30, o=far), UNSUPPORTED, "4 GiB")
    status(run(ns=16, ip=1 << 29, nf=1, op=fp, o=far), UNSUPPORTED, "4 GiB")  # fpw rows cross signals 4 GiB apart
    status(run(ns=16, nf=1, op=1 << 29, o=far), UNSUPPORTED, "4 GiB")  # ... whose output rows are 4 GiB apart
    status(run(ns=1 << 20, il=2048 * 64, ip=2048 * 64, nf=2048, op=2048 * fp, o=far), UNSUPPORTED, "2^31")
    plan.wait()
    # the binding: overlapping tensors, geometry bounds, before the library is called
    with pytest.raises(pf.invalid_configuration, match="frame 4 starts at sample 1000"):
        plan.stft(x, y, 250)
    with pytest.raises(pf.invalid_configuration, match="frame 4 ends at sample 1004"):
        plan.stft(x, y, 187, pad="reflect")
    both = torch.zeros(3 * 1000 + 8, dtype=torch.float32, device="cuda")
    with pytest.raises(pf.invalid_configuration, match="overlap"):
        plan.stft(both[:3000].view(3, 1000), torch.view_as_complex(both[1000:1000 + 2 * 3 * 129].view(-1, 2)).view(3, 1, 129), 64)
    plan.stft(x, y, 64).wait()
    assert float(y.abs().max()) == 0.0


@pytest.mark.parametrize("prec,n", [("f32", 4096), ("f64", 6000)])
def test_dependencies_and_events(prec, n):
    G, pf, torch = _mods()
    rt, ct = _types(prec)
    plan, scale, _ = _plan(pf, n, prec)
    rng = np.random.Generator(np.random.SFC64(5 * n))
    x = rng.uniform(-1, 1, (4, 2 * n + 11)).astype(rt)
    w = rng.uniform(-1, 1, n).astype(rt)
    plan.set_window(torch.from_numpy(w).cuda())
    hop, lead = n // 2, n // 2
    frames = _max_frames(n, x.shape[1], hop, lead, "reflect")
    bits = _stft(G, torch, plan, scale, n, x, w, hop, lead, "reflect", frames, (prec, n, "plain call"))
    seen = {}

    def with_events(xv, yv):
        # the input is written by another stream; the execute is ordered behind it by the event alone
        side = torch.cuda.Stream()
        staged = xv.clone()
        xv.zero_()
        torch.cuda.current_stream().synchronize()
        with torch.cuda.stream(side):
            xv.copy_(staged)
            dep = torch.cuda.Event()
            dep.record(side)
        ev = plan.stft(xv, yv, hop, lead=lead, pad="reflect", dependencies=[dep])
        assert ev.native
        ev.wait()
        assert ev.is_complete()
        seen["bits"] = yv.cpu().numpy().copy()  # read right behind the event, before any other wait

    ebits = _stft(G, torch, plan, scale, n, x, w, hop, lead, "reflect", frames, (prec, n, "with events"), verb=with_events)
    H.check_unchanged(bits, ebits, what="stft with a dependency and a returned event")
    H.check_unchanged(bits, seen["bits"], what="the output behind the returned event")
    xd = torch.from_numpy(x).cuda()
    y = torch.empty(4, frames, n // 2 + 1, dtype=torch.from_numpy(np.zeros(0, dtype=ct)).dtype, device="cuda")
    ev = plan.stft(xd, y, hop, lead=lead, pad="reflect", want_event=False)
    assert not ev.native
    ev.wait()
    _check(y.cpu().numpy(), _reference(scale, x, w, n, hop, lead, "reflect", frames), ct, n, (prec, n, "want_event=False"))
