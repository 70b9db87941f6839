"""fp16 storage on the GPU (PFFT_PRECISION_F16: IEEE binary16 data, fp32 arithmetic).

Accuracy criterion: Y = the exact (float64) DFT of the fp16 input, times the scale.  The kernels compute in fp32 and
round once, on the store, so every output component is round16(Y) or a neighbour:
  per component  |out - Y| <= ulp16(Y) + 1e-6 * max|Y| of the transform,
  per transform  rel-L2(out, Y) <= 1.5 * e_round + 1e-6, e_round = rel-L2(round16(Y), Y).
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import portfft_amd as pf

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAD = 3.0  # padding value outside the addressed elements (exact in fp16)
FWD, BWD = pf.direction.FORWARD, pf.direction.BACKWARD


def _torch():
    import torch
    assert torch.cuda.is_available(), "the -m gpu tests need a GPU"
    return torch


def _input(rng, n, batch):
    """uniform(-1, 1) complex values that are exact in fp16: (batch, n) complex128"""
    re = rng.uniform(-1, 1, (batch, n)).astype(np.float16).astype(np.float64)
    im = rng.uniform(-1, 1, (batch, n)).astype(np.float16).astype(np.float64)
    return re + 1j * im


def _exact(x, direction, scale):
    n = x.shape[-1]
    y = np.fft.fft(x, axis=-1) if direction == FWD else np.fft.ifft(x, axis=-1) * n
    return y * scale


def _round16(y):
    return y.real.astype(np.float16).astype(np.float64) + 1j * y.imag.astype(np.float16).astype(np.float64)


def _ulp16(v):
    return np.spacing(np.abs(v).astype(np.float16)).astype(np.float64)


def check_accuracy(out, y, what):
    """out, y: (batch, n) complex128"""
    for b in range(y.shape[0]):
        o, e = out[b], y[b]
        assert np.all(np.isfinite(o)), (what, b, "non-finite output")
        slack = 1e-6 * np.max(np.abs(e))
        bad_re = np.abs(o.real - e.real) > _ulp16(e.real) + slack
        bad_im = np.abs(o.imag - e.imag) > _ulp16(e.imag) + slack
        assert not bad_re.any() and not bad_im.any(), (what, b, int(bad_re.sum()), int(bad_im.sum()))
        den = np.linalg.norm(e)
        if den == 0:
            assert np.all(o == 0), (what, b)
            continue
        e_round = np.linalg.norm(_round16(e) - e) / den
        err = np.linalg.norm(o - e) / den
        assert err <= 1.5 * e_round + 1e-6, (what, b, err, e_round)


def _desc(n, batch=1, prec="f16", split=False, in_place=False, off_in=0, off_out=0, fwd_scale=1.0, bwd_scale=1.0):
    d = pf.descriptor([n], prec)
    d.number_of_transforms = batch
    d.complex_storage = pf.complex_storage.SPLIT_COMPLEX if split else pf.complex_storage.INTERLEAVED_COMPLEX
    d.placement = pf.placement.IN_PLACE if in_place else pf.placement.OUT_OF_PLACE
    d.forward_offset, d.backward_offset = off_in, off_out
    d.forward_scale, d.backward_scale = fwd_scale, bwd_scale
    return d


GUARD = 128  # fp16 scalars of padding in front of and behind every buffer (64 interleaved elements)


def _guarded(torch, host):
    """the host tensor copied into the middle of a device allocation with GUARD scalars of padding on either side"""
    alloc = torch.full((GUARD + host.numel() + GUARD,), PAD, dtype=host.dtype, device="cuda")
    alloc[GUARD:GUARD + host.numel()].copy_(host)
    return alloc, alloc[GUARD:GUARD + host.numel()]


def _check_guards(allocs, before, what):
    """both guards of every allocation untouched; `before`: the host copies of the inputs of an out-of-place execute,
    which must come back unchanged, bit for bit"""
    import helpers as H
    for i, a in enumerate(allocs):
        h = a.cpu().numpy()
        H.check_guards(h, GUARD, h.size - 2 * GUARD, pad=PAD, what="%s buffer %d" % (what, i))
    for i, (a, b) in enumerate(before):
        H.check_unchanged(b.numpy(), a[GUARD:GUARD + b.numel()].cpu().numpy(), what="%s: input %d" % (what, i))


def run_half(plan, desc, direction, x, real_view=False):
    """x: (batch, n) complex128, exact in fp16.  Returns (out (batch, n) complex128, the whole output buffer(s) as
    float64 for the padding checks, the output offset).  Every buffer lies between guard bands, which must stay
    untouched; an out-of-place execute must leave its input alone."""
    torch = _torch()
    n, batch = desc.lengths[0], desc.number_of_transforms
    off_in = desc.get_offset(direction)
    off_out = desc.get_offset(pf.inv(direction))
    split = desc.complex_storage == pf.complex_storage.SPLIT_COMPLEX
    in_place = desc.placement == pf.placement.IN_PLACE
    n_in, n_out = desc.get_input_count(direction), desc.get_output_count(direction)
    size = max(n_in, n_out) if in_place else n_in
    fn = plan.compute_forward if direction == FWD else plan.compute_backward
    flat = x.reshape(-1)
    if split:
        planes, hosts = [], []
        for part in (flat.real, flat.imag):
            t = torch.full((size,), PAD, dtype=torch.float16)
            t[off_in:off_in + n * batch] = torch.from_numpy(part.astype(np.float16))
            planes.append(_guarded(torch, t))
            hosts.append(t)
        if in_place:
            fn(*[p for _, p in planes]).wait()
            outs = [p for _, p in planes]
            _check_guards([a for a, _ in planes], [], "in place split")
        else:
            oal = [_guarded(torch, torch.full((n_out,), PAD, dtype=torch.float16)) for _ in range(2)]
            outs = [o for _, o in oal]
            fn(planes[0][1], planes[1][1], outs[0], outs[1]).wait()
            _check_guards([a for a, _ in planes + oal], [(a, h) for (a, _), h in zip(planes, hosts)], "split")
        re, im = (o.cpu().numpy().astype(np.float64) for o in outs)
        full = (re, im)
        vals = re[off_out:off_out + n * batch] + 1j * im[off_out:off_out + n * batch]
    else:
        t = torch.full((2 * size,), PAD, dtype=torch.float16)
        inter = np.empty(2 * n * batch, dtype=np.float16)
        inter[0::2], inter[1::2] = flat.real, flat.imag
        t[2 * off_in:2 * (off_in + n * batch)] = torch.from_numpy(inter)
        host, (talloc, t) = t, _guarded(torch, t)
        arg = (lambda u: u) if real_view else (lambda u: u.view(torch.complex32))
        if in_place:
            fn(arg(t)).wait()
            o = t
            _check_guards([talloc], [], "in place interleaved")
        else:
            oalloc, o = _guarded(torch, torch.full((2 * n_out,), PAD, dtype=torch.float16))
            fn(arg(t), arg(o)).wait()
            _check_guards([talloc, oalloc], [(talloc, host)], "interleaved")
        a = o.cpu().numpy().astype(np.float64)
        full = (a,)
        seg = a[2 * off_out:2 * (off_out + n * batch)]
        vals = seg[0::2] + 1j * seg[1::2]
    return vals.reshape(batch, n), full, off_out


def check_padding(full, off_out, count, split):
    for a in full:
        lo, hi = (off_out, off_out + count) if split else (2 * off_out, 2 * (off_out + count))
        assert np.all(a[:lo] == PAD) and np.all(a[hi:] == PAD), "the padding outside the output was overwritten"


# registered (kernels_f16.hip) and runtime-specialised lengths: 3 * 2^9, 5 * 2^7, 10^4, 7^4, 37 * 8, and one of the fp32
# register-resident band (24000 = 32.30.25 ... on a 1024-lane work-group)
REGISTERED = [2, 16, 64, 256, 1024, 4096, 8192, 16384, 32768]
RUNTIME = [1536, 640, 10000, 2401, 296, 24000]

# (split, in_place, direction, batch, off_in, off_out, scale, real_view): one variant per length, rotating
VARIANTS = [
    (True, False, BWD, 33, 0, 0, 1.0, False),
    (False, True, FWD, 3, 5, 5, 0.5, False),
    (True, True, BWD, 1, 7, 7, 1.0, False),
    (False, False, BWD, 33, 3, 11, 1.0, True),
    (True, False, FWD, 3, 2, 9, 0.25, False),
    (False, True, BWD, 1, 0, 0, 2.0, True),
]


@pytest.mark.parametrize("n", REGISTERED + RUNTIME)
def test_half_parity(n):
    rng = np.random.Generator(np.random.SFC64(n))
    torch = _torch()
    # 1) interleaved, out of place, forward, batch 3, with 1/N: against the exact DFT and against the fp32 plan
    d = _desc(n, 3, fwd_scale=1.0 / n)
    plan = d.commit()
    x = _input(rng, n, 3)
    out, full, off = run_half(plan, d, FWD, x)
    check_accuracy(out, _exact(x, FWD, 1.0 / n), ("f16", n))
    check_padding(full, off, 3 * n, False)
    d32 = _desc(n, 3, prec="f32", fwd_scale=1.0 / n)
    xin = torch.from_numpy(x.reshape(-1).astype(np.complex64)).cuda()
    y32 = torch.empty_like(xin)
    d32.commit().compute_forward(xin, y32).wait()
    ref = _round16(y32.cpu().numpy().astype(np.complex128)).reshape(3, n)
    close = (np.abs(out.real - ref.real) <= _ulp16(ref.real)) & (np.abs(out.imag - ref.imag) <= _ulp16(ref.imag))
    assert close.mean() >= 0.999, ("f16 vs rounded fp32 plan", n, close.mean())
    # 2) one rotating variant: storage, placement, direction, batch, offsets, scale
    split, in_place, direction, batch, off_in, off_out, scale, real_view = VARIANTS[(REGISTERED + RUNTIME).index(n) % len(VARIANTS)]
    kw = dict(fwd_scale=scale) if direction == FWD else dict(bwd_scale=scale)
    fo, bo = (off_in, off_out) if direction == FWD else (off_out, off_in)
    d = _desc(n, batch, split=split, in_place=in_place, off_in=fo, off_out=bo, **kw)
    x = _input(rng, n, batch)
    out, full, off = run_half(d.commit(), d, direction, x, real_view)
    check_accuracy(out, _exact(x, direction, scale), ("f16 variant", n, split, in_place, int(direction), batch))
    if not in_place:
        check_padding(full, off, batch * n, split)


def test_half_ragged_batch_on_the_prefetch_kernel():
    """N = 4096 (stockham_wg_prefetch_half_kernel) at a batch around 1000 that leaves a ragged last round, both
    directions, both storages"""
    rng = np.random.Generator(np.random.SFC64(1001))
    n, batch = 4096, 1001
    x = _input(rng, n, batch)
    for split in (False, True):
        for direction in (FWD, BWD):
            d = _desc(n, batch, split=split, fwd_scale=1.0 / n)
            out, full, off = run_half(d.commit(), d, direction, x)
            scale = 1.0 / n if direction == FWD else 1.0
            pick = [0, 1, 500, 999, 1000]
            check_accuracy(out[pick], _exact(x[pick], direction, scale), ("ragged", split, int(direction)))
            check_padding(full, off, batch * n, split)


def test_scale_is_applied_before_rounding():
    """constant 4.0 at N = 32768: unscaled, DC would be 131072 (beyond the fp16 maximum 65504); with forward_scale = 1/N
    it is exactly 4.0 and every other bin is (nearly) zero"""
    torch = _torch()
    n = 32768
    d = _desc(n, 1, fwd_scale=1.0 / n)
    x = torch.full((2 * n,), 0.0, dtype=torch.float16, device="cuda")
    x[0::2] = 4.0
    y = torch.empty_like(x)
    d.commit().compute_forward(x.view(torch.complex32), y.view(torch.complex32)).wait()
    a = y.cpu().numpy().astype(np.float64)
    assert np.all(np.isfinite(a))
    assert a[0] == 4.0 and a[1] == 0.0
    assert np.max(np.abs(a[2:])) <= 1e-5


def test_plan_info_is_the_fp32_plans():
    for n in (64, 4096, 16384, 32768, 2401, 24000):
        i16, i32 = _desc(n, 2).commit().info(), _desc(n, 2, prec="f32").commit().info()
        a, b = i16.dims[0], i32.dims[0]
        assert (a.tier, a.workgroup_size, a.ffts_per_workgroup) == (b.tier, b.workgroup_size, b.ffts_per_workgroup), n
        assert list(a.factors[:a.n_factors]) == list(b.factors[:b.n_factors]), n
        assert i16.launches[0] == i16.launches[1] == 1
        assert i16.twiddle_bytes == i32.twiddle_bytes, n


def test_one_gib_buffer_sampled():
    """N = 4096 x 65536: 1 GiB per fp16 buffer, sampled transforms against the exact DFT"""
    torch = _torch()
    n, batch = 4096, 65536
    d = _desc(n, batch, fwd_scale=1.0 / n)
    x = torch.empty((batch, 2 * n), dtype=torch.float16, device="cuda").uniform_(-1, 1)
    y = torch.empty_like(x)
    d.commit().compute_forward(x.view(torch.complex32), y.view(torch.complex32)).wait()
    pick = [0, 1, 12345, 40000, 65534, 65535]
    xs = x[pick].cpu().numpy().astype(np.float64)
    ys = y[pick].cpu().numpy().astype(np.float64)
    del x, y
    check_accuracy(ys[:, 0::2] + 1j * ys[:, 1::2], _exact(xs[:, 0::2] + 1j * xs[:, 1::2], FWD, 1.0 / n), "1 GiB")


@pytest.mark.parametrize("n", [1 << 20, 67, 4 * 67])
def test_lengths_without_a_one_kernel_plan_are_unsupported_at_commit(n):
    d = _desc(n)
    d.validate()
    with pytest.raises(pf.unsupported_configuration, match="fp16"):
        d.commit()


def test_without_runtime_specialisation():
    """PFFT_JIT=0 (child process): the registered N = 4096 runs, an unregistered length is unsupported"""
    code = (
        "import numpy as np, torch, portfft_amd as pf\n"
        "d = pf.descriptor([4096], 'f16')\n"
        "x = torch.ones(2 * 4096, dtype=torch.float16, device='cuda')\n"
        "y = torch.empty_like(x)\n"
        "d.commit().compute_forward(x, y).wait()\n"
        "assert float(y[0]) == 4096.0 and float(y[1]) == 4096.0, y[:4]\n"
        "try:\n"
        "    pf.descriptor([1536], 'f16').commit()\n"
        "    raise SystemExit('1536 committed without the runtime compiler')\n"
        "except pf.unsupported_configuration as e:\n"
        "    assert 'PFFT_JIT=0' in str(e), e\n"
        "print('jit0 OK')\n")
    env = dict(os.environ, PFFT_JIT="0", PYTHONPATH=ROOT)
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "jit0 OK" in p.stdout


def test_dependencies_and_events():
    torch = _torch()
    rng = np.random.Generator(np.random.SFC64(7))
    n, batch = 1024, 33
    d = _desc(n, batch, bwd_scale=1.0 / n)
    plan = d.commit()
    x = _input(rng, n, batch)
    inter = np.empty(2 * n * batch, dtype=np.float16)
    inter[0::2], inter[1::2] = x.reshape(-1).real, x.reshape(-1).imag
    xt = torch.from_numpy(inter).cuda().view(torch.complex32)
    yt, zt = torch.empty_like(xt), torch.empty_like(xt)
    ev = plan.compute_forward(xt, yt)
    ev2 = plan.compute_backward(yt, zt, dependencies=[ev])
    ev2.wait()
    assert ev.is_complete() and ev2.is_complete()
    z = zt.view(torch.float16).cpu().numpy().astype(np.float64)
    back = (z[0::2] + 1j * z[1::2]).reshape(batch, n)
    err = np.linalg.norm(back - x) / np.linalg.norm(x)
    assert err < 1e-3, err


def test_wrong_dtypes_are_invalid():
    torch = _torch()
    n = 256
    plan = _desc(n, 2).commit()
    good = torch.zeros(2 * n, dtype=torch.complex32, device="cuda")
    for bad in (torch.complex64, torch.float32, torch.bfloat16):
        buf = torch.zeros(2 * n * 2, dtype=bad, device="cuda")
        with pytest.raises(pf.invalid_configuration):
            plan.compute_forward(buf, good)
        with pytest.raises(pf.invalid_configuration):
            plan.compute_forward(good, buf)
    ds = _desc(n, 2, split=True)
    sp = ds.commit()
    planes = [torch.zeros(2 * n, dtype=torch.float16, device="cuda") for _ in range(4)]
    sp.compute_forward(*planes).wait()
    with pytest.raises(pf.invalid_configuration):
        sp.compute_forward(torch.zeros(2 * n, dtype=torch.float32, device="cuda"), *planes[1:])
