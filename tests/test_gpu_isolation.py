"""What a transform may depend on: every case runs one committed plan twice on freshly made buffers and compares the two
whole output buffers with helpers.check_isolated.

                                                                   clean run          poisoned run
  guards, input gaps, offset prefix, pitch gaps                    PADDING_VALUE      POISON
  the rows / signals / frames / samples named poisoned             uniform noise      POISON (both components)
  the output buffer before the call, guards and gaps included      PADDING_VALUE      POISON
  everything else                                                  the same seeded noise in both

POISON is a quiet NaN written by its bit pattern (helpers.POISON).  Every scalar of an output that must not depend on a
poisoned value is bit-identical in the two runs; every output that must depend on one is non-finite (the transforms of a
poisoned row: in every scalar).  The property is exact -- the library is built without fast-math, so NaN propagates by
IEEE rules -- and no tolerance is involved.  In both runs the guards, the write set and the unchanged input of an
out-of-place execute are checked with that run's padding, and the clean run is held to the verb's usual reference, so
bit-identity is not agreement between two wrong results.

A value that is read and multiplied by an exact zero -- zero extension by a 0/1 mask, a dead row added as 0 * garbage, a
read-modify-write of the output -- passes every other yardstick of the suite and fails here (test_check_helpers.py plants
each of them into a NumPy model).  The taint sets come from the definitions in include/portfft_amd.h
(helpers.taint_frames, taint_samples, taint_filter; test_isolation_reference.py holds them against the NumPy references).
For `filter` the overlap-save segment is the unit of work: outside every segment whose window holds the poisoned sample
the outputs are bit-identical (permitted), inside the mathematical cone they are non-finite (required), in between
nothing is asked.

Poisoned rows of a batch: index 1 and batch - 2, so the first and the last transform are clean and each has a poisoned
neighbour in its own work-group or column group.  Batches: 2 FPW + 1 (FPW from plan.info()), 3 from 2^16 points on.
The lengths are one per kernel shape, from the tables of the verbs' own test files.  The complex overlap-save filter and
circular convolution exist up to fp32 N = 8192 / fp64 N = 4096 (include/portfft_amd.h), so their lists end there; padded
distances exist up to the LDS-resident lengths, and above them the commit's refusal is what is asserted.
prepare_dct and prepare_dct4 take no array; their verbs run in the real-row cases.

No case is skipped; an unsupported_configuration is a failure."""
import os
import time

import numpy as np
import pytest

import helpers as H

pytestmark = pytest.mark.gpu

F, B = H.FORWARD, H.BACKWARD
CLEAN, POISONED = H.PADDING_VALUE, H.POISON
LDS_RESIDENT = {"f32": 16384, "f64": 8192}  # the longest one-work-group plans that take strides, distances and offsets

_slowest = [0.0, ""]


@pytest.fixture(autouse=True)
def _timed(request):
    t0 = time.perf_counter()
    yield
    dt = time.perf_counter() - t0
    if dt > _slowest[0]:
        _slowest[:] = [dt, request.node.name]
    print("%s: %.2f s; slowest case so far %.2f s (%s)" % (request.node.name, dt, _slowest[0], _slowest[1]))


def _mods():
    import gpu_utils as G
    import portfft_amd as pf
    return G, pf, G.torch_mod()


def _types(prec):
    return (np.float32, np.complex64) if prec == "f32" else (np.float64, np.complex128)


def _odd(v):
    return v | 1


def _fpw(plan):
    return max(1, plan.info().dims[0].ffts_per_workgroup)


def _poisoned_rows(batch):
    assert batch >= 3
    return sorted({1, batch - 2})


def _uniform(rng, shape, dtype):
    dtype = np.dtype(dtype)
    if dtype.kind == "c":
        rt = np.float32 if dtype == np.complex64 else np.float64
        return (rng.uniform(-1, 1, shape).astype(rt) + 1j * rng.uniform(-1, 1, shape).astype(rt)).astype(dtype)
    return rng.uniform(-1, 1, shape).astype(dtype)


def _locate(idx, names=("row", "element")):
    """locate= of check_isolated from the index array [rows, elements] of an output domain"""
    flat = idx.reshape(idx.shape[0], -1)

    def where(p):
        r, e = np.argwhere(flat == p)[0]
        return "(%s %d, %s %d)" % (names[0], r, names[1], e)
    return where


def _rel_l2_rows(got, ref, ct, n, what):
    got = np.asarray(got).astype(np.complex128).reshape(len(ref), -1)
    ref = np.asarray(ref).astype(np.complex128).reshape(len(ref), -1)
    err = np.linalg.norm(got - ref, axis=1) / np.maximum(np.linalg.norm(ref, axis=1), 1e-300)
    assert np.all(err <= H.REL_L2_TOL[np.dtype(ct)]), (what, "row", int(np.argmax(err)), float(err.max()))
    assert H.check_reference_rule(got, ref.astype(ct), n), (what, "per-element reference rule")


# ---------------------------------------------------------------------------------------------------------------------
# 3a. complex transforms

def _complex_case(d, direction, x, what, guard=None, rule_n=None):
    """the packed rows x [batch, *dims] through d's layout, clean and with rows 1 and batch - 2 poisoned"""
    G, pf, torch = _mods()
    guard = G.GUARD if guard is None else guard
    dirn = pf.direction.FORWARD if direction == F else pf.direction.BACKWARD
    inv = pf.inv(dirn)
    plan = d.commit()
    batch, dims = x.shape[0], list(x.shape[1:])
    bad = _poisoned_rows(batch)
    good = [b for b in range(batch) if b not in bad]
    xp = x.copy()
    for b in bad:
        H.poison_numpy(xp[b])
    got, clean = G.transform_packed(d, dirn, x, plan, guard, pad=CLEAN)
    _, poisoned = G.transform_packed(d, dirn, xp, plan, guard, pad=POISONED)
    axes = tuple(range(1, len(dims) + 1))
    xd = x.astype(np.complex128)
    n = int(np.prod(dims))
    ref = np.fft.fftn(xd, axes=axes) * d.forward_scale if direction == F else np.fft.ifftn(xd, axes=axes) * (n * d.backward_scale)
    _rel_l2_rows(got, ref, x.dtype, rule_n or n, what)
    idx = H.element_indices(batch, dims, d.get_strides(inv), d.get_distance(inv), d.get_offset(inv)).reshape(batch, -1)
    H.check_isolated(clean, poisoned, idx[good], idx[bad], str(what), _locate(idx), every_scalar=True)


def _batch_of(n, plan):
    return 3 if n >= (1 << 16) else 2 * _fpw(plan) + 1


PACKED = {"f32": [2, 17, 64, 100, 1024, 2048, 4096, 8192, 15360, 16384, 32768, 30000, 1 << 16, 1 << 20, 68640],
          "f64": [64, 1024, 4096, 12000, 16384, 1 << 16, 1 << 20]}
PACKED_CASES = [(p, n) for p in ("f32", "f64") for n in PACKED[p]]


@pytest.mark.parametrize("prec,n", PACKED_CASES)
def test_packed_rows_with_poisoned_neighbours(prec, n):
    """packed, out of place and in place, both directions"""
    G, pf, torch = _mods()
    ct = _types(prec)[1]
    batch = _batch_of(n, G.make_descriptor([n], prec).commit())
    x = _uniform(np.random.Generator(np.random.SFC64(n)), (batch, n), ct)
    for placement in (1, 0):
        d = G.make_descriptor([n], prec, batch=batch, placement=placement)
        for direction in (F, B):
            _complex_case(d, direction, x, (prec, n, "batch", batch, "ip" if placement == 0 else "oop", "bwd" if direction else "fwd"))
    torch.cuda.empty_cache()


@pytest.mark.parametrize("prec,n", PACKED_CASES)
def test_padded_rows_with_poisoned_gaps_and_neighbours(prec, n):
    """distances n + 5 on either side and on both, different offsets, a base one element off 128 bytes: the three shapes
    of test_gpu_anylen._both_directions.  Above the LDS-resident lengths (fp32 16384, fp64 8192) the register-resident
    kernels and the multi-kernel plans exist in the packed layout only: there the library's refusal is what is checked,
    and nothing is launched."""
    G, pf, torch = _mods()
    ct = _types(prec)[1]
    batch = _batch_of(n, G.make_descriptor([n], prec).commit())
    x = _uniform(np.random.Generator(np.random.SFC64(n + 1)), (batch, n), ct)
    for name, placement, dist, off, guard in (("padded input", 1, (n + 5, n), (5, 2), (65, 63)),
                                              ("padded output", 1, (n, n + 5), (0, 3), None),
                                              ("ip padded", 0, (n + 5, n + 5), (3, 3), (63, 65))):
        d = G.make_descriptor([n], prec, batch=batch, placement=placement, fwd_distance=dist[0], bwd_distance=dist[1],
                              fwd_offset=off[0], bwd_offset=off[1])
        if n > LDS_RESIDENT[prec]:
            with pytest.raises(pf.unsupported_configuration, match="only supported for 1-D transforms in the default"):
                d.commit()
            continue
        for direction in (F, B):
            _complex_case(d, direction, x, (prec, n, "batch", batch, name, "bwd" if direction else "fwd"), guard)
    torch.cuda.empty_cache()


@pytest.mark.parametrize("layout", ["bi-bi-ip", "bi-bi-oop", "p-bi", "bi-p", "bi-bi-split", "strided-gaps"])
@pytest.mark.parametrize("n", [64, 100, 1024, 1536, 2048])
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_strided_layouts_with_poisoned_columns(prec, n, layout):
    """the layouts of test_gpu_basis.LAYOUTS (batch-interleaved on either side, in place, split planes) and one strided
    layout with gaps (element strides 3 and 2, distances beyond the rows); a batch of one full column group plus three"""
    from test_gpu_basis import LAYOUTS
    G, pf, torch = _mods()
    ct = _types(prec)[1]
    batch = max(16, _fpw(G.make_descriptor([n], prec).commit())) + 3
    x = _uniform(np.random.Generator(np.random.SFC64(n + 2)), (batch, n), ct)
    if layout == "strided-gaps":
        d = G.make_descriptor([n], prec, batch=batch, fwd_strides=[3], fwd_distance=3 * n + 7, bwd_strides=[2],
                              bwd_distance=2 * n + 5, fwd_offset=4, bwd_offset=1)
        for direction in (F, B):
            _complex_case(d, direction, x, (prec, n, layout, "bwd" if direction else "fwd"))
        return
    place, lin, lout, storage, direction = LAYOUTS[layout]
    kw = {}
    fwd_l, bwd_l = (lin, lout) if direction == F else (lout, lin)
    if fwd_l == "BI":
        kw.update(fwd_strides=[batch], fwd_distance=1)
    if bwd_l == "BI":
        kw.update(bwd_strides=[batch], bwd_distance=1)
    d = G.make_descriptor([n], prec, batch=batch, storage=storage, placement=place, **kw)
    _complex_case(d, direction, x, (prec, n, layout))


@pytest.mark.parametrize("prec,dims", [(p, d) for p in ("f32", "f64") for d in ([64, 64], [16, 16, 16])] + [("f32", [1024, 1024])])
def test_nd_shapes_with_poisoned_neighbours(prec, dims):
    """the fused N-D kernels, and the two-pass 2-D plan of 1024 x 1024"""
    G, pf, torch = _mods()
    ct = _types(prec)[1]
    batch = 3 if dims[0] == 1024 else 2 * _fpw(G.make_descriptor(dims, prec).commit()) + 1
    x = _uniform(np.random.Generator(np.random.SFC64(sum(dims))), [batch] + dims, ct)
    for placement, direction in ((1, F), (0, B)):
        d = G.make_descriptor(dims, prec, batch=batch, placement=placement)
        _complex_case(d, direction, x, (prec, dims, "ip" if placement == 0 else "oop", "bwd" if direction else "fwd"))
    torch.cuda.empty_cache()


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_generic_tier_with_poisoned_neighbours(prec):
    """37 * 64 without runtime specialisation: the runtime-radix kernel"""
    G, pf, torch = _mods()
    n = 37 * 64
    ct = _types(prec)[1]
    os.environ["PFFT_JIT"] = "0"
    try:
        batch = 2 * _fpw(G.make_descriptor([n], prec).commit()) + 1
        x = _uniform(np.random.Generator(np.random.SFC64(n)), (batch, n), ct)
        for placement in (1, 0):
            d = G.make_descriptor([n], prec, batch=batch, placement=placement)
            for direction in (F, B):
                _complex_case(d, direction, x, (prec, n, "generic tier", placement, direction))
    finally:
        del os.environ["PFFT_JIT"]


@pytest.mark.parametrize("prec,n", [("f32", 67), ("f32", 1031), ("f64", 1021)])
def test_any_length_with_poisoned_gaps_and_neighbours(prec, n):
    from test_gpu_anylen import _desc
    G, pf, torch = _mods()
    ct = _types(prec)[1]
    batch = 2 * _fpw(_desc(pf, n, prec).commit()) + 1
    x = _uniform(np.random.Generator(np.random.SFC64(n)), (batch, n), ct)
    for name, ip, dist, off, guard in (("oop", False, None, (0, 0), None), ("ip", True, None, (0, 0), None),
                                       ("padded input", False, (n + 5, n), (5, 2), (65, 63)),
                                       ("padded output", False, (n, n + 5), (0, 3), None),
                                       ("ip padded", True, (n + 5, n + 5), (3, 3), (63, 65))):
        for direction in (F, B):
            _complex_case(_desc(pf, n, prec, batch, ip, dist, off), direction, x, (prec, n, "any length", name, direction), guard)


def _half_run(torch, G, plan, direction, x16, in_place, pad):
    """x16: float16 [batch, n, 2].  Guarded buffers of interleaved binary16 pairs; returns the whole output (numpy float16)"""
    count = x16.size
    gin = G.Guarded(count, torch.float16, pad=pad)
    gin.buf.copy_(torch.from_numpy(x16.reshape(-1)))
    gout = gin if in_place else G.Guarded(count, torch.float16, pad=pad)
    fn = plan.compute_forward if direction == F else plan.compute_backward
    fn(*([gin.buf.view(torch.complex32)] if in_place else [gin.buf.view(torch.complex32), gout.buf.view(torch.complex32)]))
    plan.wait()
    gin.check("fp16 input")
    gout.check("fp16 output")
    if not in_place:
        H.check_unchanged(x16.reshape(-1), gin.buf.cpu().numpy(), what="fp16: the input of an out-of-place execute")
    return gout.buf.cpu().numpy()


def _half_lengths():
    from test_gpu_half import REGISTERED, RUNTIME
    return [REGISTERED[0], RUNTIME[0], 4096]


@pytest.mark.parametrize("n", [2, 1536, 4096])
def test_fp16_storage_with_poisoned_neighbours(n):
    from test_gpu_half import check_accuracy, _exact, _input, FWD, BWD
    assert n in _half_lengths()
    G, pf, torch = _mods()
    fpw = _fpw(G.make_descriptor([n], "f32").commit())
    batch = 2 * fpw + 1
    x = _input(np.random.Generator(np.random.SFC64(n)), n, batch)
    x16 = np.stack([x.real, x.imag], axis=-1).astype(np.float16)
    bad = _poisoned_rows(batch)
    good = [b for b in range(batch) if b not in bad]
    xp = x16.copy()
    for b in bad:
        H.poison_numpy(xp[b])
    rows = np.arange(batch * n * 2).reshape(batch, n * 2)  # scalars
    for in_place, direction, scale in ((False, F, 1.0 / n), (True, B, 0.5)):
        kw = dict(fwd_scale=scale) if direction == F else dict(bwd_scale=scale)
        plan = G.make_descriptor([n], "f16", batch=batch, placement=0 if in_place else 1, **kw).commit()
        clean = _half_run(torch, G, plan, direction, x16, in_place, CLEAN)
        poisoned = _half_run(torch, G, plan, direction, xp, in_place, POISONED)
        got = clean.astype(np.float64).reshape(batch, n, 2)
        check_accuracy(got[..., 0] + 1j * got[..., 1], _exact(x, FWD if direction == F else BWD, scale), ("f16", n, in_place))
        H.check_isolated(clean, poisoned, rows[good], rows[bad], "fp16 N=%d %s" % (n, "ip bwd" if in_place else "oop fwd"),
                         lambda p: "(row %d, scalar %d)" % (p // (2 * n), p % (2 * n)))


# ---------------------------------------------------------------------------------------------------------------------
# pitched launches of the fused verbs

def _launch(inputs, in_count, in_idx, out_dtype, out_count, out_idx, call, pad, what, guard=None, in_place=False):
    """One launch between guard bands.  inputs: the packed input values (numpy), laid at the flat indices in_idx of a
    buffer of in_count elements; the rest of it, both guards and the whole output buffer of out_count elements hold `pad`.
    call(in_buffer, out_buffer) runs the verb on the flat device buffers (in place: the same buffer twice).  The guards,
    the write set out_idx and the unchanged input of an out-of-place launch are checked; returns the whole output
    buffer (numpy)."""
    G, pf, torch = _mods()
    guard = G.GUARD if guard is None else guard
    host = H.full(in_count, pad, inputs.dtype)
    host[np.asarray(in_idx).ravel()] = inputs.ravel()
    gin = G.Guarded(in_count, torch.from_numpy(host[:0]).dtype, guard, pad=pad)
    gin.buf.copy_(torch.from_numpy(host))
    if in_place:
        gout = gin
    else:
        gout = G.Guarded(out_count, torch.from_numpy(np.zeros(0, dtype=out_dtype)).dtype, guard, pad=pad)
    call(gin.buf, gout.buf)
    gin.check(str(what) + ": input")
    gout.check(str(what) + ": output")
    if not in_place:
        H.check_unchanged(host, gin.buf.cpu().numpy(), what=str(what) + ": the input")
    raw = gout.buf.cpu().numpy()
    H.check_write_set(raw, out_idx, pad=pad, what=str(what) + ": output buffer")
    return raw


def _rows_idx(rows, pitch, width, offset=0):
    return (offset + np.arange(rows, dtype=np.int64)[:, None] * pitch + np.arange(width, dtype=np.int64)[None, :])


def _frames_idx(ns, out_pitch, frames, frame_pitch, width):
    return (np.arange(ns, dtype=np.int64)[:, None, None] * out_pitch + np.arange(frames, dtype=np.int64)[None, :, None] * frame_pitch
            + np.arange(width, dtype=np.int64)[None, None, :])


# ---------------------------------------------------------------------------------------------------------------------
# 3b. real rows: R2C, C2R, DCT-II / III, DCT-IV

REAL = {"f32": [4, 64, 512, 4096, 16384, 2000], "f64": [128, 8192]}
REAL_CASES = [(p, n) for p in ("f32", "f64") for n in REAL[p]]


def _real_run(d, plan, direction, packed, pad, what):
    """R2C / C2R through the descriptor's layout (test_gpu_real._execute with a padding value).  Returns (the whole output
    as an array of the output domain's elements, the index array [batch, width] of the output domain)."""
    G, pf, torch = _mods()
    rt, ct = _types(d.scalar)
    n, batch = d.lengths[0], d.number_of_transforms
    bins = n // 2 + 1
    fwd = direction == F
    in_place = d.placement == pf.placement.IN_PLACE
    ridx = _rows_idx(batch, d.forward_distance, n, d.forward_offset)
    cidx = _rows_idx(batch, d.backward_distance, bins, d.backward_offset)
    n_real, n_cplx = d.get_input_count(pf.direction.FORWARD), d.get_output_count(pf.direction.FORWARD)
    fn = plan.compute_forward if fwd else plan.compute_backward

    def call(a, b):
        fn(*([a] if in_place else [a, b]))
        plan.wait()

    if in_place:
        count = max(n_real, 2 * n_cplx)  # scalars; every row slot holds 2 * bins of them
        assert count % 2 == 0
        if fwd:
            inputs, in_idx = packed.astype(rt), ridx
        else:  # the bins as scalar pairs
            inputs = np.ascontiguousarray(packed.astype(ct)).view(rt).reshape(batch, 2 * bins)
            in_idx = _rows_idx(batch, 2 * d.backward_distance, 2 * bins, 2 * d.backward_offset)
        slots = _rows_idx(batch, 2 * d.backward_distance, 2 * bins, 2 * d.backward_offset)
        raw = _launch(inputs, count, in_idx, rt, count, slots, call, pad, what, in_place=True)
        return (raw.view(ct), cidx) if fwd else (raw, ridx)
    if fwd:
        return _launch(packed.astype(rt), n_real, ridx, ct, n_cplx, cidx, call, pad, what), cidx
    return _launch(packed.astype(ct), n_cplx, cidx, rt, n_real, ridx, call, pad, what), ridx


@pytest.mark.parametrize("prec,n", REAL_CASES)
def test_real_transforms_with_poisoned_neighbours(prec, n):
    """R2C and C2R, out of place (offsets 5 / 2) and in place (padded rows); and C2R with only the documented-ignored
    scalars poisoned -- the imaginary parts of bins 0 and N/2 of every row -- where nothing is tainted"""
    from test_gpu_real import _desc
    G, pf, torch = _mods()
    rt, ct = _types(prec)
    m = n // 2
    batch = 2 * _fpw(pf.real_descriptor(n, prec).commit()) + 1
    rng = np.random.Generator(np.random.SFC64(n + 3))
    x, y = _uniform(rng, (batch, n), rt), _uniform(rng, (batch, m + 1), ct)
    bad = _poisoned_rows(batch)
    good = [b for b in range(batch) if b not in bad]
    xp, yp, yi = x.copy(), y.copy(), y.copy()
    for b in bad:
        H.poison_numpy(xp[b])
        H.poison_numpy(yp[b])
    H.poison_numpy(yi.view(rt), (np.arange(batch)[:, None] * 2 * (m + 1) + np.array([1, 2 * m + 1])[None, :]).ravel())
    assert np.all(np.isnan(yi[:, [0, m]].imag)) and np.all(np.isfinite(yi.real)) and np.all(np.isfinite(yi[:, 1:m].imag))
    yd = y.astype(np.complex128)
    yd[:, [0, m]] = yd[:, [0, m]].real
    for in_place, offsets in ((False, (5, 2)), (True, (6, 3))):
        d = _desc(pf, n, prec, batch, in_place, offsets, (1.0, 1.0))
        plan = d.commit()
        tag = (prec, n, "batch", batch, "ip" if in_place else "oop")
        clean, idx = _real_run(d, plan, F, x, CLEAN, tag + ("R2C",))
        poisoned, _ = _real_run(d, plan, F, xp, POISONED, tag + ("R2C poisoned",))
        _rel_l2_rows(clean[idx], np.fft.rfft(x.astype(np.float64), axis=1), ct, n, tag + ("R2C",))
        H.check_isolated(clean, poisoned, idx[good], idx[bad], str(tag + ("R2C",)), _locate(idx))
        clean, idx = _real_run(d, plan, B, y, CLEAN, tag + ("C2R",))
        poisoned, _ = _real_run(d, plan, B, yp, POISONED, tag + ("C2R poisoned",))
        _rel_l2_rows(clean[idx], n * np.fft.irfft(yd, n, axis=1), ct, n, tag + ("C2R",))
        H.check_isolated(clean, poisoned, idx[good], idx[bad], str(tag + ("C2R",)), _locate(idx))
        ignored, _ = _real_run(d, plan, B, yi, POISONED, tag + ("C2R ignored imaginary parts",))
        H.check_isolated(clean, ignored, idx, [], str(tag + ("C2R, Im of bins 0 and N/2 poisoned",)), _locate(idx))


def _pitched_rows(fn, x, in_place, pad, what, guard=None):
    """rows of N scalars at odd pitches (test_gpu_dct._dct with a padding value); fn(in view, out view)"""
    rows, n = x.shape
    in_pitch = _odd(n + 3)
    out_pitch = in_pitch if in_place else _odd(n + 7)

    def call(a, b):
        xv = a.as_strided((rows, n), (in_pitch, 1))
        fn(xv, xv if in_place else b.as_strided((rows, n), (out_pitch, 1)))

    idx = _rows_idx(rows, out_pitch, n)
    return _launch(x, rows * in_pitch, _rows_idx(rows, in_pitch, n), x.dtype, rows * out_pitch, idx, call, pad, what, guard,
                   in_place), idx


@pytest.mark.parametrize("prec,n", REAL_CASES)
def test_dcts_with_poisoned_gaps_and_neighbours(prec, n):
    """DCT-II, DCT-III and DCT-IV (both directions), out of place and in place, rows at odd pitches"""
    from dct_ref import dct_reference
    from dct4_ref import dct4_reference
    G, pf, torch = _mods()
    rt, ct = _types(prec)
    plan = pf.real_descriptor(n, prec).commit()
    plan.prepare_dct()
    plan.prepare_dct4()
    batch = 2 * _fpw(plan) + 1
    x = _uniform(np.random.Generator(np.random.SFC64(n + 4)), (batch, n), rt)
    bad = _poisoned_rows(batch)
    good = [b for b in range(batch) if b not in bad]
    xp = x.copy()
    for b in bad:
        H.poison_numpy(xp[b])

    def wait(f):
        def run(a, b):
            f(a, b)
            plan.wait()
        return run

    verbs = [("DCT-II", wait(lambda a, b: plan.dct(a, b, type=2)), lambda v: dct_reference(v, 2)),
             ("DCT-III", wait(lambda a, b: plan.dct(a, b, type=3)), lambda v: dct_reference(v, 3)),
             ("DCT-IV", wait(lambda a, b: plan.dct4(a, b)), dct4_reference),
             ("DCT-IV inverse", wait(lambda a, b: plan.dct4(a, b, inverse=True)), dct4_reference)]
    for name, fn, ref in verbs:
        for i, in_place in enumerate((False, True)):
            tag = "%s N=%d %s rows=%d %s" % (prec, n, name, batch, "in place" if in_place else "out of place")
            guard = (65, 63) if i else None
            clean, idx = _pitched_rows(fn, x, in_place, CLEAN, tag, guard)
            poisoned, _ = _pitched_rows(fn, xp, in_place, POISONED, tag + " poisoned", guard)
            _rel_l2_rows(clean[idx], ref(x), ct, n, tag)
            H.check_isolated(clean, poisoned, idx[good], idx[bad], tag, _locate(idx))


# ---------------------------------------------------------------------------------------------------------------------
# 3c. circular convolution

CONV = {"f32": [64, 1024, 8192], "f64": [128, 4096]}
CONV_CASES = [(p, n) for p in ("f32", "f64") for n in CONV[p]]


@pytest.mark.parametrize("prec,n", CONV_CASES)
def test_complex_convolution_with_a_poisoned_filter_and_rows(prec, n):
    """rows 1 and batch - 2 poisoned with two clean filters; then filter 1 of 2 poisoned entirely: the odd rows are tainted"""
    import test_gpu_conv as C
    G, pf, torch = _mods()
    ct = _types(prec)[1]
    rng = np.random.Generator(np.random.SFC64(n + 5))
    batch = 2 * C._fpw(pf, n, prec)[0] + 1
    x, h = _uniform(rng, (batch, n), ct), _uniform(rng, (2, n), ct)
    bad = _poisoned_rows(batch)
    xp, hp = x.copy(), h.copy()
    for b in bad:
        H.poison_numpy(xp[b])
    H.poison_numpy(hp[1])
    rows = np.arange(batch)
    for name, in_place, dist, off, guard in (("oop padded", False, (n + 5, n + 3), (5, 2), (65, 63)), ("ip", True, None, (0, 0), None)):
        d = C._desc(pf, n, prec, batch, in_place, dist, off)
        plan = d.commit()
        idx = _rows_idx(batch, d.backward_distance, n, d.backward_offset)
        for correlate in (False, True):
            tag = (prec, n, "batch", batch, name, "corr" if correlate else "conv")
            verb = C._verb(plan, correlate)
            plan.set_filter(torch.from_numpy(h).cuda())
            got, clean = G.transform_packed(d, pf.direction.FORWARD, x, verb, guard or G.GUARD, pad=CLEAN)
            C._check(got, C._reference(d, x, h, correlate), ct, n, tag)
            _, poisoned = G.transform_packed(d, pf.direction.FORWARD, xp, verb, guard or G.GUARD, pad=POISONED)
            good = [b for b in rows if b not in bad]
            H.check_isolated(clean, poisoned, idx[good], idx[bad], str(tag + ("rows",)), _locate(idx), every_scalar=True)
            plan.set_filter(torch.from_numpy(hp).cuda())
            _, poisoned = G.transform_packed(d, pf.direction.FORWARD, x, verb, guard or G.GUARD, pad=POISONED)
            H.check_isolated(clean, poisoned, idx[rows % 2 == 0], idx[rows % 2 == 1], str(tag + ("filter 1",)), _locate(idx),
                             every_scalar=True)


@pytest.mark.parametrize("prec,n", CONV_CASES)
def test_real_convolution_with_a_poisoned_filter_rows_and_ignored_parts(prec, n):
    """the same on real rows, out of place and in == out on padded rows; and the imaginary parts of bins 0 and N/2 of both
    spectra poisoned: nothing is tainted"""
    import test_gpu_rconv as C
    G, pf, torch = _mods()
    rt, ct = _types(prec)
    m = n // 2
    rng = np.random.Generator(np.random.SFC64(n + 6))
    batch = 2 * C._fpw(pf, n, prec)[0] + 1
    x, h = _uniform(rng, (batch, n), rt), C._spectra(rng, 2, n, ct)
    bad = _poisoned_rows(batch)
    rows = np.arange(batch)
    good = [b for b in rows if b not in bad]
    xp, hp, hi = x.copy(), h.copy(), h.copy()
    for b in bad:
        H.poison_numpy(xp[b])
    H.poison_numpy(hp[1])
    H.poison_numpy(hi.view(rt), (np.arange(2)[:, None] * 2 * (m + 1) + np.array([1, 2 * m + 1])[None, :]).ravel())
    assert np.all(np.isnan(hi[:, [0, m]].imag)) and np.all(np.isfinite(hi.real))
    for name, padded, offset, same in (("oop", False, 5, False), ("in == out padded", True, 3, True)):
        d = C._desc(pf, n, prec, batch, padded, offset)
        plan = d.commit()
        count = d.get_input_count(pf.direction.FORWARD)
        idx = _rows_idx(batch, d.forward_distance, n, d.forward_offset)
        for correlate in (False, True):
            tag = (prec, n, "batch", batch, name, "corr" if correlate else "conv")
            fn = plan.correlate if correlate else plan.convolve

            def call(a, b):
                fn(*([a] if same else [a, b]))
                plan.wait()

            def run(data, pad, what):
                return _launch(data, count, idx, rt, count, idx, call, pad, str(tag + (what,)), in_place=same)

            plan.set_filter(torch.from_numpy(h).cuda())
            clean = run(x, CLEAN, "clean")
            C._check(clean[idx], C._reference(d, x, h, correlate), ct, n, tag)
            H.check_isolated(clean, run(xp, POISONED, "rows"), idx[good], idx[bad], str(tag + ("rows",)), _locate(idx))
            plan.set_filter(torch.from_numpy(hp).cuda())
            H.check_isolated(clean, run(x, POISONED, "filter 1"), idx[rows % 2 == 0], idx[rows % 2 == 1],
                             str(tag + ("filter 1",)), _locate(idx))
            plan.set_filter(torch.from_numpy(hi).cuda())
            H.check_isolated(clean, run(x, POISONED, "ignored"), idx, [], str(tag + ("Im of bins 0 and N/2 of the spectra",)),
                             _locate(idx))


# ---------------------------------------------------------------------------------------------------------------------
# 3d. long-signal verbs

SIGNALS = 3


def _ragged(fpw, per_signal):
    """a count per signal of at least `per_signal` whose total over the three signals leaves a ragged last work-group (where
    one exists: with three rows per group every total is whole groups, and the groups straddle the signals instead)"""
    c = per_signal
    while fpw > 1 and SIGNALS % fpw != 0 and (SIGNALS * c) % fpw == 0:
        c += 1
    return c


def _three_poisonings(x, positions, poison_unit, taint_of, out_idx, what, run, clean=None):
    """x: (signals, ...) inputs.  run(data, pad, what) -> whole output.  1. only what lies outside the signals; 2. signal 1
    entirely; 3. one unit (sample or frame) of signal 0 at each of `positions`.  taint_of(position) -> (required,
    permitted) positions in out_idx[0] (flat, per signal).  Returns the clean output."""
    flat = out_idx.reshape(SIGNALS, -1)
    loc = _locate(out_idx.reshape(SIGNALS, -1), ("signal", "element"))
    clean = run(x, CLEAN, "clean") if clean is None else clean
    H.check_isolated(clean, run(x, POISONED, "outside"), flat, [], "%s: only the outside poisoned" % (what,), loc)
    xp = x.copy()
    H.poison_numpy(xp[1])
    H.check_isolated(clean, run(xp, POISONED, "signal 1"), flat[[0, 2]], flat[1], "%s: signal 1 poisoned" % (what,), loc)
    for pos in positions:
        xp = x.copy()
        poison_unit(xp[0], pos)
        required, permitted = taint_of(pos)
        assert len(required) > 0, (what, pos, "an empty taint set")
        keep = np.ones(flat.shape[1], dtype=bool)
        keep[permitted] = False
        untainted = np.concatenate([flat[0][keep], flat[1], flat[2]])
        H.check_isolated(clean, run(xp, POISONED, "unit %d" % pos), untainted, flat[0][required],
                         "%s: unit %d of signal 0 poisoned" % (what, pos), loc)
    return clean


LONG = {"f32": [4, 64, 512, 4096, 16384, 2000], "f64": [128, 8192]}
LONG_CASES = [(p, n) for p in ("f32", "f64") for n in LONG[p]]

_real_plans = {}


def _real_plan(pf, n, prec):
    if (n, prec) not in _real_plans:
        _real_plans[(n, prec)] = pf.real_descriptor(n, prec).commit()
    return _real_plans[(n, prec)]


def _analysis_geometry(n, fpw, pad):
    """(hop, lead, frames, in_length): odd hop and lead, the last frame runs past the end (zeros) or ends in the reflection"""
    m = n // 2
    hop = _odd(n // 4 + 1)
    lead = m - 1 if (m - 1) % 2 else m + 1
    frames = _ragged(fpw, max(5, -(-(2 * fpw + 1) // SIGNALS)))
    if pad == "zero":
        length = max((frames - 1) * hop - lead + m + 1, 2)
    else:
        length = max((frames - 1) * hop + n - 2 * lead, lead + 1)
    return hop, lead, frames, length


@pytest.mark.parametrize("pad", ["zero", "reflect"])
@pytest.mark.parametrize("prec,n", LONG_CASES)
def test_stft_reads_its_frames_only(prec, n, pad):
    import test_gpu_stft as S
    G, pf, torch = _mods()
    rt, ct = _types(prec)
    m = n // 2
    plan = _real_plan(pf, n, prec)
    hop, lead, frames, length = _analysis_geometry(n, _fpw(plan), pad)
    assert S._max_frames(n, length, hop, lead, pad) >= frames
    rng = np.random.Generator(np.random.SFC64(n + 7))
    x, w = _uniform(rng, (SIGNALS, length), rt), _uniform(rng, n, rt)
    plan.set_window(torch.from_numpy(w).cuda())
    in_pitch, frame_pitch = _odd(length + 3), m + 2
    out_pitch = frames * frame_pitch + 3
    out_idx = _frames_idx(SIGNALS, out_pitch, frames, frame_pitch, m + 1)
    tag = "stft %s N=%d %s hop %d lead %d frames %d in %d" % (prec, n, pad, hop, lead, frames, length)

    def call(a, b):
        plan.stft(a.as_strided((SIGNALS, length), (in_pitch, 1)), b.as_strided((SIGNALS, frames, m + 1), (out_pitch, frame_pitch, 1)),
                  hop, lead=lead, pad=pad)
        plan.wait()

    def run(data, p, what):
        return _launch(data, SIGNALS * in_pitch, _rows_idx(SIGNALS, in_pitch, length), ct, SIGNALS * out_pitch, out_idx, call, p,
                       tag + ": " + what)

    def taint(t):
        f = H.taint_frames(t, n, hop, lead, pad, frames, length)
        e = (f[:, None] * (m + 1) + np.arange(m + 1)[None, :]).ravel()
        return e, e

    clean = run(x, CLEAN, "clean")
    got = clean[out_idx]
    assert np.all(got[:, :, 0].imag == 0) and np.all(got[:, :, m].imag == 0)
    S._check(got, S._reference(1.0, x, w, n, hop, lead, pad, frames), ct, n, tag)
    _three_poisonings(x, (1 if length > 2 else 0, length // 2, length - 1), lambda sig, t: H.poison_numpy(sig, [t]), taint,
                      out_idx, tag, run, clean)


@pytest.mark.parametrize("pad", ["zero", "reflect"])
@pytest.mark.parametrize("prec,n", LONG_CASES)
def test_periodogram_reads_its_frames_only(prec, n, pad):
    """frames_per_row 1, 3 and n_frames: a dead frame of the ragged last row adds nothing, whatever lies behind the signal"""
    import test_gpu_periodogram as P
    import test_gpu_stft as S
    G, pf, torch = _mods()
    rt, ct = _types(prec)
    m = n // 2
    plan = _real_plan(pf, n, prec)
    hop, lead, frames, length = _analysis_geometry(n, _fpw(plan), pad)
    rng = np.random.Generator(np.random.SFC64(n + 8))
    x, w = _uniform(rng, (SIGNALS, length), rt), _uniform(rng, n, rt)
    plan.set_periodogram_window(torch.from_numpy(w).cuda())
    power = np.abs(S._reference(1.0, x, w, n, hop, lead, pad, frames)) ** 2
    in_pitch, row_pitch = _odd(length + 3), m + 3
    for avg in (1, 3, frames):
        n_rows = -(-frames // avg)
        out_pitch = n_rows * row_pitch + 3
        out_idx = _frames_idx(SIGNALS, out_pitch, n_rows, row_pitch, m + 1)
        tag = "periodogram %s N=%d %s hop %d lead %d frames %d A %d in %d" % (prec, n, pad, hop, lead, frames, avg, length)

        def call(a, b):
            plan.periodogram(a.as_strided((SIGNALS, length), (in_pitch, 1)),
                             b.as_strided((SIGNALS, n_rows, m + 1), (out_pitch, row_pitch, 1)), hop, frames,
                             frames_per_row=avg, lead=lead, pad=pad)
            plan.wait()

        def run(data, p, what):
            return _launch(data, SIGNALS * in_pitch, _rows_idx(SIGNALS, in_pitch, length), rt, SIGNALS * out_pitch, out_idx,
                           call, p, tag + ": " + what)

        def taint(t):
            c = H.taint_periodogram_rows(t, n, hop, lead, pad, frames, length, avg)
            e = (c[:, None] * (m + 1) + np.arange(m + 1)[None, :]).ravel()
            return e, e

        clean = run(x, CLEAN, "clean")
        P.check_rows(clean[out_idx], P.rows_of(power, avg), prec, n, avg, tag)
        _three_poisonings(x, (1 if length > 2 else 0, length // 2, length - 1), lambda sig, t: H.poison_numpy(sig, [t]), taint,
                          out_idx, tag, run, clean)


@pytest.mark.parametrize("prec,n", LONG_CASES)
def test_mdct_reads_its_frames_only(prec, n):
    import test_gpu_dct4 as D
    from dct4_ref import frames_of, mdct_reference
    G, pf, torch = _mods()
    rt, ct = _types(prec)
    plan = _real_plan(pf, n, prec)
    frames = _ragged(_fpw(plan), max(5, -(-(2 * _fpw(plan) + 1) // SIGNALS)))
    lead = n + 1
    length = (frames - 2) * n + n // 2  # the last frame holds N / 2 + 1 samples
    rng = np.random.Generator(np.random.SFC64(n + 9))
    x, w = _uniform(rng, (SIGNALS, length), rt), _uniform(rng, 2 * n, rt)
    plan.set_mdct_window(torch.from_numpy(w).cuda())
    in_pitch, frame_pitch = _odd(length + 3), _odd(n + 3)
    out_pitch = _odd(frames * frame_pitch + 5)
    out_idx = _frames_idx(SIGNALS, out_pitch, frames, frame_pitch, n)
    tag = "mdct %s N=%d lead %d frames %d in %d" % (prec, n, lead, frames, length)

    def call(a, b):
        plan.mdct(a.as_strided((SIGNALS, length), (in_pitch, 1)), b.as_strided((SIGNALS, frames, n), (out_pitch, frame_pitch, 1)),
                  lead=lead)
        plan.wait()

    def run(data, p, what):
        return _launch(data, SIGNALS * in_pitch, _rows_idx(SIGNALS, in_pitch, length), rt, SIGNALS * out_pitch, out_idx, call, p,
                       tag + ": " + what)

    def taint(t):
        f = H.taint_frames(t, 2 * n, n, lead, "zero", frames, length)
        e = (f[:, None] * n + np.arange(n)[None, :]).ravel()
        return e, e

    clean = run(x, CLEAN, "clean")
    D._check(clean[out_idx].reshape(-1, n), mdct_reference(frames_of(x, n, lead, frames, w)).reshape(-1, n), ct, n, tag)
    _three_poisonings(x, (0, length // 2, length - 1), lambda sig, t: H.poison_numpy(sig, [t]), taint, out_idx, tag, run, clean)


def _synthesis(prec, n, name, frame_len, width, hop, set_window, verb, reference, check):
    """istft / imdct: frames of `width` input elements that cover frame_len samples each; poisoning 3 at chunk_frames 0, 1
    and 2 FPW + 1 -- the recomputed halo between chunks must not widen the taint"""
    G, pf, torch = _mods()
    rt, ct = _types(prec)
    plan = _real_plan(pf, n, prec)
    fpw = _fpw(plan)
    frames = 4 * fpw + 3  # at least three chunks of 2 FPW + 1 frames
    lead = (n + 1) if frame_len == 2 * n else (n // 2 - 1 if (n // 2 - 1) % 2 else n // 2 + 1)
    olen = (frames - 1) * hop + frame_len - lead - 3
    in_dtype = rt if frame_len == 2 * n else ct
    rng = np.random.Generator(np.random.SFC64(n + 10))
    y = _uniform(rng, (SIGNALS, frames, width), in_dtype)
    w = rng.uniform(0.5, 1, frame_len).astype(rt)  # no envelope falls to the threshold of NORMALIZE
    set_window(plan, torch.from_numpy(w).cuda())
    frame_pitch = _odd(width + 2)
    in_pitch, out_pitch = frames * frame_pitch + 3, _odd(olen + 4)
    in_idx = _frames_idx(SIGNALS, in_pitch, frames, frame_pitch, width)
    out_idx = _rows_idx(SIGNALS, out_pitch, olen)
    tag = "%s %s N=%d hop %d lead %d frames %d out %d" % (name, prec, n, hop, lead, frames, olen)
    ref = reference(y, w, lead, olen)

    def taint(f):
        e = H.taint_samples(f, frame_len, hop, lead, olen)
        return e, e

    for chunk in (0, 1, 2 * fpw + 1):
        def call(a, b):
            verb(plan, a.as_strided((SIGNALS, frames, width), (in_pitch, frame_pitch, 1)),
                 b.as_strided((SIGNALS, olen), (out_pitch, 1)), lead, chunk)
            plan.wait()

        def run(data, p, what):
            return _launch(data, SIGNALS * in_pitch, in_idx, rt, SIGNALS * out_pitch, out_idx, call, p,
                           "%s chunk %d: %s" % (tag, chunk, what))

        clean = run(y, CLEAN, "clean")
        check(clean[out_idx], ref, ct, n, "%s chunk %d" % (tag, chunk))
        _three_poisonings(y, (0, frames // 2, frames - 1), lambda sig, f: H.poison_numpy(sig[f]), taint, out_idx,
                          "%s chunk %d" % (tag, chunk), run, clean)


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("prec,n", LONG_CASES)
def test_istft_spreads_a_frame_over_its_samples_only(prec, n, normalize):
    import test_gpu_istft as I
    hop = min(_odd(n // 4 + 1), n)

    def reference(y, w, lead, olen):
        ola, env = I._reference(1.0, y, w, n, hop, lead, olen)
        assert env.min() >= 0.25
        return ola / env if normalize else ola

    _synthesis(prec, n, "istft normalize" if normalize else "istft plain", n, n // 2 + 1, hop,
               lambda plan, w: plan.set_synthesis_window(w),
               lambda plan, a, b, lead, chunk: plan.istft(a, b, hop, lead=lead, normalize=normalize, chunk_frames=chunk),
               reference, I._check)


@pytest.mark.parametrize("prec,n", LONG_CASES)
def test_imdct_spreads_a_frame_over_its_samples_only(prec, n):
    import test_gpu_imdct as I
    from imdct_ref import imdct_reference
    _synthesis(prec, n, "imdct", 2 * n, n, n, lambda plan, w: plan.set_imdct_window(w),
               lambda plan, a, b, lead, chunk: plan.imdct(a, b, lead=lead, chunk_frames=chunk),
               lambda y, w, lead, olen: imdct_reference(y, w, n, lead, olen), I._check)


FILTER_COMPLEX = {"f32": [4, 64, 512, 4096, 8192, 2000], "f64": [128, 4096]}


def _filter_cases():
    out = []
    for real, table in ((False, FILTER_COMPLEX), (True, LONG)):
        for p in ("f32", "f64"):
            for n in table[p]:
                for k in sorted({1, 5, n // 4 + 1}):
                    if k <= (n - 2 if real else n):
                        out.append(("real" if real else "complex", p, n, k))
    return out


@pytest.mark.parametrize("correlate", [False, True])
@pytest.mark.parametrize("kind,prec,n,k", _filter_cases())
def test_filter_outputs_between_the_cone_and_the_segments(kind, prec, n, k, correlate):
    import test_gpu_filter as FC
    import test_gpu_rfilter as FR
    G, pf, torch = _mods()
    rt, ct = _types(prec)
    real = kind == "real"
    mod = FR if real else FC
    dt = rt if real else ct
    plan, c, fpw = mod._plan(pf, n, prec)
    hop, lead = H.filter_geometry(n, k, correlate, real)
    segments = _ragged(fpw, max(4, -(-(2 * fpw + 1) // SIGNALS)))
    olen = (segments - 1) * hop + hop // 2 + 1  # the last segment is partial
    length = olen if correlate else max(olen - (k - 1), 1)
    rng = np.random.Generator(np.random.SFC64(n + k))
    x, h = _uniform(rng, (SIGNALS, length), dt), _uniform(rng, (1, k), dt)
    plan.set_filter_taps(torch.from_numpy(h).cuda())
    in_pitch, out_pitch = _odd(length + 3), _odd(olen + 5)
    out_idx = _rows_idx(SIGNALS, out_pitch, olen)
    tag = "filter %s %s N=%d K=%d %s hop %d segments %d in %d out %d" % (kind, prec, n, k, "corr" if correlate else "conv", hop,
                                                                        segments, length, olen)

    def call(a, b):
        plan.filter(a.as_strided((SIGNALS, length), (in_pitch, 1)), b.as_strided((SIGNALS, olen), (out_pitch, 1)), correlate=correlate)
        plan.wait()

    def run(data, p, what):
        return _launch(data, SIGNALS * in_pitch, _rows_idx(SIGNALS, in_pitch, length), dt, SIGNALS * out_pitch, out_idx, call, p,
                       tag + ": " + what)

    clean = run(x, CLEAN, "clean")
    got = clean[out_idx]
    mod._check(got.astype(np.complex128) if not real else got, mod._reference(c, x, h, olen, correlate), ct, n, tag)
    positions = sorted({0, length // 2, length - 1})  # the first segment, the middle, the last sample
    _three_poisonings(x, positions, lambda sig, t: H.poison_numpy(sig, [t]),
                      lambda t: H.taint_filter(t, n, k, correlate, real, olen), out_idx, tag, run, clean)


# ---------------------------------------------------------------------------------------------------------------------
# 3e. table-setting calls: the array comes from a buffer between poisoned guards

def _guarded_array(G, torch, a, pad):
    g = G.Guarded(a.size, torch.from_numpy(a[:0]).dtype, (65, 63), pad=pad)
    g.buf.copy_(torch.from_numpy(a.reshape(-1)))
    return g


SETTERS = ["set_filter", "set_filter_taps", "set_filter real", "set_filter_taps real", "set_window", "set_synthesis_window",
           "set_mdct_window", "set_imdct_window", "set_periodogram_window"]


@pytest.mark.parametrize("setter", SETTERS)
def test_table_setting_calls_read_their_array_only(setter):
    """every array argument lies between guards of POISON; the verb's output is bit-identical to the run whose guards held
    the padding value.  set_filter_taps: n_taps < N, the plan pads the taps with zeros on the device"""
    G, pf, torch = _mods()
    n, prec = 1024, "f32"
    rt, ct = _types(prec)
    m = n // 2
    rng = np.random.Generator(np.random.SFC64(len(setter)))
    real = not setter.startswith("set_filter") or setter.endswith("real")
    if setter.startswith("set_filter"):
        d = pf.real_convolution_descriptor(n, prec) if real else pf.convolution_descriptor([n], prec)
        d.number_of_transforms = SIGNALS
        plan = d.commit()
    else:
        plan = pf.real_descriptor(n, prec).commit()
    dt = rt if real else ct
    length = 3 * n + 1
    x = torch.from_numpy(_uniform(rng, (SIGNALS, length), dt)).cuda()
    if setter.startswith("set_filter_taps"):
        table, shape = _uniform(rng, (2, 37), dt), (2, 37)
    elif setter.startswith("set_filter"):
        table = _uniform(rng, (2, m + 1 if real else n), ct)
        shape = table.shape
    else:
        table = rng.uniform(0.5, 1, 2 * n if "mdct" in setter else n).astype(rt)
        shape = table.shape
    outs = []
    for pad in (CLEAN, POISONED):
        g = _guarded_array(G, torch, table, pad)
        getattr(plan, setter.split()[0])(g.buf.view(*shape))
        if setter.startswith("set_filter_taps"):
            y = torch.zeros(SIGNALS, length, dtype=x.dtype, device="cuda")
            plan.filter(x, y)
        elif setter.startswith("set_filter"):
            y = torch.zeros(SIGNALS, n, dtype=x.dtype, device="cuda")
            plan.convolve(x[:, :n].contiguous().reshape(-1), y.reshape(-1))  # (row t: filter t mod 2)
        elif setter == "set_window":
            y = torch.zeros(SIGNALS, 5, m + 1, dtype=torch.complex64, device="cuda")
            plan.stft(x, y, n // 2 + 1, lead=m - 1, pad="reflect")
        elif setter == "set_periodogram_window":
            y = torch.zeros(SIGNALS, 2, m + 1, dtype=x.dtype, device="cuda")
            plan.periodogram(x, y, n // 2 + 1, 5, frames_per_row=3, lead=m - 1, pad="reflect")
        elif setter == "set_synthesis_window":
            bins = torch.from_numpy(_uniform(np.random.Generator(np.random.SFC64(1)), (SIGNALS, 5, m + 1), ct)).cuda()
            y = torch.zeros(SIGNALS, 4 * (m + 1) + n - (m - 1), dtype=x.dtype, device="cuda")
            plan.istft(bins, y, m + 1, lead=m - 1, normalize=True)
        elif setter == "set_mdct_window":
            y = torch.zeros(SIGNALS, 4, n, dtype=x.dtype, device="cuda")
            plan.mdct(x, y)
        else:
            coeff = torch.from_numpy(_uniform(np.random.Generator(np.random.SFC64(2)), (SIGNALS, 4, n), rt)).cuda()
            y = torch.zeros(SIGNALS, 4 * n, dtype=x.dtype, device="cuda")
            plan.imdct(coeff, y)
        plan.wait()
        g.check(setter + ": the array's guards")
        out = y.cpu().numpy().reshape(-1)
        assert np.all(np.isfinite(out.view(rt))) and np.any(out != 0), (setter, "the output")
        outs.append(out)
    H.check_isolated(outs[0], outs[1], np.arange(outs[0].size), [], setter + ": guards of the array poisoned")
