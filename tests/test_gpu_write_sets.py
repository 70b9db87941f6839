"""Where stray writes come from: ragged batch tails per tier, gapped layouts, the last chunk of chunked plans and base
pointers off the 128-byte alignment -- through gpu_utils.transform_packed, which places every buffer between guard bands,
checks that an out-of-place execute leaves its input alone and that every element of the output buffer outside the
output domain still holds the padding value.  Every transform is compared with NumPy in double precision."""
import os

import numpy as np
import pytest

import helpers as H

pytestmark = pytest.mark.gpu


def _mods():
    import gpu_utils as G
    import portfft_amd as pf
    return G, pf


class _env:
    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        os.environ.update(self.kv)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _check_all(got, ref, dtype, what):
    """rel-L2 of EVERY transform against the fp64 result"""
    got = np.asarray(got).astype(np.complex128).reshape(ref.shape[0], -1)
    ref = np.asarray(ref).astype(np.complex128).reshape(ref.shape[0], -1)
    err = np.linalg.norm(got - ref, axis=1) / np.maximum(np.linalg.norm(ref, axis=1), 1e-300)
    tol = H.REL_L2_TOL[np.dtype(dtype)]
    assert np.all(err <= tol), (what, "transform", int(np.argmax(err)), float(err.max()))


def _both_ways(G, pf, d, dims, batch, dtype, what, guard=None, plan=None, scale=(1.0, 1.0)):
    """forward and backward through the descriptor's layout; write sets checked by transform_packed"""
    n = int(np.prod(dims))
    x, y = H.gen_fourier_data(batch, dims, dtype, seed=(n + batch) % 1000)
    kw = {} if guard is None else {"guard": guard}
    plan = plan or d.commit()
    got, _ = G.transform_packed(d, pf.direction.FORWARD, x, plan=plan, **kw)
    _check_all(got, scale[0] * y.astype(np.complex128), dtype, (what, "fwd"))
    back, _ = G.transform_packed(d, pf.direction.BACKWARD, y, plan=plan, **kw)
    _check_all(back, scale[1] * n * x.astype(np.complex128), dtype, (what, "bwd"))


# (precision, length, layout, expected tiers): one register length, one LDS work-group length, one register-resident
# length, one batch-interleaved strided length, one runtime-specialised length
TIER_CASES = [("f32", 16, "P", (0,)), ("f32", 4096, "P", (1,)), ("f32", 24576, "P", (1,)), ("f32", 64, "BI", (0, 1)),
              ("f32", 1200, "P", (0, 1))]


@pytest.mark.parametrize("prec,n,layout,tiers", TIER_CASES)
def test_ragged_tails_per_tier(prec, n, layout, tiers):
    """batches 1, fpw - 1, fpw + 1, 2 fpw - 1 (fpw: transforms per work-group) in both directions, placements and
    storages, and one batch just above a full wave of work-groups (8 per CU)"""
    G, pf = _mods()
    dtype = np.complex64 if prec == "f32" else np.complex128

    def desc(batch, place, storage):
        kw = dict(fwd_strides=[batch], fwd_distance=1, bwd_strides=[batch], bwd_distance=1) if layout == "BI" else {}
        return G.make_descriptor([n], prec, batch=batch, placement=place, storage=storage, **kw)

    info = desc(1, 1, 0).commit().info()
    fpw = max(1, info.dims[0].ffts_per_workgroup)
    wave = info.n_compute_units * 8 * fpw + 1
    batches = sorted({1, max(1, fpw - 1), fpw + 1, max(1, 2 * fpw - 1)})
    for batch in batches:
        for place in (1, 0):
            for storage in (0, 1):
                d = desc(batch, place, storage)
                plan = d.commit()
                assert plan.info().dims[0].tier in tiers, (n, layout, batch, plan.info().dims[0].tier)
                _both_ways(G, pf, d, [n], batch, dtype, ("tail", prec, n, layout, batch, place, storage), plan=plan)
    if wave * n <= (1 << 24):
        for place, storage in ((1, 0), (0, 1)):
            d = desc(wave, place, storage)
            plan = d.commit()
            assert plan.info().dims[0].tier in tiers
            _both_ways(G, pf, d, [n], wave, dtype, ("wave", prec, n, layout, wave, place, storage), plan=plan)


def test_gapped_layouts_in_place_and_out_of_place():
    """UNPACKED row pitches, stride > 1 with distance > N * stride, and two-pass 2-D shapes with offsets: the gaps hold
    padding before and must hold it after, in place too"""
    G, pf = _mods()
    cases = [  # (prec, dims, fwd strides, fwd distance, bwd strides, bwd distance, batch)
        ("f32", [4096], [1], 4160, [1], 4160, 5), ("f32", [1200], [1], 1280, [1], 1280, 6),
        ("f64", [4096], [1], 4100, [1], 4100, 3), ("f32", [64], [3], 199, [3], 199, 33),
        ("f64", [625], [2], 1300, [2], 1300, 6), ("f32", [96], [3], 300, [3], 300, 10),
        ("f32", [16], [1], 20, [1], 20, 33)]
    for prec, dims, fs, fd, bs, bd, batch in cases:
        dtype = np.complex64 if prec == "f32" else np.complex128
        for place in (1, 0):
            for storage in (0, 1):
                d = G.make_descriptor(dims, prec, batch=batch, placement=place, storage=storage, fwd_strides=fs,
                                      fwd_distance=fd, bwd_strides=bs, bwd_distance=bd, fwd_offset=3,
                                      bwd_offset=3 if place == 0 else 9)
                _both_ways(G, pf, d, dims, batch, dtype, ("gapped", prec, dims, fs, fd, place, storage))
    # out of place onto a layout of other strides: packed rows in, strided columns out
    d = G.make_descriptor([64], "f32", batch=7, fwd_strides=[1], fwd_distance=70, bwd_strides=[5], bwd_distance=331)
    _both_ways(G, pf, d, [64], 7, np.complex64, "rows to strided")
    # the two-pass 2-D plan with offsets on both sides
    for prec, dims in (("f32", [256, 256]), ("f64", [64, 1024]), ("f32", [1080, 64])):
        dtype = np.complex64 if prec == "f32" else np.complex128
        for place in (1, 0):
            for storage in (0, 1):
                d = G.make_descriptor(dims, prec, batch=2, placement=place, storage=storage, fwd_offset=7,
                                      bwd_offset=7 if place == 0 else 13, fwd_scale=0.5)
                _both_ways(G, pf, d, dims, 2, dtype, ("2-D offsets", prec, dims, place, storage), scale=(0.5, 1.0))


def test_chunked_plans_at_chunk_boundaries():
    """A last chunk of exactly one transform and one a transform short of a full chunk, in plans whose consecutive
    chunks overlap (second stream, first launch of a chunk without the in-order barrier).  The chunk size follows from
    PFFT_CACHE_CHUNK_MIB the way plan_core.cpp derives it (even_chunks: the same number of chunks, equally filled)."""
    G, pf = _mods()

    def even_chunks(cap, count):
        n_chunks = -(-count // cap)
        return -(-count // n_chunks), n_chunks

    # (prec, dims, bytes of intermediate per transform, chunk MiB, batch, wanted size of the last chunk, storages)
    # ((fp64 2-D split planes run streamed, one launch per pass: plan_nd.cpp takes cache-sized chunks for split storage
    #  only on the registered writer / reader twins)
    cases = [("f32", [1024, 1024], 8 << 20, 16, 3, "one", (0, 1)), ("f32", [1024, 1024], 8 << 20, 24, 5, "short", (0, 1)),
             ("f64", [512, 512], 4 << 20, 8, 3, "one", (0,)), ("f32", [65536], 512 << 10, 1, 3, "one", (0, 1)),
             ("f32", [65536], 512 << 10, 2, 7, "short", (0, 1))]
    for prec, dims, per, mib, batch, want, storages in cases:
        dtype = np.complex64 if prec == "f32" else np.complex128
        chunk, n_chunks = even_chunks((mib << 20) // per, batch)
        last = batch - (n_chunks - 1) * chunk
        assert n_chunks > 1 and last == (1 if want == "one" else chunk - 1), (dims, mib, batch, chunk, last)
        for place in (1, 0):
            for storage in storages:
                with _env(PFFT_CACHE_CHUNK_MIB=str(mib)):
                    d = G.make_descriptor(dims, prec, batch=batch, placement=place, storage=storage)
                    plan = d.commit()
                launches = list(plan.info().launches)
                assert launches[0] >= 2 * n_chunks, (prec, dims, mib, batch, place, storage, launches)
                _both_ways(G, pf, d, dims, batch, dtype, ("chunks", prec, dims, mib, batch, place, storage),
                           plan=plan)


def test_base_pointers_off_the_line_alignment():
    """every buffer one element past a 128-byte boundary (an odd front guard), interleaved and split, both placements"""
    G, pf = _mods()
    for prec, dims, storage, batch, layout in (("f32", [4096], 0, 5, "P"), ("f64", [4096], 1, 3, "P"),
                                              ("f32", [64], 0, 33, "BI"), ("f32", [1200], 1, 6, "P"),
                                              ("f32", [256, 256], 0, 2, "P")):
        dtype = np.complex64 if prec == "f32" else np.complex128
        for place in (1, 0):
            kw = dict(fwd_strides=[batch], fwd_distance=1, bwd_strides=[batch], bwd_distance=1) if layout == "BI" else {}
            d = G.make_descriptor(dims, prec, batch=batch, placement=place, storage=storage, **kw)
            _both_ways(G, pf, d, dims, batch, dtype, ("misaligned", prec, dims, storage, layout, place), guard=(65, 63))
