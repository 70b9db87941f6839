"""Every twiddle on the GPU: transforms of unit impulses against the rows of the transform's matrix, element by element,
with the derived bound of helpers.check_basis_rows.

The transform of e_j is row j of the DFT matrix.  Every butterfly sees at most one non-zero operand and adding zeros is
exact, so an output element is the product of the twiddles on its path: at most P(N) = ceil(log2 N) + (odd prime factors)
+ 1 multiplies of 3.3 u each (helpers.twiddle_path_length).  One table entry that is 1e-5 off -- 170 fp32 ulps -- fails
here; on random data it passes the relative-L2 and per-element yardsticks of every other test (test_check_helpers.py
shows both).  The row names the input digit and the element the output digit of the entry.

Bounds, as derived (u = 2^-24 for fp32 arithmetic, 2^-53 for fp64; scales multiply both sides):
  complex, forward and backward    3.3 u sum over the axes of P(N_a)
  R2C of a real impulse            3.3 u (P(N/2) + 3)
  C2R of a unit bin                2 * 3.3 u (P(N/2) + 3)         (amplitude 2)
  DCT-II, DCT-III, DCT-IV          2 * 3.3 u (P(N/2) + 4)
  fp16 storage, per component      the fp32 bound + half a binary16 ulp of the reference component
No bound here is fitted to what a kernel produced.

Rows: "all" is the N x N identity as one batch of N transforms; "some" (some_rows) is the ends and the middle, 2^i and
2^i +- 1, f and f +- 1 for every partial product f of the plan's factors from both ends, and 32 seeded random rows.
The impulses are generated and the outputs compared on the device; the packed runs lie between guard bands and leave the
input of an out-of-place execute alone, the layouts go through gpu_utils.transform_packed (write set, guards, input), the
real and DCT plans through the harnesses of test_gpu_real.py, test_gpu_dct.py and test_gpu_dct4.py.

Each test prints the worst ratio to the bound of every case and asserts it is at most 1.  No case is skipped.

Worst ratio per family as measured on the MI355X (records, not inputs to the bound; fp32 / fp64): complex 1-D 0.17 (N =
2^18) / 0.22 (2^20), N-D 0.09 / 0.13, R2C 0.11 / 0.15, C2R 0.10 / 0.16, DCT-II 0.10 / 0.13, DCT-III 0.11 / 0.15, DCT-IV 0.10 /
0.15; fp16 storage 0.99 (the rounding of the store reaches its half ulp).  A case takes 0.1 - 2.6 s; the one exception is
61 * 61 * 8 from an empty code-object cache, whose commit compiles the radix-61 kernels for 9 - 11 s (the length
test_gpu_parity.test_wave64_prime_factors commits too)."""
import os

import numpy as np
import pytest

import helpers as H
from test_gpu_half import REGISTERED, RUNTIME
from test_gpu_real import LENGTHS as REAL_LENGTHS

pytestmark = pytest.mark.gpu

F, B = H.FORWARD, H.BACKWARD


def _mods():
    import gpu_utils as G
    import portfft_amd as pf
    return G, pf, G.torch_mod()


def some_rows(n, factors=(), seed=0):
    """the ends and the middle; 2^i, 2^i +- 1; f, f +- 1 for every partial product f of `factors` from both ends; 32 seeded
    random rows (sorted, inside [0, n))"""
    rows = {0, 1, 2, 3, n // 2 - 1, n // 2, n // 2 + 1, n - 2, n - 1}
    i = 1
    while i < n:
        rows |= {i - 1, i, i + 1}
        i *= 2
    for order in (list(factors), list(factors)[::-1]):
        f = 1
        for v in order:
            f *= int(v)
            rows |= {f - 1, f, f + 1}
    rows |= set(int(v) for v in np.random.default_rng(seed + n).integers(0, n, 32))
    return np.array(sorted(r for r in rows if 0 <= r < n), dtype=np.int64)


def _factors(plan):
    d = plan.info().dims[0]
    return [int(v) for v in d.factors[:d.n_factors]]


def _cplx_rows(prec, dims, rows, direction, in_place=False, scale=1.0, what=""):
    """The transforms of e_rows (flat indices of the shape dims) as one packed batch, impulses made and outputs compared on
    the device: guard bands round both buffers, the input of an out-of-place execute unchanged.  Returns the worst ratio."""
    G, pf, torch = _mods()
    dims = [int(v) for v in np.atleast_1d(dims)]
    n, batch = int(np.prod(dims)), len(rows)
    kw = dict(fwd_scale=scale) if direction == F else dict(bwd_scale=scale)
    plan = G.make_descriptor(dims, prec, batch=batch, placement=0 if in_place else 1, **kw).commit()
    half = prec == "f16"
    tt = torch.float16 if half else torch.complex64 if prec == "f32" else torch.complex128
    unit = 2 if half else 1  # scalars per element of the buffers
    pos = torch.arange(batch, dtype=torch.int64, device="cuda") * n + torch.from_numpy(np.asarray(rows)).cuda()
    gin = G.Guarded(unit * batch * n, tt, fill=0)
    gin.buf[unit * pos] = 1
    gout = gin if in_place else G.Guarded(unit * batch * n, tt)
    view = (lambda t: t.view(torch.complex32)) if half else (lambda t: t)
    fn = plan.compute_forward if direction == F else plan.compute_backward
    fn(*([view(gin.buf)] if in_place else [view(gin.buf), view(gout.buf)]))
    plan.wait()
    gin.check(what + ": input")
    gout.check(what + ": output")
    if not in_place:
        flat = gin.buf if half else torch.view_as_real(gin.buf)
        assert int(torch.count_nonzero(flat)) == batch and bool((gin.buf[unit * pos] == 1).all()), \
            what + ": the input of an out-of-place execute changed"
    got = gout.buf.view(batch, n, 2).float() if half else gout.buf.view(batch, n)
    if half:
        got = torch.view_as_complex(got)
    ratio = H.check_basis_rows(got, rows, dims if len(dims) > 1 else n, "c2c", prec, scale=scale, direction=direction,
                               what=what)
    assert ratio <= 1.0
    return ratio


# ---------------------------------------------------------------------------------------------------------------------
# complex, packed

ALL_ROWS = [2, 3, 4, 8, 16, 17, 30, 64, 96, 100, 128, 256, 512, 592, 1000, 1024, 1536, 2048]
ALL_CASES = [(p, n) for p in ("f32", "f64") for n in ALL_ROWS] + [("f32", 4096)]
# LDS-resident and two-per-CU lengths, the register-resident lengths, four-step and persistent launches, prime factors
SOME_ROWS = {"f32": [8192, 10240, 15360, 16384, 20480, 32768, 30000], "f64": [4096, 16384, 12000]}
LONG = [1 << 16, 1 << 18, 1 << 20, 1 << 22, 68640, 61 * 61 * 8]
SOME_CASES = [(p, n) for p in ("f32", "f64") for n in SOME_ROWS[p] + LONG]


@pytest.mark.parametrize("prec,n", ALL_CASES)
def test_every_row_of_the_dft_matrix(prec, n):
    """the N x N identity as one batch: forward out of place, backward in place"""
    rows = np.arange(n)
    _cplx_rows(prec, n, rows, F, what="all rows fwd")
    _cplx_rows(prec, n, rows, B, in_place=True, what="all rows bwd in place")


@pytest.mark.parametrize("prec,n", SOME_CASES)
def test_rows_of_long_transforms(prec, n):
    G, pf, torch = _mods()
    rows = some_rows(n, _factors(G.make_descriptor([n], prec).commit()))
    _cplx_rows(prec, n, rows, F, what="some rows fwd")
    _cplx_rows(prec, n, rows, B, in_place=True, what="some rows bwd in place")
    torch.cuda.empty_cache()


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_rows_on_the_generic_tier(prec):
    """37 * 64 without runtime specialisation: the runtime-radix kernel and its tables"""
    G, pf, torch = _mods()
    n = 37 * 64
    os.environ["PFFT_JIT"] = "0"
    try:
        rows = some_rows(n, _factors(G.make_descriptor([n], prec).commit()))
        _cplx_rows(prec, n, rows, F, what="generic tier fwd")
        _cplx_rows(prec, n, rows, B, what="generic tier bwd")
    finally:
        del os.environ["PFFT_JIT"]


# ---------------------------------------------------------------------------------------------------------------------
# complex, layouts and shapes

# (placement, input layout, output layout, storage, direction)
LAYOUTS = {"bi-bi-ip": (0, "BI", "BI", 0, F), "bi-bi-oop": (1, "BI", "BI", 0, B), "p-bi": (1, "P", "BI", 0, F),
           "bi-p": (1, "BI", "P", 0, B), "bi-bi-split": (1, "BI", "BI", 1, F)}


@pytest.mark.parametrize("layout", list(LAYOUTS) + ["offsets-scale"])
@pytest.mark.parametrize("n", [64, 100, 1024, 1536, 2048])
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_every_row_in_strided_layouts(prec, n, layout):
    """the identity through batch-interleaved layouts (batch = N transforms, element stride N) on either side, in place
    and out of place, split planes once; and a packed descriptor with offsets and forward_scale = 0.5"""
    G, pf, torch = _mods()
    dtype = np.complex64 if prec == "f32" else np.complex128
    eye = np.eye(n, dtype=dtype)
    if layout == "offsets-scale":
        d = G.make_descriptor([n], prec, batch=n, fwd_offset=24, bwd_offset=8, fwd_scale=0.5)
        direction, scale = F, 0.5
    else:
        place, lin, lout, storage, direction = LAYOUTS[layout]
        kw = {}
        fwd_l, bwd_l = (lin, lout) if direction == F else (lout, lin)
        if fwd_l == "BI":
            kw.update(fwd_strides=[n], fwd_distance=1)
        if bwd_l == "BI":
            kw.update(bwd_strides=[n], bwd_distance=1)
        d = G.make_descriptor([n], prec, batch=n, storage=storage, placement=place, **kw)
        scale = 1.0
    got, _ = G.transform_packed(d, pf.direction.FORWARD if direction == F else pf.direction.BACKWARD, eye)
    ratio = H.check_basis_rows(torch.from_numpy(np.ascontiguousarray(got)).cuda(), np.arange(n), n, "c2c", prec, scale=scale,
                               direction=direction, what=layout)
    assert ratio <= 1.0


@pytest.mark.parametrize("dims", [[64, 64], [16, 16, 16]])
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_every_row_of_the_fused_nd_shapes(prec, dims):
    """the bound of a rank-2 or rank-3 shape is the sum of P over its axes"""
    rows = np.arange(int(np.prod(dims)))
    _cplx_rows(prec, dims, rows, F, what="fused N-D fwd")
    _cplx_rows(prec, dims, rows, B, in_place=True, what="fused N-D bwd in place")


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_rows_of_a_large_2d_shape(prec):
    n = 1024
    a = some_rows(n, [32, 32], seed=1)[::3]
    rows = np.unique(np.concatenate([some_rows(n * n, [n]), a * n + a[::-1], a * n, a]))  # both axes, one axis alone
    _cplx_rows(prec, [n, n], rows, F, what="1024 x 1024 fwd")
    _cplx_rows(prec, [n, n], rows, B, what="1024 x 1024 bwd")


@pytest.mark.parametrize("prec,n,pitch", [("f32", 4096, 4160), ("f64", 64, 80), ("f32", 1200, 1280)])
def test_rows_in_a_padded_row_layout(prec, n, pitch):
    """UNPACKED: rows of a padded matrix on both sides (runtime strides on the packed kernels' configurations)"""
    G, pf, torch = _mods()
    dtype = np.complex64 if prec == "f32" else np.complex128
    rows = np.arange(n) if n <= 1024 else some_rows(n, _factors(G.make_descriptor([n], prec).commit()))
    x = np.zeros((rows.size, n), dtype=dtype)
    x[np.arange(rows.size), rows] = 1
    d = G.make_descriptor([n], prec, batch=rows.size, fwd_strides=[1], fwd_distance=pitch, bwd_strides=[1],
                          bwd_distance=pitch, fwd_offset=5, bwd_offset=2)
    for direction in (F, B):
        got, _ = G.transform_packed(d, pf.direction.FORWARD if direction == F else pf.direction.BACKWARD, x)
        assert H.check_basis_rows(torch.from_numpy(np.ascontiguousarray(got)).cuda(), rows, n, "c2c", prec,
                                  direction=direction, what="padded rows") <= 1.0


# ---------------------------------------------------------------------------------------------------------------------
# fp16 storage

HALF = [4096, 32768, 1536]
assert set(HALF[:2]) <= set(REGISTERED) and HALF[2] in RUNTIME


@pytest.mark.parametrize("n", HALF)
def test_rows_with_fp16_storage(n):
    """binary16 data, fp32 arithmetic, one rounding on the store: per component the fp32 bound plus half a binary16 ulp"""
    G, pf, torch = _mods()
    rows = np.arange(n) if n <= 4096 else some_rows(n, _factors(G.make_descriptor([n], "f32").commit()))
    _cplx_rows("f16", n, rows, F, what="fp16 fwd")
    _cplx_rows("f16", n, rows, B, in_place=True, scale=0.5, what="fp16 bwd in place, scale 0.5")


# ---------------------------------------------------------------------------------------------------------------------
# real plans

REAL = {"f32": [4, 6, 8, 30, 64, 592, 1000, 1024, 4096, 16384, 20000], "f64": [4, 6, 8, 30, 64, 592, 1000, 1024, 4096, 8192, 6000]}
assert all(set(REAL[p]) <= set(REAL_LENGTHS[p]) for p in REAL)
REAL_CASES = [(p, n) for p in ("f32", "f64") for n in REAL[p]]
SCALES = (0.5, 0.25)  # forward_scale, backward_scale of the scaled plans


def _real_rows(pf, n, prec, dct_plan=None):
    """all rows up to N = 1024, some above (with the factors of the plan's N/2-point transform); the DCT rows always hold
    j = M - 1 and M and the outputs k = 0 and N - 1: both ends of the quarter-wave and a/b tables"""
    if n <= 1024:
        return np.arange(n)
    plan = dct_plan or pf.real_descriptor(n, prec).commit()
    return some_rows(n, _factors(plan))


def _impulses(rows, width, dtype):
    x = np.zeros((rows.size, width), dtype=dtype)
    x[np.arange(rows.size), rows] = 1
    return x


@pytest.mark.parametrize("prec,n", REAL_CASES)
def test_real_transforms_of_basis_vectors(prec, n):
    """R2C of every real impulse and C2R of every unit bin (0 and N/2 included: +-1 rows), out of place and in place, and
    once more on a scaled plan with offsets"""
    import test_gpu_real as R
    G, pf, torch = _mods()
    rt, ct = R._types(prec)
    rows = _real_rows(pf, n, prec)
    bins = np.unique(np.concatenate([rows[rows <= n // 2], [n // 2]]))
    worst = 0.0
    for in_place, offsets, scales in ((False, (0, 0), (1.0, 1.0)), (True, (0, 0), (1.0, 1.0)),
                                      (False, (5, 2), SCALES), (True, (6, 3), SCALES)):
        what = "%s%s" % ("in place" if in_place else "out of place", " scaled" if scales != (1.0, 1.0) else "")
        d = R._desc(pf, n, prec, rows.size, in_place, offsets, scales)
        y, _ = R._execute(pf, torch, d, d.commit(), pf.direction.FORWARD, _impulses(rows, n, rt))
        worst = max(worst, H.check_basis_rows(torch.from_numpy(np.ascontiguousarray(y)).cuda(), rows, n, "r2c", prec,
                                              scale=scales[0], what="R2C " + what))
        d = R._desc(pf, n, prec, bins.size, in_place, offsets, scales)
        x, _ = R._execute(pf, torch, d, d.commit(), pf.direction.BACKWARD, _impulses(bins, n // 2 + 1, ct))
        worst = max(worst, H.check_basis_rows(torch.from_numpy(np.ascontiguousarray(x)).cuda(), bins, n, "c2r", prec,
                                              scale=scales[1], what="C2R " + what))
    assert worst <= 1.0


@pytest.mark.parametrize("prec,n", REAL_CASES)
def test_dct_2_and_3_of_basis_vectors(prec, n):
    import test_gpu_dct as D
    G, pf, torch = _mods()
    rt, _ = D._types(prec)
    worst = 0.0
    for scaled, in_place in ((False, False), (False, True), (True, False)):
        plan, (fs, bs), _ = D._plan(pf, n, prec, scaled)
        rows = _real_rows(pf, n, prec, plan)
        x = _impulses(rows, n, rt)
        for kind, scale in ((2, fs), (3, bs)):
            what = "DCT-%s %s%s" % ("II" if kind == 2 else "III", "in place" if in_place else "out of place",
                                    " scaled" if scaled else "")
            y = D._dct(G, torch, plan, kind, x, in_place, what)
            worst = max(worst, H.check_basis_rows(torch.from_numpy(y).cuda(), rows, n, "dct%d" % kind, prec, scale=scale,
                                                  what=what))
    assert worst <= 1.0


@pytest.mark.parametrize("prec,n", REAL_CASES)
def test_dct_4_of_basis_vectors(prec, n):
    """both directions: `inverse` is the same matrix times the backward scale"""
    import test_gpu_dct4 as D
    G, pf, torch = _mods()
    rt, _ = D._types(prec)
    worst = 0.0
    for scaled, in_place in ((False, False), (False, True), (True, False)):
        plan, (fs, bs), _ = D._plan(pf, n, prec, scaled)
        rows = _real_rows(pf, n, prec, plan)
        x = _impulses(rows, n, rt)
        for inverse, scale in ((False, fs), (True, bs)):
            what = "DCT-IV %s %s%s" % ("inverse" if inverse else "forward", "in place" if in_place else "out of place",
                                       " scaled" if scaled else "")
            y = D._dct4(G, torch, plan, inverse, x, in_place, what)
            worst = max(worst, H.check_basis_rows(torch.from_numpy(y).cuda(), rows, n, "dct4", prec, scale=scale, what=what))
    assert worst <= 1.0
