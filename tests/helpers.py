"""Shared test helpers: reference-style data generation, layout scatter/gather, error metrics, test tables."""
import numpy as np

FORWARD, BACKWARD = 0, 1
PADDING_VALUE = -5.0  # test/unit_test/fft_test_utils.hpp:452


class _Poison:
    """A quiet NaN per scalar type, defined by its bit pattern (bytes per scalar -> bits): POISON[np.float32] is the
    scalar.  As a `pad=` argument it stands for that NaN of the buffer's own scalar type, in both components of a
    complex element.  Arrays and tensors are filled through an integer view, so host and device hold the same bits."""
    BITS = {2: 0x7E00, 4: 0x7FC00000, 8: 0x7FF8000000000000}

    def __getitem__(self, dtype):
        dt = np.dtype(dtype)
        dt = np.dtype({8: np.float32, 16: np.float64}[dt.itemsize]) if dt.kind == "c" else dt
        return np.array([self.BITS[dt.itemsize]], dtype="u%d" % dt.itemsize).view(dt)[0]

    def __repr__(self):
        return "POISON"


POISON = _Poison()


def _uint_view(a):
    """the scalars of a numpy array (complex: both components) as unsigned integers, a writable view"""
    if a.dtype.kind == "c":
        a = a.view(a.real.dtype)
    return a.view("u%d" % a.itemsize)


def poison_numpy(a, index=None):
    """POISON into every scalar of the numpy array `a` (or of the elements a.ravel()[index]), in place, by bit pattern"""
    assert a.flags.c_contiguous
    bits = _uint_view(a.reshape(-1)).reshape(a.size, -1)
    bits[slice(None) if index is None else np.asarray(index, dtype=np.int64).ravel()] = POISON.BITS[bits.itemsize]
    return a


def poison_torch(t, index=None):
    """POISON into every scalar of the contiguous torch tensor `t` (or of the elements t.reshape(-1)[index]), in place,
    through an integer view; float16 tensors that hold interleaved pairs are indexed in scalars"""
    import torch
    flat = torch.view_as_real(t).reshape(t.numel(), 2) if t.is_complex() else t.reshape(-1, 1)
    it = {2: torch.int16, 4: torch.int32, 8: torch.int64}[flat.element_size()]
    bits = flat.view(it)
    assert bits.data_ptr() == t.data_ptr(), "poison_torch needs a view of t"
    if index is None:
        bits.fill_(POISON.BITS[flat.element_size()])
    else:
        bits[torch.as_tensor(np.asarray(index, dtype=np.int64).ravel(), device=t.device)] = POISON.BITS[flat.element_size()]
    return t


def full_torch(count, pad, dtype, device):
    """torch.full (flat) for a padding value that may be POISON"""
    import torch
    if pad is POISON:
        return poison_torch(torch.empty(count, dtype=dtype, device=device))
    return torch.full((count,), pad, dtype=dtype, device=device)


def full(count, pad, dtype):
    """np.full for a padding value that may be POISON"""
    if pad is POISON:
        return poison_numpy(np.empty(count, dtype=dtype))
    return np.full(count, pad, dtype=dtype)


def gen_fourier_data(batch, dims, dtype, seed=0):
    """The reference test generator (test/common/reference_data_wrangler.hpp:117-145): (forward data, backward data)
    as packed arrays of shape [batch, *dims]."""
    is_double = np.dtype(dtype) in (np.dtype(np.complex128), np.dtype(np.float64))
    scalar = np.double if is_double else np.single
    ctype = np.complex128 if is_double else np.complex64
    shape = [batch] + list(dims)
    rng = np.random.Generator(np.random.SFC64(seed))
    x = rng.uniform(-1, 1, shape).astype(scalar)
    x = x + 1j * rng.uniform(-1, 1, shape).astype(scalar)
    y = np.fft.fftn(x, axes=range(1, len(dims) + 1))
    return x.astype(ctype), y.astype(ctype)


def golden_global_cases(golden):
    """(key, precision, n, input, expected output) of the GLOBAL-level fixture (tests/golden/fft_vectors_global.npz:
    the reference's GlobalTest / WorkgroupOrGlobal sizes, batch 1).  Only the output is stored; the input is regenerated
    from the reference generator's seed and must hash to the stored sha256."""
    import hashlib
    g = golden["global"]
    for k in sorted(f[:-4] for f in g.files if f.endswith("_out")):
        prec, _, n = k.split("_")
        x, _ = gen_fourier_data(1, [int(n)], np.complex64 if prec == "f32" else np.complex128)
        digest = hashlib.sha256(np.ascontiguousarray(x).tobytes()).digest()
        assert digest == g[k + "_in_sha256"].tobytes(), "the regenerated input of %s is not the fixture's" % k
        yield k, prec, int(n), x, g[k + "_out"]


def default_strides(dims):
    s, t = [0] * len(dims), 1
    for i in reversed(range(len(dims))):
        s[i] = t
        t *= dims[i]
    return s


def element_indices(batch, dims, strides, distance, offset):
    """flat index of every element of a [batch, *dims] array in a strided buffer"""
    idx = offset + np.arange(batch, dtype=np.int64).reshape([batch] + [1] * len(dims)) * distance
    for ax, (n, s) in enumerate(zip(dims, strides)):
        shape = [1] * (len(dims) + 1)
        shape[ax + 1] = n
        idx = idx + np.arange(n, dtype=np.int64).reshape(shape) * s
    return idx


def scatter(packed, strides, distance, offset, count, pad=PADDING_VALUE):
    """lay a packed [batch, *dims] array out in a flat buffer of `count` elements (padding value elsewhere), as
    reference_data_wrangler.hpp:52-90 does"""
    buf = full(count, pad, packed.dtype)
    idx = element_indices(packed.shape[0], packed.shape[1:], strides, distance, offset)
    buf[idx.ravel()] = packed.ravel()
    return buf


def gather(buf, batch, dims, strides, distance, offset):
    idx = element_indices(batch, dims, strides, distance, offset)
    return buf[idx.ravel()].reshape([batch] + list(dims))


def rel_l2(a, b):
    a = np.asarray(a).astype(np.complex128).ravel()
    b = np.asarray(b).astype(np.complex128).ravel()
    den = np.linalg.norm(b)
    return float(np.linalg.norm(a - b) / (den if den > 0 else 1.0))


def reference_tolerance(dtype, n):
    """per-element abs-or-rel tolerance of the reference tests: 2 * eps * N * log2(N) (fft_test_utils.hpp:461-464)"""
    eps = np.finfo(np.float64 if np.dtype(dtype) == np.dtype(np.complex128) else np.float32).eps
    return 2.0 * eps * n * max(np.log2(n), 1.0)


def check_reference_rule(out, ref, n):
    """reference_data_wrangler.hpp:355-370: every element within tol absolutely OR relatively"""
    tol = reference_tolerance(np.asarray(ref).dtype if np.asarray(ref).dtype.kind == "c" else np.complex64, n)
    out = np.asarray(out).astype(np.complex128).ravel()
    ref = np.asarray(ref).astype(np.complex128).ravel()
    absd = np.abs(out - ref)
    reld = absd / np.maximum(np.abs(ref), 1e-300)
    return bool(np.all((absd <= tol) | (reld <= tol)))


# FP tolerance of this repo's parity tests: relative L2 error per transform against the double-precision result.
# north_star asks for <= 1e-4; we hold the implementation to the precision it actually has.
REL_L2_TOL = {np.dtype(np.complex64): 2e-6, np.dtype(np.complex128): 5e-15}


# invalid descriptors of test/unit_test/instantiate_fft_tests.hpp:322-373:
# (lengths, fwd_strides, bwd_strides, fwd_distance, bwd_distance, batch, placement) -- None = default
IN_PLACE, OUT_OF_PLACE = 0, 1
INVALID_CASES = [
    ("InvalidLength", [0], None, None, None, None, 1, OUT_OF_PLACE),
    ("InvalidBatch", [1], None, None, None, None, 0, OUT_OF_PLACE),
    ("InvalidDistance0", [5], [5], [1], 0, 5, 2, OUT_OF_PLACE),
    ("InvalidDistance1", [5], [1], [5], 5, 0, 2, OUT_OF_PLACE),
    ("InvalidNonPositiveStrides0", [5], [0], [1], None, None, 1, OUT_OF_PLACE),
    ("InvalidNonPositiveStrides1", [5], [1], [0], None, None, 1, OUT_OF_PLACE),
    ("InvalidNonPositiveStrides2", [5, 12], [12, 1], [12, 0], None, None, 1, OUT_OF_PLACE),
    ("InvalidShortDistance0", [8], [1], [1], 7, 8, 2, OUT_OF_PLACE),
    ("InvalidShortDistance1", [8, 4], [8, 2], [4, 1], 24, 24, 2, OUT_OF_PLACE),
    ("InvalidIPNotMatching0", [8], [2], [1], 16, 8, 2, IN_PLACE),
    ("InvalidIPNotMatching1", [8, 4], [8, 2], [8, 2], 48, 50, 2, IN_PLACE),
    ("InvalidOverlap0", [4], [1], [1], 1, 4, 3, OUT_OF_PLACE),
    ("InvalidOverlap1", [4], [1], [2], 4, 3, 3, OUT_OF_PLACE),
    ("InvalidOverlapLarge", [8], [3333333], [3333333], 1, 1, 3333334, OUT_OF_PLACE),
    ("InvalidStrideEqualsDistance0", [8], [2], [2], 2, 2, 2, OUT_OF_PLACE),
    ("InvalidStrideEqualsDistance1", [8], [1], [1], 1, 1, 2, OUT_OF_PLACE),
]

# valid strided layouts of instantiate_fft_tests.hpp:237-319: (lengths, fwd_strides, bwd_strides, fwd_dist, bwd_dist)
STRIDED_OOP_CASES = [
    ([3], [4], [7], None, None),
    ([8], [11], [2], None, None),
    ([9], [3], [4], 30, 40),
    ([64], [1], [7], None, None),
    ([64], [4], [7], None, None),
    ([75], [3], [2], 300, 200),
    ([104], [3], [4], None, None),
]
STRIDED_OOP_BATCH_INTERLEAVED_LIKE = [
    ([8], [33], [99], 1, 3),
    ([8], [33], [2], 1, 16),
    ([8], [2], [66], 16, 2),
    ([64], [33], [99], 1, 3),
    ([96], [33], [2], 1, 192),
    ([70], [2], [66], 140, 2),
]
STRIDED_IP_CASES = [
    ([3], [4], [4], None, None),
    ([9], [3], [3], 25, 25),
    ([75], [4], [4], None, None),
    ([96], [3], [3], 286, 286),
]


# ---------------------------------------------------------------------------------------------------------------------
# write-set checks: what an execute may and may not touch (reference_data_wrangler.hpp:299-320 checks the padding)

def _scalar_bits(a):
    """the bits of every scalar of `a` (complex: real and imaginary part), as one unsigned integer each"""
    a = np.ascontiguousarray(a)
    if a.dtype.kind == "c":
        a = a.view(a.real.dtype)
    return a.view({4: np.uint32, 8: np.uint64, 2: np.uint16}[a.itemsize])


def _planes(buf):
    """a buffer as a list of (name, array): one interleaved array, or the two planes of split storage"""
    if isinstance(buf, (tuple, list)):
        return list(zip(("re", "im"), buf))
    return [("", buf)]


def _where(bad, limit=4):
    pos = np.flatnonzero(bad)
    return "%d element(s), first at %s" % (pos.size, [int(p) for p in pos[:limit]])


def check_unchanged(before, after, what="buffer"):
    """every scalar of `after` equals `before` bit for bit (both planes of split storage)"""
    for (name, b), (_, a) in zip(_planes(before), _planes(after)):
        b, a = np.asarray(b), np.asarray(a)
        assert a.shape == b.shape, (what, name, a.shape, b.shape)
        bb, ab = _scalar_bits(b), _scalar_bits(a)
        if b.dtype.kind == "c":
            bad = (bb.reshape(-1, 2) != ab.reshape(-1, 2)).any(axis=1)
        else:
            bad = bb != ab
        assert not bad.any(), "%s%s changed: %s" % (what, " (%s plane)" % name if name else "", _where(bad))


def check_guards(alloc, lo, count, pad=PADDING_VALUE, what="buffer"):
    """alloc: a whole allocation (or its two planes) = `lo` guard elements, the `count` elements of the user's buffer,
    guard elements up to the end.  Both guards must still hold the padding value, bit for bit."""
    for name, a in _planes(alloc):
        a = np.asarray(a)
        want = _scalar_bits(full(1, pad, a.dtype))
        bits = _scalar_bits(a).reshape(a.size, -1)
        bad = (bits != want.reshape(1, -1)).any(axis=1)
        plane = " (%s plane)" % name if name else ""
        before, after = bad[:lo], bad[lo + count:]
        assert not before.any(), "%s%s: the guard before the buffer was written at element(s) %s" % (
            what, plane, [int(p) - lo for p in np.flatnonzero(before)[:4]])
        assert not after.any(), "%s%s: the guard after the buffer was written at element(s) %s" % (
            what, plane, [count + int(p) for p in np.flatnonzero(after)[:4]])


def check_write_set(buf, index_set, pad=PADDING_VALUE, what="output"):
    """buf: a whole user buffer (or its two planes).  Every element outside `index_set` (flat indices, e.g. the output
    domain's element_indices) must still hold the padding value, bit for bit."""
    for name, a in _planes(buf):
        a = np.asarray(a)
        outside = np.ones(a.size, dtype=bool)
        idx = np.asarray(index_set, dtype=np.int64).ravel()
        outside[idx[idx < a.size]] = False
        want = _scalar_bits(full(1, pad, a.dtype))
        bad = outside & (_scalar_bits(a).reshape(a.size, -1) != want.reshape(1, -1)).any(axis=1)
        assert not bad.any(), "%s%s: written outside its index set: %s" % (
            what, " (%s plane)" % name if name else "", _where(bad))


# ---------------------------------------------------------------------------------------------------------------------
# read sets: what a result may depend on.  Two runs that differ only in values that must not matter agree bit for bit,
# and a poisoned value that must matter reaches every result that depends on it.

def rows_of(distance, offset=0, names=("row", "element")):
    """locate= of check_isolated for rows `distance` elements apart: flat index -> "(row r, element e)" """
    return lambda p: "(%s %d, %s %d)" % (names[0], (p - offset) // distance, names[1], (p - offset) % distance)


def frames_of(out_pitch, frame_pitch, names=("signal", "frame", "bin")):
    """locate= of check_isolated for frame-major outputs: flat index -> "(signal i, frame f, bin k)" """
    return lambda p: "(%s %d, %s %d, %s %d)" % (names[0], p // out_pitch, names[1], p % out_pitch // frame_pitch,
                                                 names[2], p % out_pitch % frame_pitch)


def check_isolated(clean, poisoned, untainted, tainted, what, locate=None, every_scalar=False):
    """clean, poisoned: the whole output buffers of two runs of one plan (numpy; real, complex, or the (re, im) planes of
    split storage) that differ only in poisoned values.  untainted, tainted: flat element indices.  Every scalar at an
    untainted index must be bit-identical in the two runs; every element at a tainted index must be non-finite in the
    poisoned run -- a complex element in at least one component, with every_scalar=True in both.  A failure names `what`,
    the first offending flat index and, through locate(index), its (row, element) or (signal, frame, bin)."""
    cp, pp = _planes(clean), _planes(poisoned)
    assert len(cp) == len(pp), (what, "planes")
    un = np.asarray(untainted, dtype=np.int64).ravel()
    ta = np.asarray(tainted, dtype=np.int64).ravel()
    assert np.intersect1d(un, ta).size == 0, (what, "an index is both tainted and untainted")
    where = (lambda p: " " + locate(int(p))) if locate is not None else (lambda p: "")
    finite = None
    for (name, c), (_, q) in zip(cp, pp):
        c, q = np.asarray(c), np.asarray(q)
        assert c.shape == q.shape and c.dtype == q.dtype and c.ndim == 1, (what, name, c.shape, q.shape, c.dtype, q.dtype)
        plane = " (%s plane)" % name if name else ""
        cb, qb = _scalar_bits(c).reshape(c.size, -1), _scalar_bits(q).reshape(q.size, -1)
        bad = (cb[un] != qb[un]).any(axis=1)
        if bad.any():
            first = un[np.flatnonzero(bad)[0]]
            raise AssertionError("%s%s: depends on a value it must not read: %d untainted element(s) differ between the "
                                 "clean and the poisoned run, first at %d%s: clean %r, poisoned %r" % (
                                     what, plane, int(bad.sum()), int(first), where(first), c[first], q[first]))
        parts = [q.real, q.imag] if q.dtype.kind == "c" else [q]
        for part in parts:
            f = np.isfinite(part[ta].astype(np.float64))
            finite = f if finite is None else (finite | f if every_scalar else finite & f)
    if finite is not None and finite.any():
        first = ta[np.flatnonzero(finite)[0]]
        vals = [np.asarray(q)[first] for _, q in pp]
        raise AssertionError("%s: drops a value it must propagate: %d tainted element(s) are finite in the poisoned run, "
                             "first at %d%s: %r" % (what, int(finite.sum()), int(first), where(first),
                                                    vals[0] if len(vals) == 1 else tuple(vals)))


def frame_sources(n, hop, lead, pad, n_frames, in_length):
    """[n_frames, n] the sample of the signal that element j of frame f reads, -1 for a zero of the extension: the
    definition of pfft_execute_stft (include/portfft_amd.h): xe[f * hop - lead + j], xe = x extended by zeros ("zero")
    or xe[-p] = x[p], xe[L - 1 + p] = x[L - 1 - p] ("reflect")"""
    e = np.arange(n_frames, dtype=np.int64)[:, None] * hop - lead + np.arange(n, dtype=np.int64)[None, :]
    if pad == "reflect":
        e = np.where(e < 0, -e, e)
        e = np.where(e >= in_length, 2 * (in_length - 1) - e, e)
        assert e.min() >= 0 and e.max() < in_length, "an index reflected twice"
        return e
    assert pad == "zero"
    return np.where((e >= 0) & (e < in_length), e, -1)


def taint_frames(t, n, hop, lead, pad, n_frames, in_length):
    """the frames of stft (frames of n = N samples) or mdct (n = 2N, hop = N, "zero") whose extended index set contains
    input sample t"""
    return np.flatnonzero((frame_sources(n, hop, lead, pad, n_frames, in_length) == t).any(axis=1))


def taint_periodogram_rows(t, n, hop, lead, pad, n_frames, in_length, avg_frames):
    """the output rows c = f // avg_frames of periodogram that sum a frame containing input sample t"""
    return np.unique(taint_frames(t, n, hop, lead, pad, n_frames, in_length) // avg_frames)


def taint_samples(f, n, hop, lead, out_length):
    """the output samples of istft (frames of n = N samples) or imdct (n = 2N, hop = N) that frame f covers:
    0 <= t + lead - f * hop < n, t < out_length"""
    t = np.arange(out_length, dtype=np.int64)
    u = t + lead - f * hop
    return t[(u >= 0) & (u < n)]


def filter_geometry(n, k, correlate, real):
    """(hop, lead) of overlap-save with N-point segments and K taps (include/portfft_amd.h): segment s holds the input
    samples [s * hop - lead, s * hop - lead + N) and stores the outputs [s * hop, (s + 1) * hop).  Complex: hop = N - K + 1,
    lead = K - 1 (convolve) or 0 (correlate).  Real: the geometry is even -- lead = K - 1 rounded up and hop = N - lead
    (convolve), hop = N - K + 1 rounded down (correlate)."""
    if not real:
        return n - k + 1, 0 if correlate else k - 1
    if correlate:
        return (n - k + 1) // 2 * 2, 0
    lead = (k - 1 + 1) // 2 * 2
    return n - lead, lead


def taint_filter(t, n, k, correlate, real, out_length):
    """(required, permitted) output samples of `filter` that depend on input sample t.  required: the mathematical cone,
    y[t ... t + K - 1] (convolve) or y[t - K + 1 ... t] (correlate), clipped to [0, out_length).  permitted: every output
    of every segment whose N-sample window contains t (the segment is the unit of work)."""
    lo, hi = (t - k + 1, t + 1) if correlate else (t, t + k)
    required = np.arange(max(lo, 0), min(hi, out_length), dtype=np.int64)
    hop, lead = filter_geometry(n, k, correlate, real)
    s = np.arange(-(-out_length // hop), dtype=np.int64)
    first = s * hop - lead
    hit = s[(first <= t) & (t < first + n)]
    permitted = (hit[:, None] * hop + np.arange(hop, dtype=np.int64)[None, :]).ravel()
    return required, permitted[permitted < out_length]


# ---------------------------------------------------------------------------------------------------------------------
# every transform against an fp64 reference: a direct DFT at a few probed bins per transform (torch, on the data's
# device -- CPU tensors too)

PROBE_TAU = {"f32": 4 * REL_L2_TOL[np.dtype(np.complex64)], "f64": 1e-12}
PROBE_FIXED = 3  # probes at flat bins 0, N/2, N-1 of every transform
PROBE_BLOCK = 1 << 14  # terms per partial sum of the reference


def _probe_bins(lengths, batch, k_rot, b0, b1, torch, dev):
    """per-axis bins [b1 - b0, k_rot + 3, rank] probed in transforms b0 .. b1-1, and the per-axis shift of each transform:
    transform b probes the flat bins (j + b * k_rot) mod N (j < k_rot, carried per axis) and the fixed bins"""
    n = int(np.prod(lengths))
    rank = len(lengths)
    dims = torch.tensor(lengths, dtype=torch.int64, device=dev)
    inner = torch.tensor(default_strides(lengths), dtype=torch.int64, device=dev)
    b = torch.arange(b0, b1, dtype=torch.int64, device=dev)
    shift = ((b * k_rot) % n)[:, None] // inner[None, :] % dims[None, :]                      # [bc, rank]
    base = torch.arange(k_rot, dtype=torch.int64, device=dev)[:, None] // inner % dims        # [k_rot, rank]
    fixed = torch.tensor([0, n // 2, n - 1], dtype=torch.int64, device=dev)[:, None] // inner % dims
    rot = (base[None, :, :] + shift[:, None, :]) % dims                                        # [bc, k_rot, rank]
    return torch.cat([rot, fixed[None].expand(b1 - b0, PROBE_FIXED, rank)], dim=1), shift, base, fixed


def _gather(buf, idx, torch):
    """complex128 values of a flat buffer (or its two planes) at the int64 indices `idx`"""
    if isinstance(buf, (tuple, list)):
        return torch.complex(buf[0][idx].double(), buf[1][idx].double())
    return buf[idx].to(torch.complex128)


def check_every_transform(x, y, lengths, batch, in_layout=None, out_layout=None, scale=1.0, direction=FORWARD,
                          prec="f32", what="", k=8, chunk_bytes=256 << 20, tau=None):
    """Compare EVERY transform of an execute with an fp64 direct DFT at k bins: k - 3 bins that move with the transform
    index (transform b: flat bins (j + b (k - 3)) mod N, so that across a batch of N / (k - 3) transforms every bin is
    probed) and the fixed bins 0, N/2, N-1.  x, y: flat torch tensors (complex, or the (re, im) planes of split storage)
    holding the input / output domain laid out as `in_layout` / `out_layout` = (strides, distance, offset) (None:
    packed).  The reference is formed with phases reduced exactly in int64, (n k) mod N, angles in fp64 and one
    complex128 matmul per chunk of at most `chunk_bytes` of fp64 data.  Criterion per transform b and probed bin:
    |Y_b[k] - s R_b[k]| <= tau |s| ||x_b||_2 (tau: PROBE_TAU).  Returns {max, tau, transforms, probes}; max is the
    largest |Y - s R| / (|s| ||x_b||)."""
    import torch
    lengths = [int(v) for v in lengths]
    rank, n = len(lengths), int(np.prod(lengths))
    tau = PROBE_TAU[prec] if tau is None else tau
    k_rot = k - PROBE_FIXED
    assert k_rot >= 1
    dev = (x[0] if isinstance(x, (tuple, list)) else x).device
    sign = -1.0 if direction == FORWARD else 1.0
    packed = (default_strides(lengths), n, 0)
    in_s, in_d, in_o = in_layout or packed
    out_s, out_d, out_o = out_layout or packed
    dims = torch.tensor(lengths, dtype=torch.int64, device=dev)
    inner = torch.tensor(default_strides(lengths), dtype=torch.int64, device=dev)
    in_st = torch.tensor([int(s) for s in in_s], dtype=torch.int64, device=dev)
    out_st = torch.tensor([int(s) for s in out_s], dtype=torch.int64, device=dev)
    elems = max(1, chunk_bytes // 16)
    n_chunk = min(n, elems)
    b_chunk = max(1, elems // n_chunk)
    worst, worst_at = 0.0, None
    two_pi = 2.0 * np.pi
    for b0 in range(0, batch, b_chunk):
        b1 = min(batch, b0 + b_chunk)
        bins, shift, base, fixed = _probe_bins(lengths, batch, k_rot, b0, b1, torch, dev)
        b = torch.arange(b0, b1, dtype=torch.int64, device=dev)
        r_rot = torch.zeros(b1 - b0, k_rot, dtype=torch.complex128, device=dev)
        r_fix = torch.zeros(b1 - b0, PROBE_FIXED, dtype=torch.complex128, device=dev)
        norm2 = torch.zeros(b1 - b0, dtype=torch.float64, device=dev)
        for n0 in range(0, n, n_chunk):
            flat = torch.arange(n0, min(n, n0 + n_chunk), dtype=torch.int64, device=dev)
            na = flat[:, None] // inner[None, :] % dims[None, :]                                # [nc, rank]
            xc = _gather(x, in_o + b[:, None] * in_d + (na * in_st).sum(1)[None, :], torch)  # [bc, nc]
            norm2 += (xc.real ** 2 + xc.imag ** 2).sum(1)
            # modulation by the transform's shift: exp(sign 2 pi i sum_a ((n_a c_a) mod N_a) / N_a)
            frac = (((na[None, :, :] * shift[:, None, :]) % dims) .double() / dims.double()).sum(2)
            xm = xc * torch.polar(torch.ones_like(frac), sign * two_pi * torch.frac(frac))
            del frac
            nc = flat.numel()
            blk = PROBE_BLOCK if nc % PROBE_BLOCK == 0 and nc > PROBE_BLOCK else nc
            for mat, rhs, acc in ((base, xm, r_rot), (fixed, xc, r_fix)):
                f = (((na[:, None, :] * mat[None, :, :]) % dims).double() / dims.double()).sum(2)   # [nc, kk]
                e = torch.polar(torch.ones_like(f), sign * two_pi * torch.frac(f))
                # the sum in blocks of PROBE_BLOCK terms, the block sums added pairwise: a long transform's reference
                # keeps its fp64 accuracy
                part = torch.matmul(rhs.reshape(-1, nc // blk, blk).transpose(0, 1), e.reshape(nc // blk, blk, -1))
                acc += part.sum(0)
            del xc, xm
        ref = torch.cat([r_rot, r_fix], dim=1) * scale
        got = _gather(y, out_o + b[:, None] * out_d + (bins * out_st).sum(2), torch)
        err = (got - ref).abs() / (abs(scale) * norm2.sqrt().clamp_min(1e-300))[:, None]
        m = float(err.max())
        if not (m <= worst) or worst_at is None:
            i = int(torch.argmax(err))
            worst, worst_at = m, (b0 + i // k, [int(v) for v in bins.reshape(-1, rank)[i]])
        if not (m <= tau):
            bad = (~(err <= tau)).nonzero()
            tb, jb = int(bad[0, 0]), int(bad[0, 1])
            raise AssertionError("%s: transform %d of %d, bin %s: |Y - sR| / (|s| ||x||) = %.3g > tau = %.3g (%d bad probes "
                                 "in transforms %d .. %d)" % (what, b0 + tb, batch, [int(v) for v in bins[tb, jb]],
                                                               float(err[tb, jb]), tau, bad.shape[0], b0, b1 - 1))
    stats = {"what": str(what), "max": worst, "tau": tau, "transforms": batch, "probes": batch * k, "worst_at": worst_at}
    _log_probe(stats)
    return stats


def _log_probe(stats):
    import json
    import os
    path = os.environ.get("PFFT_TEST_PROBE_LOG")
    if path:
        stats = dict(stats, test=os.environ.get("PYTEST_CURRENT_TEST", "").split(" ")[0])
        with open(path, "a") as f:
            f.write(json.dumps(stats) + "\n")


# ---------------------------------------------------------------------------------------------------------------------
# every output element of a launch of several GiB, on the data's device (torch; CPU tensors too): periodic inputs, a
# small fp64 reference, one criterion per work-group row

def periodic_signal(base, i, t0, t1, length):
    """samples t0 .. t1-1 of signal i of a periodic test input (numpy): x_i[t] = base[(t + i) mod P] for 0 <= t < length,
    zero outside"""
    t = np.arange(t0, t1, dtype=np.int64)
    x = np.asarray(base)[(t + i) % len(base)].copy()
    x[(t < 0) | (t >= length)] = 0
    return x


def fill_periodic(buf, base, n_signals, length, pitch, torch, chunk=1 << 24):
    """write x_i[t] = base[(t + i) mod P] into buf[i * pitch + t] (t < length); everything else of buf is left alone.
    buf: flat torch tensor, base: 1-D torch tensor of buf's dtype on its device"""
    p = base.numel()
    per = max(1, chunk // length)
    for i0 in range(0, n_signals, per):
        i1 = min(n_signals, i0 + per)
        for t0 in range(0, length, chunk):
            t1 = min(length, t0 + chunk)
            i = torch.arange(i0, i1, dtype=torch.int64, device=buf.device)[:, None]
            t = torch.arange(t0, t1, dtype=torch.int64, device=buf.device)[None, :]
            if i1 - i0 == 1:
                buf[i0 * pitch + t0:i0 * pitch + t1] = base[((t + i) % p).reshape(-1)]
            else:
                buf[(i * pitch + t).reshape(-1)] = base[((t + i) % p).reshape(-1)]


def check_periodic(buf, base, n_signals, length, pitch, torch, what="input", chunk=1 << 24):
    """buf[i * pitch + t] still holds base[(t + i) mod P], bit for bit (what fill_periodic wrote), compared with the
    generator chunk by chunk: no second buffer"""
    p = base.numel()
    per = max(1, chunk // length)
    for i0 in range(0, n_signals, per):
        i1 = min(n_signals, i0 + per)
        for t0 in range(0, length, chunk):
            t1 = min(length, t0 + chunk)
            i = torch.arange(i0, i1, dtype=torch.int64, device=buf.device)[:, None]
            t = torch.arange(t0, t1, dtype=torch.int64, device=buf.device)[None, :]
            pos = (i * pitch + t).reshape(-1)
            got = buf[i0 * pitch + t0:i0 * pitch + t1] if i1 - i0 == 1 else buf[pos]
            bad = (_bit_rows(got, torch) != _bit_rows(base[((t + i) % p).reshape(-1)], torch)).any(dim=1)
            if bool(bad.any()):
                raise AssertionError("%s changed: %d element(s), first at %s" % (
                    what, int(bad.sum()), [int(v) for v in pos[bad][:4]]))


def _ulp16(v, torch):
    """np.spacing of |v| rounded to binary16, as float64 (torch)"""
    a = v.abs().to(torch.float16).double()
    _, e = torch.frexp(a)
    ulp = torch.ldexp(torch.ones_like(a), e - 11).clamp_min(2.0 ** -24)
    return torch.where(a == 0, torch.full_like(a, 2.0 ** -24), ulp)


def check_rows(out, start, valid, key, ref, tol, what="", rule_n=None, pairs=False, fp16=False, chunk=1 << 24):
    """Every row of a launch against a small fp64 reference, on out's device.  Row r of the launch -- one transform, one
    overlap-save segment's hop outputs, one STFT frame: what one work-group row stores -- is out[start[r] : start[r] +
    valid[r]] and must equal ref[key[r], :valid[r]].  out: the flat user buffer (torch; complex, real, or with
    pairs=True a real tensor of interleaved (re, im) scalars indexed in complex elements); start, valid, key: int64
    sequences of one entry per row; ref: (rows of the reference, W) float64 / complex128.  Criterion PER ROW: relative
    L2 over the row's valid elements <= tol (a float, or one value per reference row), never one norm over the whole
    buffer: a single wrong row fails, and the error names it.  rule_n: also helpers.check_reference_rule's per-element
    abs-or-rel rule with n = rule_n.  fp16: also test_gpu_half's per-component rule |out - Y| <= ulp16(Y) + 1e-6 max|Y|.

    The inputs these references belong to are periodic: row b holds base[b mod P], a long signal base[t mod P], with P
    an odd prime.  BLIND SPOT: a result displaced by a whole multiple of P rows (samples) equals the correct one.  An
    address that wrapped in 32 bits displaces by a power of two bytes, hence by a power of two rows or samples (or a
    fraction of one), which an odd prime never divides -- so wrap-around cannot hide; any other displacement can, which is
    why every case is launched a second time on random data and checked at marked rows.  Returns the worst rel-L2."""
    import torch
    dev = out.device
    start = torch.as_tensor(np.asarray(start, dtype=np.int64), device=dev)
    valid = torch.as_tensor(np.asarray(valid, dtype=np.int64), device=dev)
    key = torch.as_tensor(np.asarray(key, dtype=np.int64), device=dev)
    ref = torch.as_tensor(ref, device=dev)
    ref = ref.to(torch.complex128 if ref.is_complex() else torch.float64)
    rows, w = start.numel(), ref.shape[1]
    tol_t = torch.as_tensor(tol, dtype=torch.float64, device=dev).expand(ref.shape[0]) if np.ndim(tol) else None
    rule = None
    if rule_n is not None:
        single = out.dtype in (torch.complex64, torch.float32)
        rule = reference_tolerance(np.complex64 if single else np.complex128, rule_n)
    cols = torch.arange(w, dtype=torch.int64, device=dev)[None, :]
    per = max(1, chunk // w)
    worst, worst_row = 0.0, -1
    for r0 in range(0, rows, per):
        r1 = min(rows, r0 + per)
        live = cols < valid[r0:r1, None]
        idx = torch.where(live, start[r0:r1, None] + cols, start[r0:r1, None])
        if pairs:
            got = torch.complex(out[2 * idx].double(), out[2 * idx + 1].double())
        else:
            got = out[idx].to(ref.dtype)
        k = key[r0:r1]
        exp = ref[k]
        zero = torch.zeros((), dtype=ref.dtype, device=dev)
        diff = torch.where(live, got - exp, zero)
        expv = torch.where(live, exp, zero)
        den = torch.linalg.vector_norm(expv, dim=1).clamp_min(1e-300)
        err = torch.linalg.vector_norm(diff, dim=1) / den
        lim = tol_t[k] if tol_t is not None else torch.full_like(err, float(tol))
        bad = ~(err <= lim)
        if rule is not None:
            absd = diff.abs()
            bad |= (~((absd <= rule) | (absd <= rule * expv.abs()))).any(dim=1)
        if fp16:
            slack = 1e-6 * expv.abs().amax(dim=1, keepdim=True)
            parts = ((diff.real, expv.real), (diff.imag, expv.imag)) if ref.is_complex() else ((diff, expv),)
            for dpart, epart in parts:
                bad |= (live & ~(dpart.abs() <= _ulp16(epart, torch) + slack)).any(dim=1)
        if bool(bad.any()):
            b = int(bad.nonzero()[0, 0])
            raise AssertionError("%s: row %d of %d (element %d of the buffer, reference row %d): rel-L2 %.3g, limit %.3g%s; "
                                 "%d bad row(s) among rows %d .. %d" % (
                                     what, r0 + b, rows, int(start[r0 + b]), int(k[b]), float(err[b]), float(lim[b]),
                                     "" if float(err[b]) > float(lim[b]) else " (per-element rule)", int(bad.sum()), r0,
                                     r1 - 1))
        m = float(err.max())
        if m > worst:
            worst, worst_row = m, r0 + int(torch.argmax(err))
    print("%s: %d rows, worst rel-L2 %.3e (row %d)" % (what, rows, worst, worst_row))
    return worst


def _bit_rows(t, torch):
    """the bits of every element of a flat tensor as (elements, k) integers"""
    if t.is_complex():
        t = torch.view_as_real(t)
    it = {2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()]
    return t.contiguous().view(it).reshape(t.shape[0], -1) if t.dim() > 1 else t.view(it).reshape(-1, 1)


def check_untouched(buf, start, valid, pad=PADDING_VALUE, what="output", unit=1, chunk=1 << 26):
    """Every element of the flat torch tensor `buf` outside the rows [start[r], start[r] + valid[r]) still holds the
    padding value, bit for bit -- the gaps between pitched signals and frames included.  On buf's device, in chunks;
    unit: scalars of buf per indexed element (2 for interleaved fp16 pairs)."""
    import torch
    dev = buf.device
    count = buf.numel() // unit
    written = torch.zeros(count, dtype=torch.bool, device=dev)
    start = torch.as_tensor(np.asarray(start, dtype=np.int64), device=dev)
    valid = torch.as_tensor(np.asarray(valid, dtype=np.int64), device=dev)
    w = int(valid.max()) if valid.numel() else 0
    if w > (1 << 16):  # a few long rows (whole signals): slices
        for s0, v in zip(start.tolist(), valid.tolist()):
            written[s0:s0 + v] = True
    else:
        cols = torch.arange(w, dtype=torch.int64, device=dev)[None, :]
        per = max(1, (chunk // 4) // max(w, 1))
        for r0 in range(0, start.numel(), per):
            idx = start[r0:r0 + per, None] + cols
            written[idx[cols < valid[r0:r0 + per, None]]] = True
    want = _bit_rows(full_torch(1, pad, buf.dtype, dev), torch)
    if unit > 1:
        want = want.reshape(1, 1).expand(1, unit)
    for c0 in range(0, count, chunk):
        c1 = min(count, c0 + chunk)
        bits = _bit_rows(buf[c0 * unit:c1 * unit], torch)
        if unit > 1:
            bits = bits.reshape(c1 - c0, unit)
        bad = (bits != want).any(dim=1) & ~written[c0:c1]
        if bool(bad.any()):
            pos = bad.nonzero()[:4, 0] + c0
            raise AssertionError("%s: written outside its index set: %d element(s) in [%d, %d), first at %s" % (
                what, int(bad.sum()), c0, c1, [int(p) for p in pos]))


def check_same_bits(a, b, what="buffer", chunk=1 << 26):
    """two flat torch tensors of one type hold the same bits (on their device, in chunks)"""
    import torch
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    for c0 in range(0, a.numel(), chunk):
        x, y = _bit_rows(a[c0:c0 + chunk], torch), _bit_rows(b[c0:c0 + chunk], torch)
        bad = (x != y).any(dim=1)
        if bool(bad.any()):
            raise AssertionError("%s changed: %d element(s) in [%d, %d), first at %s" % (
                what, int(bad.sum()), c0, c0 + bad.numel(), [int(p) + c0 for p in bad.nonzero()[:4, 0]]))


def filter_rows(base, taps, c, n_signals, in_length, out_length, out_pitch, hop, correlate):
    """The rows of an overlap-save launch on the periodic input x_i[t] = base[(t + i) mod P] (periodic_signal) with filter
    i mod F of taps (F, K): row (i, s) is the `hop` outputs from sample s * hop of signal i.  Returns (start, valid, key,
    ref) for check_rows, all fp64 and by direct sums (np.convolve / np.correlate):
      y_i[t] = c sum_k h[k] x_i[t - k]   or, correlate,   c sum_k conj(h[k]) x_i[t + k],   x_i zero outside [0, in_length)
    A row whose sums stay inside the signal depends only on the filter and on (s * hop + i) mod P: P references per
    filter.  The other rows -- a signal's first (convolve) and the ones that reach its end -- depend on (i mod P, i mod F,
    s) and are summed on their own."""
    base = np.asarray(base)
    taps = np.asarray(taps)
    taps = taps.astype(np.complex128 if taps.dtype.kind == "c" else np.float64)
    based = base.astype(np.complex128 if base.dtype.kind == "c" else np.float64)
    p, (nf, k) = len(base), taps.shape
    n_seg = -(-out_length // hop)
    i = np.repeat(np.arange(n_signals, dtype=np.int64), n_seg)
    s = np.tile(np.arange(n_seg, dtype=np.int64), n_signals)
    first = s * hop
    valid = np.minimum(hop, out_length - first)
    lo = first if correlate else first - (k - 1)        # the samples a row's sums read: [lo, first + valid + k - 1) or
    hi = first + valid + (k - 1 if correlate else 0)    # [lo, first + valid)
    inner = (lo >= 0) & (hi <= in_length) & (valid == hop)
    key = (i % nf) * p + (first + i) % p
    refs = np.zeros((nf * p, hop), dtype=np.result_type(based.dtype, taps.dtype))

    def sums(x, h, count):
        full = np.correlate(x, h, "valid") if correlate else np.convolve(x, h, "valid")
        return c * full[:count]

    for f in range(nf):
        for ph in range(p):
            t = np.arange(hop + k - 1, dtype=np.int64) + ph - (0 if correlate else k - 1)
            refs[f * p + ph] = sums(based[t % p], taps[f], hop)
    extra, memo = [], {}
    for r in np.flatnonzero(~inner):
        sig = (int(i[r]) % p, int(i[r]) % nf, int(s[r]))
        if sig not in memo:
            x = periodic_signal(based, int(i[r]), int(first[r]) - (0 if correlate else k - 1),
                                int(first[r]) + hop + (k - 1 if correlate else 0), in_length)
            memo[sig] = nf * p + len(extra)
            extra.append(sums(x, taps[sig[1]], hop))
        key[r] = memo[sig]
    ref = np.concatenate([refs, np.array(extra).reshape(len(extra), hop)]) if extra else refs
    return i * out_pitch + first, valid, key, ref


def stft_frame(x_of, window, scale, n, e0, in_length, pad):
    """scale * rfft(window * xe[e0 : e0 + n]) in double; x_of(t0, t1): samples t0 .. t1-1 of the signal (inside it), xe its
    extension by zeros or by np.pad's "reflect" """
    t = np.arange(e0, e0 + n, dtype=np.int64)
    if pad == "reflect":
        t = np.where(t < 0, -t, t)
        t = np.where(t >= in_length, 2 * (in_length - 1) - t, t)
        assert t.min() >= 0 and t.max() < in_length
        inside = np.ones(n, dtype=bool)
    else:
        inside = (t >= 0) & (t < in_length)
    frame = np.zeros(n, dtype=np.float64)
    if inside.any():
        lo, hi = int(t[inside].min()), int(t[inside].max()) + 1
        frame[inside] = np.asarray(x_of(lo, hi), dtype=np.float64)[t[inside] - lo]
    return scale * np.fft.rfft(frame * window)


def stft_rows(base, window, scale, n, n_signals, in_length, hop, lead, pad, n_frames, frame_pitch, out_pitch):
    """The rows (frames) of an STFT launch on the periodic input x_i[t] = base[(t + i) mod P]: (start, valid, key, ref) for
    check_rows.  A frame inside its signal is determined by (f * hop - lead + i) mod P: P rffts.  Frames that touch an
    end (zeros or reflection) depend on (i mod P, f) and are computed on their own."""
    based = np.asarray(base, dtype=np.float64)
    p, m = len(based), n // 2
    wd = np.ones(n) if window is None else np.asarray(window, dtype=np.float64)
    i = np.repeat(np.arange(n_signals, dtype=np.int64), n_frames)
    f = np.tile(np.arange(n_frames, dtype=np.int64), n_signals)
    e0 = f * hop - lead
    inner = (e0 >= 0) & (e0 + n <= in_length)
    key = (e0 + i) % p
    t = np.arange(n, dtype=np.int64)
    refs = [scale * np.fft.rfft(based[(t + ph) % p] * wd) for ph in range(p)]
    memo = {}
    for r in np.flatnonzero(~inner):
        sig = (int(i[r]) % p, int(f[r]))
        if sig not in memo:
            memo[sig] = len(refs)
            refs.append(stft_frame(lambda a, b, ii=int(i[r]): periodic_signal(based, ii, a, b, in_length), wd, scale, n,
                                   int(e0[r]), in_length, pad))
        key[r] = memo[sig]
    return i * out_pitch + f * frame_pitch, np.full(i.size, m + 1, dtype=np.int64), key, np.array(refs)


# ---------------------------------------------------------------------------------------------------------------------
# basis vectors: the transform of a unit impulse is one row of the transform's matrix, every butterfly sees at most one
# non-zero operand, and an output element is a product of the twiddles on its path.  Its error has a derived bound.

BASIS_U = {"f16": 2.0 ** -24, "f32": 2.0 ** -24, "f64": 2.0 ** -53}  # unit round-off of the plan's arithmetic
BASIS_MUL = 3.3  # one multiply on the path: a stored twiddle within u, a complex product within sqrt(5) u; 1 + sqrt(5) < 3.3
BASIS_KINDS = ("c2c", "r2c", "c2r", "dct2", "dct3", "dct4")
BASIS_REF_MARGIN = 16.0  # the reference's own error stays at or below bound / 16


def twiddle_path_length(n):
    """P(n) = ceil(log2 n) + (odd prime factors of n, with multiplicity) + 1: no more twiddle multiplies than this lie on
    the path of one output element of an n-point transform of a unit impulse.  A radix-2^a pass has at most a - 1 internal
    levels plus one inter-pass twiddle, so the powers of two cost at most log2 n in all; an odd prime radix costs its
    constant and the inter-pass twiddle.  P(1) = 1."""
    n = int(n)
    assert n >= 1
    odd, m, p = 0, n, 3
    while m % 2 == 0:
        m //= 2
    while p * p <= m:
        while m % p == 0:
            odd, m = odd + 1, m // p
        p += 2
    odd += m > 1
    return (n - 1).bit_length() + odd + 1


def basis_multiplies(n, kind):
    """the count c of the bound amplitude * 3.3 u c of a family: the sum of P over the axes (complex; n an int or the
    dims), P(N/2) + 3 (R2C, C2R: the untangle step sees one non-zero term), P(N/2) + 4 (DCT-II / III / IV)"""
    if kind == "c2c":
        return sum(twiddle_path_length(v) for v in (n if np.ndim(n) else [n]))
    assert kind in BASIS_KINDS and int(n) % 2 == 0, (kind, n)
    return twiddle_path_length(int(n) // 2) + (3 if kind in ("r2c", "c2r") else 4)


def basis_amplitude(kind):
    """the largest modulus of a reference element: 1 (complex rows, R2C), 2 (C2R of a unit bin, the DCTs)"""
    return 1.0 if kind in ("c2c", "r2c") else 2.0


def basis_bound(n, kind, prec, scale=1.0):
    """per-element bound on |got - ref| for the transform of a unit impulse (fp16 storage: add half a binary16 ulp of
    the reference component)"""
    return abs(scale) * basis_amplitude(kind) * BASIS_MUL * BASIS_U[prec] * basis_multiplies(n, kind)


def _octant_circle(length, dtype):
    """(cos, sin)(2 pi p / length), p = 0 .. length - 1, in `dtype`, every angle reduced exactly (in integers) to
    [0, pi/4]: pi = 4 arctan(1) in dtype, the multiples of a quarter turn exact"""
    p = np.arange(length, dtype=np.int64)
    octant, r = np.divmod(8 * p, length)                    # angle = (octant + r / length) pi / 4
    odd = (octant & 1).astype(bool)
    r = np.where(odd, length - r, r)                        # an odd octant counts back from its upper end
    phi = (np.arctan(dtype(1)) * r.astype(dtype)) / dtype(length)
    a, b = np.cos(phi), np.sin(phi)
    q = (octant + 1) // 2 % 4                               # the nearest multiple of pi/2: angle = q pi/2 +- phi
    sg = np.where(odd, dtype(-1), dtype(1))                 # (odd octants lie below it)
    c = np.select([q == 0, q == 1, q == 2], [a, -sg * b, -a], sg * b)
    s = np.select([q == 0, q == 1, q == 2], [sg * b, a, -sg * b], -a)
    return c.astype(dtype), s.astype(dtype)


_circles = {}


def basis_circle(length, route=None):
    """The unit circle at `length` points, (cos, sin) with exactly reduced phases, for the basis references.  route
    "longdouble": np.longdouble with at least 63 mantissa bits (error about 2^-63); "float64": fp64 with the phase
    reduced to the first octant (error below 2^-52).  None: longdouble where the platform has it, else float64."""
    if route is None:
        route = "longdouble" if np.finfo(np.longdouble).nmant >= 63 else "float64"
    key = (int(length), route)
    if key not in _circles:
        if len(_circles) >= 6:
            _circles.pop(next(iter(_circles)))
        if route == "longdouble":
            assert np.finfo(np.longdouble).nmant >= 63, "np.longdouble is no wider than double here"
            _circles[key] = _octant_circle(int(length), np.longdouble)
        else:
            _circles[key] = _octant_circle(int(length), np.float64)
    return _circles[key]


def basis_table_length(n, kind):
    """L of basis_phase: the lcm of the dims (c2c), N (r2c, c2r), 4N (dct2, dct3), 8N (dct4)"""
    if kind == "c2c":
        return int(np.lcm.reduce([int(v) for v in (n if np.ndim(n) else [n])]))
    return int(n) * {"r2c": 1, "c2r": 1, "dct2": 4, "dct3": 4, "dct4": 8}[kind]


def basis_phase(rows, cols, n, kind):
    """(table length L, index [rows, cols] into basis_circle(L), weight [rows, 1] or None) of the reference of `kind`:
    integer arithmetic only (int64 numpy arrays or torch tensors; rows a column, cols a row vector).
      c2c   exp(-+2 pi i sum_a j_a k_a / N_a): L = lcm of the dims, index sum_a ((j_a k_a) mod N_a) L / N_a mod L
      r2c   exp(-2 pi i j k / N), k = 0 .. N/2
      c2r   of the unit bin k0: 2 cos(2 pi k0 t / N), weight 1 at k0 = 0 and N/2
      dct2  of e_j: 2 cos(pi k (2j + 1) / 2N): L = 4N, index k (2j + 1) mod 4N
      dct3  of e_j: 2 cos(pi j (2k + 1) / 2N), weight 1 at j = 0
      dct4  of e_j: 2 cos(pi (2j + 1)(2k + 1) / 4N): L = 8N, index (2j + 1)(2k + 1) mod 8N"""
    if kind == "c2c":
        dims = [int(v) for v in (n if np.ndim(n) else [n])]
        big = basis_table_length(n, kind)
        idx, inner = 0, int(np.prod(dims))
        for d in dims:
            inner //= d
            idx = idx + ((rows // inner % d) * (cols // inner % d)) % d * (big // d)
        return big, idx % big, None
    n = int(n)
    if kind == "r2c":
        return n, (rows * cols) % n, None
    if kind == "c2r":
        return n, (rows * cols) % n, ((rows % (n // 2)) != 0) + 1
    if kind == "dct2":
        return 4 * n, (cols * (2 * rows + 1)) % (4 * n), None
    if kind == "dct3":
        return 4 * n, (rows * (2 * cols + 1)) % (4 * n), (rows != 0) + 1
    if kind == "dct4":
        return 8 * n, ((2 * rows + 1) * (2 * cols + 1)) % (8 * n), None
    raise ValueError(kind)


def basis_width(n, kind):
    return int(np.prod(n)) if kind == "c2c" else int(n) // 2 + 1 if kind == "r2c" else int(n)


def basis_reference(rows, n, kind, direction=FORWARD, route=None):
    """the reference rows themselves (numpy, in the route's type): complex [len(rows), width] for c2c / r2c, real else"""
    rows = np.asarray(rows, dtype=np.int64).reshape(-1, 1)
    cols = np.arange(basis_width(n, kind), dtype=np.int64).reshape(1, -1)
    big, idx, weight = basis_phase(rows, cols, n, kind)
    c, s = basis_circle(big, route)
    if kind in ("c2c", "r2c"):
        return c[idx] + 1j * (-s[idx] if direction == FORWARD else s[idx])
    return 2 * c[idx] if weight is None else c[idx] * weight.astype(c.dtype)


def check_basis_rows(got, rows, n, kind, prec, scale=1.0, what="", direction=FORWARD, route=None, chunk=1 << 22):
    """The transforms of unit impulses against the matrix rows, element by element, with the derived bound.

    got: [len(rows), width] (torch tensor on any device, or numpy): row i is the transform of e_rows[i] (c2c: rows are flat
    indices of the shape n, width prod(n), complex; r2c: N/2 + 1 complex bins; c2r: the N reals of the unit bin rows[i];
    dct2 / dct3 / dct4: N reals).  prec: the plan's ("f16": got holds the binary16 values in a wider type).  Every element
    must satisfy |got - scale ref| <= basis_bound(n, kind, prec, scale); with fp16 storage, per component, that plus half a
    binary16 ulp of the reference component.  A failure names the row, the element and the ratio to the bound; the worst
    ratio is returned.

    The reference is a gather from basis_circle at exactly reduced integer phases, so its error is the table's.  On
    got's device in fp64 (torch) the table is the long double one rounded to fp64 (error <= 2^-53 of the amplitude) or
    the octant-reduced fp64 one (<= 2^-52); where that exceeds bound / 16 -- fp64 plans with fewer than 5 (10)
    multiplies in the bound -- the comparison runs on the host in np.longdouble instead.  route: force "longdouble" (host)
    or "float64" (torch, octant-reduced table).  Rows are taken `chunk` elements at a time: no second copy of got."""
    import torch
    assert kind in BASIS_KINDS and prec in BASIS_U
    rows = np.asarray(rows, dtype=np.int64).ravel()
    width = basis_width(n, kind)
    assert tuple(got.shape) == (rows.size, width), (what, tuple(got.shape), (rows.size, width))
    cplx = kind in ("c2c", "r2c")
    amp = basis_amplitude(kind)
    bound = basis_bound(n, kind, prec, scale)
    have_ld = np.finfo(np.longdouble).nmant >= 63
    if route is None:
        table_err = (1.0 if have_ld else 2.0) * 2.0 ** -53 * amp * abs(scale)
        route = "float64" if table_err <= bound / BASIS_REF_MARGIN or not have_ld else "longdouble"
        table_route = None
    else:
        table_route = route
    per = max(1, chunk // width)
    sign = -1.0 if direction == FORWARD else 1.0
    worst, worst_at = 0.0, None
    if route == "float64":
        g = torch.as_tensor(got)
        dev = g.device
        c, s = basis_circle(basis_table_length(n, kind), table_route)
        c = torch.from_numpy(c.astype(np.float64)).to(dev)
        s = torch.from_numpy(s.astype(np.float64)).to(dev) if cplx else None
        cols = torch.arange(width, dtype=torch.int64, device=dev).reshape(1, -1)
        rows_t = torch.from_numpy(rows).to(dev).reshape(-1, 1)
    for r0 in range(0, rows.size, per):
        r1 = min(rows.size, r0 + per)
        if route == "float64":
            _, idx, weight = basis_phase(rows_t[r0:r1], cols, n, kind)
            part = g[r0:r1]
            if cplx:
                part = part.to(torch.complex128)
                d_re = part.real - scale * c[idx]
                d_im = part.imag - (sign * scale) * s[idx]
                if prec == "f16":
                    ratio = torch.maximum(d_re.abs() / (bound + 0.5 * _ulp16(scale * c[idx], torch)),
                                          d_im.abs() / (bound + 0.5 * _ulp16(scale * s[idx], torch)))
                else:
                    ratio = torch.hypot(d_re, d_im) / bound
            else:
                ref = c[idx] * (2.0 * scale if weight is None else weight.double() * scale)
                diff = (part.double() - ref).abs()
                ratio = diff / (bound + 0.5 * _ulp16(ref, torch)) if prec == "f16" else diff / bound
            ratio = torch.where(torch.isfinite(ratio), ratio, torch.full_like(ratio, float("inf")))
            m, pos = float(ratio.max()), int(torch.argmax(ratio))
        else:
            assert prec != "f16", "fp16 storage is compared in fp64"
            part = got[r0:r1]
            part = part.cpu().numpy() if hasattr(part, "cpu") else np.asarray(part)
            ref = basis_reference(rows[r0:r1], n, kind, direction, "longdouble") * np.longdouble(scale)
            ratio = np.abs(part.astype(ref.dtype) - ref) / np.longdouble(bound)
            ratio = np.where(np.isfinite(ratio), ratio, np.inf)
            m, pos = float(ratio.max()), int(np.argmax(ratio))
        if worst_at is None or m > worst:
            worst, worst_at = m, (int(rows[r0 + pos // width]), pos % width)
        if not (m <= 1.0):
            raise AssertionError("%s: %s %s n=%s: the transform of e_%d, element %d: |got - ref| is %.3g of the bound %.3g "
                                 "(%d multiplies)" % (what, kind, prec, n, worst_at[0], worst_at[1], m, bound,
                                                      basis_multiplies(n, kind)))
    print("%s: %s %s n=%s, %d rows: worst |got - ref| / bound %.3f (row %d, element %d)" % (
        what, kind, prec, n, rows.size, worst, worst_at[0], worst_at[1]))
    return worst


# ---------------------------------------------------------------------------------------------------------------------
# odd-radix and ragged configurations of the runtime planner (choose_spec_params, jit_planner.cpp): one length M of the
# complex passes per configuration class and precision.  The fused real verbs run them at N = 2M, the complex ones at
# N = M (test_gpu_odd_radix.py); test_odd_radix_classes.py asks the host planner for every row and asserts the class's
# property, so a planner change that moves a length out of its class fails there.
#
#   work-item ...         one lane per transform (a single radix), 256 transforms per group; the LDS pitch of a transform
#                         is padded only when M is even.  The planner takes a single radix for M <= 16, the composites 18,
#                         20, 21, 22 (fp32; fp64: 18) and every prime up to 61 -- 25 and 27 are two passes
#   all radices odd       odd M, three odd radices, a ragged pass (fewer butterflies than lanes), no "+1 per 16" padding
#   odd prime power       every radix a power of one odd prime
#   odd first radix       even M whose first radix is odd: the padding is absent although M is even
#   composite radix       a composite radix of 17 ... 32 (fp32 only: fp64 caps composite radices at 16 unless a prime of
#                         37 ... 61 forces the rest into one radix, and that is the prime-lanes row)
#   prime lanes M/P, P    a prime P of 37 ... 61 with 16 <= M / P <= 32: radices {M / P, P}, 16 or 32 lanes
#   prime lanes P, rest   the same rule with 32 < M / P <= 64: radices {P, rest ...}; the planner's own 128 lanes stay
#                         (fp64: the lengths of this row are past the cap of a quick test and the body is the fp32 one)
#   prime lanes odd M     two primes of 37 ... 61 (M / P > 32: prime first), 64 lanes (fp32; fp64 plans 1369 the same way
#                         with one transform per group, and every verb would compile the radix-37 butterfly once more)
#   lanes no power of two more than one transform shares a work-group whose lane count per transform is no power of two
#
# The kernels of a prime radix cost their commit-time compile: measured cold for one verb on the MI355X, 1.8 s per case with
# radix 37, 7.6 s with 47 x 43 (M = 2021), 8.8 s with radix 61 in the work-item form and 10.4 s at 976 = 16 x 61.  So the
# rows of a prime take 37 (592 = 16 x 37, 2368 = 37 x 8 x 8, 1369 = 37 x 37 and 37 itself), and radix 61 runs in
# ODD_RADIX_61 for one verb of each family of real kernel bodies only -- R2C / C2R (the untangle items) and the DCT-IV
# (its own item scheme), 10.5 s and 7.2 s cold; the families left out at radix 61 are the windowed frame loads (stft,
# periodogram, mdct), the overlap-add stores (istft, imdct), the DCT-II / III, the real and complex convolutions and
# filters (a convolution commit compiles four radix-61 kernels: 45 s) and the pairs.
ODD_RADIX_LENGTHS = {
    "f32": [(7, "work-item odd prime"), (37, "work-item odd prime"), (15, "work-item odd composite"),
            (21, "work-item odd composite"), (22, "work-item even"), (1001, "all radices odd"), (243, "odd prime power"),
            (343, "odd prime power"), (150, "odd first radix"), (315, "composite radix"), (592, "prime lanes M/P, P"),
            (2368, "prime lanes P, rest"), (1369, "prime lanes odd M"), (27, "lanes no power of two")],
    "f64": [(13, "work-item odd prime"), (15, "work-item odd composite"), (18, "work-item even"), (1001, "all radices odd"),
            (243, "odd prime power"), (150, "odd first radix"), (592, "prime lanes M/P, P"), (27, "lanes no power of two")],
}
ODD_RADIX_61 = {"f32": [(976, "prime lanes M/P, P")], "f64": []}


ODD_RADIX_M = sorted({m for table in (ODD_RADIX_LENGTHS, ODD_RADIX_61) for rows in table.values() for m, _ in rows})
# N = 2M of the tables up to the longest length the CPU reference tests had before (2000; 2002 = 2 * 7 * 11 * 13 with it):
# odd M, M prime (14, 26, 74), every radix odd.  2738 and 4736 would cost an N x N long-double matrix of 0.1 - 0.3 GB each.
ODD_RADIX_REFERENCE_N = tuple(2 * m for m in ODD_RADIX_M if 2 * m <= 2002)


def _is_prime(v):
    return v > 1 and all(v % i for i in range(2, int(v ** 0.5) + 1))


def odd_radix_hop(n):
    """the hop of the stft-style verbs on the table's lengths: the first odd number from N / 4 + 1 on that is coprime to N"""
    hop = (n // 4 + 1) | 1
    while np.gcd(hop, n) != 1:
        hop += 2
    return int(hop)


def odd_radix_class_miss(cls, m, radices, lanes, fpw, pads=None):
    """None when the configuration (radices, lanes per transform, transforms per group, LDS padding period -- None: not
    known, as from plan.info()) of an M-point transform has the property its class is named for; else what is missing"""
    radices = [int(r) for r in radices]
    if int(np.prod(radices)) != m:
        return "the radices %s do not multiply to M = %d" % (radices, m)
    ragged = any(m // r < lanes for r in radices)
    power_of_two = lanes & (lanes - 1) == 0
    checks = []
    if cls.startswith("work-item"):
        checks += [("a single radix", len(radices) == 1), ("one lane per transform", lanes == 1),
                   ("128 or 256 transforms per group", fpw in (128, 256))]
        if cls == "work-item odd prime":
            checks += [("M an odd prime", m % 2 == 1 and _is_prime(m)), ("no padded pitch", pads in (None, 0))]
        elif cls == "work-item odd composite":
            checks += [("M odd and composite", m % 2 == 1 and not _is_prime(m)), ("no padded pitch", pads in (None, 0))]
        else:
            checks += [("M even", m % 2 == 0), ("the pitch padded by one element per transform", pads in (None, m))]
    elif cls == "all radices odd":
        checks += [("three passes", len(radices) == 3), ("every radix odd", all(r % 2 for r in radices)),
                   ("three different primes", len(set(radices)) == 3 and all(_is_prime(r) for r in radices)),
                   ("a ragged pass", ragged), ("no padding", pads in (None, 0))]
    elif cls == "odd prime power":
        p = min(r for r in range(3, m + 1) if m % r == 0)
        checks += [("M a power of an odd prime", _is_prime(p) and p % 2 == 1 and p ** round(np.log(m) / np.log(p)) == m),
                   ("at least two passes", len(radices) >= 2), ("no padding", pads in (None, 0)),
                   ("lanes no power of two", not power_of_two)]
    elif cls == "odd first radix":
        checks += [("M even", m % 2 == 0), ("the first radix odd", radices[0] % 2 == 1), ("at least two passes", len(radices) >= 2),
                   ("no padding", pads in (None, 0))]
    elif cls == "composite radix":
        big = max(radices)
        checks += [("the largest radix composite and in 17 ... 32", 17 <= big <= 32 and not _is_prime(big)),
                   ("at least two passes", len(radices) >= 2)]
    elif cls == "prime lanes M/P, P":
        checks += [("two passes", len(radices) == 2), ("the prime of 37 ... 61 last", _is_prime(radices[-1]) and 37 <= radices[-1] <= 61),
                   ("M / P in 16 ... 32 first", 16 <= radices[0] <= 32),
                   ("lanes M / P rounded up to 16 or 32", lanes in (16, 32) and lanes // 2 < radices[0] <= lanes)]
    elif cls == "prime lanes P, rest":
        checks += [("the prime of 37 ... 61 first", _is_prime(radices[0]) and 37 <= radices[0] <= 61),
                   ("the rest behind it, 32 < M / P <= 64", len(radices) >= 3 and 32 < m // radices[0] <= 64),
                   ("64 or 128 lanes", lanes in (64, 128))]
    elif cls == "prime lanes odd M":
        checks += [("M odd", m % 2 == 1), ("two primes of 37 ... 61", len(radices) == 2 and all(_is_prime(r) and 37 <= r <= 61 for r in radices)),
                   ("64 lanes", lanes == 64), ("a ragged pass", ragged)]
    elif cls == "lanes no power of two":
        checks += [("lanes no power of two", not power_of_two), ("more than one transform per group", fpw > 1),
                   ("at least two passes", len(radices) >= 2)]
    else:
        return "unknown class %r" % (cls,)
    missing = [name for name, ok in checks if not ok]
    return None if not missing else "%s: M = %d planned as radices %s, %d lanes, %d per group, padding %s: not %s" % (
        cls, m, radices, lanes, fpw, pads, "; not ".join(missing))
