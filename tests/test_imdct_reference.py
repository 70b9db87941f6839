"""The reference the inverse MDCT tests compare against, and a NumPy model of the fused kernel's steps, without a GPU.

The reference (imdct_ref.py, shared with test_gpu_imdct.py) reads the bins 2n + 1 + N of a zero-stuffed NumPy FFT of 8N
points in double and adds the frames in ascending f.  It is held against the cosine matrix with EXACTLY reduced arguments
-- ((2k + 1)(2n + 1 + N)) mod 8N in integers, the cosine in np.longdouble -- to a relative L2 of 1e-15 per frame, and
against overlap_add(tdac_unfold(dct4_reference(.)) * w) of dct4_ref.py.

The model (model_imdct) walks stockham_wg_imdct.hpp with explicit indices: a group owns (chunk c) of a signal and runs the
frames max(0, c C - 1) ... end of chunk, FPW per step; the items of a frame fill its image t, T = DFT_M(t), the items turn
slot k into u[k] = T[k] b_k = (Y[2k], -Y[N - 1 - 2k]) / 2 in place; every entry (block, j < M) of the step takes `cur` from
its block's image and `prev` from the image in front -- block 0 of a step from the carry of M halved values, or +0 in the
first step of a run -- and stores the positions j and N - 1 - j of the block, which share the two values, each when its
index relative to the chunk's first owned sample is below n_own.  Images, carry and
output start as NaN and every store is counted: a slot nobody fills, a sample nobody writes or one written twice shows.
The outputs of chunk = 1, 3 and F are IDENTICAL, bit for bit, and equal the reference to 1e-15-style bounds, for even and
odd M.

The round trip: sine window, lead = N, ceil(L / N) + 1 frames, scale 1 / (2N) reproduces x."""
import numpy as np
import pytest

from dct4_ref import dct4_reference, frames_of, mdct_reference, overlap_add, tdac_unfold
from imdct_ref import imdct_frames, imdct_reference
from test_dct_reference import LENGTHS, TOL, rel_l2

MODEL_LENGTHS = (4, 6, 30, 64) + tuple(n for n in LENGTHS if n not in (4, 6, 30, 64) and n <= 128 and n % 4 == 2)  # (odd M)


def exact_imdct_matrix(n):
    """2 cos(pi (2j + 1 + N)(2k + 1) / (4N)), j < 2N rows, k < N columns, the argument reduced mod 8N in integers"""
    j = np.arange(2 * n).reshape(-1, 1)
    k = np.arange(n).reshape(1, -1)
    r = ((2 * k + 1) * (2 * j + 1 + n)) % (8 * n)
    pi = np.arccos(np.longdouble(-1))
    return 2 * np.cos(pi * r.astype(np.longdouble) / np.longdouble(4 * n))


def _coeff(n, n_frames, seed):
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1, 1, (n_frames, n))
    x[0] = 0.0
    x[0, n - 1] = 1.0  # a unit row
    return x


@pytest.mark.parametrize("n", LENGTHS)
def test_unfolded_frames_against_the_exact_matrix(n):
    x = _coeff(n, 6, 100 * n + 6)
    want = (exact_imdct_matrix(n) @ x.astype(np.longdouble).T).T
    got = imdct_frames(x)
    worst = max(rel_l2(got[i], want[i]) for i in range(x.shape[0]))
    print("N=%d unfolded frame vs exact matrix: %.2e" % (n, worst))
    assert worst <= TOL


@pytest.mark.parametrize("n", LENGTHS)
@pytest.mark.parametrize("lead_of", (lambda n: 0, lambda n: 1, lambda n: n, lambda n: 2 * n - 1))
def test_reference_against_the_unfold_of_dct4(n, lead_of):
    lead = lead_of(n)
    n_frames = 5
    x = _coeff(n, n_frames, 31 * n + lead)
    w = np.random.default_rng(n).uniform(0.25, 1.0, 2 * n)
    length = (n_frames + 1) * n - lead
    want = overlap_add(tdac_unfold(dct4_reference(x)) * w, n, lead, length)
    got = imdct_reference(x, w, n, lead, length)
    # (both sides are sums of two products of O(N) terms: an absolute bound against the largest sample)
    err = float(np.max(np.abs(got - want)) / np.max(np.abs(want)))
    print("N=%d lead=%d reference vs unfold of dct4: %.2e" % (n, lead, err))
    assert err <= 1e-13


def _tables(n):
    m = n // 2
    pi = np.arccos(np.longdouble(-1))
    a = np.exp(-1j * (pi * (4 * np.arange(m) + 1) / (4 * n)).astype(np.float64))
    b = np.exp(-1j * (pi * np.arange(m) / n).astype(np.float64))
    return a, b


def _half(img, m_idx, n):
    """Y[m] / 2 of an image whose slot k holds (Y[2k], -Y[N - 1 - 2k]) / 2"""
    return -img[(n - 1 - m_idx) >> 1].imag if m_idx & 1 else img[m_idx >> 1].real


def model_imdct(coeff, w, n, lead, out_length, chunk, fpw, scale):
    """one signal through stockham_wg_imdct_kernel: coeff (F, N) -> out_length samples; returns (samples, stores per sample)"""
    m = n // 2
    n_frames = coeff.shape[0]
    a, b = _tables(n)
    out = np.full(out_length, np.nan)
    stores = np.zeros(out_length, dtype=int)
    s2 = 2.0 * scale
    n_chunks = -(-n_frames // chunk)
    for c in range(n_chunks):
        cf0 = c * chunk
        last_chunk = c == n_chunks - 1
        fe = n_frames if last_chunk else cf0 + chunk
        fs = cf0 - 1 if cf0 > 0 else 0
        lo = max(0, cf0 * n - lead)
        hi = out_length if last_chunk else fe * n - lead
        hi = max(lo, min(hi, out_length))
        n_own = hi - lo
        carry = np.full(m, np.nan)
        for f0 in range(fs, fe, fpw):
            live = min(fpw, fe - f0)
            imgs = np.full((fpw, m), np.nan + 0j)
            for r in range(live):  # items in, passes, items out
                x = coeff[f0 + r]
                img = np.full(m, np.nan + 0j)
                for j in range((m + 1) // 2):
                    pa = (x[2 * j], x[2 * j + 1])
                    pb = (x[2 * (m - 1 - j)], x[2 * (m - 1 - j) + 1])
                    img[j] = (pa[0] + 1j * pb[1]) * a[j]
                    if 2 * j + 1 != m:
                        img[m - 1 - j] = (pb[0] + 1j * pa[1]) * a[m - 1 - j]
                assert not np.isnan(img).any(), "a slot nobody filled"
                big_t = np.fft.fft(img)
                for k in range((m + 1) // 2):
                    u, v = big_t[k] * b[k], big_t[m - 1 - k] * b[m - 1 - k]
                    big_t[k] = u
                    if 2 * k + 1 != m:
                        big_t[m - 1 - k] = v
                imgs[r] = big_t
            all_out = last_chunk and f0 + live == fe
            ents = (live + 1 if all_out else live) * m
            carried = f0 != fs
            rel0 = f0 * n - lead - lo  # (negative: in front of the chunk; the kernel's unsigned index is then beyond n_own)
            for e in range(ents):  # entry e: the positions j and N - 1 - j of block blk share their two values
                blk, j = divmod(e, m)
                ra, rb = rel0 + blk * n + j, rel0 + blk * n + (n - 1 - j)
                if not (0 <= ra < n_own or 0 <= rb < n_own):
                    continue
                yp = yc = w0 = w1 = w2 = w3 = 0.0
                if blk > 0 or carried:
                    yp = _half(imgs[blk - 1], m - 1 - j, n) if blk > 0 else carry[m - 1 - j]
                    w2, w3 = w[n + j], w[2 * n - 1 - j]
                if blk < live:
                    yc = _half(imgs[blk], m + j, n)
                    w0, w1 = w[j], w[n - 1 - j]
                if 0 <= ra < n_own:
                    out[lo + ra] = s2 * (w0 * yc - w2 * yp)
                    stores[lo + ra] += 1
                if 0 <= rb < n_own:
                    out[lo + rb] = s2 * (w1 * -yc - w3 * yp)
                    stores[lo + rb] += 1
            if f0 + fpw < fe:
                carry = np.array([_half(imgs[fpw - 1], i, n) for i in range(m)])
    return out, stores


@pytest.mark.parametrize("n", MODEL_LENGTHS)
@pytest.mark.parametrize("fpw", (1, 2, 4))
def test_the_steps_of_the_kernel(n, fpw):
    n_frames = 2 * 4 + 1  # a ragged last step at every fpw
    x = _coeff(n, n_frames, 77 * n + fpw)
    w = np.random.default_rng(5 * n).uniform(0.25, 1.0, 2 * n)  # not symmetric
    scale = 1.0 / (2 * n)
    worst = 0.0
    for lead in (0, 1, n - 2, n, 2 * n - 1):
        full = (n_frames + 1) * n - lead
        for length in (full, full - n - n // 2 - 1):
            want = scale * imdct_reference(x, w, n, lead, length)
            first = None
            for chunk in (1, 3, n_frames):
                got, stores = model_imdct(x, w, n, lead, length, chunk, fpw, scale)
                assert (stores == 1).all(), "every sample is stored exactly once (chunk %d)" % chunk
                assert not np.isnan(got).any(), "a value that came from an unfilled slot or carry (chunk %d)" % chunk
                if first is None:
                    first = got
                assert np.array_equal(got, first), "the result depends on chunk_frames (chunk %d)" % chunk
            # (a sample is the sum of two products of sums of N terms: bound against the largest sample, as above)
            worst = max(worst, float(np.max(np.abs(first - want)) / np.max(np.abs(want))))
    print("N=%d FPW=%d kernel steps vs reference: %.2e" % (n, fpw, worst))
    assert worst <= 1e-13


@pytest.mark.parametrize("n", LENGTHS)
def test_round_trip_through_the_mdct_reference(n):
    rng = np.random.default_rng(29 * n)
    length = 5 * n + 3
    x = rng.uniform(-1, 1, (2, length))
    w = np.sin(np.pi * (np.arange(2 * n) + 0.5) / (2 * n))
    n_frames = -(-length // n) + 1
    coeff = mdct_reference(frames_of(x, n, n, n_frames, w))
    back = imdct_reference(coeff, w, n, n, length) / (2 * n)
    err = rel_l2(back, x)
    print("N=%d imdct(mdct(x)) vs x: %.2e" % (n, err))
    assert err <= 1e-12
