"""The references the DCT-IV / MDCT tests compare against, and a NumPy model of the fused kernel's item scheme, without a GPU.

The references (dct4_ref.py, shared with test_gpu_dct4.py) read the odd bins of a zero-stuffed NumPy FFT of 8N points in
double.  They are held against the cosine matrices with EXACTLY reduced arguments -- ((2k + 1)(2n + 1)) mod 8N for the
DCT-IV and ((2k + 1)(2n + 1 + N)) mod 8N for the MDCT, in integers, the cosine in np.longdouble -- to a relative L2 of
1e-15 per row (measured: at most 3.7e-16 for both), and against scipy.fft.dct(type=4) where scipy imports.

The model (model_dct4 / model_mdct) walks the items of stockham_wg_dct4.hpp with explicit indices: item j owns the input
pairs j and M - 1 - j, forms t0[j] and t0[M - 1 - j] from them, multiplies by a_j and a_{M-1-j}, T = DFT_M(t), the same item
multiplies T[k], T[M - 1 - k] by b_k, b_{M-1-k} and writes the output pairs k and M - 1 - k; for the MDCT the two pairs come
from four frame pairs (the middle item of an odd M: four scalars) under a per-scalar predicate.  Images and outputs start
as NaN, so a slot nobody fills or an output nobody writes shows.  M odd and even; the same 1e-15.

The reconstruction (time-domain alias cancellation): sine window, lead = N, ceil(L / N) + 1 frames, DCT-IV of the MDCT
rows, unfold, window, overlap-add gives 2N x."""
import numpy as np
import pytest

from dct4_ref import dct4_reference, frames_of, mdct_reference, overlap_add, tdac_unfold
from test_dct_reference import LENGTHS, TOL, _rows, rel_l2

MODEL_LENGTHS = (4, 6, 8, 10, 12, 14, 30, 64, 256, 512, 2000) + tuple(n for n in LENGTHS if n not in (4, 6, 8, 14, 30, 64, 256, 512, 2000))


def exact_dct4_matrix(n):
    """2 cos(pi (2k + 1)(2j + 1) / (4N)) with the argument reduced mod 8N in integers, in long double"""
    k = np.arange(n).reshape(-1, 1)
    j = np.arange(n).reshape(1, -1)
    r = ((2 * k + 1) * (2 * j + 1)) % (8 * n)
    pi = np.arccos(np.longdouble(-1))
    return 2 * np.cos(pi * r.astype(np.longdouble) / np.longdouble(4 * n))


def exact_mdct_matrix(n):
    """2 cos(pi (2j + 1 + N)(2k + 1) / (4N)), k < N, j < 2N, reduced the same way"""
    k = np.arange(n).reshape(-1, 1)
    j = np.arange(2 * n).reshape(1, -1)
    r = ((2 * k + 1) * (2 * j + 1 + n)) % (8 * n)
    pi = np.arccos(np.longdouble(-1))
    return 2 * np.cos(pi * r.astype(np.longdouble) / np.longdouble(4 * n))


@pytest.mark.parametrize("n", LENGTHS)
def test_dct4_reference_against_the_exact_matrix(n):
    x = _rows(n, 100 * n + 4)
    want = (exact_dct4_matrix(n) @ x.astype(np.longdouble).T).T
    got = dct4_reference(x)
    worst = max(rel_l2(got[i], want[i]) for i in range(x.shape[0]))
    print("N=%d DCT-IV reference vs exact matrix: %.2e" % (n, worst))
    assert worst <= TOL


@pytest.mark.parametrize("n", LENGTHS)
def test_mdct_reference_against_the_exact_matrix(n):
    v = _rows(2 * n, 100 * n + 5)
    want = (exact_mdct_matrix(n) @ v.astype(np.longdouble).T).T
    got = mdct_reference(v)
    worst = max(rel_l2(got[i], want[i]) for i in range(v.shape[0]))
    print("N=%d MDCT reference vs exact matrix: %.2e" % (n, worst))
    assert worst <= TOL


@pytest.mark.parametrize("n", LENGTHS)
def test_dct4_reference_against_scipy(n):
    sfft = pytest.importorskip("scipy.fft")
    x = _rows(n, 7 * n + 4)
    want = sfft.dct(x, type=4, norm=None, axis=-1)
    got = dct4_reference(x)
    worst = max(rel_l2(got[i], want[i]) for i in range(x.shape[0]))
    print("N=%d DCT-IV reference vs scipy: %.2e" % (n, worst))
    assert worst <= 1e-14  # (scipy's own error is in this figure)


def _tables(n):
    m = n // 2
    pi = np.arccos(np.longdouble(-1))
    a = np.exp(-1j * (pi * (4 * np.arange(m) + 1) / (4 * n)).astype(np.float64))
    b = np.exp(-1j * (pi * np.arange(m) / n).astype(np.float64))
    return a, b


def _items_out(big_t, b, n):
    m = n // 2
    y = np.full(n, np.nan)
    for k in range((m + 1) // 2):
        u = big_t[k] * b[k]
        v = big_t[m - 1 - k] * b[m - 1 - k]
        y[2 * k], y[2 * k + 1] = 2 * u.real, -2 * v.imag                        # output pair k
        if 2 * k + 1 != m:
            y[2 * (m - 1 - k)], y[2 * (m - 1 - k) + 1] = 2 * v.real, -2 * u.imag  # output pair M - 1 - k
    return y


def model_dct4(x):
    """one row through the items of stockham_wg_dct4_kernel<Cfg, false>"""
    n = x.shape[0]
    m = n // 2
    a, b = _tables(n)
    img = np.full(m, np.nan + 0j)
    for j in range((m + 1) // 2):
        pa = (x[2 * j], x[2 * j + 1])                          # input pair j
        pb = (x[2 * (m - 1 - j)], x[2 * (m - 1 - j) + 1])      # input pair M - 1 - j
        img[j] = (pa[0] + 1j * pb[1]) * a[j]
        if 2 * j + 1 != m:
            img[m - 1 - j] = (pb[0] + 1j * pa[1]) * a[m - 1 - j]
    assert not np.isnan(img).any()
    return _items_out(np.fft.fft(img), b, n)


def model_mdct(signal, w, n, lead, f):
    """frame f of one signal through the items of stockham_wg_dct4_kernel<Cfg, true>"""
    m = n // 2
    length = signal.shape[0]
    a, b = _tables(n)

    def scalar(i):  # v[i], the sample predicated on its own index
        assert 0 <= i < 2 * n
        q = f * n + i
        return (signal[q - lead] if lead <= q < lead + length else 0.0) * w[i]

    def pair(i):
        return scalar(i), scalar(i + 1)

    img = np.full(m, np.nan + 0j)
    for j in range((m + 1) // 2):
        if m % 2 == 1 and 2 * j + 1 == m:
            img[j] = ((-scalar(n) - scalar(2 * n - 1)) + 1j * (scalar(0) - scalar(n - 1))) * a[j]
            continue
        c1, c2 = pair(3 * m - 2 - 2 * j), pair(3 * m + 2 * j)
        c3, c4 = pair(m - 2 - 2 * j), pair(m + 2 * j)
        img[j] = ((-c1[1] - c2[0]) + 1j * (c3[1] - c4[0])) * a[j]
        img[m - 1 - j] = ((c3[0] - c4[1]) + 1j * (-c1[0] - c2[1])) * a[m - 1 - j]
    assert not np.isnan(img).any()
    return _items_out(np.fft.fft(img), b, n)


@pytest.mark.parametrize("n", MODEL_LENGTHS)
def test_the_item_scheme_of_the_rows_kernel(n):
    x = _rows(n, 13 * n + 4)
    want = dct4_reference(x)
    worst = 0.0
    for i in range(x.shape[0]):
        got = model_dct4(x[i])
        assert not np.isnan(got).any(), "an output nobody wrote"
        worst = max(worst, rel_l2(got, want[i]))
    print("N=%d DCT-IV item scheme vs reference: %.2e" % (n, worst))
    assert worst <= TOL


@pytest.mark.parametrize("n", MODEL_LENGTHS)
def test_the_item_scheme_of_the_mdct_kernel(n):
    rng = np.random.default_rng(17 * n)
    length = 3 * n + n // 2 + 1  # no multiple of N
    x = rng.uniform(-1, 1, length)
    w = rng.uniform(0.25, 1.0, 2 * n)  # not symmetric
    worst = 0.0
    for lead in (0, 1, n, 2 * n - 1):
        n_frames = (length + lead - 1) // n + 1  # the last frame holds at least one sample, the first is cut at lead > 0
        want = mdct_reference(frames_of(x, n, lead, n_frames, w))
        for f in range(n_frames):
            got = model_mdct(x, w, n, lead, f)
            assert not np.isnan(got).any(), "an output nobody wrote"
            worst = max(worst, rel_l2(got, want[f]))
    print("N=%d MDCT item scheme vs reference: %.2e" % (n, worst))
    assert worst <= TOL


@pytest.mark.parametrize("n", MODEL_LENGTHS)
def test_a_rotated_post_twiddle_is_far_off_the_reference(n):
    """why no test may rest on the round trip alone: with a_k behind the transform instead of b_k every output is rotated
    by pi / (4N) -- far off the reference"""
    x = _rows(n, 19 * n)[0]
    m = n // 2
    a, _ = _tables(n)
    img = np.array([(x[2 * j] + 1j * x[n - 1 - 2 * j]) * a[j] for j in range(m)])
    wrong = _items_out(np.fft.fft(img), a, n)
    assert rel_l2(wrong, dct4_reference(x)) > 1e-4 / n


@pytest.mark.parametrize("n", LENGTHS)
def test_time_domain_alias_cancellation(n):
    rng = np.random.default_rng(23 * n)
    length = 5 * n + 3
    x = rng.uniform(-1, 1, (2, length))
    w = np.sin(np.pi * (np.arange(2 * n) + 0.5) / (2 * n))
    n_frames = -(-length // n) + 1
    coeff = mdct_reference(frames_of(x, n, n, n_frames, w))
    back = overlap_add(tdac_unfold(dct4_reference(coeff)) * w, n, n, length)
    err = rel_l2(back, 2 * n * x)
    print("N=%d TDAC reconstruction: %.2e" % (n, err))
    assert err <= 1e-14  # (three transforms deep; measured 3.4e-16 at the issue's lengths)
