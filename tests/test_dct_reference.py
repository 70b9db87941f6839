"""The reference the DCT tests compare against, and a NumPy model of the fused kernels' index maps, without a GPU.

The reference (dct_ref.py, shared with test_gpu_dct.py) is NumPy's FFT in double:
  type 2:  2 * Re(exp(-i pi k / 2N) * fft(x, 2N)[:N])
  type 3:  Re(2N * ifft(pad(a * x * exp(+i pi k / 2N), 2N))[:N]),  a_0 = 1, a_k = 2
It is held against the cosine matrix with EXACTLY reduced arguments -- (k (2n + 1)) mod 4N in integers, the cosine in
np.longdouble -- to a relative L2 of 1e-15 per row (measured: at most 3.3e-16; a matrix of np.cos(pi k (2n+1) / (2N)) in
double is 1.7e-13 off at N = 2000 and is no yardstick), and against scipy.fft.dct where scipy imports.

The model (model_dct2 / model_dct3) walks the steps of stockham_wg_dct.hpp with explicit indices: the scatter of the
aligned pairs into the scalar slots of the image, z and Z = DFT_M(z), the R2C untangle step with the four-output
twiddle step and its two special items, and for type 3 the pre-step, the C2R untangle-in formulas, the conjugate-in
backward transform and the copy-out with its sign by parity.  M odd and even; the same 1e-15."""
import numpy as np
import pytest

import helpers as H
from dct_ref import dct_reference

# (and N = 2M of the odd-radix table, helpers.ODD_RADIX_REFERENCE_N: odd M, M prime -- test_dct4_reference.py and
#  test_imdct_reference.py take the list from here)
LENGTHS = (4, 6, 8, 30, 64, 256, 512, 2000) + tuple(n for n in H.ODD_RADIX_REFERENCE_N if n != 30)
TOL = 1e-15


def exact_matrix(n, kind):
    """C[k][j] = cos(pi k (2j + 1) / (2N)) with the argument reduced mod 4N in integers, in long double; type 2 is
    2 C x, type 3 is C^T (a x)"""
    k = np.arange(n).reshape(-1, 1)
    j = np.arange(n).reshape(1, -1)
    r = (k * (2 * j + 1)) % (4 * n)
    pi = np.arccos(np.longdouble(-1))
    c = np.cos(pi * r.astype(np.longdouble) / np.longdouble(2 * n))
    if kind == 2:
        return 2 * c
    a = np.where(np.arange(n) == 0, 1, 2).astype(np.longdouble)
    return c.T * a.reshape(1, -1)


def rel_l2(got, want):
    got = np.asarray(got, dtype=np.longdouble)
    want = np.asarray(want, dtype=np.longdouble)
    return float(np.sqrt(np.sum((got - want) ** 2) / np.sum(want ** 2)))


def _rows(n, seed):
    rng = np.random.default_rng(seed)
    rows = [rng.uniform(-1, 1, n), np.full(n, 0.75)]
    for p in (0, 1, n // 2 - 1, n // 2, n - 2, n - 1):
        e = np.zeros(n)
        e[p] = 1.0
        rows.append(e)
    return np.stack(rows)


@pytest.mark.parametrize("kind", (2, 3))
@pytest.mark.parametrize("n", LENGTHS)
def test_reference_against_the_exact_matrix(n, kind):
    x = _rows(n, 100 * n + kind)
    want = (exact_matrix(n, kind) @ x.astype(np.longdouble).T).T
    got = dct_reference(x, kind)
    worst = max(rel_l2(got[i], want[i]) for i in range(x.shape[0]))
    print("N=%d type %d reference vs exact matrix: %.2e" % (n, kind, worst))
    assert worst <= TOL


@pytest.mark.parametrize("kind", (2, 3))
@pytest.mark.parametrize("n", LENGTHS)
def test_reference_against_scipy(n, kind):
    sfft = pytest.importorskip("scipy.fft")
    x = _rows(n, 7 * n + kind)
    want = sfft.dct(x, type=kind, norm=None, axis=-1)
    got = dct_reference(x, kind)
    assert max(rel_l2(got[i], want[i]) for i in range(x.shape[0])) <= TOL


def test_round_trip_is_2n():
    x = _rows(30, 5)
    assert np.allclose(dct_reference(dct_reference(x, 2), 3), 2 * 30 * x, rtol=0, atol=1e-12)


# ---- the kernels' index maps ------------------------------------------------------------------------------------------


def _tables(n):
    m = n // 2
    wk = np.exp(-2j * np.pi * np.arange(m // 2 + 1) / n)  # the real plan's untangle twiddles, k = 0 ... M/2
    ck = np.exp(-1j * np.pi * np.arange(m + 1) / (2 * n))  # the quarter-wave table c_0 ... c_M
    return m, wk, ck


def model_dct2(x):
    """one row through the type-2 kernel: copy-in scatter, M-point forward transform, untangle + four outputs per item"""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[0]
    m, wk, ck = _tables(n)
    image = np.zeros(n)  # scalar slot s is .re (s even) or .im (s odd) of complex slot s / 2
    for p in range(m):  # pair p = (x[2p], x[2p + 1]), loaded as one aligned element
        image[p] = x[2 * p]
        image[n - 1 - p] = x[2 * p + 1]
    z = image[0::2] + 1j * image[1::2]
    zz = np.fft.fft(z)
    y = np.full(n, np.nan)
    for k in range(m // 2 + 1):
        a = zz[k]
        if k == 0:
            y[0] = 2.0 * (a.real + a.imag)
            y[m] = np.sqrt(2.0) * (a.real - a.imag)
            continue
        b = np.conj(zz[m - k])
        s, d = a + b, a - b
        t = d * wk[k]
        vk = 0.5 * complex(s.real + t.imag, s.imag - t.real)  # V[k]
        vmk = 0.5 * complex(s.real - t.imag, -(s.imag + t.real))  # V[M - k]
        u = ck[k] * vk
        y[k] = 2.0 * u.real
        y[n - k] = -2.0 * u.imag
        if 2 * k != m:
            u = ck[m - k] * vmk
            y[m - k] = 2.0 * u.real
            y[m + k] = -2.0 * u.imag
    return y


def model_dct3(x):
    """one row through the type-3 kernel: pre-step, C2R untangle-in, conjugate-in backward transform, copy-out"""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[0]
    m, wk, ck = _tables(n)
    img = np.full(m, np.nan + 0j)  # conj(Z'), what the backward passes read
    for k in range(m // 2 + 1):
        if k == 0:
            bx, by = complex(x[0], 0.0), complex(np.sqrt(2.0) * x[m], 0.0)  # V'[0], V'[M]: exactly real
        else:
            bx = np.conj(ck[k]) * complex(x[k], -x[n - k])  # V'[k]
            by = np.conj(ck[m - k]) * complex(x[m - k], -x[m + k])  # V'[M - k]
        s = complex(bx.real + by.real, bx.imag - by.imag)
        d = complex(bx.real - by.real, bx.imag + by.imag)
        q = np.conj(wk[k]) * d
        img[k] = complex(s.real - q.imag, -(s.imag + q.real))
        if k != 0 and 2 * k != m:
            img[m - k] = complex(s.real + q.imag, s.imag - q.real)
    out = np.fft.fft(img)  # the forward passes on conj(Z') leave conj(z') in the image
    v = np.empty(n)  # scalar slot s of the image, with the sign the C2R copy-out applies: v[2j] = re, v[2j + 1] = -im
    v[0::2] = out.real
    v[1::2] = -out.imag
    y = np.empty(n)
    for p in range(m):  # output pair p = (v[p], v[N - 1 - p])
        y[2 * p] = v[p]
        y[2 * p + 1] = v[n - 1 - p]
    return y


@pytest.mark.parametrize("kind", (2, 3))
@pytest.mark.parametrize("n", LENGTHS + tuple(n for n in (10, 12, 14) if n not in LENGTHS))
def test_kernel_index_maps(n, kind):
    x = _rows(n, 31 * n + kind)
    model = model_dct2 if kind == 2 else model_dct3
    want = dct_reference(x, kind)
    got = np.stack([model(r) for r in x])
    assert not np.isnan(got).any()  # every output written, every image slot filled
    worst = max(rel_l2(got[i], want[i]) for i in range(x.shape[0]))
    print("N=%d type %d model vs reference: %.2e" % (n, kind, worst))
    assert worst <= TOL
