"""The reference of the DCT tests: scipy.fft.dct(x, type, norm=None) from NumPy's FFT alone, in double (scipy is not
needed where the GPU tests run).  test_dct_reference.py holds it against the cosine matrix with exactly reduced arguments
to 1e-15; a matrix of np.cos(pi k (2n + 1) / (2N)) in double is 1.7e-13 off at N = 2000 and is no yardstick."""
import numpy as np


def dct_reference(x, kind):
    """type 2:  2 * Re(exp(-i pi k / 2N) * fft(x, 2N)[:N])
    type 3:  Re(2N * ifft(pad(a * x * exp(+i pi k / 2N), 2N))[:N]),  a_0 = 1, a_k = 2       (rows: the last axis)"""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[-1]
    k = np.arange(n)
    if kind == 2:
        return 2.0 * np.real(np.exp(-1j * np.pi * k / (2 * n)) * np.fft.fft(x, 2 * n, axis=-1)[..., :n])
    if kind == 3:
        a = np.where(k == 0, 1.0, 2.0)
        spec = np.zeros(x.shape[:-1] + (2 * n,), dtype=np.complex128)
        spec[..., :n] = a * x * np.exp(1j * np.pi * k / (2 * n))
        return np.real(2 * n * np.fft.ifft(spec, axis=-1)[..., :n])
    raise ValueError(kind)
