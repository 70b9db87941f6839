"""The reference of the inverse MDCT tests, from NumPy's FFT alone, in double (scipy is not needed where the GPU tests run).
The unfolded frame g[n] = 2 sum_k X[k] cos(pi (2n + 1 + N)(2k + 1) / (4N)), n < 2N, is read at the bins 2n + 1 + N of one
zero-stuffed transform of 8N points: it knows neither the unfold [q, -rev q, -rev p, -p] nor the twiddle factorisation
the kernel uses.  The frames are added by an explicit loop in ascending f.  test_imdct_reference.py holds it against the
cosine matrix with exactly reduced arguments."""
import numpy as np


def imdct_frames(coeff):
    """rows of N coefficients -> the 2N scalars g[n] = 2 Re(fft(u, 8N)[2n + 1 + N]) with u[2k + 1] = X[k]  (the last axis)"""
    coeff = np.asarray(coeff, dtype=np.float64)
    n = coeff.shape[-1]
    u = np.zeros(coeff.shape[:-1] + (8 * n,))
    u[..., 1:2 * n:2] = coeff
    return 2.0 * np.real(np.fft.fft(u, axis=-1)[..., n + 1:5 * n:2])


def imdct_reference(coeff, w, n, lead, out_length):
    """coeff (..., F, N), w: 2N scalars or None (ones) -> (..., out_length): y[t] = sum_f w[u - f N] g[f][u - f N], u = t +
    lead, over the frames with 0 <= u - f N < 2N, ascending f; unscaled"""
    coeff = np.asarray(coeff, dtype=np.float64)
    assert coeff.shape[-1] == n
    n_frames = coeff.shape[-2]
    g = imdct_frames(coeff)
    if w is not None:
        g = g * np.asarray(w, dtype=np.float64)
    acc = np.zeros(coeff.shape[:-2] + (max(lead + out_length, (n_frames + 1) * n),))
    for f in range(n_frames):
        acc[..., f * n:f * n + 2 * n] += g[..., f, :]
    return acc[..., lead:lead + out_length]
