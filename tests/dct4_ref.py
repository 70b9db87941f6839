"""The references of the DCT-IV / MDCT tests, from NumPy's FFT alone, in double (scipy is not needed where the GPU tests
run).  Both read the odd bins of one zero-stuffed transform of 8N points, so neither knows the fold identity or the
twiddle factorisation the kernel uses.  test_dct4_reference.py holds them against the cosine matrices with exactly
reduced arguments to 1e-15."""
import numpy as np


def dct4_reference(x):
    """scipy.fft.dct(x, 4, norm=None): y[k] = 2 sum_n x[n] cos(pi (2n + 1)(2k + 1) / (4N)) = 2 Re(fft(u, 8N)[2k + 1]) with
    u[2n + 1] = x[n]                                                                              (rows: the last axis)"""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[-1]
    u = np.zeros(x.shape[:-1] + (8 * n,))
    u[..., 1:2 * n:2] = x
    return 2.0 * np.real(np.fft.fft(u, axis=-1)[..., 1:2 * n:2])


def mdct_reference(v):
    """MDCT of already windowed frames v of 2N samples: X[k] = 2 sum_n v[n] cos(pi (2n + 1 + N)(2k + 1) / (4N)) =
    2 Re(fft(u, 8N)[2k + 1]) with u[2n + 1 + N] = v[n]                                            (frames: the last axis)"""
    v = np.asarray(v, dtype=np.float64)
    n = v.shape[-1] // 2
    assert v.shape[-1] == 2 * n
    u = np.zeros(v.shape[:-1] + (8 * n,))
    u[..., n + 1:5 * n:2] = v
    return 2.0 * np.real(np.fft.fft(u, axis=-1)[..., 1:2 * n:2])


def frames_of(x, n, lead, n_frames, window=None):
    """the windowed frames an MDCT of hop N reads: (..., n_frames, 2N) from signals x (..., L) extended by zeros"""
    x = np.asarray(x, dtype=np.float64)
    length = x.shape[-1]
    xe = np.zeros(x.shape[:-1] + (lead + length + (n_frames + 2) * n,))
    xe[..., lead:lead + length] = x
    fr = np.stack([xe[..., f * n:f * n + 2 * n] for f in range(n_frames)], axis=-2)
    return fr if window is None else fr * np.asarray(window, dtype=np.float64)


def tdac_unfold(y):
    """rows y = [p, q] of N DCT-IV outputs of MDCT coefficients -> the 2N time-aliased samples [q, -rev(q), -rev(p), -p]"""
    n = y.shape[-1]
    p, q = y[..., :n // 2], y[..., n // 2:]
    return np.concatenate([q, -q[..., ::-1], -p[..., ::-1], -p], axis=-1)


def overlap_add(frames, n, lead, length):
    """sum of frames (..., F, 2N) at hop N, frame f starting at sample f * N - lead; the first `length` samples"""
    n_frames = frames.shape[-2]
    acc = np.zeros(frames.shape[:-2] + (lead + length + (n_frames + 2) * n,))
    for f in range(n_frames):
        acc[..., f * n:f * n + 2 * n] += frames[..., f, :]
    return acc[..., lead:lead + length]
