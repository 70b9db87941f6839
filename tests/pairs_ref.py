"""Reference of convolve_pairs / correlate_pairs in double precision (NumPy): the route of the definition -- extend both
rows with zeros to N, rfft, product (conjugate of the second spectrum for the correlation), optional phase transform,
irfft -- and a NumPy model of the kernel's pair step (stockham_wg_pairs.hpp), which works on the two M-point spectra of
the rows read as M complex numbers.  tests/test_pairs_reference.py holds the first against the O(N^2) sums of the
definitions and the second against the first."""
import numpy as np


def extend(x, n):
    """the rows of x (rows, L <= n) extended with zeros to n scalars, in double"""
    x = np.atleast_2d(np.asarray(x, dtype=np.float64))
    assert x.shape[1] <= n
    out = np.zeros((x.shape[0], n))
    out[:, :x.shape[1]] = x
    return out


def cross_spectrum(x, y, n, correlate):
    """P = X * Y, or X * conj(Y): the unscaled half spectra (n / 2 + 1 bins) of the extended rows multiplied"""
    fx, fy = np.fft.rfft(extend(x, n), axis=1), np.fft.rfft(extend(y, n), axis=1)
    return fx * (np.conj(fy) if correlate else fy)


def phat_weight(p, floor):
    """P / max(|P|, floor)"""
    return p / np.maximum(np.abs(p), floor)


def pairs(x, y, n, correlate, out_length=None, forward_scale=1.0, backward_scale=1.0, phat_floor=None):
    """the rows convolve_pairs (correlate=False) or correlate_pairs (correlate=True) store, in double:
    forward_scale ** 2 * backward_scale * n * irfft(P), or backward_scale * n * irfft(P / max(|P|, phat_floor))"""
    p = cross_spectrum(x, y, n, correlate)
    if phat_floor is None:
        r = forward_scale * forward_scale * backward_scale * n * np.fft.irfft(p, n, axis=1)
    else:
        assert correlate, "the phase transform belongs to the correlation"
        r = backward_scale * n * np.fft.irfft(phat_weight(p, phat_floor), n, axis=1)
    return r[:, :n if out_length is None else out_length]


def direct(x, y, n, correlate):
    """the O(N^2) sums of the definitions, scales of 1:
    convolve   r[l] = sum_n xe[n] * ye[(l - n) mod N];   correlate   r[l] = sum_n xe[(n + l) mod N] * ye[n]"""
    xe, ye = extend(x, n), extend(y, n)
    r = np.zeros_like(xe)
    idx = np.arange(n)
    for l in range(n):
        if correlate:
            r[:, l] = (xe[:, (idx + l) % n] * ye).sum(axis=1)
        else:
            r[:, l] = (xe * ye[:, (l - idx) % n]).sum(axis=1)
    return r


def pair_step_model(x, y, n, correlate, phat_floor=None):
    """What the kernel computes with scales of 1, step by step as it does: the rows as M = n / 2 complex numbers z[j] =
    x[2j] + i x[2j+1], their M-point spectra ZA, ZB, the pair step over k = 0 ... M/2 -- untangle both, multiply, weight,
    re-tangle into conj(Z') -- and the conjugate-in / conjugate-out inverse, whose real and imaginary parts are the even
    and odd result scalars."""
    m = n // 2
    xe, ye = extend(x, n), extend(y, n)
    za = np.fft.fft(xe[:, 0::2] + 1j * xe[:, 1::2], axis=1)
    zb = np.fft.fft(ye[:, 0::2] + 1j * ye[:, 1::2], axis=1)
    img = za.copy()  # image A: read and rewritten in place, slots k and M - k by the same work item
    floor = 0.0 if phat_floor is None else float(phat_floor)

    def untangle(a, b, w):  # a = Z[k], b = conj(Z[M-k]) -> X[k], X[M-k]
        s, d = a + b, a - b
        t = d * w
        return 0.5 * (s - 1j * t), np.conj(0.5 * (s + 1j * t))

    for k in range(m // 2 + 1):
        a, ya = za[:, k], zb[:, k]
        if k == 0:
            p0 = (a.real + a.imag) * (ya.real + ya.imag)
            pm = (a.real - a.imag) * (ya.real - ya.imag)
            if floor > 0:
                p0 = p0 / np.maximum(np.abs(p0), floor)
                pm = pm / np.maximum(np.abs(pm), floor)
            img[:, 0] = (p0 + pm) + 1j * (pm - p0)
            continue
        w = np.exp(-2j * np.pi * k / n)
        xk, xm = untangle(a, np.conj(za[:, m - k]), w)
        yk, ym = untangle(ya, np.conj(zb[:, m - k]), w)
        if correlate:
            yk, ym = np.conj(yk), np.conj(ym)
        pk, pm = xk * yk, xm * ym
        if floor > 0:
            pk = pk / np.maximum(np.abs(pk), floor)
            pm = pm / np.maximum(np.abs(pm), floor)
        s = pk + np.conj(pm)
        q = 1j * np.conj(w) * (pk - np.conj(pm))
        img[:, k] = np.conj(s + q)
        if 2 * k != m:
            img[:, m - k] = s - q
    z = np.conj(np.fft.fft(img, axis=1))  # conj(DFT_M(conj(Z'))): the unnormalised inverse of Z'
    r = np.empty_like(xe)
    r[:, 0::2], r[:, 1::2] = z.real, z.imag
    return r
