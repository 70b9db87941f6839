"""The double-precision reference of convolve_pairs / correlate_pairs (tests/pairs_ref.py) against the O(N^2) sums of the
definitions, against np.convolve / np.correlate where nothing aliases, and the NumPy model of the kernel's pair step
against the reference: the algebra of stockham_wg_pairs.hpp and its factors of 1/2, pinned without a GPU.

The backward transform is unnormalised, as everywhere in the library: with scales of 1 a result row is N times the sum of
the definition (N * irfft in NumPy's terms), and backward_scale = 1 / N gives the plain sum."""
import numpy as np
import pytest

import pairs_ref as R

LENGTHS = (4, 8, 12, 64) + (14, 26, 30, 54, 122)  # (odd M = N / 2, prime and composite: helpers.ODD_RADIX_LENGTHS)


def _rows(rng, rows, length):
    return rng.uniform(-1, 1, (rows, length))


def _shapes(n):
    """(x_length, y_length): full rows, lengths below N and odd, one scalar, the alias-free halves"""
    return sorted({(n, n), (n - 1, n // 2 + 1), (1, n), (n // 2, n // 2), (3, n - 1)})


@pytest.mark.parametrize("n", LENGTHS)
def test_the_reference_is_the_direct_sum(n):
    rng = np.random.default_rng(n)
    for lx, ly in _shapes(n):
        x, y = _rows(rng, 3, lx), _rows(rng, 3, ly)
        for correlate in (False, True):
            got, want = R.pairs(x, y, n, correlate), n * R.direct(x, y, n, correlate)
            assert np.abs(got - want).max() <= 1e-13 * n * n, (n, lx, ly, correlate)
            scaled = R.pairs(x, y, n, correlate, out_length=n - 1, forward_scale=0.5, backward_scale=1.0 / n)
            assert scaled.shape == (3, n - 1)
            assert np.abs(scaled - 0.25 / n * want[:, :n - 1]).max() <= 1e-13 * n


@pytest.mark.parametrize("n", LENGTHS)
def test_without_aliasing_it_is_numpys_linear_convolution_and_correlation(n):
    rng = np.random.default_rng(100 + n)
    lx, ly = n // 2, n // 2
    x, y = _rows(rng, 2, lx), _rows(rng, 2, ly)
    conv, corr = (R.pairs(x, y, n, mode, backward_scale=1.0 / n) for mode in (False, True))
    for t in range(2):
        full = np.convolve(x[t], y[t])
        assert np.abs(conv[t, :lx + ly - 1] - full).max() <= 1e-13
        assert np.abs(conv[t, lx + ly - 1:]).max() <= 1e-13
        lags = np.correlate(x[t], y[t], "full")  # lags -(ly - 1) ... lx - 1
        assert np.abs(corr[t, :lx] - lags[ly - 1:]).max() <= 1e-13  # lags 0 ... lx - 1 at the front
        assert np.abs(corr[t, n - (ly - 1):] - lags[:ly - 1]).max() <= 1e-13  # lags -(ly - 1) ... -1 up to r[N - 1]
        assert np.abs(corr[t, lx:n - (ly - 1)]).max() <= 1e-13


@pytest.mark.parametrize("n", LENGTHS)
def test_the_sign_convention_is_the_filters(n):
    """correlate_pairs(x, y) is what filter(correlate=True) computes with y as the filter: sum_k conj(h[k]) x[l + k]"""
    rng = np.random.default_rng(200 + n)
    x, h = _rows(rng, 1, n), _rows(rng, 1, n // 2)
    got = R.pairs(x, h, n, True, backward_scale=1.0 / n)[0]
    want = np.array([sum(h[0, k] * x[0, (l + k) % n] for k in range(n // 2)) for l in range(n)])
    assert np.abs(got - want).max() <= 1e-13 * n


@pytest.mark.parametrize("n", LENGTHS)
def test_the_pair_step_model_is_the_reference(n):
    rng = np.random.default_rng(300 + n)
    for lx, ly in _shapes(n):
        x, y = _rows(rng, 3, lx), _rows(rng, 3, ly)
        for correlate in (False, True):
            got, want = R.pair_step_model(x, y, n, correlate), R.pairs(x, y, n, correlate)
            assert np.abs(got - want).max() <= 1e-13 * max(1.0, np.abs(want).max()), (n, lx, ly, correlate)
        p = np.abs(R.cross_spectrum(x, y, n, True))
        for floor in (float(np.median(p)), 1e-3, 1e30):  # both branches in one row; all above; all below
            got = R.pair_step_model(x, y, n, True, phat_floor=floor)
            want = R.pairs(x, y, n, True, phat_floor=floor)
            assert np.abs(got - want).max() <= 1e-13 * max(1.0, np.abs(want).max()), (n, lx, ly, floor)


def test_the_phase_transform_of_a_rotation_is_a_delta():
    n, d = 64, 5
    rng = np.random.default_rng(7)
    y = _rows(rng, 1, n)
    x = np.roll(y, d, axis=1)  # x[n] = y[n - d]: x lags y by d
    r = R.pairs(x, y, n, True, phat_floor=1e-12)[0]
    assert int(np.argmax(r)) == d
    assert abs(r[d] - n) <= 1e-9 and np.abs(np.delete(r, d)).max() <= 1e-9
    # with a huge floor the weights are P / floor: floor * r is the plain correlation
    plain = R.pairs(x, y, n, True)[0]
    assert np.abs(1e30 * R.pairs(x, y, n, True, phat_floor=1e30)[0] - plain).max() <= 1e-12 * np.abs(plain).max()
    # silence stays silent
    assert not R.pairs(np.zeros((1, n)), y, n, True, phat_floor=1e-3).any()
