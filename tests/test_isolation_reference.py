"""The taint sets of helpers (taint_frames, taint_periodogram_rows, taint_samples, taint_filter) against the NumPy references
of the verbs, on the CPU: the reference runs on data with one poisoned sample or frame, and the non-finite part of its
result must be exactly the set the helper names -- for `filter` between the required cone and the permitted segments.  The
sets come from the definitions in include/portfft_amd.h; the references know nothing of them.  Geometries: odd hop and
lead, reflection at both ends inside one frame, a sample in the last partial frame, the last partial segment."""
import numpy as np
import pytest

import helpers as H
from dct4_ref import frames_of, mdct_reference
from imdct_ref import imdct_reference
from test_gpu_istft import _reference as istft_reference
from test_gpu_periodogram import rows_of
from test_gpu_stft import _reference as stft_reference

P_LONG = 211  # an odd prime above in_length + signals: one sample per signal of a periodic input is poisoned


def _nonfinite_rows(a):
    """rows of a 2-D result that are non-finite; a row must be so in every element or in none"""
    bad = ~np.isfinite(a)
    assert np.all(bad.all(axis=1) == bad.any(axis=1)), "a row is partly non-finite"
    return np.flatnonzero(bad.any(axis=1))


# (n, hop, lead, pad, in_length, frames, samples to poison)
STFT = [
    (16, 5, 7, "zero", 37, 9, (0, 3, 18, 36)),        # odd hop and lead; 36 lies in the partial frames at the end
    (16, 5, 7, "reflect", 37, 7, (0, 1, 6, 18, 35, 36)),
    (16, 16, 7, "reflect", 8, 1, (0, 3, 7)),          # both ends reflect inside the one frame
    (16, 1, 7, "reflect", 8, 2, (0, 7)),
    (8, 11, 0, "zero", 30, 3, (8, 9, 10, 29)),        # hop above N: samples 8 ... 10 lie in no frame
    (4, 3, 1, "zero", 9, 4, (8,)),                    # the last frame holds x[L-1] only
    (14, 5, 8, "zero", 33, 7, (0, 3, 17, 32)),        # odd M = N / 2 (helpers.ODD_RADIX_LENGTHS): M = 7, an even lead
    (14, 5, 8, "reflect", 33, 7, (0, 1, 7, 17, 32)),
    (26, 7, 14, "zero", 61, 8, (0, 5, 30, 60)),       # M = 13
    (30, 11, 16, "reflect", 70, 6, (0, 15, 35, 69)),  # M = 15
]


@pytest.mark.parametrize("n,hop,lead,pad,length,frames,samples", STFT)
def test_stft_and_periodogram_frames_that_hold_a_sample(n, hop, lead, pad, length, frames, samples):
    rng = np.random.default_rng(n + hop)
    x = rng.uniform(-1, 1, (2, length))
    w = rng.uniform(0.5, 1, n)
    for t in samples:
        xp = x.copy()
        H.poison_numpy(xp[0], [t])
        got = stft_reference(1.0, xp, w, n, hop, lead, pad, frames)
        want = H.taint_frames(t, n, hop, lead, pad, frames, length)
        assert np.array_equal(_nonfinite_rows(got[0]), want), (t, want)
        assert np.all(np.isfinite(got[1]))
        for avg in (1, 2, frames):
            rows = rows_of(np.abs(got) ** 2, avg)
            assert np.array_equal(_nonfinite_rows(rows[0]), H.taint_periodogram_rows(t, n, hop, lead, pad, frames, length, avg))
            assert np.all(np.isfinite(rows[1]))
    if hop > n:
        assert H.taint_frames(n, n, hop, lead, pad, frames, length).size == 0


@pytest.mark.parametrize("n,hop,lead,pad,length,frames", [c[:6] for c in STFT if c[3] == "zero" or c[1] >= 5])
def test_stft_rows_of_a_periodic_input(n, hop, lead, pad, length, frames):
    """helpers.stft_rows on base[(t + i) mod P] with P above the signals: base[b] is sample b - i of signal i"""
    ns, m = 3, n // 2
    base = np.random.default_rng(3).uniform(-1, 1, P_LONG)
    for b in (2, length // 2, length - 1):
        bp = base.copy()
        H.poison_numpy(bp, [b])
        start, valid, key, ref = H.stft_rows(bp, None, 1.0, n, ns, length, hop, lead, pad, frames, m + 2, frames * (m + 2) + 3)
        bad = _nonfinite_rows(ref[key]).tolist()
        want = [i * frames + int(f) for i in range(ns) for f in H.taint_frames(b - i, n, hop, lead, pad, frames, length)]
        assert bad == want, (b, bad, want)


@pytest.mark.parametrize("n,lead,length,frames", [(8, 8, 29, 5), (8, 5, 29, 5), (4, 0, 13, 3), (16, 31, 40, 5), (14, 15, 50, 5),
                                                  (26, 27, 95, 5)])
def test_mdct_frames_that_hold_a_sample(n, lead, length, frames):
    rng = np.random.default_rng(n + lead)
    x = rng.uniform(-1, 1, length)
    w = rng.uniform(0.5, 1, 2 * n)
    for t in (0, 1, length // 2, length - 1):
        xp = x.copy()
        H.poison_numpy(xp, [t])
        got = mdct_reference(frames_of(xp, n, lead, frames, w))
        assert np.array_equal(_nonfinite_rows(got), H.taint_frames(t, 2 * n, n, lead, "zero", frames, length)), t


ISTFT = [(16, 5, 7, 9, 49), (16, 5, 7, 9, 46), (16, 16, 0, 3, 48), (8, 3, 1, 6, 20), (8, 8, 7, 4, 25),  # n, hop, lead, frames, out
         (14, 5, 8, 9, 40), (26, 7, 14, 9, 60)]  # (odd M = N / 2)


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("n,hop,lead,frames,olen", ISTFT)
def test_istft_samples_that_a_frame_covers(n, hop, lead, frames, olen, normalize):
    rng = np.random.default_rng(n + hop)
    y = rng.uniform(-1, 1, (2, frames, n // 2 + 1)) + 1j * rng.uniform(-1, 1, (2, frames, n // 2 + 1))
    w = rng.uniform(0.5, 1, n)
    for f in (0, frames // 2, frames - 1):
        yp = y.copy()
        H.poison_numpy(yp[0, f])
        ola, env = istft_reference(1.0, yp, w, n, hop, lead, olen)
        assert env.min() >= 0.25
        got = np.where(env > 1e-11, ola / env, 0.0) if normalize else ola
        want = H.taint_samples(f, n, hop, lead, olen)
        assert want.size and np.array_equal(np.flatnonzero(~np.isfinite(got[0])), want), (f, want)
        assert np.all(np.isfinite(got[1]))


def test_istft_samples_without_envelope_are_zero_whatever_the_frames_hold():
    """periodic Hann at hop = N: w[0] = 0, the envelope at the frame starts is exactly 0 and NORMALIZE defines those samples
    as exactly 0 -- untainted, though a poisoned frame covers them"""
    n, frames = 16, 3
    w = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(n) / n)
    assert w[0] == 0.0
    rng = np.random.default_rng(9)
    y = rng.uniform(-1, 1, (1, frames, n // 2 + 1)) + 0j
    H.poison_numpy(y[0, 1])
    ola, env = istft_reference(1.0, y, w, n, n, 0, frames * n)
    got = np.where(env > 1e-11, ola / np.where(env > 1e-11, env, 1.0), 0.0)
    covered = H.taint_samples(1, n, n, 0, frames * n)
    assert covered[0] == n and env[n] == 0.0 and not np.isfinite(ola[0, n])
    assert got[0, n] == 0.0
    assert np.array_equal(np.flatnonzero(~np.isfinite(got[0])), covered[1:])


@pytest.mark.parametrize("n,lead,frames,olen", [(8, 8, 5, 32), (8, 8, 5, 29), (8, 5, 4, 27), (4, 0, 3, 16), (16, 31, 4, 33),
                                                (14, 15, 5, 55), (26, 27, 4, 77)])
def test_imdct_samples_that_a_frame_covers(n, lead, frames, olen):
    rng = np.random.default_rng(n + lead)
    c = rng.uniform(-1, 1, (2, frames, n))
    w = rng.uniform(0.5, 1, 2 * n)
    for f in (0, frames // 2, frames - 1):
        cp = c.copy()
        H.poison_numpy(cp[0, f])
        got = imdct_reference(cp, w, n, lead, olen)
        want = H.taint_samples(f, 2 * n, n, lead, olen)
        assert want.size and np.array_equal(np.flatnonzero(~np.isfinite(got[0])), want), (f, want)
        assert np.all(np.isfinite(got[1]))


@pytest.mark.parametrize("real", [False, True])
@pytest.mark.parametrize("correlate", [False, True])
@pytest.mark.parametrize("n,k", [(16, 1), (16, 5), (16, 4), (32, 9), (16, 14), (14, 7), (26, 24), (30, 1)])
def test_filter_outputs_between_the_cone_and_the_segments(n, k, correlate, real):
    """helpers.filter_rows (direct sums) on a periodic input with P above the signals"""
    ns, length = 3, 61
    olen = length if correlate else length + k - 1
    hop, lead = H.filter_geometry(n, k, correlate, real)
    olen -= olen % hop == 0  # the last segment is partial
    assert hop >= 1 and olen % hop != 0 and (not real or (hop % 2 == 0 and lead % 2 == 0))
    rng = np.random.default_rng(n + k)
    base = rng.uniform(-1, 1, P_LONG) + (0 if real else 1j * rng.uniform(-1, 1, P_LONG))
    taps = rng.uniform(-1, 1, (2, k)) + (0 if real else 1j * rng.uniform(-1, 1, (2, k)))
    out_pitch = olen + 3
    for b in (2, 30, length - 1):  # the first segment, the middle, the last sample of signal 0
        bp = base.copy()
        H.poison_numpy(bp, [b])
        start, valid, key, ref = H.filter_rows(bp, taps, 1.0, ns, length, olen, out_pitch, hop, correlate)
        y = np.zeros(ns * out_pitch, dtype=ref.dtype)
        for r in range(start.size):
            y[start[r]:start[r] + valid[r]] = ref[key[r], :valid[r]]
        for i in range(ns):
            bad = np.flatnonzero(~np.isfinite(y[i * out_pitch:i * out_pitch + olen]))
            required, permitted = H.taint_filter(b - i, n, k, correlate, real, olen)
            assert required.size and np.isin(required, bad).all() and np.isin(bad, permitted).all(), (b, i, bad, required)
            assert np.isin(required, permitted).all()
            assert np.array_equal(bad, required)  # (direct sums: exactly the cone)


def test_the_permitted_set_is_whole_segments_and_the_real_geometry_is_even():
    # complex convolve, N = 16, K = 5: hop 12, segment s holds samples [12 s - 4, 12 s + 12)
    req, per = H.taint_filter(10, 16, 5, False, False, 40)
    assert req.tolist() == [10, 11, 12, 13, 14] and per.tolist() == list(range(0, 24))
    req, per = H.taint_filter(39, 16, 5, False, False, 40)
    assert req.tolist() == [39] and per.tolist() == list(range(36, 40))
    # real convolve, K = 4: lead 4 (K - 1 rounded up), hop 12; correlate: hop 12 (13 rounded down), windows [12 s, 12 s + 16)
    assert H.filter_geometry(16, 4, False, True) == (12, 4) and H.filter_geometry(16, 4, True, True) == (12, 0)
    req, per = H.taint_filter(13, 16, 4, True, True, 30)
    assert req.tolist() == [10, 11, 12, 13] and per.tolist() == list(range(0, 24))
    assert H.filter_geometry(16, 5, False, False) == (12, 4) and H.filter_geometry(16, 5, True, False) == (12, 0)
