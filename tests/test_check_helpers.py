"""The checks of the GPU harness, on the CPU: each checker passes a correct output (NumPy) and fails the same output with
one planted defect, naming the element or transform.  (helpers.check_write_set / check_guards / check_unchanged behind
gpu_utils.run and transform_packed; helpers.check_every_transform behind the full-size, big-buffer and XCD-local tests.)"""
import re

import numpy as np
import pytest
import torch

import helpers as H


# ---------------------------------------------------------------------------------------------------------------------
# write sets

def _gapped(storage, seed=0):
    """an UNPACKED output (rows of 16 in a pitch of 20, offset 3) and its index set, as a correct execute leaves it"""
    batch, n, pitch, off = 4, 16, 20, 3
    x, y = H.gen_fourier_data(batch, [n], np.complex64, seed=seed)
    buf = H.scatter(y, [1], pitch, off, off + batch * pitch,
                    pad=H.PADDING_VALUE * (1 + 1j) if storage == "split" else H.PADDING_VALUE)
    idx = H.element_indices(batch, [n], [1], pitch, off)
    if storage == "split":
        return (buf.real.copy(), buf.imag.copy()), idx
    return buf, idx


@pytest.mark.parametrize("storage", ["interleaved", "split"])
def test_write_set_passes_a_clean_output_and_fails_one_gap_element(storage):
    buf, idx = _gapped(storage)
    H.check_write_set(buf, idx)
    gaps = np.setdiff1d(np.arange(83), idx.ravel())
    for gap in (0, int(gaps[5]), 82):  # before the offset, between two rows, the last element
        bad = tuple(p.copy() for p in buf) if storage == "split" else buf.copy()
        if storage == "split":
            bad[1][gap] = 0.0  # the imaginary plane alone
        else:
            bad[gap] = complex(H.PADDING_VALUE, 1e-30)  # one bit pattern off, in the imaginary part
        with pytest.raises(AssertionError, match=r"first at \[%d\]" % gap):
            H.check_write_set(bad, idx)


def test_write_set_sees_a_negative_zero_and_a_nan():
    buf, idx = _gapped("interleaved")
    gap = int(np.setdiff1d(np.arange(83), idx.ravel())[0])
    for v in (complex(H.PADDING_VALUE, -0.0), complex(np.nan, 0.0)):
        bad = buf.copy()
        bad[gap] = v
        with pytest.raises(AssertionError, match="written outside"):
            H.check_write_set(bad, idx)


@pytest.mark.parametrize("storage", ["interleaved", "split"])
def test_guards_pass_untouched_bands_and_fail_one_written_element(storage):
    lo, count, hi = 64, 100, 64
    rng = np.random.default_rng(1)
    body = (rng.standard_normal(count) + 1j * rng.standard_normal(count)).astype(np.complex128)

    def alloc():
        if storage == "split":  # the padding value in both planes
            planes = [np.full(lo + count + hi, H.PADDING_VALUE) for _ in range(2)]
            planes[0][lo:lo + count], planes[1][lo:lo + count] = body.real, body.imag
            return tuple(planes)
        a = np.full(lo + count + hi, H.PADDING_VALUE, dtype=np.complex128)
        a[lo:lo + count] = body
        return a

    H.check_guards(alloc(), lo, count)
    for pos, side, name in ((lo - 1, "before", -1), (0, "before", -64), (lo + count, "after", count),
                            (lo + count + hi - 1, "after", count + hi - 1)):
        a = alloc()
        if storage == "split":
            a[0][pos] = 1.0
        else:
            a[pos] = 1.0
        with pytest.raises(AssertionError, match=r"guard %s the buffer was written at element\(s\) \[%d\]" % (side, name)):
            H.check_guards(a, lo, count)


@pytest.mark.parametrize("storage", ["interleaved", "split"])
def test_unchanged_input_passes_a_copy_and_fails_one_changed_element(storage):
    x, _ = H.gen_fourier_data(3, [64], np.complex64, seed=2)
    x = x.ravel()
    before = (x.real.copy(), x.imag.copy()) if storage == "split" else x.copy()
    after = tuple(p.copy() for p in before) if storage == "split" else before.copy()
    H.check_unchanged(before, after, what="input")
    if storage == "split":
        after[1][77] = np.nextafter(after[1][77], np.float32(2))
    else:
        after[77] = complex(after[77].real, np.nextafter(after[77].imag, np.float32(2)))
    with pytest.raises(AssertionError, match=r"input.*changed: 1 element\(s\), first at \[77\]"):
        H.check_unchanged(before, after, what="input")


# ---------------------------------------------------------------------------------------------------------------------
# every transform against the fp64 probe

def _batch(lengths, batch, prec, seed=3, direction=H.FORWARD, scale=1.0):
    """input, and the output of a correct execute in the precision under test (NumPy, rounded to the storage type)"""
    dtype = np.complex64 if prec == "f32" else np.complex128
    x, _ = H.gen_fourier_data(batch, lengths, dtype, seed=seed)
    axes = tuple(range(1, len(lengths) + 1))
    xd = x.astype(np.complex128)
    y = np.fft.fftn(xd, axes=axes) if direction == H.FORWARD else np.fft.ifftn(xd, axes=axes) * np.prod(lengths)
    return x, (y * scale).astype(dtype)


def _flat(a):
    return torch.from_numpy(np.ascontiguousarray(a).ravel())


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("lengths,direction,scale", [([4096], H.FORWARD, 1.0), ([96], H.BACKWARD, 0.5),
                                                     ([12, 40], H.FORWARD, -2.0), ([1], H.FORWARD, 1.0)])
def test_probe_passes_correct_outputs(prec, lengths, direction, scale):
    batch = 37
    x, y = _batch(lengths, batch, prec, direction=direction, scale=scale)
    st = H.check_every_transform(_flat(x), _flat(y), lengths, batch, scale=scale, direction=direction, prec=prec)
    assert st["transforms"] == batch and st["probes"] == 8 * batch
    assert st["max"] <= st["tau"] / 2, st


def test_probe_covers_every_bin_across_the_batch():
    """with batch * (k - 3) >= N every bin of the transform is probed in some transform"""
    n, batch, k = 96, 20, 8
    bins, _, _, _ = H._probe_bins([n], batch, k - 3, 0, batch, torch, torch.device("cpu"))
    assert set(bins[:, :, 0].ravel().tolist()) == set(range(n))
    assert all({0, n // 2, n - 1} <= set(bins[b, :, 0].tolist()) for b in range(batch))


def test_probe_passes_strided_split_and_chunked_layouts():
    """batch-interleaved input, a padded row layout with an offset on the output in split planes, and chunks smaller
    than one transform (the reference accumulated over several chunks of N)"""
    n, batch = 512, 24
    x, y = _batch([n], batch, "f32")
    xbi = np.ascontiguousarray(x.T).ravel()                  # strides [batch], distance 1
    pitch, off = n + 8, 5
    ybuf = H.scatter(y, [1], pitch, off, off + batch * pitch)
    st = H.check_every_transform(torch.from_numpy(xbi), (torch.from_numpy(ybuf.real.copy()), torch.from_numpy(ybuf.imag.copy())),
                                 [n], batch, in_layout=([batch], 1, 0), out_layout=([1], pitch, off), chunk_bytes=16 * 100)
    assert st["max"] <= st["tau"] / 2, st


def _planted(kind, prec="f32"):
    lengths, batch = [256], 64
    x, y = _batch(lengths, batch, prec)
    b = batch // 2 + 1
    bad = y.copy()
    k1 = (b * 5 + 1) % 256  # a bin that transform b probes (its moving probes start at b * (k - 3))
    if kind == "swap":
        bad[b, [k1, 200]] = bad[b, [200, k1]]
    elif kind == "other transform":
        bad[b] = y[b + 3]
    elif kind == "one bin 1e-4":
        bad[b, k1] += 1e-4 * np.abs(bad[b, k1]) * np.exp(0.7j)
    return x, bad, lengths, batch, b


@pytest.mark.parametrize("kind", ["swap", "other transform", "one bin 1e-4"])
def test_probe_fails_planted_defects_and_names_the_transform(kind):
    x, bad, lengths, batch, b = _planted(kind)
    with pytest.raises(AssertionError, match=r"transform %d of %d" % (b, batch)):
        H.check_every_transform(_flat(x), _flat(bad), lengths, batch, prec="f32", what=kind)


def test_probe_sees_a_swap_at_a_fixed_bin_in_every_transform():
    """two bins of the last transform swapped, one of them N/2 (probed in every transform)"""
    x, y = _batch([256], 50, "f64")
    y[49, [128, 3]] = y[49, [3, 128]]
    with pytest.raises(AssertionError, match=r"transform 49 of 50, bin \[(128|3)\]"):
        H.check_every_transform(_flat(x), _flat(y), [256], 50, prec="f64")


def test_probe_fails_a_defect_in_a_2d_transform():
    x, y = _batch([16, 24], 10, "f32")
    y[7, 0, 0] *= -1.0  # the DC bin, a fixed probe
    with pytest.raises(AssertionError, match=r"transform 7 of 10, bin \[0, 0\]"):
        H.check_every_transform(_flat(x), _flat(y), [16, 24], 10, prec="f32")


# ---------------------------------------------------------------------------------------------------------------------
# every row of a huge launch against a small periodic reference (check_rows / check_untouched / check_same_bits behind
# test_gpu_address_range.py)

P_ROWS = 7  # an odd prime of distinct rows / the period of a long signal


def _periodic_fft_case():
    """40 transforms of 16 points in a pitch of 20: row b holds base[b mod P]; the output of a correct execute"""
    batch, n, pitch = 40, 16, 20
    base, _ = H.gen_fourier_data(P_ROWS, [n], np.complex64, seed=5)
    ref = np.fft.fft(base.astype(np.complex128), axis=1)
    b = np.arange(batch)
    out = H.scatter(ref[b % P_ROWS].astype(np.complex64), [1], pitch, 0, batch * pitch)
    return out, b * pitch, np.full(batch, n), b % P_ROWS, ref, n


def test_rows_pass_a_correct_output_and_fail_a_row_displaced_by_a_power_of_two():
    out, start, valid, key, ref, n = _periodic_fft_case()
    tol = H.REL_L2_TOL[np.dtype(np.complex64)]
    worst = H.check_rows(torch.from_numpy(out), start, valid, key, ref, tol, rule_n=n, chunk=16 * 7)
    assert 0 < worst <= tol / 2
    H.check_untouched(torch.from_numpy(out), start, valid)
    for shift in (1, 2, 4, 8, 16):  # what a wrapped offset does: never a multiple of the odd prime
        bad = out.copy()
        bad[9 * 20:9 * 20 + n] = out[(9 + shift) * 20:(9 + shift) * 20 + n]
        with pytest.raises(AssertionError, match=r"row 9 of 40 \(element 180"):
            H.check_rows(torch.from_numpy(bad), start, valid, key, ref, tol, rule_n=n, what="displaced")
    bad = out.copy()  # the blind spot the docstring names: a whole multiple of P rows
    bad[9 * 20:9 * 20 + n] = out[(9 + P_ROWS) * 20:(9 + P_ROWS) * 20 + n]
    H.check_rows(torch.from_numpy(bad), start, valid, key, ref, tol, rule_n=n)


def test_rows_hold_one_element_to_the_per_element_rule_and_fp16_to_its_ulp():
    out, start, valid, key, ref, n = _periodic_fft_case()
    bad = out.copy()
    small = int(np.argmin(np.abs(ref[31 % P_ROWS])))
    bad[31 * 20 + small] += 3e-4  # within the row's relative L2, beyond 2 eps N log2 N
    H.check_rows(torch.from_numpy(bad), start, valid, key, ref, 1e-4)
    with pytest.raises(AssertionError, match=r"row 31 of 40 .*per-element rule"):
        H.check_rows(torch.from_numpy(bad), start, valid, key, ref, 1e-4, rule_n=n)
    # fp16 storage as interleaved scalar pairs: round16 of the reference passes, one component two ulps off fails
    r16 = ref[key]
    pairs = np.full((40, 20, 2), H.PADDING_VALUE, dtype=np.float16)
    pairs[:, :n, 0], pairs[:, :n, 1] = r16.real, r16.imag
    e = ref.astype(np.complex128)
    rounded = e.real.astype(np.float16).astype(np.float64) + 1j * e.imag.astype(np.float16).astype(np.float64)
    tol16 = 1.5 * np.linalg.norm(rounded - e, axis=1) / np.linalg.norm(e, axis=1) + 1e-6
    H.check_rows(torch.from_numpy(pairs.reshape(-1)), start, valid, key, ref, tol16, pairs=True, fp16=True)
    H.check_untouched(torch.from_numpy(pairs.reshape(-1)), start, valid, unit=2)
    big = int(np.argmax(np.abs(ref[3].real)))
    pairs[3, big, 0] += 2 * np.spacing(np.abs(pairs[3, big, 0]))
    with pytest.raises(AssertionError, match=r"row 3 of 40"):
        H.check_rows(torch.from_numpy(pairs.reshape(-1)), start, valid, key, ref, np.full(P_ROWS, 1.0), pairs=True, fp16=True)
    v = np.array([0.0, 1.0, -3.0, 1e-6, 0.7, 1024.0, 2.0 ** -14, 6e-8])
    assert np.array_equal(H._ulp16(torch.from_numpy(v), torch).numpy(), np.spacing(np.abs(v).astype(np.float16)).astype(np.float64))


def _filter_case(correlate, real=False):
    """3 signals of 3 ragged segments, a filter per signal, pitched: (x, out, rows) of a correct NumPy result"""
    rng = np.random.default_rng(11)
    k, hop, ns, in_length, in_pitch = 5, 12, 3, 31, 37
    out_length = in_length if correlate else in_length + k - 1
    out_pitch = out_length + 3
    if real:
        base, taps = rng.uniform(-1, 1, P_ROWS).astype(np.float32), rng.uniform(-1, 1, (ns, k)).astype(np.float32)
    else:
        base = (rng.uniform(-1, 1, P_ROWS) + 1j * rng.uniform(-1, 1, P_ROWS)).astype(np.complex64)
        taps = (rng.uniform(-1, 1, (ns, k)) + 1j * rng.uniform(-1, 1, (ns, k))).astype(np.complex64)
    x = torch.full((ns * in_pitch,), H.PADDING_VALUE, dtype=torch.from_numpy(base).dtype)
    H.fill_periodic(x, torch.from_numpy(base), ns, in_length, in_pitch, torch, chunk=8)
    out = np.full(ns * out_pitch, H.PADDING_VALUE, dtype=base.dtype)
    for i in range(ns):
        xi = x.numpy()[i * in_pitch:i * in_pitch + in_length].astype(np.complex128 if not real else np.float64)
        np.testing.assert_array_equal(xi, H.periodic_signal(base, i, 0, in_length, in_length))
        if correlate:
            full = np.correlate(np.concatenate([xi, np.zeros(k - 1)]), taps[i].astype(xi.dtype), "valid")
        else:
            full = np.convolve(xi, taps[i].astype(xi.dtype))
        out[i * out_pitch:i * out_pitch + out_length] = 2.0 * full[:out_length]
    rows = H.filter_rows(base, taps, 2.0, ns, in_length, out_length, out_pitch, hop, correlate)
    return out, rows, hop, out_pitch


@pytest.mark.parametrize("real", [False, True])
@pytest.mark.parametrize("correlate", [False, True])
def test_rows_of_a_filter_pass_numpy_and_fail_a_segment_taken_from_another(correlate, real):
    out, (start, valid, key, ref), hop, out_pitch = _filter_case(correlate, real)
    tol = H.REL_L2_TOL[np.dtype(np.complex64)]
    assert len(start) == 9 and ref.shape[0] > 3 * P_ROWS  # the rows at the ends of a signal have references of their own
    H.check_rows(torch.from_numpy(out), start, valid, key, ref, tol, rule_n=16, what="filter")
    H.check_untouched(torch.from_numpy(out), start, valid)
    bad = out.copy()  # segment 1 of signal 1 holds the outputs of segment 0 of signal 2
    bad[out_pitch + hop:out_pitch + 2 * hop] = out[2 * out_pitch:2 * out_pitch + hop]
    with pytest.raises(AssertionError, match=r"row 4 of 9 \(element %d" % (out_pitch + hop)):
        H.check_rows(torch.from_numpy(bad), start, valid, key, ref, tol, rule_n=16, what="filter")
    bad = out.copy()  # ... and those of its own neighbour, one hop on
    bad[out_pitch + hop:out_pitch + 2 * hop - 5] = out[out_pitch + 2 * hop:out_pitch + 3 * hop - 5]
    with pytest.raises(AssertionError, match=r"row 4 of 9"):
        H.check_rows(torch.from_numpy(bad), start, valid, key, ref, tol, rule_n=16, what="filter")


@pytest.mark.parametrize("pad", ["zero", "reflect"])
def test_rows_of_an_stft_pass_numpy_and_fail_one_frame_and_one_gap_element(pad):
    rng = np.random.default_rng(12)
    n, hop, lead, ns, in_length = 16, 5, 8, 3, 61
    m, frames = n // 2, 10
    frame_pitch, out_pitch = m + 3, 10 * (m + 3) + 2
    base = rng.uniform(-1, 1, P_ROWS).astype(np.float32)
    w = rng.uniform(-1, 1, n).astype(np.float32)
    out = np.full(ns * out_pitch, H.PADDING_VALUE, dtype=np.complex64)
    for i in range(ns):
        xi = H.periodic_signal(base, i, 0, in_length, in_length).astype(np.float64)
        xe = np.pad(xi, (lead, lead + n), mode="reflect" if pad == "reflect" else "constant")
        for f in range(frames):
            out[i * out_pitch + f * frame_pitch:][:m + 1] = 0.5 * np.fft.rfft(xe[f * hop:f * hop + n] * w)
    start, valid, key, ref = H.stft_rows(base, w, 0.5, n, ns, in_length, hop, lead, pad, frames, frame_pitch, out_pitch)
    assert ref.shape[0] > P_ROWS  # frames at the ends
    tol = H.REL_L2_TOL[np.dtype(np.complex64)]
    H.check_rows(torch.from_numpy(out), start, valid, key, ref, tol, rule_n=n, what="stft")
    H.check_untouched(torch.from_numpy(out), start, valid)
    bad = out.copy()  # frame 4 of signal 1 holds frame 6
    bad[out_pitch + 4 * frame_pitch:][:m + 1] = out[out_pitch + 6 * frame_pitch:][:m + 1]
    with pytest.raises(AssertionError, match=r"row 14 of 30"):
        H.check_rows(torch.from_numpy(bad), start, valid, key, ref, tol, rule_n=n, what="stft")
    for gap in (m + 1, out_pitch - 1, 2 * out_pitch + 3 * frame_pitch - 1):  # behind a frame, between two signals
        bad = out.copy()
        bad[gap] = complex(H.PADDING_VALUE, 1e-30)
        with pytest.raises(AssertionError, match=r"first at \[%d\]" % gap):
            H.check_untouched(torch.from_numpy(bad), start, valid, chunk=64)


def test_same_bits_names_the_first_changed_element():
    a = torch.arange(1000, dtype=torch.float32)
    b = a.clone()
    H.check_same_bits(a, b, chunk=128)
    b[777] = -0.0 + 777  # the same value: still equal
    H.check_same_bits(a, b, chunk=128)
    b[0] = -0.0
    with pytest.raises(AssertionError, match=r"input changed: 1 element\(s\) in \[0, 128\), first at \[0\]"):
        H.check_same_bits(a, b, what="input", chunk=128)


# ---------------------------------------------------------------------------------------------------------------------
# basis vectors: the derived per-element bound

def test_twiddle_path_length():
    want = {1: 1, 2: 2, 3: 4, 4: 3, 8: 4, 13: 6, 30: 8, 37: 8, 100: 10, 1000: 14, 4096: 13, 1536: 13, 68640: 22}
    assert {n: H.twiddle_path_length(n) for n in want} == want
    assert H.basis_multiplies([64, 64], "c2c") == 14 and H.basis_multiplies(1024, "r2c") == 13
    assert H.basis_multiplies(1024, "dct4") == 14
    u = 2.0 ** -24
    assert H.basis_bound(4096, "c2c", "f32") == 3.3 * u * 13 and H.basis_bound(64, "c2r", "f32", 0.5) == 3.3 * u * 9
    assert H.basis_bound(64, "dct2", "f64") == 2 * 3.3 * 2.0 ** -53 * 10


def test_basis_references_are_the_matrix_rows():
    """every reference against NumPy's own transform of the identity (double: 1e-13 is its yardstick, not ours), and the
    exact values at the multiples of an eighth of a turn"""
    for n in (4, 6, 30, 64):
        eye = np.eye(n)
        rows = np.arange(n)
        assert np.abs(H.basis_reference(rows, n, "c2c") - np.fft.fft(eye, axis=1)).max() < 1e-13
        assert np.abs(H.basis_reference(rows, n, "c2c", H.BACKWARD) - n * np.fft.ifft(eye, axis=1)).max() < 1e-13
        assert np.abs(H.basis_reference(rows, n, "r2c") - np.fft.rfft(eye, axis=1)).max() < 1e-13
        bins = np.arange(n // 2 + 1)
        assert np.abs(H.basis_reference(bins, n, "c2r") - n * np.fft.irfft(np.eye(n // 2 + 1), n, axis=1)).max() < 1e-13
        from dct4_ref import dct4_reference
        from dct_ref import dct_reference
        assert np.abs(H.basis_reference(rows, n, "dct2") - dct_reference(eye, 2)).max() < 1e-13
        assert np.abs(H.basis_reference(rows, n, "dct3") - dct_reference(eye, 3)).max() < 1e-13
        assert np.abs(H.basis_reference(rows, n, "dct4") - dct4_reference(eye)).max() < 1e-13
    dims = [4, 6, 5]
    eye = np.eye(120).reshape([120] + dims)
    ref = H.basis_reference(np.arange(120), dims, "c2c")
    assert np.abs(ref - np.fft.fftn(eye, axes=(1, 2, 3)).reshape(120, 120)).max() < 1e-13
    for route in ("longdouble", "float64"):
        c, s = H.basis_circle(16, route)
        h = np.sqrt(c.dtype.type(0.5))
        assert list(c[[0, 4, 8, 12]]) == [1, 0, -1, 0] and list(s[[0, 4, 8, 12]]) == [0, 1, 0, -1]
        assert np.abs(np.abs(c[2::4]) - h).max() <= np.finfo(c.dtype).eps and np.abs(np.abs(s[2::4]) - h).max() <= np.finfo(c.dtype).eps


def test_the_two_reference_routes_agree_within_the_margin():
    """np.longdouble (host) and fp64 with the phase reduced to the first octant: they differ by less than 2^-52 of the
    amplitude, which is below 1/16 of every fp32 bound and of the fp64 bounds with 10 multiplies or more (5 where the fp64
    table is the long double one rounded) -- the split check_basis_rows makes"""
    assert np.finfo(np.longdouble).nmant >= 63
    for n in (2, 3, 8, 100, 1000, 4096, 68640, 1 << 20):
        (cl, sl), (cd, sd) = H.basis_circle(n, "longdouble"), H.basis_circle(n, "float64")
        diff = float(np.hypot(cl - cd, sl - sd).max())
        rounded = float(np.hypot(cl - cl.astype(np.float64), sl - sl.astype(np.float64)).max())
        assert diff <= 2.0 ** -52 and rounded <= 2.0 ** -53, (n, diff, rounded)
        assert diff <= H.basis_bound(n, "c2c", "f32") / H.BASIS_REF_MARGIN
        if H.twiddle_path_length(n) >= 10:
            assert diff <= H.basis_bound(n, "c2c", "f64") / H.BASIS_REF_MARGIN
        if H.twiddle_path_length(n) >= 5:
            assert rounded <= H.basis_bound(n, "c2c", "f64") / H.BASIS_REF_MARGIN
    # and check_basis_rows gives the same verdict and (nearly) the same ratio on both
    n = 64
    got = np.fft.fft(np.eye(n), axis=1).astype(np.complex64)
    a = H.check_basis_rows(got, np.arange(n), n, "c2c", "f32", route="longdouble")
    b = H.check_basis_rows(torch.from_numpy(got), np.arange(n), n, "c2c", "f32", route="float64")
    assert 0 < a < 0.5 and abs(a - b) <= 1.0 / H.BASIS_REF_MARGIN


def _two_stage_4096(x, delta=0.0, at=(37, 63)):
    """a 64 x 64 two-stage restatement of the forward FFT of N = 4096 (rows of x) in double, the inter-stage twiddle
    W^(k1 n2) at (k1, n2) = `at` scaled by 1 + delta; the result rounded to fp32"""
    r = np.arange(64)
    f64 = np.exp(-2j * np.pi * ((r[:, None] * r[None, :]) % 64) / 64)
    tw = np.exp(-2j * np.pi * (r[:, None] * r[None, :]) / 4096)   # [k1, n2]
    tw[at] *= 1 + delta
    a = np.asarray(x, dtype=np.complex128).reshape(-1, 64, 64)         # [b, n1, n2], n = 64 n1 + n2
    b = np.einsum("kn,bnm->bkm", f64, a) * tw                           # [b, k1, n2]
    d = np.einsum("bkm,mj->bkj", b, f64)                                # [b, k1, k2], k = k1 + 64 k2
    return d.transpose(0, 2, 1).reshape(-1, 4096).astype(np.complex64)


def test_one_wrong_twiddle_passes_the_old_yardsticks_and_fails_the_basis_check():
    n = 4096
    x, y = H.gen_fourier_data(8, [n], np.complex64, seed=3)
    rows = np.concatenate([64 * np.arange(64) + 63, [0, 1, 2, 62, 64, 4094]])   # every n1 at n2 = 63, and rows off it
    eye = np.zeros((rows.size, n))
    eye[np.arange(rows.size), rows] = 1
    for delta in (0.0, 1e-5):
        out = _two_stage_4096(x, delta)
        assert max(H.rel_l2(out[b], y[b]) for b in range(8)) <= H.REL_L2_TOL[np.dtype(np.complex64)]
        assert H.check_reference_rule(out, y, n)
    assert H.check_basis_rows(_two_stage_4096(eye), rows, n, "c2c", "f32", what="clean") < 0.1
    with pytest.raises(AssertionError, match=r"the transform of e_63, element \d+: \|got - ref\| is 3\.9\d* of the bound") as e:
        H.check_basis_rows(_two_stage_4096(eye, 1e-5), rows, n, "c2c", "f32", what="planted")
    # the row and the element name the entry: input digit n2 = 63, output digit k1 = 37
    assert int(re.search(r"element (\d+)", str(e.value)).group(1)) % 64 == 37
    # (the rows off n2 = 63 never meet the entry)
    H.check_basis_rows(_two_stage_4096(eye[64:], 1e-5), rows[64:], n, "c2c", "f32", what="planted, other rows")


def _dct2_quarter_wave(x, delta=0.0, at=1023):
    """DCT-II of the rows of x (N = 1024) in double by the even-odd permutation, one N-point FFT and the quarter-wave
    factors c_k = exp(-i pi k / 2N), the entry `at` scaled by 1 + delta; the result rounded to fp32"""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[1]
    v = np.concatenate([x[:, 0::2], x[:, ::-1][:, 0::2]], axis=1)
    c = np.exp(-1j * np.pi * np.arange(n) / (2 * n))
    c[at] *= 1 + delta
    return (2 * np.real(c * np.fft.fft(v, axis=1))).astype(np.float32)


def test_one_wrong_quarter_wave_factor_passes_the_old_yardsticks_and_fails_the_basis_check():
    from dct_ref import dct_reference
    n = 1024
    x = np.random.default_rng(5).uniform(-1, 1, (8, n)).astype(np.float32)
    ref = dct_reference(x, 2)
    for delta in (0.0, 1e-5):
        out = _dct2_quarter_wave(x, delta).astype(np.float64)
        err = np.linalg.norm(out - ref, axis=1) / np.linalg.norm(ref, axis=1)
        assert err.max() <= H.REL_L2_TOL[np.dtype(np.complex64)]
        assert H.check_reference_rule(out, ref.astype(np.complex64), n)
    eye = np.eye(n)
    assert H.check_basis_rows(_dct2_quarter_wave(eye), np.arange(n), n, "dct2", "f32", what="clean") < 0.1
    with pytest.raises(AssertionError, match=r"the transform of e_\d+, element 1023: .* of the bound"):
        H.check_basis_rows(_dct2_quarter_wave(eye, 1e-5), np.arange(n), n, "dct2", "f32", what="planted")


def test_basis_check_names_the_element_on_every_route_and_with_fp16_storage():
    n = 16
    rows = np.arange(n)
    ref = H.basis_reference(rows, n, "c2c", H.BACKWARD).astype(np.complex128)
    for prec, route, off in (("f64", None, 2e-15), ("f64", "longdouble", 2e-15), ("f32", None, 1e-6)):
        got = ref.astype(np.complex64 if prec == "f32" else np.complex128)
        H.check_basis_rows(got, rows, n, "c2c", prec, direction=H.BACKWARD, route=route)
        got[5, 9] += off
        with pytest.raises(AssertionError, match="the transform of e_5, element 9"):
            H.check_basis_rows(got, rows, n, "c2c", prec, direction=H.BACKWARD, route=route)
    # a length below 5 multiplies in fp64 takes the host route by itself
    eye4 = np.fft.fft(np.eye(4), axis=1)
    assert H.check_basis_rows(eye4, np.arange(4), 4, "c2c", "f64") <= 0.5
    # fp16 storage: half a binary16 ulp of the component on top of the fp32 bound; a whole ulp fails
    half = 0.25 * ref
    r16 = half.real.astype(np.float16).astype(np.float64) + 1j * half.imag.astype(np.float16).astype(np.float64)
    H.check_basis_rows(r16, rows, n, "c2c", "f16", scale=0.25, direction=H.BACKWARD)
    r16[3, 1] += np.spacing(np.float16(r16[3, 1].real)).astype(np.float64)
    with pytest.raises(AssertionError, match="the transform of e_3, element 1"):
        H.check_basis_rows(r16, rows, n, "c2c", "f16", scale=0.25, direction=H.BACKWARD)


# ---------------------------------------------------------------------------------------------------------------------
# read sets (check_isolated behind test_gpu_isolation.py): NumPy models of a kernel that read a value they must not depend
# on and multiply it by an exact zero.  On finite padding every yardstick passes; with POISON in those places the
# untainted results change.

def test_poison_is_the_quiet_nan_of_each_type_bit_for_bit():
    for dt, ut, bits in ((np.float16, np.uint16, 0x7E00), (np.float32, np.uint32, 0x7FC00000),
                         (np.float64, np.uint64, 0x7FF8000000000000)):
        assert np.isnan(H.POISON[dt]) and H.POISON[dt].dtype == np.dtype(dt)
        a = H.full(5, H.POISON, dt)
        assert np.all(a.view(ut) == bits)
        t = H.full_torch(5, H.POISON, torch.from_numpy(a[:0]).dtype, "cpu")
        assert np.all(t.numpy().view(ut) == bits)
    c = H.full(3, H.POISON, np.complex64)
    assert np.all(c.view(np.uint32) == 0x7FC00000)  # both components
    tc = torch.zeros(4, dtype=torch.complex128)
    H.poison_torch(tc, [1, 3])
    assert np.all(tc.numpy().view(np.uint64).reshape(4, 2)[[1, 3]] == 0x7FF8000000000000) and tc[0] == 0 and tc[2] == 0
    x = np.zeros((2, 3), dtype=np.float32)
    H.poison_numpy(x, [4])
    assert np.isnan(x[1, 1]) and np.count_nonzero(np.isnan(x)) == 1
    # guards and write sets that hold POISON are compared by their bits like any other padding
    buf = H.scatter(np.ones((2, 4), dtype=np.complex64), [1], 6, 1, 13, pad=H.POISON)
    idx = H.element_indices(2, [4], [1], 6, 1)
    H.check_write_set(buf, idx, pad=H.POISON)
    alloc = H.full(8, H.POISON, np.complex64)
    alloc[2:6] = 1
    H.check_guards(alloc, 2, 4, pad=H.POISON)
    with pytest.raises(AssertionError, match="guard after the buffer was written"):
        H.check_guards(alloc, 2, 3, pad=H.POISON)
    other = buf.copy()
    other.view(np.uint32)[2 * 12] = 0x7FC00001  # another NaN
    with pytest.raises(AssertionError, match=r"first at \[12\]"):
        H.check_write_set(other, idx, pad=H.POISON)


def _stft_model(buf, ns, in_pitch, in_length, n, hop, lead, frames, defect):
    """rfft of the zero-extended frames of the signals in the flat buffer `buf`, in double, rounded to fp32; defect: the
    extension as mask * x_clamped -- the clamped address stays inside the buffer, not inside the signal"""
    e = np.arange(frames)[:, None] * hop - lead + np.arange(n)[None, :]
    inside = (e >= 0) & (e < in_length)
    out = np.empty((ns, frames, n // 2 + 1), dtype=np.complex64)
    for i in range(ns):
        pos = np.clip(i * in_pitch + e, 0, buf.size - 1)
        if defect:
            frame = inside.astype(np.float64) * buf[pos].astype(np.float64)
        else:
            frame = np.where(inside, buf[np.where(inside, pos, 0)].astype(np.float64), 0.0)
        out[i] = np.fft.rfft(frame, axis=-1)
    return out


def _periodogram_model(buf, ns, in_pitch, in_length, n, hop, frames, avg, defect):
    """sums of avg consecutive |rfft|^2 of the signals' frames (lead 0, the signals hold every live frame); the last row
    is ragged.  defect: its dead frames are computed from whatever follows the signal and added as 0 * |X|^2"""
    n_rows = -(-frames // avg)
    out = np.zeros((ns, n_rows, n // 2 + 1))
    for i in range(ns):
        for f in range(n_rows * avg):
            live = f < frames
            if not live and not defect:
                continue
            pos = np.clip(i * in_pitch + f * hop + np.arange(n), 0, buf.size - 1)
            out[i, f // avg] += (1.0 if live else 0.0) * np.abs(np.fft.rfft(buf[pos].astype(np.float64))) ** 2
    return out.astype(np.float32)


def _rows_model(buf, out_before, batch, n, pitch, defect):
    """forward DFT of `batch` rows of n elements `pitch` apart, written into a copy of out_before at the same pitch.
    defects: "rmw" forms the output as 0 * out_before + result; "gap" transforms the whole pitch of a row with a matrix
    whose gap columns are 0; "cleans" runs nan_to_num over its input"""
    out = out_before.copy()
    for b in range(batch):
        row = buf[b * pitch:b * pitch + n].astype(np.complex128)
        if defect == "cleans":
            row = np.nan_to_num(row)
        if defect == "gap":
            w = np.zeros((n, pitch), dtype=np.complex128)
            w[:, :n] = np.exp(-2j * np.pi * np.outer(np.arange(n), np.arange(n)) / n)
            with np.errstate(invalid="ignore"):
                y = w @ buf[b * pitch:(b + 1) * pitch].astype(np.complex128)
        else:
            y = np.fft.fft(row)
        if defect == "rmw":
            y = 0 * out[b * pitch:b * pitch + n].astype(np.complex128) + y
        out[b * pitch:b * pitch + n] = y.astype(np.complex64)
    return out


def _passes_the_old_yardsticks(got, ref, n):
    ref = np.asarray(ref).astype(np.complex128)
    for g, r in zip(np.asarray(got).reshape(len(ref), -1), ref.reshape(len(ref), -1)):
        assert H.rel_l2(g, r) <= H.REL_L2_TOL[np.dtype(np.complex64)]
    assert H.check_reference_rule(np.asarray(got).ravel(), ref.ravel().astype(np.complex64), n)


def test_zero_extension_by_a_mask_passes_the_old_yardsticks_and_fails_the_isolation_check():
    from test_gpu_stft import _reference
    ns, n, hop, lead, length, frames = 3, 16, 5, 7, 37, 9
    in_pitch = 41
    x = np.random.default_rng(1).uniform(-1, 1, (ns, length)).astype(np.float32)
    ref = _reference(1.0, x, None, n, hop, lead, "zero", frames)
    everything = np.arange(ns * frames * (n // 2 + 1))
    for defect in (False, True):
        runs = []
        for pad in (H.PADDING_VALUE, H.POISON):
            buf = H.scatter(x, [1], in_pitch, 0, ns * in_pitch, pad=pad)
            with np.errstate(invalid="ignore"):
                runs.append(_stft_model(buf, ns, in_pitch, length, n, hop, lead, frames, defect).ravel())
        _passes_the_old_yardsticks(runs[0].reshape(ns, -1), ref.reshape(ns, -1), n)
        if not defect:
            H.check_isolated(runs[0], runs[1], everything, [], "stft model", H.frames_of(frames * 9, 9))
            continue
        # frame 6 covers samples 23 ... 38 of a signal of 37: the first that reaches into the pitch gap
        with pytest.raises(AssertionError, match=r"stft model: depends on a value it must not read: .* first at 54 "
                                                 r"\(signal 0, frame 6, bin 0\)"):
            H.check_isolated(runs[0], runs[1], everything, [], "stft model", H.frames_of(frames * 9, 9))


def test_a_dead_frame_times_zero_passes_the_old_yardsticks_and_fails_the_isolation_check():
    from test_gpu_stft import _reference
    ns, n, hop, frames, avg = 3, 16, 5, 7, 3
    length = (frames - 1) * hop + n
    in_pitch = length + 3
    x = np.random.default_rng(2).uniform(-1, 1, (ns, length)).astype(np.float32)
    power = np.abs(_reference(1.0, x, None, n, hop, 0, "zero", frames)) ** 2
    ref = np.concatenate([power, np.zeros((ns, 2, n // 2 + 1))], axis=1).reshape(ns, 3, avg, -1).sum(axis=2)
    everything = np.arange(ns * 3 * (n // 2 + 1))
    for defect in (False, True):
        runs = []
        for pad in (H.PADDING_VALUE, H.POISON):
            buf = H.scatter(x, [1], in_pitch, 0, ns * in_pitch, pad=pad)
            runs.append(_periodogram_model(buf, ns, in_pitch, length, n, hop, frames, avg, defect).ravel())
        _passes_the_old_yardsticks(np.sqrt(runs[0]).reshape(ns, -1), np.sqrt(ref).reshape(ns, -1), n)
        if not defect:
            H.check_isolated(runs[0], runs[1], everything, [], "periodogram model", H.frames_of(27, 9, ("signal", "row", "bin")))
            continue
        with pytest.raises(AssertionError, match=r"periodogram model: depends on .* first at 18 \(signal 0, row 2, bin 0\)"):
            H.check_isolated(runs[0], runs[1], everything, [], "periodogram model", H.frames_of(27, 9, ("signal", "row", "bin")))


@pytest.mark.parametrize("defect", ["rmw", "gap"])
def test_a_read_of_the_output_or_of_the_gap_passes_the_old_yardsticks_and_fails_the_isolation_check(defect):
    batch, n, pitch = 4, 16, 21
    x, y = H.gen_fourier_data(batch, [n], np.complex64, seed=4)
    idx = H.element_indices(batch, [n], [1], pitch, 0).ravel()
    for planted in (None, defect):
        runs = []
        for pad in (H.PADDING_VALUE, H.POISON):
            buf = H.scatter(x, [1], pitch, 0, batch * pitch, pad=pad)
            out = _rows_model(buf, H.full(batch * pitch, pad, np.complex64), batch, n, pitch, planted)
            H.check_write_set(out, idx, pad=pad)  # (the write set is right in both runs)
            runs.append(out)
        _passes_the_old_yardsticks(runs[0][idx].reshape(batch, n), y, n)
        if planted is None:
            H.check_isolated(runs[0], runs[1], idx, [], "rows model", H.rows_of(pitch))
            continue
        with pytest.raises(AssertionError, match=r"rows model: depends on a value it must not read: 64 untainted element\(s\) "
                                                 r"differ .* first at 0 \(row 0, element 0\)"):
            H.check_isolated(runs[0], runs[1], idx, [], "rows model", H.rows_of(pitch))


def test_a_model_that_cleans_its_input_fails_on_the_tainted_side():
    batch, n, pitch = 4, 16, 21
    x, y = H.gen_fourier_data(batch, [n], np.complex64, seed=5)
    rows = H.element_indices(batch, [n], [1], pitch, 0)
    poisoned = x.copy()
    H.poison_numpy(poisoned[2])
    for defect in (None, "cleans"):
        runs = []
        for data, pad in ((x, H.PADDING_VALUE), (poisoned, H.POISON)):
            buf = H.scatter(data, [1], pitch, 0, batch * pitch, pad=pad)
            runs.append(_rows_model(buf, H.full(batch * pitch, pad, np.complex64), batch, n, pitch, defect))
        _passes_the_old_yardsticks(runs[0][rows.ravel()].reshape(batch, n), y, n)
        untainted, tainted = rows[[0, 1, 3]].ravel(), rows[2]
        if defect is None:
            H.check_isolated(runs[0], runs[1], untainted, tainted, "rows model", H.rows_of(pitch), every_scalar=True)
            continue
        with pytest.raises(AssertionError, match=r"rows model: drops a value it must propagate: 16 tainted element\(s\) are "
                                                 r"finite in the poisoned run, first at 42 \(row 2, element 0\)"):
            H.check_isolated(runs[0], runs[1], untainted, tainted, "rows model", H.rows_of(pitch))


def test_isolation_check_reads_split_planes_and_one_finite_component():
    clean = (np.arange(6, dtype=np.float32), np.arange(6, dtype=np.float32))
    poisoned = (clean[0].copy(), clean[1].copy())
    H.poison_numpy(poisoned[0], [4])
    H.check_isolated(clean, poisoned, [0, 1, 2, 3, 5], [4], "split")  # one component is enough ...
    with pytest.raises(AssertionError, match="split: drops a value it must propagate: 1 tainted .* first at 4"):
        H.check_isolated(clean, poisoned, [0, 1, 2, 3, 5], [4], "split", every_scalar=True)  # ... unless both are asked for
    poisoned[1][1] = np.nextafter(np.float32(1), np.float32(2))
    with pytest.raises(AssertionError, match=r"split \(im plane\): depends on .* first at 1"):
        H.check_isolated(clean, poisoned, [0, 1, 2, 3, 5], [4], "split")


# ---------------------------------------------------------------------------------------------------------------------
# odd-radix configurations: defects that only exist where M = N / 2 is odd or the first radix brings no LDS padding

def _r2c_model(x, pads, defect=None):
    """R2C of the rows of x (N = 2M scalars) the way the fused real kernels do it, in double, rounded to fp32: the pairs
    z[p] = x[2p] + i x[2p + 1] are stored into the LDS image at slot p + p // 16 when the configuration pads (`pads`: the
    planner pads only behind a first radix of 8, 16 or 32) and at slot p when it does not; the first pass reads them back;
    Z = DFT_M(z); item 0 gives bins 0 and M, item k = 1 ... (M - 1) / 2 the bins k and M - k, and an even M has the item
    2k = M on top.  Defects, both invisible at every even M with a padded image:
      "middle"   the items run over k < M / 2 in integers and the 2k = M item follows -- right for an even M; an odd M
                 loses its middle item k = (M - 1) / 2, whose bins keep what the output held (zero here)
      "padding"  the first pass reads slot p + p // 16 whatever the configuration stored"""
    x = np.asarray(x, dtype=np.float64)
    rows, n = x.shape
    m = n // 2
    image = np.zeros((rows, m + m // 16 + 1), dtype=np.complex128)
    p = np.arange(m)
    image[:, p + (p // 16 if pads else 0)] = x[:, 0::2] + 1j * x[:, 1::2]
    zz = np.fft.fft(image[:, p + (p // 16 if pads or defect == "padding" else 0)], axis=1)
    out = np.zeros((rows, m + 1), dtype=np.complex128)
    out[:, 0] = zz[:, 0].real + zz[:, 0].imag
    out[:, m] = zz[:, 0].real - zz[:, 0].imag
    items = list(range(1, m // 2 if defect == "middle" else (m + 1) // 2))
    for k in items:
        a, b = zz[:, k], np.conj(zz[:, m - k])
        t = (a - b) * np.exp(-2j * np.pi * k / n)
        out[:, k] = 0.5 * ((a + b) - 1j * t)
        out[:, m - k] = np.conj(0.5 * ((a + b) + 1j * t))
    if m % 2 == 0:
        out[:, m // 2] = np.conj(zz[:, m // 2])
    return out.astype(np.complex64)


@pytest.mark.parametrize("defect", ["middle", "padding"])
def test_a_lost_middle_item_and_a_padding_that_is_not_there_pass_the_old_shapes_and_fail_the_odd_radix_ones(defect):
    """the suite's shapes before test_gpu_odd_radix.py -- an even M behind a padded image, N = 2048 as 16 x 8 x 8 -- give the
    defective model a large random batch and all impulses and see nothing; the table's shapes (helpers.ODD_RADIX_LENGTHS:
    M = 27 as 9 x 3, M = 1001 as 13 x 11 x 7, no padding, odd M) fail it on random rows and on impulses, the basis check
    naming the row and the element"""
    tol = H.REL_L2_TOL[np.dtype(np.complex64)]

    def yardsticks(n, pads, which, rows=64):
        x = np.random.default_rng(n).uniform(-1, 1, (rows, n)).astype(np.float32)
        ref = np.fft.rfft(x.astype(np.float64), axis=1)
        got = _r2c_model(x, pads, which).astype(np.complex128)
        err = np.linalg.norm(got - ref, axis=1) / np.linalg.norm(ref, axis=1)
        return float(err.max()) <= tol and H.check_reference_rule(got, ref.astype(np.complex64), n)

    assert yardsticks(2048, True, None, 512) and yardsticks(2048, True, defect, 512)  # a large batch at an old shape
    eye = np.eye(2048)
    assert H.check_basis_rows(_r2c_model(eye, True, defect), np.arange(2048), 2048, "r2c", "f32", what="old shape") < 0.2
    table = dict(H.ODD_RADIX_LENGTHS["f32"])
    for m in (27, 1001):
        n = 2 * m
        assert m in table and m % 2 == 1 and m >= 16
        assert yardsticks(n, False, None)
        assert H.check_basis_rows(_r2c_model(np.eye(n), False), np.arange(n), n, "r2c", "f32", what="clean") < 0.2
        assert not yardsticks(n, False, defect), (defect, n, "rel-L2 and the per-element rule on random rows")
        with pytest.raises(AssertionError, match=r"r2c f32 n=%d: the transform of e_\d+, element \d+: .* of the bound" % n) as e:
            H.check_basis_rows(_r2c_model(np.eye(n), False, defect), np.arange(n), n, "r2c", "f32", what="planted " + defect)
        if defect == "middle":  # every impulse loses the same bin, the middle item's k = (M - 1) / 2
            assert int(re.search(r"element (\d+)", str(e.value)).group(1)) == (m - 1) // 2
