"""The checks of the GPU harness, on the CPU: each checker passes a correct output (NumPy) and fails the same output with
one planted defect, naming the element or transform.  (helpers.check_write_set / check_guards / check_unchanged behind
gpu_utils.run and transform_packed; helpers.check_every_transform behind the full-size, big-buffer and XCD-local tests.)"""
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
