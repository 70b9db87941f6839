"""Overlap-save filtering (set_filter_taps / filter of a plan with PFFT_EXT_CONVOLUTION) on the host side: the three new
symbols of the C ABI and their binding, what they answer on no plan, and the argument errors the Python verbs raise
before the library is called."""
import ctypes as C
import shutil
import subprocess

import pytest

import portfft_amd as pf
from portfft_amd import _lib

NEW = ("pfft_plan_set_filter_taps", "pfft_execute_filter", "pfft_execute_filter_ex")


def test_the_library_exports_the_three_new_symbols():
    nm = shutil.which("nm") or "/usr/bin/nm"
    out = subprocess.run([nm, "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for sym in NEW:
        assert sym in names, sym
        assert sym in _lib.SYMBOLS
    u64, vp = C.c_uint64, C.c_void_p
    assert _lib.SYMBOLS["pfft_plan_set_filter_taps"] == (C.c_int, [vp, vp, u64, u64])
    assert _lib.SYMBOLS["pfft_execute_filter"] == (C.c_int, [vp, C.c_int32, vp, vp, u64, u64, u64, u64, u64])
    assert _lib.SYMBOLS["pfft_execute_filter_ex"][1][:9] == _lib.SYMBOLS["pfft_execute_filter"][1]
    assert len(_lib.SYMBOLS["pfft_execute_filter_ex"][1]) == 12


def test_the_verbs_refuse_no_plan():
    lib = _lib.lib
    assert lib.pfft_plan_set_filter_taps(None, None, 1, 1) == 1  # PFFT_INVALID_CONFIGURATION
    assert b"null plan" in lib.pfft_last_error()
    assert lib.pfft_execute_filter(None, _lib.CONVOLVE, None, None, 1, 1, 1, 1, 1) == 1
    ev = C.c_void_p()
    assert lib.pfft_execute_filter_ex(None, _lib.CORRELATE, None, None, 1, 1, 1, 1, 1, 0, None, C.byref(ev)) == 1
    assert not ev.value


def _shell(conv, scalar="f32"):
    """a committed_descriptor without a plan (no GPU here): what the verbs check before they call the library"""
    import torch
    p = object.__new__(pf.committed_descriptor)
    p._plan = None
    p._conv = conv
    p._torch = torch
    p._device = None
    p._scalar = scalar
    p._real_dtype, p._cplx_dtype = (torch.float32, torch.complex64) if scalar == "f32" else (torch.float64, torch.complex128)
    p.params = pf.convolution_descriptor([64], scalar)
    return p, torch


def test_the_verbs_belong_to_a_convolution_descriptor():
    p, torch = _shell(False)
    t = torch.zeros(2, 9, dtype=torch.complex64)
    with pytest.raises(pf.invalid_configuration, match="not a convolution_descriptor"):
        p.set_filter_taps(t)
    with pytest.raises(pf.invalid_configuration, match="not a convolution_descriptor"):
        p.filter(t, t.clone())


def test_taps_are_checked_before_the_library_is_called():
    p, torch = _shell(True)
    c64 = torch.complex64
    for bad, text in ((torch.zeros(2, 65, dtype=c64), "1 <= K <= 64"), (torch.zeros(2, 0, dtype=c64), "1 <= K <= 64"),
                      (torch.zeros(2, 3, 9, dtype=c64), "shape"), (torch.zeros(2, 9, dtype=torch.complex128), "dtype"),
                      (torch.zeros(2, 9), "dtype"), (torch.zeros(2, 9, dtype=c64).numpy(), "torch tensor"),
                      (torch.zeros(2, 9, dtype=c64), "not in device memory")):
        with pytest.raises(pf.invalid_configuration, match=text):
            p.set_filter_taps(bad)


def test_signals_are_checked_before_the_library_is_called():
    p, torch = _shell(True)
    c64 = torch.complex64
    x, y = torch.zeros(3, 200, dtype=c64), torch.zeros(3, 208, dtype=c64)
    for bx, by, text in ((x.to(torch.complex128), y, "dtype"), (x, y.real.contiguous(), "dtype"),
                         (x[:2], y, "3 output signals"), (x, y[:, ::2], "unit inner stride"),
                         (x.reshape(3, 2, 100), y, "1-D or 2-D"), (x[:, :0], y, "not empty"), (x.numpy(), y, "torch tensors"),
                         (x, y, "not in device memory")):
        with pytest.raises(pf.invalid_configuration, match=text):
            p.filter(bx, by)
    overlapping = torch.zeros(500, dtype=c64).as_strided((3, 200), (100, 1))
    with pytest.raises(pf.invalid_configuration, match="signals of the in tensor overlap"):
        p.filter(overlapping, y)
