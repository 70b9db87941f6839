"""Discrete cosine transforms (prepare_dct / dct of a plan of the REAL domain) on the host side: the three new verbs of the
C ABI and their binding, what they answer on no plan, the two type constants, that no extension bit was added, and the
argument errors the Python verbs raise before the library is called -- each names the offending quantity."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

import portfft_amd as pf
from portfft_amd import _lib

NEW = ("pfft_plan_prepare_dct", "pfft_execute_dct", "pfft_execute_dct_ex")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_library_exports_the_three_new_symbols():
    nm = shutil.which("nm") or "/usr/bin/nm"
    out = subprocess.run([nm, "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for sym in NEW:
        assert sym in names, sym
        assert sym in _lib.SYMBOLS
    u64, vp = C.c_uint64, C.c_void_p
    assert _lib.SYMBOLS["pfft_plan_prepare_dct"] == (C.c_int, [vp])
    assert _lib.SYMBOLS["pfft_execute_dct"] == (C.c_int, [vp, C.c_int32, vp, vp, u64, u64, u64])
    assert _lib.SYMBOLS["pfft_execute_dct_ex"][1][:7] == _lib.SYMBOLS["pfft_execute_dct"][1]
    assert _lib.SYMBOLS["pfft_execute_dct_ex"][1][7:] == [C.c_int32, C.POINTER(vp), C.POINTER(vp)]
    assert (_lib.DCT_II, _lib.DCT_III) == (2, 3)


def test_the_header_declares_them():
    text = open(os.path.join(ROOT, "include", "portfft_amd.h")).read()
    for sym in NEW:
        assert re.search(r"pfft_status %s\(" % sym, text), sym
    assert "PFFT_DCT_II = 2, PFFT_DCT_III = 3" in text
    assert re.search(r"pfft_plan_prepare_dct\(pfft_plan_t\* plan\);", text)
    # the argument order of the issue: plan, type, in, out, n_rows, in_pitch, out_pitch
    assert re.search(r"pfft_execute_dct\(pfft_plan_t\* plan, int32_t type, const void\* in, void\* out, uint64_t n_rows,\s+"
                     r"uint64_t in_pitch, uint64_t out_pitch\);", text)
    assert "4 GiB" in text[text.index("PFFT_DCT_II:"):text.index("pfft_plan_prepare_dct(")]


def test_the_verbs_refuse_no_plan():
    lib = _lib.lib
    assert lib.pfft_plan_prepare_dct(None) == 1  # PFFT_INVALID_CONFIGURATION
    assert b"null plan" in lib.pfft_last_error()
    assert lib.pfft_execute_dct(None, _lib.DCT_II, None, None, 1, 64, 64) == 1
    assert b"null plan" in lib.pfft_last_error()
    ev = C.c_void_p()
    assert lib.pfft_execute_dct_ex(None, _lib.DCT_III, None, None, 1, 64, 64, 0, None, C.byref(ev)) == 1
    assert b"null plan" in lib.pfft_last_error()
    assert not ev.value


def test_no_extension_bit_was_added():
    assert pf.real_descriptor(64)._c().extensions == 1 and pf.real_convolution_descriptor(64)._c().extensions == 16
    c = pf.real_descriptor(64)._c()
    for bits in (4, 32, 64, 1 | 32):
        c.extensions = bits
        assert _lib.lib.pfft_desc_validate(C.byref(c)) == 1
        assert b"extension" in _lib.lib.pfft_last_error()


def _shell(real, scalar="f32", n=64):
    """a committed_descriptor without a plan (no GPU here): what the verbs check before they call the library"""
    import torch
    p = object.__new__(pf.committed_descriptor)
    p._plan = None
    p._real = real
    p._torch = torch
    p._device = None
    p._scalar = scalar
    p._real_dtype, p._cplx_dtype = (torch.float32, torch.complex64) if scalar == "f32" else (torch.float64, torch.complex128)
    p.params = pf.real_descriptor(n, scalar) if real else pf.descriptor([n], scalar)
    return p, torch


def test_the_verbs_belong_to_a_real_plan():
    p, torch = _shell(False)
    with pytest.raises(pf.invalid_configuration, match="not of the REAL domain"):
        p.prepare_dct()
    with pytest.raises(pf.invalid_configuration, match="not of the REAL domain"):
        p.dct(torch.zeros(3, 64), torch.zeros(3, 64))


def test_rows_are_checked_before_the_library_is_called():
    p, torch = _shell(True)
    x, y = torch.zeros(3, 64), torch.zeros(3, 64)
    cases = (
        (dict(x=x.double()), "dtype .* in tensor"), (dict(y=y.double()), "dtype .* out tensor"),
        (dict(x=torch.zeros(3, 64, dtype=torch.complex64)), "dtype .* in tensor"),
        (dict(x=torch.zeros(3, 63)), "last dimension of the in tensor is 63"),
        (dict(y=torch.zeros(3, 66)), "last dimension of the out tensor is 66"),
        (dict(y=y[:2]), "3 input rows but 2 output rows"), (dict(x=x[0]), "1 input rows but 3 output rows"),
        (dict(type=4), "type 4"), (dict(type=1), "type 1"), (dict(type=0), "type 0"),
        (dict(x=torch.zeros(3, 128)[:, ::2]), "in tensor needs unit inner stride"),
        (dict(y=torch.zeros(3, 128)[:, ::2]), "out tensor needs unit inner stride"),
        (dict(x=x.reshape(3, 2, 32)), "1-D or 2-D"), (dict(y=y[:0]), "not empty"), (dict(x=x.numpy()), "torch tensors"),
        (dict(x=torch.zeros(200).as_strided((3, 64), (60, 1))), "rows of the in tensor overlap"),
        (dict(y=torch.zeros(200).as_strided((3, 64), (63, 1))), "rows of the out tensor overlap"),
        (dict(), "in tensor is not in device memory"),
    )
    for change, text in cases:
        kw = dict(x=x, y=y, type=2)
        kw.update(change)
        with pytest.raises(pf.invalid_configuration, match=text):
            p.dct(kw["x"], kw["y"], type=kw["type"])
    # the first accepted shape of each kind gets as far as the device check
    wide = torch.zeros(3, 67)
    for kw in (dict(x=x, y=y), dict(x=x, y=y, type=3), dict(x=x[0], y=y[0]), dict(x=x, y=x), dict(x=wide[:, :64], y=y),
               dict(x=x, y=wide[:, :64]), dict(x=torch.zeros(192).as_strided((3, 64), (64, 1)), y=y)):
        with pytest.raises(pf.invalid_configuration, match="not in device memory"):
            p.dct(kw["x"], kw["y"], type=kw.get("type", 2))
    p64, _ = _shell(True, "f64", 128)
    with pytest.raises(pf.invalid_configuration, match="dtype .* in tensor"):
        p64.dct(torch.zeros(2, 128), torch.zeros(2, 128, dtype=torch.float64))
    with pytest.raises(pf.invalid_configuration, match="not in device memory"):
        p64.dct(torch.zeros(2, 128, dtype=torch.float64), torch.zeros(2, 128, dtype=torch.float64))
