"""DCT-IV and MDCT (prepare_dct4 / dct4 / set_mdct_window / mdct of a plan of the REAL domain) on the host side: the six
new verbs of the C ABI and their binding, what they answer on no plan, that no extension bit was added, and the argument
errors the Python verbs raise before the library is called -- each names the offending quantity."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

import portfft_amd as pf
from portfft_amd import _lib

NEW = ("pfft_plan_prepare_dct4", "pfft_execute_dct4", "pfft_execute_dct4_ex", "pfft_plan_set_mdct_window",
       "pfft_execute_mdct", "pfft_execute_mdct_ex")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_library_exports_the_six_new_symbols():
    nm = shutil.which("nm") or "/usr/bin/nm"
    out = subprocess.run([nm, "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    # (names with a digit are bound from _lib.SYMBOLS_NUMBERED: test_host_api.py reads the header's names as [a-z_]+)
    bound = dict(_lib.SYMBOLS, **_lib.SYMBOLS_NUMBERED)
    for sym in NEW:
        assert sym in names, sym
        assert sym in bound
        assert getattr(_lib.lib, sym).argtypes == bound[sym][1]
    u64, vp = C.c_uint64, C.c_void_p
    assert bound["pfft_plan_prepare_dct4"] == (C.c_int, [vp])
    assert bound["pfft_execute_dct4"] == (C.c_int, [vp, C.c_int32, vp, vp, u64, u64, u64])
    assert bound["pfft_execute_dct4_ex"][1][:7] == bound["pfft_execute_dct4"][1]
    assert bound["pfft_execute_dct4_ex"][1][7:] == [C.c_int32, C.POINTER(vp), C.POINTER(vp)]
    assert _lib.SYMBOLS["pfft_plan_set_mdct_window"] == (C.c_int, [vp, vp])
    assert _lib.SYMBOLS["pfft_execute_mdct"] == (C.c_int, [vp, vp, vp] + [u64] * 7)
    assert _lib.SYMBOLS["pfft_execute_mdct_ex"][1][:10] == _lib.SYMBOLS["pfft_execute_mdct"][1]
    assert _lib.SYMBOLS["pfft_execute_mdct_ex"][1][10:] == [C.c_int32, C.POINTER(vp), C.POINTER(vp)]


def test_the_header_declares_them():
    text = open(os.path.join(ROOT, "include", "portfft_amd.h")).read()
    for sym in NEW:
        assert re.search(r"pfft_status %s\(" % sym, text), sym
    assert re.search(r"pfft_plan_prepare_dct4\(pfft_plan_t\* plan\);", text)
    assert re.search(r"pfft_execute_dct4\(pfft_plan_t\* plan, int32_t inverse, const void\* in, void\* out, uint64_t n_rows,\s+"
                     r"uint64_t in_pitch, uint64_t out_pitch\);", text)
    assert re.search(r"pfft_plan_set_mdct_window\(pfft_plan_t\* plan, const void\* window\);", text)
    # the argument order of the issue: in, out, n_signals, in_length, in_pitch, lead, n_frames, frame_pitch, out_pitch
    assert re.search(r"pfft_execute_mdct\(pfft_plan_t\* plan, const void\* in, void\* out, uint64_t n_signals, uint64_t in_length,\s+"
                     r"uint64_t in_pitch, uint64_t lead, uint64_t n_frames, uint64_t frame_pitch,\s+uint64_t out_pitch\);", text)
    block = text[text.index("Discrete cosine transform of type 4"):text.index("pfft_plan_prepare_dct4(pfft_plan_t")]
    for word in ("4 GiB", "2N * x", "lead", "In place", "Not in place"):
        assert word in block, word


def test_the_verbs_refuse_no_plan():
    lib = _lib.lib
    assert lib.pfft_plan_prepare_dct4(None) == 1  # PFFT_INVALID_CONFIGURATION
    assert b"null plan" in lib.pfft_last_error()
    assert lib.pfft_execute_dct4(None, 0, None, None, 1, 64, 64) == 1
    assert b"null plan" in lib.pfft_last_error()
    ev = C.c_void_p()
    assert lib.pfft_execute_dct4_ex(None, 1, None, None, 1, 64, 64, 0, None, C.byref(ev)) == 1
    assert b"null plan" in lib.pfft_last_error()
    assert not ev.value
    assert lib.pfft_plan_set_mdct_window(None, None) == 1
    assert b"null plan" in lib.pfft_last_error()
    assert lib.pfft_execute_mdct(None, None, None, 1, 192, 192, 64, 4, 64, 256) == 1
    assert b"null plan" in lib.pfft_last_error()
    assert lib.pfft_execute_mdct_ex(None, None, None, 1, 192, 192, 64, 4, 64, 256, 0, None, C.byref(ev)) == 1
    assert b"null plan" in lib.pfft_last_error()
    assert not ev.value


def test_no_extension_bit_was_added():
    assert pf.real_descriptor(64)._c().extensions == 1 and pf.real_convolution_descriptor(64)._c().extensions == 16
    c = pf.real_descriptor(64)._c()
    for bits in (4, 32, 64, 1 | 32):
        c.extensions = bits
        assert _lib.lib.pfft_desc_validate(C.byref(c)) == 1
        assert b"extension" in _lib.lib.pfft_last_error()


def test_dct_type_4_stays_refused():
    """DCT-IV has verbs of its own: plan.dct keeps its two types"""
    p, torch = _shell(True)
    with pytest.raises(pf.invalid_configuration, match="type 4"):
        p.dct(torch.zeros(3, 64), torch.zeros(3, 64), type=4)


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
    for call in (p.prepare_dct4, lambda: p.dct4(torch.zeros(3, 64), torch.zeros(3, 64)), lambda: p.set_mdct_window(None),
                 lambda: p.mdct(torch.zeros(192), torch.zeros(4, 64))):
        with pytest.raises(pf.invalid_configuration, match="not of the REAL domain"):
            call()


def test_dct4_rows_are_checked_before_the_library_is_called():
    p, torch = _shell(True)
    x, y = torch.zeros(3, 64), torch.zeros(3, 64)
    cases = (
        (dict(x=x.double()), "dtype .* in tensor"), (dict(y=y.double()), "dtype .* out tensor"),
        (dict(x=torch.zeros(3, 64, dtype=torch.complex64)), "dtype .* in tensor"),
        (dict(x=torch.zeros(3, 63)), "last dimension of the in tensor is 63"),
        (dict(y=torch.zeros(3, 66)), "last dimension of the out tensor is 66"),
        (dict(y=y[:2]), "3 input rows but 2 output rows"), (dict(x=x[0]), "1 input rows but 3 output rows"),
        (dict(x=torch.zeros(3, 128)[:, ::2]), "in tensor needs unit inner stride"),
        (dict(y=torch.zeros(3, 128)[:, ::2]), "out tensor needs unit inner stride"),
        (dict(x=x.reshape(3, 2, 32)), "1-D or 2-D"), (dict(y=y[:0]), "not empty"), (dict(x=x.numpy()), "torch tensors"),
        (dict(x=torch.zeros(200).as_strided((3, 64), (60, 1))), "rows of the in tensor overlap"),
        (dict(y=torch.zeros(200).as_strided((3, 64), (63, 1))), "rows of the out tensor overlap"),
        (dict(), "in tensor is not in device memory"),
    )
    for change, text in cases:
        kw = dict(x=x, y=y)
        kw.update(change)
        for inverse in (False, True):
            with pytest.raises(pf.invalid_configuration, match=text):
                p.dct4(kw["x"], kw["y"], inverse=inverse)
    wide = torch.zeros(3, 67)
    for kw in (dict(x=x, y=y), dict(x=x[0], y=y[0]), dict(x=x, y=x), dict(x=wide[:, :64], y=y), dict(x=x, y=wide[:, :64])):
        with pytest.raises(pf.invalid_configuration, match="not in device memory"):
            p.dct4(kw["x"], kw["y"])
    p64, _ = _shell(True, "f64", 128)
    with pytest.raises(pf.invalid_configuration, match="dtype .* in tensor"):
        p64.dct4(torch.zeros(2, 128), torch.zeros(2, 128, dtype=torch.float64))
    with pytest.raises(pf.invalid_configuration, match="not in device memory"):
        p64.dct4(torch.zeros(2, 128, dtype=torch.float64), torch.zeros(2, 128, dtype=torch.float64))


def test_the_mdct_window_is_2n_scalars_of_the_real_type():
    p, torch = _shell(True)
    for w, text in ((torch.zeros(64), r"shape \(128,\) is needed"), (torch.zeros(2, 64), r"shape \(128,\) is needed"),
                    (torch.zeros(128, dtype=torch.float64), "dtype"), ([0.0] * 128, "torch tensor")):
        with pytest.raises(pf.invalid_configuration, match=text):
            p.set_mdct_window(w)


def test_mdct_signals_and_frames_are_checked_before_the_library_is_called():
    p, torch = _shell(True)
    n = 64
    x, y = torch.zeros(3, 200), torch.zeros(3, 4, n)
    cases = (
        (dict(x=x.double()), "dtype .* in tensor"), (dict(y=y.double()), "dtype .* out tensor"),
        (dict(y=torch.zeros(3, 4, n, dtype=torch.complex64)), "dtype .* out tensor"),
        (dict(y=torch.zeros(3, 4, n + 1)), "last dimension of the out tensor is 65"),
        (dict(y=torch.zeros(3, 4, n // 2 + 1)), "last dimension of the out tensor is 33"),
        (dict(y=y[:2]), "3 input signals but 2 output signals"), (dict(x=x[0]), "out tensor must be 2-D"),
        (dict(y=y[0]), "out tensor must be 3-D"), (dict(x=x.reshape(3, 2, 100)), "1-D or 2-D"), (dict(y=y[:, :0]), "not empty"),
        (dict(x=torch.zeros(3, 400)[:, ::2]), "in tensor needs unit inner stride"),
        (dict(y=torch.zeros(3, 4, 2 * n)[:, :, ::2]), "out tensor needs unit inner stride"),
        (dict(x=torch.zeros(600).as_strided((3, 200), (190, 1))), "signals of the in tensor overlap"),
        (dict(y=torch.zeros(800).as_strided((3, 4, n), (256, 60, 1))), "frames of the out tensor overlap"),
        (dict(y=torch.zeros(800).as_strided((3, 4, n), (250, 64, 1))), "signals of the out tensor overlap"),
        (dict(lead=-1), "lead -1"), (dict(lead=2 * n), r"lead 128, must be in \[0, 128\)"),
        (dict(y=torch.zeros(3, 6, n)), "frame 5 starts at sample 320 - lead 64, beyond the in_length 200"),
        (dict(lead=0, y=torch.zeros(3, 5, n)), "frame 4 starts at sample 256 - lead 0"),
        (dict(x=x.numpy()), "torch tensors"),
        (dict(), "in tensor is not in device memory"),
    )
    for change, text in cases:
        kw = dict(x=x, y=y, lead=None)
        kw.update(change)
        with pytest.raises(pf.invalid_configuration, match=text):
            p.mdct(kw["x"], kw["y"], lead=kw["lead"])
    # accepted shapes get as far as the device check: lead None is N (five frames of 200 samples need it), 0 and 2N - 1
    for kw in (dict(x=x, y=torch.zeros(3, 5, n)), dict(x=x, y=y, lead=0), dict(x=x, y=y, lead=2 * n - 1), dict(x=x[0], y=y[0]),
               dict(x=x, y=torch.zeros(3, 4, n + 3)[:, :, :n]), dict(x=torch.zeros(3, 203)[:, :200], y=y)):
        with pytest.raises(pf.invalid_configuration, match="not in device memory"):
            p.mdct(kw["x"], kw["y"], lead=kw.get("lead"))
