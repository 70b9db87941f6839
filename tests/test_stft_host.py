"""Short-time Fourier transform (set_window / stft of a plan of the REAL domain) on the host side: the three new symbols
of the C ABI and their binding, what they answer on no plan, that no extension bit was added, and the argument errors
the Python verbs raise before the library is called -- each names the offending quantity."""
import ctypes as C
import shutil
import subprocess

import pytest

import portfft_amd as pf
from portfft_amd import _lib

NEW = ("pfft_plan_set_window", "pfft_execute_stft", "pfft_execute_stft_ex")


def test_the_library_exports_the_three_new_symbols():
    nm = shutil.which("nm") or "/usr/bin/nm"
    out = subprocess.run([nm, "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for sym in NEW:
        assert sym in names, sym
        assert sym in _lib.SYMBOLS
    u64, vp = C.c_uint64, C.c_void_p
    assert _lib.SYMBOLS["pfft_plan_set_window"] == (C.c_int, [vp, vp])
    assert _lib.SYMBOLS["pfft_execute_stft"] == (C.c_int, [vp, vp, vp, u64, u64, u64, u64, u64, C.c_int32, u64, u64, u64])
    assert _lib.SYMBOLS["pfft_execute_stft_ex"][1][:12] == _lib.SYMBOLS["pfft_execute_stft"][1]
    assert len(_lib.SYMBOLS["pfft_execute_stft_ex"][1]) == 15
    assert (_lib.PAD_ZERO, _lib.PAD_REFLECT) == (0, 1)


def test_the_verbs_refuse_no_plan():
    lib = _lib.lib
    assert lib.pfft_plan_set_window(None, None) == 1  # PFFT_INVALID_CONFIGURATION
    assert b"null plan" in lib.pfft_last_error()
    assert lib.pfft_execute_stft(None, None, None, 1, 1, 1, 1, 0, _lib.PAD_ZERO, 1, 1, 1) == 1
    assert b"null plan" in lib.pfft_last_error()
    ev = C.c_void_p()
    assert lib.pfft_execute_stft_ex(None, None, None, 1, 1, 1, 1, 0, _lib.PAD_REFLECT, 1, 1, 1, 0, None, C.byref(ev)) == 1
    assert not ev.value


def test_no_extension_bit_was_added():
    assert pf.real_descriptor(64)._c().extensions == 1 and pf.real_convolution_descriptor(64)._c().extensions == 16
    c = pf.real_descriptor(64)._c()
    for bits in (4, 32, 1 | 32):
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
        p.set_window(torch.zeros(64))
    with pytest.raises(pf.invalid_configuration, match="not of the REAL domain"):
        p.set_window(None)
    with pytest.raises(pf.invalid_configuration, match="not of the REAL domain"):
        p.stft(torch.zeros(2, 200), torch.zeros(2, 5, 33, dtype=torch.complex64), 16)


def test_the_window_is_checked_before_the_library_is_called():
    p, torch = _shell(True)
    for bad, text in ((torch.zeros(63), r"shape \(64,\)"), (torch.zeros(2, 64), r"shape \(64,\)"),
                      (torch.zeros(64, dtype=torch.float64), "dtype"), (torch.zeros(64, dtype=torch.complex64), "dtype"),
                      (torch.zeros(64).numpy(), "torch tensor"),
                      (torch.zeros(64), "not in device memory")):
        with pytest.raises(pf.invalid_configuration, match=text):
            p.set_window(bad)


def test_signals_and_geometry_are_checked_before_the_library_is_called():
    p, torch = _shell(True)
    c64 = torch.complex64
    x, y = torch.zeros(3, 200), torch.zeros(3, 5, 33, dtype=c64)
    cases = (
        (dict(x=x.double()), "dtype .* in tensor"), (dict(y=y.to(torch.complex128)), "dtype .* out tensor"),
        (dict(y=torch.zeros(3, 5, 33)), "dtype .* out tensor"),
        (dict(x=x[:2]), "2 input signals but 3 output signals"), (dict(x=x[:, ::2]), "in tensor needs unit inner stride"),
        (dict(y=torch.zeros(3, 5, 66, dtype=c64)[:, :, ::2]), "out tensor needs unit inner stride"),
        (dict(x=x.reshape(3, 2, 100)), "1-D or 2-D"), (dict(x=x[:, :0]), "not empty"), (dict(y=y[0]), "3-D"),
        (dict(x=x[0], y=y), "2-D"), (dict(y=y[:, :0]), "not empty"), (dict(x=x.numpy()), "torch tensors"),
        (dict(y=torch.zeros(3, 5, 32, dtype=c64)), "32 bins per frame"),
        (dict(hop=0), "hop 0"), (dict(lead=64), "lead 64"), (dict(lead=-1), "lead -1"), (dict(pad="edge"), "pad must be"),
        # zero: frame 4 must start in front of sample 200 + lead
        (dict(hop=50, lead=0), "frame 4 starts at sample 200"), (dict(hop=58, lead=32), "frame 4 starts at sample 232"),
        # reflect: lead at most in_length - 1, the last frame inside the padded signal
        (dict(x=torch.zeros(3, 20), y=y[:, :1], lead=20, pad="reflect"), "lead 20 above in_length - 1 = 19"),
        (dict(hop=51, lead=32, pad="reflect"), "frame 4 ends at sample 268"),
        (dict(hop=35, lead=0, pad="reflect"), "frame 4 ends at sample 204"),
        (dict(x=torch.zeros(600).as_strided((3, 200), (100, 1))), "signals of the in tensor overlap"),
        (dict(y=torch.zeros(600, dtype=c64).as_strided((3, 5, 33), (165, 20, 1))), "frames of the out tensor overlap"),
        (dict(y=torch.zeros(600, dtype=c64).as_strided((3, 5, 33), (100, 33, 1))), "signals of the out tensor overlap"),
        (dict(), "not in device memory"),
    )
    for change, text in cases:
        kw = dict(x=x, y=y, hop=16, lead=0, pad="zero")
        kw.update(change)
        with pytest.raises(pf.invalid_configuration, match=text):
            p.stft(kw["x"], kw["y"], kw["hop"], lead=kw["lead"], pad=kw["pad"])
    # the first accepted value of each geometry bound gets as far as the device check
    for kw in (dict(hop=49, lead=0), dict(hop=57, lead=32), dict(hop=50, lead=32, pad="reflect"), dict(hop=34, lead=0, pad="reflect")):
        with pytest.raises(pf.invalid_configuration, match="not in device memory"):
            p.stft(x, y, kw["hop"], lead=kw["lead"], pad=kw.get("pad", "zero"))
