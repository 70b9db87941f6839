"""Power spectrogram / periodogram (set_periodogram_window / periodogram of a plan of the REAL domain) on the host side: the
three new verbs of the C ABI and their binding, what they answer on no plan, that no extension bit was added, and the
argument errors the Python verbs raise before the library is called -- each names the offending quantity.  (The refusal of
a call without a window needs a plan and stands in test_gpu_periodogram.py.)"""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

import portfft_amd as pf
from portfft_amd import _lib

NEW = ("pfft_plan_set_periodogram_window", "pfft_execute_periodogram", "pfft_execute_periodogram_ex")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_library_exports_the_three_new_symbols():
    nm = shutil.which("nm") or "/usr/bin/nm"
    out = subprocess.run([nm, "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for sym in NEW:
        assert sym in names, sym
        assert sym in _lib.SYMBOLS
        assert getattr(_lib.lib, sym).argtypes == _lib.SYMBOLS[sym][1]
    u64, vp = C.c_uint64, C.c_void_p
    assert _lib.SYMBOLS["pfft_plan_set_periodogram_window"] == (C.c_int, [vp, vp])
    # the argument list of pfft_execute_stft with avg_frames in front of the two output pitches
    assert _lib.SYMBOLS["pfft_execute_periodogram"] == (C.c_int, [vp, vp, vp] + [u64] * 5 + [C.c_int32] + [u64] * 4)
    assert _lib.SYMBOLS["pfft_execute_periodogram"][1][:10] == _lib.SYMBOLS["pfft_execute_stft"][1][:10]
    assert _lib.SYMBOLS["pfft_execute_periodogram_ex"][1][:13] == _lib.SYMBOLS["pfft_execute_periodogram"][1]
    assert _lib.SYMBOLS["pfft_execute_periodogram_ex"][1][13:] == [C.c_int32, C.POINTER(vp), C.POINTER(vp)]


def test_the_header_declares_them():
    text = open(os.path.join(ROOT, "include", "portfft_amd.h")).read()
    for sym in NEW:
        assert re.search(r"pfft_status %s\(" % sym, text), sym
    assert re.search(r"pfft_plan_set_periodogram_window\(pfft_plan_t\* plan, const void\* window\);", text)
    # the argument order of the issue
    assert re.search(r"pfft_execute_periodogram\(pfft_plan_t\* plan, const void\* in, void\* out, uint64_t n_signals, "
                     r"uint64_t in_length,\s+uint64_t in_pitch, uint64_t hop, uint64_t lead, int32_t pad_mode, uint64_t "
                     r"n_frames,\s+uint64_t avg_frames, uint64_t row_pitch, uint64_t out_pitch\);", text)
    block = text[text.index("Power spectrogram and Welch periodogram"):text.index("pfft_plan_set_periodogram_window(pfft_plan_t")]
    for word in ("4 GiB", "ascending f", "SUM, not a mean", "not doubled", "Not in place", "avg_frames > n_frames", "bit for bit",
                 "no extension bit", "no atomics", "forward_scale"):
        assert word in block, word
    facade = open(os.path.join(ROOT, "include", "portfft", "portfft.hpp")).read()
    assert "void set_periodogram_window(const scalar_type* window)" in facade
    assert re.search(r"event periodogram\(const scalar_type\* in, scalar_type\* out,", facade)


def test_the_verbs_refuse_no_plan():
    lib = _lib.lib
    assert lib.pfft_plan_set_periodogram_window(None, None) == 1  # PFFT_INVALID_CONFIGURATION
    assert b"null plan" in lib.pfft_last_error()
    assert lib.pfft_execute_periodogram(None, None, None, 1, 256, 256, 16, 0, 0, 4, 2, 33, 66) == 1
    assert b"null plan" in lib.pfft_last_error()
    ev = C.c_void_p()
    assert lib.pfft_execute_periodogram_ex(None, None, None, 1, 256, 256, 16, 0, 0, 4, 2, 33, 66, 0, None, C.byref(ev)) == 1
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
    for call in (lambda: p.set_periodogram_window(None), lambda: p.periodogram(torch.zeros(300), torch.zeros(4, 33), 16, 4)):
        with pytest.raises(pf.invalid_configuration, match="not of the REAL domain"):
            call()


def test_the_periodogram_window_is_n_scalars_of_the_real_type():
    p, torch = _shell(True)
    for w, text in ((torch.zeros(128), r"shape \(64,\) is needed"), (torch.zeros(2, 32), r"shape \(64,\) is needed"),
                    (torch.zeros(64, dtype=torch.float64), "dtype"), ([0.0] * 64, "torch tensor")):
        with pytest.raises(pf.invalid_configuration, match=text):
            p.set_periodogram_window(w)


def test_periodogram_arguments_are_checked_before_the_library_is_called():
    p, torch = _shell(True)
    n, m1 = 64, 33
    # 3 signals of 300 samples, hop 16, 10 frames in rows of 3: R = 4
    x, out = torch.zeros(3, 300), torch.zeros(3, 4, m1)
    cases = (
        (dict(x=x.double()), "dtype .* in tensor"), (dict(out=out.double()), "dtype .* out tensor"),
        (dict(out=torch.zeros(3, 4, m1, dtype=torch.complex64)), "dtype torch.complex64 of the out tensor"),
        (dict(out=torch.zeros(3, 4, m1 + 1)), "holds 34 bins per row, a frame of 64 scalars has 33"),
        (dict(out=out[:2]), "3 input signals but 2 output signals"), (dict(x=x[0]), "out tensor must be 2-D"),
        (dict(out=out[0]), "out tensor must be 3-D"), (dict(x=x.reshape(3, 2, 150)), "1-D or 2-D"), (dict(x=x[:, :0]), "not empty"),
        (dict(out=out[:, :0]), "not empty"),
        (dict(x=torch.zeros(3, 600)[:, ::2]), "in tensor needs unit inner stride"),
        (dict(out=torch.zeros(3, 4, 2 * m1)[:, :, ::2]), "out tensor needs unit inner stride"),
        (dict(n_frames=0), "n_frames 0, must be at least 1"),
        (dict(frames_per_row=0), r"frames_per_row 0, must be in \[1, n_frames = 10\]"),
        (dict(frames_per_row=11), r"frames_per_row 11, must be in \[1, n_frames = 10\]"),
        (dict(frames_per_row=2), r"holds 4 rows, ceil\(n_frames 10 / frames_per_row 2\) is 5"),
        (dict(n_frames=13), r"holds 4 rows, ceil\(n_frames 13 / frames_per_row 3\) is 5"),
        (dict(frames_per_row=10), "holds 4 rows, .* is 1"),
        (dict(x=torch.zeros(900).as_strided((3, 300), (290, 1))), "signals of the in tensor overlap"),
        (dict(out=torch.zeros(600).as_strided((3, 4, m1), (140, 32, 1))), "rows of the out tensor overlap"),
        (dict(out=torch.zeros(600).as_strided((3, 4, m1), (130, 33, 1))), "signals of the out tensor overlap"),
        (dict(hop=0), "hop 0, must be at least 1"), (dict(lead=-1), "lead -1"), (dict(lead=n), r"lead 64, must be in \[0, 64\)"),
        (dict(pad="edge"), "pad must be"),
        (dict(hop=40), "frame 9 starts at sample 360 - lead 0, beyond the in_length 300"),
        (dict(pad="reflect", hop=30), "frame 9 ends at sample 334 - lead 0"),
        (dict(pad="reflect", lead=40, x=torch.zeros(3, 40), n_frames=1, frames_per_row=1, out=torch.zeros(3, 1, m1)),
         "lead 40 above in_length - 1 = 39"),
        (dict(x=x.numpy()), "torch tensors"),
        (dict(), "in tensor is not in device memory"),
    )
    for change, text in cases:
        kw = dict(x=x, out=out, hop=16, n_frames=10, frames_per_row=3, lead=0, pad="zero")
        kw.update(change)
        with pytest.raises(pf.invalid_configuration, match=text):
            p.periodogram(kw["x"], kw["out"], kw["hop"], kw["n_frames"], frames_per_row=kw["frames_per_row"], lead=kw["lead"],
                          pad=kw["pad"])
    # accepted shapes get as far as the device check: one row per signal, one frame per row, odd hop and lead, reflection,
    # pitched tensors, one signal
    for kw in (dict(frames_per_row=10, out=torch.zeros(3, 1, m1)), dict(frames_per_row=1, out=torch.zeros(3, 10, m1)),
               dict(hop=17, lead=n - 1), dict(pad="reflect", lead=32), dict(x=x[0], out=out[0]),
               dict(out=torch.zeros(3, 4, m1 + 3)[:, :, :m1]), dict(x=torch.zeros(3, 303)[:, :300]),
               dict(out=torch.zeros(3, 6, m1)[:, :4])):
        full = dict(x=x, out=out, hop=16, n_frames=10, frames_per_row=3, lead=0, pad="zero")
        full.update(kw)
        with pytest.raises(pf.invalid_configuration, match="not in device memory"):
            p.periodogram(full["x"], full["out"], full["hop"], full["n_frames"], frames_per_row=full["frames_per_row"],
                          lead=full["lead"], pad=full["pad"])
    p64, _ = _shell(True, "f64", 128)
    with pytest.raises(pf.invalid_configuration, match="dtype .* in tensor"):
        p64.periodogram(torch.zeros(300), torch.zeros(4, 65, dtype=torch.float64), 16, 4)
    with pytest.raises(pf.invalid_configuration, match="dtype .* out tensor"):
        p64.periodogram(torch.zeros(300, dtype=torch.float64), torch.zeros(4, 65), 16, 4)
    with pytest.raises(pf.invalid_configuration, match="not in device memory"):
        p64.periodogram(torch.zeros(300, dtype=torch.float64), torch.zeros(4, 65, dtype=torch.float64), 16, 4)
