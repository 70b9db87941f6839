"""Inverse MDCT (set_imdct_window / imdct_chunk_frames / imdct of a plan of the REAL domain) on the host side: the four new
verbs of the C ABI and their binding, what they answer on no plan, that no extension bit was added, and the argument
errors the Python verbs raise before the library is called -- each names the offending quantity."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

import portfft_amd as pf
from portfft_amd import _lib

NEW = ("pfft_plan_set_imdct_window", "pfft_plan_imdct_chunk_frames", "pfft_execute_imdct", "pfft_execute_imdct_ex")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_library_exports_the_four_new_symbols():
    nm = shutil.which("nm") or "/usr/bin/nm"
    out = subprocess.run([nm, "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for sym in NEW:
        assert sym in names, sym
        assert sym in _lib.SYMBOLS  # (no digit in the names: the header regex of test_host_api.py finds them)
        assert getattr(_lib.lib, sym).argtypes == _lib.SYMBOLS[sym][1]
    u64, vp = C.c_uint64, C.c_void_p
    assert _lib.SYMBOLS["pfft_plan_set_imdct_window"] == (C.c_int, [vp, vp])
    assert _lib.SYMBOLS["pfft_plan_imdct_chunk_frames"] == (C.c_int, [vp, u64, u64, C.POINTER(u64)])
    assert _lib.SYMBOLS["pfft_execute_imdct"] == (C.c_int, [vp, vp, vp] + [u64] * 8)
    assert _lib.SYMBOLS["pfft_execute_imdct_ex"][1][:11] == _lib.SYMBOLS["pfft_execute_imdct"][1]
    assert _lib.SYMBOLS["pfft_execute_imdct_ex"][1][11:] == [C.c_int32, C.POINTER(vp), C.POINTER(vp)]


def test_the_header_declares_them():
    text = open(os.path.join(ROOT, "include", "portfft_amd.h")).read()
    for sym in NEW:
        assert re.search(r"pfft_status %s\(" % sym, text), sym
    assert re.search(r"pfft_plan_set_imdct_window\(pfft_plan_t\* plan, const void\* window\);", text)
    assert re.search(r"pfft_plan_imdct_chunk_frames\(const pfft_plan_t\* plan, uint64_t n_signals, uint64_t n_frames,\s+"
                     r"uint64_t\* chunk_frames\);", text)
    # the argument order of the issue: in, out, n_signals, n_frames, frame_pitch, in_pitch, lead, out_length, out_pitch,
    # chunk_frames
    assert re.search(r"pfft_execute_imdct\(pfft_plan_t\* plan, const void\* in, void\* out, uint64_t n_signals, uint64_t n_frames,\s+"
                     r"uint64_t frame_pitch, uint64_t in_pitch, uint64_t lead, uint64_t out_length,\s+uint64_t out_pitch, "
                     r"uint64_t chunk_frames\);", text)
    block = text[text.index("Inverse modified discrete cosine transform"):text.index("pfft_plan_set_imdct_window(pfft_plan_t")]
    for word in ("4 GiB", "ascending f", "lead", "Not in place", "chunk_frames", "bit for bit", "no extension bit"):
        assert word in block, word
    assert "A fused inverse MDCT is not offered" not in text


def test_the_verbs_refuse_no_plan():
    lib = _lib.lib
    assert lib.pfft_plan_set_imdct_window(None, None) == 1  # PFFT_INVALID_CONFIGURATION
    assert b"null plan" in lib.pfft_last_error()
    chunk = C.c_uint64(7)
    assert lib.pfft_plan_imdct_chunk_frames(None, 2, 8, C.byref(chunk)) == 1
    assert b"null argument" in lib.pfft_last_error() and chunk.value == 7
    assert lib.pfft_execute_imdct(None, None, None, 1, 4, 64, 256, 64, 256, 256, 0) == 1
    assert b"null plan" in lib.pfft_last_error()
    ev = C.c_void_p()
    assert lib.pfft_execute_imdct_ex(None, None, None, 1, 4, 64, 256, 64, 256, 256, 0, 0, None, C.byref(ev)) == 1
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
    for call in (lambda: p.set_imdct_window(None), lambda: p.imdct_chunk_frames(2, 8),
                 lambda: p.imdct(torch.zeros(4, 64), torch.zeros(192))):
        with pytest.raises(pf.invalid_configuration, match="not of the REAL domain"):
            call()


def test_the_imdct_window_is_2n_scalars_of_the_real_type():
    p, torch = _shell(True)
    for w, text in ((torch.zeros(64), r"shape \(128,\) is needed"), (torch.zeros(2, 64), r"shape \(128,\) is needed"),
                    (torch.zeros(128, dtype=torch.float64), "dtype"), ([0.0] * 128, "torch tensor")):
        with pytest.raises(pf.invalid_configuration, match=text):
            p.set_imdct_window(w)


def test_imdct_frames_and_signals_are_checked_before_the_library_is_called():
    p, torch = _shell(True)
    n = 64
    y, x = torch.zeros(3, 4, n), torch.zeros(3, 200)  # 4 frames at lead 64 cover 256 samples; frame 3 starts at 128
    cases = (
        (dict(y=y.double()), "dtype .* in tensor"), (dict(x=x.double()), "dtype .* out tensor"),
        (dict(y=torch.zeros(3, 4, n, dtype=torch.complex64)), "dtype .* in tensor"),
        (dict(y=torch.zeros(3, 4, n + 1)), "last dimension of the in tensor is 65"),
        (dict(y=torch.zeros(3, 4, n // 2 + 1)), "last dimension of the in tensor is 33"),
        (dict(y=y[:2]), "2 input signals but 3 output signals"), (dict(x=x[0]), "in tensor must be 2-D"),
        (dict(y=y[0]), "in tensor must be 3-D"), (dict(x=x.reshape(3, 2, 100)), "1-D or 2-D"), (dict(y=y[:, :0]), "not empty"),
        (dict(x=x[:, :0]), "not empty"),
        (dict(x=torch.zeros(3, 400)[:, ::2]), "out tensor needs unit inner stride"),
        (dict(y=torch.zeros(3, 4, 2 * n)[:, :, ::2]), "in tensor needs unit inner stride"),
        (dict(x=torch.zeros(600).as_strided((3, 200), (190, 1))), "signals of the out tensor overlap"),
        (dict(y=torch.zeros(800).as_strided((3, 4, n), (256, 60, 1))), "frames of the in tensor overlap"),
        (dict(y=torch.zeros(800).as_strided((3, 4, n), (250, 64, 1))), "signals of the in tensor overlap"),
        (dict(lead=-1), "lead -1"), (dict(lead=2 * n), r"lead 128, must be in \[0, 128\)"),
        (dict(chunk_frames=-1), "chunk_frames -1"),
        (dict(x=torch.zeros(3, 257)), r"out_length 257 above \(n_frames - 1\) \* N \+ 2N - lead = 256"),
        (dict(lead=0, x=torch.zeros(3, 321)), "out_length 321 above .* = 320"),
        (dict(y=torch.zeros(3, 6, n)), "frame 5 starts at sample 320 - lead 64, beyond the out_length 200"),
        (dict(lead=0, y=torch.zeros(3, 5, n)), "frame 4 starts at sample 256 - lead 0"),
        (dict(x=x.numpy()), "torch tensors"),
        (dict(), "in tensor is not in device memory"),
    )
    for change, text in cases:
        kw = dict(x=x, y=y, lead=None, chunk_frames=0)
        kw.update(change)
        with pytest.raises(pf.invalid_configuration, match=text):
            p.imdct(kw["y"], kw["x"], lead=kw["lead"], chunk_frames=kw["chunk_frames"])
    # accepted shapes get as far as the device check: lead None is N, 0 and 2N - 1, a chunk, pitched tensors, one signal
    for kw in (dict(y=torch.zeros(3, 5, n)), dict(lead=0), dict(lead=2 * n - 1, x=torch.zeros(3, 100)), dict(chunk_frames=3),
               dict(x=x[0], y=y[0]), dict(y=torch.zeros(3, 4, n + 3)[:, :, :n]), dict(x=torch.zeros(3, 203)[:, :200]),
               dict(x=torch.zeros(3, 256))):
        full = dict(x=x, y=y, lead=None, chunk_frames=0)
        full.update(kw)
        with pytest.raises(pf.invalid_configuration, match="not in device memory"):
            p.imdct(full["y"], full["x"], lead=full["lead"], chunk_frames=full["chunk_frames"])
    p64, _ = _shell(True, "f64", 128)
    with pytest.raises(pf.invalid_configuration, match="dtype .* in tensor"):
        p64.imdct(torch.zeros(2, 128), torch.zeros(256, dtype=torch.float64))
    with pytest.raises(pf.invalid_configuration, match="not in device memory"):
        p64.imdct(torch.zeros(2, 128, dtype=torch.float64), torch.zeros(256, dtype=torch.float64))
