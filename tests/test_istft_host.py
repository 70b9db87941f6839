"""Inverse short-time Fourier transform (set_synthesis_window / istft of a plan of the REAL domain) on the host side: the
three new verbs of the C ABI (and the chunk-length query next to them) and their binding, what they answer on no plan,
that no extension bit was added, and the argument errors the Python verbs raise before the library is called -- each
names the offending quantity."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

import portfft_amd as pf
from portfft_amd import _lib

NEW = ("pfft_plan_set_synthesis_window", "pfft_execute_istft", "pfft_execute_istft_ex")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_library_exports_the_three_new_symbols():
    nm = shutil.which("nm") or "/usr/bin/nm"
    out = subprocess.run([nm, "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for sym in NEW + ("pfft_plan_istft_chunk_frames",):
        assert sym in names, sym
        assert sym in _lib.SYMBOLS
    u64, vp = C.c_uint64, C.c_void_p
    assert _lib.SYMBOLS["pfft_plan_set_synthesis_window"] == (C.c_int, [vp, vp])
    assert _lib.SYMBOLS["pfft_execute_istft"] == (C.c_int, [vp, vp, vp, u64, u64, u64, u64, u64, u64, C.c_int32, u64, u64, u64])
    assert _lib.SYMBOLS["pfft_execute_istft_ex"][1][:13] == _lib.SYMBOLS["pfft_execute_istft"][1]
    assert len(_lib.SYMBOLS["pfft_execute_istft_ex"][1]) == 16
    assert _lib.SYMBOLS["pfft_plan_istft_chunk_frames"] == (C.c_int, [vp, u64, u64, u64, C.POINTER(u64)])
    assert (_lib.ISTFT_PLAIN, _lib.ISTFT_NORMALIZE) == (0, 1)


def test_the_header_declares_them_and_names_the_threshold():
    text = open(os.path.join(ROOT, "include", "portfft_amd.h")).read()
    for sym in NEW + ("pfft_plan_istft_chunk_frames",):
        assert re.search(r"pfft_status %s\(" % sym, text), sym
    assert "PFFT_ISTFT_PLAIN = 0, PFFT_ISTFT_NORMALIZE = 1" in text
    assert re.search(r"#define PFFT_ISTFT_ENV_MIN 1e-11\b", text)
    # the argument order of the issue: counts, pitches on the bin side, hop, lead, mode, the sample side, the chunk
    assert re.search(r"pfft_execute_istft\(pfft_plan_t\* plan, const void\* in, void\* out, uint64_t n_signals, uint64_t n_frames,\s+"
                     r"uint64_t frame_pitch, uint64_t in_pitch, uint64_t hop, uint64_t lead, int32_t mode,\s+"
                     r"uint64_t out_length, uint64_t out_pitch, uint64_t chunk_frames\);", text)


def test_the_verbs_refuse_no_plan():
    lib = _lib.lib
    assert lib.pfft_plan_set_synthesis_window(None, None) == 1  # PFFT_INVALID_CONFIGURATION
    assert b"null plan" in lib.pfft_last_error()
    assert lib.pfft_execute_istft(None, None, None, 1, 1, 1, 1, 1, 0, _lib.ISTFT_PLAIN, 1, 1, 0) == 1
    assert b"null plan" in lib.pfft_last_error()
    ev = C.c_void_p()
    assert lib.pfft_execute_istft_ex(None, None, None, 1, 1, 1, 1, 1, 0, _lib.ISTFT_NORMALIZE, 1, 1, 0, 0, None, C.byref(ev)) == 1
    assert not ev.value
    chunk = C.c_uint64(7)
    assert lib.pfft_plan_istft_chunk_frames(None, 1, 1, 1, C.byref(chunk)) == 1 and chunk.value == 7


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
        p.set_synthesis_window(torch.zeros(64))
    with pytest.raises(pf.invalid_configuration, match="not of the REAL domain"):
        p.set_synthesis_window(None)
    with pytest.raises(pf.invalid_configuration, match="not of the REAL domain"):
        p.istft(torch.zeros(2, 5, 33, dtype=torch.complex64), torch.zeros(2, 100), 16)


def test_the_window_is_checked_before_the_library_is_called():
    p, torch = _shell(True)
    for bad, text in ((torch.zeros(63), r"shape \(64,\)"), (torch.zeros(2, 64), r"shape \(64,\)"),
                      (torch.zeros(64, dtype=torch.float64), "dtype"), (torch.zeros(64, dtype=torch.complex64), "dtype"),
                      (torch.zeros(64).numpy(), "torch tensor"),
                      (torch.zeros(64), "not in device memory")):
        with pytest.raises(pf.invalid_configuration, match=text):
            p.set_synthesis_window(bad)


def test_bins_and_geometry_are_checked_before_the_library_is_called():
    p, torch = _shell(True)
    c64 = torch.complex64
    # 5 frames of 64 at hop 16 cover positions 0 ... 128: with lead 0 out_length may be 65 ... 128
    y, x = torch.zeros(3, 5, 33, dtype=c64), torch.zeros(3, 128)
    cases = (
        (dict(y=y.to(torch.complex128)), "dtype .* in tensor"), (dict(y=torch.zeros(3, 5, 33)), "dtype .* in tensor"),
        (dict(x=x.double()), "dtype .* out tensor"),
        (dict(x=x[:2]), "3 input signals but 2 output signals"), (dict(x=torch.zeros(3, 256)[:, ::2]), "out tensor needs unit inner stride"),
        (dict(y=torch.zeros(3, 5, 66, dtype=c64)[:, :, ::2]), "in tensor needs unit inner stride"),
        (dict(x=x.reshape(3, 2, 64)), "1-D or 2-D"), (dict(x=x[:, :0]), "not empty"), (dict(y=y[0]), "3-D"),
        (dict(x=x[0], y=y), "2-D"), (dict(y=y[:, :0]), "not empty"), (dict(x=x.numpy()), "torch tensors"),
        (dict(y=torch.zeros(3, 5, 32, dtype=c64)), "32 bins per frame"),
        (dict(hop=0), "hop 0"), (dict(hop=65, x=torch.zeros(3, 300)), "hop 65 above the frame length 64"),
        (dict(lead=64), "lead 64"), (dict(lead=-1), "lead -1"), (dict(chunk_frames=-1), "chunk_frames -1"),
        # a sample that no frame covers: out_length above (F - 1) hop + N - lead
        (dict(x=torch.zeros(3, 129)), "out_length 129 above .* = 128"), (dict(lead=32), "out_length 128 above .* = 96"),
        # a frame that contributes nothing: (F - 1) hop >= out_length + lead
        (dict(x=x[:, :64]), "frame 4 starts at sample 64"), (dict(x=x[:, :32], lead=32), "frame 4 starts at sample 64"),
        (dict(x=torch.zeros(600).as_strided((3, 128), (100, 1))), "signals of the out tensor overlap"),
        (dict(y=torch.zeros(600, dtype=c64).as_strided((3, 5, 33), (165, 20, 1))), "frames of the in tensor overlap"),
        (dict(y=torch.zeros(600, dtype=c64).as_strided((3, 5, 33), (100, 33, 1))), "signals of the in tensor overlap"),
        (dict(), "not in device memory"),
    )
    for change, text in cases:
        kw = dict(y=y, x=x, hop=16, lead=0, chunk_frames=0)
        kw.update(change)
        with pytest.raises(pf.invalid_configuration, match=text):
            p.istft(kw["y"], kw["x"], kw["hop"], lead=kw["lead"], normalize=True, chunk_frames=kw["chunk_frames"])
    # the first accepted value of each geometry bound gets as far as the device check
    for kw in (dict(x=x, lead=0), dict(x=x[:, :96], lead=32), dict(x=x[:, :65], lead=0), dict(x=x[:, :33], lead=32),
               dict(x=torch.zeros(3, 320), hop=64, lead=0), dict(x=x, lead=0, chunk_frames=1), dict(x=x[0], y=y[0], lead=0)):
        with pytest.raises(pf.invalid_configuration, match="not in device memory"):
            p.istft(kw.get("y", y), kw["x"], kw.get("hop", 16), lead=kw["lead"], chunk_frames=kw.get("chunk_frames", 0))
