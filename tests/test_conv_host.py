"""Fused convolution (PFFT_EXT_CONVOLUTION) on the host side: the opt-in descriptor and its defaults (those of a plain
complex descriptor), the rules of the extension word -- bit 8, alone, on a COMPLEX descriptor; 4 stays unassigned --,
what validate() refuses and why, and the three new symbols of the C ABI."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

import portfft_amd as pf
from portfft_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F, B = pf.direction.FORWARD, pf.direction.BACKWARD


def test_constructor_sets_the_bit_and_the_complex_defaults():
    d = pf.convolution_descriptor([1000])
    assert _lib.EXT_CONVOLUTION == 8 and d._c().extensions == 8
    p = pf.descriptor([1000])
    assert d.domain == pf.domain.COMPLEX and d.scalar == "f32"
    for name in ("lengths", "forward_scale", "backward_scale", "number_of_transforms", "complex_storage", "placement",
                 "forward_strides", "backward_strides", "forward_distance", "backward_distance", "forward_offset",
                 "backward_offset"):
        assert getattr(d, name) == getattr(p, name), name
    for direction in (F, B):
        assert d.get_input_count(direction) == p.get_input_count(direction) == 1000
        assert d.get_layout(direction) == pf.layout.PACKED
    assert pf.convolution_descriptor([64], "f64")._c().precision == 1
    assert pf.descriptor([1000])._c().extensions == 0


def _invalid_extension(c):
    assert _lib.lib.pfft_desc_validate(C.byref(c)) == 1  # PFFT_INVALID_CONFIGURATION
    assert b"extension" in _lib.lib.pfft_last_error()


def test_rules_of_the_extension_word():
    c = pf.descriptor([64], "f32", pf.domain.REAL)._c()  # the bit on a REAL descriptor
    c.extensions = 8
    _invalid_extension(c)
    c = pf.real_descriptor(64)._c()  # with PFFT_EXT_REAL_TRANSFORMS, on either domain
    c.extensions = 8 | 1
    _invalid_extension(c)
    c = pf.convolution_descriptor([64])._c()
    c.extensions = 8 | 1
    _invalid_extension(c)
    c.extensions = 8 | 2  # with PFFT_EXT_ANY_LENGTH
    _invalid_extension(c)
    c.extensions = 8 | 4  # 4 is not assigned
    _invalid_extension(c)
    c.extensions = 16
    _invalid_extension(c)
    c.extensions = 8
    assert _lib.lib.pfft_desc_validate(C.byref(c)) == 0


def _refused(d, exc=pf.unsupported_configuration):
    with pytest.raises(exc) as e:
        d.validate()
    return str(e.value)


def test_validate_names_what_fused_convolution_does_not_cover():
    assert "fp16" in _refused(pf.convolution_descriptor([4096], "f16"))
    sp = pf.convolution_descriptor([4096])
    sp.complex_storage = pf.complex_storage.SPLIT_COMPLEX
    assert "SPLIT_COMPLEX" in _refused(sp)
    assert "1-D" in _refused(pf.convolution_descriptor([128, 4]))
    bi = pf.convolution_descriptor([128])  # batch-interleaved
    bi.number_of_transforms = 8
    bi.forward_strides = bi.backward_strides = [8]
    bi.forward_distance = bi.backward_distance = 1
    assert "batch-interleaved" in _refused(bi)
    st = pf.convolution_descriptor([128])  # every other sample
    st.forward_strides = st.backward_strides = [2]
    st.forward_distance = st.backward_distance = 256
    assert "unit strides" in _refused(st)
    for side in ("forward_distance", "backward_distance"):  # a single transform may carry any distance elsewhere
        sd = pf.convolution_descriptor([128])
        setattr(sd, side, 127)
        msg = _refused(sd)
        assert "distances of at least the length 128" in msg, msg
        plain = pf.descriptor([128])
        setattr(plain, side, 127)
        plain.validate()


def test_a_supported_descriptor_validates():
    for prec in ("f32", "f64"):
        d = pf.convolution_descriptor([1000], prec)
        d.number_of_transforms = 5
        d.forward_distance, d.backward_distance = 1005, 1000
        d.forward_offset, d.backward_offset = 7, 2
        d.forward_scale, d.backward_scale = 0.5, 0.25 / 1000
        d.validate()
        assert d.get_input_count(F) == 7 + 4 * 1005 + 1000 and d.get_output_count(F) == 2 + 5 * 1000
    ip = pf.convolution_descriptor([4096])
    ip.placement = pf.placement.IN_PLACE
    ip.number_of_transforms = 4
    ip.forward_distance = ip.backward_distance = 4101
    ip.validate()
    pf.convolution_descriptor([67 * 8]).validate()  # (the length is the plan's business: refused at commit)


def test_the_library_exports_the_three_new_symbols():
    nm = shutil.which("nm") or "/usr/bin/nm"
    out = subprocess.run([nm, "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for sym in ("pfft_plan_set_filter", "pfft_execute_convolve", "pfft_execute_convolve_ex"):
        assert sym in names, sym
        assert sym in _lib.SYMBOLS
