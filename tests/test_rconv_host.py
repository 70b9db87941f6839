"""Fused convolution of real data (PFFT_EXT_REAL_CONVOLUTION) on the host side: the opt-in descriptor and its defaults
(those of a real_descriptor), the rules of the extension word -- bit 16, alone, on a REAL descriptor; 4 stays unassigned
--, what validate() refuses and why (the rules of PFFT_EXT_REAL_TRANSFORMS), and the new symbol of the C ABI."""
import ctypes as C
import shutil
import subprocess

import pytest

import portfft_amd as pf
from portfft_amd import _lib

F, B = pf.direction.FORWARD, pf.direction.BACKWARD


def test_constructor_sets_the_bit_and_the_real_defaults():
    d = pf.real_convolution_descriptor(1000)
    assert _lib.EXT_REAL_CONVOLUTION == 16 and d._c().extensions == 16
    r = pf.real_descriptor(1000)
    assert d.domain == pf.domain.REAL and d.scalar == "f32"
    for name in ("lengths", "forward_scale", "backward_scale", "number_of_transforms", "complex_storage", "placement",
                 "forward_strides", "backward_strides", "forward_distance", "backward_distance", "forward_offset",
                 "backward_offset"):
        assert getattr(d, name) == getattr(r, name), name
    assert d.forward_distance == 1000 and d.backward_distance == 501
    for direction in (F, B):
        assert d.get_input_count(direction) == r.get_input_count(direction)
        assert d.get_output_count(direction) == r.get_output_count(direction)
        assert d.get_layout(direction) == r.get_layout(direction) == pf.layout.PACKED
    assert d.get_input_count(F) == 1000 and d.get_output_count(F) == 501
    assert pf.real_convolution_descriptor(64, "f64")._c().precision == 1
    assert pf.real_descriptor(1000)._c().extensions == 1
    # the C constructor gives the same descriptor
    c = _lib.pfft_desc_t()
    assert _lib.lib.pfft_desc_init_real_convolution(C.byref(c), 0, 1000) == 0
    ref = d._c()
    for name, _ in _lib.pfft_desc_t._fields_:
        a, b = getattr(c, name), getattr(ref, name)
        assert (list(a) == list(b)) if hasattr(a, "__len__") else (a == b), name
    # counts, distances and offsets of a batched and of a padded in-place descriptor: those of the real descriptor
    for make in (pf.real_convolution_descriptor, pf.real_descriptor):
        d = make(64)
        d.number_of_transforms = 5
        d.forward_offset, d.backward_offset = 5, 2
        d.validate()
        assert d.get_input_count(F) == 5 + 4 * 64 + 64 and d.get_output_count(F) == 2 + 4 * 33 + 33
        ip = make(64)
        ip.placement = pf.placement.IN_PLACE
        ip.number_of_transforms = 3
        ip.forward_distance = 66
        ip.forward_offset, ip.backward_offset = 6, 3
        ip.validate()
        assert ip.get_input_count(F) == 6 + 2 * 66 + 64


def _invalid_extension(c):
    assert _lib.lib.pfft_desc_validate(C.byref(c)) == 1  # PFFT_INVALID_CONFIGURATION
    assert b"extension" in _lib.lib.pfft_last_error()


def test_rules_of_the_extension_word():
    c = pf.real_convolution_descriptor(64)._c()
    assert c.extensions == 16 and _lib.lib.pfft_desc_validate(C.byref(c)) == 0  # alone, on REAL
    for bits in (16 | 1, 16 | 2, 16 | 8, 16 | 4, 32):
        c.extensions = bits
        _invalid_extension(c)
    c = pf.descriptor([64])._c()  # the bit on a COMPLEX descriptor
    c.extensions = 16
    _invalid_extension(c)
    c = pf.convolution_descriptor([64])._c()
    c.extensions = 16 | 8
    _invalid_extension(c)
    # bit 8 on a REAL descriptor stays invalid, 4 stays unassigned
    c = pf.real_descriptor(64)._c()
    for bits in (8, 8 | 1, 4):
        c.extensions = bits
        _invalid_extension(c)


def _refused(d, exc=pf.unsupported_configuration):
    with pytest.raises(exc) as e:
        d.validate()
    return str(e.value)


def test_validate_names_what_is_refused():
    assert "fp16" in _refused(pf.real_convolution_descriptor(4096, "f16"))
    assert "odd length 1001" in _refused(pf.real_convolution_descriptor(1001))
    assert "at least 4" in _refused(pf.real_convolution_descriptor(2))
    r2 = pf.real_convolution_descriptor(128)
    r2.lengths = [128, 4]
    r2.forward_strides = r2.backward_strides = [4, 1]
    assert "1-D" in _refused(r2)
    st = pf.real_convolution_descriptor(128)
    st.forward_strides = [2]
    assert "unit strides" in _refused(st)
    wide = pf.real_convolution_descriptor(128)  # (as for real transforms: PACKED, or the padded in-place pair)
    wide.forward_distance = 131
    assert "PACKED" in _refused(wide)
    sp = pf.real_convolution_descriptor(128)
    sp.complex_storage = pf.complex_storage.SPLIT_COMPLEX
    assert "SPLIT_COMPLEX" in _refused(sp)
    # every message is the real descriptor's own
    for make_bad in (lambda m: m(1001), lambda m: m(4096, "f16")):
        assert _refused(make_bad(pf.real_convolution_descriptor)) == _refused(make_bad(pf.real_descriptor))


def test_the_library_exports_the_new_symbol():
    nm = shutil.which("nm") or "/usr/bin/nm"
    out = subprocess.run([nm, "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert "pfft_desc_init_real_convolution" in names
    assert "pfft_desc_init_real_convolution" in _lib.SYMBOLS
