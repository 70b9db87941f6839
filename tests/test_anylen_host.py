"""Any-length transforms (PFFT_EXT_ANY_LENGTH) on the host side: the opt-in descriptor, its counts, distances and
layouts (those of a plain complex descriptor), the rules of the extension word and what validate() refuses and why.
The bit is a permission: it changes nothing for a descriptor whose lengths have an ordinary plan."""
import ctypes as C

import pytest

import portfft_amd as pf
from portfft_amd import _lib

F, B = pf.direction.FORWARD, pf.direction.BACKWARD


def test_any_length_descriptor_validates_and_carries_the_bit():
    d = pf.any_length_descriptor([4093])
    d.validate()
    assert d.domain == pf.domain.COMPLEX and d.scalar == "f32"
    assert _lib.EXT_ANY_LENGTH == 2 and d._c().extensions == 2
    pf.any_length_descriptor([2039], "f64").validate()
    assert pf.descriptor([4093])._c().extensions == 0


@pytest.mark.parametrize("n", [4093, 1000])
def test_counts_layouts_and_distances_are_the_plain_descriptors(n):
    def fill(d):
        d.number_of_transforms = 3
        d.forward_distance, d.backward_distance = n + 5, n
        d.forward_offset, d.backward_offset = 7, 2
        return d
    a, p = fill(pf.any_length_descriptor([n])), fill(pf.descriptor([n]))
    a.validate()
    for direction in (F, B):
        assert a.get_input_count(direction) == p.get_input_count(direction)
        assert a.get_output_count(direction) == p.get_output_count(direction)
        assert a.get_layout(direction) == p.get_layout(direction)
        assert a.get_distance(direction) == p.get_distance(direction)
        assert a.get_strides(direction) == p.get_strides(direction)
    assert a.get_input_count(F) == 7 + 2 * (n + 5) + n and a.get_output_count(F) == 2 + 3 * n
    assert a.get_layout(F) == pf.layout.UNPACKED and a.get_layout(B) == pf.layout.PACKED
    ip = pf.any_length_descriptor([n])
    ip.placement = pf.placement.IN_PLACE
    ip.number_of_transforms = 4
    ip.forward_distance = ip.backward_distance = n + 5
    ip.validate()


def _invalid_extension(c):
    assert _lib.lib.pfft_desc_validate(C.byref(c)) == 1  # PFFT_INVALID_CONFIGURATION
    assert b"extension" in _lib.lib.pfft_last_error()


def test_rules_of_the_extension_word():
    c = pf.descriptor([64], "f32", pf.domain.REAL)._c()  # the bit on a REAL descriptor
    c.extensions = 2
    _invalid_extension(c)
    c = pf.real_descriptor(64)._c()  # both extensions
    c.extensions = 3
    _invalid_extension(c)
    c = pf.any_length_descriptor([64])._c()
    c.extensions = 3
    _invalid_extension(c)
    c = pf.any_length_descriptor([64])._c()  # unknown bits
    c.extensions = 4
    _invalid_extension(c)
    c.extensions = 6
    _invalid_extension(c)
    c.extensions = 2
    assert _lib.lib.pfft_desc_validate(C.byref(c)) == 0


def _refused(d, exc=pf.unsupported_configuration):
    with pytest.raises(exc) as e:
        d.validate()
    return str(e.value)


def test_validate_names_what_any_length_transforms_do_not_cover():
    assert "fp16" in _refused(pf.any_length_descriptor([4093], "f16"))
    sp = pf.any_length_descriptor([4093])
    sp.complex_storage = pf.complex_storage.SPLIT_COMPLEX
    assert "SPLIT_COMPLEX" in _refused(sp)
    assert "1-D" in _refused(pf.any_length_descriptor([127, 4]))
    assert "1-D" in _refused(pf.any_length_descriptor([4, 127]))
    bi = pf.any_length_descriptor([127])  # batch-interleaved
    bi.number_of_transforms = 8
    bi.forward_strides = bi.backward_strides = [8]
    bi.forward_distance = bi.backward_distance = 1
    assert "batch-interleaved" in _refused(bi)
    st = pf.any_length_descriptor([127])  # every other sample
    st.forward_strides = st.backward_strides = [2]
    st.forward_distance = st.backward_distance = 254
    assert "unit strides" in _refused(st)


def test_the_bit_is_a_permission_for_lengths_with_an_ordinary_plan():
    # none of the restrictions above applies when no length has a prime factor above 61
    pf.any_length_descriptor([4096], "f16").validate()
    sp = pf.any_length_descriptor([61 * 64])
    sp.complex_storage = pf.complex_storage.SPLIT_COMPLEX
    sp.validate()
    pf.any_length_descriptor([128, 4]).validate()
    bi = pf.any_length_descriptor([128])
    bi.number_of_transforms = 8
    bi.forward_strides = bi.backward_strides = [8]
    bi.forward_distance = bi.backward_distance = 1
    bi.validate()
