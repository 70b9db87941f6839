"""Real transforms (PFFT_EXT_REAL_TRANSFORMS) on the host side: the opt-in descriptor, its counts, distances and
layouts, what validate() refuses and why, the C entry point, and -- without a GPU -- hiprtc compilation of the real
kernel forms for gfx950.  A plain REAL descriptor keeps the reference's answer."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

import portfft_amd as pf
from portfft_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F, B = pf.direction.FORWARD, pf.direction.BACKWARD


def test_real_descriptor_validates_with_real_defaults():
    d = pf.real_descriptor(4096)
    d.validate()
    assert d.domain == pf.domain.REAL and d.scalar == "f32"
    assert (d.forward_distance, d.backward_distance) == (4096, 2049)
    assert d.get_input_count(F) == 4096 and d.get_output_count(F) == 2049
    assert d.get_input_count(B) == 2049 and d.get_output_count(B) == 4096
    assert d.get_layout(F) == d.get_layout(B) == pf.layout.PACKED
    assert d._c().extensions == 1
    pf.real_descriptor(4096, "f64").validate()


def test_counts_with_offsets_and_batch():
    d = pf.real_descriptor(4096)
    d.number_of_transforms = 3
    d.forward_offset, d.backward_offset = 5, 2
    d.validate()
    assert d.get_input_count(F) == 5 + 2 * 4096 + 4096
    assert d.get_output_count(F) == 2 + 2 * 2049 + 2049
    assert d.get_layout(F) == d.get_layout(B) == pf.layout.PACKED


def test_in_place_is_the_padded_pair():
    d = pf.real_descriptor(4096)
    d.number_of_transforms = 3
    d.placement = pf.placement.IN_PLACE
    d.forward_distance = 2 * 2049
    d.forward_offset, d.backward_offset = 6, 3
    d.validate()
    assert d.get_layout(F) == d.get_layout(B) == pf.layout.PACKED
    assert d.get_input_count(F) == 6 + 2 * 4098 + 4096
    assert d.get_output_count(F) == 3 + 2 * 2049 + 2049
    # out of place the padded forward distance is UNPACKED (and refused)
    d.placement = pf.placement.OUT_OF_PLACE
    assert d.get_layout(F) == pf.layout.UNPACKED


def test_c_init_real_and_exported_symbol():
    c = _lib.pfft_desc_t()
    assert _lib.lib.pfft_desc_init_real(C.byref(c), 1, 64) == 0
    assert (c.domain, c.extensions, c.precision, c.rank) == (0, 1, 1, 1)
    assert (c.forward_distance, c.backward_distance, c.placement) == (64, 33, 1)
    assert _lib.lib.pfft_desc_validate(C.byref(c)) == 0
    plain = _lib.pfft_desc_t()
    n = (C.c_uint64 * 1)(64)
    assert _lib.lib.pfft_desc_init(C.byref(plain), 0, 0, 1, n) == 0
    assert plain.extensions == 0
    nm = shutil.which("nm")
    if nm:
        out = subprocess.run([nm, "-D", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
        assert " T pfft_desc_init_real" in out


def _refused(d, exc=pf.unsupported_configuration):
    with pytest.raises(exc) as e:
        d.validate()
    return str(e.value)


def test_plain_real_descriptor_and_unknown_bits_are_refused():
    assert "REAL domain is unsupported" in _refused(pf.descriptor([64], "f32", pf.domain.REAL))
    c = pf.real_descriptor(64)._c()
    c.extensions = 3
    assert _lib.lib.pfft_desc_validate(C.byref(c)) == 1  # PFFT_INVALID_CONFIGURATION
    assert b"extension" in _lib.lib.pfft_last_error()
    c = pf.descriptor([64])._c()  # the bit on a COMPLEX descriptor
    c.extensions = 1
    assert _lib.lib.pfft_desc_validate(C.byref(c)) == 1


def test_validate_names_what_real_transforms_do_not_cover():
    assert "even" in _refused(pf.real_descriptor(63))
    assert "at least 4" in _refused(pf.real_descriptor(2))
    assert "fp16" in _refused(pf.real_descriptor(64, "f16"))
    nd = pf.real_descriptor(64)
    nd.lengths = [64, 64]
    nd.forward_strides = nd.backward_strides = [64, 1]
    assert "1-D" in _refused(nd)
    sp = pf.real_descriptor(64)
    sp.complex_storage = pf.complex_storage.SPLIT_COMPLEX
    assert "SPLIT_COMPLEX" in _refused(sp)
    ip = pf.real_descriptor(64)  # in place without padded rows
    ip.placement = pf.placement.IN_PLACE
    assert "padded" in _refused(ip, pf.invalid_configuration)
    ip.forward_distance, ip.backward_distance = 80, 40  # padded, but not the PACKED pair
    assert "PACKED" in _refused(ip)
    bi = pf.real_descriptor(64)  # batch-interleaved
    bi.number_of_transforms = 8
    bi.forward_strides = bi.backward_strides = [8]
    bi.forward_distance = bi.backward_distance = 1
    assert "batch-interleaved" in _refused(bi)
    up = pf.real_descriptor(64)
    up.number_of_transforms = 2
    up.forward_distance = 70
    assert "PACKED" in _refused(up)


def test_real_kernel_forms_compile_with_hiprtc(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = os.path.join(ROOT, "build", "real_jit_test")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.run([hipcc, "-std=c++17", "-O1", os.path.join(ROOT, "tests", "cpp", "real_jit_test.cpp"), "-L",
                    os.path.join(ROOT, "portfft_amd"), "-lportfft_amd", "-Wl,-rpath," + os.path.join(ROOT, "portfft_amd"),
                    "-o", exe], check=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=900,
                       env=dict(os.environ, PFFT_JIT_CACHE_DIR=str(tmp_path)))
    assert p.returncode == 0, p.stdout + p.stderr
    assert "real jit OK" in p.stdout
    assert p.stdout.count("hiprtc real n=") == 3
