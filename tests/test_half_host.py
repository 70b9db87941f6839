"""fp16 storage (PFFT_PRECISION_F16, IEEE binary16 data computed in fp32) on the host side: the precision names, the
descriptor's counts and layouts, what validate() refuses, and -- without a GPU -- hiprtc compilation of the converting
kernel forms for gfx950."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

import portfft_amd as pf
from portfft_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", ["f16", "half", "float16", 2])
def test_half_precision_names(name):
    d = pf.descriptor([64], name)
    assert d.scalar == "f16"
    d.validate()


def test_torch_half_dtypes_name_the_precision():
    torch = pytest.importorskip("torch")
    for dt in (torch.float16, torch.complex32):
        assert pf.descriptor([64], dt).scalar == "f16"
    assert pf.descriptor([64], torch.complex64).scalar == "f32"


def test_counts_and_layouts_match_f32():
    for lengths, batch in (([4096], 3), ([10000], 1), ([7], 33)):
        h, s = pf.descriptor(lengths, "f16"), pf.descriptor(lengths, "f32")
        for d in (h, s):
            d.number_of_transforms = batch
            d.forward_offset = 5
            d.backward_offset = 2
        for dr in (pf.direction.FORWARD, pf.direction.BACKWARD):
            assert h.get_input_count(dr) == s.get_input_count(dr)
            assert h.get_output_count(dr) == s.get_output_count(dr)
            assert h.get_layout(dr) == s.get_layout(dr) == pf.layout.PACKED
        h.validate()


def test_offsets_scales_storage_and_placement_validate():
    d = pf.descriptor([32768], "f16")
    d.number_of_transforms = 4
    d.forward_offset = d.backward_offset = 3
    d.forward_scale = 1.0 / 32768
    d.complex_storage = pf.complex_storage.SPLIT_COMPLEX
    d.placement = pf.placement.IN_PLACE
    d.validate()


def _refused(d, exc=pf.unsupported_configuration):
    with pytest.raises(exc) as e:
        d.validate()
    return str(e.value)


def test_validate_refuses_what_fp16_storage_does_not_cover():
    assert "1-D" in _refused(pf.descriptor([64, 64], "f16"))
    bi = pf.descriptor([256], "f16")  # batch-interleaved
    bi.number_of_transforms = 8
    bi.forward_strides = bi.backward_strides = [8]
    bi.forward_distance = bi.backward_distance = 1
    assert bi.get_layout(pf.direction.FORWARD) == pf.layout.BATCH_INTERLEAVED
    assert "PACKED" in _refused(bi)
    up = pf.descriptor([256], "f16")  # unpacked: padded rows
    up.number_of_transforms = 4
    up.forward_distance = up.backward_distance = 300
    assert up.get_layout(pf.direction.FORWARD) == pf.layout.UNPACKED
    assert "PACKED" in _refused(up)
    up2 = pf.descriptor([256], "f16")  # unpacked: every other sample, on one side only
    up2.backward_strides = [2]
    up2.backward_distance = 512
    _refused(up2)
    _refused(pf.descriptor([64], "f16", pf.domain.REAL))
    # the same descriptors in fp32 stay valid
    for d in (bi, up, up2):
        d.scalar = "f32"
        d.validate()


def test_other_precision_codes_stay_invalid():
    with pytest.raises(pf.invalid_configuration):
        pf.descriptor([64], "bf16")
    for code in (3, -1):
        c = pf.descriptor([64], "f16")._c()
        c.precision = code
        assert _lib.lib.pfft_desc_validate(C.byref(c)) == 1  # PFFT_INVALID_CONFIGURATION


def test_half_kernel_forms_compile_with_hiprtc(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = os.path.join(ROOT, "build", "half_jit_test")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.run([hipcc, "-std=c++17", "-O1", os.path.join(ROOT, "tests", "cpp", "half_jit_test.cpp"), "-L",
                    os.path.join(ROOT, "portfft_amd"), "-lportfft_amd", "-Wl,-rpath," + os.path.join(ROOT, "portfft_amd"),
                    "-o", exe], check=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=900,
                       env=dict(os.environ, PFFT_JIT_CACHE_DIR=str(tmp_path)))
    assert p.returncode == 0, p.stdout + p.stderr
    assert "half jit OK" in p.stdout
    assert p.stdout.count("hiprtc half n=") == 3
