"""The C++ facade with the DCT-IV and the MDCT: prepare_dct4, dct4, set_mdct_window and mdct on the committed type of
portfft::amd::real_descriptor and real_convolution_descriptor (tests/cpp/dct4_facade_test.cpp).  CPU: it compiles and
links as user code, the verbs have the right types, the C entry points answer a null plan.  GPU: dct4 forward and inverse
and mdct against direct sums in double precision, out of place and in place, untouched scalars between the rows and the
frames; the verbs before their prepare call, what the C ABI refuses, and all four verbs on a COMPLEX plan throw
invalid_configuration."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "build", "dct4_facade_test")


def _build():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    subprocess.run([hipcc, "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "dct4_facade_test.cpp"), "-L", os.path.join(ROOT, "portfft_amd"),
                    "-lportfft_amd", "-Wl,-rpath," + os.path.join(ROOT, "portfft_amd"), "-o", EXE], check=True)


def test_dct4_facade_builds_and_host_checks_pass():
    _build()
    p = subprocess.run([EXE, "host"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "dct4 host checks OK" in p.stdout


@pytest.mark.gpu
def test_dct4_facade_on_gpu():
    _build()
    p = subprocess.run([EXE], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "dct4 facade OK" in p.stdout
    print(p.stdout)
