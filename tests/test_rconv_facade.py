"""The C++ facade with fused convolution and overlap-save filtering of real data: portfft::amd::real_convolution_descriptor
and the verbs on real scalars of its committed type (tests/cpp/rconv_facade_test.cpp).  CPU: it compiles as user code,
the verbs have the right types and the descriptor carries the bit.  GPU: convolve, correlate and filter in both modes
against direct sums in double precision."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "build", "rconv_facade_test")


def _build():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    subprocess.run([hipcc, "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "rconv_facade_test.cpp"), "-L", os.path.join(ROOT, "portfft_amd"),
                    "-lportfft_amd", "-Wl,-rpath," + os.path.join(ROOT, "portfft_amd"), "-o", EXE], check=True)


def test_rconv_facade_builds_and_host_checks_pass():
    _build()
    p = subprocess.run([EXE, "host"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "rconv host checks OK" in p.stdout


@pytest.mark.gpu
def test_rconv_facade_on_gpu():
    _build()
    p = subprocess.run([EXE], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "rconv facade OK" in p.stdout
    print(p.stdout)
