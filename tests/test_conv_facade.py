"""The C++ facade with the fused convolution: portfft::amd::convolution_descriptor<float> and <double>
(tests/cpp/conv_facade_test.cpp).  CPU: it compiles as user code, its descriptor carries PFFT_EXT_CONVOLUTION and the
descriptor rules answer as documented.  GPU: convolve and correlate against a direct circular convolution in double precision."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "build", "conv_facade_test")


def _build():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    subprocess.run([hipcc, "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "conv_facade_test.cpp"), "-L", os.path.join(ROOT, "portfft_amd"),
                    "-lportfft_amd", "-Wl,-rpath," + os.path.join(ROOT, "portfft_amd"), "-o", EXE], check=True)


def test_conv_facade_builds_and_host_checks_pass():
    _build()
    p = subprocess.run([EXE, "host"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "conv host checks OK" in p.stdout


@pytest.mark.gpu
def test_conv_facade_on_gpu():
    _build()
    p = subprocess.run([EXE], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "conv facade OK" in p.stdout
    print(p.stdout)
