"""The C++ facade with real transforms: portfft::amd::real_descriptor<float> and <double> (tests/cpp/real_facade_test.cpp).
CPU: it compiles as user code, counts and refusals.  GPU: both directions against a double-precision DFT, in place,
and a COMPLEX plan's real overloads still throw."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "build", "real_facade_test")


def _build():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    subprocess.run([hipcc, "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "real_facade_test.cpp"), "-L", os.path.join(ROOT, "portfft_amd"),
                    "-lportfft_amd", "-Wl,-rpath," + os.path.join(ROOT, "portfft_amd"), "-o", EXE], check=True)


def test_real_facade_builds_and_host_checks_pass():
    _build()
    p = subprocess.run([EXE, "host"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "real host checks OK" in p.stdout


@pytest.mark.gpu
def test_real_facade_on_gpu():
    _build()
    p = subprocess.run([EXE], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "real facade OK" in p.stdout
    print(p.stdout)
