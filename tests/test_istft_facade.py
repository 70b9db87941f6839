"""The C++ facade with the inverse short-time Fourier transform: set_synthesis_window and istft on the committed type of
portfft::amd::real_descriptor and real_convolution_descriptor (tests/cpp/istft_facade_test.cpp).  CPU: it compiles as user
code, the verbs have the right types, the C entry points answer a null plan.  GPU: both modes against direct sums in
double precision, untouched elements behind out_length and between the signals, and a COMPLEX plan refuses both verbs."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "build", "istft_facade_test")


def _build():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    subprocess.run([hipcc, "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "istft_facade_test.cpp"), "-L", os.path.join(ROOT, "portfft_amd"),
                    "-lportfft_amd", "-Wl,-rpath," + os.path.join(ROOT, "portfft_amd"), "-o", EXE], check=True)


def test_istft_facade_builds_and_host_checks_pass():
    _build()
    p = subprocess.run([EXE, "host"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "istft host checks OK" in p.stdout


@pytest.mark.gpu
def test_istft_facade_on_gpu():
    _build()
    p = subprocess.run([EXE], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "istft facade OK" in p.stdout
    print(p.stdout)
