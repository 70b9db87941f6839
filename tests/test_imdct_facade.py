"""The C++ facade with the inverse MDCT: set_imdct_window, imdct_chunk_frames and imdct on the committed type of
portfft::amd::real_descriptor and real_convolution_descriptor (tests/cpp/imdct_facade_test.cpp).  CPU: it compiles and
links as user code, the verbs have the right types, the C entry points answer a null plan.  GPU: imdct against the direct
sum in double precision with odd pitches, untouched scalars behind the signals, the plan's own chunk and chunks of 2 frames
bit for bit; the verbs before their window, what the C ABI refuses, and the three verbs on a COMPLEX plan throw
invalid_configuration."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "build", "imdct_facade_test")


def _build():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    subprocess.run([hipcc, "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "imdct_facade_test.cpp"), "-L", os.path.join(ROOT, "portfft_amd"),
                    "-lportfft_amd", "-Wl,-rpath," + os.path.join(ROOT, "portfft_amd"), "-o", EXE], check=True)


def test_imdct_facade_builds_and_host_checks_pass():
    _build()
    p = subprocess.run([EXE, "host"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "imdct host checks OK" in p.stdout


@pytest.mark.gpu
def test_imdct_facade_on_gpu():
    _build()
    p = subprocess.run([EXE], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "imdct facade OK" in p.stdout
    print(p.stdout)
