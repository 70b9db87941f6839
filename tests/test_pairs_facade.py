"""The C++ facade with the pair verbs: prepare_pairs, convolve_pairs and correlate_pairs on the committed type of
portfft::amd::real_descriptor and real_convolution_descriptor (tests/cpp/pairs_facade_test.cpp).  CPU: it compiles and links
as user code, the verbs have the right types, the C entry points answer a null plan.  GPU: one shape per precision against
the direct double-precision sums in the program itself, relative L2 per row within REL_L2_TOL, lengths below N on all three
sides, odd pitches, untouched scalars between the rows, a second call bit for bit, the peak of the phase transform at the
rotation; the verbs before prepare_pairs, what the C ABI refuses, and the verbs on a COMPLEX plan throw
invalid_configuration."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "build", "pairs_facade_test")


def _build():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    subprocess.run([hipcc, "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "pairs_facade_test.cpp"), "-L", os.path.join(ROOT, "portfft_amd"),
                    "-lportfft_amd", "-Wl,-rpath," + os.path.join(ROOT, "portfft_amd"), "-o", EXE], check=True)


def test_pairs_facade_builds_and_host_checks_pass():
    _build()
    p = subprocess.run([EXE, "host"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "pairs host checks OK" in p.stdout


@pytest.mark.gpu
def test_pairs_facade_on_gpu():
    _build()
    p = subprocess.run([EXE], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "pairs facade OK" in p.stdout
    print(p.stdout)
