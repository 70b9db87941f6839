"""The call-geometry rules of filter, stft, istft and dct (portfft_amd/csrc/verb_geometry.hpp) without a GPU and without
the library (tests/cpp/verb_geometry_test.cpp): every refusal with its status and text, each 32-bit boundary as the pair
(largest admitted value, that value + 1), the kernel arguments of admitted calls against hand-computed values, and the
order of the checks -- the rules tests/test_gpu_address_range.py exercises on the device."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_verb_geometry_rules():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = os.path.join(ROOT, "build", "verb_geometry_test")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.run([hipcc, "-std=c++17", "-O1", "-Wall", "-Wextra", "-x", "c++",
                    os.path.join(ROOT, "tests", "cpp", "verb_geometry_test.cpp"), "-o", exe], check=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "verb geometry OK" in p.stdout
    assert "FAIL" not in p.stdout
