"""The call-geometry rules of periodogram (portfft_amd/csrc/verb_geometry.hpp) without a GPU and without the library
(tests/cpp/periodogram_geometry_test.cpp): every refusal with its status and text, the order of the checks through calls
that break two rules, each 32-bit boundary as the pair (largest admitted value, that value + 1), and the kernel arguments
and `groups` of admitted calls against hand-computed values, with rows that do not divide the frames and one row per
signal."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_periodogram_geometry_rules():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = os.path.join(ROOT, "build", "periodogram_geometry_test")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.run([hipcc, "-std=c++17", "-O1", "-Wall", "-Wextra", "-x", "c++",
                    os.path.join(ROOT, "tests", "cpp", "periodogram_geometry_test.cpp"), "-o", exe], check=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "periodogram geometry OK" in p.stdout
    assert "FAIL" not in p.stdout
