"""The call-geometry rules of convolve_pairs / correlate_pairs (portfft_amd/csrc/verb_geometry.hpp) without a GPU and
without the library (tests/cpp/pairs_geometry_test.cpp, a program of its own): every refusal with its status and text in
the order of the checks, calls that break two rules, each 32-bit boundary as the pair (largest admitted value, that value +
1), and the kernel arguments and `groups` of admitted calls against hand-computed values.  The program runs twice: plainly,
and built with the address and undefined-behaviour sanitizers of the host compiler (the checks do 64- and 128-bit
arithmetic on values up to 2^63)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name,flags", [("pairs_geometry_test", ["-O1"]),
                                        ("pairs_geometry_test_san", ["-O1", "-g", "-fsanitize=address,undefined",
                                                                     "-fno-sanitize-recover=all"])])
def test_pairs_geometry_rules(name, flags):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = os.path.join(ROOT, "build", name)
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.run([hipcc, "-std=c++17", "-Wall", "-Wextra"] + flags + ["-x", "c++",
                    os.path.join(ROOT, "tests", "cpp", "pairs_geometry_test.cpp"), "-o", exe], check=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "pairs geometry OK" in p.stdout
    assert "FAIL" not in p.stdout
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr
