"""The DCT-IV / MDCT kernels under the runtime compiler, without a GPU (tests/cpp/dct4_jit_test.cpp): the appended family
number JF_DCT4 = 16, the older pinned numbers unchanged, the open form behind the two pinned tables and the one accessor
that serves all three (relations only: the size of the open table is pinned nowhere), the spelling of the instantiations,
and hiprtc builds of both cells for gfx950 -- the half lengths of N = 2000 and N = 12000 in fp32 and of N = 6000 in fp64,
the odd half length of N = 30, a STAGED and a TW_REGS configuration."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dct4_kernel_forms_compile_with_hiprtc(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = os.path.join(ROOT, "build", "dct4_jit_test")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.run([hipcc, "-std=c++17", "-O1", os.path.join(ROOT, "tests", "cpp", "dct4_jit_test.cpp"), "-L",
                    os.path.join(ROOT, "portfft_amd"), "-lportfft_amd", "-Wl,-rpath," + os.path.join(ROOT, "portfft_amd"),
                    "-o", exe], check=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=900,
                       env=dict(os.environ, PFFT_JIT_CACHE_DIR=str(tmp_path)))
    assert p.returncode == 0, p.stdout + p.stderr
    assert "dct4 jit OK" in p.stdout
    assert "FAIL" not in p.stdout
    assert p.stdout.count("hiprtc dct4 ") == 6
