"""The pair kernel under the runtime compiler, without a GPU (tests/cpp/pairs_jit_test.cpp).  Relations only: the family
is appended, the form is an open form (at or behind N_SPEC_FORMS_END) whose cells() point into open_form, the row of the
family table exists and spells the conjugate as the trailing bool, the LDS rule is the real form's plus a second image
set plus two windows per staged row; and hiprtc builds both kernels for gfx950 at M = 3 and M = 296, the half length of
N = 2000 in fp32 and of N = 6000 in fp64."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pairs_kernel_form_compiles_with_hiprtc(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = os.path.join(ROOT, "build", "pairs_jit_test")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.run([hipcc, "-std=c++17", "-O1", os.path.join(ROOT, "tests", "cpp", "pairs_jit_test.cpp"), "-L",
                    os.path.join(ROOT, "portfft_amd"), "-lportfft_amd", "-Wl,-rpath," + os.path.join(ROOT, "portfft_amd"),
                    "-o", exe], check=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=900,
                       env=dict(os.environ, PFFT_JIT_CACHE_DIR=str(tmp_path)))
    assert p.returncode == 0, p.stdout + p.stderr
    assert "pairs jit OK" in p.stdout
    assert "FAIL" not in p.stdout
    assert p.stdout.count("hiprtc pairs ") == 4
    assert p.stdout.count("lds M=") == 4
