"""The inverse MDCT kernel under the runtime compiler, without a GPU (tests/cpp/imdct_jit_test.cpp): the appended family
number JF_IMDCT = 17, the older pinned numbers unchanged, the open form behind WF_DCT4 reached through cells() (relations
only), the spelling of the one kernel that fills both cells, the LDS rule (the real form's bytes and a carry of M scalars)
and hiprtc builds for gfx950 -- M = 3 and M = 296, the half lengths of N = 2000 and N = 12000 in fp32 and of N = 6000 in
fp64, the odd half length of N = 30."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_imdct_kernel_form_compiles_with_hiprtc(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = os.path.join(ROOT, "build", "imdct_jit_test")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.run([hipcc, "-std=c++17", "-O1", os.path.join(ROOT, "tests", "cpp", "imdct_jit_test.cpp"), "-L",
                    os.path.join(ROOT, "portfft_amd"), "-lportfft_amd", "-Wl,-rpath," + os.path.join(ROOT, "portfft_amd"),
                    "-o", exe], check=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=900,
                       env=dict(os.environ, PFFT_JIT_CACHE_DIR=str(tmp_path)))
    assert p.returncode == 0, p.stdout + p.stderr
    assert "imdct jit OK" in p.stdout
    assert "FAIL" not in p.stdout
    assert p.stdout.count("hiprtc imdct ") == 6
    assert p.stdout.count("lds M=") == 6
