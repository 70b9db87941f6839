"""The pair verbs (prepare_pairs / convolve_pairs / correlate_pairs of a plan of the REAL domain) on the host side: the
three new entry points of the C ABI and their binding, what they answer on no plan, that no extension bit was added, and
the argument errors the Python verbs raise before the library is called -- each names the offending quantity.  (What the
library itself refuses on a plan stands in tests/cpp/pairs_geometry_test.cpp and test_gpu_pairs.py.)"""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

import portfft_amd as pf
from portfft_amd import _lib

NEW = ("pfft_plan_prepare_pairs", "pfft_execute_pairs", "pfft_execute_pairs_ex")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_library_exports_the_three_new_symbols():
    nm = shutil.which("nm") or "/usr/bin/nm"
    out = subprocess.run([nm, "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for sym in NEW:
        assert sym in names, sym
        assert sym in _lib.SYMBOLS
        assert getattr(_lib.lib, sym).argtypes == _lib.SYMBOLS[sym][1]
    u64, vp = C.c_uint64, C.c_void_p
    assert _lib.SYMBOLS["pfft_plan_prepare_pairs"] == (C.c_int, [vp])
    # plan, mode, x, y, out, n_rows, (length, pitch) of x, of y, of out, phat_floor
    assert _lib.SYMBOLS["pfft_execute_pairs"] == (C.c_int, [vp, C.c_int32, vp, vp, vp] + [u64] * 7 + [C.c_double])
    assert _lib.SYMBOLS["pfft_execute_pairs_ex"][1][:13] == _lib.SYMBOLS["pfft_execute_pairs"][1]
    assert _lib.SYMBOLS["pfft_execute_pairs_ex"][1][13:] == [C.c_int32, C.POINTER(vp), C.POINTER(vp)]


def test_the_header_declares_them():
    text = open(os.path.join(ROOT, "include", "portfft_amd.h")).read()
    for sym in NEW:
        assert re.search(r"pfft_status %s\(" % sym, text), sym
    assert re.search(r"pfft_plan_prepare_pairs\(pfft_plan_t\* plan\);", text)
    # the argument order of the issue
    assert re.search(r"pfft_execute_pairs\(pfft_plan_t\* plan, int32_t mode, const void\* x, const void\* y, void\* out, "
                     r"uint64_t n_rows,\s+uint64_t x_length, uint64_t x_pitch, uint64_t y_length, uint64_t y_pitch,\s+"
                     r"uint64_t out_length, uint64_t out_pitch, double phat_floor\);", text)
    block = text[text.index("Circular convolution and correlation of PAIRS"):text.index("pfft_plan_prepare_pairs(pfft_plan_t")]
    for word in ("4 GiB", "GCC-PHAT", "no extension bit", "forward_scale^2 * backward_scale", "max(|P[k]|, f)", "autocorrelation",
                 "x_length - 1", "r[N - 1]", "uploads nothing", "do not fit", "PFFT_CORRELATE", "2^31"):
        assert word in block, word
    facade = open(os.path.join(ROOT, "include", "portfft", "portfft.hpp")).read()
    assert "void prepare_pairs()" in facade
    assert re.search(r"event convolve_pairs\(const scalar_type\* x, const scalar_type\* y, scalar_type\* out,", facade)
    assert re.search(r"event correlate_pairs\(const scalar_type\* x, const scalar_type\* y, scalar_type\* out,", facade)
    assert "double phat_floor = 0)" in facade


def test_what_the_second_image_set_leans_on_in_other_headers():
    """stockham_wg_pairs.hpp hands the passes the wrapped row f - FPW for an image of y, so that they find the one TWL copy.
    That is right as long as wg_pass takes the row as `unsigned`, uses it for the TWL copy in exactly this expression and
    otherwise only for the io's offsets, and slot_io ignores the row.  A change of either text fails here and points at the
    kernel (which the TWL lines of test_gpu_pairs.py / test_gpu_pairs_registry.py run)."""
    csrc = os.path.join(ROOT, "portfft_amd", "csrc")
    wg = open(os.path.join(csrc, "stockham_wg.hpp")).read()
    body = wg[wg.index("PFA_DEV void wg_pass(const IO& io, unsigned f, cx<typename Cfg::T>* lds, int tid,"):
              wg.index("PFA_DEV void wg_passes(const IO& io, unsigned f, cx<typename Cfg::T>* lds, int tid,")]
    assert "const cx<T>* twl = lds + (Cfg::FPW - f) * Cfg::LDS_PER_FFT;" in body
    # every other use of the row inside a pass is an offset of the io
    uses = re.findall(r"[^\n]*\bf\b[^\n]*", body.split("{", 1)[1])
    others = [u.strip() for u in uses if "(Cfg::FPW - f)" not in u and "io.in_off(f," not in u and "io.out_off(f," not in u
              and not u.strip().startswith("//")]
    assert others == [], others
    ols = open(os.path.join(csrc, "stockham_wg_ols.hpp")).read()
    assert "static PFA_DEV unsigned in_off(unsigned, unsigned j) { return j; }" in ols
    assert "static PFA_DEV unsigned out_off(unsigned, unsigned j) { return j; }" in ols
    assert "struct window_io : slot_io {" in ols
    pairs = open(os.path.join(csrc, "stockham_wg_pairs.hpp")).read()
    assert "const unsigned fy = static_cast<unsigned>(f - Cfg::FPW);" in pairs
    assert "wg_passes<Cfg, false, 0, WG_LAST_TO_LDS>(ioy, fy, ldsy, tid, twp, twr, scale);" in pairs
    assert "test_pairs_host.py" in pairs


def test_the_verbs_refuse_no_plan():
    lib = _lib.lib
    assert lib.pfft_plan_prepare_pairs(None) == 1  # PFFT_INVALID_CONFIGURATION
    assert b"null plan" in lib.pfft_last_error()
    assert lib.pfft_execute_pairs(None, 1, None, None, None, 1, 64, 64, 64, 64, 64, 64, 0.0) == 1
    assert b"null plan" in lib.pfft_last_error()
    ev = C.c_void_p()
    assert lib.pfft_execute_pairs_ex(None, 1, None, None, None, 1, 64, 64, 64, 64, 64, 64, 0.0, 0, None, C.byref(ev)) == 1
    assert b"null plan" in lib.pfft_last_error()
    assert not ev.value


def test_no_extension_bit_was_added():
    assert pf.real_descriptor(64)._c().extensions == 1 and pf.real_convolution_descriptor(64)._c().extensions == 16
    c = pf.real_descriptor(64)._c()
    for bits in (4, 32, 64, 1 | 32):
        c.extensions = bits
        assert _lib.lib.pfft_desc_validate(C.byref(c)) == 1
        assert b"extension" in _lib.lib.pfft_last_error()


def _shell(real, scalar="f32", n=64, prepared=True):
    """a committed_descriptor without a plan (no GPU here): what the verbs check before they call the library"""
    import torch
    p = object.__new__(pf.committed_descriptor)
    p._plan = None
    p._real = real
    p._torch = torch
    p._device = None
    p._scalar = scalar
    p._real_dtype, p._cplx_dtype = (torch.float32, torch.complex64) if scalar == "f32" else (torch.float64, torch.complex128)
    p.params = pf.real_descriptor(n, scalar) if real else pf.descriptor([n], scalar)
    if prepared:
        p._pairs_prepared = True
    return p, torch


def test_the_verbs_belong_to_a_real_plan():
    p, torch = _shell(False)
    z = torch.zeros(3, 64)
    for call in (p.prepare_pairs, lambda: p.convolve_pairs(z, z, z.clone()), lambda: p.correlate_pairs(z, z, z.clone())):
        with pytest.raises(pf.invalid_configuration, match="not of the REAL domain"):
            call()


def test_the_verbs_need_prepare_pairs():
    p, torch = _shell(True, prepared=False)
    z = torch.zeros(3, 64)
    for call, verb in ((lambda: p.convolve_pairs(z, z, z.clone()), "convolve_pairs"),
                       (lambda: p.correlate_pairs(z, z, z.clone(), phat_floor=1e-3), "correlate_pairs")):
        with pytest.raises(pf.invalid_configuration, match="%s: prepare_pairs missing" % verb):
            call()
    # ... and that answers before any look at the arguments
    with pytest.raises(pf.invalid_configuration, match="prepare_pairs missing"):
        p.correlate_pairs(None, None, None, phat_floor=-1)


def test_pairs_arguments_are_checked_before_the_library_is_called():
    p, torch = _shell(True)
    n = 64
    x, y, out = torch.zeros(3, 63), torch.zeros(3, 33), torch.zeros(3, 64)
    cases = (
        (dict(x=x.double()), "dtype torch.float64 of the x tensor"), (dict(y=y.double()), "dtype .* y tensor"),
        (dict(out=out.double()), "dtype .* out tensor"),
        (dict(out=torch.zeros(3, 64, dtype=torch.complex64)), "dtype torch.complex64 of the out tensor"),
        (dict(x=x.reshape(3, 7, 9)), "x tensor must be 1-D or 2-D"), (dict(y=y.reshape(3, 3, 11)), "y tensor must be 1-D or 2-D"),
        (dict(out=out.reshape(3, 8, 8)), "out tensor must be 1-D or 2-D"), (dict(x=x[:, :0]), "x tensor .* not empty"),
        (dict(out=out[:0]), "out tensor .* not empty"),
        (dict(x=torch.zeros(3, 65)), "last dimension of the x tensor is 65, above the descriptor's length 64"),
        (dict(y=torch.zeros(3, 65)), "last dimension of the y tensor is 65"),
        (dict(out=torch.zeros(3, 65)), "last dimension of the out tensor is 65"),
        (dict(x=torch.zeros(3, 126)[:, ::2]), "x tensor needs unit inner stride, got 2"),
        (dict(y=torch.zeros(3, 66)[:, ::2]), "y tensor needs unit inner stride"),
        (dict(out=torch.zeros(3, 128)[:, ::2]), "out tensor needs unit inner stride"),
        (dict(x=x[:2]), "2 rows of x, 3 rows of y, 3 rows of out: the row counts must be equal"),
        (dict(y=y[0]), "3 rows of x, 1 rows of y, 3 rows of out"), (dict(out=out[:1]), "3 rows of x, 3 rows of y, 1 rows of out"),
        (dict(x=torch.zeros(200).as_strided((3, 63), (60, 1))), "rows of the x tensor overlap .stride 60 below the length 63"),
        (dict(out=torch.zeros(200).as_strided((3, 64), (63, 1))), "rows of the out tensor overlap"),
        (dict(phat_floor=0), "phat_floor 0 must be None"), (dict(phat_floor=0.0), "phat_floor 0.0 must be None"),
        (dict(phat_floor=-1), "phat_floor -1 must be None"), (dict(phat_floor=float("nan")), "phat_floor nan"),
        (dict(phat_floor=float("inf")), "phat_floor inf"), (dict(phat_floor=1e-50), "phat_floor 1e-50 .* normal number"),
        (dict(phat_floor=1e39), "phat_floor 1e\\+39"),
        (dict(x=x.numpy()), "torch tensors"),
        (dict(), "x tensor is not in device memory"),
        (dict(phat_floor=1e-3), "x tensor is not in device memory"),
        (dict(phat_floor=1.2e-38), "not in device memory"),
    )
    for change, text in cases:
        kw = dict(x=x, y=y, out=out, phat_floor=None)
        kw.update(change)
        with pytest.raises(pf.invalid_configuration, match=text):
            p.correlate_pairs(kw["x"], kw["y"], kw["out"], phat_floor=kw["phat_floor"])
        if kw["phat_floor"] is None:
            with pytest.raises(pf.invalid_configuration, match=text.replace("correlate", "convolve")):
                p.convolve_pairs(kw["x"], kw["y"], kw["out"])
    # convolve_pairs has no floor
    with pytest.raises(TypeError):
        p.convolve_pairs(x, y, out, phat_floor=1e-3)
    # accepted shapes get as far as the device check: one row as 1-D tensors, pitched rows, the same tensor twice, one scalar
    for kw in (dict(x=x[0], y=y[0], out=out[0]), dict(x=torch.zeros(3, 70)[:, :63]), dict(out=torch.zeros(3, 67)[:, :1]),
               dict(y=x), dict(x=torch.zeros(3, 1)), dict(x=torch.zeros(3, 64), y=torch.zeros(3, 64))):
        full = dict(x=x, y=y, out=out)
        full.update(kw)
        with pytest.raises(pf.invalid_configuration, match="not in device memory"):
            p.correlate_pairs(full["x"], full["y"], full["out"])
    p64, _ = _shell(True, "f64", 128)
    d = torch.zeros(2, 128, dtype=torch.float64)
    with pytest.raises(pf.invalid_configuration, match="dtype .* x tensor"):
        p64.correlate_pairs(torch.zeros(2, 128), d, d.clone())
    with pytest.raises(pf.invalid_configuration, match="not in device memory"):
        p64.correlate_pairs(d, d, d.clone(), phat_floor=1e-50)  # a normal number in double
    with pytest.raises(pf.invalid_configuration, match="phat_floor 1e-310"):
        p64.correlate_pairs(d, d, d.clone(), phat_floor=1e-310)
