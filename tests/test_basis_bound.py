"""The derived per-element bound on the transform of a unit impulse (helpers.check_basis_rows), held against correct
implementations on the CPU: the committed oracle in fp32 and fp64, forward and backward, and scipy.fft in single and
double precision for the real and DCT bounds.  The bound is not fitted to any of them: every output element of the
transform of e_j is a product of at most helpers.twiddle_path_length twiddles, each multiply within 3.3 u.

Complex (oracle): the full N x N identity at one length per path up to 4096, 40 rows at 8192, 65536 and 68640, and the
prime lengths 37 and 61 * 16 planned with a sub-group of 64.  Real and DCT (scipy): the full identity up to 1024, 40 rows
above.  The test prints the worst ratio of every family and asserts that each stays below 0.6: a correct implementation
has honest headroom under the bound the GPU kernels are held to (measured: oracle fp32 <= 0.16, fp64 <= 0.53, scipy
0.03 - 0.14).  Every M of helpers.ODD_RADIX_LENGTHS and N = 2M run too; on those the oracle is held to the bound itself
(measured: fp32 0.19, fp64 0.67 at 243 = 3^5) and scipy stays below 0.17."""
import numpy as np
import pytest

import helpers as H

FULL = [2, 3, 4, 8, 13, 16, 30, 64, 96, 100, 256, 1000, 1024, 1536, 2048, 4096]
SAMPLED = [8192, 65536, 68640]
HEADROOM = 0.6


def sampled_rows(n, count=40, seed=0):
    """the ends, the middle and seeded random rows"""
    fixed = [0, 1, 2, 3, n // 2 - 1, n // 2, n // 2 + 1, n - 2, n - 1]
    rng = np.random.default_rng(seed + n)
    return np.unique(np.concatenate([fixed, rng.integers(0, n, count - len(fixed))]) % n)


def _oracle_rows(oracle, n, rows, prec, direction, sg):
    x = np.zeros((len(rows), n), dtype=np.complex64 if prec == "f32" else np.complex128)
    x[np.arange(len(rows)), rows] = 1
    out = oracle.compute(oracle.make_desc([n], prec, batch=len(rows)), direction, x.ravel(), sg=sg, threads=4)
    return out.reshape(len(rows), n)


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_the_oracle_stays_inside_the_complex_bound(oracle, prec):
    worst = 0.0
    cases = [(n, np.arange(n), oracle.DEFAULT_SG) for n in FULL] + [(n, sampled_rows(n), oracle.DEFAULT_SG) for n in SAMPLED]
    cases += [(37, np.arange(37), 64), (61 * 16, np.arange(61 * 16), 64)]
    # every M of the odd-radix table (helpers.ODD_RADIX_LENGTHS): P(M) with odd primes of multiplicity up to 5 (243), three
    # different odd primes (1001) and primes above 31 (37, 1369, 976), which the oracle plans with a sub-group of 64.  These
    # are held to the bound itself, which is what the GPU kernels are held to; the headroom below is a record of the
    # lengths above (the oracle runs 243 = 3^5 as five radix-3 passes: measured fp32 0.19, fp64 0.67 of the bound).
    done = {n for n, _, _ in cases}
    table = [(m, np.arange(m) if m <= 1024 else sampled_rows(m), 64 if any(m % p == 0 for p in (37, 43, 47, 61)) else oracle.DEFAULT_SG)
             for m in H.ODD_RADIX_M if m not in done]
    worst_table = 0.0
    for n, rows, sg in cases + table:
        for direction in (oracle.FORWARD, oracle.BACKWARD):
            got = _oracle_rows(oracle, n, rows, prec, direction, sg)
            ratio = H.check_basis_rows(got, rows, n, "c2c", prec, direction=direction,
                                       what="oracle sg=%d %s" % (sg, "fwd" if direction == oracle.FORWARD else "bwd"))
            if n in {m for m, _, _ in table}:
                worst_table = max(worst_table, ratio)
            else:
                worst = max(worst, ratio)
    print("oracle %s: worst ratio to the bound %.3f, on the odd-radix table %.3f" % (prec, worst, worst_table))
    assert worst < HEADROOM and worst_table <= 1.0


REAL_LENGTHS = [4, 6, 8, 30, 64, 592, 1000, 1024, 4096, 20000]
REAL_LENGTHS += [2 * m for m in H.ODD_RADIX_M if 2 * m not in REAL_LENGTHS]  # N = 2M of the odd-radix table: P(M) + 3 or 4


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_scipy_stays_inside_the_real_and_dct_bounds(prec):
    sf = pytest.importorskip("scipy.fft")
    rt = np.float32 if prec == "f32" else np.float64
    worst = {}
    for n in REAL_LENGTHS:
        rows = np.arange(n) if n <= 1024 else sampled_rows(n)
        eye = np.zeros((rows.size, n), dtype=rt)
        eye[np.arange(rows.size), rows] = 1
        bins = rows[rows <= n // 2]
        spec = np.zeros((bins.size, n // 2 + 1), dtype=np.complex64 if prec == "f32" else np.complex128)
        spec[np.arange(bins.size), bins] = 1
        runs = {"r2c": (sf.rfft(eye, axis=1), rows), "c2r": (sf.irfft(spec, n, axis=1, norm="forward"), bins),
                "dct2": (sf.dct(eye, 2, axis=1), rows), "dct3": (sf.dct(eye, 3, axis=1), rows),
                "dct4": (sf.dct(eye, 4, axis=1), rows)}
        for kind, (got, r) in runs.items():
            assert got.dtype == (spec.dtype if kind == "r2c" else rt), (kind, got.dtype)
            worst[kind] = max(worst.get(kind, 0.0), H.check_basis_rows(got, r, n, kind, prec, what="scipy"))
    print("scipy %s: worst ratio to the bound %s" % (prec, {k: round(v, 3) for k, v in worst.items()}))
    assert max(worst.values()) < HEADROOM
