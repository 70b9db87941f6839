"""helpers.ODD_RADIX_LENGTHS without a GPU: the host planner (choose_spec_params, through build/jit_planner_test "plan") is
asked for every row of the table and must give the configuration the row's class is named for -- the property itself, not
a recorded radix list: first radix odd, M odd, the number of passes, the largest radix, the lanes per transform, a ragged
pass, the padding (helpers.odd_radix_class_miss).  test_gpu_odd_radix.py runs every fused verb on these lengths and asserts
the same property on plan.info(); a planner change that moves a length out of its class fails here first.

Also: the hop test_gpu_odd_radix.py gives the stft-style verbs is odd and coprime to N = 2M at every row; and what the
predicate refuses, so that it cannot pass everything."""
import math
import re
import subprocess

import pytest

import helpers as H
from test_jit_planner import EXE, _build

ROWS = [(p, m, cls) for p in ("f32", "f64") for m, cls in H.ODD_RADIX_LENGTHS[p] + H.ODD_RADIX_61[p]]
CLASSES = ["work-item odd prime", "work-item odd composite", "work-item even", "all radices odd", "odd prime power",
           "odd first radix", "composite radix", "prime lanes M/P, P", "prime lanes P, rest", "prime lanes odd M",
           "lanes no power of two"]
FP32_ONLY = {"composite radix", "prime lanes P, rest", "prime lanes odd M"}  # (the table's comment says why)

_plans = {}


def planned(prec, m):
    """{radices, lanes, fpw, wg, pads, staged, regs} of the packed planner's choice for an M-point transform"""
    if not _plans:
        _build()
        for p in ("f32", "f64"):
            ms = sorted({m_ for p_, m_, _ in ROWS if p_ == p})
            out = subprocess.run([EXE, "plan", p] + [str(v) for v in ms], capture_output=True, text=True, timeout=60, check=True).stdout
            for ln in out.splitlines():
                f = re.match(r"plan (\w+) n=(\d+) radices=([\dx]+) lanes=(\d+) fpw=(\d+) wg=(\d+) pads=(\d+) staged=(\d+) regs=(\d+)$", ln)
                assert f, ln
                _plans[f[1], int(f[2])] = dict(radices=[int(v) for v in f[3].split("x")], lanes=int(f[4]), fpw=int(f[5]),
                                               wg=int(f[6]), pads=int(f[7]), staged=int(f[8]), regs=int(f[9]))
    return _plans[prec, m]


def test_every_class_has_a_row():
    for prec in ("f32", "f64"):
        have = {cls for _, cls in H.ODD_RADIX_LENGTHS[prec]}
        want = set(CLASSES) - (FP32_ONLY if prec == "f64" else set())
        assert have == want, (prec, sorted(want - have), sorted(have - want))
        ms = [m for m, _ in H.ODD_RADIX_LENGTHS[prec]]
        assert len(ms) == len(set(ms)) and max(ms) <= 2500


@pytest.mark.parametrize("prec,m,cls", ROWS)
def test_the_planner_gives_the_row_its_class(prec, m, cls):
    p = planned(prec, m)
    print("%s M=%d %s: %s" % (prec, m, cls, p))
    assert p["wg"] == p["lanes"] * p["fpw"]
    miss = H.odd_radix_class_miss(cls, m, p["radices"], p["lanes"], p["fpw"], p["pads"])
    assert miss is None, miss
    # no "+1 per 16" padding anywhere in the table but the padded pitch of the even work-item row
    assert p["pads"] == (m if cls == "work-item even" else 0)


@pytest.mark.parametrize("prec,m,cls", ROWS)
def test_the_hop_is_odd_and_coprime_to_n(prec, m, cls):
    """(the hop of test_gpu_isolation.py, N / 4 + 1 made odd, is 9 at N = 30: helpers.odd_radix_hop steps on from there)"""
    n = 2 * m
    hop = H.odd_radix_hop(n)
    assert hop % 2 == 1 and math.gcd(hop, n) == 1 and n // 4 < hop < n, (n, hop)


def test_the_predicate_refuses_a_neighbouring_class():
    """every row's configuration under every other class name: refused, except where two classes really overlap"""
    overlap = {("odd prime power", "lanes no power of two"), ("lanes no power of two", "odd prime power"),
               ("all radices odd", "lanes no power of two"), ("odd first radix", "lanes no power of two"),
               ("composite radix", "lanes no power of two"), ("prime lanes P, rest", "odd first radix")}
    for prec, m, cls in ROWS:
        p = planned(prec, m)
        for other in CLASSES:
            if other == cls or (cls, other) in overlap:
                continue
            assert H.odd_radix_class_miss(other, m, p["radices"], p["lanes"], p["fpw"], p["pads"]) is not None, (prec, m, cls, other)
    assert "unknown class" in H.odd_radix_class_miss("no such class", 7, [7], 1, 256, 0)
    assert "do not multiply" in H.odd_radix_class_miss("work-item odd prime", 7, [5], 1, 256, 0)
