#!/usr/bin/env python3
"""Overlap-save FIR filtering of REAL signals in one kernel against the best a user has without it, on the same device,
in one process.

    python tools/bench_rfilter.py [--reps 15] [--warmup 3] [--gib 1.0] [--cases f32:2048:129,...] [--out DIR]

For every (precision, N, K): `signals` real signals of L samples (about --gib GiB in all), filtered to as many outputs of
L samples (the causal linear convolution, one shared filter).  Three candidates are timed alternately (a, b, c, a, ...),
each rep bracketed by HIP events on the plans' stream after a warm-up:
  (a) fused     plan.filter of a pf.real_convolution_descriptor(N) plan: one kernel on the real signals
  (b) composed  the best that exists without the feature (the yardstick): an interleave copy of two real signals into
                one complex signal, plan.filter of a pf.convolution_descriptor plan on the signals / 2 complex signals
                (real taps: the two parts are filtered independently), and a de-interleave copy; both copies are timed.
                The complex plan has the real plan's N where that commits, otherwise N / 2 (reported as complex_n)
  (c) cfilter   the complex plan.filter of (b) alone: the same byte count through the complex kernel (context)
Reported: the median and the min / max of the reps in microseconds, the ratios composed / fused and fused / cfilter, and
for the fused verb the algorithmic HBM fraction (in_length + out_length) * scalar bytes * signals / time over 8 TB/s.
`gate`: fused beats composed by more than the spread (max - min) of the composed route's reps.  A window at the front of
one signal, one in its middle and its last samples are checked against np.convolve in double precision, for the fused
and for the composed output (both must pass: a wrong yardstick is no yardstick).  One JSON line per case; --out DIR also
writes them to DIR/bench_rfilter.json.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
os.environ.setdefault("PFFT_JIT_CACHE_DIR", os.path.join(ROOT, "build", "jit_cache"))
sys.path.insert(0, ROOT)

DEFAULT_CASES = "f32:2048:129,f32:8192:513,f32:16384:1025,f32:12000:1001,f64:2048:129,f64:8192:513"
HBM_PEAK = 8e12  # bytes / s
SIGNALS = 64


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--gib", type=float, default=1.0, help="GiB of real signal per execute")
    ap.add_argument("--cases", default=DEFAULT_CASES, help="comma-separated PRECISION:N:K")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    import portfft_amd as pf
    if not torch.cuda.is_available():
        sys.exit("bench_rfilter.py needs a GPU")
    torch.cuda.set_device(0)
    stream = torch.cuda.current_stream()
    lines = []
    for case in a.cases.split(","):
        prec, n, k = case.split(":")
        n, k = int(n), int(k)
        hop = n - (k & ~1)  # the real kernel's even geometry (convolve)
        sb = 4 if prec == "f32" else 8
        rt, ct = (torch.float32, torch.complex64) if prec == "f32" else (torch.float64, torch.complex128)
        ns = SIGNALS
        seg = max(1, int(a.gib * 2 ** 30 / (ns * sb)) // hop)
        length = seg * hop
        plan = pf.real_convolution_descriptor(n, prec).commit(stream)
        complex_n = n
        try:
            cplan = pf.convolution_descriptor([complex_n], prec).commit(stream)
        except pf.unsupported_configuration:
            complex_n = n // 2
            cplan = pf.convolution_descriptor([complex_n], prec).commit(stream)
        taps = (torch.empty(k, dtype=torch.float64, device="cuda").uniform_(-1, 1) / k ** 0.5).to(rt)
        plan.set_filter_taps(taps)
        cplan.set_filter_taps(taps.to(ct))
        x = torch.empty(ns, length, dtype=torch.float64, device="cuda").uniform_(-1, 1).to(rt)
        y_fused = torch.empty(ns, length, dtype=rt, device="cuda")
        y_comp = torch.empty(ns, length, dtype=rt, device="cuda")
        xc = torch.empty(ns // 2, length, dtype=ct, device="cuda")
        yc = torch.empty(ns // 2, length, dtype=ct, device="cuda")

        def run_fused():
            plan.filter(x, y_fused, want_event=False)

        def run_composed():
            torch.view_as_real(xc).copy_(x.view(ns // 2, 2, length).transpose(1, 2))  # signals 2i, 2i + 1 -> re, im
            cplan.filter(xc, yc, want_event=False)
            y_comp.view(ns // 2, 2, length).copy_(torch.view_as_real(yc).transpose(1, 2))

        def run_cfilter():
            cplan.filter(xc, yc, want_event=False)

        cands = (("fused", run_fused), ("composed", run_composed), ("cfilter", run_cfilter))
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        times = {name: [] for name, _ in cands}
        for rep in range(a.warmup + a.reps):
            for name, fn in cands:
                ev[0].record(stream)
                fn()
                ev[1].record(stream)
                ev[1].synchronize()
                if rep >= a.warmup:
                    times[name].append(ev[0].elapsed_time(ev[1]) * 1e3)  # us
        torch.cuda.synchronize()
        pick = ns // 2 + 1
        xr = x[pick].cpu().numpy().astype(np.float64)
        hr = taps.cpu().numpy().astype(np.float64)
        span = min(length, 2 * hop)
        starts = sorted({0, (seg // 2) * hop - span // 2 if seg > 2 else 0, length - span})
        errs = {"fused": 0.0, "composed": 0.0}
        for s0 in starts:
            lo = max(0, s0 - (k - 1))
            ref = n * np.convolve(xr[lo:s0 + span], hr)[s0 - lo:s0 - lo + span]
            # (the composed route's factor is the complex plan's N)
            for name, out, c in (("fused", y_fused, 1.0), ("composed", y_comp, n / complex_n)):
                got = c * out[pick, s0:s0 + span].cpu().numpy().astype(np.float64)
                errs[name] = max(errs[name], float(np.linalg.norm(got - ref) / np.linalg.norm(ref)))
        tol = 2e-6 if prec == "f32" else 5e-15
        dim = plan.info().dims[0]
        rec = {"precision": prec, "n": n, "taps": k, "hop": hop, "signals": ns, "length": length, "rows": ns * seg,
               "complex_n": complex_n, "reps": a.reps, "check_rel_l2": errs,
               "check_ok": bool(errs["fused"] <= tol and errs["composed"] <= tol),
               "factors": [int(v) for v in dim.factors[:dim.n_factors]]}
        for name, _ in cands:
            t = times[name]
            rec[name] = {"median_us": round(statistics.median(t), 1), "min_us": round(min(t), 1), "max_us": round(max(t), 1)}
        f_us, comp = rec["fused"]["median_us"], rec["composed"]
        rec["gate"] = bool(comp["median_us"] - f_us > comp["max_us"] - comp["min_us"])
        rec["composed_over_fused_time"] = round(comp["median_us"] / f_us, 3)
        rec["fused_over_cfilter_time"] = round(f_us / rec["cfilter"]["median_us"], 3)
        rec["fused_hbm_fraction"] = round(2 * length * sb * ns / (f_us * 1e-6) / HBM_PEAK, 4)
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        del plan, cplan, x, y_fused, y_comp, xc, yc
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "bench_rfilter.json"), "w") as f:
            json.dump(lines, f, indent=1)
    if not all(r["check_ok"] for r in lines):
        sys.exit("bench_rfilter.py: a sampled fused or composed output failed the accuracy check")
    if not all(r["gate"] for r in lines):
        sys.exit("bench_rfilter.py: the fused verb did not beat the composed route at every case")


if __name__ == "__main__":
    main()
