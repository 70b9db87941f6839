#!/usr/bin/env python3
"""Fused circular convolution of REAL rows against what a user has without it, on the same device, in one process.

    python tools/bench_rconv.py [--reps 15] [--warmup 3] [--gib 1.0] [--cases f32:2048,f32:8192,...] [--out DIR]

For every (precision, N), with one shared filter, three candidates are timed alternately (a, b, c, a, ...), each rep
bracketed by HIP events on the plans' stream after a warm-up, at the same batch (about --gib GiB of real input, a
multiple of 64):
  (a) fused     pf.real_convolution_descriptor(N).commit().convolve: one kernel, N scalars in, N scalars out
  (b) composed  what exists without the feature (the yardstick): compute_forward (R2C) of a pf.real_descriptor plan, an
                in-place torch multiply with the half spectrum, compute_backward (C2R)
  (c) r2c       one compute_forward of that real plan   (context)
Reported: the median and the min / max of the reps in microseconds, the ratios composed / fused and fused / r2c, and for
the fused verb the algorithmic HBM fraction 2 * N * scalar bytes * batch / time over 8 TB/s.  `gate`: fused beats composed
by more than the spread (max - min) of the composed route's reps.  One sampled row of the fused and of the composed output
is checked against NumPy in double precision (both must pass: a wrong yardstick is no yardstick).  One JSON line per
case; --out DIR also writes them to DIR/bench_rconv.json.
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

DEFAULT_CASES = "f32:2048,f32:8192,f32:16384,f32:12000,f64:2048,f64:8192"
HBM_PEAK = 8e12  # bytes / s


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--gib", type=float, default=1.0, help="GiB of real input per execute")
    ap.add_argument("--cases", default=DEFAULT_CASES, help="comma-separated PRECISION:N")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    import portfft_amd as pf
    if not torch.cuda.is_available():
        sys.exit("bench_rconv.py needs a GPU")
    torch.cuda.set_device(0)
    stream = torch.cuda.current_stream()
    lines = []
    for case in a.cases.split(","):
        prec, n = case.split(":")
        n = int(n)
        bins = n // 2 + 1
        sb = 4 if prec == "f32" else 8
        rt, ct = (torch.float32, torch.complex64) if prec == "f32" else (torch.float64, torch.complex128)
        batch = max(64, int(a.gib * 2 ** 30 / (n * sb)) // 64 * 64)
        d = pf.real_convolution_descriptor(n, prec)
        d.number_of_transforms = batch
        plan = d.commit(stream)
        r = pf.real_descriptor(n, prec)  # what the parent offers
        r.number_of_transforms = batch
        real = r.commit(stream)
        x = torch.empty(batch * n, dtype=torch.float64, device="cuda").uniform_(-1, 1).to(rt)
        h = torch.view_as_complex(torch.empty(bins, 2, dtype=torch.float64, device="cuda").uniform_(-1, 1)).to(ct)
        plan.set_filter(h)
        y_fused = torch.empty_like(x)
        y_comp = torch.empty_like(x)
        spec = torch.empty(batch * bins, dtype=ct, device="cuda")
        spec_c = torch.empty(batch * bins, dtype=ct, device="cuda")

        def run_fused():
            plan.convolve(x, y_fused, want_event=False)

        def run_composed():
            real.compute_forward(x, spec, want_event=False)
            spec.view(batch, bins).mul_(h)
            real.compute_backward(spec, y_comp, want_event=False)

        def run_r2c():
            real.compute_forward(x, spec_c, want_event=False)

        cands = (("fused", run_fused), ("composed", run_composed), ("r2c", run_r2c))
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        times = {k: [] for k, _ in cands}
        for rep in range(a.warmup + a.reps):
            for name, fn in cands:
                ev[0].record(stream)
                fn()
                ev[1].record(stream)
                ev[1].synchronize()
                if rep >= a.warmup:
                    times[name].append(ev[0].elapsed_time(ev[1]) * 1e3)  # us
        torch.cuda.synchronize()
        pick = batch // 2 + 1
        xr = x[pick * n:(pick + 1) * n].cpu().numpy().astype(np.float64)
        hr = h.cpu().numpy().astype(np.complex128)
        hr[0], hr[-1] = hr[0].real, hr[-1].real
        ref = n * np.fft.irfft(np.fft.rfft(xr) * hr, n)
        errs = {}
        for name, out in (("fused", y_fused), ("composed", y_comp)):
            got = out[pick * n:(pick + 1) * n].cpu().numpy().astype(np.float64)
            errs[name] = float(np.linalg.norm(got - ref) / np.linalg.norm(ref))
        tol = 2e-6 if prec == "f32" else 5e-15
        dim = plan.info().dims[0]
        rec = {"precision": prec, "n": n, "batch": batch, "reps": a.reps, "check_rel_l2": errs,
               "check_ok": bool(errs["fused"] <= tol and errs["composed"] <= tol),
               "factors": [int(v) for v in dim.factors[:dim.n_factors]]}
        for name, _ in cands:
            t = times[name]
            rec[name] = {"median_us": round(statistics.median(t), 1), "min_us": round(min(t), 1), "max_us": round(max(t), 1)}
        f_us, comp = rec["fused"]["median_us"], rec["composed"]
        rec["gate"] = bool(comp["median_us"] - f_us > comp["max_us"] - comp["min_us"])
        rec["composed_over_fused_time"] = round(comp["median_us"] / f_us, 3)
        rec["fused_over_r2c_time"] = round(f_us / rec["r2c"]["median_us"], 3)
        rec["fused_hbm_fraction"] = round(2 * n * sb * batch / (f_us * 1e-6) / HBM_PEAK, 4)
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        del plan, real, x, h, y_fused, y_comp, spec, spec_c
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "bench_rconv.json"), "w") as f:
            json.dump(lines, f, indent=1)
    if not all(r["check_ok"] for r in lines):
        sys.exit("bench_rconv.py: a sampled fused or composed output failed the accuracy check")
    if not all(r["gate"] for r in lines):
        sys.exit("bench_rconv.py: the fused verb did not beat the composed route at every length")


if __name__ == "__main__":
    main()
