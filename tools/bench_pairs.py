#!/usr/bin/env python3
"""Fused correlation of pairs of REAL rows against what a user has without it, on the same device, in one process.

    python tools/bench_pairs.py [--reps 15] [--warmup 3] [--gib 1.0] [--cases f32:2048,f32:8192,...] [--out DIR]

For every (precision, N) five candidates are timed alternately (a, b, c, d, e, a, ...), each rep bracketed by HIP events
on the plans' stream after a warm-up, at the same batch (about --gib GiB of input in x and y together, a multiple of 64
rows):
  (a) fused          pf.real_descriptor(N).commit().correlate_pairs(x, y, r): one kernel, 2 N scalars in, N out
  (b) fused_phat     the same with phat_floor (GCC-PHAT)
  (c) composed       what exists without the feature (the yardstick): two compute_forward (R2C) of the same plan, a torch
                     multiply with the conjugate, compute_backward (C2R)
  (d) composed_phat  the same with abs, clamp to the floor and divide between the multiply and the C2R
  (e) r2c            one compute_forward of that plan   (context)
Reported: the median and the min / max of the reps in microseconds, the ratios composed / fused, and for the fused verbs
the algorithmic HBM fraction 3 * N * scalar bytes * batch / time over 8 TB/s.  `gate`: fused beats composed by more than
the spread (max - min) of the composed route's reps; a case that misses it is recorded and named, not dropped.  One sampled
row of each of the four outputs is checked against NumPy in double precision (all must pass: a wrong yardstick is no
yardstick).  One JSON line per case; --out DIR also writes them to DIR/bench_pairs.json.
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

DEFAULT_CASES = "f32:512,f32:2048,f32:8192,f32:16384,f32:12000,f64:2048,f64:8192"
HBM_PEAK = 8e12  # bytes / s


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--gib", type=float, default=1.0, help="GiB of real input (x and y together) per execute")
    ap.add_argument("--cases", default=DEFAULT_CASES, help="comma-separated PRECISION:N")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    import portfft_amd as pf
    if not torch.cuda.is_available():
        sys.exit("bench_pairs.py needs a GPU")
    torch.cuda.set_device(0)
    stream = torch.cuda.current_stream()
    lines = []
    for case in a.cases.split(","):
        prec, n = case.split(":")
        n = int(n)
        bins = n // 2 + 1
        sb = 4 if prec == "f32" else 8
        rt, ct = (torch.float32, torch.complex64) if prec == "f32" else (torch.float64, torch.complex128)
        batch = max(64, int(a.gib * 2 ** 30 / (2 * n * sb)) // 64 * 64)
        d = pf.real_descriptor(n, prec)
        d.number_of_transforms = batch
        plan = d.commit(stream)
        plan.prepare_pairs()
        x = torch.empty(batch, n, dtype=torch.float64, device="cuda").uniform_(-1, 1).to(rt)
        y = torch.empty(batch, n, dtype=torch.float64, device="cuda").uniform_(-1, 1).to(rt)
        # the floor: the median |P| of a sampled row, so that both branches of the phase transform are live
        pick = batch // 2 + 1
        xr, yr = x[pick].cpu().numpy().astype(np.float64), y[pick].cpu().numpy().astype(np.float64)
        p_ref = np.fft.rfft(xr) * np.conj(np.fft.rfft(yr))
        floor = float(np.float32(np.median(np.abs(p_ref))))
        outs = {k: torch.empty(batch, n, dtype=rt, device="cuda") for k in ("fused", "fused_phat", "composed", "composed_phat")}
        sx = torch.empty(batch, bins, dtype=ct, device="cuda")
        sy = torch.empty(batch, bins, dtype=ct, device="cuda")
        mag = torch.empty(batch, bins, dtype=rt, device="cuda")

        def run_fused():
            plan.correlate_pairs(x, y, outs["fused"], want_event=False)

        def run_fused_phat():
            plan.correlate_pairs(x, y, outs["fused_phat"], phat_floor=floor, want_event=False)

        def spectra():
            plan.compute_forward(x.view(-1), sx.view(-1), want_event=False)
            plan.compute_forward(y.view(-1), sy.view(-1), want_event=False)
            torch.mul(sx, sy.conj(), out=sx)

        def run_composed():
            spectra()
            plan.compute_backward(sx.view(-1), outs["composed"].view(-1), want_event=False)

        def run_composed_phat():
            spectra()
            torch.abs(sx, out=mag)
            mag.clamp_(min=floor)
            sx.div_(mag)
            plan.compute_backward(sx.view(-1), outs["composed_phat"].view(-1), want_event=False)

        def run_r2c():
            plan.compute_forward(x.view(-1), sy.view(-1), want_event=False)

        cands = (("fused", run_fused), ("fused_phat", run_fused_phat), ("composed", run_composed),
                 ("composed_phat", run_composed_phat), ("r2c", run_r2c))
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
        refs = {"plain": n * np.fft.irfft(p_ref, n), "phat": n * np.fft.irfft(p_ref / np.maximum(np.abs(p_ref), floor), n)}
        kappa = np.sqrt(2.0) * np.abs(p_ref).max() / floor
        tau = 2e-6 if prec == "f32" else 5e-15
        errs, ok = {}, True
        for name, out in outs.items():
            ref = refs["phat" if name.endswith("phat") else "plain"]
            got = out[pick].cpu().numpy().astype(np.float64)
            errs[name] = float(np.linalg.norm(got - ref) / np.linalg.norm(ref))
            ok = ok and errs[name] <= (kappa + 1 if name.endswith("phat") else 1) * tau
        dim = plan.info().dims[0]
        rec = {"precision": prec, "n": n, "batch": batch, "reps": a.reps, "phat_floor": floor, "check_rel_l2": errs,
               "check_ok": bool(ok), "factors": [int(v) for v in dim.factors[:dim.n_factors]],
               "ffts_per_workgroup": int(dim.ffts_per_workgroup)}
        for name, _ in cands:
            t = times[name]
            rec[name] = {"median_us": round(statistics.median(t), 1), "min_us": round(min(t), 1), "max_us": round(max(t), 1)}
        for fused, comp in (("fused", "composed"), ("fused_phat", "composed_phat")):
            f_us, c = rec[fused]["median_us"], rec[comp]
            rec["gate_" + fused] = bool(c["median_us"] - f_us > c["max_us"] - c["min_us"])
            rec[comp + "_over_" + fused + "_time"] = round(c["median_us"] / f_us, 3)
            rec[fused + "_over_r2c_time"] = round(f_us / rec["r2c"]["median_us"], 3)
            rec[fused + "_hbm_fraction"] = round(3 * n * sb * batch / (f_us * 1e-6) / HBM_PEAK, 4)
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        del plan, x, y, outs, sx, sy, mag
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "bench_pairs.json"), "w") as f:
            json.dump(lines, f, indent=1)
    if not all(r["check_ok"] for r in lines):
        sys.exit("bench_pairs.py: a sampled fused or composed output failed the accuracy check")
    missed = ["%s N=%d %s" % (r["precision"], r["n"], k[5:]) for r in lines for k in ("gate_fused", "gate_fused_phat") if not r[k]]
    print("gate: %d of %d cases pass%s" % (2 * len(lines) - len(missed), 2 * len(lines),
                                           "; missed by " + ", ".join(missed) if missed else ""))


if __name__ == "__main__":
    main()
