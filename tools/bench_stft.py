#!/usr/bin/env python3
"""The short-time Fourier transform of real signals in one kernel against the best a user has without it, on the same
device, in one process.

    python tools/bench_stft.py [--reps 15] [--warmup 3] [--gib 2.0] [--cases f32:512:128,...] [--out FILE]

For every (precision, N, hop): 16 real signals whose frames of N scalars every `hop` scalars (lead 0, every frame inside
its signal, periodic Hann window) make about --gib GiB of bins.  Three candidates are timed alternately (a, b, c, a, ...),
each rep bracketed by HIP events on the plan's stream after a warm-up, all on ONE plan of pf.real_descriptor(N):
  (a) fused     plan.stft: one kernel, straight from the signals
  (b) composed  the best that exists without the feature (the yardstick): one torch gather-and-multiply of the
                overlapping frames into a frame buffer of rows * N scalars, and compute_forward of the plan on it
  (c) r2c       compute_forward alone on the pre-gathered frames: the floor -- the same stores as (a), which reads N / hop
                times fewer distinct input bytes (through L2) but addresses and windows them itself
Reported: the median and the min / max of the reps in microseconds, the ratios composed / fused and fused / r2c, and for
the fused verb the algorithmic HBM fraction (signal bytes + bin bytes) / time over 8 TB/s.  `gate`: fused beats composed
by more than the spread (max - min) of the composed route's reps.  The first, a middle and the last frame of one signal
are checked against np.fft.rfft in double precision, for the fused and for the composed output (both must pass: a wrong
yardstick is no yardstick).  One JSON line per case on stdout; the table goes to --out (default profiles/stft_bench.txt).
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

DEFAULT_CASES = ("f32:512:128,f32:512:256,f32:1024:256,f32:1024:512,f32:4096:1024,f32:4096:2048,f32:16384:4096,"
                 "f32:16384:8192,f64:1024:256,f64:1024:512,f64:8192:2048,f64:8192:4096")
HBM_PEAK = 8e12  # bytes / s
SIGNALS = 16


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--gib", type=float, default=2.0, help="GiB of bins per execute")
    ap.add_argument("--cases", default=DEFAULT_CASES, help="comma-separated PRECISION:N:HOP")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stft_bench.txt"))
    a = ap.parse_args()

    import torch
    import portfft_amd as pf
    if not torch.cuda.is_available():
        sys.exit("bench_stft.py needs a GPU")
    torch.cuda.set_device(0)
    stream = torch.cuda.current_stream()
    lines = []
    for case in a.cases.split(","):
        prec, n, hop = case.split(":")
        n, hop = int(n), int(hop)
        m = n // 2
        sb = 4 if prec == "f32" else 8
        rt, ct = (torch.float32, torch.complex64) if prec == "f32" else (torch.float64, torch.complex128)
        ns = SIGNALS
        frames = max(1, int(a.gib * 2 ** 30 / (ns * (m + 1) * 2 * sb)))
        length = (frames - 1) * hop + n
        rows = ns * frames
        d = pf.real_descriptor(n, prec)
        d.number_of_transforms = rows
        plan = d.commit(stream)
        w = (0.5 - 0.5 * torch.cos(2 * np.pi * torch.arange(n, dtype=torch.float64, device="cuda") / n)).to(rt)
        plan.set_window(w)
        x = torch.empty(ns, length, dtype=torch.float64, device="cuda").uniform_(-1, 1).to(rt)
        y_fused = torch.empty(ns, frames, m + 1, dtype=ct, device="cuda")
        y_comp = torch.empty(ns, frames, m + 1, dtype=ct, device="cuda")
        fbuf = torch.empty(ns, frames, n, dtype=rt, device="cuda")
        windows = x.unfold(-1, n, hop)  # (ns, frames, n): overlapping views of the signals

        def run_fused():
            plan.stft(x, y_fused, hop, want_event=False)

        def run_composed():
            torch.mul(windows, w, out=fbuf)
            plan.compute_forward(fbuf.view(-1), y_comp.view(-1), want_event=False)

        def run_r2c():
            plan.compute_forward(fbuf.view(-1), y_comp.view(-1), want_event=False)

        cands = (("fused", run_fused), ("composed", run_composed), ("r2c", run_r2c))
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
        wd = w.cpu().numpy().astype(np.float64)
        errs = {"fused": 0.0, "composed": 0.0}
        for f in sorted({0, frames // 2, frames - 1}):
            ref = np.fft.rfft(x[pick, f * hop:f * hop + n].cpu().numpy().astype(np.float64) * wd)
            for name, out in (("fused", y_fused), ("composed", y_comp)):
                got = out[pick, f].cpu().numpy().astype(np.complex128)
                errs[name] = max(errs[name], float(np.linalg.norm(got - ref) / np.linalg.norm(ref)))
        tol = 2e-6 if prec == "f32" else 5e-15
        dim = plan.info().dims[0]
        rec = {"precision": prec, "n": n, "hop": hop, "signals": ns, "frames": frames, "length": length, "rows": rows,
               "reps": a.reps, "check_rel_l2": errs, "check_ok": bool(errs["fused"] <= tol and errs["composed"] <= tol),
               "factors": [int(v) for v in dim.factors[:dim.n_factors]], "fpw": int(dim.ffts_per_workgroup)}
        for name, _ in cands:
            t = times[name]
            rec[name] = {"median_us": round(statistics.median(t), 1), "min_us": round(min(t), 1), "max_us": round(max(t), 1)}
        f_us, comp = rec["fused"]["median_us"], rec["composed"]
        rec["gate"] = bool(comp["median_us"] - f_us > comp["max_us"] - comp["min_us"])
        rec["composed_over_fused_time"] = round(comp["median_us"] / f_us, 3)
        rec["fused_over_r2c_time"] = round(f_us / rec["r2c"]["median_us"], 3)
        rec["fused_hbm_fraction"] = round((ns * length * sb + rows * (m + 1) * 2 * sb) / (f_us * 1e-6) / HBM_PEAK, 4)
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        del plan, x, y_fused, y_comp, fbuf, windows
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("tools/bench_stft.py: medians of %d alternating event-timed reps after %d warm-up reps, %d real signals, "
                    "about %.1f GiB of bins, lead 0, periodic Hann window\n\n" % (a.reps, a.warmup, SIGNALS, a.gib))
            f.write("prec      N    hop     rows |  fused us (min/max)        | composed us (min/max)     | r2c us (min/max)          "
                    "| comp/fused fused/r2c   HBM   gate  check rel-L2 fused / composed\n")
            for r in lines:
                def col(k):
                    return "%9.1f (%.1f/%.1f)" % (r[k]["median_us"], r[k]["min_us"], r[k]["max_us"])
                f.write("%-4s %6d %6d %8d | %-26s | %-25s | %-25s | %9.3f %9.3f %6.3f  %-5s %.2e / %.2e\n"
                        % (r["precision"], r["n"], r["hop"], r["rows"], col("fused"), col("composed"), col("r2c"),
                           r["composed_over_fused_time"], r["fused_over_r2c_time"], r["fused_hbm_fraction"],
                           "pass" if r["gate"] else "FAIL", r["check_rel_l2"]["fused"], r["check_rel_l2"]["composed"]))
    if not all(r["check_ok"] for r in lines):
        sys.exit("bench_stft.py: a sampled fused or composed output failed the accuracy check")
    if not all(r["gate"] for r in lines):
        sys.exit("bench_stft.py: the fused verb did not beat the composed route at every case")


if __name__ == "__main__":
    main()
