#!/usr/bin/env python3
"""The power spectrogram / Welch periodogram of real signals in one kernel against the best a user has without it, on the
same device, in one process.

    python tools/bench_periodogram.py [--reps 15] [--warmup 3] [--gib 1.0] [--cases f32:512:128,...] [--out FILE]

For every (precision, N, hop): 16 real signals whose frames of N scalars every `hop` scalars (lead 0, every frame inside
its signal, periodic Hann window) would make about --gib GiB of complex bins, and for every A in {1, 8, a Welch-like A that
leaves 128 rows per signal -- 2048 units} (equal values once; the frame count is a multiple of all three).  Three
candidates are timed alternately (a, b, c, a, ...), each rep bracketed by HIP events on the plan's stream after a
warm-up, all on ONE plan of pf.real_descriptor(N):
  (a) fused     plan.periodogram: one kernel, straight from the signals, S * R * (M + 1) real scalars stored
  (b) composed  the best that exists without the feature (the yardstick): plan.stft into a bin buffer, y.real ** 2 +
                y.imag ** 2 by torch, and for A > 1 a reshaped sum over the A frames of a row
  (c) stft      plan.stft alone: what the bins cost before anything squares them
Reported: the median and the min / max of the reps in microseconds, the ratios composed / fused and stft / fused, and for
the fused verb the algorithmic HBM fraction (signal bytes + output bytes) / time over 8 TB/s.  `gate`: fused beats
composed by more than the spread (max - min) of the composed route's reps; no ratio is fixed in advance, and a case that
misses the gate is recorded as such, not dropped.  The first, a middle and the last row of one signal are checked against
NumPy in double precision (abs(rfft) ** 2 summed), for the fused and for the composed output.  One JSON line per case on
stdout; the table goes to --out (default profiles/periodogram_bench.txt).
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
WELCH_ROWS = 128


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--gib", type=float, default=1.0, help="GiB of complex bins the composed route writes per execute")
    ap.add_argument("--cases", default=DEFAULT_CASES, help="comma-separated PRECISION:N:HOP")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "periodogram_bench.txt"))
    a = ap.parse_args()

    import torch
    import portfft_amd as pf
    if not torch.cuda.is_available():
        sys.exit("bench_periodogram.py needs a GPU")
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
        frames = max(8, int(a.gib * 2 ** 30 / (ns * (m + 1) * 2 * sb)))
        welch = 8 * max(1, -(-frames // (WELCH_ROWS * 8)))
        frames = max(1, frames // welch) * welch
        length = (frames - 1) * hop + n
        plan = pf.real_descriptor(n, prec).commit(stream)
        w = (0.5 - 0.5 * torch.cos(2 * np.pi * torch.arange(n, dtype=torch.float64, device="cuda") / n)).to(rt)
        plan.set_window(w)
        plan.set_periodogram_window(w)
        x = torch.empty(ns, length, dtype=torch.float64, device="cuda").uniform_(-1, 1).to(rt)
        y = torch.empty(ns, frames, m + 1, dtype=ct, device="cuda")
        wd = w.cpu().numpy().astype(np.float64)
        pick = ns // 2 + 1
        xp = x[pick].cpu().numpy().astype(np.float64)
        for avg in sorted({1, 8, welch}):
            n_rows = frames // avg
            p_fused = torch.empty(ns, n_rows, m + 1, dtype=rt, device="cuda")
            kept = {}

            def run_fused():
                plan.periodogram(x, p_fused, hop, frames, frames_per_row=avg, want_event=False)

            def run_composed():
                plan.stft(x, y, hop, want_event=False)
                p = y.real ** 2 + y.imag ** 2
                kept["p"] = p if avg == 1 else p.view(ns, n_rows, avg, m + 1).sum(dim=2)

            def run_stft():
                plan.stft(x, y, hop, want_event=False)

            cands = (("fused", run_fused), ("composed", run_composed), ("stft", run_stft))
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
            errs = {"fused": 0.0, "composed": 0.0}
            for c in sorted({0, n_rows // 2, n_rows - 1}):
                idx = (np.arange(c * avg, (c + 1) * avg)[:, None] * hop + np.arange(n)[None, :])
                ref = (np.abs(np.fft.rfft(xp[idx] * wd, axis=-1)) ** 2).sum(axis=0)
                for name, out in (("fused", p_fused), ("composed", kept["p"])):
                    got = out[pick, c].cpu().numpy().astype(np.float64)
                    errs[name] = max(errs[name], float(np.abs(got - ref).sum() / ref.sum()))
            tau, u = (2e-6, 2.0 ** -24) if prec == "f32" else (5e-15, 2.0 ** -53)
            tol = 2 * tau + tau * tau + (avg + 2) * u
            dim = plan.info().dims[0]
            rec = {"precision": prec, "n": n, "hop": hop, "signals": ns, "frames": frames, "avg_frames": avg,
                   "units": ns * n_rows, "length": length, "reps": a.reps, "check_rel_l1": errs,
                   "check_ok": bool(errs["fused"] <= tol and errs["composed"] <= tol),
                   "factors": [int(v) for v in dim.factors[:dim.n_factors]], "fpw": int(dim.ffts_per_workgroup)}
            for name, _ in cands:
                t = times[name]
                rec[name] = {"median_us": round(statistics.median(t), 1), "min_us": round(min(t), 1), "max_us": round(max(t), 1)}
            f_us, comp = rec["fused"]["median_us"], rec["composed"]
            rec["gate"] = bool(comp["median_us"] - f_us > comp["max_us"] - comp["min_us"])
            rec["composed_over_fused_time"] = round(comp["median_us"] / f_us, 3)
            rec["stft_over_fused_time"] = round(rec["stft"]["median_us"] / f_us, 3)
            rec["fused_hbm_fraction"] = round((ns * length * sb + ns * n_rows * (m + 1) * sb) / (f_us * 1e-6) / HBM_PEAK, 4)
            print(json.dumps(rec), flush=True)
            lines.append(rec)
            del p_fused, kept
        del plan, x, y
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("tools/bench_periodogram.py: medians of %d alternating event-timed reps after %d warm-up reps, %d real "
                    "signals, frames worth about %.1f GiB of complex bins, lead 0, periodic Hann window\n\n"
                    % (a.reps, a.warmup, SIGNALS, a.gib))
            f.write("prec      N    hop      A    units |  fused us (min/max)        | composed us (min/max)     | stft us (min/max)         "
                    "| comp/fused stft/fused   HBM   gate  check rel-L1 fused / composed\n")
            for r in lines:
                def col(k):
                    return "%9.1f (%.1f/%.1f)" % (r[k]["median_us"], r[k]["min_us"], r[k]["max_us"])
                f.write("%-4s %6d %6d %6d %8d | %-26s | %-25s | %-25s | %9.3f %9.3f %6.3f  %-5s %.2e / %.2e\n"
                        % (r["precision"], r["n"], r["hop"], r["avg_frames"], r["units"], col("fused"), col("composed"),
                           col("stft"), r["composed_over_fused_time"], r["stft_over_fused_time"], r["fused_hbm_fraction"],
                           "pass" if r["gate"] else "FAIL", r["check_rel_l1"]["fused"], r["check_rel_l1"]["composed"]))
    if not all(r["check_ok"] for r in lines):
        sys.exit("bench_periodogram.py: a sampled fused or composed output failed the accuracy check")
    missed = [r for r in lines if not r["gate"]]
    if missed:
        sys.exit("bench_periodogram.py: %d case(s) did not beat the composed route by more than its spread (recorded in the "
                 "table)" % len(missed))


if __name__ == "__main__":
    main()
