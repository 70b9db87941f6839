#!/usr/bin/env python3
"""Real transforms against the complex path on the same device, in one process.

    python tools/bench_real.py [--reps 15] [--warmup 3] [--gib 2.0] [--cases f32:1024,f32:8192,...] [--out DIR]

For every (precision, N) three plans are committed and timed alternately (a, b, c, a, b, c, ...), each rep bracketed
by HIP events on the plan's stream after a warm-up, at the same batch (about --gib GiB of real input):
  (a) R2C of N  (pf.real_descriptor: N scalars in, N/2 + 1 bins out)
  (b) C2C of M = N/2  (the same passes, the same bytes to within (M + 1) / M)
  (c) C2C of N  (the least a user without real transforms pays: widen and slice come on top)
Reported: the median and the min / max of the reps in microseconds, the algorithmic bytes moved (read + write) and
their rate.  `gate`: R2C of N beats C2C of N by more than the spread (max - min) of the C2C's reps.  One sampled
transform of the R2C output is checked against numpy.fft.rfft in double precision.  One JSON line per case; --out DIR
also writes them to DIR/bench_real.json.
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

DEFAULT_CASES = "f32:1024,f32:8192,f32:16384,f32:20000,f64:1024,f64:8192,f64:6000"


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--gib", type=float, default=2.0, help="GiB of real input per execute")
    ap.add_argument("--cases", default=DEFAULT_CASES, help="comma-separated PRECISION:N")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    import portfft_amd as pf
    if not torch.cuda.is_available():
        sys.exit("bench_real.py needs a GPU")
    torch.cuda.set_device(0)
    stream = torch.cuda.current_stream()
    lines = []
    for case in a.cases.split(","):
        prec, n = case.split(":")
        n = int(n)
        m = n // 2
        sb = 4 if prec == "f32" else 8
        rt, ct = (torch.float32, torch.complex64) if prec == "f32" else (torch.float64, torch.complex128)
        batch = max(1, int(a.gib * 2 ** 30 / (n * sb)))
        plans, bufs, nbytes = {}, {}, {}
        d = pf.real_descriptor(n, prec)
        d.number_of_transforms = batch
        plans["r2c"] = d.commit(stream)
        x = torch.empty(batch * n, dtype=rt, device="cuda").uniform_(-1, 1)
        bufs["r2c"] = (x, torch.empty(batch * (m + 1), dtype=ct, device="cuda"))
        nbytes["r2c"] = batch * (n + 2 * (m + 1)) * sb
        for name, length in (("c2c_half", m), ("c2c_full", n)):
            c = pf.descriptor([length], prec)
            c.number_of_transforms = batch
            plans[name] = c.commit(stream)
            xi = torch.empty(batch * length * 2, dtype=rt, device="cuda").uniform_(-1, 1).view(ct)
            bufs[name] = (xi, torch.empty_like(xi))
            nbytes[name] = batch * length * 2 * sb * 2
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        times = {k: [] for k in plans}
        for rep in range(a.warmup + a.reps):
            for name in ("r2c", "c2c_half", "c2c_full"):
                xi, yo = bufs[name]
                ev[0].record(stream)
                plans[name].compute_forward(xi, yo, want_event=False)
                ev[1].record(stream)
                ev[1].synchronize()
                if rep >= a.warmup:
                    times[name].append(ev[0].elapsed_time(ev[1]) * 1e3)  # us
        pick = batch // 2
        xs = bufs["r2c"][0][pick * n:(pick + 1) * n].cpu().numpy().astype(np.float64)
        ys = bufs["r2c"][1][pick * (m + 1):(pick + 1) * (m + 1)].cpu().numpy().astype(np.complex128)
        ref = np.fft.rfft(xs)
        err = float(np.linalg.norm(ys - ref) / np.linalg.norm(ref))
        rec = {"precision": prec, "n": n, "batch": batch, "reps": a.reps, "check_rel_l2": err,
               "check_ok": bool(err <= (2e-6 if prec == "f32" else 5e-15)),
               "factors": [int(v) for v in plans["r2c"].info().dims[0].factors[:plans["r2c"].info().dims[0].n_factors]]}
        for name in plans:
            t = times[name]
            us = statistics.median(t)
            rec[name] = {"median_us": round(us, 1), "min_us": round(min(t), 1), "max_us": round(max(t), 1),
                         "bytes": int(nbytes[name]), "tb_s": round(nbytes[name] / (us * 1e-6) / 1e12, 3)}
        full = rec["c2c_full"]
        rec["gate"] = bool(full["median_us"] - rec["r2c"]["median_us"] > full["max_us"] - full["min_us"])
        rec["r2c_over_c2c_half_time"] = round(rec["r2c"]["median_us"] / rec["c2c_half"]["median_us"], 3)
        rec["c2c_full_over_r2c_time"] = round(full["median_us"] / rec["r2c"]["median_us"], 3)
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        del bufs, plans
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "bench_real.json"), "w") as f:
            json.dump(lines, f, indent=1)
    if not all(r["check_ok"] for r in lines):
        sys.exit("bench_real.py: a sampled R2C output failed the accuracy check")


if __name__ == "__main__":
    main()
