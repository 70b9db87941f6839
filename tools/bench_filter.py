#!/usr/bin/env python3
"""Overlap-save FIR filtering in one kernel against what a user has without it, on the same device, in one process.

    python tools/bench_filter.py [--reps 15] [--warmup 3] [--gib 1.0] [--cases f32:1024:129,...] [--out DIR]

For every (precision, N, K): `signals` signals of L = S * hop samples (hop = N - K + 1; about --gib GiB in all), filtered
to as many outputs of L samples (the causal linear convolution, one shared filter).  Three candidates are timed
alternately (a, b, c, a, ...), each rep bracketed by HIP events on the plans' stream after a warm-up:
  (a) fused     plan.filter: one kernel; per sample the signal is read N / hop times and written once
  (b) composed  what exists without the feature (the yardstick): a gather copy of the overlapping segments into rows of N
                (from a copy of the signals the caller keeps zero-padded in front, which is not timed), plan.convolve of
                the rows with the same spectra, and a copy of the hop valid samples of every row to their place
  (c) convolve  the plan.convolve of (b) alone: the same number of rows through the fused circular kernel (context: the
                cost of the windowed addressing is fused / convolve)
Reported: the median and the min / max of the reps in microseconds, the ratios composed / fused and fused / convolve, and
for the fused verb the algorithmic HBM fraction (in_length + out_length) * element bytes * signals / time over 8 TB/s.
`gate`: fused beats composed by more than the spread (max - min) of the composed route's reps.  A window at the front of
one signal (the zeros in front of sample 0), one across a segment boundary in its middle and its last samples are checked
against np.convolve in double precision, for the fused and for the composed output (both must pass: a wrong yardstick is
no yardstick).  One JSON line per case; --out DIR also writes them to DIR/bench_filter.json.
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

DEFAULT_CASES = "f32:1024:129,f32:4096:513,f32:8192:1025,f32:10000:1001,f64:1024:129,f64:4096:513"
HBM_PEAK = 8e12  # bytes / s
SIGNALS = 64


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--gib", type=float, default=1.0, help="GiB of signal per execute")
    ap.add_argument("--cases", default=DEFAULT_CASES, help="comma-separated PRECISION:N:K")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    import portfft_amd as pf
    if not torch.cuda.is_available():
        sys.exit("bench_filter.py needs a GPU")
    torch.cuda.set_device(0)
    stream = torch.cuda.current_stream()
    lines = []
    for case in a.cases.split(","):
        prec, n, k = case.split(":")
        n, k = int(n), int(k)
        hop = n - k + 1
        eb = 8 if prec == "f32" else 16
        ct = torch.complex64 if prec == "f32" else torch.complex128
        ns = SIGNALS
        seg = max(1, int(a.gib * 2 ** 30 / (ns * eb)) // hop)
        length = seg * hop
        rows = ns * seg
        d = pf.convolution_descriptor([n], prec)
        d.number_of_transforms = rows
        plan = d.commit(stream)
        taps = (torch.view_as_complex(torch.empty(k, 2, dtype=torch.float64, device="cuda").uniform_(-1, 1)) / k ** 0.5).to(ct)
        plan.set_filter_taps(taps)
        # the composed route's copy of the signals: K - 1 zeros in front of every signal, zeros behind to a whole window
        lead = k - 1
        xp = torch.zeros(ns, lead + length + n, dtype=ct, device="cuda")
        xp[:, lead:lead + length] = torch.view_as_complex(
            torch.empty(ns, length, 2, dtype=torch.float64, device="cuda").uniform_(-1, 1)).to(ct)
        x = xp[:, lead:lead + length].contiguous()
        windows = xp.unfold(1, n, hop)[:, :seg]  # (signal, segment, N): a view
        y_fused = torch.empty(ns, length, dtype=ct, device="cuda")
        y_comp = torch.empty(ns, length, dtype=ct, device="cuda")
        r_in = torch.empty(ns, seg, n, dtype=ct, device="cuda")
        r_out = torch.empty(ns, seg, n, dtype=ct, device="cuda")

        def run_fused():
            plan.filter(x, y_fused, want_event=False)

        def run_composed():
            r_in.copy_(windows)
            plan.convolve(r_in.view(-1), r_out.view(-1), want_event=False)
            y_comp.view(ns, seg, hop).copy_(r_out[:, :, lead:])

        def run_convolve():
            plan.convolve(r_in.view(-1), r_out.view(-1), want_event=False)

        cands = (("fused", run_fused), ("composed", run_composed), ("convolve", run_convolve))
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
        xr = x[pick].cpu().numpy().astype(np.complex128)
        hr = taps.cpu().numpy().astype(np.complex128)
        span = min(length, 2 * hop)
        starts = sorted({0, (seg // 2) * hop - span // 2 if seg > 2 else 0, length - span})
        errs = {"fused": 0.0, "composed": 0.0}
        for s0 in starts:
            lo = max(0, s0 - lead)
            ref = n * np.convolve(xr[lo:s0 + span], hr)[s0 - lo:s0 - lo + span]
            for name, out in (("fused", y_fused), ("composed", y_comp)):
                got = out[pick, s0:s0 + span].cpu().numpy().astype(np.complex128)
                errs[name] = max(errs[name], float(np.linalg.norm(got - ref) / np.linalg.norm(ref)))
        tol = 2e-6 if prec == "f32" else 5e-15
        dim = plan.info().dims[0]
        rec = {"precision": prec, "n": n, "taps": k, "hop": hop, "signals": ns, "length": length, "rows": rows,
               "reps": a.reps, "check_rel_l2": errs, "check_ok": bool(errs["fused"] <= tol and errs["composed"] <= tol),
               "factors": [int(v) for v in dim.factors[:dim.n_factors]]}
        for name, _ in cands:
            t = times[name]
            rec[name] = {"median_us": round(statistics.median(t), 1), "min_us": round(min(t), 1), "max_us": round(max(t), 1)}
        f_us, comp = rec["fused"]["median_us"], rec["composed"]
        rec["gate"] = bool(comp["median_us"] - f_us > comp["max_us"] - comp["min_us"])
        rec["composed_over_fused_time"] = round(comp["median_us"] / f_us, 3)
        rec["fused_over_convolve_time"] = round(f_us / rec["convolve"]["median_us"], 3)
        rec["fused_hbm_fraction"] = round(2 * length * eb * ns / (f_us * 1e-6) / HBM_PEAK, 4)
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        del plan, x, xp, windows, y_fused, y_comp, r_in, r_out
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "bench_filter.json"), "w") as f:
            json.dump(lines, f, indent=1)
    if not all(r["check_ok"] for r in lines):
        sys.exit("bench_filter.py: a sampled fused or composed output failed the accuracy check")
    if not all(r["gate"] for r in lines):
        sys.exit("bench_filter.py: the fused verb did not beat the composed route at every case")


if __name__ == "__main__":
    main()
