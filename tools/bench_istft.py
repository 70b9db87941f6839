#!/usr/bin/env python3
"""The inverse short-time Fourier transform (overlap-add) of real signals in one kernel against the best a user has
without it, on the same device, in one process.

    python tools/bench_istft.py [--reps 15] [--warmup 3] [--gib 2.0] [--cases f32:512:128,...] [--out FILE]

For every (precision, N, hop): 16 signals of about --gib GiB of frame-major bins in all, lead N / 2, periodic Hann as the
synthesis window, NORMALIZE, out_length = (frames - 1) * hop (torch.istft's centred convention), on ONE plan of
pf.real_descriptor(N) with backward_scale = 1 / N.  Three candidates are timed alternately (a, b, c, a, ...), each rep
bracketed by HIP events on the plan's stream after a warm-up:
  (a) fused     plan.istft: one kernel, plain stores, chunk_frames chosen by the plan
  (b) composed  what exists without the feature (the yardstick): compute_backward of the plan into a frame buffer of
                rows * N scalars, one torch multiply by the window, the faster of index_add_ and
                torch.nn.functional.fold into a zeroed buffer (timed against each other first; the winner is named), and
                the division by the (precomputed) envelope
  (c) c2r       compute_backward alone on the same bins: a yardstick, not a floor -- the same loads as (a), N / hop times
                more bytes stored
Reported: the median and the min / max of the reps in microseconds, the ratios composed / fused and fused / c2r, for the
fused verb the algorithmic HBM fraction (bin bytes + sample bytes) / time over 8 TB/s, and the chunk length the plan chose
with its redundancy H / C, H = ceil(N / hop) - 1 halo frames per chunk of C.  `gate`: fused beats composed by more than
the spread (max - min) of the composed route's reps.  The first, a middle and the last hop of one signal are checked
against NumPy in double precision, for the fused and for the composed output (both must pass: a wrong yardstick is no
yardstick).  --sweep adds the fused verb's time at 1/4, 1/2, 2 and 4 times the chosen chunk length to the JSON line.
One JSON line per case on stdout; the table goes to --out (default profiles/istft_bench.txt).
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


def reference(bins_of, wd, n, hop, lead, frames, t0, t1):
    """samples t0 .. t1-1 of the normalised overlap-add in double; bins_of(f): the bins of frame f (numpy)"""
    u = np.arange(t0, t1) + lead
    ola, env = np.zeros(t1 - t0), np.zeros(t1 - t0)
    for f in range(max(0, (int(u[0]) - n) // hop + 1), min(frames - 1, int(u[-1]) // hop) + 1):
        g = np.fft.irfft(bins_of(f).astype(np.complex128), n)  # (backward_scale * N = 1)
        off = u - f * hop
        ok = (off >= 0) & (off < n)
        ola[ok] += wd[off[ok]] * g[off[ok]]
        env[ok] += wd[off[ok]] ** 2
    return ola / env


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--gib", type=float, default=2.0, help="GiB of bins per execute")
    ap.add_argument("--cases", default=DEFAULT_CASES, help="comma-separated PRECISION:N:HOP")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "istft_bench.txt"))
    ap.add_argument("--sweep", action="store_true", help="also time the fused verb at 1/4, 1/2, 2 and 4 times the chosen chunk length")
    a = ap.parse_args()

    import torch
    import portfft_amd as pf
    if not torch.cuda.is_available():
        sys.exit("bench_istft.py needs a GPU")
    torch.cuda.set_device(0)
    stream = torch.cuda.current_stream()
    lines = []
    for case in a.cases.split(","):
        prec, n, hop = case.split(":")
        n, hop = int(n), int(hop)
        m, lead = n // 2, n // 2
        sb = 4 if prec == "f32" else 8
        rt, ct = (torch.float32, torch.complex64) if prec == "f32" else (torch.float64, torch.complex128)
        ns = SIGNALS
        frames = max(2, int(a.gib * 2 ** 30 / (ns * (m + 1) * 2 * sb)))
        olen = (frames - 1) * hop
        total = (frames - 1) * hop + n
        rows = ns * frames
        d = pf.real_descriptor(n, prec)
        d.number_of_transforms = rows
        d.backward_scale = 1.0 / n
        plan = d.commit(stream)
        w = (0.5 - 0.5 * torch.cos(2 * np.pi * torch.arange(n, dtype=torch.float64, device="cuda") / n)).to(rt)
        plan.set_synthesis_window(w)
        chunk = plan.istft_chunk_frames(ns, frames, hop)
        halo = (n + hop - 1) // hop - 1
        y = torch.view_as_complex(torch.empty(ns, frames, m + 1, 2, dtype=torch.float64, device="cuda").uniform_(-1, 1).to(rt))
        x_fused = torch.empty(ns, olen, dtype=rt, device="cuda")
        x_comp = torch.empty(ns, olen, dtype=rt, device="cuda")
        fbuf = torch.empty(ns, frames, n, dtype=rt, device="cuda")
        acc = torch.empty(ns, total, dtype=rt, device="cuda")
        env = torch.zeros(total, dtype=torch.float64, device="cuda")
        pos = (torch.arange(frames, device="cuda")[:, None] * hop + torch.arange(n, device="cuda")[None, :]).reshape(-1)
        env.index_add_(0, pos, (w.double() ** 2).repeat(frames))
        env = env[lead:lead + olen].to(rt)

        def add_index():
            acc.zero_()
            acc.index_add_(1, pos, fbuf.view(ns, -1))

        def add_fold():
            acc.view(ns, 1, 1, total).copy_(torch.nn.functional.fold(fbuf.transpose(1, 2), (1, total), (1, n), stride=(1, hop)))

        def run_fused():
            plan.istft(y, x_fused, hop, lead=lead, normalize=True, want_event=False)

        def run_c2r():
            plan.compute_backward(y.view(-1), fbuf.view(-1), want_event=False)

        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

        def timed(fn):
            ev[0].record(stream)
            fn()
            ev[1].record(stream)
            ev[1].synchronize()
            return ev[0].elapsed_time(ev[1]) * 1e3  # us

        # the better overlap-add of the two torch has, on the frames of this case
        run_c2r()
        adders = {}
        for name, fn in (("index_add_", add_index), ("fold", add_fold)):
            try:
                timed(fn)
                adders[name] = statistics.median(timed(fn) for _ in range(3))
            except RuntimeError as e:  # (out of memory on the transposed copy, an unsupported shape)
                adders[name] = float("inf")
                print("bench_istft.py: %s is not available for %s (%s)" % (name, case, str(e).splitlines()[0]), file=sys.stderr)
                torch.cuda.empty_cache()
        adder_name = min(adders, key=adders.get)
        adder = add_index if adder_name == "index_add_" else add_fold

        def run_composed():
            run_c2r()
            fbuf.mul_(w)
            adder()
            torch.div(acc[:, lead:lead + olen], env, out=x_comp)

        cands = (("fused", run_fused), ("composed", run_composed), ("c2r", run_c2r))
        times = {name: [] for name, _ in cands}
        for rep in range(a.warmup + a.reps):
            for name, fn in cands:
                t = timed(fn)
                if rep >= a.warmup:
                    times[name].append(t)
        torch.cuda.synchronize()
        pick = ns // 2 + 1
        wd = w.cpu().numpy().astype(np.float64)
        errs = {"fused": 0.0, "composed": 0.0}
        for t0 in sorted({0, (olen // 2 // hop) * hop, olen - hop}):
            ref = reference(lambda f: y[pick, f].cpu().numpy(), wd, n, hop, lead, frames, t0, t0 + hop)
            for name, out in (("fused", x_fused), ("composed", x_comp)):
                got = out[pick, t0:t0 + hop].cpu().numpy().astype(np.float64)
                errs[name] = max(errs[name], float(np.linalg.norm(got - ref) / np.linalg.norm(ref)))
        tol = 2e-6 if prec == "f32" else 5e-15
        dim = plan.info().dims[0]
        rec = {"precision": prec, "n": n, "hop": hop, "signals": ns, "frames": frames, "out_length": olen, "rows": rows,
               "reps": a.reps, "check_rel_l2": errs, "check_ok": bool(errs["fused"] <= tol and errs["composed"] <= tol),
               "factors": [int(v) for v in dim.factors[:dim.n_factors]], "fpw": int(dim.ffts_per_workgroup),
               "chunk_frames": chunk, "halo_frames": halo, "redundancy": round(halo / chunk, 4), "overlap_add": adder_name,
               "overlap_add_us": {k: (round(v, 1) if v != float("inf") else None) for k, v in adders.items()}}
        if a.sweep:  # what the default chunk rule was tuned against
            rec["chunk_sweep_us"] = {}
            for c in sorted({max(1, chunk // 4), max(1, chunk // 2), chunk, min(frames, chunk * 2), min(frames, chunk * 4)}):
                def run_at():
                    plan.istft(y, x_fused, hop, lead=lead, normalize=True, chunk_frames=c, want_event=False)
                timed(run_at)
                rec["chunk_sweep_us"][c] = round(statistics.median(timed(run_at) for _ in range(5)), 1)
        for name, _ in cands:
            t = times[name]
            rec[name] = {"median_us": round(statistics.median(t), 1), "min_us": round(min(t), 1), "max_us": round(max(t), 1)}
        f_us, comp = rec["fused"]["median_us"], rec["composed"]
        rec["gate"] = bool(comp["median_us"] - f_us > comp["max_us"] - comp["min_us"])
        rec["composed_over_fused_time"] = round(comp["median_us"] / f_us, 3)
        rec["fused_over_c2r_time"] = round(f_us / rec["c2r"]["median_us"], 3)
        rec["fused_hbm_fraction"] = round((rows * (m + 1) * 2 * sb + ns * olen * sb) / (f_us * 1e-6) / HBM_PEAK, 4)
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        del plan, y, x_fused, x_comp, fbuf, acc, env, pos
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("tools/bench_istft.py: medians of %d alternating event-timed reps after %d warm-up reps, %d signals, about "
                    "%.1f GiB of bins, lead N/2, periodic Hann, NORMALIZE, out_length (frames - 1) * hop\n\n"
                    % (a.reps, a.warmup, SIGNALS, a.gib))
            f.write("prec      N    hop     rows |  fused us (min/max)        | composed us (min/max)     | c2r us (min/max)          "
                    "| comp/fused fused/c2r   HBM   gate  chunk  H/C    overlap-add  check rel-L2 fused / composed\n")
            for r in lines:
                def col(k):
                    return "%9.1f (%.1f/%.1f)" % (r[k]["median_us"], r[k]["min_us"], r[k]["max_us"])
                f.write("%-4s %6d %6d %8d | %-26s | %-25s | %-25s | %9.3f %9.3f %6.3f  %-5s %5d %6.3f %-11s  %.2e / %.2e\n"
                        % (r["precision"], r["n"], r["hop"], r["rows"], col("fused"), col("composed"), col("c2r"),
                           r["composed_over_fused_time"], r["fused_over_c2r_time"], r["fused_hbm_fraction"],
                           "pass" if r["gate"] else "FAIL", r["chunk_frames"], r["redundancy"], r["overlap_add"],
                           r["check_rel_l2"]["fused"], r["check_rel_l2"]["composed"]))
    if not all(r["check_ok"] for r in lines):
        sys.exit("bench_istft.py: a sampled fused or composed output failed the accuracy check")
    if not all(r["gate"] for r in lines):
        sys.exit("bench_istft.py: the fused verb did not beat the composed route at every case")


if __name__ == "__main__":
    main()
