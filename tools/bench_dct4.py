#!/usr/bin/env python3
"""The DCT-IV of real rows and the MDCT of real signals in one kernel against the best a user has without them, on the same
device, in one process.

    python tools/bench_dct4.py [--reps 15] [--warmup 3] [--gib 1.0] [--cases f32:1024,...] [--out FILE]

For every (precision, N) and both verbs: about --gib GiB of packed real rows (dct4) or of coefficient rows (mdct: 64
signals, lead N, sine window).  The candidates are timed alternately (a, b1, b2, c, a, ...), each rep bracketed by HIP events
on the plan's stream after a warm-up:
  (a) fused      plan.dct4 / plan.mdct of pf.real_descriptor(N): one kernel
  (b) composed   the best that exists without the feature (the yardstick), on a complex plan of M = N / 2 points:
                 dct4: a torch pass that gathers t0[n] = x[2n] + i x[N - 1 - 2n] and multiplies by a_n, compute_forward, a
                       torch pass that multiplies by b_k and scatters 2 Re u[k] to y[2k] and -2 Im u[k] to y[N - 1 - 2k]
                 mdct: in front of that, a torch unfold of the (pre-padded, not timed) signal into frames of 2N at hop N, the
                       window multiply into a frame buffer, and the fold of a frame into the N scalars x'
                 The gather has two torch formulations, both timed: "gather" (one index_select with a precomputed index, then
                 torch.complex) and "slices" (two strided slice copies into the real and imaginary parts, the second
                 flipped).  The faster median is the yardstick.
  (c) r2c        compute_forward of the real plan alone on the same number of rows, as the floor
Reported: the median and the min / max of the reps in microseconds, the ratios composed / fused and fused / (c), and for
the fused verb the algorithmic HBM fraction over 8 TB/s -- dct4: 2 * N * sizeof(T) * rows / time; mdct: 2 * N * sizeof(T) *
frames / time, every sample counted once in and every coefficient once out.  `gate`: fused beats composed by more than the
spread (max - min) of the composed route's reps.  One sampled row per case is checked against NumPy in double (the odd
bins of a zero-stuffed FFT of 8N points), for the fused and for the composed output (both must pass: a wrong yardstick is no
yardstick).  One JSON line per case on stdout; the table goes to --out (default profiles/dct4_bench.txt).  Every case is
reported, also one that misses its gate.
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

DEFAULT_CASES = "f32:64,f32:512,f32:1024,f32:4096,f32:16384,f64:1024,f64:8192"
HBM_PEAK = 8e12  # bytes / s
SIGNALS = 64


def dct4_reference(x):
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[-1]
    u = np.zeros(8 * n)
    u[1:2 * n:2] = x
    return 2.0 * np.real(np.fft.fft(u)[1:2 * n:2])


def mdct_reference(v):
    v = np.asarray(v, dtype=np.float64)
    n = v.shape[-1] // 2
    u = np.zeros(8 * n)
    u[n + 1:5 * n:2] = v
    return 2.0 * np.real(np.fft.fft(u)[1:2 * n:2])


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--gib", type=float, default=1.0, help="GiB of rows per execute")
    ap.add_argument("--cases", default=DEFAULT_CASES, help="comma-separated PRECISION:N")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dct4_bench.txt"))
    a = ap.parse_args()

    import torch
    import portfft_amd as pf
    if not torch.cuda.is_available():
        sys.exit("bench_dct4.py needs a GPU")
    torch.cuda.set_device(0)
    stream = torch.cuda.current_stream()
    lines = []
    for case in a.cases.split(","):
        prec, n = case.split(":")
        n = int(n)
        m = n // 2
        sb = 4 if prec == "f32" else 8
        rt, ct = (torch.float32, torch.complex64) if prec == "f32" else (torch.float64, torch.complex128)
        frames = max(2, int(a.gib * 2 ** 30 / (n * sb)) // SIGNALS)
        rows = SIGNALS * frames
        d = pf.real_descriptor(n, prec)
        d.number_of_transforms = rows
        plan = d.commit(stream)
        kk = torch.arange(m, dtype=torch.float64, device="cuda")
        wa = torch.polar(torch.ones_like(kk), -np.pi * (4 * kk + 1) / (4 * n)).to(ct)
        wb = torch.polar(torch.ones_like(kk), -np.pi * kk / n).to(ct)
        win = torch.sin(np.pi * (torch.arange(2 * n, dtype=torch.float64, device="cuda") + 0.5) / (2 * n)).to(rt)
        plan.set_mdct_window(win)  # (prepares the type-4 stages as well)
        cd = pf.descriptor([m], prec)
        cd.number_of_transforms = rows
        cplan = cd.commit(stream)
        # the signals: `frames` frames at lead N cover (frames - 1) * N samples; N zeros on both sides for the composed route
        length = (frames - 1) * n
        xp = torch.zeros(SIGNALS, (frames + 1) * n, dtype=rt, device="cuda")
        xp[:, n:n + length].uniform_(-1, 1)
        sig = xp[:, n:n + length]
        x = torch.empty(rows, n, dtype=rt, device="cuda").uniform_(-1, 1)
        y_fused = torch.empty(rows, n, dtype=rt, device="cuda")
        y_comp = torch.empty(rows, n, dtype=rt, device="cuda")
        vbuf = torch.empty(rows, n, dtype=rt, device="cuda")
        fold = torch.empty(rows, n, dtype=rt, device="cuda")
        fbuf = torch.empty(SIGNALS, frames, 2 * n, dtype=rt, device="cuda")
        tbuf = torch.empty(rows, m, dtype=ct, device="cuda")
        cbuf = torch.empty(rows, m, dtype=ct, device="cuda")
        bins = torch.empty(rows, m + 1, dtype=ct, device="cuda")
        tr = torch.view_as_real(tbuf)
        cr = torch.view_as_real(cbuf)
        # t0 = v[:, :M] + i v[:, M:], v[j] = x[perm[j]]: the even samples ascending, then the odd samples descending
        perm = torch.cat((torch.arange(0, n, 2), torch.arange(n - 1, 0, -2))).cuda()

        for verb in ("dct4", "mdct"):
            def run_fused():
                if verb == "dct4":
                    plan.dct4(x, y_fused, want_event=False)
                else:
                    plan.mdct(sig, y_fused.view(SIGNALS, frames, n), want_event=False)

            def composed_dct4(how, src):
                if how == "gather":
                    torch.index_select(src, 1, perm, out=vbuf)
                    torch.complex(vbuf[:, :m], vbuf[:, m:], out=tbuf)
                else:
                    tr[:, :, 0].copy_(src[:, 0::2])
                    tr[:, :, 1].copy_(src[:, 1::2].flip(-1))
                tbuf.mul_(wa)
                cplan.compute_forward(tbuf.view(-1), cbuf.view(-1), want_event=False)
                cbuf.mul_(wb)
                torch.mul(cr[:, :, 0], 2, out=y_comp[:, 0::2])
                torch.mul(cr[:, :, 1].flip(-1), -2, out=y_comp[:, 1::2])

            def run_composed(how):
                if verb == "dct4":
                    composed_dct4(how, x)
                    return
                torch.mul(xp.unfold(-1, 2 * n, n), win, out=fbuf)
                v = fbuf.view(rows, 2 * n)
                torch.sub(v[:, 3 * m:].neg(), v[:, 2 * m:3 * m].flip(-1), out=fold[:, :m])
                torch.sub(v[:, :m], v[:, m:2 * m].flip(-1), out=fold[:, m:])
                composed_dct4(how, fold)

            def run_plain():
                plan.compute_forward(x.view(-1), bins.view(-1), want_event=False)

            cands = (("fused", run_fused), ("composed_gather", lambda: run_composed("gather")),
                     ("composed_slices", lambda: run_composed("slices")), ("plain", run_plain))
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            times = {name: [] for name, _ in cands}
            pick = rows // 2 + (1 if rows > 2 else 0)
            if verb == "dct4":
                ref = dct4_reference(x[pick].cpu().numpy())
            else:
                ref = mdct_reference((xp.unfold(-1, 2 * n, n).reshape(rows, 2 * n)[pick].double() * win.double()).cpu().numpy())
            errs = {}
            for rep in range(a.warmup + a.reps):
                for name, fn in cands:
                    ev[0].record(stream)
                    fn()
                    ev[1].record(stream)
                    ev[1].synchronize()
                    if rep >= a.warmup:
                        times[name].append(ev[0].elapsed_time(ev[1]) * 1e3)  # us
                    if rep == 0 and name != "plain":
                        got = (y_fused if name == "fused" else y_comp)[pick].cpu().numpy().astype(np.float64)
                        errs[name] = float(np.linalg.norm(got - ref) / np.linalg.norm(ref))
            torch.cuda.synchronize()
            tol = 2e-6 if prec == "f32" else 5e-15
            dim = plan.info().dims[0]
            rec = {"precision": prec, "n": n, "verb": verb, "rows": rows, "reps": a.reps, "check_rel_l2": errs,
                   "check_ok": bool(all(v <= tol for v in errs.values())),
                   "factors": [int(v) for v in dim.factors[:dim.n_factors]], "fpw": int(dim.ffts_per_workgroup)}
            for name, _ in cands:
                t = times[name]
                rec[name] = {"median_us": round(statistics.median(t), 1), "min_us": round(min(t), 1), "max_us": round(max(t), 1)}
            best = min(("composed_gather", "composed_slices"), key=lambda k: rec[k]["median_us"])
            rec["composed_best"] = best
            f_us, comp = rec["fused"]["median_us"], rec[best]
            rec["gate"] = bool(comp["median_us"] - f_us > comp["max_us"] - comp["min_us"])
            rec["composed_over_fused_time"] = round(comp["median_us"] / f_us, 3)
            rec["fused_over_plain_time"] = round(f_us / rec["plain"]["median_us"], 3)
            rec["fused_hbm_fraction"] = round(2 * n * sb * rows / (f_us * 1e-6) / HBM_PEAK, 4)
            print(json.dumps(rec), flush=True)
            lines.append(rec)
        del plan, cplan, x, xp, sig, y_fused, y_comp, vbuf, fold, fbuf, tbuf, cbuf, bins, tr, cr
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("tools/bench_dct4.py: medians of %d alternating event-timed reps after %d warm-up reps, about %.1f GiB of "
                    "rows (mdct: %d signals, lead N, sine window); composed = torch gather (gather: index_select + "
                    "torch.complex / slices: two strided copies) and pre-twiddle + compute_forward of a complex M-point plan + "
                    "torch post-twiddle and scatter, for mdct behind a torch unfold, window multiply and fold; the faster "
                    "formulation is the yardstick; plain = R2C of the same number of rows\n\n"
                    % (a.reps, a.warmup, a.gib, SIGNALS))
            f.write("prec      N verb     rows |  fused us (min/max)        | gather us (min/max)       | slices us (min/max)       "
                    "| plain us (min/max)        | comp/fused fused/plain   HBM   gate  check rel-L2 fused / composed\n")
            for r in lines:
                def col(k):
                    return "%9.1f (%.1f/%.1f)" % (r[k]["median_us"], r[k]["min_us"], r[k]["max_us"])
                f.write("%-4s %6d %4s %8d | %-26s | %-25s | %-25s | %-25s | %9.3f %9.3f %7.3f  %-5s %.2e / %.2e\n"
                        % (r["precision"], r["n"], r["verb"], r["rows"], col("fused"), col("composed_gather"),
                           col("composed_slices"), col("plain"), r["composed_over_fused_time"], r["fused_over_plain_time"],
                           r["fused_hbm_fraction"], "pass" if r["gate"] else "FAIL", r["check_rel_l2"]["fused"],
                           max(r["check_rel_l2"]["composed_gather"], r["check_rel_l2"]["composed_slices"])))
    if not all(r["check_ok"] for r in lines):
        sys.exit("bench_dct4.py: a sampled fused or composed output failed the accuracy check")
    if not all(r["gate"] for r in lines):
        sys.exit("bench_dct4.py: the fused verb did not beat the composed route at every case")


if __name__ == "__main__":
    main()
