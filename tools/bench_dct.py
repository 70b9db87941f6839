#!/usr/bin/env python3
"""The discrete cosine transforms of type 2 and 3 in one kernel against the best a user has without them, on the same
device, in one process.

    python tools/bench_dct.py [--reps 15] [--warmup 3] [--gib 1.0] [--cases f32:1024,...] [--out FILE]

For every (precision, N) and both types: about --gib GiB of packed real rows.  The candidates are timed alternately
(a, b1, b2, c, a, ...), each rep bracketed by HIP events on the plan's stream after a warm-up, all on ONE plan of
pf.real_descriptor(N):
  (a) fused      plan.dct: one kernel, every row read once and written once
  (b) composed   the best that exists without the feature (the yardstick), three passes over HBM:
                 type 2: Makhoul's permutation v = (x[0], x[2], ..., x[5], x[3], x[1]) by torch, compute_forward of the
                         plan, and a torch pass that multiplies the M + 1 bins by exp(-i pi k / 2N) and scatters 2 Re and
                         -2 Im into the N outputs
                 type 3: a torch pass that builds the M + 1 bins conj(c_k) (x[k] - i x[N - k]), compute_backward, and the
                         inverse permutation by torch
                 The permutation has two torch formulations, both timed: "gather" (one index_select with a precomputed
                 index) and "slices" (two strided slice copies, the second flipped).  The faster median is the yardstick.
  (c) r2c / c2r  compute_forward / compute_backward alone on the same number of rows: it moves N + 2 scalars on the
                 complex side against the verb's N, so fused near this is the target shape, not a floor
Reported: the median and the min / max of the reps in microseconds, the ratios composed / fused and fused / (c), and for
the fused verb the algorithmic HBM fraction 2 * N * sizeof(T) * rows / time over 8 TB/s.  `gate`: fused beats composed by
more than the spread (max - min) of the composed route's reps.  One sampled row per case is checked against NumPy in double
(2 Re(exp(-i pi k / 2N) fft(x, 2N)[:N]) and its type-3 counterpart), for the fused and for the composed output (both must
pass: a wrong yardstick is no yardstick).  One JSON line per case on stdout; the table goes to --out (default
profiles/dct_bench.txt).  Every case is reported, also one that misses its gate.
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


def reference(x, kind):
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[-1]
    k = np.arange(n)
    if kind == 2:
        return 2.0 * np.real(np.exp(-1j * np.pi * k / (2 * n)) * np.fft.fft(x, 2 * n)[:n])
    spec = np.zeros(2 * n, dtype=np.complex128)
    spec[:n] = np.where(k == 0, 1.0, 2.0) * x * np.exp(1j * np.pi * k / (2 * n))
    return np.real(2 * n * np.fft.ifft(spec)[:n])


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--gib", type=float, default=1.0, help="GiB of rows per execute")
    ap.add_argument("--cases", default=DEFAULT_CASES, help="comma-separated PRECISION:N")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dct_bench.txt"))
    a = ap.parse_args()

    import torch
    import portfft_amd as pf
    if not torch.cuda.is_available():
        sys.exit("bench_dct.py needs a GPU")
    torch.cuda.set_device(0)
    stream = torch.cuda.current_stream()
    lines = []
    for case in a.cases.split(","):
        prec, n = case.split(":")
        n = int(n)
        m = n // 2
        sb = 4 if prec == "f32" else 8
        rt, ct = (torch.float32, torch.complex64) if prec == "f32" else (torch.float64, torch.complex128)
        rows = max(1, int(a.gib * 2 ** 30 / (n * sb)))
        d = pf.real_descriptor(n, prec)
        d.number_of_transforms = rows
        plan = d.commit(stream)
        plan.prepare_dct()
        x = torch.empty(rows, n, dtype=rt, device="cuda").uniform_(-1, 1)
        y_fused = torch.empty(rows, n, dtype=rt, device="cuda")
        y_comp = torch.empty(rows, n, dtype=rt, device="cuda")
        vbuf = torch.empty(rows, n, dtype=rt, device="cuda")
        bins = torch.empty(rows, m + 1, dtype=ct, device="cuda")
        tbuf = torch.empty(rows, m + 1, dtype=ct, device="cuda")
        kk = torch.arange(m + 1, dtype=torch.float64, device="cuda")
        c = torch.polar(torch.ones_like(kk), -np.pi * kk / (2 * n)).to(ct)
        cc = c.conj().resolve_conj()
        # v[j] = x[perm[j]]: the even samples ascending, then the odd samples descending; inv: y[j] = v[inv[j]]
        perm = torch.cat((torch.arange(0, n, 2), torch.arange(n - 1, 0, -2))).cuda()
        inv = torch.empty_like(perm)
        inv[perm] = torch.arange(n, device="cuda")
        tr = torch.view_as_real(tbuf)
        br = torch.view_as_real(bins)

        for kind in (2, 3):
            def run_fused():
                plan.dct(x, y_fused, type=kind, want_event=False)

            def permute(how, src, dst, index):
                if how == "gather":
                    torch.index_select(src, 1, index, out=dst)
                elif kind == 2:
                    dst[:, :m].copy_(src[:, 0::2])
                    dst[:, m:].copy_(src[:, 1::2].flip(-1))
                else:
                    dst[:, 0::2].copy_(src[:, :m])
                    dst[:, 1::2].copy_(src[:, m:].flip(-1))

            def run_composed(how):
                if kind == 2:
                    permute(how, x, vbuf, perm)
                    plan.compute_forward(vbuf.view(-1), bins.view(-1), want_event=False)
                    torch.mul(bins, c, out=tbuf)
                    torch.mul(tr[:, :, 0], 2, out=y_comp[:, :m + 1])
                    torch.mul(tr[:, 1:m, 1].flip(-1), -2, out=y_comp[:, m + 1:])
                else:
                    br[:, :, 0].copy_(x[:, :m + 1])
                    br[:, 0, 1].zero_()
                    torch.neg(x[:, m:].flip(-1), out=br[:, 1:, 1])  # -x[N - k], k = 1 ... M (k = M: sqrt(2) x[M] comes out real)
                    torch.mul(bins, cc, out=tbuf)
                    plan.compute_backward(tbuf.view(-1), vbuf.view(-1), want_event=False)
                    permute(how, vbuf, y_comp, inv)

            def run_plain():
                if kind == 2:
                    plan.compute_forward(x.view(-1), bins.view(-1), want_event=False)
                else:
                    plan.compute_backward(bins.view(-1), vbuf.view(-1), want_event=False)

            cands = (("fused", run_fused), ("composed_gather", lambda: run_composed("gather")),
                     ("composed_slices", lambda: run_composed("slices")), ("plain", run_plain))
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            times = {name: [] for name, _ in cands}
            pick = rows // 2 + (1 if rows > 2 else 0)
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
                        ref = reference(x[pick].cpu().numpy(), kind)
                        got = (y_fused if name == "fused" else y_comp)[pick].cpu().numpy().astype(np.float64)
                        errs[name] = float(np.linalg.norm(got - ref) / np.linalg.norm(ref))
            torch.cuda.synchronize()
            tol = 2e-6 if prec == "f32" else 5e-15
            dim = plan.info().dims[0]
            rec = {"precision": prec, "n": n, "type": kind, "rows": rows, "reps": a.reps, "check_rel_l2": errs,
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
        del plan, x, y_fused, y_comp, vbuf, bins, tbuf, tr, br
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("tools/bench_dct.py: medians of %d alternating event-timed reps after %d warm-up reps, about %.1f GiB of "
                    "packed real rows; composed = torch permutation (gather: index_select / slices: two strided copies) + "
                    "compute_forward / compute_backward + torch twiddle pass, the faster formulation is the yardstick; "
                    "plain = R2C (type 2) / C2R (type 3) of the same rows\n\n" % (a.reps, a.warmup, a.gib))
            f.write("prec      N type     rows |  fused us (min/max)        | gather us (min/max)       | slices us (min/max)       "
                    "| plain us (min/max)        | comp/fused fused/plain   HBM   gate  check rel-L2 fused / composed\n")
            for r in lines:
                def col(k):
                    return "%9.1f (%.1f/%.1f)" % (r[k]["median_us"], r[k]["min_us"], r[k]["max_us"])
                f.write("%-4s %6d %4d %8d | %-26s | %-25s | %-25s | %-25s | %9.3f %9.3f %7.3f  %-5s %.2e / %.2e\n"
                        % (r["precision"], r["n"], r["type"], r["rows"], col("fused"), col("composed_gather"),
                           col("composed_slices"), col("plain"), r["composed_over_fused_time"], r["fused_over_plain_time"],
                           r["fused_hbm_fraction"], "pass" if r["gate"] else "FAIL", r["check_rel_l2"]["fused"],
                           max(r["check_rel_l2"]["composed_gather"], r["check_rel_l2"]["composed_slices"])))
    if not all(r["check_ok"] for r in lines):
        sys.exit("bench_dct.py: a sampled fused or composed output failed the accuracy check")
    if not all(r["gate"] for r in lines):
        sys.exit("bench_dct.py: the fused verb did not beat the composed route at every case")


if __name__ == "__main__":
    main()
