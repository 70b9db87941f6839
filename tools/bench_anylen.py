#!/usr/bin/env python3
"""Any-length (Bluestein) transforms against what a user has without them, on the same device, in one process.

    python tools/bench_anylen.py [--reps 15] [--warmup 3] [--gib 1.0] [--cases f32:127,f32:4093,...] [--out DIR]

For every (precision, N) with a prime factor above 61, P = the smallest power of two >= 2N - 1, four candidates are
timed alternately (a, b, c, d, a, ...), each rep bracketed by HIP events on the plans' stream after a warm-up, at the
same batch (about --gib GiB of input):
  (a) fused     pf.any_length_descriptor([N]): one kernel, N elements in, N elements out
  (b) composed  the same algorithm from this library's C2C of P and torch elementwise ops: pad-and-multiply, forward P,
                multiply, backward P, multiply-and-slice -- what exists without the feature
  (c) c2c_p     one C2C of P             (context)
  (d) c2c_smooth one C2C of the next length >= N without a prime factor above 61   (context)
Reported: the median and the min / max of the reps in microseconds; for the fused transform the algorithmic HBM
fraction 2 * N * element bytes * batch / time over 8 TB/s.  `gate`: fused beats composed by more than the spread
(max - min) of the composed route's reps.  One sampled transform of the fused and of the composed output is checked
against numpy.fft.fft in double precision (both must pass: a wrong yardstick is no yardstick).  One JSON line per case; --out DIR also writes them to
DIR/bench_anylen.json.
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

DEFAULT_CASES = "f32:127,f32:1021,f32:2039,f32:4093,f64:127,f64:1021,f64:2039"
HBM_PEAK = 8e12  # bytes / s


def smooth_at_least(n):
    while True:
        m = n
        for p in range(2, 62):
            while m % p == 0:
                m //= p
        if m == 1:
            return n
        n += 1


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--gib", type=float, default=1.0, help="GiB of input per execute")
    ap.add_argument("--cases", default=DEFAULT_CASES, help="comma-separated PRECISION:N")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    import portfft_amd as pf
    if not torch.cuda.is_available():
        sys.exit("bench_anylen.py needs a GPU")
    torch.cuda.set_device(0)
    stream = torch.cuda.current_stream()
    lines = []
    for case in a.cases.split(","):
        prec, n = case.split(":")
        n = int(n)
        p = 1
        while p < 2 * n - 1:
            p *= 2
        ns = smooth_at_least(n)
        eb = 8 if prec == "f32" else 16
        ct = torch.complex64 if prec == "f32" else torch.complex128
        batch = max(1, int(a.gib * 2 ** 30 / (n * eb)))

        def commit(d):
            d.number_of_transforms = batch
            return d.commit(stream)

        fused = commit(pf.any_length_descriptor([n], prec))
        plan_p = commit(pf.descriptor([p], prec))
        plan_s = commit(pf.descriptor([ns], prec))
        x = torch.view_as_complex(torch.empty(batch * n, 2, dtype=torch.float64, device="cuda").uniform_(-1, 1)).to(ct)
        y_fused = torch.empty_like(x)
        # the composed route's tables, in double precision rounded once (as the fused plan's)
        j = np.arange(n, dtype=np.int64)
        w64 = np.exp(-1j * np.pi * ((j * j) % (2 * n)) / n)
        b = np.zeros(p, np.complex128)
        b[:n] = np.conj(w64)
        b[p - j[1:]] = np.conj(w64[1:])
        w = torch.from_numpy(w64).to(ct).cuda()
        bh = torch.from_numpy(np.fft.fft(b) / p).to(ct).cuda()
        pa = torch.zeros(batch, p, dtype=ct, device="cuda")
        pb = torch.empty(batch, p, dtype=ct, device="cuda")
        y_comp = torch.empty(batch, n, dtype=ct, device="cuda")
        xs = torch.empty(batch * ns, dtype=ct, device="cuda")
        xs.real.uniform_(-1, 1)
        xs.imag.uniform_(-1, 1)
        ys = torch.empty_like(xs)

        def run_fused():
            fused.compute_forward(x, y_fused, want_event=False)

        def run_composed():
            torch.mul(x.view(batch, n), w, out=pa[:, :n])  # (the pad columns of pa stay zero: forward writes pb)
            plan_p.compute_forward(pa.view(-1), pb.view(-1), want_event=False)
            pb.mul_(bh)
            plan_p.compute_backward(pb.view(-1), pb.view(-1), want_event=False)
            torch.mul(pb[:, :n], w, out=y_comp)

        def run_p():
            plan_p.compute_forward(pa.view(-1), pb.view(-1), want_event=False)

        def run_s():
            plan_s.compute_forward(xs, ys, want_event=False)

        cands = (("fused", run_fused), ("composed", run_composed), ("c2c_p", run_p), ("c2c_smooth", run_s))
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
        run_composed()  # (run_p overwrote pb)
        torch.cuda.synchronize()
        pick = batch // 2
        ref = np.fft.fft(x[pick * n:(pick + 1) * n].cpu().numpy().astype(np.complex128))
        errs = {}
        for name, out in (("fused", y_fused[pick * n:(pick + 1) * n]), ("composed", y_comp[pick])):
            errs[name] = float(np.linalg.norm(out.cpu().numpy().astype(np.complex128) - ref) / np.linalg.norm(ref))
        tol = 2e-6 if prec == "f32" else 5e-15
        dim = fused.info().dims[0]
        rec = {"precision": prec, "n": n, "p": p, "smooth": ns, "batch": batch, "reps": a.reps,
               "check_rel_l2": errs, "check_ok": bool(errs["fused"] <= tol and errs["composed"] <= tol),
               "factors": [int(v) for v in dim.factors[:dim.n_factors]]}
        for name, _ in cands:
            t = times[name]
            rec[name] = {"median_us": round(statistics.median(t), 1), "min_us": round(min(t), 1),
                         "max_us": round(max(t), 1)}
        f_us, comp = rec["fused"]["median_us"], rec["composed"]
        rec["gate"] = bool(comp["median_us"] - f_us > comp["max_us"] - comp["min_us"])
        rec["composed_over_fused_time"] = round(comp["median_us"] / f_us, 3)
        rec["fused_over_c2c_p_time"] = round(f_us / rec["c2c_p"]["median_us"], 3)
        rec["fused_over_c2c_smooth_time"] = round(f_us / rec["c2c_smooth"]["median_us"], 3)
        rec["fused_hbm_fraction"] = round(2 * n * eb * batch / (f_us * 1e-6) / HBM_PEAK, 4)
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        del fused, plan_p, plan_s, x, y_fused, pa, pb, y_comp, xs, ys
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "bench_anylen.json"), "w") as f:
            json.dump(lines, f, indent=1)
    if not all(r["check_ok"] for r in lines):
        sys.exit("bench_anylen.py: a sampled fused or composed output failed the accuracy check")
    if not all(r["gate"] for r in lines):
        sys.exit("bench_anylen.py: the fused transform did not beat the composed route at every length")


if __name__ == "__main__":
    main()
