#!/usr/bin/env python3
"""The inverse MDCT (windowed TDAC overlap-add) in one kernel against the best a user has without it, on the same device,
in one process.

    python tools/bench_imdct.py [--reps 15] [--warmup 3] [--gib 1.0] [--cases f32:1024,...] [--out FILE]

For every (precision, N): about --gib GiB of coefficient rows, 64 signals of F frames, lead N, sine window, out_length F N
(everything the frames cover behind the lead), backward_scale 1 / (2N).  The candidates are timed alternately (a, b1, b2,
..., c, a, ...), each rep bracketed by HIP events on the plan's stream after a warm-up:
  (a) fused      plan.imdct of pf.real_descriptor(N): one kernel
  (b) composed   the best that exists without the feature (the yardstick): plan.dct4(inverse=True) of the coefficient rows
                 into a frame buffer Y = [p, q] of F x N scalars, then torch:
                   slices     the unfold [q, -rev q, -rev p, -p] times the window into a buffer of F x 2N scalars (four mul
                              passes), then one add of the adjacent halves g[f][:N] + g[f - 1][N:] and a copy of the last half
                   index_add  the same unfold and window, then two index_add_ of the halves into a zeroed output
                   fold       the same unfold and window, then torch.nn.functional.fold at stride N
                   direct     no unfolded buffer: the four quarter products are written and accumulated (mul, addcmul_)
                              straight from Y into the output blocks
                 All are timed; the fastest median is the yardstick.
  (c) dct4       plan.dct4 alone on the same rows, a yardstick only
Reported: the median and the min / max of the reps in microseconds, the ratios composed / fused and fused / (c), the
algorithmic HBM fraction of the fused verb over 8 TB/s -- 2 * N * sizeof(T) * rows / time, every coefficient counted once
in and every sample once out --, the chunk the plan chose and 1 / chunk, the share of frames transformed twice.  `gate`:
fused beats composed by more than the spread (max - min) of the composed route's reps.  One sampled block of N samples
per case is checked against NumPy in double (the bins 2n + 1 + N of a zero-stuffed FFT of 8N points), for the fused and
for every composed output (all must pass: a wrong yardstick is no yardstick).  One JSON line per case on stdout; the table
goes to --out (default profiles/imdct_bench.txt).  Every case is reported, also one that misses its gate.
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
COMPOSED = ("slices", "index_add", "fold", "direct")


def unfolded_reference(coeff):
    """g[n] = 2 sum_k X[k] cos(pi (2n + 1 + N)(2k + 1) / (4N)), n < 2N"""
    coeff = np.asarray(coeff, dtype=np.float64)
    n = coeff.shape[-1]
    u = np.zeros(8 * n)
    u[1:2 * n:2] = coeff
    return 2.0 * np.real(np.fft.fft(u)[n + 1:5 * n:2])


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--gib", type=float, default=1.0, help="GiB of coefficient rows per execute")
    ap.add_argument("--cases", default=DEFAULT_CASES, help="comma-separated PRECISION:N")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "imdct_bench.txt"))
    a = ap.parse_args()

    import torch
    import portfft_amd as pf
    if not torch.cuda.is_available():
        sys.exit("bench_imdct.py needs a GPU")
    torch.cuda.set_device(0)
    stream = torch.cuda.current_stream()
    lines = []
    for case in a.cases.split(","):
        prec, n = case.split(":")
        n = int(n)
        m = n // 2
        sb = 4 if prec == "f32" else 8
        rt = torch.float32 if prec == "f32" else torch.float64
        frames = max(2, int(a.gib * 2 ** 30 / (n * sb)) // SIGNALS)
        rows = SIGNALS * frames
        length = frames * n  # lead N: the blocks 1 ... F of the frames' axis
        d = pf.real_descriptor(n, prec)
        d.backward_scale = 1.0 / (2 * n)
        plan = d.commit(stream)
        win = torch.sin(np.pi * (torch.arange(2 * n, dtype=torch.float64, device="cuda") + 0.5) / (2 * n)).to(rt)
        plan.set_imdct_window(win)  # (prepares the type-4 stages as well)
        chunk = plan.imdct_chunk_frames(SIGNALS, frames)
        w0, w1, w2, w3 = win[:m], -win[m:n], -win[n:3 * m], -win[3 * m:]  # the window of the four quarters, signs folded in
        coeff = torch.empty(SIGNALS, frames, n, dtype=rt, device="cuda").uniform_(-1, 1)
        ybuf = torch.empty(SIGNALS, frames, n, dtype=rt, device="cuda")
        gbuf = torch.empty(SIGNALS, frames, 2 * n, dtype=rt, device="cuda")
        out_fused = torch.empty(SIGNALS, length, dtype=rt, device="cuda")
        out_comp = torch.empty(SIGNALS, frames + 1, n, dtype=rt, device="cuda")  # the blocks 0 ... F; 1 ... F are the output
        idx0 = torch.arange(frames, device="cuda")
        idx1 = idx0 + 1
        p, q = ybuf[..., :m], ybuf[..., m:]

        def run_fused():
            plan.imdct(coeff, out_fused, want_event=False)

        def run_dct4():
            plan.dct4(coeff.view(rows, n), ybuf.view(rows, n), inverse=True, want_event=False)

        def unfold_window():
            torch.mul(q, w0, out=gbuf[..., :m])
            torch.mul(q.flip(-1), w1, out=gbuf[..., m:n])
            torch.mul(p.flip(-1), w2, out=gbuf[..., n:3 * m])
            torch.mul(p, w3, out=gbuf[..., 3 * m:])

        def run_composed(how):
            run_dct4()
            blocks = out_comp[:, 1:]
            if how == "direct":
                torch.mul(q[:, 1:], w0, out=blocks[:, :-1, :m])
                blocks[:, :-1, :m].addcmul_(p[:, :-1].flip(-1), w2)
                torch.mul(q[:, 1:].flip(-1), w1, out=blocks[:, :-1, m:])
                blocks[:, :-1, m:].addcmul_(p[:, :-1], w3)
                torch.mul(p[:, -1].flip(-1), w2, out=blocks[:, -1, :m])
                torch.mul(p[:, -1], w3, out=blocks[:, -1, m:])
                return
            unfold_window()
            if how == "slices":
                torch.add(gbuf[:, 1:, :n], gbuf[:, :-1, n:], out=blocks[:, :-1])
                blocks[:, -1].copy_(gbuf[:, -1, n:])
            elif how == "index_add":
                out_comp.zero_()
                out_comp.index_add_(1, idx0, gbuf[..., :n])
                out_comp.index_add_(1, idx1, gbuf[..., n:])
            else:
                folded = torch.nn.functional.fold(gbuf.transpose(1, 2), (1, (frames + 1) * n), (1, 2 * n), stride=(1, n))
                out_comp.view(SIGNALS, -1).copy_(folded.view(SIGNALS, -1))

        cands = [("fused", run_fused)] + [("composed_" + h, (lambda h=h: run_composed(h))) for h in COMPOSED] + [("dct4", run_dct4)]
        # the sampled block: signal s, block b of the frames' axis = output samples (b - 1) N ... b N - 1
        s, b = SIGNALS // 2, frames // 2 + 1
        wn = win.double().cpu().numpy()
        ref = (wn[:n] * unfolded_reference(coeff[s, b].cpu().numpy())[:n] if b < frames else 0.0) \
            + wn[n:] * unfolded_reference(coeff[s, b - 1].cpu().numpy())[n:]
        ref = ref / (2 * n)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        times, errs, dropped = {name: [] for name, _ in cands}, {}, {}
        for rep in range(a.warmup + a.reps):
            for name, fn in cands:
                if name in dropped:
                    continue
                ev[0].record(stream)
                try:
                    fn()
                except RuntimeError as e:  # (a torch formulation this build of torch does not have at this size or type)
                    dropped[name] = str(e).splitlines()[0][:120]
                    torch.cuda.synchronize()
                    continue
                ev[1].record(stream)
                ev[1].synchronize()
                if rep >= a.warmup:
                    times[name].append(ev[0].elapsed_time(ev[1]) * 1e3)  # us
                if rep == 0 and name != "dct4":
                    got = out_fused[s, (b - 1) * n:b * n] if name == "fused" else out_comp[s, b]
                    got = got.cpu().numpy().astype(np.float64)
                    errs[name] = float(np.linalg.norm(got - ref) / np.linalg.norm(ref))
        torch.cuda.synchronize()
        if "fused" in dropped:
            sys.exit("bench_imdct.py: the fused verb failed: " + dropped["fused"])
        tol = 2e-6 if prec == "f32" else 5e-15
        dim = plan.info().dims[0]
        rec = {"precision": prec, "n": n, "signals": SIGNALS, "frames": frames, "rows": rows, "reps": a.reps,
               "chunk_frames": int(chunk), "halo_share": round(1.0 / chunk, 5), "check_rel_l2": errs,
               "check_ok": bool(all(v <= tol for v in errs.values())), "dropped": dropped,
               "factors": [int(v) for v in dim.factors[:dim.n_factors]], "fpw": int(dim.ffts_per_workgroup)}
        for name, _ in cands:
            t = times[name]
            if t:
                rec[name] = {"median_us": round(statistics.median(t), 1), "min_us": round(min(t), 1), "max_us": round(max(t), 1)}
        best = min((k for k in ("composed_" + h for h in COMPOSED) if k in rec), key=lambda k: rec[k]["median_us"])
        rec["composed_best"] = best
        f_us, comp = rec["fused"]["median_us"], rec[best]
        rec["gate"] = bool(comp["median_us"] - f_us > comp["max_us"] - comp["min_us"])
        rec["composed_over_fused_time"] = round(comp["median_us"] / f_us, 3)
        rec["fused_over_dct4_time"] = round(f_us / rec["dct4"]["median_us"], 3)
        rec["fused_hbm_fraction"] = round(2 * n * sb * rows / (f_us * 1e-6) / HBM_PEAK, 4)
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        del plan, coeff, ybuf, gbuf, out_fused, out_comp, p, q
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("tools/bench_imdct.py: medians of %d alternating event-timed reps after %d warm-up reps, about %.1f GiB of "
                    "coefficient rows, %d signals, lead N, sine window, out_length F N; composed = plan.dct4 into a frame buffer, "
                    "then torch: slices (unfold and window into F x 2N, one add of adjacent halves) / index_add / fold / direct "
                    "(quarter products accumulated straight into the output); the fastest is the yardstick; dct4 = plan.dct4 "
                    "alone on the same rows; chunk = the plan's choice, 1/C the share of frames transformed twice\n\n"
                    % (a.reps, a.warmup, a.gib, SIGNALS))
            f.write("prec      N     rows chunk    1/C |  fused us (min/max)        | slices us (min/max)       | index_add us (min/max)    "
                    "| fold us (min/max)         | direct us (min/max)       | dct4 us (min/max)         | best      comp/fused fused/dct4   "
                    "HBM   gate  check rel-L2 fused / composed\n")
            for r in lines:
                def col(k):
                    if k not in r:
                        return "n/a"
                    return "%9.1f (%.1f/%.1f)" % (r[k]["median_us"], r[k]["min_us"], r[k]["max_us"])
                f.write("%-4s %6d %8d %5d %6.4f | %-26s | %-25s | %-25s | %-25s | %-25s | %-25s | %-9s %9.3f %9.3f %7.3f  %-5s %.2e / %.2e\n"
                        % (r["precision"], r["n"], r["rows"], r["chunk_frames"], r["halo_share"], col("fused"),
                           col("composed_slices"), col("composed_index_add"), col("composed_fold"), col("composed_direct"),
                           col("dct4"), r["composed_best"][len("composed_"):], r["composed_over_fused_time"],
                           r["fused_over_dct4_time"], r["fused_hbm_fraction"], "pass" if r["gate"] else "FAIL",
                           r["check_rel_l2"]["fused"], max(v for k, v in r["check_rel_l2"].items() if k != "fused")))
            for r in lines:
                for k, why in r["dropped"].items():
                    f.write("%s N=%d: %s not timed: %s\n" % (r["precision"], r["n"], k, why))
    if not all(r["check_ok"] for r in lines):
        sys.exit("bench_imdct.py: a sampled fused or composed output failed the accuracy check")
    if not all(r["gate"] for r in lines):
        sys.exit("bench_imdct.py: the fused verb did not beat the composed route at every case")


if __name__ == "__main__":
    main()
