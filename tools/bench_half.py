#!/usr/bin/env python3
"""fp16 storage against fp32 on the same shapes (PFFT_PRECISION_F16: fp16 in HBM, the fp32 plan's arithmetic).

    python tools/bench_half.py [--reps 20] [--warmup 5] [--shapes 4096x65536,1024x262144,...] [--out DIR]

For every shape both plans are committed in this process and timed alternately (f16, f32, f16, ...), each rep
bracketed by HIP events on the plan's stream after a warm-up.  Reported per precision: the median kernel time, the
algorithmic bytes (read + write of the batch: 2 x N x batch x element size) over that time against the 8 TB/s HBM
peak, and the f16 / f32 transform-rate ratio.  Sampled f16 outputs are checked against a float64 NumPy DFT of the
same fp16 input (rel-L2 within 1.5 x the fp16 output rounding).  One JSON line per shape; --out DIR also writes them
to DIR/bench_half.json.
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

HBM_PEAK = 8.0e12
DEFAULT_SHAPES = "4096x65536,1024x262144,16384x16384,32768x8192,10240x26214"


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--shapes", default=DEFAULT_SHAPES, help="comma-separated NxBATCH")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    import portfft_amd as pf
    if not torch.cuda.is_available():
        sys.exit("bench_half.py needs a GPU")
    torch.cuda.set_device(0)
    stream = torch.cuda.current_stream()
    lines = []
    for shape in a.shapes.split(","):
        n, batch = (int(v) for v in shape.lower().split("x"))
        bufs, plans = {}, {}
        for prec, dt in (("f16", torch.complex32), ("f32", torch.complex64)):
            d = pf.descriptor([n], prec)
            d.number_of_transforms = batch
            d.forward_scale = 1.0 / n
            plans[prec] = d.commit(stream)
            real = torch.float16 if prec == "f16" else torch.float32
            x = torch.empty((batch, 2 * n), dtype=real, device="cuda").uniform_(-1, 1)
            bufs[prec] = (x.view(dt), torch.empty_like(x).view(dt))
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        times = {"f16": [], "f32": []}
        for rep in range(a.warmup + a.reps):
            for prec in ("f16", "f32"):
                x, y = bufs[prec]
                ev[0].record(stream)
                plans[prec].compute_forward(x, y, want_event=False)
                ev[1].record(stream)
                ev[1].synchronize()
                if rep >= a.warmup:
                    times[prec].append(ev[0].elapsed_time(ev[1]) * 1e3)  # us
        # sampled f16 outputs against float64 NumPy on the same fp16 input
        x, y = bufs["f16"]
        pick = sorted({0, batch // 3, batch // 2, batch - 1})
        xs = x.view(torch.float16)[pick].cpu().numpy().astype(np.float64)
        ys = y.view(torch.float16)[pick].cpu().numpy().astype(np.float64)
        xc, yc = xs[:, 0::2] + 1j * xs[:, 1::2], ys[:, 0::2] + 1j * ys[:, 1::2]
        ref = np.fft.fft(xc, axis=1) / n
        r16 = ref.real.astype(np.float16).astype(np.float64) + 1j * ref.imag.astype(np.float16).astype(np.float64)
        err = float(np.max(np.linalg.norm(yc - ref, axis=1) / np.linalg.norm(ref, axis=1)))
        e_round = float(np.max(np.linalg.norm(r16 - ref, axis=1) / np.linalg.norm(ref, axis=1)))
        rec = {"n": n, "batch": batch, "reps": a.reps, "check_rel_l2": err, "check_e_round": e_round,
               "check_ok": bool(err <= 1.5 * e_round + 1e-6)}
        for prec, es in (("f16", 4), ("f32", 8)):
            us = statistics.median(times[prec])
            algo = 2.0 * n * batch * es
            rec[prec] = {"kernel_us": round(us, 2), "min_us": round(min(times[prec]), 2),
                         "bytes": int(algo), "tb_s": round(algo / (us * 1e-6) / 1e12, 3),
                         "frac_hbm_peak": round(algo / (us * 1e-6) / HBM_PEAK, 3),
                         "tier": int(plans[prec].info().dims[0].tier)}
        rec["f16_over_f32_rate"] = round(rec["f32"]["kernel_us"] / rec["f16"]["kernel_us"], 3)
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        del bufs, plans
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "bench_half.json"), "w") as f:
            json.dump(lines, f, indent=1)
    if not all(r["check_ok"] for r in lines):
        sys.exit("bench_half.py: sampled f16 outputs failed the accuracy check")


if __name__ == "__main__":
    main()
