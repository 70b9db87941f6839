"""Fingerprint of the 1-D planner: a fixed list of descriptors that reaches every tier plan_1d tries, both of its
refusals and every rule of the four-step planner (plan_global.cpp).  One JSON line per case -- every field of
plan.info() except xcd_recoveries, and the SHA-256 of the forward and of the backward output on a seeded input; a
refusal of the library is a result (status name + message text) -- and, at the end, the sorted file names of the JIT
cache directory: exactly which kernels the commits compiled.  A HIP error ends the run.

A planner change that is meant to leave every plan alone runs this before and after, each time with its own empty
cache directory, and diffs the two outputs: they must be identical byte for byte (profiles/plan_fingerprint.txt holds
the last one recorded on an MI355X).  PFFT_PLAN_MEASURE=1 is not in the list: its result depends on timing
(tests/test_gpu_plan_measure.py covers it).

usage: plan_fingerprint.py CACHE_DIR [substring of the case names to run]"""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, S = "interleaved", "split"


def case(name, lengths, prec="f32", batch=1, storage=P, bi=False, pad=0, env=None):
    return dict(name=name, lengths=lengths, prec=prec, batch=batch, storage=storage, bi=bi, pad=pad, env=env or {})


CASES = [
    # ---- tiers before GLOBAL ----
    case("packed f32 4096", [4096], batch=8),  # plan_packed, pre-compiled
    case("packed f16 4096", [4096], "f16", batch=8),  # plan_packed, fp16 storage
    case("f16 2^18 refused", [1 << 18], "f16"),  # the fp16 refusal text
    case("unpacked f32 1024 padded rows", [1024], batch=4, pad=8),  # plan_unpacked
    case("BI f32 2048 x 16", [2048], batch=16, bi=True),  # plan_wide_group, single width
    case("BI split f32 768 x 32", [768], batch=32, storage=S, bi=True),  # plan_wide_group, double width
    case("BI f32 4096 x 16", [4096], batch=16, bi=True),  # batch-interleaved two-stage plan, its n1 = 128 rule
    case("2-D f32 4096 x 16", [4096, 16]),  # the N-D branch of the same: a long column dimension
    case("BI f32 256 x 64", [256], batch=64, bi=True),  # plan_strided: a column-shaped stage
    case("BI f32 256 x 32771", [256], batch=32771, bi=True),  # plan_strided, policy 3: unaligned pitch, 64 MiB of data
    case("generic f32 1001 no JIT", [1001], batch=3, env={"PFFT_JIT": "0"}),  # the generic tier
    case("unpacked f32 2^17 padded rows", [1 << 17], batch=2, pad=8),  # first refusal: GLOBAL needs packed 1-D data
    case("2-D f32 4 x 65536", [4, 65536]),  # ... and rank 1
    case("f32 2 * 10007", [2 * 10007]),  # second refusal: a large prime factor, no two factors fit local memory
    # ---- four-step pairs ----
    case("f32 2^20", [1 << 20]),  # full pair
    case("f64 2^20", [1 << 20], "f64"),  # full pair, twiddles on stage B's loads (ltw)
    case("f32 2^20 no ltw", [1 << 20], env={"PFFT_NO_LTW": "1"}),
    case("f64 2^20 no ltw", [1 << 20], "f64", env={"PFFT_NO_LTW": "1"}),
    case("f32 2^20 no pairs", [1 << 20], env={"PFFT_NO_FS_PAIRS": "1"}),  # the default kernels of a registered length
    case("f64 2^20 no pairs", [1 << 20], "f64", env={"PFFT_NO_FS_PAIRS": "1"}),
    case("f32 2^18", [1 << 18]),  # the paired short stage A (256 x 1024)
    case("f32 3 * 2^18", [3 << 18]),  # half pair
    case("f32 5 * 2^17", [5 << 17]),  # half pair
    case("f32 3 * 2^18 no half pairs", [3 << 18], env={"PFFT_NO_HALF_PAIRS": "1"}),
    case("f32 5 * 2^17 no half pairs", [5 << 17], env={"PFFT_NO_HALF_PAIRS": "1"}),
    case("f32 3 * 2^19", [3 << 19]),  # tiles twice as wide as stage B's groups
    case("f32 3 * 2^19 no wide tiles", [3 << 19], env={"PFFT_NO_WIDE_TILES": "1"}),
    # ---- four-step without a pair, and the debug knobs ----
    case("f32 68640", [68640]),  # no pair; a split entry of the tuned table (104 x 660); no tiled intermediate
    case("f32 10^5", [100000]),
    case("f32 10^6", [1000000]),
    case("f32 68640 no tuned table", [68640], env={"PFFT_NO_TUNED_TABLE": "1"}),  # the "closest to 500" rule
    case("f32 10^5 no tuned table", [100000], env={"PFFT_NO_TUNED_TABLE": "1"}),
    case("f32 68640 no split rule", [68640], env={"PFFT_NO_SPLIT_RULE": "1"}),  # the balanced split over strided kernels
    case("f64 68640", [68640], "f64"),  # no pair, no rule: the balanced split
    case("f32 68640 n1 = 104", [68640], env={"PFFT_GLOBAL_N1": "104"}),  # the forced first factor
    case("f32 10^6 no JIT", [1000000], env={"PFFT_JIT": "0"}),  # balanced split over generic lengths, generic stages
    case("f32 68640 no JIT", [68640], env={"PFFT_JIT": "0"}),
    case("f32 61^2 * 4 no JIT", [61 * 61 * 4], env={"PFFT_JIT": "0"}),
    case("f32 2^20 generic A", [1 << 20], env={"PFFT_DEBUG_GLOBAL": "ga"}),  # stage A on the generic kernel
    case("f32 2^20 generic B", [1 << 20], env={"PFFT_DEBUG_GLOBAL": "gb"}),
    case("f32 2^20 layout b", [1 << 20], env={"PFFT_GLOBAL_LAYOUT": "b"}),  # tile_intermediate's other layout
    case("f32 2^20 no tiled scratch", [1 << 20], env={"PFFT_NO_TILED_SCRATCH": "1"}),  # row-major intermediate
    # ---- four-step, SPLIT_COMPLEX and chunking ----
    case("split f32 2^20", [1 << 20], storage=S),  # mixed-storage stages, group-major intermediate
    case("split f32 2^20 no split tiled", [1 << 20], storage=S, env={"PFFT_NO_SPLIT_TILED": "1"}),
    case("split f32 2^20 streamed", [1 << 20], storage=S, batch=4, env={"PFFT_SPLIT_CACHED": "0", "PFFT_CACHE_CHUNK_MIB": "16"}),
    case("split f32 2^20 chunked", [1 << 20], storage=S, batch=4, env={"PFFT_CACHE_CHUNK_MIB": "16"}),
    # chunks of 2 of 4 transforms: pre-compiled interleaved stages (the overlap halves the scratch) ...
    case("f32 2^20 x 4 chunked", [1 << 20], batch=4, env={"PFFT_CACHE_CHUNK_MIB": "16"}),
    case("f32 2^20 x 4 chunked by the cap", [1 << 20], batch=4, env={"PFFT_GLOBAL_CHUNK_MIB": "16", "PFFT_CACHE_CHUNK_MIB": "0"}),
    case("f64 2^20 x 4 chunked, one per CU", [1 << 20], "f64", batch=4, env={"PFFT_CACHE_CHUNK_MIB": "32", "PFFT_CHUNK_OVERLAP": "0"}),
    case("f32 3 * 2^18 x 4 chunked", [3 << 18], batch=4, env={"PFFT_CACHE_CHUNK_MIB": "16"}),  # ... runtime-compiled stage A
    # ---- other GLOBAL plans ----
    case("f32 2^23", [1 << 23]),  # three-stage plan
    case("split f32 2^23", [1 << 23], storage=S),
    case("f32 2^18 x 256", [1 << 18], batch=256),  # XCD-local launch at its entry's minimum (512 MiB)
    case("f32 2^18 x 256 no XCD-local", [1 << 18], batch=256, env={"PFFT_NO_XCD_LOCAL": "1"}),
]


def descriptor_of(pf, c):
    d = pf.descriptor(c["lengths"], c["prec"])
    d.number_of_transforms = c["batch"]
    if c["storage"] == S:
        d.complex_storage = pf.complex_storage.SPLIT_COMPLEX
    if c["bi"]:  # batch-interleaved on both sides
        d.forward_strides = d.backward_strides = [c["batch"]]
        d.forward_distance = d.backward_distance = 1
    if c["pad"]:  # padded rows on both sides
        d.forward_distance = d.backward_distance = c["lengths"][0] + c["pad"]
    return d


def seeded(np, torch, scalars, dtype):
    """uniform(-1, 1) scalars: a seeded block of 2^20, repeated"""
    block = np.random.Generator(np.random.SFC64(7)).uniform(-1, 1, 1 << 20).astype(np.float32)
    return torch.from_numpy(np.resize(block, scalars)).to(dtype).cuda()


def sha(torch, *tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.cpu().contiguous().view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


def run_case(pf, np, torch, c):
    d = descriptor_of(pf, c)
    plan = d.commit()
    info = plan.info()
    rec = dict(rank=info.rank, n_compute_units=info.n_compute_units, twiddle_bytes=info.twiddle_bytes,
               scratch_bytes=info.scratch_bytes, launches=list(info.launches), xcd_local=list(info.xcd_local),
               knob_mask=info.knob_mask,
               dims=[dict(length=x.length, tier=x.tier, factors=list(x.factors[:x.n_factors]), workgroup_size=x.workgroup_size,
                          ffts_per_workgroup=x.ffts_per_workgroup, lds_bytes=x.lds_bytes) for x in info.dims[:info.rank]])
    dtype = {"f32": torch.float32, "f64": torch.float64, "f16": torch.float16}[c["prec"]]
    count = max(d.get_input_count(pf.direction.FORWARD), d.get_output_count(pf.direction.FORWARD))
    if c["storage"] == S:
        x = seeded(np, torch, 2 * count, dtype)
        bufs = [[x[:count].contiguous(), x[count:].contiguous()]] + [[torch.zeros(count, dtype=dtype, device="cuda") for _ in range(2)]
                                                                     for _ in range(2)]
    else:
        bufs = [[seeded(np, torch, 2 * count, dtype)]] + [[torch.zeros(2 * count, dtype=dtype, device="cuda")] for _ in range(2)]
    plan.compute_forward(*bufs[0], *bufs[1]).wait()
    plan.compute_backward(*bufs[1], *bufs[2]).wait()
    torch.cuda.synchronize()
    rec["forward"] = sha(torch, *bufs[1])
    rec["backward"] = sha(torch, *bufs[2])
    return rec


def main():
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    cache = os.path.abspath(sys.argv[1])
    only = sys.argv[2] if len(sys.argv) > 2 else ""
    os.makedirs(cache, exist_ok=True)
    if os.listdir(cache):
        sys.exit("plan_fingerprint: %s is not empty" % cache)
    os.environ["PFFT_JIT_CACHE_DIR"] = cache
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import portfft_amd as pf
    torch.cuda.set_device(0)
    for c in CASES:
        if only not in c["name"]:
            continue
        saved = {k: os.environ.get(k) for k in c["env"]}
        os.environ.update(c["env"])
        try:
            rec = dict(status="ok", **run_case(pf, np, torch, c))
        except pf.hip_error:
            raise
        except pf.base_error as e:  # a refusal is a result
            rec = dict(status=type(e).__name__, message=str(e))
        finally:
            for k, v in saved.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v
        print(json.dumps(dict(case=c["name"], env=c["env"], **rec), sort_keys=True), flush=True)
        sys.stderr.write("== %s\n" % c["name"])  # (lines up a library's own diagnostics with the cases)
        sys.stderr.flush()
    print(json.dumps(dict(cache=sorted(os.listdir(cache)))), flush=True)


if __name__ == "__main__":
    main()
