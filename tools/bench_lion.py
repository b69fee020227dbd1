#!/usr/bin/env python3
"""Measure Lion's three kernels (kf_lion_update_batch, kf_lion_signs_batch,
kf_lion_apply_signs_batch) by tools/bench_mx8.py's method: every
call between its own pair of HIP events, 10 warm-up calls, then 100 calls
rotating over copies of the buffers that together exceed the L2 and the
Infinity Cache; medians with the 10th and 90th percentiles.

In one loop, call by call, on the same shards: the dense update, the signs
kernel, the apply kernel (on a shard's worth of parameters: at world W a step
runs it W times over) and the yardstick, kf_sgd_update_batch with momentum.
Two layouts: one segment of 2^26 elements, and ResNet-50's 16 buckets' shards
of 1/8. GB/s are against algorithmic bytes per element: the update and SGD
5 x sz, signs 3 x sz + 0.25, apply 2 x sz + 0.25.

--cases and --dtypes choose what one process measures, so that a driver can
give every case its own time limit. One JSON object per line goes to --out
(and stdout).
"""
import argparse
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [ROOT, HERE]

import torch  # noqa: E402

import bench_sharded_adam as b0  # noqa: E402  (stats, time_calls, emit, the model)

DT = {"float32": torch.float32, "bfloat16": torch.bfloat16}
WORLD = 8
LION = {"lr": 1e-4, "betas": (0.9, 0.99), "weight_decay": 0.1}


def shards_of(case, dev):
    if case == "one":
        return [1 << 26]
    from kungfu_amd.collective import GradBuckets
    layout = GradBuckets(b0.model_sizes(), torch.float32, dev, WORLD, n_buckets=16)
    return [b.numel() // WORLD for b in layout.buckets]


def kernel_case(case, dname, args):
    from kungfu_amd import ops
    dev = torch.device("cuda:0")
    dt, sz = DT[dname], DT[dname].itemsize
    shards = shards_of(case, dev)
    n, nb = sum(shards), len(shards)
    gen = torch.Generator(device=dev).manual_seed(1)
    rand = lambda k: torch.randn(k, device=dev, generator=gen).to(dt)  # noqa: E731
    copies = max(2, -(-b0.ROTATE_BYTES // int(n * 3 * sz)))
    sr = ([0] * nb, list(range(nb)), 5)
    hs, sgd = [LION] * nb, [b0.SGD] * nb
    fns, keep = {"update": [], "signs": [], "apply": [], "sgd": []}, []
    for _ in range(copies):
        p, g, m = ([rand(q) for q in shards] for _ in range(3))
        codes = [torch.zeros(ops.lion_sign_bytes(q) // 4, dtype=torch.int32, device=dev)
                 for q in shards]
        ops.lion_signs_batch_(g, [x.clone() for x in m], codes, hs)  # real codes for apply
        keep.append((p, g, m, codes))
        fns["update"].append(lambda p=p, g=g, m=m: ops.lion_update_batch_(p, g, m, hs, WORLD, sr))
        fns["signs"].append(lambda g=g, m=m, c=codes: ops.lion_signs_batch_(g, m, c, hs, WORLD))
        fns["apply"].append(lambda p=p, c=codes: ops.lion_apply_signs_batch_(p, c, hs, sr))
        fns["sgd"].append(lambda p=p, g=g, m=m: ops.sgd_update_batch_(p, g, m, sgd, WORLD))
    turn = lambda xs, k: xs[k % copies:] + xs[:k % copies]  # noqa: E731
    fns = {k: turn(f, i) for i, (k, f) in enumerate(fns.items())}
    us = b0.time_calls(fns, args.reps, args.warmup)
    row = {"what": "Lion: update, signs, apply and kf_sgd_update_batch with momentum",
           "case": case, "dtype": dname, "elements": n, "segments": nb, "copies": copies}
    for k, per in (("update", 5 * sz), ("signs", 3 * sz + 0.25), ("apply", 2 * sz + 0.25),
                   ("sgd", 5 * sz)):
        row[k] = b0.stats(us[k])
        row[k]["bytes_per_element"] = per
        row[k]["GBps"] = round(per * n / (row[k]["median_us"] * 1e-6) / 1e9, 1)
    for k in ("update", "signs"):
        row[k + "_over_sgd"] = round(row[k]["median_us"] / row["sgd"]["median_us"], 4)
    b0.emit(row, args)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=100, help="timed calls per kind")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--cases", default="one,shard", help="comma list of one, shard")
    ap.add_argument("--dtypes", default="float32,bfloat16")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lion", "bench.jsonl"),
                    help="append the JSON lines here")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_lion: needs a GPU (no CPU path)")
    for case in args.cases.split(","):
        for dname in args.dtypes.split(","):
            kernel_case(case, dname, args)


if __name__ == "__main__":
    main()
