#!/usr/bin/env python3
"""Time the MXFP8 wire's three packs against each other (kf_mx8_pack_batch,
kf_mx8_pack_ef_batch, kf_mx8_pack_sr_batch) by
tools/bench_mx8.py's method: one process, every call between its own pair of
HIP events, 10 warm-up calls, then 100 rounds that call the three packs in
turn on the same rotating copies of the gradient buckets, which together
exceed the L2 and the Infinity Cache; medians with the 10th and 90th
percentiles. World 8; the layouts are bench_mx8.py's: one segment of 2^26
elements, and ResNet-50's 16 buckets.

GB/s are against algorithmic bytes per bucket element: sz + 1.03125 for the
nearest and the stochastic pack, sz + 8 + 1.03125 under error feedback (the
f32 residual read and written). Every row also says how far a variant's
median lies from the plain pack's, beside that pack's own p10-p90 spread.

--lib names another build of the library (a cache-policy A/B of the residual's
loads and stores: make EXTRA=-DKF_MX8_EF_R_NT=1 OUT=... OBJDIR=...); --tag
goes into the row. One JSON object per line goes to --out (and stdout).
"""
import argparse
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [ROOT, HERE]

import torch  # noqa: E402

import bench_mx8  # noqa: E402  (the layouts)
import bench_sharded_adam as b0  # noqa: E402  (stats, time_calls, emit)

WORLD = bench_mx8.WORLD


def pack_case(case, dname, args):
    from kungfu_amd import ops
    dev = torch.device("cuda:0")
    dt, sz = bench_mx8.DT[dname], bench_mx8.DT[dname].itemsize
    buckets, _ = bench_mx8.layouts(case, dev)
    n = sum(buckets)
    gen = torch.Generator(device=dev).manual_seed(1)
    copies = max(2, -(-b0.ROTATE_BYTES // int(n * (sz + 1.03125))))
    near, ef, sr, keep = [], [], [], []
    for c in range(copies):
        grads = [torch.randn(k, device=dev, generator=gen).to(dt) for k in buckets]
        packed = ops.mx8_pack_batch_(grads, WORLD)
        res = [torch.zeros(k, dtype=torch.float32, device=dev) for k in buckets]
        keep.append((grads, packed, res))
        near.append(lambda g=grads, p=packed: ops.mx8_pack_batch_(g, WORLD, p))
        ef.append(lambda g=grads, p=packed, r=res: ops.mx8_pack_ef_batch_(g, r, WORLD, p))
        sr.append(lambda g=grads, p=packed, s=c: ops.mx8_pack_sr_batch_(g, WORLD, 1, s, 3, 0, p))
    us = b0.time_calls({"nearest": near, "error_feedback": ef, "stochastic": sr}, args.reps,
                       args.warmup)
    row = {"what": "MXFP8 wire: the three packs, same buffers, same loop", "tag": args.tag,
           "case": case, "dtype": dname, "world": WORLD, "bucket_elements": n,
           "segments": len(buckets) * WORLD, "copies": copies}
    for k, per in (("nearest", sz + 1.03125), ("error_feedback", sz + 8 + 1.03125),
                   ("stochastic", sz + 1.03125)):
        row[k] = b0.stats(us[k])
        row[k]["bytes_per_element"] = per
        row[k]["GBps"] = round(per * n / (row[k]["median_us"] * 1e-6) / 1e9, 1)
    base = row["nearest"]
    row["nearest_spread_us"] = round(base["p90_us"] - base["p10_us"], 3)
    for k in ("error_feedback", "stochastic"):
        row[k]["over_nearest"] = round(row[k]["median_us"] / base["median_us"], 4)
    b0.emit(row, args)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=100, help="timed rounds")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--cases", default="one,shard", help="comma list of one, shard")
    ap.add_argument("--dtypes", default="float32,bfloat16")
    ap.add_argument("--lib", default=None, help="another build of libkungfu_amd.so to measure")
    ap.add_argument("--tag", default="product", help="what the row calls the build")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mx8_wire", "bench_packs.jsonl"),
                    help="append the JSON lines here")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_mx8_packs: needs a GPU (no CPU path)")
    if args.lib:
        from kungfu_amd import _lib
        _lib.LIB_PATH = os.path.abspath(args.lib)
    for case in args.cases.split(","):
        for dname in args.dtypes.split(","):
            pack_case(case, dname, args)


if __name__ == "__main__":
    main()
