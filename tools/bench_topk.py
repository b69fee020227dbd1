#!/usr/bin/env python3
"""Time the top-k gradient wire's two kernels against the 1-bit wire's
(kf_topk_pack_ef_batch and kf_sign1_pack_ef_batch, kf_topk_fold_batch and
kf_sign1_fold_batch) by tools/bench_sign1.py's method: one
process, every call between its own pair of HIP events, 10 warm-up calls, then
100 rounds that call every kernel in turn (the 1-bit pair and the top-k pair
at k = 1, 4 and 8, alternating) on the same rotating copies of the buffers,
which together exceed the L2 and the Infinity Cache; medians with the 10th and
90th percentiles. World 8; the layouts are bench_mx8.py's (§25's bucket sizes):
one segment of 2^26 elements, and ResNet-50's 16 buckets.

GB/s are against algorithmic bytes: the packs per bucket element, sz + 8 +
0.1875 (1-bit) and sz + 8 + 5 k / 64 (top-k); the folds per shard element,
8 x 0.1875 + sz and 8 x 5 k / 64 + sz. Every top-k entry says how far its
median lies from the 1-bit kernel's, beside that one's p10-p90 spread. One
JSON object per line goes to --out (and stdout).
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
KS = (1, 4, 8)
WIRE = dict({"sign1": 0.1875}, **{"topk%d" % k: 5 * k / 64 for k in KS})  # bytes per element on the wire


def case_row(case, dname, args):
    from kungfu_amd import ops
    dev = torch.device("cuda:0")
    dt, sz = bench_mx8.DT[dname], bench_mx8.DT[dname].itemsize
    buckets, shards = bench_mx8.layouts(case, dev)
    nb_, ns = sum(buckets), sum(shards)
    gen = torch.Generator(device=dev).manual_seed(1)
    rand = lambda n: torch.randn(n, device=dev, generator=gen).to(dt)  # noqa: E731
    copies = max(2, -(-b0.ROTATE_BYTES // int(nb_ * (sz + 8 + 0.1875))))
    packs = {"sign1": ops.sign1_pack_ef_batch_}
    folds = {"sign1": ops.sign1_fold_batch_}
    for k in KS:
        packs["topk%d" % k] = lambda g, r, w, p=None, k=k: ops.topk_pack_ef_batch_(g, r, w, k, p)
        folds["topk%d" % k] = lambda p, o, w, n, k=k: ops.topk_fold_batch_(p, o, w, k, n)
    fns, keep = {w + kind: [] for w in WIRE for kind in ("_pack", "_fold")}, []
    for _ in range(copies):
        grads = [rand(n) for n in buckets]
        res = [torch.zeros(n, dtype=torch.float32, device=dev) for n in buckets]
        outs = [torch.empty(q, dtype=dt, device=dev) for q in shards]
        src = [rand(q * WORLD) for q in shards]
        for w in WIRE:
            packed = packs[w](grads, res, WORLD)
            # the pieces a rank receives for its shards: any packed data of the right size
            recvd = packs[w](src, [torch.zeros(q * WORLD, dtype=torch.float32, device=dev) for q in shards], WORLD)
            keep.append((grads, res, outs, packed, recvd))
            fns[w + "_pack"].append(lambda w=w, g=grads, r=res, p=packed: packs[w](g, r, WORLD, p))
            fns[w + "_fold"].append(lambda w=w, r=recvd, o=outs: folds[w](r, o, WORLD, WORLD))
    us = b0.time_calls(fns, args.reps, args.warmup)
    row = {"what": "top-k wire against the 1-bit wire: EF pack and fold, same buffers, same loop",
           "case": case, "dtype": dname, "world": WORLD, "bucket_elements": nb_,
           "shard_elements": ns, "copies": copies}
    for w, wire in WIRE.items():
        for kind, per, n in (("_pack", sz + 8 + wire, nb_), ("_fold", WORLD * wire + sz, ns)):
            row[w + kind] = b0.stats(us[w + kind])
            row[w + kind]["bytes_per_element"] = per
            row[w + kind]["GBps"] = round(per * n / (row[w + kind]["median_us"] * 1e-6) / 1e9, 1)
    for kind in ("_pack", "_fold"):
        base = row["sign1" + kind]
        base["spread_us"] = round(base["p90_us"] - base["p10_us"], 3)
        for k in KS:
            e = row["topk%d" % k + kind]
            e["over_sign1"] = round(e["median_us"] / base["median_us"], 4)
    b0.emit(row, args)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=100, help="timed rounds")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--cases", default="one,shard", help="comma list of one, shard")
    ap.add_argument("--dtypes", default="float32,bfloat16")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "topk_wire", "bench.jsonl"),
                    help="append the JSON lines here")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_topk: needs a GPU (no CPU path)")
    for case in args.cases.split(","):
        for dname in args.dtypes.split(","):
            case_row(case, dname, args)


if __name__ == "__main__":
    main()
