#!/usr/bin/env python3
"""Measure the MXFP8 gradient wire's two kernels (kf_mx8_pack_batch,
kf_mx8_fold_batch) by tools/bench_sharded_lars.py's method:
every call between its own pair of HIP events, 10 warm-up calls, then 100 calls
rotating over copies of the buffers that together exceed the L2 and the
Infinity Cache; medians with the 10th and 90th percentiles.

In one loop, call by call, at world 8: the pack of the gradient buckets, the
fold of the eight received pieces of every shard (/ 8 fused), and the pass
the fold replaces, kf_bucket_reduce_batch's k = 8 fold of the same shards in
the bucket's dtype (/ 8 fused). Two layouts: one shard of 2^26 elements (its
bucket is 2^26 elements too: pack's count is the shard's), and ResNet-50's 16
buckets with their world-8 shards. GB/s are against algorithmic bytes: pack
sz + 1.03125 per bucket element, fold 8 x 1.03125 + sz per shard element, the
k = 8 fold 9 x sz.

--cases and --dtypes choose what one process measures, so that a driver can
give every case its own time limit. One JSON object per line goes to --out
(and stdout).
"""
import argparse
import ctypes
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [ROOT, HERE]

import torch  # noqa: E402

import bench_sharded_adam as b0  # noqa: E402  (stats, time_calls, emit, the model)

DT = {"float32": torch.float32, "bfloat16": torch.bfloat16}
WORLD = 8
KF_SUM = 0


def layouts(case, dev):
    """(bucket counts for pack, shard counts for the folds)."""
    if case == "one":
        return [1 << 26], [1 << 26]
    from kungfu_amd.collective import GradBuckets
    layout = GradBuckets(b0.model_sizes(), torch.float32, dev, WORLD, n_buckets=16)
    return [b.numel() for b in layout.buckets], [b.numel() // WORLD for b in layout.buckets]


def kernel_case(case, dname, args):
    from kungfu_amd import _lib, ops
    lib = _lib.load()
    dev = torch.device("cuda:0")
    dt, sz = DT[dname], DT[dname].itemsize
    buckets, shards = layouts(case, dev)
    nb_, ns = sum(buckets), sum(shards)
    gen = torch.Generator(device=dev).manual_seed(1)
    rand = lambda n: torch.randn(n, device=dev, generator=gen).to(dt)  # noqa: E731
    copies = max(2, -(-b0.ROTATE_BYTES // int(ns * (WORLD * 1.03125 + sz))))
    stream = torch.cuda.current_stream(dev).cuda_stream
    pack, fold, fold8, keep = [], [], [], []
    for _ in range(copies):
        grads = [rand(n) for n in buckets]
        packed = ops.mx8_pack_batch_(grads, WORLD)
        # the pieces a rank receives for its shards: any packed data of the right size
        recvd = ops.mx8_pack_batch_([rand(q * WORLD) for q in shards], WORLD)
        outs = [torch.empty(q, dtype=dt, device=dev) for q in shards]
        ins = [rand(q) for q in shards for _ in range(WORLD)]
        sums = [torch.empty(q, dtype=dt, device=dev) for q in shards]
        tabs = (_lib.ptr_array([t.data_ptr() for t in ins]), _lib.ptr_array([t.data_ptr() for t in sums]),
                (ctypes.c_size_t * len(shards))(*shards))
        keep.append((grads, packed, recvd, outs, ins, sums, tabs))
        pack.append(lambda g=grads, p=packed: ops.mx8_pack_batch_(g, WORLD, p))
        fold.append(lambda r=recvd, o=outs: ops.mx8_fold_batch_(r, o, WORLD, WORLD))
        fold8.append(lambda t=tabs: _lib.check(lib.kf_bucket_reduce_batch(
            t[0], WORLD, t[1], t[2], len(shards), int(ops.kungfu_dtype(sums[0])), KF_SUM, WORLD,
            stream), "kf_bucket_reduce_batch"))
    turn = lambda xs, k: xs[k % copies:] + xs[:k % copies]  # noqa: E731
    fns = {"pack": pack, "fold": turn(fold, 1), "fold_k8": turn(fold8, 2)}
    us = b0.time_calls(fns, args.reps, args.warmup)
    row = {"what": "MXFP8 wire: pack, fold and the k = 8 fold it replaces", "case": case,
           "dtype": dname, "world": WORLD, "bucket_elements": nb_, "shard_elements": ns,
           "segments": len(shards), "copies": copies}
    for k, per, n in (("pack", sz + 1.03125, nb_), ("fold", WORLD * 1.03125 + sz, ns),
                      ("fold_k8", (WORLD + 1) * sz, ns)):
        row[k] = b0.stats(us[k])
        row[k]["bytes_per_element"] = per
        row[k]["GBps"] = round(per * n / (row[k]["median_us"] * 1e-6) / 1e9, 1)
    row["fold_over_fold_k8"] = round(row["fold"]["median_us"] / row["fold_k8"]["median_us"], 4)
    b0.emit(row, args)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=100, help="timed calls per kind")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--cases", default="one,shard", help="comma list of one, shard")
    ap.add_argument("--dtypes", default="float32,bfloat16")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mx8_wire", "bench.jsonl"),
                    help="append the JSON lines here")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_mx8: needs a GPU (no CPU path)")
    for case in args.cases.split(","):
        for dname in args.dtypes.split(","):
            kernel_case(case, dname, args)


if __name__ == "__main__":
    main()
