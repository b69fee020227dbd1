#!/usr/bin/env python3
"""Measure the sharded LARS step (kf_lars_trust_update, kf_lars_apply_run,
ShardedLARSOptimizer) by tools/bench_sharded_lamb.py's method:
every call between its own pair of HIP events, 10 warm-up calls, then 100 calls
rotating over copies of the buffers that together exceed the L2 and the
Infinity Cache; medians with the 10th and 90th percentiles.

  kernel  In one loop, on the same element counts, call by call: the SGD
          kernel (kf_sgd_update_batch, momentum on: 20 bytes per f32 element)
          and the LARS apply launch (20 bytes for f32, 18 + 2 on the master
          path), and for information the norm plan over the pieces of p and g
          (8 bytes) and the trust launch. Two layouts: one segment of 2^26
          elements, and ResNet-50's 25,583,592 elements as 16 shards of 1/8
          with the "tensor ∩ shard" pieces.
  step1   For information: step() at world 1 on ResNet-50 in f32,
          ShardedLARSOptimizer and ShardedSGDOptimizer alternating in one loop
          (the bytes say 28 / 20).

--lib PATH loads another build of libkungfu_amd.so (a kernel variant);
--variant NAME goes into every row. One JSON object per line goes to --out
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
from bench_sharded_lamb import pieces_of  # noqa: E402

DT = {"float32": torch.float32, "bfloat16": torch.bfloat16}
LARS = dict(b0.SGD, weight_decay=1e-4, trust_coefficient=0.001, eps=1e-8, adapt=True)


def layouts(case, dev):
    """(segment counts, [(segment, offset, count)] pieces)."""
    if case == "one":
        return [1 << 26], [(0, 0, 1 << 26)]
    from kungfu_amd.collective import GradBuckets
    sizes = b0.model_sizes()
    layout = GradBuckets(sizes, torch.float32, dev, 8, n_buckets=16)
    counts = [b.numel() // 8 for b in layout.buckets]
    return counts, pieces_of(sizes, layout, 8)


def kernel_case(case, dname, args):
    from kungfu_amd import ops
    dev = torch.device("cuda:0")
    dt, f32 = DT[dname], torch.float32
    master = dt != f32
    counts, pieces = layouts(case, dev)
    n, P = sum(counts), len(pieces)
    gen = torch.Generator(device=dev).manual_seed(1)
    filled = lambda dtype: [torch.randn(c, device=dev, generator=gen).to(dtype)  # noqa: E731
                            for c in counts]
    copies = max(2, -(-b0.ROTATE_BYTES // (20 * n)))
    group_of = torch.zeros(P, dtype=torch.int32, device=dev)
    sq = torch.ones(2 * P, dtype=torch.float64, device=dev)
    coef = torch.zeros(ops.LARS_COEF * P, dtype=torch.float64, device=dev)
    ratio = torch.ones(P, dtype=torch.float64, device=dev)

    def trust():
        ops.lars_trust_update_(sq, 1, group_of, [LARS], coef, ratio, args.np)

    trust()
    sgd, apply_, norm, keep = [], [], [], []
    cut = lambda ts: [ts[s][o:o + c] for s, o, c in pieces]  # noqa: E731
    for _ in range(copies):
        p, g, m = filled(f32), filled(dt), filled(f32)
        p16 = filled(dt) if master else None
        if not master:  # the parent's kernel, at the same 20 bytes per element
            sgd.append(lambda p=p, g=g, m=m: ops.sgd_update_batch_(p, g, m, [b0.SGD] * len(p),
                                                                   args.np))
        plan = ops.lars_apply_plan(cut(p), cut(g), cut(m), list(range(P)), P,
                                   cut(p16) if master else None)
        out = torch.zeros(2 * P + 1, dtype=torch.float64, device=dev)
        if master:
            sa, sb = ops.SegNorm(cut(p)), ops.SegNorm(cut(g))
            norm.append(lambda sa=sa, sb=sb, out=out: (sa.run("sq", out=out[:P + 1]),
                                                       sb.run("sq", out=out[P:])))
        else:
            sn = ops.SegNorm(cut(p) + cut(g))
            norm.append(lambda sn=sn, out=out: sn.run("sq", out=out))
        keep.append((p, g, m, p16, plan, out))
        apply_.append(lambda plan=plan: plan.run(coef, args.np))
    turn = lambda xs, k: xs[k % copies:] + xs[:k % copies]  # noqa: E731
    fns = {"apply": apply_, "norm": turn(norm, 1), "trust": [trust]}
    if sgd:
        fns["sgd"] = turn(sgd, 2)
    us = b0.time_calls(fns, args.reps, args.warmup)
    row = {"what": "LARS apply launch against the SGD kernel", "case": case, "dtype": dname,
           "variant": args.variant, "elements": n, "segments": len(counts), "pieces": P,
           "copies": copies, "np": args.np}
    for k in fns:
        row[k] = b0.stats(us[k])
    for k, per in (("apply", 20), ("norm", 6 if master else 8), ("sgd", 20)):
        if k in row:
            row[k]["bytes_per_element"] = per
            row[k]["GBps"] = round(per * n / (row[k]["median_us"] * 1e-6) / 1e9, 1)
    if sgd:
        row["apply_over_sgd"] = round(row["apply"]["median_us"] / row["sgd"]["median_us"], 4)
    b0.emit(row, args)


def step_world1(args):
    from kungfu_amd.optimizers import ShardedLARSOptimizer, ShardedSGDOptimizer
    dev = torch.device("cuda:0")
    pl, ps = b0.make_model(dev), b0.make_model(dev)
    kw = dict(lr=0.1, momentum=0.9, weight_decay=1e-4)
    lars = ShardedLARSOptimizer(torch.optim.SGD(pl, **kw))
    sgd = ShardedSGDOptimizer(torch.optim.SGD(ps, **kw))
    b0.give_grads(pl, dev)
    b0.give_grads(ps, dev)
    us = b0.time_calls({"lars": [lars.step], "sgd": [sgd.step]}, args.steps, args.warmup)
    row = {"what": "step time, world 1 (for information)", "model": "resnet50-imagenet",
           "dtype": "float32", "variant": args.variant, "elements": sum(b0.model_sizes()),
           "lars": b0.stats(us["lars"]), "sgd": b0.stats(us["sgd"])}
    row["lars_over_sgd"] = round(row["lars"]["median_us"] / row["sgd"]["median_us"], 4)
    b0.emit(row, args)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--what", default="kernel,step1", help="comma list of kernel, step1")
    ap.add_argument("--reps", type=int, default=100, help="timed kernel calls per kind")
    ap.add_argument("--steps", type=int, default=40, help="timed steps per optimizer, world 1")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--np", type=int, default=8, help="the update's /np (0: none)")
    ap.add_argument("--kernel-cases", default="one,shard", help="comma list of one, shard")
    ap.add_argument("--dtypes", default="float32,bfloat16")
    ap.add_argument("--lib", default=None, help="another build of libkungfu_amd.so to load")
    ap.add_argument("--variant", default="product")
    ap.add_argument("--out", default=None, help="append the JSON lines here")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_sharded_lars: needs a GPU (no CPU path)")
    if args.lib:
        from kungfu_amd import _lib
        _lib.LIB_PATH = os.path.abspath(args.lib)
    what = args.what.split(",")
    for case in args.kernel_cases.split(",") if "kernel" in what else []:
        for dname in args.dtypes.split(","):
            kernel_case(case, dname, args)
    if "step1" in what:
        step_world1(args)


if __name__ == "__main__":
    main()
