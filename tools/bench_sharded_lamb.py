#!/usr/bin/env python3
"""Measure the sharded LAMB step (kf_lamb_moments_batch,
kf_lamb_master_moments_batch, kf_lamb_trust_update, kf_lamb_apply_run,
ShardedLAMBOptimizer) by tools/bench_sharded_adam_gated.py's
method: ResNet-50's 25,583,592 elements in 16 buckets and in 16 shards of 1/8,
weight_decay 1e-2, np = 8, every call between its own pair of HIP events, 10
warm-up calls, then 100 calls rotating over copies of the buffers that
together exceed the L2 and the Infinity Cache; medians with the 10th and 90th
percentiles.

  kernel  In one loop, on the same buffers' element count, call by call: the
          Adam kernel (f32 kf_adam_update_batch; bf16 kf_adam_master_update_batch,
          28 bytes per element), the LAMB moments kernel (28 / 26 bytes), the
          apply plan over the "tensor ∩ segment" pieces (12 / 14 bytes), and
          for information the norm pass over the pieces of p and u (8 bytes)
          and the trust launch. GOALS, recorded and not gates: the moments
          median is at most the Adam median plus the Adam kernel's own
          p90 - p10 width in that run; the apply median is at most 12/28 of
          the Adam median plus the same width.
  step1   For information: step() at world 1 on an f32 model,
          ShardedLAMBOptimizer and ShardedAdamOptimizer alternating in one loop.

One JSON object per line goes to --out (and stdout).
"""
import argparse
import ctypes
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [ROOT, HERE]

import torch  # noqa: E402

import bench_sharded_adam as b0  # noqa: E402  (pct, stats, time_calls, emit, the model, the hypers)

DT = {"float32": torch.float32, "bfloat16": torch.bfloat16, "float16": torch.float16}
LAMB = dict(b0.ADAM, decoupled=False, eps=1e-6)


def pieces_of(sizes, gb, shard_of):
    """[(segment, offset, count)]: every tensor's intersection with the first
    1 / shard_of of every bucket of the one-flat-buffer layout."""
    out, starts, at = [], [], 0
    for n in sizes:
        starts.append(at)
        at += n
    base = gb.flats[0].data_ptr()
    esz = gb.flats[0].element_size()
    for s, b in enumerate(gb.buckets):
        lo = (b.data_ptr() - base) // esz
        hi = lo + b.numel() // shard_of
        for t0, n in zip(starts, sizes):
            a, e = max(t0, lo), min(t0 + n, hi)
            if a < e:
                out.append((s, a - lo, e - a))
    return out


def kernel_case(name, shard_of, dname, args):
    from kungfu_amd import _lib, ops
    from kungfu_amd.collective import GradBuckets
    dev = torch.device("cuda:0")
    dt, f32 = DT[dname], torch.float32
    master = dt != f32
    sizes = b0.model_sizes()
    gen = torch.Generator(device=dev).manual_seed(1)

    def segs(gb):
        return [b[:b.numel() // shard_of] for b in gb.buckets]

    # the segments' lengths and the pieces come from the f32 layout; every
    # buffer of every dtype is a tensor of its own of exactly that length
    layout = GradBuckets(sizes, f32, dev, shard_of, n_buckets=16)
    counts = [s.numel() for s in segs(layout)]
    pieces = pieces_of(sizes, layout, shard_of)
    n, nb = sum(counts), len(counts)
    del layout

    def filled(dtype, square=False):
        out = []
        for c in counts:
            r = torch.randn(c, device=dev, generator=gen)
            out.append((r * r if square else r).to(dtype))  # exp_avg_sq is not negative
        return out

    copies = max(2, -(-b0.ROTATE_BYTES // (16 * n)))
    lib = _lib.load()
    ha = _lib.adam_hyper_array([b0.ADAM] * nb)
    hl = _lib.adam_hyper_array([LAMB] * nb)
    cnt = (ctypes.c_size_t * nb)(*counts)
    stream = torch.cuda.current_stream(dev).cuda_stream
    kdt = int(ops.kungfu_dtype(torch.empty(1, dtype=dt, device=dev)))
    keep = []

    def tables(bufs):
        keep.append(bufs)
        return [_lib.ptr_array([t.data_ptr() for t in ts]) for ts in bufs]

    def call(fn, what, *a):
        def run():
            _lib.check(fn(*a), what, source="")
        return run

    P = len(pieces)
    nlr = torch.full((P,), -1e-3, dtype=torch.float64, device=dev)
    ratio = torch.ones(P, dtype=torch.float64, device=dev)
    group_of = torch.zeros(P, dtype=torch.int32, device=dev)
    sq = torch.ones(2 * P, dtype=torch.float64, device=dev)
    adam, moments, apply_, norm = [], [], [], []
    for _ in range(copies):
        # p16 (master path only), g, p or master, m, v, u
        p16 = filled(dt) if master else None
        g, p, m, v, u = filled(dt), filled(f32), filled(f32), filled(f32, True), filled(f32)
        if master:
            adam.append(call(lib.kf_adam_master_update_batch, "adam", *tables([p16, g, p, m, v]),
                             cnt, nb, kdt, args.np, ha, stream))
            moments.append(call(lib.kf_lamb_master_moments_batch, "moments",
                                *tables([g, p, m, v, u]), cnt, nb, kdt, args.np, hl, stream))
        else:
            adam.append(call(lib.kf_adam_update_batch, "adam", *tables([p, g, m, v]), cnt, nb, kdt,
                             args.np, ha, stream))
            moments.append(call(lib.kf_lamb_moments_batch, "moments", *tables([p, g, m, v, u]),
                                cnt, nb, kdt, args.np, hl, stream))
        pp = [p[s][o:o + c] for s, o, c in pieces]
        uu = [u[s][o:o + c] for s, o, c in pieces]
        plan = ops.LambApplyPlan(pp, uu, list(range(P)), P,
                                 [p16[s][o:o + c] for s, o, c in pieces] if master else None)
        sn = ops.SegNorm(pp + uu)
        out = torch.zeros(2 * P + 1, dtype=torch.float64, device=dev)
        keep.append((plan, sn, out))
        apply_.append(lambda plan=plan: plan.run(nlr))
        norm.append(lambda sn=sn, out=out: sn.run("sq", out=out))
    # every kind starts on a copy of its own: none finds the buffers the
    # call before it touched in the Infinity Cache
    turn = lambda xs, k: xs[k % copies:] + xs[:k % copies]  # noqa: E731

    def trust():
        ops.lamb_trust_update_(sq, 1, group_of, [{"lr": 1e-3, "adapt": True}], nlr, ratio)

    fns = {"adam": adam, "moments": turn(moments, 1), "norm": turn(norm, 2),
           "apply": turn(apply_, 3), "trust": [trust]}
    us = b0.time_calls(fns, args.reps, args.warmup)
    bytes_per = {"adam": 28, "moments": 26 if master else 28, "norm": 8,
                 "apply": 14 if master else 12}
    row = {"what": "LAMB kernels against the Adam kernel", "case": name, "dtype": dname,
           "elements": n, "segments": nb, "pieces": P, "copies": copies, "np": args.np,
           "lamb": "weight_decay 1e-2, step 7, eps 1e-6"}
    for k in fns:
        row[k] = b0.stats(us[k])
        if k in bytes_per:
            row[k]["bytes_per_element"] = bytes_per[k]
            row[k]["fraction_of_8TBps"] = round(
                bytes_per[k] * n / (row[k]["median_us"] * 1e-6) / b0.HBM_PEAK, 4)
    y = row["adam"]
    width = y["p90_us"] - y["p10_us"]
    for k, share in (("moments", 1.0), ("apply", 12.0 / 28.0)):
        goal = share * y["median_us"] + width
        row[k]["goal_us"] = round(goal, 3)
        row[k]["over_adam"] = round(row[k]["median_us"] / y["median_us"], 4)
        row[k]["goal_met"] = row[k]["median_us"] <= goal
    lamb_total = sum(row[k]["median_us"] for k in ("moments", "norm", "trust", "apply"))
    row["norm_share_of_lamb_kernels"] = round(row["norm"]["median_us"] / lamb_total, 4)
    b0.emit(row, args)


def step_world1(args):
    from kungfu_amd.optimizers import ShardedAdamOptimizer, ShardedLAMBOptimizer
    dev = torch.device("cuda:0")
    pl, pa = b0.make_model(dev), b0.make_model(dev)
    lamb = ShardedLAMBOptimizer(torch.optim.AdamW(pl, lr=1e-3, weight_decay=1e-2, eps=1e-6))
    adam = ShardedAdamOptimizer(torch.optim.AdamW(pa, lr=1e-3, weight_decay=1e-2))
    b0.give_grads(pl, dev)
    b0.give_grads(pa, dev)
    us = b0.time_calls({"lamb": [lamb.step], "adam": [adam.step]}, args.steps, args.warmup)
    row = {"what": "step time, world 1 (for information)", "model": "resnet50-imagenet",
           "dtype": "float32", "elements": sum(b0.model_sizes()),
           "optimizer": "AdamW, lr 1e-3, weight_decay 1e-2",
           "lamb": b0.stats(us["lamb"]), "adam": b0.stats(us["adam"]),
           "pieces": sum(len(L["owners"]) for L in lamb._kf_lamb)}
    row["lamb_over_adam"] = round(row["lamb"]["median_us"] / row["adam"]["median_us"], 4)
    b0.emit(row, args)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--what", default="kernel,step1", help="comma list of kernel, step1")
    ap.add_argument("--reps", type=int, default=100, help="timed kernel calls per kind")
    ap.add_argument("--steps", type=int, default=40, help="timed steps per optimizer, world 1")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--np", type=int, default=8, help="the moments' /np (0: none)")
    ap.add_argument("--kernel-cases", default="full,shard", help="comma list of full, shard")
    ap.add_argument("--dtypes", default="float32,bfloat16",
                    help="comma list of float32, bfloat16, float16")
    ap.add_argument("--out", default=None, help="append the JSON lines here")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_sharded_lamb: needs a GPU (no CPU path)")
    what = args.what.split(",")
    cases = [(c, n, s) for c, n, s in (("full", "resnet50, 16 buckets", 1),
                                       ("shard", "resnet50, 16 shards of 1/8", 8))
             if c in args.kernel_cases]
    for _, name, shard_of in cases if "kernel" in what else []:
        for dname in args.dtypes.split(","):
            kernel_case(name, shard_of, dname, args)
    if "step1" in what:
        step_world1(args)


if __name__ == "__main__":
    main()
