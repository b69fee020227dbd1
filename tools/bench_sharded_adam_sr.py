#!/usr/bin/env python3
"""Measure the stochastic-rounding Adam update (kf_adam_sr_update_batch,
ShardedAdamOptimizer(stochastic_rounding=True)) by
tools/bench_sharded_lamb.py's method: ResNet-50's 25,583,592 elements as bf16
in 16 buckets and in 16 shards of 1/8, weight_decay 1e-2, np = 8, every call
between its own pair of HIP events, 10 warm-up calls, then 100 calls rotating
over copies of the buffers that together exceed the L2 and the Infinity Cache;
medians with the 10th and 90th percentiles.

  kernel  In one loop, on buffers of the same lengths, call by call: the pure
          bf16 kernel (kf_adam_update_batch, 14 bytes per element), the master
          kernel (kf_adam_master_update_batch, 28 bytes) and the
          stochastic-rounding kernel (14 bytes). kf_adam.hip and
          kf_adam_master.hip are the parent commit's files, unchanged. GOAL,
          recorded and not a gate: the SR median is at most the bf16 Adam
          median plus that kernel's own p90 - p10 width in the same run.
          FLOOR of usefulness: the SR median is below the master kernel's.
  step1   For information: step() at world 1 on a bf16 model, the pure-bf16,
          the master-weights and the stochastic-rounding optimizers
          alternating in one loop.

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


def kernel_case(name, shard_of, args):
    from kungfu_amd import _lib, ops
    from kungfu_amd.collective import GradBuckets
    dev = torch.device("cuda:0")
    bf16, f32 = torch.bfloat16, torch.float32
    sizes = b0.model_sizes()
    gen = torch.Generator(device=dev).manual_seed(1)
    layout = GradBuckets(sizes, bf16, dev, shard_of, n_buckets=16)
    counts = [b.numel() // shard_of for b in layout.buckets]
    n, nb = sum(counts), len(counts)
    del layout

    def filled(dtype, square=False):
        out = []
        for c in counts:
            r = torch.randn(c, device=dev, generator=gen)
            out.append((r * r if square else r).to(dtype))  # exp_avg_sq is not negative
        return out

    copies = max(2, -(-b0.ROTATE_BYTES // (8 * n)))
    lib = _lib.load()
    ha = _lib.adam_hyper_array([b0.ADAM] * nb)
    cnt = (ctypes.c_size_t * nb)(*counts)
    bases = (ctypes.c_uint64 * nb)(*[0] * nb)
    streams = (ctypes.c_uint32 * nb)(*range(1, nb + 1))
    stream = torch.cuda.current_stream(dev).cuda_stream
    kdt = int(ops.kungfu_dtype(torch.empty(1, dtype=bf16, device=dev)))
    keep = []

    def tables(bufs):
        keep.append(bufs)
        return [_lib.ptr_array([t.data_ptr() for t in ts]) for ts in bufs]

    def call(fn, what, *a):
        def run():
            _lib.check(fn(*a), what, source="")
        return run

    adam, master, sr = [], [], []
    for i in range(copies):
        p, g, m, v = filled(bf16), filled(bf16), filled(bf16), filled(bf16, True)
        adam.append(call(lib.kf_adam_update_batch, "adam", *tables([p, g, m, v]), cnt, nb, kdt,
                         args.np, ha, stream))
        p, g, m, v = filled(bf16), filled(bf16), filled(bf16), filled(bf16, True)
        sr.append(call(lib.kf_adam_sr_update_batch, "sr", *tables([p, g, m, v]), cnt, bases,
                       streams, nb, kdt, args.np, ha, 1 + i, stream))
        p16, g, w, m, v = filled(bf16), filled(bf16), filled(f32), filled(f32), filled(f32, True)
        master.append(call(lib.kf_adam_master_update_batch, "master", *tables([p16, g, w, m, v]),
                           cnt, nb, kdt, args.np, ha, stream))
    fns = {"adam_bf16": adam, "sr": sr, "master": master}
    us = b0.time_calls(fns, args.reps, args.warmup)
    bytes_per = {"adam_bf16": 14, "sr": 14, "master": 28}
    row = {"what": "stochastic-rounding Adam kernel against the bf16 and master kernels",
           "case": name, "dtype": "bfloat16", "elements": n, "segments": nb, "copies": copies,
           "np": args.np, "adam": "AdamW, weight_decay 1e-2, step 7"}
    for k in fns:
        row[k] = b0.stats(us[k])
        row[k]["bytes_per_element"] = bytes_per[k]
        row[k]["fraction_of_8TBps"] = round(
            bytes_per[k] * n / (row[k]["median_us"] * 1e-6) / b0.HBM_PEAK, 4)
    y = row["adam_bf16"]
    goal = y["median_us"] + (y["p90_us"] - y["p10_us"])
    row["sr"]["goal_us"] = round(goal, 3)
    row["sr"]["over_adam_bf16"] = round(row["sr"]["median_us"] / y["median_us"], 4)
    row["sr"]["goal_met"] = row["sr"]["median_us"] <= goal
    row["sr"]["over_master"] = round(row["sr"]["median_us"] / row["master"]["median_us"], 4)
    row["sr"]["floor_met"] = row["sr"]["median_us"] < row["master"]["median_us"]
    b0.emit(row, args)


def step_world1(args):
    from kungfu_amd.optimizers import ShardedAdamOptimizer
    dev = torch.device("cuda:0")

    def model():
        ps = b0.make_model(dev)
        for p in ps:
            p.data = p.data.to(torch.bfloat16)
        gen = torch.Generator(device=dev).manual_seed(3)
        for p in ps:
            p.grad = torch.randn(p.numel(), device=dev, generator=gen).to(torch.bfloat16)
        return ps

    kinds = {"bf16": {}, "master": {"master_weights": True}, "sr": {"stochastic_rounding": True}}
    opts = {k: ShardedAdamOptimizer(torch.optim.AdamW(model(), lr=1e-3, weight_decay=1e-2), **kw)
            for k, kw in kinds.items()}
    us = b0.time_calls({k: [o.step] for k, o in opts.items()}, args.steps, args.warmup)
    row = {"what": "step time, world 1 (for information)", "model": "resnet50-imagenet",
           "dtype": "bfloat16", "elements": sum(b0.model_sizes()),
           "optimizer": "AdamW, lr 1e-3, weight_decay 1e-2"}
    for k in kinds:
        row[k] = b0.stats(us[k])
    row["sr_over_bf16"] = round(row["sr"]["median_us"] / row["bf16"]["median_us"], 4)
    row["sr_over_master"] = round(row["sr"]["median_us"] / row["master"]["median_us"], 4)
    b0.emit(row, args)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--what", default="kernel,step1", help="comma list of kernel, step1")
    ap.add_argument("--reps", type=int, default=100, help="timed kernel calls per kind")
    ap.add_argument("--steps", type=int, default=40, help="timed steps per optimizer, world 1")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--np", type=int, default=8, help="the update's /np (0: none)")
    ap.add_argument("--kernel-cases", default="full,shard", help="comma list of full, shard")
    ap.add_argument("--out", default=None, help="append the JSON lines here")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_sharded_adam_sr: needs a GPU (no CPU path)")
    what = args.what.split(",")
    cases = [(c, n, s) for c, n, s in (("full", "resnet50, 16 buckets", 1),
                                       ("shard", "resnet50, 16 shards of 1/8", 8))
             if c in args.kernel_cases]
    for _, name, shard_of in cases if "kernel" in what else []:
        kernel_case(name, shard_of, args)
    if "step1" in what:
        step_world1(args)


if __name__ == "__main__":
    main()
