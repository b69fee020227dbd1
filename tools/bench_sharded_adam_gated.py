#!/usr/bin/env python3
"""Measure the gated Adam step (kf_adam_update_batch_gated,
kf_adam_master_update_batch_gated, kf_step_gate_update,
ShardedAdamOptimizer(max_grad_norm, loss_scale)) by
tools/bench_sharded_adam_master.py's method: ResNet-50's 25,583,592 elements
in 16 buckets and in 16 shards of 1/8, AdamW with weight_decay 1e-2, np = 8,
every call between its own pair of HIP events, 10 warm-up calls, then 100
calls rotating over copies of the buffers that together exceed the L2 and the
Infinity Cache; medians with the 10th and 90th percentiles.

  kernel  In one loop, on the same element count, call by call: each ungated
          parent kernel (f32 kf_adam_update_batch; bf16 and f16
          kf_adam_master_update_batch) and its gated twin under an open gate
          (skip 0, grad_mul 0.37). GOAL, recorded and not a gate: the gated
          kernel's median is at most its parent's median plus the parent's
          own p90 - p10 width in that run. A skipped launch is timed too.
  verdict For information: steps B to D on one rank, the norm pass over the
          gradient shards (2 or 4 bytes per element, ops.SegNorm) and the
          one-lane gate launch, each timed alone.
  step1   For information: step() at world 1 on a bf16 model with master
          weights, gated (max_grad_norm 1.0, dynamic loss scale) and ungated
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
import bench_sharded_adam_master as b1  # noqa: E402  (the 16-bit model and its gradients)

DT = {"float32": torch.float32, "bfloat16": torch.bfloat16, "float16": torch.float16}
GATED_HYPER = {k: v for k, v in b0.ADAM.items() if k != "step"}


def open_gate(dev, skip=0):
    """A gate and one group's step state as a verdict leaves them after
    b0.ADAM's 7 applied steps."""
    import numpy as np
    from kungfu_amd import _lib
    b1_, b2_ = b0.ADAM["betas"]
    t = b0.ADAM["step"]
    g = np.zeros(1, _lib.step_gate_dtype())
    g["skip"], g["grad_mul"], g["loss_scale"] = skip, 0.37, 1.0
    s = np.zeros(1, _lib.step_state_dtype())
    s["beta1_pow"], s["beta2_pow"], s["step"] = b1_ ** t, b2_ ** t, t
    s["s2_f64"] = (1.0 - b2_ ** t) ** 0.5
    s["nss_f64"] = -(b0.ADAM["lr"] / (1.0 - b1_ ** t))
    s["s2"], s["nss"] = s["s2_f64"], s["nss_f64"]
    return [torch.from_numpy(a.view(np.uint8).copy()).to(dev) for a in (g, s)]


def kernel_case(name, shard_of, args):
    from kungfu_amd import _lib, ops
    from kungfu_amd.collective import GradBuckets
    dev = torch.device("cuda:0")
    sizes = b0.model_sizes()
    gen = torch.Generator(device=dev).manual_seed(1)

    def segs(gb):
        return [b[:b.numel() // shard_of] for b in gb.buckets]

    def filled(dtype, square=False):
        gb = GradBuckets(sizes, dtype, dev, shard_of, n_buckets=16)
        for f in gb.flats:
            r = torch.randn(f.numel(), device=dev, generator=gen)
            f.copy_(r * r if square else r)  # exp_avg_sq is not negative
        return segs(gb)

    probe = segs(GradBuckets(sizes, torch.float32, dev, shard_of, n_buckets=16))
    n, nb = sum(s.numel() for s in probe), len(probe)
    counts = [s.numel() for s in probe]
    del probe
    copies = max(2, -(-b0.ROTATE_BYTES // (16 * n)))
    f32 = torch.float32
    lib = _lib.load()
    ha = _lib.adam_hyper_array([b0.ADAM] * nb)
    hg = _lib.adam_hyper_array([dict(GATED_HYPER, step=1)])
    cnt = (ctypes.c_size_t * nb)(*counts)
    stream = torch.cuda.current_stream(dev).cuda_stream
    gate, state = open_gate(dev)
    shut, _ = open_gate(dev, skip=1)
    keep = [gate, state, shut]

    def tables(bufs):
        keep.append(bufs)
        return [_lib.ptr_array([t.data_ptr() for t in ts]) for ts in bufs]

    def call(fn, what, *a):
        def run():
            _lib.check(fn(*a), what, source="")
        return run

    fns, pairs = {}, []
    for dname in args.dtypes.split(","):
        dt = DT[dname]
        kdt = int(ops.kungfu_dtype(torch.empty(1, dtype=dt, device=dev)))
        if dt == f32:
            sets = [tables([filled(f32), filled(f32), filled(f32), filled(f32, True)])
                    for _ in range(copies)]
            parent, gated = lib.kf_adam_update_batch, lib.kf_adam_update_batch_gated
        else:
            sets = [tables([filled(dt), filled(dt), filled(f32), filled(f32), filled(f32, True)])
                    for _ in range(copies)]
            parent, gated = lib.kf_adam_master_update_batch, lib.kf_adam_master_update_batch_gated
        fns[dname] = [call(parent, "parent", *t, cnt, nb, kdt, args.np, ha, stream) for t in sets]
        # the twin starts on another copy: it never finds the parent's
        # buffers in the Infinity Cache
        turned = sets[1:] + sets[:1]
        fns[dname + ":gated"] = [call(gated, "gated", *t, cnt, nb, kdt, args.np, hg,
                                      gate.data_ptr(), state.data_ptr(), stream) for t in turned]
        fns[dname + ":skipped"] = [call(gated, "gated", *t, cnt, nb, kdt, args.np, hg,
                                        shut.data_ptr(), state.data_ptr(), stream) for t in turned]
        pairs.append(dname)
    us = b0.time_calls(fns, args.reps, args.warmup)
    row = {"what": "gated kernels against their ungated parents", "case": name, "elements": n,
           "segments": nb, "copies": copies, "np": args.np, "bytes_per_element": 28,
           "adam": "AdamW, weight_decay 1e-2, step 7, grad_mul 0.37"}
    for k in fns:
        row[k] = b0.stats(us[k])
        if not k.endswith(":skipped"):
            row[k]["fraction_of_8TBps"] = round(28 * n / (row[k]["median_us"] * 1e-6) / b0.HBM_PEAK, 4)
    for d in pairs:
        y, g = row[d], row[d + ":gated"]
        goal = y["median_us"] + (y["p90_us"] - y["p10_us"])
        g["goal_us"] = round(goal, 3)
        g["over_parent"] = round(g["median_us"] / y["median_us"], 4)
        g["goal_met"] = g["median_us"] <= goal
    b0.emit(row, args)


def verdict_case(name, shard_of, args):
    from kungfu_amd import ops
    from kungfu_amd.collective import GradBuckets
    dev = torch.device("cuda:0")
    sizes = b0.model_sizes()
    gen = torch.Generator(device=dev).manual_seed(4)
    row = {"what": "steps B and D of a gated step (for information)", "case": name}
    for dname in args.dtypes.split(","):
        dt = DT[dname]
        esz = torch.empty(0, dtype=dt).element_size()
        n = sum(b.numel() // shard_of
                for b in GradBuckets(sizes, dt, dev, shard_of, n_buckets=16).buckets)
        copies = max(2, -(-b0.ROTATE_BYTES // (esz * n)))
        plans, outs = [], []
        for _ in range(copies):
            gb = GradBuckets(sizes, dt, dev, shard_of, n_buckets=16)
            for f in gb.flats:
                f.copy_(torch.randn(f.numel(), device=dev, generator=gen))
            shards = [b[:b.numel() // shard_of] for b in gb.buckets]
            plans.append((ops.SegNorm(shards), gb))
            outs.append(torch.zeros(len(shards) + 1, dtype=torch.float64, device=dev))
        gate, states = ops.new_step_gate(dev, 65536.0), ops.new_step_states(dev, 1)
        sq = outs[0][-1:]
        hs = [GATED_HYPER]

        def norm(i):
            return lambda: plans[i][0].run("sq", out=outs[i])

        def verdict():
            ops.step_gate_update_(sq, 1, [args.np], hs, states, gate, max_norm=1.0,
                                  growth_factor=2.0, backoff_factor=0.5, growth_interval=2000)

        us = b0.time_calls({"norm": [norm(i) for i in range(copies)], "gate": [verdict]},
                           args.reps, args.warmup)
        row[dname] = {"elements": n, "bytes_per_element": esz, "copies": copies,
                      "norm_pass": b0.stats(us["norm"]), "gate_launch": b0.stats(us["gate"])}
        row[dname]["norm_pass"]["fraction_of_8TBps"] = round(
            esz * n / (row[dname]["norm_pass"]["median_us"] * 1e-6) / b0.HBM_PEAK, 4)
    b0.emit(row, args)


def step_world1(args):
    from kungfu_amd.optimizers import ShardedAdamOptimizer
    dev = torch.device("cuda:0")
    dtype = torch.bfloat16
    pg, pp = b1.make_model(dev, dtype), b1.make_model(dev, dtype)
    gated = ShardedAdamOptimizer(torch.optim.AdamW(pg, lr=1e-3, weight_decay=1e-2),
                                 master_weights=True, max_grad_norm=1.0, loss_scale="dynamic")
    plain = ShardedAdamOptimizer(torch.optim.AdamW(pp, lr=1e-3, weight_decay=1e-2),
                                 master_weights=True)
    b1.give_grads(pg, dev)
    b1.give_grads(pp, dev)
    us = b0.time_calls({"gated": [gated.step], "ungated": [plain.step]}, args.steps, args.warmup)
    row = {"what": "step time, world 1 (for information)", "model": "resnet50-imagenet",
           "dtype": "bfloat16", "elements": sum(b0.model_sizes()),
           "optimizer": "AdamW, lr 1e-3, weight_decay 1e-2, master weights",
           "gated": b0.stats(us["gated"]), "ungated": b0.stats(us["ungated"]),
           "steps_taken": args.warmup + args.steps, "applied_steps": gated.applied_steps(),
           "skipped_steps": gated.skipped_steps(), "last_grad_norm": gated.last_grad_norm()}
    row["gated_over_ungated"] = round(row["gated"]["median_us"] / row["ungated"]["median_us"], 4)
    b0.emit(row, args)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--what", default="kernel,verdict,step1",
                    help="comma list of kernel, verdict, step1")
    ap.add_argument("--reps", type=int, default=100, help="timed kernel calls per kind")
    ap.add_argument("--steps", type=int, default=40, help="timed steps per optimizer, world 1")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--np", type=int, default=8, help="the update's /np (0: none)")
    ap.add_argument("--kernel-cases", default="full,shard", help="comma list of full, shard")
    ap.add_argument("--dtypes", default="float32,bfloat16,float16",
                    help="comma list of float32, bfloat16, float16")
    ap.add_argument("--out", default=None, help="append the JSON lines here")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_sharded_adam_gated: needs a GPU (no CPU path)")
    what = args.what.split(",")
    cases = [(c, n, s) for c, n, s in (("full", "resnet50, 16 buckets", 1),
                                       ("shard", "resnet50, 16 shards of 1/8", 8))
             if c in args.kernel_cases]
    for _, name, shard_of in cases if "kernel" in what else []:
        kernel_case(name, shard_of, args)
    for _, name, shard_of in cases if "verdict" in what else []:
        verdict_case(name, shard_of, args)
    if "step1" in what:
        step_world1(args)


if __name__ == "__main__":
    main()
