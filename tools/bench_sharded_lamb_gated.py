#!/usr/bin/env python3
"""Measure the LAMB step under a gate (kf_lamb_moments_batch_gated,
kf_lamb_master_moments_batch_gated, kf_lamb_trust_update_gated,
kf_lamb_apply_run_gated, ShardedLAMBOptimizer(gate=...)) by
tools/bench_sharded_lamb.py's method and on its buffers: ResNet-50's
25,583,592 elements in 16 buckets and in 16 shards of 1/8, weight_decay 1e-2,
np = 8, every call between its own pair of HIP events, 10 warm-up calls, then
100 calls rotating over copies of the buffers that together exceed the L2 and
the Infinity Cache; medians with the 10th and 90th percentiles.

  kernel  In one loop, call by call: every gated kernel and its ungated parent
          (moments, trust, apply) on the same element count, the gate holding
          skip = 0 and grad_mul = 0.37. GOAL, the project's standing rule: a
          gated median is at most its parent's median plus the parent's own
          p90 - p10 width in that run (--gated-first swaps the two in a round:
          a kernel called straight after another large one runs slower than
          after a small one). For information, without a goal: the
          same gated launches under skip = 1, and the gradient-norm pass over
          the gradient segments.
  step1   For information: step() at world 1 on an f32 model,
          ShardedLAMBOptimizer with gate={"max_grad_norm": 1.0} and without a
          gate alternating in one loop.

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

import bench_sharded_adam as b0  # noqa: E402  (pct, stats, time_calls, emit, the model)
import bench_sharded_lamb as b1  # noqa: E402  (the pieces, the LAMB hyper)

DT, LAMB = b1.DT, b1.LAMB
GRAD_MUL, STEP = 0.37, 7


def device_gate(dev, skip):
    """(gate, states): as a verdict with lr = 1 leaves them after STEP applied
    steps at LAMB's betas, grad_mul = GRAD_MUL."""
    import numpy as np
    from kungfu_amd import _lib
    b1_, b2_ = LAMB["betas"]
    g = np.zeros(1, _lib.step_gate_dtype())
    g["skip"], g["grad_mul"], g["loss_scale"] = skip, GRAD_MUL, 1.0
    s = np.zeros(1, _lib.step_state_dtype())
    s["beta1_pow"], s["beta2_pow"], s["step"] = b1_ ** STEP, b2_ ** STEP, STEP
    s["s2_f64"] = (1.0 - b2_ ** STEP) ** 0.5
    s["nss_f64"] = -(1.0 / (1.0 - b1_ ** STEP))
    s["s2"], s["nss"] = s["s2_f64"], s["nss_f64"]
    return (torch.from_numpy(g.view(np.uint8).copy()).to(dev),
            torch.from_numpy(s.view(np.uint8).copy()).to(dev))


def kernel_case(name, shard_of, dname, args):
    from kungfu_amd import _lib, ops
    from kungfu_amd.collective import GradBuckets
    dev = torch.device("cuda:0")
    dt, f32 = DT[dname], torch.float32
    master = dt != f32
    sizes = b0.model_sizes()
    gen = torch.Generator(device=dev).manual_seed(1)
    layout = GradBuckets(sizes, f32, dev, shard_of, n_buckets=16)
    counts = [b.numel() // shard_of for b in layout.buckets]
    pieces = b1.pieces_of(sizes, layout, shard_of)
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
    hl = _lib.adam_hyper_array([LAMB] * nb)
    one = _lib.adam_hyper_array([LAMB])
    cnt = (ctypes.c_size_t * nb)(*counts)
    stream = torch.cuda.current_stream(dev).cuda_stream
    kdt = int(ops.kungfu_dtype(torch.empty(1, dtype=dt, device=dev)))
    gates = {0: device_gate(dev, 0), 1: device_gate(dev, 1)}
    keep = [gates]

    def tables(bufs):
        keep.append(bufs)
        return [_lib.ptr_array([t.data_ptr() for t in ts]) for ts in bufs]

    def call(fn, what, *a):
        def run():
            _lib.check(fn(*a), what, source="")
        return run

    P = len(pieces)
    f64 = dict(dtype=torch.float64, device=dev)
    nlr, ratio = torch.full((P,), -1e-3, **f64), torch.ones(P, **f64)
    group_of = torch.zeros(P, dtype=torch.int32, device=dev)
    sq = torch.ones(2 * P, **f64)
    kinds = ("moments", "moments_gated", "moments_skipped", "apply", "apply_gated",
             "apply_skipped", "grad_norm")
    if args.gated_first:  # the pair's order in a round, to tell a kernel's time from its place
        kinds = ("moments_gated", "moments", "moments_skipped", "apply_gated", "apply",
                 "apply_skipped", "grad_norm")
    fns = {k: [] for k in kinds}
    for _ in range(copies):
        p16 = filled(dt) if master else None
        g, p, m, v, u = filled(dt), filled(f32), filled(f32), filled(f32, True), filled(f32)
        tabs = tables([g, p, m, v, u] if master else [p, g, m, v, u])
        parent = lib.kf_lamb_master_moments_batch if master else lib.kf_lamb_moments_batch
        child = lib.kf_lamb_master_moments_batch_gated if master else \
            lib.kf_lamb_moments_batch_gated
        fns["moments"].append(call(parent, "moments", *tabs, cnt, nb, kdt, args.np, hl, stream))
        for k, skip in (("moments_gated", 0), ("moments_skipped", 1)):
            gate, st = gates[skip]
            fns[k].append(call(child, k, *tabs, cnt, nb, kdt, args.np, one, gate.data_ptr(),
                               st.data_ptr(), stream))
        pp = [p[s][o:o + c] for s, o, c in pieces]
        uu = [u[s][o:o + c] for s, o, c in pieces]
        plan = ops.LambApplyPlan(pp, uu, list(range(P)), P,
                                 [p16[s][o:o + c] for s, o, c in pieces] if master else None)
        sn = ops.SegNorm(g)
        out = torch.zeros(nb + 1, **f64)
        keep.append((plan, sn, out))
        fns["apply"].append(lambda plan=plan: plan.run(nlr))
        fns["apply_gated"].append(lambda plan=plan: plan.run(nlr, gate=gates[0][0]))
        fns["apply_skipped"].append(lambda plan=plan: plan.run(nlr, gate=gates[1][0]))
        fns["grad_norm"].append(lambda sn=sn, out=out: sn.run("sq", out=out))
    # every kind starts on a copy of its own: none finds the buffers the call
    # before it touched in the Infinity Cache
    turn = lambda xs, k: xs[k % copies:] + xs[:k % copies]  # noqa: E731
    fns = {k: turn(f, i) for i, (k, f) in enumerate(fns.items())}
    groups = [{"lr": 1e-3, "adapt": True}]
    fns["trust"] = [lambda: ops.lamb_trust_update_(sq, 1, group_of, groups, nlr, ratio)]
    for k, skip in (("trust_gated", 0), ("trust_skipped", 1)):
        fns[k] = [lambda skip=skip: ops.lamb_trust_update_gated_(sq, 1, group_of, groups, nlr,
                                                                 ratio, gates[skip][0])]
    us = b0.time_calls(fns, args.reps, args.warmup)
    bytes_per = {"moments": 26 if master else 28, "apply": 14 if master else 12,
                 "grad_norm": 2 if master else 4}
    row = {"what": "gated LAMB kernels against their parents", "case": name, "dtype": dname,
           "elements": n, "segments": nb, "pieces": P, "copies": copies, "np": args.np,
           "order": "gated first" if args.gated_first else "parent first",
           "lamb": "weight_decay 1e-2, step %d, eps 1e-6, grad_mul %g" % (STEP, GRAD_MUL)}
    for k in fns:
        row[k] = b0.stats(us[k])
        base = k.split("_")[0] if k != "grad_norm" else k
        if base in bytes_per and not k.endswith("_skipped"):
            row[k]["bytes_per_element"] = bytes_per[base]
            row[k]["fraction_of_8TBps"] = round(
                bytes_per[base] * n / (row[k]["median_us"] * 1e-6) / b0.HBM_PEAK, 4)
    for k in ("moments", "trust", "apply"):
        y, z = row[k], row[k + "_gated"]
        goal = y["median_us"] + (y["p90_us"] - y["p10_us"])
        z["goal_us"] = round(goal, 3)
        z["over_parent"] = round(z["median_us"] / y["median_us"], 4)
        z["goal_met"] = z["median_us"] <= goal
    b0.emit(row, args)


def step_world1(args):
    from kungfu_amd.optimizers import ShardedLAMBOptimizer
    dev = torch.device("cuda:0")
    pg, pu = b0.make_model(dev), b0.make_model(dev)
    new = lambda ps, **kw: ShardedLAMBOptimizer(  # noqa: E731
        torch.optim.AdamW(ps, lr=1e-3, weight_decay=1e-2, eps=1e-6), **kw)
    gated, plain = new(pg, gate={"max_grad_norm": 1.0}), new(pu)
    b0.give_grads(pg, dev)
    b0.give_grads(pu, dev)
    us = b0.time_calls({"gated": [gated.step], "ungated": [plain.step]}, args.steps, args.warmup)
    row = {"what": "step time, world 1 (for information)", "model": "resnet50-imagenet",
           "dtype": "float32", "elements": sum(b0.model_sizes()),
           "optimizer": "AdamW, lr 1e-3, weight_decay 1e-2", "gate": "max_grad_norm 1.0",
           "gated": b0.stats(us["gated"]), "ungated": b0.stats(us["ungated"]),
           "applied_steps": gated.applied_steps(), "skipped_steps": gated.skipped_steps()}
    row["gated_over_ungated"] = round(row["gated"]["median_us"] / row["ungated"]["median_us"], 4)
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
    ap.add_argument("--gated-first", action="store_true",
                    help="call every gated kernel before its parent in a round")
    ap.add_argument("--out", default=None, help="append the JSON lines here")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_sharded_lamb_gated: needs a GPU (no CPU path)")
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
