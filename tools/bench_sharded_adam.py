#!/usr/bin/env python3
"""Measure the sharded Adam step (ShardedAdamOptimizer, kf_adam_update_batch).

Model: ResNet-50's 25,583,592 fp32 (tests/golden/models.json), AdamW with
torch's defaults and weight_decay 1e-2.

  kernel  (a) kf_adam_update_batch over the model in 16 buckets
          (GradBuckets(n_buckets=16)) and over the shard form (1/8 of every
          bucket), as a fraction of the 8 TB/s HBM peak: 7 accesses per
          element (g, p, m, v read; p, m, v written). Beside it
          kf_sgd_update_batch with momentum on the same param, grad and
          exp_avg buffers in the same loop (5 accesses). Calls rotate over
          copies of the buffers that together exceed the L2 and the 256 MiB
          Infinity Cache. --dtypes adds bfloat16 / float64 rows.
  step1   (b) step() at world 1, the two optimizers alternating in one loop
          over the same model, gradients and bucket layout:
            new     ShardedAdamOptimizer(AdamW).step()
            parent  SynchronousSGDOptimizer(AdamW).step()
          GATE: new / parent <= 1.0 on the median (exit status 1 otherwise).
          Also the largest parameter difference between the two after all
          the steps (warm-up + timed = 50 by default).
  memory  (c) optimizer-state bytes per rank: measured on the world-1
          optimizer's shards, and from the bucket layout at world 8.

Every timed call sits between its own pair of HIP events; times are medians
in microseconds with the 10th and 90th percentiles. One JSON object per line
goes to --out (and stdout).
"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

HBM_PEAK = 8.0e12  # bytes / s, the roofline the project quotes against
ROTATE_BYTES = 640 << 20  # more than L2 + Infinity Cache
ADAM = {"lr": 1e-3, "betas": (0.9, 0.999), "eps": 1e-8, "weight_decay": 1e-2, "decoupled": True,
        "step": 7}
SGD = {"lr": 0.1, "momentum": 0.9, "dampening": 0.0, "weight_decay": 0.0, "nesterov": False,
       "first": False}


def pct(xs, q):
    xs = sorted(xs)
    return xs[min(len(xs) - 1, int(q * len(xs)))]


def stats(us):
    return {"median_us": round(pct(us, 0.5), 3), "p10_us": round(pct(us, 0.1), 3),
            "p90_us": round(pct(us, 0.9), 3), "reps": len(us)}


def time_calls(fns, reps, warmup):
    """fns: name -> list of callables; round i calls fns[k][i % len] for every
    k in turn, each between its own pair of events."""
    for i in range(warmup):
        for f in fns.values():
            f[i % len(f)]()
    torch.cuda.synchronize()
    evs = {k: [] for k in fns}
    for i in range(reps):
        for k, f in fns.items():
            a = torch.cuda.Event(enable_timing=True)
            b = torch.cuda.Event(enable_timing=True)
            a.record()
            f[i % len(f)]()
            b.record()
            evs[k].append((a, b))
    torch.cuda.synchronize()
    return {k: [1e3 * a.elapsed_time(b) for a, b in e] for k, e in evs.items()}


def emit(row, args):
    row["device"] = torch.cuda.get_device_name(0)
    line = json.dumps(row)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as fo:
            fo.write(line + "\n")


def model_sizes():
    with open(os.path.join(ROOT, "tests", "golden", "models.json")) as f:
        return json.load(f)["resnet50-imagenet"]


# ---- (a) the kernel ----------------------------------------------------------

def kernel_case(name, shard_of, dtype, args):
    from kungfu_amd import _lib, ops
    from kungfu_amd.collective import GradBuckets
    dev = torch.device("cuda:0")
    sizes = model_sizes()
    g = torch.Generator(device=dev).manual_seed(1)
    isz = torch.empty(0, dtype=dtype).element_size()

    def segs(gb):
        return [b[:b.numel() // shard_of] for b in gb.buckets]

    world = shard_of
    probe = GradBuckets(sizes, dtype, dev, world, n_buckets=16)
    n = sum(s.numel() for s in segs(probe))
    copies = max(2, -(-ROTATE_BYTES // (4 * isz * n)))
    del probe
    sets = []
    for _ in range(copies):
        bufs = []
        for k in range(4):  # params, grads, exp_avg (SGD's momentum), exp_avg_sq
            gb = GradBuckets(sizes, dtype, dev, world, n_buckets=16)
            for f in gb.flats:
                r = torch.randn(f.numel(), device=dev, generator=g)
                f.copy_(r * r if k == 3 else r)  # exp_avg_sq is not negative
            bufs.append(segs(gb))
        sets.append(bufs)
    # the C entry points themselves, on tables built once: the Python
    # wrappers' per-call list handling (tens of microseconds) is not the kernel
    lib = _lib.load()
    nb = len(sets[0][0])
    ha = _lib.adam_hyper_array([ADAM] * nb)
    hs = _lib.sgd_hyper_array([SGD] * nb)
    cnt = (ctypes.c_size_t * nb)(*[t.numel() for t in sets[0][0]])
    kdt = int(ops.kungfu_dtype(sets[0][0][0]))
    stream = torch.cuda.current_stream(dev).cuda_stream

    def tables(s):
        return [_lib.ptr_array([t.data_ptr() for t in ts]) for ts in s]

    def adam(t):
        def run():
            _lib.check(lib.kf_adam_update_batch(t[0], t[1], t[2], t[3], cnt, nb, kdt, args.np, ha,
                                                stream), "kf_adam_update_batch", source="")
        return run

    def sgd(t):
        def run():
            _lib.check(lib.kf_sgd_update_batch(t[0], t[1], t[2], cnt, nb, kdt, args.np, hs, stream),
                       "kf_sgd_update_batch", source="")
        return run

    tabs = [tables(s) for s in sets]
    fns = {"adam_update": [adam(t) for t in tabs], "sgd_update": [sgd(t) for t in tabs]}
    us = time_calls(fns, args.reps, args.warmup)
    row = {"what": "kernel rate", "case": name, "dtype": str(dtype).replace("torch.", ""),
           "elements": n, "segments": nb, "copies": copies, "np": args.np,
           "adam": "AdamW, weight_decay 1e-2, step 7", "sgd": "momentum 0.9"}
    for k, acc in (("adam_update", 7), ("sgd_update", 5)):
        row[k] = stats(us[k])
        row[k]["accesses_per_element"] = acc
        row[k]["fraction_of_8TBps"] = round(acc * isz * n / (row[k]["median_us"] * 1e-6) / HBM_PEAK, 4)
    row["adam_minus_sgd_fraction"] = round(row["adam_update"]["fraction_of_8TBps"] -
                                           row["sgd_update"]["fraction_of_8TBps"], 4)
    emit(row, args)


# ---- (b), (c) the optimizers ---------------------------------------------------

def make_model(dev, seed=2):
    g = torch.Generator(device=dev).manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(n, device=dev, generator=g)) for n in model_sizes()]


def give_grads(ps, dev, seed=3):
    g = torch.Generator(device=dev).manual_seed(seed)
    for p in ps:
        p.grad = torch.randn(p.numel(), device=dev, generator=g)


def step_world1(args):
    from kungfu_amd.optimizers import ShardedAdamOptimizer, SynchronousSGDOptimizer
    dev = torch.device("cuda:0")
    pn, pp = make_model(dev), make_model(dev)
    new = ShardedAdamOptimizer(torch.optim.AdamW(pn, lr=1e-3, weight_decay=1e-2))
    parent = SynchronousSGDOptimizer(torch.optim.AdamW(pp, lr=1e-3, weight_decay=1e-2))
    give_grads(pn, dev)
    give_grads(pp, dev)
    walls = {"new": [], "parent": []}

    def timed(name, opt):
        def run():
            t0 = time.perf_counter()
            opt.step()
            walls[name].append(1e6 * (time.perf_counter() - t0))
        return run

    us = time_calls({"new": [timed("new", new)], "parent": [timed("parent", parent)]},
                    args.steps, args.warmup)
    # the same arithmetic up to torch's lerp and its fused a + alpha*b
    diff = max(float((a.detach() - b.detach()).abs().max()) for a, b in zip(pn, pp))
    row = {"what": "step time, world 1", "model": "resnet50-imagenet", "dtype": "float32",
           "elements": sum(model_sizes()), "optimizer": "AdamW, lr 1e-3, weight_decay 1e-2",
           "new": stats(us["new"]), "parent": stats(us["parent"]),
           "new_host_enqueue_us": round(pct(walls["new"][args.warmup:], 0.5), 1),
           "parent_host_enqueue_us": round(pct(walls["parent"][args.warmup:], 0.5), 1),
           "steps_taken": args.warmup + args.steps, "max_abs_param_difference": diff}
    row["new_over_parent"] = round(row["new"]["median_us"] / row["parent"]["median_us"], 4)
    row["gate_new_over_parent_le_1"] = row["new_over_parent"] <= 1.0
    emit(row, args)
    memory(new, parent, pp, args)
    return row["gate_new_over_parent_le_1"]


def memory(new, parent, parent_params, args):
    from kungfu_amd.collective import GradBuckets
    sizes = model_sizes()
    elements = sum(sizes)
    shard = sum(t.numel() * t.element_size() for G in new._kf_groups for t in G["m"] + G["v"])
    full = sum(t.numel() * t.element_size() for p in parent_params
               for k, t in parent.state[p].items() if k in ("exp_avg", "exp_avg_sq"))
    dev = parent_params[0].device
    gb8 = GradBuckets(sizes, torch.float32, dev, 8, bucket_bytes=new._kf_bucket_bytes)
    at8 = sum(2 * (b.numel() // 8) * b.element_size() for b in gb8.buckets)
    emit({"what": "optimizer-state bytes per rank (exp_avg + exp_avg_sq)", "model": "resnet50-imagenet",
          "dtype": "float32", "elements": elements,
          "world1_sharded_measured": shard, "world1_torch_measured": full,
          "world8_sharded_from_layout": at8, "world8_torch": full,
          "world8_sharded_over_torch": round(at8 / full, 4)}, args)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--what", default="kernel,step1", help="comma list of kernel, step1")
    ap.add_argument("--reps", type=int, default=100, help="timed kernel calls per kind")
    ap.add_argument("--steps", type=int, default=40, help="timed steps per optimizer, world 1")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--np", type=int, default=8, help="the update's /np (0: none)")
    ap.add_argument("--kernel-cases", default="full,shard",
                    help="comma list of full, shard (one at a time under a kernel trace)")
    ap.add_argument("--dtypes", default="float32", help="comma list of float32, bfloat16, float64")
    ap.add_argument("--out", default=None, help="append the JSON lines here")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_sharded_adam: needs a GPU (no CPU path)")
    what = args.what.split(",")
    ok = True
    if "kernel" in what:
        for name in args.dtypes.split(","):
            dtype = getattr(torch, name)
            if "full" in args.kernel_cases:
                kernel_case("resnet50, 16 buckets", 1, dtype, args)
            if "shard" in args.kernel_cases:
                kernel_case("resnet50, 16 shards of 1/8", 8, dtype, args)
    if "step1" in what:
        ok = step_world1(args)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
