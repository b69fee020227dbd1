#!/usr/bin/env python3
"""Measure the sharded SGD step (ShardedSGDOptimizer, kf_sgd_update_batch).

Model: ResNet-50's 25,583,592 fp32 (tests/golden/models.json), momentum 0.9.

  kernel  (a) kf_sgd_update_batch over the model in 16 buckets
          (GradBuckets(n_buckets=16)) and over the shard form (1/8 of every
          bucket), as a fraction of the 8 TB/s HBM peak: 5 accesses per
          element (g, p, m read; p, m written). Beside it kf_sma_blend_batch
          on the same param and grad buffers in the same loop (3 accesses),
          the sibling whose rate is known. Calls rotate over copies of the
          buffers that together exceed the L2 and the 256 MiB Infinity Cache.
  step1   (b) step() at world 1, the two optimizers alternating in one loop
          over the same model, gradients and bucket layout:
            new     ShardedSGDOptimizer(SGD(momentum=0.9)).step()
            parent  SynchronousSGDOptimizer(SGD(momentum=0.9)).step()
          GATE: new / parent <= 1.0 on the median (exit status 1 otherwise).
  step8   (c) reported only: both at world 8 as threads over the loopback
          test transport (tests/loopback.py), with the native exchange's
          phase_times. That transport stages through the host: it says
          nothing about xGMI and nothing is gated on it.

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
HYPER = {"lr": 0.1, "momentum": 0.9, "dampening": 0.0, "weight_decay": 0.0, "nesterov": False,
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

def kernel_case(name, shard_of, args):
    from kungfu_amd import _lib, ops
    from kungfu_amd.collective import GradBuckets
    dev = torch.device("cuda:0")
    sizes = model_sizes()
    g = torch.Generator(device=dev).manual_seed(1)

    def segs(gb):
        out = []
        for b in gb.buckets:
            q = b.numel() // shard_of
            out.append(b[:q])
        return out

    world = shard_of
    probe = GradBuckets(sizes, torch.float32, dev, world, n_buckets=16)
    n = sum(s.numel() for s in segs(probe))
    copies = max(2, -(-ROTATE_BYTES // (3 * 4 * n)))
    del probe
    sets = []
    for _ in range(copies):
        bufs = []
        for _k in range(3):  # params, grads, momenta
            gb = GradBuckets(sizes, torch.float32, dev, world, n_buckets=16)
            for f in gb.flats:
                f.copy_(torch.randn(f.numel(), device=dev, generator=g))
            bufs.append(segs(gb))
        sets.append(bufs)
    # the C entry points themselves, on tables built once: the Python
    # wrappers' per-call list handling (tens of microseconds) is not the kernel
    lib = _lib.load()
    nb = len(sets[0][0])
    hs = _lib.sgd_hyper_array([HYPER] * nb)
    cnt = (ctypes.c_size_t * nb)(*[t.numel() for t in sets[0][0]])
    f32 = int(ops.kungfu_dtype(sets[0][0][0]))
    stream = torch.cuda.current_stream(dev).cuda_stream

    def tables(s):
        return [_lib.ptr_array([t.data_ptr() for t in ts]) for ts in s]

    def sgd(t):
        def run():
            _lib.check(lib.kf_sgd_update_batch(t[0], t[1], t[2], cnt, nb, f32, args.np, hs, stream),
                       "kf_sgd_update_batch", source="")
        return run

    def sma(t):
        def run():
            _lib.check(lib.kf_sma_blend_batch(t[0], t[1], cnt, nb, f32, max(1, args.np), 0.1, stream),
                       "kf_sma_blend_batch", source="")
        return run

    tabs = [tables(s) for s in sets]
    fns = {"sgd_update": [sgd(t) for t in tabs], "sma_blend": [sma(t) for t in tabs]}
    us = time_calls(fns, args.reps, args.warmup)
    row = {"what": "kernel rate", "case": name, "dtype": "float32", "elements": n,
           "segments": nb, "copies": copies, "np": args.np, "momentum": 0.9}
    for k, acc in (("sgd_update", 5), ("sma_blend", 3)):
        row[k] = stats(us[k])
        row[k]["accesses_per_element"] = acc
        row[k]["fraction_of_8TBps"] = round(acc * 4 * n / (row[k]["median_us"] * 1e-6) / HBM_PEAK, 4)
    row["sgd_minus_sma_fraction"] = round(row["sgd_update"]["fraction_of_8TBps"] -
                                          row["sma_blend"]["fraction_of_8TBps"], 4)
    emit(row, args)


# ---- (b), (c) the optimizers ---------------------------------------------------

def make_model(dev, seed=2):
    g = torch.Generator(device=dev).manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(n, device=dev, generator=g)) for n in model_sizes()]


def give_grads(ps, dev, seed=3):
    g = torch.Generator(device=dev).manual_seed(seed)
    for p in ps:
        p.grad = torch.randn(p.numel(), device=dev, generator=g)


def make_opts(dev, ex_new, ex_parent):
    from kungfu_amd.optimizers import ShardedSGDOptimizer, SynchronousSGDOptimizer
    pn, pp = make_model(dev), make_model(dev)
    new = ShardedSGDOptimizer(torch.optim.SGD(pn, lr=0.1, momentum=0.9), exchange=ex_new)
    parent = SynchronousSGDOptimizer(torch.optim.SGD(pp, lr=0.1, momentum=0.9), exchange=ex_parent)
    give_grads(pn, dev)
    give_grads(pp, dev)
    return pn, pp, new, parent


def step_world1(args):
    dev = torch.device("cuda:0")
    pn, pp, new, parent = make_opts(dev, None, None)
    walls = {"new": [], "parent": []}

    def timed(name, opt):
        def run():
            t0 = time.perf_counter()
            opt.step()
            walls[name].append(1e6 * (time.perf_counter() - t0))
        return run

    us = time_calls({"new": [timed("new", new)], "parent": [timed("parent", parent)]},
                    args.steps, args.warmup)
    # the same arithmetic up to torch's own rounding of a + alpha*b
    diff = max(float((a.detach() - b.detach()).abs().max()) for a, b in zip(pn, pp))
    row = {"what": "step time, world 1", "model": "resnet50-imagenet", "dtype": "float32",
           "elements": sum(model_sizes()), "momentum": 0.9,
           "new": stats(us["new"]), "parent": stats(us["parent"]),
           "new_host_enqueue_us": round(pct(walls["new"][args.warmup:], 0.5), 1),
           "parent_host_enqueue_us": round(pct(walls["parent"][args.warmup:], 0.5), 1),
           "max_abs_param_difference": diff}
    row["new_over_parent"] = round(row["new"]["median_us"] / row["parent"]["median_us"], 4)
    row["gate_new_over_parent_le_1"] = row["new_over_parent"] <= 1.0
    emit(row, args)
    return row["gate_new_over_parent_le_1"]


def step_world8(args):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import loopback
    world = 8
    dev = torch.device("cuda:0")
    out = {}

    def body(rank, ex):
        ex2 = group2.exchange(rank)
        pn, pp, new, parent = make_opts(dev, ex, ex2)
        for _ in range(args.warmup8):
            new.step()
            parent.step()
        torch.cuda.synchronize()
        ex.set_timing(True)
        ex2.set_timing(True)
        t = {"new": [], "parent": []}
        for _ in range(args.steps8):
            for name, opt in (("new", new), ("parent", parent)):
                t0 = time.perf_counter()
                opt.step()
                torch.cuda.synchronize()
                t[name].append(1e6 * (time.perf_counter() - t0))
        out[rank] = (t, ex.phase_times(), ex2.phase_times())
        ex2.close()

    group2 = loopback.LoopbackGroup(world)
    loopback.loop_ranks(world, body, timeout=1500)
    group2.close()
    t, ph_new, ph_parent = out[0]
    row = {"what": "step time, world 8 over the loopback test transport (host-staged: not xGMI), "
                   "rank 0, host clock around step() and a device synchronise; reported only",
           "model": "resnet50-imagenet", "dtype": "float32", "momentum": 0.9,
           "new": stats(t["new"]), "parent": stats(t["parent"]),
           "new_phase_times_us": ph_new, "parent_exchange_phase_times_us": ph_parent,
           "note": "the parent's phase times cover its gradient all-reduce only; its "
                   "torch.optim.SGD step runs outside the exchange"}
    emit(row, args)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--what", default="kernel,step1,step8",
                    help="comma list of kernel, step1, step8")
    ap.add_argument("--reps", type=int, default=100, help="timed kernel calls per kind")
    ap.add_argument("--steps", type=int, default=40, help="timed steps per optimizer, world 1")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--steps8", type=int, default=20)
    ap.add_argument("--warmup8", type=int, default=2)
    ap.add_argument("--np", type=int, default=8, help="the update's /np (0: none)")
    ap.add_argument("--kernel-cases", default="full,shard",
                    help="comma list of full, shard (one at a time under a kernel trace)")
    ap.add_argument("--out", default=None, help="append the JSON lines here")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_sharded_sgd: needs a GPU (no CPU path)")
    what = args.what.split(",")
    ok = True
    if "kernel" in what:
        if "full" in args.kernel_cases:
            kernel_case("resnet50, 16 buckets", 1, args)
        if "shard" in args.kernel_cases:
            kernel_case("resnet50, 16 shards of 1/8", 8, args)
    if "step1" in what:
        ok = step_world1(args)
    if "step8" in what:
        step_world8(args)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
