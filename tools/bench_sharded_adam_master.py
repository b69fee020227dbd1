#!/usr/bin/env python3
"""Measure the master-weights Adam update (kf_adam_master_update_batch,
ShardedAdamOptimizer(master_weights=True)) by tools/bench_sharded_adam.py's
method: ResNet-50's 25,583,592 elements in 16 buckets and in 16 shards of 1/8,
AdamW with weight_decay 1e-2, np = 8, every call between its own pair of HIP
events, 10 warm-up calls, then 100 calls rotating over copies of the buffers
that together exceed the L2 and the Infinity Cache; medians with the 10th and
90th percentiles.

  kernel  In one loop, on the same element count: kf_adam_update_batch on f32
          buffers (the yardstick: 7 x 4 bytes per element) and
          kf_adam_master_update_batch on bf16 and on f16 parameters and
          gradients with fp32 master, exp_avg and exp_avg_sq (2 + 12 read,
          12 + 2 written: 28 bytes as well). GOAL, recorded and not a gate:
          the new kernel's median is at most the f32 kernel's median plus the
          f32 kernel's own p90 - p10 width in that run.
          --variants name=path[,name=path...] times the same entry point of
          other builds of the library beside them (another lane mapping or
          tile depth: `make -C kungfu_amd/csrc EXTRA="-DKF_ADAM_MASTER_ELTS=8"
          OUT=<path> OBJDIR=<dir>`).
  step1   For information: step() at world 1 on a bf16 model, the optimizer
          with master weights and without alternating in one loop; and the
          optimizer-state bytes per rank of both.

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

DT16 = {"bfloat16": torch.bfloat16, "float16": torch.float16}


def load_variant(path):
    """Another build of the library: only kf_adam_master_update_batch is called."""
    from kungfu_amd import _lib
    main = _lib.load()
    lib = ctypes.CDLL(os.path.abspath(path))
    lib.kf_adam_master_update_batch.argtypes = main.kf_adam_master_update_batch.argtypes
    lib.kf_adam_master_update_batch.restype = ctypes.c_int
    return lib


def kernel_case(name, shard_of, args, variants):
    from kungfu_amd import _lib, ops
    from kungfu_amd.collective import GradBuckets
    dev = torch.device("cuda:0")
    sizes = b0.model_sizes()
    gen = torch.Generator(device=dev).manual_seed(1)
    world = shard_of

    def segs(gb):
        return [b[:b.numel() // shard_of] for b in gb.buckets]

    def filled(dtype, square=False):
        gb = GradBuckets(sizes, dtype, dev, world, n_buckets=16)
        for f in gb.flats:
            r = torch.randn(f.numel(), device=dev, generator=gen)
            f.copy_(r * r if square else r)  # exp_avg_sq is not negative
        return segs(gb)

    probe = segs(GradBuckets(sizes, torch.float32, dev, world, n_buckets=16))
    n, nb = sum(s.numel() for s in probe), len(probe)
    counts = [s.numel() for s in probe]
    del probe
    copies = max(2, -(-b0.ROTATE_BYTES // (16 * n)))  # 16 bytes of buffers per element, either kind
    f32 = torch.float32
    lib = _lib.load()
    ha = _lib.adam_hyper_array([b0.ADAM] * nb)
    cnt = (ctypes.c_size_t * nb)(*counts)
    stream = torch.cuda.current_stream(dev).cuda_stream
    keep = []  # the tensors behind the pointer tables
    kdt32 = int(ops.kungfu_dtype(torch.empty(1, dtype=f32, device=dev)))

    def tables(bufs):
        keep.append(bufs)
        return [_lib.ptr_array([t.data_ptr() for t in ts]) for ts in bufs]

    def f32_call(t):
        def run():
            _lib.check(lib.kf_adam_update_batch(t[0], t[1], t[2], t[3], cnt, nb, kdt32, args.np, ha,
                                                stream), "kf_adam_update_batch", source="")
        return run

    def master_call(which, t, kdt):
        def run():
            rc = which.kf_adam_master_update_batch(t[0], t[1], t[2], t[3], t[4], cnt, nb, kdt, args.np,
                                                   ha, stream)
            if rc != 0:
                raise RuntimeError("kf_adam_master_update_batch: status %d" % rc)
        return run

    fns = {"f32": [f32_call(tables([filled(f32), filled(f32), filled(f32), filled(f32, True)]))
                   for _ in range(copies)]}
    kinds = {"f32": None}
    for dname in args.dtypes.split(","):
        d16 = DT16[dname]
        sets = [tables([filled(d16), filled(d16), filled(f32), filled(f32), filled(f32, True)])
                for _ in range(copies)]
        kdt = int(ops.kungfu_dtype(torch.empty(1, dtype=d16, device=dev)))
        for j, (vname, vlib) in enumerate([("", lib)] + variants):
            key = dname + (":" + vname if vname else "")
            # consecutive builds start on different copies: none finds the
            # previous one's buffers in the Infinity Cache
            fns[key] = [master_call(vlib, t, kdt) for t in sets[j % copies:] + sets[:j % copies]]
            kinds[key] = (dname, vname or "built library")
    us = b0.time_calls(fns, args.reps, args.warmup)
    row = {"what": "master-weights kernel against the f32 kernel", "case": name, "elements": n,
           "segments": nb, "copies": copies, "np": args.np, "bytes_per_element": 28,
           "adam": "AdamW, weight_decay 1e-2, step 7"}
    for k in fns:
        row[k] = b0.stats(us[k])
        row[k]["fraction_of_8TBps"] = round(28 * n / (row[k]["median_us"] * 1e-6) / b0.HBM_PEAK, 4)
    y = row["f32"]
    goal = y["median_us"] + (y["p90_us"] - y["p10_us"])
    row["goal_us"] = round(goal, 3)
    for k, kind in kinds.items():
        if kind is not None:
            row[k]["dtype"], row[k]["build"] = kind
            row[k]["over_f32"] = round(row[k]["median_us"] / y["median_us"], 4)
            row[k]["goal_met"] = row[k]["median_us"] <= goal
    b0.emit(row, args)


def make_model(dev, dtype, seed=2):
    g = torch.Generator(device=dev).manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(n, device=dev, generator=g).to(dtype))
            for n in b0.model_sizes()]


def give_grads(ps, dev, seed=3):
    g = torch.Generator(device=dev).manual_seed(seed)
    for p in ps:
        p.grad = torch.randn(p.numel(), device=dev, generator=g).to(p.dtype)


def step_world1(args):
    from kungfu_amd.optimizers import ShardedAdamOptimizer
    dev = torch.device("cuda:0")
    for dname in args.dtypes.split(","):
        if dname == "float16":
            continue  # without master weights f16 is refused: nothing to alternate with
        dtype = DT16[dname]
        pm, pp = make_model(dev, dtype), make_model(dev, dtype)
        new = ShardedAdamOptimizer(torch.optim.AdamW(pm, lr=1e-3, weight_decay=1e-2),
                                   master_weights=True)
        plain = ShardedAdamOptimizer(torch.optim.AdamW(pp, lr=1e-3, weight_decay=1e-2))
        give_grads(pm, dev)
        give_grads(pp, dev)
        us = b0.time_calls({"master": [new.step], "plain": [plain.step]}, args.steps, args.warmup)
        moved = [sum(int((p.detach() != q).sum()) for p, q in zip(ps, make_model(dev, dtype)))
                 for ps in (pm, pp)]

        def state_bytes(opt):
            return sum(t.numel() * t.element_size() for G in opt._kf_groups
                       for k in ("w", "m", "v") for t in (G[k] or []))

        row = {"what": "step time, world 1 (for information)", "model": "resnet50-imagenet",
               "dtype": dname, "elements": sum(b0.model_sizes()),
               "optimizer": "AdamW, lr 1e-3, weight_decay 1e-2",
               "master_weights": b0.stats(us["master"]), "without": b0.stats(us["plain"]),
               "steps_taken": args.warmup + args.steps,
               "parameters_changed_master_weights": moved[0], "parameters_changed_without": moved[1],
               "state_bytes_master_weights": state_bytes(new), "state_bytes_without": state_bytes(plain)}
        row["master_over_without"] = round(row["master_weights"]["median_us"] /
                                           row["without"]["median_us"], 4)
        b0.emit(row, args)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--what", default="kernel,step1", help="comma list of kernel, step1")
    ap.add_argument("--reps", type=int, default=100, help="timed kernel calls per kind")
    ap.add_argument("--steps", type=int, default=40, help="timed steps per optimizer, world 1")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--np", type=int, default=8, help="the update's /np (0: none)")
    ap.add_argument("--kernel-cases", default="full,shard", help="comma list of full, shard")
    ap.add_argument("--dtypes", default="bfloat16,float16", help="comma list of bfloat16, float16")
    ap.add_argument("--variants", default="", help="name=path,... other builds of the library")
    ap.add_argument("--out", default=None, help="append the JSON lines here")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_sharded_adam_master: needs a GPU (no CPU path)")
    variants = [(v.split("=", 1)[0], load_variant(v.split("=", 1)[1]))
                for v in args.variants.split(",") if v]
    what = args.what.split(",")
    if "kernel" in what:
        if "full" in args.kernel_cases:
            kernel_case("resnet50, 16 buckets", 1, args, variants)
        if "shard" in args.kernel_cases:
            kernel_case("resnet50, 16 shards of 1/8", 8, args, variants)
    if "step1" in what:
        step_world1(args)


if __name__ == "__main__":
    main()
