#!/usr/bin/env python3
"""Measure the 8-bit block-wise Adam update (kf_adam8_update_batch,
kf_adam8_master_update_batch, ShardedAdamOptimizer(state_bits=8); DESIGN.md
§20) by tools/bench_sharded_adam_sr.py's method: every call between its own
pair of HIP events, 10 warm-up calls, then 100 calls rotating over copies of
the buffers that together exceed the L2 and the Infinity Cache; medians with
the 10th and 90th percentiles.

  kernel  In one loop, on the same element counts, call by call: the f32
          kernel (kf_adam_update_batch, 28 bytes per element), the master
          kernel (kf_adam_master_update_batch, bf16, 28 bytes) and their 8-bit
          twins (16.25 bytes). kf_adam.hip and kf_adam_master.hip are the
          parent commit's files, unchanged. Two layouts: ResNet-50's
          25,583,592 elements in 16 shards of 1/8, and one segment of 2^26
          elements (256 MiB of f32 parameters). Nothing here is a gate: the
          byte counts suggest 0.58 of the 32-bit kernel's time for a kernel
          that stays memory-bound.
  memory  State bytes per rank of ShardedAdamOptimizer on ResNet-50's and
          BERT's layouts at world 1 and 8, summed over the optimizer's own
          state tensors (rank 0's), for state_bits 32 and 8, f32 and bf16 with
          master weights.

One JSON object per line goes to --out (and stdout).
"""
import argparse
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [ROOT, HERE]

import torch  # noqa: E402

import bench_sharded_adam as b0  # noqa: E402  (pct, stats, time_calls, emit, the model, the hypers)

BIG = 1 << 26


def kernel_case(name, counts, args):
    from kungfu_amd import _lib, ops
    dev = torch.device("cuda:0")
    bf16, f32, u8 = torch.bfloat16, torch.float32, torch.uint8
    gen = torch.Generator(device=dev).manual_seed(1)
    n, nb = sum(counts), len(counts)

    def filled(dtype, square=False):
        out = []
        for c in counts:
            r = torch.randn(c, device=dev, generator=gen)
            out.append((r * r if square else r).to(dtype))  # exp_avg_sq is not negative
        return out

    def state8():
        """A previous state as the kernel leaves one: random moments quantized."""
        mc, ms, vc, vs = [], [], [], []
        for m, v in zip(filled(f32), filled(f32, True)):
            c, s = ops.adam8_quantize(m, 0)
            mc.append(c)
            ms.append(s)
            c, s = ops.adam8_quantize(v, 1)
            vc.append(c)
            vs.append(s)
        return mc, vc, ms, vs

    copies = max(2, -(-b0.ROTATE_BYTES // (6 * n)))
    lib = _lib.load()
    ha = _lib.adam_hyper_array([b0.ADAM] * nb)
    cnt = (ctypes.c_size_t * nb)(*counts)
    stream = torch.cuda.current_stream(dev).cuda_stream
    k32 = int(ops.kungfu_dtype(torch.empty(1, dtype=f32, device=dev)))
    k16 = int(ops.kungfu_dtype(torch.empty(1, dtype=bf16, device=dev)))
    keep = []

    def tables(bufs):
        keep.append(bufs)
        return [_lib.ptr_array([t.data_ptr() for t in ts]) for ts in bufs]

    def call(fn, what, *a):
        def run():
            _lib.check(fn(*a), what, source="")
        return run

    adam32, adam8, master32, master8 = [], [], [], []
    for _ in range(copies):
        adam32.append(call(lib.kf_adam_update_batch, "adam32",
                           *tables([filled(f32), filled(f32), filled(f32), filled(f32, True)]),
                           cnt, nb, k32, args.np, ha, stream))
        adam8.append(call(lib.kf_adam8_update_batch, "adam8",
                          *tables([filled(f32), filled(f32), *state8()]),
                          cnt, nb, k32, args.np, ha, stream))
        master32.append(call(lib.kf_adam_master_update_batch, "master32",
                             *tables([filled(bf16), filled(bf16), filled(f32), filled(f32),
                                      filled(f32, True)]), cnt, nb, k16, args.np, ha, stream))
        master8.append(call(lib.kf_adam8_master_update_batch, "master8",
                            *tables([filled(bf16), filled(bf16), filled(f32), *state8()]),
                            cnt, nb, k16, args.np, ha, stream))
    fns = {"adam32": adam32, "adam8": adam8, "master32": master32, "master8": master8}
    us = b0.time_calls(fns, args.reps, args.warmup)
    bytes_per = {"adam32": 28, "adam8": 16.25, "master32": 28, "master8": 16.25}
    row = {"what": "8-bit Adam kernels against the 32-bit-state kernels", "case": name,
           "elements": n, "segments": nb, "copies": copies, "np": args.np,
           "adam": "AdamW, weight_decay 1e-2, step 7"}
    for k in fns:
        row[k] = b0.stats(us[k])
        row[k]["bytes_per_element"] = bytes_per[k]
        gbs = bytes_per[k] * n / (row[k]["median_us"] * 1e-6)
        row[k]["GBps"] = round(gbs / 1e9, 1)
        row[k]["fraction_of_8TBps"] = round(gbs / b0.HBM_PEAK, 4)
    row["adam8"]["over_adam32"] = round(row["adam8"]["median_us"] / row["adam32"]["median_us"], 4)
    row["master8"]["over_master32"] = round(
        row["master8"]["median_us"] / row["master32"]["median_us"], 4)
    row["bytes_ratio"] = round(16.25 / 28, 4)
    b0.emit(row, args)


class _World:
    """An exchange of `world` ranks that is never stepped: rank 0's layout."""

    def __init__(self, world):
        self.world, self.rank = world, 0

    def adam_step_(self, *a):
        raise NotImplementedError

    adam_master_step_ = reduce_shards_ = grad_shards_ = gather_params_ = adam_step_


def memory(args):
    from kungfu_amd.optimizers import ShardedAdamOptimizer
    dev = torch.device("cuda:0")
    with open(os.path.join(ROOT, "tests", "golden", "models.json")) as f:
        models = json.load(f)
    for model in ("resnet50-imagenet", "bert"):
        sizes = models[model]
        for dtype, master in ((torch.float32, False), (torch.bfloat16, True)):
            row = {"what": "optimizer state bytes per rank, from the optimizer's tensors",
                   "model": model, "elements": sum(sizes), "dtype": str(dtype).split(".")[1],
                   "master_weights": master}
            for world in (1, 8):
                for bits in (32, 8):
                    ps = [torch.nn.Parameter(torch.zeros(n, dtype=dtype, device=dev))
                          for n in sizes]
                    opt = ShardedAdamOptimizer(torch.optim.AdamW(ps, lr=1e-3),
                                               exchange=_World(world), master_weights=master,
                                               state_bits=bits)
                    opt._kf_build_sharded()
                    total = 0
                    for G in opt._kf_groups:
                        opt._kf_states(G)
                        for key in ("m", "v", "ms", "vs", "w"):
                            total += sum(t.numel() * t.element_size() for t in G[key] or [])
                    row["world%d_bits%d" % (world, bits)] = total
                    row["world%d_bits%d_per_element" % (world, bits)] = round(
                        total * world / sum(sizes), 4)
                    del opt, ps
                    torch.cuda.empty_cache()
            b0.emit(row, args)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--what", default="kernel,memory", help="comma list of kernel, memory")
    ap.add_argument("--reps", type=int, default=100, help="timed kernel calls per kind")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--np", type=int, default=8, help="the update's /np (0: none)")
    ap.add_argument("--kernel-cases", default="shard,big", help="comma list of shard, big")
    ap.add_argument("--out", default=None, help="append the JSON lines here")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_sharded_adam8: needs a GPU (no CPU path)")
    what = args.what.split(",")
    if "kernel" in what:
        from kungfu_amd.collective import GradBuckets
        if "shard" in args.kernel_cases:
            layout = GradBuckets(b0.model_sizes(), torch.float32, torch.device("cuda:0"), 8,
                                 n_buckets=16)
            counts = [b.numel() // 8 for b in layout.buckets]
            del layout
            kernel_case("resnet50 f32 layout, 16 shards of 1/8", counts, args)
        if "big" in args.kernel_cases:
            kernel_case("one segment of 2^26 elements", [BIG], args)
    if "memory" in what:
        memory(args)


if __name__ == "__main__":
    main()
