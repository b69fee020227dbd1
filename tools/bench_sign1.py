#!/usr/bin/env python3
"""Time the 1-bit gradient wire's two kernels against their MXFP8 counterparts
(kf_sign1_pack_ef_batch and kf_mx8_pack_ef_batch, kf_sign1_fold_batch and
kf_mx8_fold_batch) by tools/bench_mx8_packs.py's method: one
process, every call between its own pair of HIP events, 10 warm-up calls, then
100 rounds that call the four kernels in turn on the same rotating copies of
the buffers, which together exceed the L2 and the Infinity Cache; medians with
the 10th and 90th percentiles. World 8; the layouts are bench_mx8.py's: one
segment of 2^26 elements, and ResNet-50's 16 buckets.

GB/s are against algorithmic bytes: the packs per bucket element, sz + 8 +
1.03125 (MXFP8) and sz + 8 + 0.1875 (1-bit); the folds per shard element,
8 x 1.03125 + sz and 8 x 0.1875 + sz. Every row says how far the 1-bit
kernel's median lies from its counterpart's, beside that one's p10-p90 spread.
One JSON object per line goes to --out (and stdout).
"""
import argparse
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [ROOT, HERE]

import torch  # noqa: E402

import bench_mx8  # noqa: E402  (the layouts)
import bench_sharded_adam as b0  # noqa: E402  (stats, time_calls, emit)

WORLD = bench_mx8.WORLD
WIRE = {"mx8": 1.03125, "sign1": 0.1875}  # bytes per element on the wire


def case_row(case, dname, args):
    from kungfu_amd import ops
    dev = torch.device("cuda:0")
    dt, sz = bench_mx8.DT[dname], bench_mx8.DT[dname].itemsize
    buckets, shards = bench_mx8.layouts(case, dev)
    nb_, ns = sum(buckets), sum(shards)
    gen = torch.Generator(device=dev).manual_seed(1)
    rand = lambda n: torch.randn(n, device=dev, generator=gen).to(dt)  # noqa: E731
    copies = max(2, -(-b0.ROTATE_BYTES // int(nb_ * (sz + 8 + 1.03125))))
    packs = {"mx8": ops.mx8_pack_ef_batch_, "sign1": ops.sign1_pack_ef_batch_}
    folds = {"mx8": ops.mx8_fold_batch_, "sign1": ops.sign1_fold_batch_}
    fns, keep = {w + k: [] for w in WIRE for k in ("_pack", "_fold")}, []
    for _ in range(copies):
        grads = [rand(n) for n in buckets]
        res = [torch.zeros(n, dtype=torch.float32, device=dev) for n in buckets]
        outs = [torch.empty(q, dtype=dt, device=dev) for q in shards]
        for w in WIRE:
            packed = packs[w](grads, res, WORLD)
            # the pieces a rank receives for its shards: any packed data of the right size
            recvd = packs[w]([rand(q * WORLD) for q in shards],
                             [torch.zeros(q * WORLD, dtype=torch.float32, device=dev) for q in shards], WORLD)
            keep.append((grads, res, outs, packed, recvd))
            fns[w + "_pack"].append(lambda w=w, g=grads, r=res, p=packed: packs[w](g, r, WORLD, p))
            fns[w + "_fold"].append(lambda w=w, r=recvd, o=outs: folds[w](r, o, WORLD, WORLD))
    us = b0.time_calls(fns, args.reps, args.warmup)
    row = {"what": "1-bit wire against the MXFP8 wire: EF pack and fold, same buffers, same loop",
           "case": case, "dtype": dname, "world": WORLD, "bucket_elements": nb_,
           "shard_elements": ns, "copies": copies}
    for w, wire in WIRE.items():
        for k, per, n in (("_pack", sz + 8 + wire, nb_), ("_fold", WORLD * wire + sz, ns)):
            row[w + k] = b0.stats(us[w + k])
            row[w + k]["bytes_per_element"] = per
            row[w + k]["GBps"] = round(per * n / (row[w + k]["median_us"] * 1e-6) / 1e9, 1)
    for k in ("_pack", "_fold"):
        base = row["mx8" + k]
        row["sign1" + k]["over_mx8"] = round(row["sign1" + k]["median_us"] / base["median_us"], 4)
        row["mx8" + k]["spread_us"] = round(base["p90_us"] - base["p10_us"], 3)
    b0.emit(row, args)


def phase1_row(args):
    """reduce_shards_ of ResNet-50's 16 f32 buckets at world 2 under each wire:
    the exchange's own phase-1 time (pack and collectives) and phase-2 time
    (folds) per call. The two ranks are threads on ONE GPU over the tests'
    loopback transport: not an xGMI or network number."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import loopback
    from kungfu_amd.collective import GradBuckets
    wires = {"none": (None, {}), "mx8": ("mx8", {}), "mx8_ef": ("mx8", {"error_feedback": True}),
             "sign1": ("sign1", {"error_feedback": True})}
    got = {}

    def body(r, ex):
        dev = torch.device("cuda:0")
        lay = GradBuckets(b0.model_sizes(), torch.float32, dev, 2, n_buckets=16)
        src = [torch.randn(b.numel(), device=dev) for b in lay.buckets]
        for name, (wire, kw) in wires.items():
            ex.set_grad_wire(wire, **kw)
            for i in range(args.warmup + args.reps):
                if i == args.warmup:
                    torch.cuda.synchronize()
                    ex.set_timing(True)
                torch._foreach_copy_(lay.buckets, src)
                ex.reduce_shards_(lay.buckets)
            torch.cuda.synchronize()
            t = ex.phase_times()
            ex.set_timing(False)
            got[(r, name)] = {"phase1_us": round(t["reduce_scatter"] / t["calls"], 2),
                              "phase2_us": round(t["epilogue"] / t["calls"], 2), "calls": t["calls"]}

    loopback.loop_ranks(2, body)
    row = {"what": "phase 1 of reduce_shards_ at world 2 under each wire; two ranks as threads on "
                   "one GPU over the loopback test transport, not xGMI or a network",
           "bucket_elements": sum(b0.model_sizes()), "dtype": "float32"}
    row.update({name: got[(0, name)] for name in wires})
    b0.emit(row, args)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--phase1", action="store_true", help="the world-2 phase-1 row instead")
    ap.add_argument("--reps", type=int, default=100, help="timed rounds")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--cases", default="one,shard", help="comma list of one, shard")
    ap.add_argument("--dtypes", default="float32,bfloat16")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sign1_wire", "bench.jsonl"),
                    help="append the JSON lines here")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_sign1: needs a GPU (no CPU path)")
    if args.phase1:
        return phase1_row(args)
    for case in args.cases.split(","):
        for dname in args.dtypes.split(","):
            case_row(case, dname, args)


if __name__ == "__main__":
    main()
