#!/usr/bin/env python3
"""Time the segmented squared-norm kernels (kf_segnorm_*) on the GPU.

  (a) SQ over ONE 256 MiB segment, as time and as a fraction of 8 TB/s for
      the 256 MiB read; in fp32 (the case DESIGN.md quotes), and in fp64 and
      bf16 for the same bytes, which shows whether the widening to fp64 binds
      (fp64 needs none, bf16 twice fp32's per byte); fp32 also at other caps
      on a segment's blocks (KUNGFU_AMD_SEGNORM_MAX_BLOCKS, read at create).
  (b) SQ over ResNet-50's 214 and BERT's first 201 tensor sizes
      (tests/golden/models.json) laid out by GradBuckets, one segment per
      tensor, in f32 and bf16, beside torch._foreach_norm on the same views
      in the same loop (what a user would otherwise call), alternating.

Every timed call is bracketed by HIP events; inputs rotate over copies that
together exceed the L2 and the 256 MiB Infinity Cache, so no call finds its
input cached. One JSON object per line goes to --out (and stdout); times are
medians in microseconds with the 10th and 90th percentiles as the spread.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

HBM_PEAK = 8.0e12  # bytes / s, the roofline the project quotes against
ROTATE_BYTES = 640 << 20  # more than L2 + Infinity Cache


def pct(xs, q):
    xs = sorted(xs)
    return xs[min(len(xs) - 1, int(q * len(xs)))]


def stats(us):
    return {"median_us": round(pct(us, 0.5), 3), "p10_us": round(pct(us, 0.1), 3),
            "p90_us": round(pct(us, 0.9), 3), "reps": len(us)}


def time_calls(fns, reps, warmup):
    """fns: list of lists of callables; round i calls fns[k][i % len(fns[k])]
    for every k in turn (alternating), each between its own pair of events.
    Returns one list of microseconds per k."""
    for i in range(warmup):
        for f in fns:
            f[i % len(f)]()
    torch.cuda.synchronize()
    evs = [[] for _ in fns]
    for i in range(reps):
        for k, f in enumerate(fns):
            a = torch.cuda.Event(enable_timing=True)
            b = torch.cuda.Event(enable_timing=True)
            a.record()
            f[i % len(f)]()
            b.record()
            evs[k].append((a, b))
    torch.cuda.synchronize()
    return [[1e3 * a.elapsed_time(b) for a, b in e] for e in evs]


def one_segment(dtype, nbytes, cap, dev, args):
    from kungfu_amd import ops
    n = nbytes // torch.empty((), dtype=dtype).element_size()
    copies = max(2, -(-ROTATE_BYTES // nbytes))
    bufs = [torch.randn(n, device=dev, dtype=torch.float32).to(dtype) if dtype != torch.float32
            else torch.randn(n, device=dev) for _ in range(copies)]
    if cap:
        os.environ["KUNGFU_AMD_SEGNORM_MAX_BLOCKS"] = str(cap)
    else:
        os.environ.pop("KUNGFU_AMD_SEGNORM_MAX_BLOCKS", None)
    plans = [ops.SegNorm([b]) for b in bufs]
    os.environ.pop("KUNGFU_AMD_SEGNORM_MAX_BLOCKS", None)
    outs = [torch.empty(2, dtype=torch.float64, device=dev) for _ in plans]
    fns = [[(lambda p=p, o=o: p.run("sq", out=o)) for p, o in zip(plans, outs)]]
    us = time_calls(fns, args.reps, args.warmup)[0]
    ref = float(torch.linalg.vector_norm(bufs[0].double()) ** 2)
    got = float(outs[0][0])
    row = {"case": "a", "what": "SQ over one segment", "dtype": str(dtype).split(".")[1],
           "bytes": nbytes, "max_blocks": cap or "default", "copies": copies,
           "rel_diff_vs_torch_fp64": abs(got - ref) / ref}
    row.update(stats(us))
    row["fraction_of_8TBps"] = round(nbytes / (row["median_us"] * 1e-6) / HBM_PEAK, 4)
    for p in plans:
        p.close()
    return row


def model_case(name, sizes, dtype, dev, args):
    from kungfu_amd import ops
    from kungfu_amd.collective import GradBuckets
    itemsize = torch.empty((), dtype=dtype).element_size()
    nbytes = sum(sizes) * itemsize
    copies = max(2, -(-ROTATE_BYTES // nbytes))
    gbs = [GradBuckets(sizes, dtype, dev, 1) for _ in range(copies)]
    g = torch.Generator(device=dev).manual_seed(1)
    for gb in gbs:
        for v in gb.views:
            v.copy_(torch.randn(v.numel(), device=dev, generator=g).to(dtype))
    plans = [ops.SegNorm(gb.views) for gb in gbs]
    outs = [torch.empty(len(sizes) + 1, dtype=torch.float64, device=dev) for _ in plans]
    ours = [(lambda p=p, o=o: p.run("sq", out=o)) for p, o in zip(plans, outs)]
    theirs = [(lambda vs=gb.views: torch._foreach_norm(vs)) for gb in gbs]
    us, them = time_calls([ours, theirs], args.reps, args.warmup)
    ref = torch.stack([t.double() for t in torch._foreach_norm(gbs[0].views)]) ** 2
    rel = float(((outs[0][:-1] - ref).abs() / ref).max())
    row = {"case": "b", "what": "SQ, one segment per tensor, GradBuckets layout", "model": name,
           "tensors": len(sizes), "dtype": str(dtype).split(".")[1], "bytes": nbytes,
           "buckets": len(gbs[0].buckets), "copies": copies,
           "segnorm": stats(us), "torch_foreach_norm": stats(them),
           "max_rel_diff_vs_torch": rel}
    row["segnorm"]["fraction_of_8TBps"] = round(
        nbytes / (row["segnorm"]["median_us"] * 1e-6) / HBM_PEAK, 4)
    row["speedup_median"] = round(row["torch_foreach_norm"]["median_us"] /
                                  row["segnorm"]["median_us"], 3)
    for p in plans:
        p.close()
    return row


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None, help="append the JSON lines here")
    ap.add_argument("--caps", default="0,1024,4096,8192",
                    help="block caps for case (a) fp32; 0 = the library's default")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_segnorm: needs a GPU (no CPU path)")
    dev = torch.device("cuda:0")
    with open(os.path.join(ROOT, "tests", "golden", "models.json")) as f:
        models = json.load(f)
    rows = []

    def emit(row):
        row["device"] = torch.cuda.get_device_name(0)
        rows.append(row)
        line = json.dumps(row)
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as fo:
                fo.write(line + "\n")

    for cap in [int(c) for c in args.caps.split(",")]:
        emit(one_segment(torch.float32, 256 << 20, cap, dev, args))
    for dt in (torch.float64, torch.bfloat16):
        emit(one_segment(dt, 256 << 20, 0, dev, args))
    for name, sizes in (("resnet50-imagenet", models["resnet50-imagenet"]),
                        ("bert-201", models["bert"][:201])):
        for dt in (torch.float32, torch.bfloat16):
            emit(model_case(name, sizes, dt, dev, args))


if __name__ == "__main__":
    main()
