#!/usr/bin/env python3
"""Time the pair-averaging model store (kf_pairavg_*) with two ranks on one GPU.

Rank 0 is timed; rank 1 publishes once and then waits on the host. For
ResNet-50's 214 fp32 tensors (tests/golden/models.json, laid out by
GradBuckets) and for one 256 MiB fp32 span:

  publish        kf_pairavg_publish (begin, copy, end)
  pull_average   kf_pairavg_pull_average from rank 1 (pick, fetch, check, blend)
  copy_reduce    what the same step costs with the pieces that existed before
                 the store: kf_copy_segments of rank 1's buckets (mapped over
                 HIP IPC) into a private buffer, then kf_bucket_reduce_avg
                 ([v, copy], np = 2) per bucket; no consistency check at all
  and pick, fetch, check and blend singly, which says where a pull's time goes.

Every timed call is bracketed by HIP events; the calls of one kind rotate over
copies of the model (each with its own store on both ranks) that together
exceed the L2 and the 256 MiB Infinity Cache, and the kinds alternate in one
loop. One JSON object per line goes to --out (and stdout); times are medians
in microseconds with the 10th and 90th percentiles as the spread.

Both ranks share one GPU, so the "remote" slot is local HBM: the numbers say
nothing about an xGMI link.
"""
import argparse
import ctypes
import json
import os
import socket
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.multiprocessing as mp  # noqa: E402

HBM_PEAK = 8.0e12  # bytes / s, the roofline the project quotes against
ROTATE_BYTES = 640 << 20  # more than L2 + Infinity Cache


def pct(xs, q):
    xs = sorted(xs)
    return xs[min(len(xs) - 1, int(q * len(xs)))]


def stats(us):
    return {"median_us": round(pct(us, 0.5), 3), "p10_us": round(pct(us, 0.1), 3),
            "p90_us": round(pct(us, 0.9), 3), "reps": len(us)}


def time_calls(fns, reps, warmup):
    """fns: dict name -> list of callables; round i calls fns[k][i % len] for
    every k in turn, each between its own pair of events."""
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


def case(name, sizes, rank, world, dev, args):
    import torch.distributed as dist
    from kungfu_amd import _lib, ops
    from kungfu_amd.collective import GradBuckets
    from kungfu_amd.p2p import share_ipc
    from kungfu_amd.pairavg import PeerModelStore
    lib = _lib.load()
    nbytes = 4 * sum(sizes)
    copies = max(2, -(-ROTATE_BYTES // nbytes))
    g = torch.Generator(device=dev).manual_seed(1 + rank)
    gbs, stores, spans = [], [], []
    for _ in range(copies):
        gb = GradBuckets(sizes, torch.float32, dev, 1)
        for v in gb.views:
            v.copy_(torch.randn(v.numel(), device=dev, generator=g))
        sp = [b[:n] for b, n in zip(gb.buckets, gb.spans)]
        gbs.append(gb)
        spans.append(sp)
        stores.append(PeerModelStore(sp))
    # the comparison's view of rank 1's buckets, and its private buffers
    bases = {}
    rows = [share_ipc(lib, None, world, rank, [b.data_ptr() for b in gb.buckets], bases)
            for gb in gbs]
    for st in stores:
        st.publish()
    torch.cuda.synchronize()
    dist.barrier()
    row = None
    if rank == 0:
        priv = [[torch.empty_like(b) for b in gb.buckets] for gb in gbs]
        s = torch.cuda.current_stream().cuda_stream

        def copy_reduce(c):
            # whole (padded) buckets: their lengths are multiples of 16 bytes
            sp, pv, rw = gbs[c].buckets, priv[c], rows[c]
            lens = (ctypes.c_size_t * len(sp))(*[b.numel() * 4 for b in sp])
            dsts = _lib.ptr_array([p.data_ptr() for p in pv])
            srcs = _lib.ptr_array([r[1] for r in rw])

            def run():
                _lib.check(lib.kf_copy_segments(dsts, srcs, lens, len(sp), s), "kf_copy_segments")
                for b, p in zip(sp, pv):
                    ops.bucket_reduce_avg([b, p], 2, out=b)
            return run

        fns = {
            "publish": [st.publish for st in stores],
            "pull_average": [(lambda st=st: st.pull_average_(1)) for st in stores],
            "copy_reduce": [copy_reduce(c) for c in range(copies)],
            "pick": [(lambda st=st: st._pick(1)) for st in stores],
            "fetch": [(lambda st=st: st._fetch(1)) for st in stores],
            "check": [(lambda st=st: st._check_(1)) for st in stores],
            "blend": [(lambda st=st: st._blend()) for st in stores],
        }
        us = time_calls(fns, args.reps, args.warmup)
        row = {"what": "pair averaging, 2 ranks on one GPU, timed on rank 0", "model": name,
               "dtype": "float32", "bytes": nbytes, "spans": len(spans[0]), "copies": copies,
               "note": "the remote slot is local HBM: nothing here measures an xGMI link"}
        for k, v in us.items():
            row[k] = stats(v)
        # bytes moved once in each direction by the two copies
        for k in ("publish", "fetch"):
            row[k]["copy_rate_fraction_of_8TBps"] = round(
                2 * nbytes / (row[k]["median_us"] * 1e-6) / HBM_PEAK, 4)
        row["pull_average_over_copy_reduce"] = round(
            row["pull_average"]["median_us"] / row["copy_reduce"]["median_us"], 4)
        c = stores[0].counters()
        row["counters_store0"] = c
        assert c["torn"] == 0 and c["empty"] == 0, c
    torch.cuda.synchronize()
    dist.barrier()
    for st in stores:
        st.close()
    for b in bases.values():
        lib.kf_ipc_close(b)
    return row


def body(rank, world, port, args):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    dev = torch.device("cuda:0")
    with open(os.path.join(ROOT, "tests", "golden", "models.json")) as f:
        models = json.load(f)
    for name, sizes in (("resnet50-imagenet", models["resnet50-imagenet"]),
                        ("one-256MiB-span", [(256 << 20) // 4])):
        row = case(name, sizes, rank, world, dev, args)
        if row is not None:
            row["device"] = torch.cuda.get_device_name(0)
            line = json.dumps(row)
            print(line, flush=True)
            if args.out:
                os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                with open(args.out, "a") as fo:
                    fo.write(line + "\n")
    dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None, help="append the JSON lines here")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_pairavg: needs a GPU (no CPU path)")
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    ps = [ctx.Process(target=body, args=(r, 2, port, args)) for r in range(2)]
    for p in ps:
        p.start()
    for p in ps:
        p.join()
    sys.exit(max(abs(p.exitcode or 0) for p in ps))


if __name__ == "__main__":
    main()
