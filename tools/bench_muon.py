"""Time Muon's Newton-Schulz chain (ops.MuonPlan: the grouped MFMA GEMM) beside
the same chain written with torch.matmul in bf16 and beside the plan with
symmetric=True (the symmetric-product kernel for X X^T and b A + c A A), and
the whole world-1 step of ShardedMuonOptimizer, general and symmetric, beside
ShardedSGDOptimizer's.

  python tools/bench_muon.py [--window 0.5] [--repeats 5] [--only CASE]
                             [--out profiles/muon/bench.jsonl]

Every figure is the median of `repeats` windows (the smallest and the largest
are recorded beside it); a window is as many runs as fill `window` seconds,
sized from a first short window, between HIP events, after 3 warm-up runs,
four buffer sets used in turn. The sides of a case alternate window by
window. One JSON line per case. Needs a GPU."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from kungfu_amd import ops  # noqa: E402

A, B, C = ops.MUON_COEFFS


def resnet50_convs():
    """The 53 convolution weights of ResNet-50 as shapes. tests/golden/models.json
    holds the model's tensors as element counts only, so the shapes are He et
    al. 2015, table 1, and are held to the fixture: its counts above 2048 (the
    widest batch-norm vector) other than the classifier's 2048 x 1000 must be
    these shapes' products, in any order."""
    shapes, inp = [(64, 3, 7, 7)], 64
    for planes, blocks in ((64, 3), (128, 4), (256, 6), (512, 3)):
        for b in range(blocks):
            shapes += [(planes, inp, 1, 1), (planes, planes, 3, 3), (4 * planes, planes, 1, 1)]
            if b == 0:
                shapes.append((4 * planes, inp, 1, 1))
            inp = 4 * planes
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
    with open(os.path.join(root, "tests", "golden", "models.json")) as f:
        left = sorted(n for n in json.load(f)["resnet50-imagenet"] if n > 2048 and n != 2048000)
    if left != sorted(s[0] * s[1] * s[2] * s[3] for s in shapes):
        raise SystemExit("tests/golden/models.json and resnet50_convs() disagree")
    return shapes


def flops(shapes, steps):
    """The chain's multiply-adds times two: per step X X^T, A A and B X."""
    total = 0
    for s in shapes:
        r = s[0]
        c = 1
        for d in s[1:]:
            c *= d
        short, long_ = min(r, c), max(r, c)
        total += steps * (4 * short * short * long_ + 2 * short ** 3)
    return total


def torch_chain(ts, steps):
    out = []
    for t in ts:
        x = t.view(t.shape[0], -1)
        x = x / (x.float().norm() + 1e-7).to(torch.bfloat16)
        tall = x.shape[0] > x.shape[1]
        for _ in range(steps):
            a = x.T @ x if tall else x @ x.T
            b = B * a + C * (a @ a)
            x = A * x + (x @ b if tall else b @ x)
        out.append(x)
    return out


def _window(fns, iters):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for i in range(iters):
        fns[i % len(fns)]()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / iters


def timed(sides, window, repeats):
    """Per side (a list of callables used in turn) -> {ms, ms_min, ms_max,
    iters}: the median, the smallest and the largest of `repeats` windows of
    about `window` seconds each, the sides alternating."""
    iters = []
    for fns in sides:
        for i in range(3):
            fns[i % len(fns)]()
        torch.cuda.synchronize()
        iters.append(max(5, int(window * 1e3 / _window(fns, 5))))
    got = [[] for _ in sides]
    for _ in range(repeats):
        for k, fns in enumerate(sides):
            got[k].append(_window(fns, iters[k]))
    return [{"ms": sorted(g)[len(g) // 2], "ms_min": min(g), "ms_max": max(g), "iters": n}
            for g, n in zip(got, iters)]


def chain_case(name, shapes, window, repeats, steps=5):
    sets = [[torch.randn(s, device="cuda").to(torch.bfloat16) for s in shapes] for _ in range(4)]
    plans, sym = ([ops.MuonPlan([t.view(-1) for t in ts],
                                [(t.shape[0], t.numel() // t.shape[0]) for t in ts], symmetric)
                   for ts in sets] for symmetric in (False, True))
    ours, theirs, syrk = timed([[lambda p=p: p.run(steps) for p in plans],
                                [lambda ts=ts: torch_chain(ts, steps) for ts in sets],
                                [lambda p=p: p.run(steps) for p in sym]], window, repeats)
    same = all(torch.equal(x, y) for x, y in zip(plans[0].run(steps), sym[0].run(steps)))
    worst = max(float((x.float() - y.float()).abs().max())
                for x, y in zip(plans[0].run(steps), torch_chain(sets[0], steps)))
    f = flops(shapes, steps)
    return {"case": name, "tensors": len(shapes), "steps": steps, "grouped": ours,
            "torch_matmul": theirs, "torch_over_grouped": theirs["ms"] / ours["ms"],
            "symmetric": syrk, "symmetric_over_grouped": syrk["ms"] / ours["ms"],
            "symmetric_same_bytes": same,
            "grouped_tflops": f / ours["ms"] / 1e9, "torch_tflops": f / theirs["ms"] / 1e9,
            "max_abs_difference": worst}


def step_case(window, repeats):
    """The world-1 step on ResNet-50's convolutions: Muon beside sharded SGD."""
    from kungfu_amd.exchange import NativeExchange
    from kungfu_amd.optimizers import ShardedMuonOptimizer, ShardedSGDOptimizer
    opts, keep = [], []
    for make in (ShardedMuonOptimizer, ShardedSGDOptimizer,
                 lambda o, **kw: ShardedMuonOptimizer(o, symmetric=True, **kw)):
        ps = [torch.nn.Parameter(torch.randn(s, device="cuda") * 0.05) for s in resnet50_convs()]
        ex = NativeExchange()
        opts.append(make(torch.optim.SGD(ps, lr=0.02, momentum=0.95, nesterov=True), exchange=ex))
        for p in ps:
            p.grad = torch.randn_like(p)
        keep.append((ps, ex))
    muon, sgd, sym = timed([[o.step] for o in opts], window, repeats)
    for _, ex in keep:
        ex.close()
    return {"case": "step_world1_resnet50_convs", "muon": muon, "sgd": sgd, "muon_symmetric": sym}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--only", default=None, help="one case by name (for a kernel trace)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    cases = [("resnet50_convs", lambda: chain_case("resnet50_convs", resnet50_convs(),
                                                   args.window, args.repeats))]
    for r, c in ((1024, 1024), (1024, 4096), (4096, 4096)):
        name = "%dx%d" % (r, c)
        cases.append((name, lambda name=name, r=r, c=c: chain_case(name, [(r, c)], args.window,
                                                                  args.repeats)))
    cases.append(("step", lambda: step_case(args.window, args.repeats)))
    rows = []
    for name, run in cases:
        if args.only in (None, name):
            rows.append(run())
            print(json.dumps(rows[-1]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.writelines(json.dumps(row) + "\n" for row in rows)


if __name__ == "__main__":
    main()
