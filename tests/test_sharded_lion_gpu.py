"""Lion on the GPU, bit for bit against tests/lion_ref.py: the three kernels on
whole guarded buffers, the apply kernel over a bucket's pieces, and
ShardedLionOptimizer end to end, dense and over the sign wire."""
import functools

import numpy as np
import pytest
import torch

import adam8_cpu
import capture
import lion_ref
import loopback
import test_sharded_lars as lars_cpu
from adam8_cpu import to_numpy, to_torch

pytestmark = pytest.mark.gpu

TILE = 4096  # elements of a tile of all three kernels, both dtypes (kf_lion.hip kLionTile)
COUNTS = [32, 64, TILE - 32, TILE, TILE + 32, 2 * TILE + 37 * 32, 0]
SPECIAL_AT = (0, 15, 16, 1008, 1023)  # a lane's edges, and the first wave's last lane
_TORCH = {"f32": torch.float32, "bf16": torch.bfloat16}


def _segments(dt, seed):
    """Per segment (p, g, m) with c = +0 (under a -0 parameter), c = -0 and c = NaN at
    SPECIAL_AT, and the segment's hyper: weight decay on every other one."""
    rng, segs, hs = np.random.default_rng(seed), [], []
    for b, n in enumerate(COUNTS):
        p, g, m = (adam8_cpu.narrow(rng.standard_normal(n).astype(np.float32), dt) for _ in range(3))
        for k, at in enumerate(a for a in SPECIAL_AT if a < n):
            g[at], m[at] = adam8_cpu.narrow(np.float32([(0.0, 0.0), (-0.0, -0.0), (np.nan, 1.0)][k % 3]), dt)
            p[at] = adam8_cpu.narrow(np.float32([-0.0]), dt)[0] if k % 3 == 0 else p[at]
        segs.append((p, g, m))
        hs.append(lion_ref.hyper(1e-3 * (b + 1), (0.9, 0.99), 0.1 * (b % 2)))
    return segs, hs


@pytest.mark.parametrize("np_", [0, 2, 3])
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_three_kernels(dt, np_):
    from kungfu_amd import ops
    segs, hs = _segments(dt, 7 + np_)
    bases, streams, key = [8192 * b for b in range(len(COUNTS))], [77 + b for b in range(len(COUNTS))], 0xC0FFEE
    sr = (bases, streams, key)
    want = [lion_ref.update(p, g, m, dt, h, np_, bs, st, key)
            for (p, g, m), h, bs, st in zip(segs, hs, bases, streams)]
    codes = [lion_ref.signs(g, m, dt, h, np_)[1] for (p, g, m), h in zip(segs, hs)]
    bufs = capture.Guarded()
    t = _TORCH[dt]
    p1, p2 = (bufs.add_all([s[0] for s in segs], t, "p") for _ in range(2))
    gs = bufs.add_all([s[1] for s in segs], t, "g")
    m1, m2 = (bufs.add_all([s[2] for s in segs], t, "m") for _ in range(2))
    cd = bufs.add_all([np.full(c.size, -1, np.int32) for c in codes], None, "codes")
    ops.lion_update_batch_(p1, gs, m1, hs, np_, sr)
    ops.lion_signs_batch_(gs, m2, cd, hs, np_)
    ops.lion_apply_signs_batch_(p2, cd, hs, sr)
    bufs.check_sentinels()
    raw = np.uint16 if dt == "bf16" else np.float32
    for b, ((p, g, m), (wp, wm)) in enumerate(zip(segs, want)):
        assert capture.host(gs[b], raw).tobytes() == g.tobytes(), b      # the gradients untouched
        assert capture.host(cd[b], np.uint32).tolist() == codes[b].tolist(), b  # the padding zero
        for got, w in ((p1[b], wp), (p2[b], wp), (m1[b], wm), (m2[b], wm)):
            assert capture.host(got, raw).tobytes() == w.tobytes(), (b, COUNTS[b])
    k = np.concatenate([lion_ref.codes_of(c, n) for c, n in zip(codes, COUNTS)])
    assert all((k == code).any() for code in range(4))


@pytest.mark.parametrize("world", [1, 2, 3])
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_apply_over_pieces(dt, world):
    """A bucket's pieces in one call, and piece by piece in calls of their own,
    against the restatement on the whole bucket: the draws know no geometry."""
    from kungfu_amd import ops
    q, rng = TILE + 32, np.random.default_rng(world)
    h, stream, key = lion_ref.hyper(2e-3, weight_decay=0.05), 9, 3
    p = adam8_cpu.narrow(rng.standard_normal(world * q).astype(np.float32), dt)
    whole = rng.integers(0, 4, world * q).astype(np.uint32)
    words = np.zeros(world * q // 16, np.uint32)
    np.bitwise_or.at(words, np.arange(world * q) // 16, whole << (2 * (np.arange(world * q) % 16)).astype(np.uint32))
    want = lion_ref.apply(p, words, dt, h, 0, stream, key)
    pad = np.zeros(lion_ref.sign_bytes(q) // 4 - q // 16, np.uint32)
    bufs = capture.Guarded()
    once, each = (bufs.add(p, _TORCH[dt], "p") for _ in range(2))
    cd = bufs.add_all([np.concatenate([words[j * q // 16:(j + 1) * q // 16], pad]).view(np.int32)
                       for j in range(world)], None, "codes")
    cut = lambda t: [t[j * q:(j + 1) * q] for j in range(world)]  # noqa: E731
    bases = [j * q for j in range(world)]
    ops.lion_apply_signs_batch_(cut(once), cd, [h] * world, (bases, [stream] * world, key))
    for j in range(world):
        ops.lion_apply_signs_batch_(cut(each)[j:j + 1], cd[j:j + 1], [h], (bases[j:j + 1], [stream], key))
    bufs.check_sentinels()
    raw = np.uint16 if dt == "bf16" else np.float32
    assert capture.host(once, raw).tobytes() == want.tobytes()
    assert capture.host(each, raw).tobytes() == want.tobytes()


# ---- the optimizer end to end ---------------------------------------------------
GROUPS = ({"lr": 2e-3, "betas": (0.9, 0.99), "weight_decay": 0.1},
          {"lr": 1e-3, "betas": (0.95, 0.98), "weight_decay": 0.0})
STEPS = (0, 1, 2)
SEED = 12345


def _make(ex, kind, sign_wire):
    from kungfu_amd.optimizers import ShardedLionOptimizer
    ps = [torch.nn.Parameter(to_torch(a, kind).cuda()) for a in lars_cpu.model_arrays(kind)]
    k = len(ps) // 2
    groups = [dict(GROUPS[0], params=ps[:k]), dict(GROUPS[1], params=ps[k:])]
    opt = ShardedLionOptimizer(torch.optim.AdamW(groups, lr=1e-3), exchange=ex, sr_seed=SEED,
                               bucket_bytes=lars_cpu.BUCKET_ELTS * ps[0].element_size(),
                               sign_wire=sign_wire)
    return ps, opt


def _feed(ps, opt, kind, world, rank, s):
    for g, h in zip(opt.param_groups, GROUPS):
        g["lr"] = h["lr"] * 0.5 ** s
    for p, g in zip(ps, lars_cpu.grad_arrays(world, s)[rank]):
        p.grad = to_torch(adam8_cpu.narrow(g, kind), kind).cuda()


def _run(ex, kind, world, rank, sign_wire, graph=False):
    """-> per bucket group (parameter buckets, this rank's momentum shards), as numpy."""
    ps, opt = _make(ex, kind, sign_wire)
    replayed = held = None
    for i, s in enumerate(STEPS + STEPS[-1:] if graph else STEPS):
        if replayed is None:
            _feed(ps, opt, kind, world, rank, s)
        if graph and i == len(STEPS) - 1:
            held = [p.grad for p in ps]  # alive: the captured copies into the buckets read these
            replayed = capture.capture(lambda stream: opt.step())
        replayed.replay() if replayed is not None else opt.step()
    torch.cuda.synchronize()
    del held
    return [([to_numpy(b) for b in G["pb"].buckets], [to_numpy(m) for m in G["moms"]])
            for G in opt._kf_groups]


@functools.lru_cache(maxsize=None)
def _numpy_run(kind, world, steps, key_steps):
    """The same steps by lion_ref on whole buckets (a CPU twin of the layout):
    -> per group (parameter buckets, whole momentum buckets)."""
    from kungfu_amd.collective import GradBuckets
    from kungfu_amd.optimizers import splitmix64, sr_stream_word
    arrays = lars_cpu.model_arrays(kind)
    k, out = len(arrays) // 2, []
    for j, hyp in enumerate(GROUPS):
        mine = arrays[j * k:(j + 1) * k]
        lay = GradBuckets([a.size for a in mine], _TORCH[kind], "cpu", world,
                          bucket_bytes=lars_cpu.BUCKET_ELTS * mine[0].itemsize)

        def buckets(tensors):
            for v, a in zip(lay.views, tensors):
                v.copy_(to_torch(a, kind))
            return [to_numpy(b) for b in lay.buckets]

        pb = buckets(mine)
        mb = [np.zeros_like(b) for b in pb]
        for s, ks in zip(steps, key_steps):
            per_rank = [buckets([adam8_cpu.narrow(g, kind) for g in lars_cpu.grad_arrays(world, s)[r][j * k:(j + 1) * k]])
                        for r in range(world)]
            h = dict(hyp, lr=hyp["lr"] * 0.5 ** s)
            key = splitmix64(splitmix64(SEED) ^ ks) & 0xffffffff
            for i in range(len(pb)):
                # the ranks' sum in f32, in rank order, then / world: one rounding to bf16
                total = sum((adam8_cpu.widen(g[i], kind) for g in per_rank[1:]),
                            adam8_cpu.widen(per_rank[0][i], kind))
                avg = adam8_cpu.narrow(total / np.float32(world), kind)
                pb[i], mb[i] = lion_ref.update(pb[i], avg, mb[i], kind, h, 0, 0,
                                               sr_stream_word(SEED, j, i), key)
        out.append((pb, mb))
    return out


@functools.lru_cache(maxsize=None)
def _device_run(kind, how, sign_wire):
    from kungfu_amd.exchange import NativeExchange
    got = {}
    if how == "loopback2":
        loopback.loop_ranks(2, lambda r, ex: got.update({r: _run(ex, kind, 2, r, sign_wire)}))
    else:
        ex = NativeExchange()
        if how == "mx8":
            ex.set_grad_wire("mx8")
        got[0] = _run(ex, kind, 1, 0, sign_wire, graph=how == "graph")
        ex.close()
    return got


def _assert_matches(got, want, world):
    for r in got:
        for (pb, ms), (wp, wm) in zip(got[r], want):
            for i in range(len(wp)):
                q = wp[i].size // world
                assert pb[i].tobytes() == wp[i].tobytes(), ("params", r, i)
                assert ms[i].tobytes() == wm[i][r * q:(r + 1) * q].tobytes(), ("momentum", r, i)


@pytest.mark.parametrize("how", ["builtin1", "loopback2"])
@pytest.mark.parametrize("sign_wire", [False, True])
@pytest.mark.parametrize("kind", ["f32", "bf16"])
def test_optimizer_end_to_end(kind, sign_wire, how):
    world = 2 if how == "loopback2" else 1
    got = _device_run(kind, how, sign_wire)
    _assert_matches(got, _numpy_run(kind, world, STEPS, (1, 2, 3)), world)  # every rank, so alike
    other = _device_run(kind, how, not sign_wire)
    for r in got:  # the sign wire changes no bit of the parameters or the momentum
        for (pa, ma), (pb, mb) in zip(got[r], other[r]):
            assert capture.same_bytes(pa, pb) and capture.same_bytes(ma, mb)


def test_graph_replay_sign_wire():
    """The built-in world-1 exchange, sign wire on, bf16: the last step captured
    and replayed twice. The key is a host argument: both replays draw with the
    captured step's."""
    got = _device_run("bf16", "graph", True)
    n = len(STEPS)
    _assert_matches(got, _numpy_run("bf16", 1, STEPS + STEPS[-1:], tuple(range(1, n)) + (n, n)), 1)


@pytest.mark.parametrize("kind", ["f32", "bf16"])
def test_sign_wire_under_mx8_grad_wire(kind):
    """set_grad_wire("mx8") in front (a lossy phase 1, so no restatement here):
    the sign wire still changes no bit, and the step moved the parameters."""
    (on,), (off,) = _device_run(kind, "mx8", True).values(), _device_run(kind, "mx8", False).values()
    start = lars_cpu.model_arrays(kind)[0]
    for (pa, ma), (pb, mb) in zip(on, off):
        assert capture.same_bytes(pa, pb) and capture.same_bytes(ma, mb)
    assert on[0][0][0][:start.size].tobytes() != start.tobytes()
