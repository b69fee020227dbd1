"""The MXFP8 gradient wire on the GPU, bit for bit against tests/mx8_ref.py:
the pack and fold kernels (whole buffers, sentinel bytes behind them), the
exchange's reduce_shards_ under set_grad_wire("mx8"), one optimizer step."""
import numpy as np
import pytest
import torch

import loopback
import mx8_ref
from kungfu_amd import ops
from kungfu_amd.exchange import NativeExchange
from kungfu_amd.optimizers import ShardedAdamOptimizer, ShardedLARSOptimizer

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KINDS = ("f32", "bf16", "f16")
# shard lengths: one block, two, a tile less a block, a wave tile, one more block, two tiles
# and 37 blocks (the fold's lane pairs end mid-wave), an empty bucket
SHARDS = (32, 64, 480, 512, 544, 2 * 512 + 37 * 32, 0)
# block scales: the format's range, less what 16 ranks' f32 sum needs (f16: its own range)
EXPS = {"f32": (-140, 120), "bf16": (-140, 120), "f16": (-24, 14)}


def special_blocks():
    rng = np.random.default_rng(3)
    out = []
    for pos in (0, 7, 8, 24, 31):  # lane and quad edges, both signs
        for sign in (1.0, -1.0):
            b = rng.uniform(-1, 1, 32).astype(np.float32)
            b[pos] = sign * 3.0
            out.append(b)
    out.append(np.full(32, 1.5, np.float32))
    for big in (1.75, np.nextafter(np.float32(1.75), np.float32(2)),
                np.nextafter(np.float32(1.75), np.float32(0)), np.finfo(np.float32).max):
        b = rng.uniform(-1, 1, 32).astype(np.float32)
        b[11] = big
        out.append(b)
    ties = np.zeros(32, np.float32)  # X = 1: E4M3 ties and near-ties
    ties[:9] = [256, 17, 18.999, 19, 1.5 * 2.0 ** -9, -17, -19, -1.5 * 2.0 ** -9, 2.0 ** -10]
    out.append(ties)
    for bad in (np.nan, np.inf, -np.inf):
        b = rng.uniform(-1, 1, 32).astype(np.float32)
        b[13] = bad
        out.append(b)
    out.append(np.zeros(32, np.float32))
    zero = np.zeros(32, np.float32)
    zero[21] = -0.0
    out.append(zero)
    for hi in (2, 1 << 10, 1 << 23):  # subnormals only
        out.append(rng.integers(0, hi, 32).astype(np.uint32).view(np.float32) * np.float32(-1) ** np.arange(32))
    return np.concatenate(out)


SPECIAL = special_blocks()


def random_blocks(n, kind, seed, special=False):
    """n elements (whole blocks) of `kind` on the device, a scale per block."""
    rng = np.random.default_rng(seed)
    e = rng.integers(EXPS[kind][0], EXPS[kind][1] + 1, n // 32).repeat(32)
    x = np.ldexp(rng.standard_normal(n), e).astype(np.float32)
    if special and n >= SPECIAL.size:
        x[n - SPECIAL.size:] = SPECIAL
    return torch.from_numpy(x).to(mx8_ref.TORCH[kind]).to(DEV)


def same_bits(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, what
    if got.numel() == 0:
        return
    g, w = got.cpu().contiguous().view(torch.uint8), want.cpu().contiguous().view(torch.uint8)
    bad = (g != w).nonzero().flatten()
    assert bad.numel() == 0, "%s: %d bytes differ, first at %d: %s != %s" % (
        what, bad.numel(), bad[0], g[bad[:8]].tolist(), w[bad[:8]].tolist())


@pytest.mark.parametrize("world", (1, 2, 3))
@pytest.mark.parametrize("kind", KINDS)
def test_pack(kind, world):
    grads = [random_blocks(q * world, kind, 10 * world + b, special=True)
             for b, q in enumerate(SHARDS)]
    before = [g.clone() for g in grads]
    need = [world * mx8_ref.piece_bytes(q) for q in SHARDS]
    bufs = [torch.full((n + 64,), 0xA5, dtype=torch.uint8, device=DEV) for n in need]
    ops.mx8_pack_batch_(grads, world, [b[:n] for b, n in zip(bufs, need)])
    for b, (q, g) in enumerate(zip(SHARDS, grads)):
        x = mx8_ref.widen(g)
        want = [mx8_ref.pack(x[j * q:(j + 1) * q]) for j in range(world)] + [np.full(64, 0xA5, np.uint8)]
        same_bits(bufs[b], torch.from_numpy(np.concatenate(want)), "bucket %d (q = %d)" % (b, q))
        same_bits(g, before[b], "the gradients of bucket %d" % b)


@pytest.mark.parametrize("div", (False, True))
@pytest.mark.parametrize("world", (1, 2, 3, 4, 16))
@pytest.mark.parametrize("kind", KINDS)
def test_fold(kind, world, div):
    np_ = world if div else 0
    packed, outs, want = [], [], []
    for b, q in enumerate(SHARDS):
        pieces = []
        for r in range(world):
            x = mx8_ref.widen(random_blocks(q, "f32", 100 * b + r))
            if q:
                x[:32] = 60000.0 - r  # the ranks' sum leaves f16's range from world 2 on
            if q > 32 and r == world // 2:
                x[40] = np.nan        # a 0xFF-scale block in one rank only
            pieces.append(mx8_ref.pack(x))
        packed.append(torch.from_numpy(np.concatenate(pieces)).to(DEV))
        outs.append(torch.full((q + 8,), -7.0, dtype=mx8_ref.TORCH[kind], device=DEV))
        want.append(torch.cat([mx8_ref.fold(pieces, np_, kind) if q else outs[-1][:0].cpu(),
                               torch.full((8,), -7.0, dtype=mx8_ref.TORCH[kind])]))
    ops.mx8_fold_batch_(packed, [o[:q] for o, q in zip(outs, SHARDS)], world, np_)
    for b, q in enumerate(SHARDS):
        same_bits(outs[b], want[b], "shard %d (q = %d)" % (b, q))


COUNTS = (64, 544, 32)  # shard lengths of the exchange's three buckets; the second has a tail


@pytest.mark.parametrize("world", (1, 2))
@pytest.mark.parametrize("kind", ("f32", "bf16"))
def test_exchange_reduce_shards(kind, world):
    counts = [q * world + (b == 1) * (world - 1) for b, q in enumerate(COUNTS)]
    data = [[random_blocks((n + 31) // 32 * 32, kind, 7 * r + b)[:n].clone()
             for b, n in enumerate(counts)] for r in range(world)]
    host = [[mx8_ref.widen(t) for t in row] for row in data]

    def body(r, ex):
        mine = [t.clone() for t in data[r]]
        ex.algo = "a2a"
        tails = ex.all_reduce_([t.clone() for t in data[r]], average=True, coalesce=False)
        assert ex.set_grad_wire("mx8").reduce_shards_(mine) == 0
        shards = ex.grad_shards_(mine)
        for b, q in enumerate(COUNTS):
            pieces = [mx8_ref.pack(host[j][b][r * q:(r + 1) * q]) for j in range(world)]
            same_bits(shards[b], mx8_ref.fold(pieces, world, kind), "rank %d bucket %d" % (r, b))
            same_bits(mine[b][q * world:], tails[b][q * world:], "rank %d tail %d" % (r, b))

    if world == 1:
        ex = NativeExchange(device=DEV)
        body(0, ex)
        ex.close()
    else:
        loopback.loop_ranks(world, body)


@pytest.mark.parametrize("make", (
    lambda ps, ex: ShardedAdamOptimizer(torch.optim.Adam(ps, lr=1e-2), exchange=ex),
    lambda ps, ex: ShardedLARSOptimizer(torch.optim.SGD(ps, lr=0.1, momentum=0.9, weight_decay=1e-2),
                                        exchange=ex)), ids=("adam", "lars"))
def test_optimizer_step_matches_roundtripped_gradients(make):
    """Two steps at world 1: the wire on, against the wire off fed
    unpack(pack(g)). Every tensor is whole blocks, so the bucket's blocks are the tensors'."""
    def run(wire):
        torch.manual_seed(5)
        model = torch.nn.Sequential(torch.nn.Linear(32, 64), torch.nn.Linear(64, 32)).to(DEV)
        ex = NativeExchange(device=DEV).set_grad_wire(wire)
        opt = make(list(model.parameters()), ex)
        for step in range(2):
            for i, p in enumerate(model.parameters()):
                g = random_blocks(p.numel(), "f16", 50 * step + i).float().clamp(-3e4, 3e4).view_as(p)
                p.grad = g if wire else mx8_ref.roundtrip(g.flatten()).view_as(p).to(DEV)
            opt.step()
        torch.cuda.synchronize()
        ex.close()
        return [p.detach().clone() for p in model.parameters()]

    for i, (a, b) in enumerate(zip(run("mx8"), run(None))):
        same_bits(a, b, "parameter %d" % i)
