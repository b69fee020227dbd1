"""The 1-bit gradient wire on the GPU, bit for bit against tests/sign1_ref.py:
the pack and fold kernels (whole buffers, sentinels behind every packed area,
residual and shard), reduce_shards_ under set_grad_wire("sign1"), two steps
of two optimizers."""
import numpy as np
import pytest
import torch

import loopback
import sign1_ref as ref
from kungfu_amd import ops
from kungfu_amd.exchange import NativeExchange
from kungfu_amd.optimizers import ShardedAdamOptimizer, ShardedLionOptimizer
from test_mx8_gpu import DEV, KINDS, random_blocks, same_bits

pytestmark = pytest.mark.gpu
# shard lengths in blocks of 64. A wave's tile is 8 blocks and its scale store ends in one of
# five ways (1, 2 or 4, 3 or 5, 6 or 8, 7 blocks left); a workgroup's tile is 32 blocks.
# One block; 2, 3, 5, 6; a wave's tile less a block, exactly, plus one; a workgroup's plus one; empty
SHARDS = tuple(64 * k for k in (1, 2, 3, 5, 6, 7, 8, 9, 33, 0))


def special(kind):
    """(g, r) of eight blocks: r dominating g; g + r = +0; = -0; all zero; one
    inf; one NaN; a finite block whose sum overflows (64 x 2^122; f16
    gradients cannot reach it: an ordinary block there); f32-subnormal sums."""
    rng = np.random.default_rng(4)
    g = torch.from_numpy(rng.uniform(-1, 1, (8, 64))).to(ref.TORCH[kind]).float().numpy()
    r = g * np.float32(0.25)
    r[0] = 1000 * g[0][::-1]
    r[1] = -g[1]
    g[2], r[2] = -0.0, -0.0
    g[3], r[3] = 0.0, 0.0
    g[4, 9], g[5, 63] = np.inf, np.nan
    if kind != "f16":
        g[6], r[6] = 2.0 ** 122, 0.0
    g[7], r[7] = 0.0, rng.integers(0, 1 << 17, 64).astype(np.uint32).view(np.float32) * np.float32(-1) ** np.arange(64)
    return torch.from_numpy(g.ravel()).to(ref.TORCH[kind]), r.ravel()


@pytest.mark.parametrize("world", (1, 2, 3))
@pytest.mark.parametrize("kind", KINDS)
def test_pack_ef(kind, world):
    sg, sr = special(kind)
    grads, res = [], []
    rng = np.random.default_rng(world)
    for b, q in enumerate(SHARDS):  # a world - 1 tail behind every second bucket
        n = q * world + (b % 2) * (world - 1)
        g = random_blocks((n + 63) // 64 * 64, kind, 10 * world + b)[:n].clone()
        r = np.full(n + 8, -7.0, np.float32)  # the tail and 8 sentinels: -7
        r[:q * world] = ref.widen(g)[:q * world] * rng.uniform(-1, 1, q * world)
        if q * world >= sg.numel():
            g[:sg.numel()], r[:sr.size] = sg.to(DEV), sr
        grads.append(g)
        res.append(r)
    before, host = [g.clone() for g in grads], [ref.widen(g) for g in grads]
    dres = [torch.from_numpy(r).to(DEV) for r in res]
    need = [world * ref.piece_bytes(q) for q in SHARDS]
    for call in range(2):  # the residual left in place feeds the second call
        bufs = [torch.full((n + 64,), 0xA5, dtype=torch.uint8, device=DEV) for n in need]
        ops.sign1_pack_ef_batch_(grads, [r[:g.numel()] for r, g in zip(dres, grads)], world,
                                 [b[:n] for b, n in zip(bufs, need)])
        for b, q in enumerate(SHARDS):
            pieces = []
            for j in range(world):
                cut = slice(j * q, (j + 1) * q)
                p, res[b][cut] = ref.pack_ef(host[b][cut], res[b][cut])
                pieces.append(p)
            what = "call %d bucket %d (q = %d)" % (call, b, q)
            same_bits(bufs[b], torch.from_numpy(np.concatenate(pieces + [np.full(64, 0xA5, np.uint8)])), what)
            same_bits(dres[b], torch.from_numpy(res[b]), "the residual, " + what)
            same_bits(grads[b], before[b], "the gradients, " + what)


@pytest.mark.parametrize("world,np_", [(w, n) for w in (1, 2, 3, 16) for n in sorted({0, w, 3})])
@pytest.mark.parametrize("kind", KINDS)
def test_fold(kind, world, np_):
    packed, outs, want = [], [], []
    for b, q in enumerate(SHARDS):
        pieces = []
        for r in range(world):
            x = ref.widen(random_blocks(q, "f32", 100 * b + r))
            if q > 64:
                x[:64] = 60000.0 - r  # the ranks' sum leaves f16's range from world 2 on
            p = ref.pack_ef(x, np.zeros(q, np.float32))[0]
            if q and r == world // 2:  # the last block's scale is not finite; its bits stay, and are ignored
                assert p[q // 8 - 8:q // 8].any()
                p[q // 8 + q // 16 - 4:q // 8 + q // 16] = np.array([ref.NAN]).view(np.uint8)
            pieces.append(p)
        packed.append(torch.from_numpy(np.concatenate(pieces)).to(DEV))
        outs.append(torch.full((q + 8,), -7.0, dtype=ref.TORCH[kind], device=DEV))
        want.append(torch.cat([ref.fold(pieces, np_, kind, q) if q else outs[-1][:0].cpu(),
                               torch.full((8,), -7.0, dtype=ref.TORCH[kind])]))
    ops.sign1_fold_batch_(packed, [o[:q] for o, q in zip(outs, SHARDS)], world, np_)
    for b, q in enumerate(SHARDS):
        same_bits(outs[b], want[b], "shard %d (q = %d)" % (b, q))


COUNTS = (64, 576, 128)  # shard lengths of the exchange's three buckets; the second has a tail


@pytest.mark.parametrize("world", (1, 2))
def test_exchange_reduce_shards(world):
    counts = [q * world + (b == 1) * (world - 1) for b, q in enumerate(COUNTS)]
    data = [[random_blocks((n + 63) // 64 * 64, "bf16", 7 * r + b)[:n].clone()
             for b, n in enumerate(counts)] for r in range(world)]
    host = [[ref.widen(t) for t in row] for row in data]
    res = [[np.zeros(n, np.float32) for n in counts] for _ in range(world)]
    pieces = []  # [call][rank][bucket][piece]
    for call in range(2):
        pieces.append([[[] for _ in counts] for _ in range(world)])
        for r in range(world):
            for b, q in enumerate(COUNTS):
                for j in range(world):
                    cut = slice(j * q, (j + 1) * q)
                    p, res[r][b][cut] = ref.pack_ef(host[r][b][cut], res[r][b][cut])
                    pieces[call][r][b].append(p)

    def body(r, ex):
        ex.algo = "a2a"
        tails = ex.all_reduce_([t.clone() for t in data[r]], average=True, coalesce=False)
        ex.set_grad_wire("sign1", error_feedback=True)
        mine = [t.clone() for t in data[r]]
        for call in range(2):
            for m, t in zip(mine, data[r]):
                m.copy_(t)
            assert ex.reduce_shards_(mine) == 0
            for b, (q, s) in enumerate(zip(COUNTS, ex.grad_shards_(mine))):
                got = [pieces[call][j][b][r] for j in range(world)]
                same_bits(s, ref.fold(got, world, "bf16", q), "call %d rank %d bucket %d" % (call, r, b))
                same_bits(mine[b][q * world:], tails[b][q * world:], "rank %d tail %d" % (r, b))
        kept = ex.grad_residuals()
        assert len(kept) == len(counts)
        for b, t in enumerate(kept):
            same_bits(t, torch.from_numpy(res[r][b]), "rank %d residual %d" % (r, b))

    if world == 1:
        ex = NativeExchange(device=DEV)
        body(0, ex)
        ex.close()
    else:
        loopback.loop_ranks(world, body)


@pytest.mark.parametrize("make", (
    lambda ps, ex: ShardedAdamOptimizer(torch.optim.Adam(ps, lr=1e-2), exchange=ex),
    lambda ps, ex: ShardedLionOptimizer(torch.optim.AdamW(ps, lr=1e-3), exchange=ex, sign_wire=True)),
    ids=("adam", "lion-sign-wire"))
def test_two_steps_leave_identical_replicas(make):
    """Two steps at world 2 under the wire: every rank ends with the same
    parameters, bit for bit, and the exchange keeps one residual per bucket."""
    torch.manual_seed(5)
    start = torch.nn.Sequential(torch.nn.Linear(32, 64), torch.nn.Linear(64, 32)).state_dict()
    got = {}

    def body(r, ex):
        model = torch.nn.Sequential(torch.nn.Linear(32, 64), torch.nn.Linear(64, 32))
        model.load_state_dict(start)
        model.to(DEV)
        opt = make(list(model.parameters()), ex.set_grad_wire("sign1", error_feedback=True))
        for step in range(2):
            for i, p in enumerate(model.parameters()):
                p.grad = random_blocks(p.numel(), "f16", 50 * step + 7 * r + i).float().view_as(p)
            opt.step()
        torch.cuda.synchronize()
        assert len(ex.grad_residuals()) == sum(len(G["gb"].buckets) for G in opt._kf_groups) > 0
        assert all(t.abs().sum() > 0 for t in ex.grad_residuals())
        got[r] = [p.detach().clone() for p in model.parameters()]

    loopback.loop_ranks(2, body)
    for i, (a, b) in enumerate(zip(got[0], got[1])):
        same_bits(a, b, "parameter %d" % i)
        assert torch.isfinite(a).all(), i
