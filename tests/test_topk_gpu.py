"""The top-k gradient wire on the GPU, bit for bit against tests/topk_ref.py, sentinels behind every buffer."""
import numpy as np
import pytest
import torch

import loopback
import topk_ref as ref
from kungfu_amd import ops
from kungfu_amd.exchange import NativeExchange
from kungfu_amd.optimizers import ShardedAdamOptimizer
from test_mx8_gpu import DEV, KINDS, random_blocks, same_bits

pytestmark = pytest.mark.gpu
SHARDS = tuple(64 * n for n in (1, 2, 3, 5, 7, 8, 9, 33, 0))  # the pack's tiles: 8 blocks a wave, 32 a workgroup
FOLD_SHARDS = SHARDS + tuple(64 * n for n in (15, 16, 17))     # the fold's tile: 16 blocks


def special(kind):
    # seven blocks: ties with mixed signs; zeros; -0; r over g; a NaN; ten non-finite values; subnormals
    rng = np.random.default_rng(4)
    g = torch.from_numpy(rng.uniform(-1, 1, (7, 64))).to(ref.TORCH[kind]).float().numpy()
    r = g * np.float32(0.25)
    g[0], r[0] = 1.5 * np.float32(-1) ** (np.arange(64) // 3), 0.0
    g[1], r[1], g[2], r[2] = 0.0, 0.0, -0.0, -0.0
    r[3] = 1000 * g[3][::-1]
    g[4, 9] = np.nan
    g[5, 3:33:3] = np.array([np.inf, -np.inf, np.nan, np.inf, np.inf] * 2, np.float32)
    g[6], r[6] = 0.0, rng.integers(0, 1 << 17, 64).astype(np.uint32).view(np.float32) * np.float32(-1) ** np.arange(64)
    return torch.from_numpy(g.ravel()).to(ref.TORCH[kind]), r.ravel()


@pytest.mark.parametrize("world", (1, 2, 3))
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("k", ref.KS)
def test_pack_ef(k, kind, world):
    sg, sr = special(kind)
    grads, res, rng = [], [], np.random.default_rng(world)
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
    need = [world * ref.piece_bytes(q, k) for q in SHARDS]
    for call in range(2):  # the residual left in place feeds the second call
        bufs = [torch.full((n + 64,), 0xA5, dtype=torch.uint8, device=DEV) for n in need]
        ops.topk_pack_ef_batch_(grads, [r[:g.numel()] for r, g in zip(dres, grads)], world, k,
                                [b[:n] for b, n in zip(bufs, need)])
        for b, q in enumerate(SHARDS):
            pieces = ref.pack_pieces(host[b], res[b], q, world, k)
            what = "call %d bucket %d (q = %d)" % (call, b, q)
            same_bits(bufs[b], torch.from_numpy(np.concatenate(pieces + [np.full(64, 0xA5, np.uint8)])), what)
            same_bits(dres[b], torch.from_numpy(res[b]), "the residual, " + what)
            same_bits(grads[b], before[b], "the gradients, " + what)


@pytest.mark.parametrize("world,np_", [(w, n) for w in (1, 2, 3, 16) for n in sorted({0, w, 3})])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("k", ref.KS)
def test_fold(k, kind, world, np_):
    packed, outs, want = [], [], []
    for b, q in enumerate(FOLD_SHARDS):
        pieces = []
        for r in range(world):
            x = ref.widen(random_blocks(q, "f32", 100 * b + r))
            if q > 128:
                x[:64] = np.arange(64) % 7 - 3.0
                x[5] = 60000.0 - r  # every rank sends index 5: the sum leaves f16's range from world 2 on
                x[64:128] = 0.0     # ranks 0 .. 64 / k - 1 send places of their own
                x[64 + (r * k + np.arange(k)) % 64] = 1.0 + r + np.arange(k)
                x[q - 57] = np.nan if r == world // 2 else x[q - 57]
            pieces.append(ref.pack_ef(x, np.zeros(q, np.float32), k)[0])
        packed.append(torch.from_numpy(np.concatenate(pieces)).to(DEV))
        outs.append(torch.full((q + 8,), -7.0, dtype=ref.TORCH[kind], device=DEV))
        want.append(torch.cat([ref.fold(pieces, np_, kind, q, k) if q else outs[-1][:0].cpu(),
                               torch.full((8,), -7.0, dtype=ref.TORCH[kind])]))
    ops.topk_fold_batch_(packed, [o[:q] for o, q in zip(outs, FOLD_SHARDS)], world, k, np_)
    for b, q in enumerate(FOLD_SHARDS):
        same_bits(outs[b], want[b], "shard %d (q = %d)" % (b, q))


COUNTS = (64, 576, 128)  # shard lengths of the exchange's three buckets; the second has a tail


def exchange_case(world, k):  # -> buckets [rank][b], pieces [call][rank][b][piece], residuals after two calls
    counts = [q * world + (b == 1) * (world - 1) for b, q in enumerate(COUNTS)]
    data = [[random_blocks((n + 63) // 64 * 64, "bf16", 7 * r + b)[:n].clone()
             for b, n in enumerate(counts)] for r in range(world)]
    res = [[np.zeros(n, np.float32) for n in counts] for _ in range(world)]
    pieces = [[[ref.pack_pieces(ref.widen(data[r][b]), res[r][b], q, world, k) for b, q in enumerate(COUNTS)]
               for r in range(world)] for call in range(2)]
    return data, pieces, res


@pytest.mark.parametrize("world,k", ((1, 4), (2, 4), (2, 1), (1, 8)))
def test_exchange_reduce_shards(world, k):
    data, pieces, res = exchange_case(world, k)

    def body(r, ex):
        ex.algo = "a2a"
        tails = ex.all_reduce_([t.clone() for t in data[r]], average=True, coalesce=False)
        ex.set_grad_wire("topk", error_feedback=True, k=k)
        mine = [t.clone() for t in data[r]]
        for call in range(2):
            torch._foreach_copy_(mine, data[r])
            assert ex.reduce_shards_(mine) == 0
            for b, (q, s) in enumerate(zip(COUNTS, ex.grad_shards_(mine))):
                got = [pieces[call][j][b][r] for j in range(world)]
                same_bits(s, ref.fold(got, world, "bf16", q, k), "call %d rank %d bucket %d" % (call, r, b))
                same_bits(mine[b][q * world:], tails[b][q * world:], "rank %d tail %d" % (r, b))
        assert len(ex.grad_residuals()) == len(COUNTS)
        for b, t in enumerate(ex.grad_residuals()):
            same_bits(t, torch.from_numpy(res[r][b]), "rank %d residual %d" % (r, b))

    if world > 1:
        return loopback.loop_ranks(world, body)
    ex = NativeExchange(device=DEV)
    body(0, ex)
    ex.close()


def test_exchange_reduce_shards_from_a_graph():
    # world 1: two replays against two eager calls on twin buffers, all eager calls first and on the captured stream
    data = exchange_case(1, 2)[0][0]
    ex = NativeExchange(device=DEV).set_grad_wire("topk", error_feedback=True, k=2)
    eager, cap = ([t.clone() for t in data] for _ in range(2))
    want, graph, side = [], torch.cuda.CUDAGraph(), torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for call in range(2):
            torch._foreach_copy_(eager, data)
            assert ex.reduce_shards_(eager) == 0
            want.append([t.clone() for t in eager + ex.grad_residuals()[:3]])
        assert ex.reduce_shards_(cap) == 0
        mine = ex.grad_residuals()[3:]
        torch._foreach_zero_(mine)
        with torch.cuda.graph(graph, stream=side):
            assert ex.reduce_shards_(cap) == 0
        for call in range(2):
            torch._foreach_copy_(cap, data)
            graph.replay()
            torch.cuda.synchronize()
            for i, (got, w) in enumerate(zip(cap + mine, want[call])):
                same_bits(got, w, "replay %d tensor %d" % (call, i))
    ex.close()


def test_two_steps_leave_identical_replicas():  # world 2; finite; one non-zero residual per bucket
    torch.manual_seed(5)
    start = torch.nn.Sequential(torch.nn.Linear(32, 64), torch.nn.Linear(64, 32)).state_dict()
    got = {}

    def body(r, ex):
        model = torch.nn.Sequential(torch.nn.Linear(32, 64), torch.nn.Linear(64, 32))
        model.load_state_dict(start)
        model.to(DEV)
        opt = ShardedAdamOptimizer(torch.optim.Adam(model.parameters(), lr=1e-2),
                                   exchange=ex.set_grad_wire("topk", error_feedback=True))
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
