"""The MXFP8 wire's error-feedback and stochastic-rounding packs on the GPU,
bit for bit against tests/mx8_ef_sr_ref.py: the two pack kernels (whole
buffers, sentinels behind codes and residuals), reduce_shards_ under each mode
of set_grad_wire, two optimizer steps under error feedback."""
import numpy as np
import pytest
import torch

import loopback
import mx8_ef_sr_ref as ref
import mx8_ref
from kungfu_amd import ops
from kungfu_amd.exchange import NativeExchange
from kungfu_amd.optimizers import ShardedAdamOptimizer
from test_mx8_ef_sr import SR_KNOWN
from test_mx8_gpu import COUNTS, DEV, KINDS, SHARDS, random_blocks, same_bits

pytestmark = pytest.mark.gpu


def ef_special(kind):
    """(g, r) of six blocks: r dominating g; g + r = +0; = -0; overflowing
    (f16 gradients cannot reach it: the largest finite sum there); f32-subnormal
    sums; r alone."""
    rng = np.random.default_rng(4)
    g = torch.from_numpy(rng.uniform(-1, 1, (6, 32))).to(mx8_ref.TORCH[kind]).float().numpy()
    r = g * np.float32(2.0 ** -5)
    r[0] = 1000 * g[0][::-1]
    r[1] = -g[1]
    g[2], r[2] = -0.0, -0.0
    g[3, 7], r[3, 7] = (65504.0 if kind == "f16" else 2.0 ** 104), np.finfo(np.float32).max
    g[4], r[4] = 0.0, rng.integers(0, 1 << 23, 32).astype(np.uint32).view(np.float32)
    g[5] = 0.0
    return torch.from_numpy(g.ravel()).to(mx8_ref.TORCH[kind]), r.ravel()


def buckets(kind, world, extra=None):
    """One bucket per SHARDS length with a world - 1 tail behind every second
    one; `extra` (a tensor of `kind`) opens every bucket it fits in."""
    out = []
    for b, q in enumerate(SHARDS):
        n = q * world + (b % 2) * (world - 1)
        g = random_blocks((n + 31) // 32 * 32, kind, 10 * world + b, special=True)[:n].clone()
        if extra is not None and q * world >= extra.numel() + 1024:
            g[:extra.numel()] = extra.to(DEV)
        out.append(g)
    return out


def packed_buffers(world):
    """every bucket's packed buffer with 64 sentinel bytes behind it, and the views without them"""
    need = [world * mx8_ref.piece_bytes(q) for q in SHARDS]
    bufs = [torch.full((n + 64,), 0xA5, dtype=torch.uint8, device=DEV) for n in need]
    return bufs, [b[:n] for b, n in zip(bufs, need)]


def want_packed(pieces):
    return torch.from_numpy(np.concatenate(list(pieces) + [np.full(64, 0xA5, np.uint8)]))


@pytest.mark.parametrize("world", (1, 2, 3))
@pytest.mark.parametrize("kind", KINDS)
def test_pack_ef(kind, world):
    sg, sr = ef_special(kind)
    grads = buckets(kind, world, sg)
    before = [g.clone() for g in grads]
    host, res = [mx8_ref.widen(g) for g in grads], []
    rng = np.random.default_rng(world)
    for x, q in zip(host, SHARDS):  # about 2^-5 of the block's scale; the tail and 8 sentinels: -7
        r = np.full(x.size + 8, -7.0, np.float32)
        top = np.nan_to_num(np.abs(x[:q * world]).reshape(-1, 32).max(axis=1), posinf=1.0).repeat(32)
        r[:q * world] = top * rng.uniform(-1, 1, q * world) * 2.0 ** -5
        if q * world >= sr.size + 1024:
            r[:sr.size] = sr
        res.append(r)
    dres = [torch.from_numpy(r).to(DEV) for r in res]
    for call in range(2):  # the residual left in place feeds the second call
        bufs, views = packed_buffers(world)
        ops.mx8_pack_ef_batch_(grads, [r[:g.numel()] for r, g in zip(dres, grads)], world, views)
        for b, q in enumerate(SHARDS):
            out = [ref.pack_ef(host[b][j * q:(j + 1) * q], res[b][j * q:(j + 1) * q]) for j in range(world)]
            for j, (_, r) in enumerate(out):
                res[b][j * q:(j + 1) * q] = r
            what = "call %d bucket %d (q = %d)" % (call, b, q)
            same_bits(bufs[b], want_packed(p for p, _ in out), what)
            same_bits(dres[b], torch.from_numpy(res[b]), "the residual, " + what)
            same_bits(grads[b], before[b], "the gradients, " + what)


@pytest.mark.parametrize("world", (1, 2, 3))
@pytest.mark.parametrize("kind", KINDS)
def test_pack_sr(kind, world):
    known = np.zeros(32, np.float32)
    known[:len(SR_KNOWN)] = [v for v, _, _ in SR_KNOWN]
    grads = buckets(kind, world, torch.from_numpy(known).to(mx8_ref.TORCH[kind]))
    host, seen = [mx8_ref.widen(g) for g in grads], []
    # (step, rank, bucket0); a rank needs a world that has it
    for step, rank, b0 in ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 5)):
        if rank >= world:
            continue
        bufs, views = packed_buffers(world)
        ops.mx8_pack_sr_batch_(grads, world, 9, step, rank, b0, views)
        for b, q in enumerate(SHARDS):
            want = [ref.pack_sr(host[b][j * q:(j + 1) * q], 9, step, rank, b0 + b, j * q)
                    for j in range(world)]
            same_bits(bufs[b], want_packed(want), "step %d rank %d bucket %d + %d" % (step, rank, b0, b))
        seen.append(torch.cat(bufs).cpu())
    assert all(not torch.equal(a, b) for i, a in enumerate(seen) for b in seen[:i])


@pytest.mark.parametrize("world", (1, 2))
@pytest.mark.parametrize("mode", ("ef", "sr"))
def test_exchange_reduce_shards(mode, world):
    counts = [q * world + (b == 1) * (world - 1) for b, q in enumerate(COUNTS)]
    data = [[random_blocks((n + 31) // 32 * 32, "bf16", 7 * r + b)[:n].clone()
             for b, n in enumerate(counts)] for r in range(world)]
    host = [[mx8_ref.widen(t) for t in row] for row in data]
    res = [[np.zeros(n, np.float32) for n in counts] for _ in range(world)]
    pieces = []  # [call][rank][bucket][piece]
    for call in range(2):
        pieces.append([[[] for _ in counts] for _ in range(world)])
        for r in range(world):
            for b, q in enumerate(COUNTS):
                for j in range(world):
                    cut = slice(j * q, (j + 1) * q)
                    if mode == "ef":
                        p, res[r][b][cut] = ref.pack_ef(host[r][b][cut], res[r][b][cut])
                    else:
                        p = ref.pack_sr(host[r][b][cut], 3, call, r, b, j * q)
                    pieces[call][r][b].append(p)

    def body(r, ex):
        ex.set_grad_wire("mx8", error_feedback=mode == "ef",
                         rounding="stochastic" if mode == "sr" else "nearest", seed=3)
        mine = [t.clone() for t in data[r]]
        for call in range(2):
            for m, t in zip(mine, data[r]):
                m.copy_(t)
            assert ex.reduce_shards_(mine) == 0
            for b, (q, s) in enumerate(zip(COUNTS, ex.grad_shards_(mine))):
                got = [pieces[call][j][b][r] for j in range(world)]
                same_bits(s, mx8_ref.fold(got, world, "bf16"), "call %d rank %d bucket %d" % (call, r, b))
        kept = ex.grad_residuals()
        assert len(kept) == (len(counts) if mode == "ef" else 0)
        for b, t in enumerate(kept):
            same_bits(t, torch.from_numpy(res[r][b]), "rank %d residual %d" % (r, b))

    if world == 1:
        ex = NativeExchange(device=DEV)
        body(0, ex)
        ex.close()
        assert ex.grad_residuals() == []
    else:
        loopback.loop_ranks(world, body)


def test_adam_steps_match_fed_back_gradients():
    """Two steps at world 1 under error feedback, against the wire off fed
    unpack(pack_ef(g, r)). Every tensor is whole blocks, so the bucket's blocks
    and residuals are the tensors'."""
    def run(wire):
        torch.manual_seed(5)
        model = torch.nn.Sequential(torch.nn.Linear(32, 64), torch.nn.Linear(64, 32)).to(DEV)
        ex = NativeExchange(device=DEV).set_grad_wire(wire, error_feedback=bool(wire))
        opt = ShardedAdamOptimizer(torch.optim.Adam(list(model.parameters()), lr=1e-2), exchange=ex)
        res = [np.zeros(p.numel(), np.float32) for p in model.parameters()]
        for step in range(2):
            for i, p in enumerate(model.parameters()):
                g = random_blocks(p.numel(), "f16", 50 * step + i).float().clamp(-3e4, 3e4)
                if not wire:
                    piece, res[i] = ref.pack_ef(mx8_ref.widen(g), res[i])
                    g = torch.from_numpy(mx8_ref.unpack(piece, g.numel())).to(DEV)
                p.grad = g.view_as(p)
            opt.step()
        torch.cuda.synchronize()
        ex.close()
        return [p.detach().clone() for p in model.parameters()]

    for i, (a, b) in enumerate(zip(run("mx8"), run(None))):
        same_bits(a, b, "parameter %d" % i)
