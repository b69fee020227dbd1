"""The sharded LARS step on the GPU, bit for bit: the apply plan and the trust kernel against
tests/lars_ref.py, ShardedLARSOptimizer against itself on tests/test_sharded_lars.py's epilogue."""
import numpy as np
import pytest
import torch

import capture
import lars_ref
import loopback
import test_sharded_lars as cpu

pytestmark = pytest.mark.gpu

_NP = {"f32": np.float32, "f64": np.float64}
_TORCH16 = {"bf16": torch.bfloat16, "f16": torch.float16}

# a tensor's row: ratio, weight_decay, momentum, 1 - dampening, -lr, flags
ROWS = np.array([[1.0, 0.0, 0.0, 1.0, -0.05, 0],                                   # momentum 0
                 [0.37, 1e-2, 0.9, 1.0, -0.05, lars_ref.MOMENTUM | lars_ref.FIRST],  # a first step
                 [2.5, 0.0, 0.9, 0.9, -0.1, lars_ref.MOMENTUM],                      # dampening
                 [1.0, 1e-2, 0.9, 1.0, -0.05, lars_ref.MOMENTUM | lars_ref.NESTEROV],
                 [0.37, 1e-2, 0.0, 1.0, -0.02, 0],
                 [0.6, 0.0, 0.8, 1.0, -0.05, lars_ref.MOMENTUM | lars_ref.NESTEROV | lars_ref.FIRST]])


def _dev(a):
    return torch.from_numpy(a.copy()).cuda()


def _dev16(bits, dt):
    return torch.from_numpy(bits.view(np.int16).copy()).cuda().view(_TORCH16[dt])


def _bytes(t):
    return t.cpu().view(torch.uint8).numpy().tobytes()


@pytest.mark.parametrize("np_", [0, 2, 3])
@pytest.mark.parametrize("dt", ["f32", "f64", "bf16", "f16"])
def test_apply_plan_bit_exact(dt, np_):
    """56 pieces: every head offset with the lengths 0, 1, N - 1, head + N, a tile -+ 1 and
    two tiles + 37, every length with every row of ROWS. Whole buffers are compared: sentinels
    around the pieces, the gradients and the momentum of a momentum-0 piece keep their bits."""
    from kungfu_amd import ops
    master = dt in _TORCH16
    cdt = "f32" if master else dt
    C, N, span = _NP[cdt], (2 if dt == "f64" else 4), (8 if master else 2 if dt == "f64" else 4)
    tile = ops.lars_apply_tile(torch.float64 if dt == "f64" else torch.float32)
    pieces, cur = [], 16
    for k in range(8):
        off = k % span
        head = (span - off) % span
        for n in (0, 1, N - 1, head + N, tile - 1, tile + 1, 2 * tile + 37):
            pieces.append((cur + off, n))
            cur = -(-(cur + off + n + 5) // 16) * 16 + 16  # sentinels between
    tensors = [i % len(ROWS) for i in range(len(pieces))]
    rng = np.random.default_rng(7)
    p, m = rng.standard_normal(cur).astype(C), rng.standard_normal(cur).astype(C)
    g = rng.standard_normal(cur).astype(C)
    g16 = lars_ref.narrow16(g, dt) if master else None
    p16 = rng.integers(0, 0x7000, cur).astype(np.uint16)
    dp, dm = _dev(p), _dev(m)
    dg = _dev16(g16, dt) if master else _dev(g)
    d16 = _dev16(p16, dt) if master else None
    cut = lambda t: [t[s:s + n] for s, n in pieces]  # noqa: E731
    plan = ops.lars_apply_plan(cut(dp), cut(dg), cut(dm), tensors, len(ROWS),
                               cut(d16) if master else None)
    plan.run(_dev(ROWS.reshape(-1)), np_)
    torch.cuda.synchronize()
    gw = lars_ref.widen16(g16, dt) if master else g
    want_p, want_m, want16 = p.copy(), m.copy(), p16.copy()
    for (s, n), t in zip(pieces, tensors):
        want_p[s:s + n], want_m[s:s + n] = lars_ref.apply(p[s:s + n], gw[s:s + n], m[s:s + n],
                                                         ROWS[t], cdt, np_)
        if master:
            want16[s:s + n] = lars_ref.narrow16(want_p[s:s + n], dt)
    assert _bytes(dp) == want_p.tobytes() and _bytes(dm) == want_m.tobytes(), "parameters, momentum"
    assert _bytes(dg) == (g16 if master else g).tobytes(), "the gradient was written"
    assert not master or _bytes(d16) == want16.tobytes(), "16-bit parameters"
    plan.close()


@pytest.mark.parametrize("np_", [0, 3])
@pytest.mark.parametrize("world", [1, 3])
def test_trust_kernel_bit_exact(world, np_):
    """17 groups (two launches), 300 tensors: adapt off (odd groups), a zero
    parameter norm, a zero gradient norm, both, and two group indices out of
    range, whose rows keep their bits."""
    from kungfu_amd import ops
    T, ngroup = 300, 17
    rng = np.random.default_rng(10 * world + np_)
    sq = np.exp2(rng.uniform(-40, 40, (world, 2 * T)))
    sq[:, 0] = sq[:, T + 1] = sq[:, 2] = sq[:, T + 2] = 0.0
    group_of = rng.integers(0, ngroup, T).astype(np.int32)
    group_of[:3], group_of[5], group_of[6] = 0, ngroup, -1
    hs = [lars_ref.hyper(1e-3 * (j + 1), 0.9 * (j % 3 != 0), 0.1 * (j % 2), 1e-4 * (j % 4),
                         j % 5 == 0, j % 7 == 0, 0.001 * (j + 1), 1e-8 * j, adapt=j % 2 == 0)
          for j in range(ngroup)]
    coef, ratio = (torch.full((k * T,), 9.0, dtype=torch.float64, device="cuda") for k in (6, 1))
    ops.lars_trust_update_(_dev(sq.reshape(-1)), world, _dev(group_of), hs, coef, ratio, np_)
    torch.cuda.synchronize()
    inside = (group_of >= 0) & (group_of < ngroup)
    want = lars_ref.trust(sq, [hs[j] if ok else hs[0] for j, ok in zip(group_of, inside)], np_)
    want[~inside] = 9.0
    assert list(want[:3, 0]) == [1.0, 1.0, 1.0] and (want[inside & (group_of % 2 == 1), 0] == 1).all()
    assert (want[inside & (group_of % 2 == 0), 0][3:] != 1).all()
    assert _bytes(coef) == want.tobytes() and _bytes(ratio) == want[:, 0].tobytes()


STEPS = (0, 1, 2, 3, 3)  # end to end: step 3's gradients and lr twice (the replays)


def _run(ex, kind, world, rank, graph=False):
    """-> (snapshot, [(gathered sums, np)] per step, what the graph reads)."""
    ps, opt = cpu.make_optimizer(ex, kind, "cuda")
    used, replayed, held = [], None, None
    for i, s in enumerate(STEPS):
        if replayed is None:
            cpu.feed(ps, opt, kind, world, rank, s, "cuda")
        if graph and i == 3:
            held = [p.grad for p in ps]  # alive: the captured copies into the buckets read these
            replayed = capture.capture(lambda stream: opt.step())
        replayed.replay() if replayed is not None else opt.step()
        (L,) = opt._kf_lars
        used.append((L["sq"].cpu().numpy().reshape(world, -1).copy(), opt._kf_groups[0]["np"]))
    return cpu.snapshot(ps, opt), used, held


@pytest.mark.parametrize("how", ["loopback2", "rccl1", "graph"])
@pytest.mark.parametrize("kind", ["f32", "bf16"])
def test_optimizer_end_to_end(kind, how):
    """Against the same optimizer on the numpy epilogue fed the device's sums.
    graph: the built-in world-1 exchange, the last two steps as replays of one
    captured step; not over the test transports: loopback synchronises the stream
    in every collective, RCCL's have never been recorded here."""
    got = {}
    if how == "loopback2":
        loopback.loop_ranks(2, lambda rank, ex: got.update({rank: _run(ex, kind, 2, rank)}))
    else:
        ex = loopback.rccl1_exchange() if how == "rccl1" else None
        got[0] = _run(ex, kind, 1, 0, graph=how == "graph")
        if ex is not None:
            ex.close()
    want, _ = cpu.run_ranks(len(got), kind, STEPS, fed=got[0][1])
    for r in got:
        cpu.assert_same(got[r][0], want[r])
    assert any(x != 1.0 for x in got[0][0][3]) and (kind == "f32" or got[0][0][2])
