"""Muon on the GPU against tests/muon_ref.py: the grouped MFMA GEMM element by
element within a derived bound, the Newton-Schulz chain within twice the
reference's own bf16-store deviation, and ShardedMuonOptimizer end to end, at
world 1 and 2 and through a captured graph."""
import functools

import numpy as np
import pytest
import torch

import capture
import loopback
import muon_ref

pytestmark = pytest.mark.gpu

NS_SHAPES = [(32, 32), (48, 80), (80, 48), (1, 64), (64, 1), (64, 3, 7, 7), (160, 272)]
SENTINEL = 0x5A5A  # a guard band's bf16 bit pattern


def _bf16_tensor(a):
    """Values exact in bf16 (any shape) -> a bf16 device tensor."""
    return torch.from_numpy(np.asarray(a, np.float32)).to(torch.bfloat16).cuda()


def _values(t):
    return t.detach().float().cpu().numpy().astype(np.float64)


def _offset_copy(a, odd):
    """a on the device as a matrix that starts one element (2 bytes) off a
    16-byte boundary when `odd`: the kernel's element-wise load path."""
    flat = torch.zeros(a.size + 8, dtype=torch.bfloat16, device="cuda")
    view = flat[int(odd):int(odd) + a.size].view(a.shape)
    view.copy_(_bf16_tensor(a))
    return view


def _guarded(m, n):
    """A sentinel-filled (m + 2) x (n + 2) matrix and its inner m x n window."""
    whole = torch.full((m + 2, n + 2), SENTINEL, dtype=torch.int16, device="cuda").view(torch.bfloat16)
    return whole, whole[1:m + 1, 1:n + 1]


@pytest.mark.parametrize("alpha,beta", [(muon_ref.A, 1.0), (muon_ref.B, muon_ref.C)])
@pytest.mark.parametrize("with_cin", [False, True])
@pytest.mark.parametrize("trans_b", [True, False], ids=["NT", "NN"])
def test_grouped_gemm(trans_b, with_cin, alpha, beta):
    from kungfu_amd import ops
    T = ops.muon_tile()
    shapes = [(1, 1, 1), (3, 7, 5), (32, 32, 16), (33, 31, 17), (48, 48, 80), (160, 272, 144),
              (2 * T + 5, 2 * T + 9, 2 * T + 3)]
    rng = np.random.default_rng(5)
    host, runs = [], ([], [])
    for i, (m, n, k) in enumerate(shapes):
        a, b, cin = (muon_ref.bf16(rng.standard_normal(s))
                     for s in ((m, k), (n, k) if trans_b else (k, n), (m, n)))
        host.append((a, b, cin if with_cin else None))
        da, db, dc = _offset_copy(a, i % 2), _offset_copy(b, i % 2), _offset_copy(cin, 0)
        for run in runs:
            whole, c = _guarded(m, n)
            run.append((whole, (da, db, c, dc if with_cin else None, False, trans_b)))
    for run in runs:
        ops.muon_gemm_grouped_([p for _, p in run], alpha, beta)
    torch.cuda.synchronize()
    for (m, n, k), (a, b, cin), (whole, prob), (again, _) in zip(shapes, host, *runs):
        ref, mag = muon_ref.gemm_ref(a, b, cin, alpha, beta, False, trans_b)
        got = _values(prob[2])
        bound = 2.0 ** -8 * np.abs(ref) + k * 2.0 ** -22 * mag
        worst = float((np.abs(got - ref) - bound).max())
        print("gemm", (m, n, k), "max |err| - bound", worst)
        assert worst <= 0, ((m, n, k), worst)
        raw = capture.host(whole.view(torch.int16), np.uint16).reshape(m + 2, n + 2).copy()
        assert raw.tobytes() == capture.host(again.view(torch.int16), np.uint16).tobytes()
        raw[1:m + 1, 1:n + 1] = SENTINEL
        assert (raw == SENTINEL).all(), ("written outside C", (m, n, k))


def _delta(d):
    """-> (pure-f64 X, the largest deviation of the bf16-store variant from it)."""
    d2 = d.reshape(d.shape[0], -1)
    pure = muon_ref.newton_schulz(d2, 5, muon_ref.identity)
    return pure, float(np.abs(muon_ref.newton_schulz(d2, 5, muon_ref.bf16) - pure).max())


def test_newton_schulz_chain():
    from kungfu_amd import ops
    rng = np.random.default_rng(1)
    ds = [muon_ref.bf16(rng.standard_normal(s)) for s in NS_SHAPES]
    ts = [_bf16_tensor(d) for d in ds]
    ops.muon_newton_schulz_(ts)
    torch.cuda.synchronize()
    for d, t in zip(ds, ts):
        pure, delta = _delta(d)
        got = _values(t).reshape(pure.shape)
        err = float(np.abs(got - pure).max())
        sv = np.linalg.svd(got, compute_uv=False)
        print("ns", d.shape, "delta", delta, "err", err, "sv", float(sv.min()), float(sv.max()))
        assert err <= 2 * delta, (d.shape, err, delta)
        assert 0.5 <= sv.min() and sv.max() <= 1.5, (d.shape, sv.min(), sv.max())


# ---- the optimizer end to end ---------------------------------------------------
HYPER = {"lr": 0.02, "momentum": 0.9, "weight_decay": 0.05}
BUCKET_ELTS = 16384  # three buckets
STEPS = (0, 1, 2)


def _params0():
    rng = np.random.default_rng(3)
    return [rng.standard_normal(s).astype(np.float32) for s in NS_SHAPES]


def _grads(world, step):
    """[rank][param] f32 whose sum over the ranks is exact: world * base."""
    rng = np.random.default_rng(11 + 100 * step)
    base = [(rng.integers(-32, 33, s) * 1.5).astype(np.float32) for s in NS_SHAPES]
    out = [[b.copy() for b in base] for _ in range(world)]
    for j, s in enumerate(NS_SHAPES if world == 2 else []):
        d = (rng.integers(-8, 9, s) * 1.5).astype(np.float32)
        out[0][j] += d
        out[1][j] -= d
    return out


def _run(ex, world, rank, nesterov, steps, graph=False):
    """-> (parameters, full momentum buffers, the buckets' padding), as numpy."""
    from kungfu_amd.optimizers import ShardedMuonOptimizer
    ps = [torch.nn.Parameter(torch.from_numpy(a).cuda()) for a in _params0()]
    opt = ShardedMuonOptimizer(torch.optim.SGD(ps, nesterov=nesterov, **HYPER), exchange=ex,
                               bucket_bytes=BUCKET_ELTS * 4)
    replayed = held = None
    for i, s in enumerate(steps):
        if replayed is None:
            for p, g in zip(ps, _grads(world, s)[rank]):
                p.grad = torch.from_numpy(g).cuda()
        if graph and i == len(steps) - 2:
            held = [p.grad for p in ps]  # alive: the captured copies into the buckets read these
            replayed = capture.capture(lambda stream: opt.step())
        replayed.replay() if replayed is not None else opt.step()
    torch.cuda.synchronize()
    del held
    moms = opt.momentum_buffers()
    (G,) = opt._kf_groups
    assert len(G["pb"].buckets) >= 2
    pads = [b[sp:].cpu().numpy() for b, sp in zip(G["pb"].buckets, G["pb"].spans)]
    return [p.detach().cpu().numpy() for p in ps], [moms[p].cpu().numpy() for p in ps], pads


@functools.lru_cache(maxsize=None)
def _device_run(how, nesterov, steps=STEPS, graph=False):
    from kungfu_amd.exchange import NativeExchange
    got = {}
    if how == "loopback2":
        loopback.loop_ranks(2, lambda r, ex: got.update({r: _run(ex, 2, r, nesterov, steps)}))
    else:
        ex = NativeExchange()
        got[0] = _run(ex, 1, 0, nesterov, steps, graph)
        ex.close()
    return got


@functools.lru_cache(maxsize=None)
def _reference(nesterov):
    """-> (parameters, momentum, per-parameter tolerance) after STEPS."""
    ps, ms = _params0(), [np.zeros(s, np.float32) for s in NS_SHAPES]
    tol = [0.0] * len(ps)
    for s in STEPS:
        g = _grads(1, s)[0]
        for j, (p, gj, m) in enumerate(zip(ps, g, ms)):  # this step's own delta per tensor
            _, d = muon_ref.momentum(gj, m, HYPER["momentum"], nesterov, 1)
            scale = max(1.0, p.shape[0] / (p.size // p.shape[0])) ** 0.5
            tol[j] += HYPER["lr"] * scale * 2 * _delta(d)[1]
        ps, ms = muon_ref.muon_step(ps, g, ms, HYPER["lr"], HYPER["momentum"], nesterov,
                                    HYPER["weight_decay"], 5)
    return ps, ms, tol


@pytest.mark.parametrize("nesterov", [False, True])
@pytest.mark.parametrize("how", ["builtin1", "loopback2"])
def test_optimizer_end_to_end(how, nesterov):
    got = _device_run(how, nesterov)
    wp, wm, tol = _reference(nesterov)
    for r, (ps, ms, pads) in got.items():
        for j, (p, m) in enumerate(zip(ps, ms)):
            assert m.tobytes() == wm[j].tobytes(), ("momentum", r, NS_SHAPES[j])
            err = float(np.abs(p.astype(np.float64) - wp[j]).max())
            print("step", how, nesterov, NS_SHAPES[j], "err", err, "tol", tol[j])
            assert err <= tol[j], ("params", r, NS_SHAPES[j], err, tol[j])
        assert all(not pad.any() for pad in pads), "the buckets' padding was written"
    if how == "loopback2":  # the replicas stay bit-identical
        assert capture.same_bytes(got[0][0], got[1][0])


def test_graph_replay():
    """The last step captured and replayed twice equals four eager steps."""
    steps = STEPS + STEPS[-1:]
    eager, replayed = _device_run("builtin1", True, steps), _device_run("builtin1", True, steps, True)
    for a, b in zip(eager[0], replayed[0]):
        assert capture.same_bytes(a, b)
