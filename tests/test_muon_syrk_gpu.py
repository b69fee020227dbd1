"""The symmetric product against tests/muon_ref.py and the general kernel's bits;
the chain and the optimizer under test_sharded_muon_gpu.py's own criteria."""
import functools

import numpy as np
import pytest
import torch

import capture
import muon_ref
import test_sharded_muon_gpu as base

pytestmark = pytest.mark.gpu

# (m, k): up to one tile; a 2 x 2 tile grid whose off-diagonal tile is one row
# wide; 3 x 3 grids (an interior off-diagonal tile), ragged and with 16-byte rows
SHAPES = [(1, 1), (3, 5), (33, 17), (64, 32), (65, 40), (2 * 64 + 5, 2 * 64 + 3), (160, 144)]
NS_SHAPES = [(32, 32), (48, 80), (80, 48), (1, 64), (64, 1), (160, 272), (272, 160)]


def _guarded(m, odd):
    """A sentinel-filled matrix and its inner m x m window: 16-byte aligned
    with 16-byte rows (the kernel's vector stores), or one element off."""
    whole = torch.full((m + 2, (m + 7) // 8 * 8 + 16), base.SENTINEL, dtype=torch.int16,
                       device="cuda").view(torch.bfloat16)
    return whole, whole[1:m + 1, 8 - 7 * odd:8 - 7 * odd + m]


def _bits(t):
    return capture.host(t.view(torch.int16), np.uint16).reshape(t.shape)


@pytest.mark.parametrize("alpha,beta", [(muon_ref.A, 1.0), (muon_ref.B, muon_ref.C)])
@pytest.mark.parametrize("with_cin", [False, True])
@pytest.mark.parametrize("trans_a", [False, True], ids=["NT", "TN"])
def test_grouped_syrk(trans_a, with_cin, alpha, beta):
    from kungfu_amd import ops
    rng = np.random.default_rng(7)
    host, runs, general, inplace = [], ([], []), [], []
    for i, (m, k) in enumerate(SHAPES):
        a, cin = (muon_ref.bf16(rng.standard_normal(s)) for s in ((k, m) if trans_a else (m, k), (m, m)))
        host.append((a, cin if with_cin else None))
        da, dc = base._offset_copy(a, i % 2), base._offset_copy(cin, i % 2) if with_cin else None
        for run in runs:
            whole, c = _guarded(m, i % 2)
            run.append((whole, (da, c, dc, trans_a)))
        general.append((da, da, torch.empty(m, m, dtype=torch.bfloat16, device="cuda"), dc,
                        trans_a, not trans_a))
        c = _guarded(m, i % 2)[1]
        if with_cin:
            c.copy_(dc)
        inplace.append((da, c, c if with_cin else None, trans_a))
    for run in runs:
        ops.muon_syrk_grouped_([p for _, p in run], alpha, beta)
    ops.muon_syrk_grouped_(inplace, alpha, beta)
    ops.muon_gemm_grouped_(general, alpha, beta)
    torch.cuda.synchronize()
    for i, ((m, k), (a, cin), (whole, prob), (again, _), gen, inp) in enumerate(
            zip(SHAPES, host, *runs, general, inplace)):
        ref, mag = muon_ref.gemm_ref(a, a, None if cin is None else np.tril(cin), alpha, beta,
                                     trans_a, not trans_a)
        got, low = base._values(prob[1]), np.tril(np.ones((m, m), bool))
        bound = 2.0 ** -8 * np.abs(ref) + k * 2.0 ** -22 * mag
        worst = float((np.abs(got - ref) - bound)[low].max())
        assert worst <= 0, ("max |err| - bound", (m, k), worst)
        bits = _bits(prob[1])
        assert (bits == bits.T).all(), ("not symmetric bit for bit", (m, k))
        assert (bits[low] == _bits(gen[2])[low]).all(), ("not the general kernel's bits", (m, k))
        assert (bits == _bits(inp[1])).all(), ("cin is c differs", (m, k))
        raw = _bits(whole)
        assert raw.tobytes() == _bits(again).tobytes()
        raw[1:m + 1, 8 - 7 * (i % 2):8 - 7 * (i % 2) + m] = base.SENTINEL
        assert (raw == base.SENTINEL).all(), ("written outside C", (m, k))


def test_newton_schulz_chain_symmetric():
    from kungfu_amd import ops
    rng = np.random.default_rng(1)
    ds = [muon_ref.bf16(rng.standard_normal(s)) for s in NS_SHAPES]
    ts, general = ([base._bf16_tensor(d) for d in ds] for _ in range(2))
    ops.muon_newton_schulz_(ts, symmetric=True)
    ops.muon_newton_schulz_(general)
    torch.cuda.synchronize()
    for d, t, g in zip(ds, ts, general):
        pure, delta = base._delta(d)
        got = base._values(t)
        err = float(np.abs(got - pure).max())
        sv = np.linalg.svd(got, compute_uv=False)
        print("ns symmetric", d.shape, "delta", delta, "err", err, "sv", float(sv.min()),
              float(sv.max()), "bytes equal the general chain's:", bool((_bits(t) == _bits(g)).all()))
        assert err <= 2 * delta, (d.shape, err, delta)
        assert 0.5 <= sv.min() and sv.max() <= 1.5, (d.shape, sv.min(), sv.max())


@pytest.fixture
def symmetric(monkeypatch):
    """test_sharded_muon_gpu.py's optimizer tests build symmetric=True, and run
    uncached: the cache of its device runs holds the general plan's results."""
    from kungfu_amd import optimizers
    monkeypatch.setattr(optimizers, "ShardedMuonOptimizer",
                        functools.partial(optimizers.ShardedMuonOptimizer, symmetric=True))
    monkeypatch.setattr(base, "_device_run", base._device_run.__wrapped__)


def test_optimizer_symmetric_world2_and_graph_replay(symmetric):
    base.test_optimizer_end_to_end("loopback2", True)
    base.test_graph_replay()
