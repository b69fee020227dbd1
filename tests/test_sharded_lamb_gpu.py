"""The sharded LAMB step on the GPU, bit for bit against tests/lamb_ref.py: the
two moments kernels, the trust kernel, the apply plan, gather_params_ and the
whole step over the loopback transport and a one-rank librccl communicator,
and ShardedLAMBOptimizer end to end."""
import numpy as np
import pytest
import torch

import lamb_ref
import loopback
import test_sharded_adam_gpu as ag
import test_sharded_lamb as cpu

pytestmark = pytest.mark.gpu

# kf_lamb.hip's launch shape, pinned to the source by tests/test_sharded_lamb.py
LAMB_SEG, LAMB_MASTER_SEG = cpu.LAMB_SEG, cpu.LAMB_MASTER_SEG
SIZES = (1, 3, 1021, 4096, 100003)
_INT = {2: np.int16, 4: np.int32, 8: np.int64}
_TORCH16 = {"bf16": torch.bfloat16, "f16": torch.float16}


def _same(got, want):
    """Bit equality of two arrays of one dtype; NaNs are compared by position."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype)
    if got.dtype.kind != "f":
        return np.array_equal(got, want)
    gn, wn = np.isnan(got), np.isnan(want)
    it = _INT[got.dtype.itemsize]
    return np.array_equal(gn, wn) and np.array_equal(got.view(it)[~gn], want.view(it)[~wn])


def _dev16(bits, dt):
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16).copy()).cuda().view(_TORCH16[dt])


def _host16(t):
    return t.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16).copy()


def _segments(dt, n_ones):
    """[(p, g, m, v)] in dt's numpy form ("f32" / "f64"): SIZES, then n_ones
    one-element segments, with tests/test_sharded_adam_gpu.py's random data,
    its all-binade v and its IEEE specials quadruples at the start of the 4096
    segment, at the end of the 1021 one and in the one-element segments."""
    sp = ag._specials(dt)
    k = len(sp[0])
    assert k <= n_ones
    segs = ag._fill(dt, SIZES + (1,) * n_ones)
    for i, seg in enumerate(segs):
        n = seg[0].size
        for a, s in zip(seg, sp):
            if n == 4096:
                a[:k] = s
            elif n == 1021:
                a[-k:] = s
            elif n == 1 and i >= len(SIZES) and i - len(SIZES) < k:
                a[0] = s[i - len(SIZES)]
    return segs


@pytest.fixture(scope="module")
def segments():
    return {"f32": _segments("f32", LAMB_SEG + 8), "f64": _segments("f64", LAMB_SEG + 8),
            "master": _segments("f32", LAMB_MASTER_SEG + 8)}


def _hypers(n, wd):
    # a hyper of its own per segment: the betas differ
    return [lamb_ref.hyper(1e-2, betas=(0.9 - 0.1 * (i % 3), 0.999), eps=1e-6, weight_decay=wd,
                           step=3) for i in range(n)]


@pytest.mark.parametrize("wd", [0.0, 1e-2])
@pytest.mark.parametrize("np_", [0, 3])
@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_moments_kernel_bit_exact(segments, dt, np_, wd):
    from kungfu_amd import ops
    segs = segments[dt]
    assert sum(1 for s in segs if s[0].size == 1) > LAMB_SEG
    hs = _hypers(len(segs), wd)
    ps, gs, ms, vs = ([ag._dev(seg[j], dt) for seg in segs] for j in range(4))
    us = [torch.full_like(p, 7.0) for p in ps]
    ops.lamb_moments_batch_(ps, gs, ms, vs, us, hs, np_=np_)
    torch.cuda.synchronize()
    for i, (seg, h) in enumerate(zip(segs, hs)):
        wm, wv, wu = lamb_ref.moments(*seg, dt, h, np_)
        where = (dt, np_, wd, i, seg[0].size)
        assert _same(ag._host(ms[i], dt), wm), ("exp_avg",) + where
        assert _same(ag._host(vs[i], dt), wv), ("exp_avg_sq",) + where
        assert _same(ag._host(us[i], dt), wu), ("update",) + where
        assert ag._host(ps[i], dt).tobytes() == seg[0].tobytes(), ("param was written",) + where
        assert ag._host(gs[i], dt).tobytes() == seg[1].tobytes(), ("grad was written",) + where


@pytest.mark.parametrize("wd", [0.0, 1e-2])
@pytest.mark.parametrize("np_", [0, 3])
@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_master_moments_kernel_bit_exact(segments, dt, np_, wd):
    """The gradient is the f32 data narrowed to 16 bits (specials included:
    the largest finite f32 becomes inf, its subnormal a zero), plus the
    16-bit format's own largest finite value and smallest subnormal."""
    from kungfu_amd import ops
    segs = segments["master"]
    assert sum(1 for s in segs if s[0].size == 1) > LAMB_MASTER_SEG
    hs = _hypers(len(segs), wd)
    g16 = [lamb_ref.narrow16(seg[1], dt) for seg in segs]
    big, sub = (0x7F7F, 0x0001) if dt == "bf16" else (0x7BFF, 0x0001)
    g16[3][40:44] = (big, big | 0x8000, sub, sub | 0x8000)
    ws, ms, vs = ([ag._dev(seg[j], "f32") for seg in segs] for j in (0, 2, 3))
    gs = [_dev16(g, dt) for g in g16]
    us = [torch.full_like(w, 7.0) for w in ws]
    ops.lamb_master_moments_batch_(gs, ws, ms, vs, us, hs, np_=np_)
    torch.cuda.synchronize()
    for i, (seg, h) in enumerate(zip(segs, hs)):
        wm, wv, wu = lamb_ref.moments(seg[0], lamb_ref.widen16(g16[i], dt), seg[2], seg[3], "f32",
                                      h, np_)
        where = (dt, np_, wd, i, seg[0].size)
        assert _same(ag._host(ms[i], "f32"), wm), ("exp_avg",) + where
        assert _same(ag._host(vs[i], "f32"), wv), ("exp_avg_sq",) + where
        assert _same(ag._host(us[i], "f32"), wu), ("update",) + where
        assert ag._host(ws[i], "f32").tobytes() == seg[0].tobytes(), ("master was written",) + where
        assert _host16(gs[i]).tobytes() == g16[i].tobytes(), ("grad was written",) + where


def test_moments_refuse_the_other_dtypes():
    from kungfu_amd import _lib, ops
    h = [lamb_ref.hyper(1e-3)]
    for dtype in (torch.float16, torch.bfloat16):
        x = [torch.zeros(8, dtype=dtype, device="cuda") for _ in range(5)]
        with pytest.raises(_lib.KungFuAMDError, match="KF_ERR_DTYPE"):
            ops.lamb_moments_batch_([x[0]], [x[1]], [x[2]], [x[3]], [x[4]], h)
    lib = _lib.load()
    x = [torch.zeros(8, device="cuda") for _ in range(5)]
    one = [_lib.ptr_array([t.data_ptr()]) for t in x]
    cnt = (cpu.ctypes.c_size_t * 1)(8)
    assert lib.kf_lamb_master_moments_batch(*one, cnt, 1, cpu.F32, 0, _lib.adam_hyper_array(h),
                                            None) == cpu.ERR_DTYPE


# ---- the trust kernel ----------------------------------------------------------

@pytest.mark.parametrize("ngroup", [1, 20])
@pytest.mark.parametrize("world,T", [(1, 1), (3, 1), (1, 300), (3, 300)])
def test_trust_kernel_bit_exact(world, T, ngroup):
    from kungfu_amd import ops
    rng = np.random.default_rng(100 * world + T + ngroup)
    sq = np.exp2(rng.uniform(-40, 40, (world, 2 * T)))
    if T > 8:
        sq[:, 0] = 0.0              # P = 0
        sq[:, T + 1] = 0.0          # U = 0
        sq[:, 2] = sq[:, T + 2] = 0.0
        sq[world - 1, 3] = np.inf
        sq[0, T + 4] = np.inf
        sq[0, 5] = sq[world - 1, T + 5] = np.inf
        sq[0, 6] = np.nan
        sq[world - 1, T + 7] = np.nan
    group_of = rng.integers(0, ngroup, T).astype(np.int32)
    for adapt_all, clip in ((None, 0.0), (None, 1.5), (False, 0.0), (True, 0.25)):
        groups = [{"lr": 1e-3 * (j + 1), "adapt": (j % 2 == 0) if adapt_all is None else adapt_all}
                  for j in range(ngroup)]
        nlr = torch.full((T,), 9.0, dtype=torch.float64, device="cuda")
        ratio = torch.full((T,), 9.0, dtype=torch.float64, device="cuda")
        ops.lamb_trust_update_(torch.from_numpy(sq.reshape(-1).copy()).cuda(), world,
                               torch.from_numpy(group_of).cuda(), groups, nlr, ratio,
                               trust_clip=clip)
        torch.cuda.synchronize()
        want_nlr, want_ratio = lamb_ref.trust(sq, [groups[j]["lr"] for j in group_of],
                                              [groups[j]["adapt"] for j in group_of], clip)
        assert _same(ratio.cpu().numpy(), want_ratio), (world, T, ngroup, adapt_all, clip)
        assert _same(nlr.cpu().numpy(), want_nlr), (world, T, ngroup, adapt_all, clip)
        if adapt_all is False:
            assert np.array_equal(want_ratio, np.ones(T))
        if T > 8 and adapt_all is not False and clip == 0.0:
            assert want_ratio[0] == 1 and want_ratio[1] == 1 and want_ratio[2] == 1


# ---- the apply plan ------------------------------------------------------------

GUARD = 5  # untouched elements before and after every piece, at least


def _layout():
    """[(start, length)] of 300+ pieces in one flat buffer: every element
    offset 0..8 from a 16-byte boundary (16 elements of any width up to 8
    bytes are a multiple of 16 bytes) with lengths 1, 2, 7, 8, 9 and 1021,
    100003 at three offsets, and small ones after them."""
    pieces, cur = [], 16

    def add(off, n):
        nonlocal cur
        start = cur + off
        pieces.append((start, n))
        cur = -(-(start + n + GUARD) // 16) * 16 + 16

    for off in range(9):
        for n in (1, 2, 7, 8, 9, 1021):
            add(off, n)
    for off in (0, 3, 5):
        add(off, 100003)
    i = 0
    while len(pieces) < 305:
        add(i % 9, 1 + (i * 7) % 23)
        i += 1
    return pieces, cur


@pytest.mark.parametrize("dt", ["f32", "f64", "bf16", "f16"])
def test_apply_plan_bit_exact(dt):
    from kungfu_amd import _lib, ops
    pieces, total = _layout()
    assert len(pieces) >= 300
    master = dt in ("bf16", "f16")
    cdt = "f32" if master else dt
    C = lamb_ref.COMPUTE[cdt]
    rng = np.random.default_rng(5)
    T = 37
    p = rng.standard_normal(total).astype(C)
    u = rng.standard_normal(total).astype(C)
    u[pieces[5][0]] = np.inf
    u[pieces[40][0]:pieces[40][0] + 3] = (np.nan, -0.0, 0.0)
    p[pieces[41][0]] = -0.0
    nlr = -np.exp2(rng.uniform(-12, 2, T))
    nlr[3] = -0.0
    p16 = rng.integers(0, 0x7000, total).astype(np.uint16)  # guard words: any finite pattern
    dp, du = ag._dev(p, cdt), ag._dev(u, cdt)
    d16 = _dev16(p16, dt) if master else None
    tensors = [i % T for i in range(len(pieces))]
    plan = ops.LambApplyPlan([dp[s:s + n] for s, n in pieces], [du[s:s + n] for s, n in pieces],
                             tensors, T,
                             [d16[s:s + n] for s, n in pieces] if master else None)
    plan.run(torch.from_numpy(nlr).cuda())
    torch.cuda.synchronize()
    want, want16 = p.copy(), p16.copy()
    for (s, n), t in zip(pieces, tensors):
        want[s:s + n] = lamb_ref.apply(p[s:s + n], u[s:s + n], nlr[t], cdt)
        want16[s:s + n] = lamb_ref.narrow16(want[s:s + n], dt) if master else 0
    # the whole buffers: the guard words around every piece keep their bits
    assert _same(ag._host(dp, cdt), want), dt
    assert ag._host(du, cdt).tobytes() == u.tobytes(), "update was written"
    if master:
        assert np.array_equal(_host16(d16), want16), dt
    plan.close()
    # a piece whose arrays do not share their offset is refused
    if not master:
        with pytest.raises(_lib.KungFuAMDError, match="KF_ERR_ARG"):
            ops.LambApplyPlan([dp[16:32]], [du[17:33]], [0], 1)
    empty = ops.LambApplyPlan([dp[16:16]], [du[16:16]], [0], 1,
                              [d16[16:16]] if master else None)
    empty.run(torch.zeros(1, dtype=torch.float64, device="cuda"))
    torch.cuda.synchronize()
    assert _same(ag._host(dp, cdt), want), "an empty plan wrote"


# ---- gather_params_ and the whole step ----------------------------------------

def test_gather_params_over_loopback():
    from kungfu_amd.collective import padded_count
    world, got, times = 3, {}, {}
    counts = [padded_count(n, world, 4) for n in (5, 1031, 2050)]

    def body(rank, ex):
        ps = []
        for b, L in enumerate(counts):
            q = L // world
            p = torch.full((L,), -1.0, device="cuda")
            p[rank * q:(rank + 1) * q] = torch.arange(q, device="cuda") + 1000.0 * rank + 10 * b
            ps.append(p)
        if rank == 0:  # counts % world: refused before any collective
            from kungfu_amd import _lib
            bad = (cpu.ctypes.c_size_t * 1)(4)
            assert ex.lib.kf_exchange_gather_params_batch(
                ex._h, _lib.ptr_array([ps[0].data_ptr()]), bad, 1, cpu.F32, None) == cpu.ERR_ARG
        ex.set_timing(True)
        ex.gather_params_(ps)
        torch.cuda.synchronize()
        times[rank] = ex.phase_times()
        ex.set_timing(False)
        got[rank] = [p.cpu().numpy() for p in ps]

    loopback.loop_ranks(world, body)
    for b, L in enumerate(counts):
        q = L // world
        want = np.concatenate([np.arange(q, dtype=np.float32) + np.float32(1000.0 * r + 10 * b)
                               for r in range(world)])
        for r in range(world):
            assert np.array_equal(got[r][b], want), (r, b)
    for r in range(world):
        assert times[r]["calls"] == 1 and times[r]["all_gather"] > 0, times[r]


def _run_model(world, rank, ex, steps=cpu.STEPS):
    """tests/test_sharded_lamb.py's model (an f32 group and an f16 group with
    master weights) on the GPU; per step the device's norm sums, at the end
    the parameters, the state and the ratios."""
    ps, opt = cpu.make_optimizer(ex, device="cuda", sixteen="f16")
    sums = []
    for s in range(steps):
        cpu.set_grads(ps, world, rank, s, device="cuda", sixteen="f16")
        opt.step()
        sums.append([L["sq"].cpu().numpy().reshape(world, -1).copy() for L in opt._kf_lamb])
        cpu.schedule(opt)
    sb = opt.state_buffers()
    ratios = opt.last_trust_ratios()
    torch.cuda.synchronize()
    none = {"exp_avg": torch.zeros(0), "exp_avg_sq": torch.zeros(0)}  # zero-element tensors
    k = len(cpu.NUMELS)
    return {"p": [cpu.to_numpy(p) for p in ps],
            "m": [sb.get(p, none)["exp_avg"].cpu().numpy().reshape(-1) for p in ps],
            "v": [sb.get(p, none)["exp_avg_sq"].cpu().numpy().reshape(-1) for p in ps],
            "w": [sb.get(p, {"master": torch.zeros(0)})["master"].cpu().numpy().reshape(-1)
                  if j >= k else None for j, p in enumerate(ps)],
            "ratio": [ratios[p] for p in ps], "sums": sums,
            "cuts": cpu.model_cuts(opt, world)}


def _check_model(got, world):
    """Every rank against lamb_ref run on the unsharded tensors with the
    device's own norm sums; the device's sums against the host's within
    kf_segnorm's bound, (n + 2) * 2^-53 relative, on both sides."""
    want = cpu.reference_run(world, sixteen="f16", sums=got[0]["sums"], cuts=got[0]["cuts"])
    for r in range(world):
        g = got[r]
        for a, b in zip(g["sums"], got[0]["sums"]):
            for x, y in zip(a, b):
                assert np.array_equal(x, y), ("ranks disagree on the sums", r)
        for j in range(len(want["p"])):
            assert _same(g["p"][j], want["p"][j]), ("param", r, j)
            assert _same(g["m"][j], want["m"][j]), ("exp_avg", r, j)
            assert _same(g["v"][j], want["v"][j]), ("exp_avg_sq", r, j)
            if want["w"][j] is not None:
                assert _same(g["w"][j], want["w"][j]), ("master", r, j)
            assert g["ratio"][j] == want["ratio"][j], ("ratio", r, j)
    for dev, host, n in want["sum_checks"]:
        assert abs(dev - host) <= 2 * (n + 2) * 2.0 ** -53 * host, (dev, host, n)
    # the zero-element tensors have ratio 1
    for j, numel in enumerate(cpu.NUMELS * 2):
        if numel == 0:
            assert got[0]["ratio"][j] == 1.0


@pytest.mark.parametrize("world", [2, 3])
def test_whole_step_over_loopback(world):
    got = {}

    def body(rank, ex):
        got[rank] = _run_model(world, rank, ex)

    loopback.loop_ranks(world, body)
    _check_model(got, world)


def test_whole_step_world1_every_exchange_same_bits():
    """A one-rank librccl communicator (the collectives run), a plain
    NativeExchange() (world 1 on the built-in transport) and the default
    collective.Exchange() give the same bits, lamb_ref's."""
    from kungfu_amd.exchange import NativeExchange
    outs = []
    for make in (loopback.rccl1_exchange, NativeExchange, lambda: None):
        ex = make()
        outs.append(_run_model(1, 0, ex))
        if ex is not None:
            ex.close()
    for o in outs:
        _check_model({0: o}, 1)
    for o in outs[1:]:
        for j in range(len(o["p"])):
            assert _same(o["p"][j], outs[0]["p"][j]), j


# ---- ShardedLAMBOptimizer on a model --------------------------------------------

def _two_layer(ex, world, rank, steps=3):
    torch.manual_seed(0)
    model = torch.nn.Sequential(torch.nn.Linear(9, 17), torch.nn.Tanh(), torch.nn.Linear(17, 3)).cuda()
    from kungfu_amd.torch.optimizers import ShardedLAMBOptimizer
    decay = [p for n, p in model.named_parameters() if n.endswith("weight")]
    plain = [p for n, p in model.named_parameters() if n.endswith("bias")]
    opt = ShardedLAMBOptimizer(
        torch.optim.AdamW([{"params": decay, "weight_decay": 1e-2},
                           {"params": plain, "weight_decay": 0.0}], lr=1e-2, eps=1e-6),
        model.named_parameters(), exchange=ex, bucket_bytes=256)
    gen = torch.Generator().manual_seed(100 + rank)
    losses = []
    for _ in range(steps):
        x = torch.randn(8, 9, generator=gen).cuda()
        y = torch.randn(8, 3, generator=gen).cuda()
        opt.zero_grad()
        loss = ((model(x) - y) ** 2).mean()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    ratios = opt.last_trust_ratios()
    torch.cuda.synchronize()
    return [p.detach().cpu().numpy().copy() for p in model.parameters()], \
        [ratios[p] for p in model.parameters()], losses


def test_optimizer_two_layer_model():
    """World 1 on every exchange: the same bits, finite, the weights' ratios
    are ||p|| / ||u|| (not 1) and the biases' (no decay, always_adapt off) are
    1. World 2 over loopback: both ranks end with the same parameters."""
    from kungfu_amd.exchange import NativeExchange
    outs = []
    for make in (loopback.rccl1_exchange, NativeExchange, lambda: None):
        ex = make()
        outs.append(_two_layer(ex, 1, 0))
        if ex is not None:
            ex.close()
    ps, ratios, _ = outs[0]
    assert all(np.isfinite(p).all() for p in ps)
    assert ratios[1] == 1.0 and ratios[3] == 1.0
    assert ratios[0] != 1.0 and ratios[2] != 1.0 and all(np.isfinite(ratios))
    for other, _, _ in outs[1:]:
        for a, b in zip(ps, other):
            assert _same(a, b)
    got = {}

    def body(rank, ex):
        got[rank] = _two_layer(ex, 2, rank)

    loopback.loop_ranks(2, body)
    for a, b in zip(got[0][0], got[1][0]):
        assert _same(a, b)
    assert got[0][1] == got[1][1]
    assert all(np.isfinite(p).all() for p in got[0][0])
