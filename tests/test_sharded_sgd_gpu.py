"""The sharded SGD step on the GPU, bit for bit against tests/sgd_ref.py: the
batched update kernel alone, the native exchange's reduce-scatter -> update
-> all-gather over the loopback transport, and ShardedSGDOptimizer end to
end."""
import ctypes

import numpy as np
import pytest
import torch

import loopback
import sgd_ref
import test_sharded_sgd as cpu

pytestmark = pytest.mark.gpu

# dt -> (numpy storage, torch dtype, numpy integer of the same width)
_DT = {"f32": (np.float32, torch.float32, np.int32),
       "f64": (np.float64, torch.float64, np.int64),
       "f16": (np.float16, torch.float16, np.int16),
       "bf16": (np.uint16, torch.bfloat16, np.int16)}


def _dev(a, dt):
    _, tt, it = _DT[dt]
    return torch.from_numpy(np.ascontiguousarray(a).view(it).copy()).cuda().view(tt)


def _host(t, dt):
    st, _, it = _DT[dt]
    return t.detach().cpu().contiguous().view(
        {np.int16: torch.int16, np.int32: torch.int32, np.int64: torch.int64}[it]).numpy().view(st).copy()


def _store(x, dt):
    """fp64 values -> dt's numpy representation."""
    if dt == "bf16":
        return sgd_ref.f32_to_bf16_bits(np.asarray(x, np.float32))
    return np.asarray(x).astype(_DT[dt][0])


def _random(dt, n, seed):
    return _store(np.random.default_rng(seed).standard_normal(n), dt)


def _isnan(a, dt):
    return np.isnan(sgd_ref.bf16_bits_to_f32(a)) if dt == "bf16" else np.isnan(a)


def _same(got, want, dt):
    """Bit equality; NaNs are compared by position."""
    gn, wn = _isnan(got, dt), _isnan(want, dt)
    if not np.array_equal(gn, wn):
        return False
    it = _DT[dt][2]
    return np.array_equal(got.view(it)[~gn], want.view(it)[~wn])


def _specials(dt):
    """(p, g, m) triples: signed zeros, +-inf, NaN, the largest finite value
    and subnormals in every role."""
    if dt == "bf16":
        one, big, sub = 0x3F80, 0x7F7F, 0x0001
        inf, nan, nz = 0x7F80, 0x7FC0, 0x8000
        neg = lambda b: b ^ 0x8000  # noqa: E731
        half = 0x7F00
    else:
        t = _DT[dt][0]
        one, big, sub = t(1), np.finfo(t).max, t(np.finfo(t).smallest_subnormal)
        inf, nan, nz = t(np.inf), t(np.nan), t(-0.0)
        neg = lambda b: -b  # noqa: E731
        half = big / t(2)
    z = nz ^ nz if dt == "bf16" else _DT[dt][0](0)
    trip = [(z, nz, z), (nz, nz, nz), (nz, z, nz), (inf, one, one), (one, inf, one),
            (one, one, neg(inf)), (inf, inf, one), (inf, neg(inf), inf), (nan, one, one),
            (one, nan, one), (one, one, nan), (big, big, big), (big, neg(big), half),
            (neg(big), big, big), (sub, sub, sub), (sub, z, neg(sub)), (neg(sub), sub, z),
            (one, sub, sub), (sub, one, big), (z, z, sub)]
    p, g, m = zip(*trip)
    return tuple(np.array(x, _DT[dt][0]) for x in (p, g, m))


SIZES = (1, 3, 1021, 4096, 100003)
N_ONES = 40  # with SIZES: more segments than one launch's table (32)


def _segments(dt):
    """[(p, g, m)] in dt's numpy form: SIZES, then N_ONES one-element
    segments. Specials sit at the start of the 4096 segment (a vector body),
    at the end of the 1021 one (its scalar tail and the vectors before it)
    and, one each, in the first one-element segments (scalar tails alone)."""
    sp, sg, sm = _specials(dt)
    k = len(sp)
    segs = []
    for i, n in enumerate(SIZES + (1,) * N_ONES):
        p, g, m = (_random(dt, n, 1000 * j + i) for j in (1, 2, 3))
        if n == 4096:
            p[:k], g[:k], m[:k] = sp, sg, sm
        elif n == 1021:
            p[-k:], g[-k:], m[-k:] = sp, sg, sm
        elif n == 1 and i >= len(SIZES) and i - len(SIZES) < k:
            j = i - len(SIZES)
            p[0], g[0], m[0] = sp[j], sg[j], sm[j]
        segs.append((p, g, m))
    return segs


@pytest.fixture(scope="module")
def segments():
    return {dt: _segments(dt) for dt in _DT}


@pytest.mark.parametrize("np_", [0, 1, 3, 8])
@pytest.mark.parametrize("dt", ["f32", "f16", "bf16", "f64"])
def test_kernel_bit_exact(segments, dt, np_):
    from kungfu_amd import ops
    segs = segments[dt]
    assert len(segs) > 32
    for row, (mu, damp, wd, nesterov) in enumerate(cpu.ROWS):
        for first in (True, False):
            # a hyper of its own per segment: the lr differs
            hs = [sgd_ref.hyper(0.1 / (1 + (i % 3)), mu, damp, wd, nesterov, first)
                  for i in range(len(segs))]
            ps = [_dev(p, dt) for p, _, _ in segs]
            gs = [_dev(g, dt) for _, g, _ in segs]
            ms = [_dev(m, dt) for _, _, m in segs] if mu else None
            ops.sgd_update_batch_(ps, gs, ms, hs, np_=np_)
            torch.cuda.synchronize()
            for i, ((p, g, m), h) in enumerate(zip(segs, hs)):
                wp, wm = sgd_ref.step(p, g, m if mu else None, dt, h, np_)
                where = (dt, np_, row, first, i, p.size)
                assert _same(_host(ps[i], dt), wp, dt), ("param",) + where
                assert _same(_host(gs[i], dt), g, dt), ("grad was written",) + where
                if mu:
                    assert _same(_host(ms[i], dt), wm, dt), ("momentum",) + where


# ---- native exchange over the loopback transport -----------------------------

NS = (1, 1021, 100003)
EX_HYPER = dict(momentum=0.9, nesterov=True, weight_decay=1e-2)
EX_LRS = (0.1, 0.05, 0.2)


def _grid(dt, n, seed):
    """Multiples of 1/4 in [-8, 8]: their sums over the ranks are exact in
    every order a transport may add in."""
    return _store(np.random.default_rng(seed).integers(-32, 33, n) / 4.0, dt)


def _exchange_reference(dt, world, counts):
    """Per bucket (params, momentum) after the steps, on the padded length."""
    from oracle import oracle
    out = []
    for b, (n, L) in enumerate(zip(NS, counts)):
        p = np.zeros(L, _DT[dt][0])
        p[:n] = _random(dt, n, 50 + b)
        m = None
        for s, lr in enumerate(EX_LRS):
            gr = []
            for r in range(world):
                g = np.zeros(L, _DT[dt][0])
                g[:n] = _grid(dt, n, 7000 + 100 * s + 10 * b + r)
                gr.append(g)
            avg = oracle.reduce_avg(gr, dt, world)
            p, m = sgd_ref.step(p, avg, m, dt, sgd_ref.hyper(lr, first=(s == 0), **EX_HYPER))
        out.append((p, m))
    return out


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("world", [2, 3, 4])
def test_native_exchange_sgd_step(world, dt):
    from kungfu_amd.collective import padded_count
    isz = np.dtype(_DT[dt][0]).itemsize
    counts = [padded_count(n, world, isz) for n in NS]
    want = _exchange_reference(dt, world, counts)
    got_p, got_m, times = {}, {}, {}

    def body(rank, ex):
        if world == 2 and rank == 0:  # counts % world: refused before any collective
            from kungfu_amd import _lib
            bad = (ctypes.c_size_t * 1)(3)
            x = torch.zeros(64, device="cuda")
            rc = ex.lib.kf_exchange_sgd_batch(ex._h, _lib.ptr_array([x.data_ptr()]),
                                              _lib.ptr_array([x.data_ptr()]), None, bad, 1,
                                              0x20408, _lib.sgd_hyper_array([sgd_ref.hyper(0.1)]),
                                              0, None)
            assert rc == 3
        ps, ms = [], []
        for b, (n, L) in enumerate(zip(NS, counts)):
            p = np.zeros(L, _DT[dt][0])
            p[:n] = _random(dt, n, 50 + b)
            ps.append(_dev(p, dt))
            ms.append(torch.zeros(L // world, dtype=_DT[dt][1], device="cuda"))
        ex.set_timing(True)
        for s, lr in enumerate(EX_LRS):
            gs = []
            for b, (n, L) in enumerate(zip(NS, counts)):
                g = np.zeros(L, _DT[dt][0])
                g[:n] = _grid(dt, n, 7000 + 100 * s + 10 * b + rank)
                gs.append(_dev(g, dt))
            hs = [sgd_ref.hyper(lr, first=(s == 0), **EX_HYPER)] * len(NS)
            ex.sgd_step_(ps, gs, ms, hs)
        torch.cuda.synchronize()
        times[rank] = ex.phase_times()
        ex.set_timing(False)
        got_p[rank] = [_host(p, dt) for p in ps]
        got_m[rank] = [_host(m, dt) for m in ms]

    loopback.loop_ranks(world, body)
    for r in range(world):
        for b, (wp, wm) in enumerate(want):
            assert _same(got_p[r][b], wp, dt), ("param", r, b)
            q = counts[b] // world
            assert _same(got_m[r][b], wm[r * q:(r + 1) * q], dt), ("momentum shard", r, b)
        t = times[r]
        assert t["calls"] == len(EX_LRS) and t["untimed_calls"] == 0, t
        assert t["epilogue"] > 0, t


# ---- the optimizer -----------------------------------------------------------

@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_optimizer_world2_bit_exact(dt):
    """tests/test_sharded_sgd.py's gloo model on the GPU over two loopback
    ranks; parameter 1 has no gradient on step 1 (updated as with zeros)."""
    world, skip = 2, (1, 1)
    want_p, want_m = cpu.reference_run(dt, world, skip=skip)
    got = {}

    def body(rank, ex):
        ps, opt = cpu.make_optimizer(dt, ex, device="cuda")
        cpu.run_steps(ps, opt, dt, world, rank, device="cuda", skip=skip)
        assert len(opt.state) == 0
        mb = opt.momentum_buffers()
        torch.cuda.synchronize()
        got[rank] = ([cpu.to_numpy(p, dt) for p in ps], [cpu.to_numpy(mb[p], dt) for p in ps])

    loopback.loop_ranks(world, body)
    for r in range(world):
        for j in range(len(want_p)):
            assert _same(got[r][0][j], want_p[j], dt), ("param", r, j)
            assert _same(got[r][1][j].reshape(-1), want_m[j], dt), ("momentum", r, j)


def test_optimizer_world1_native_and_default_same_bits():
    """No process group: a NativeExchange over a one-rank librccl
    communicator (the collectives run), a plain NativeExchange() (world 1 on
    the built-in transport: the update over the whole buckets) and the
    default collective.Exchange() give the same bits (and sgd_ref's)."""
    from kungfu_amd.exchange import NativeExchange
    dt = "f32"
    outs = []
    for make in (loopback.rccl1_exchange, NativeExchange, lambda: None):
        ex = make()
        ps, opt = cpu.make_optimizer(dt, ex, device="cuda")
        cpu.run_steps(ps, opt, dt, 1, 0, device="cuda")
        mb = opt.momentum_buffers()
        torch.cuda.synchronize()
        outs.append(([cpu.to_numpy(p, dt) for p in ps], [cpu.to_numpy(mb[p], dt) for p in ps]))
        if ex is not None:
            ex.close()
    want_p, want_m = cpu.reference_run(dt, 1)
    for j in range(len(want_p)):
        for got_p, got_m in outs:
            assert _same(got_p[j], want_p[j], dt), ("param", j)
            assert _same(got_m[j].reshape(-1), want_m[j], dt), ("momentum", j)
