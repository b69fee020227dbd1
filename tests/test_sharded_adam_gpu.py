"""The sharded Adam / AdamW step on the GPU, bit for bit against
tests/adam_ref.py: the batched update kernel alone, the native exchange's
reduce-scatter -> update -> all-gather over the loopback transport, and
ShardedAdamOptimizer end to end."""
import ctypes

import numpy as np
import pytest
import torch

import adam_ref
import loopback
import test_sharded_adam as cpu

pytestmark = pytest.mark.gpu

# dt -> (numpy storage, torch dtype, numpy integer of the same width)
_DT = {"f32": (np.float32, torch.float32, np.int32),
       "f64": (np.float64, torch.float64, np.int64),
       "bf16": (np.uint16, torch.bfloat16, np.int16)}

# kf_adam.hip's launch shape, pinned to the source by tests/test_sharded_adam.py
ADAM_SEG, BLOCK, UNROLL = cpu.ADAM_SEG, cpu.BLOCK, cpu.UNROLL


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
        return adam_ref.f32_to_bf16_bits(np.asarray(x, np.float32))
    return np.asarray(x).astype(_DT[dt][0])


def _random(dt, n, seed):
    return _store(np.random.default_rng(seed).standard_normal(n), dt)


# dt -> (exponent of the smallest subnormal, exponent of the largest binade)
_EXPONENTS = {"f32": (-149, 127), "f64": (-1074, 1023), "bf16": (-133, 127)}


def _random_v(dt, n, seed):
    """exp_avg_sq: squares of log-uniform values, over every binade of the
    type from below its smallest subnormal (zeros) to its largest; every
    seventh element of a segment of more than 8 is a zero or a subnormal."""
    lo, hi = _EXPONENTS[dt]
    rng = np.random.default_rng(seed)
    with np.errstate(under="ignore", over="ignore"):
        x = np.exp2(rng.uniform((lo - 2) / 2.0, hi / 2.0, n))
        v = _store(x * x, dt)
        if n > 8:
            sub = _store(np.exp2(rng.uniform(lo, lo + 6, n)), dt)
            v[::7] = sub[::7]
            v[::21] = 0
    return v


def _isnan(a, dt):
    return np.isnan(adam_ref.bf16_bits_to_f32(a)) if dt == "bf16" else np.isnan(a)


def _same(got, want, dt):
    """Bit equality; NaNs are compared by position."""
    gn, wn = _isnan(got, dt), _isnan(want, dt)
    if not np.array_equal(gn, wn):
        return False
    it = _DT[dt][2]
    return np.array_equal(got.view(it)[~gn], want.view(it)[~wn])


def _specials(dt):
    """(p, g, m, v) quadruples: signed zeros, +-inf, NaN, the largest finite
    value and subnormals in every role, and negative v."""
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
    quad = [(z, nz, z, z), (nz, nz, nz, z), (nz, z, nz, nz), (z, z, z, nz),
            (inf, one, one, one), (one, inf, one, one), (one, one, neg(inf), one),
            (one, one, one, inf), (inf, inf, one, inf), (inf, neg(inf), inf, inf),
            (nan, one, one, one), (one, nan, one, one), (one, one, nan, one), (one, one, one, nan),
            (big, big, big, big), (big, neg(big), half, big), (neg(big), big, big, sub),
            (big, z, big, z), (neg(big), z, big, sub),
            (sub, sub, sub, sub), (sub, z, neg(sub), z), (neg(sub), sub, z, sub),
            (one, sub, sub, z), (sub, one, big, one), (z, z, sub, z), (one, z, one, sub),
            (one, one, one, neg(one)), (one, z, one, neg(sub)), (one, one, one, neg(inf)),
            (one, z, one, neg(big))]
    return tuple(np.array(x, _DT[dt][0]) for x in zip(*quad))


SIZES = (1, 3, 1021, 4096, 100003)
N_ONES = ADAM_SEG + 8  # with SIZES: more one-element segments than one launch's table


def _fill(dt, sizes):
    return [(_random(dt, n, 1000 + i), _random(dt, n, 2000 + i), _random(dt, n, 3000 + i),
             _random_v(dt, n, 4000 + i)) for i, n in enumerate(sizes)]


def _segments(dt):
    """[(p, g, m, v)] in dt's numpy form: SIZES, then N_ONES one-element
    segments. Specials sit at the start of the 4096 segment (a vector body),
    at the end of the 1021 one (its scalar tail and the vectors before it)
    and, one each, in the one-element segments (scalar tails alone)."""
    sp = _specials(dt)
    k = len(sp[0])
    assert k <= N_ONES
    segs = _fill(dt, SIZES + (1,) * N_ONES)
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


def _rows_segments(dt):
    """Three equal segments of two tiles and a 3-element tail: the rows grid."""
    e = 16 // np.dtype(_DT[dt][0]).itemsize
    n = 2 * BLOCK * UNROLL * e + 3
    blocks = [max(-(-(n // e) // (BLOCK * UNROLL)), 1)] * 3
    assert len(blocks) > 1 and max(blocks) * len(blocks) <= 2 * sum(blocks)  # launch_adam's `rows`
    return _fill(dt, (n,) * 3)


@pytest.fixture(scope="module")
def segments():
    return {dt: (_segments(dt), _rows_segments(dt)) for dt in _DT}


@pytest.mark.parametrize("np_", [0, 1, 3, 8])
@pytest.mark.parametrize("dt", ["f32", "bf16", "f64"])
def test_kernel_bit_exact(segments, dt, np_):
    from kungfu_amd import ops
    for which, segs in enumerate(segments[dt]):
        assert which == 1 or len(segs) > ADAM_SEG + len(SIZES)
        base = [[_dev(a, dt) for a in seg] for seg in segs]
        for row, (wd, decoupled) in enumerate(cpu.ROWS):
            for step in (1, 7):
                # a hyper of its own per segment: the lr differs
                hs = [adam_ref.hyper(1e-2 / (1 + (i % 3)), weight_decay=wd, decoupled=decoupled,
                                     step=step) for i in range(len(segs))]
                ps, gs, ms, vs = ([seg[j].clone() for seg in base] for j in range(4))
                ops.adam_update_batch_(ps, gs, ms, vs, hs, np_=np_)
                torch.cuda.synchronize()
                for i, (seg, h) in enumerate(zip(segs, hs)):
                    wp, wm, wv = adam_ref.step(*seg, dt, h, np_)
                    where = (dt, np_, which, row, step, i, seg[0].size)
                    assert _same(_host(ps[i], dt), wp, dt), ("param",) + where
                    assert _same(_host(gs[i], dt), seg[1], dt), ("grad was written",) + where
                    assert _same(_host(ms[i], dt), wm, dt), ("exp_avg",) + where
                    assert _same(_host(vs[i], dt), wv, dt), ("exp_avg_sq",) + where


def test_f16_is_refused():
    from kungfu_amd import _lib, ops
    x = [torch.zeros(8, dtype=torch.float16, device="cuda") for _ in range(4)]
    with pytest.raises(_lib.KungFuAMDError, match="KF_ERR_DTYPE"):
        ops.adam_update_batch_([x[0]], [x[1]], [x[2]], [x[3]], [adam_ref.hyper(1e-3)])


# ---- native exchange over the loopback transport -----------------------------

NS = (1, 1021, 100003)
EX_LRS = (1e-2, 5e-3, 2e-2)


def _ex_hyper(dt, lr, step):
    """Adam's L2 decay for f32, AdamW's for bf16."""
    return adam_ref.hyper(lr, weight_decay=1e-2, decoupled=(dt == "bf16"), step=step)


def _grid(dt, n, seed):
    """Multiples of 1/4 in [-8, 8]: their sums over the ranks are exact in
    every order a transport may add in."""
    return _store(np.random.default_rng(seed).integers(-32, 33, n) / 4.0, dt)


def _exchange_reference(dt, world, counts):
    """Per bucket (params, exp_avg, exp_avg_sq) after the steps, on the
    padded length."""
    from oracle import oracle
    out = []
    for b, (n, L) in enumerate(zip(NS, counts)):
        p = np.zeros(L, _DT[dt][0])
        p[:n] = _random(dt, n, 50 + b)
        m, v = np.zeros(L, _DT[dt][0]), np.zeros(L, _DT[dt][0])
        for s, lr in enumerate(EX_LRS):
            gr = []
            for r in range(world):
                g = np.zeros(L, _DT[dt][0])
                g[:n] = _grid(dt, n, 7000 + 100 * s + 10 * b + r)
                gr.append(g)
            avg = oracle.reduce_avg(gr, dt, world)
            p, m, v = adam_ref.step(p, avg, m, v, dt, _ex_hyper(dt, lr, s + 1))
        out.append((p, m, v))
    return out


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("world", [2, 3, 4])
def test_native_exchange_adam_step(world, dt):
    from kungfu_amd.collective import padded_count
    isz = np.dtype(_DT[dt][0]).itemsize
    counts = [padded_count(n, world, isz) for n in NS]
    want = _exchange_reference(dt, world, counts)
    got_p, got_m, got_v, times = {}, {}, {}, {}

    def body(rank, ex):
        if world == 2 and rank == 0:  # counts % world: refused before any collective
            from kungfu_amd import _lib
            bad = (ctypes.c_size_t * 1)(3)
            x = torch.zeros(64, device="cuda")
            one = _lib.ptr_array([x.data_ptr()])
            rc = ex.lib.kf_exchange_adam_batch(ex._h, one, one, one, one, bad, 1, 0x20408,
                                               _lib.adam_hyper_array([adam_ref.hyper(1e-3)]),
                                               0, None)
            assert rc == 3
        ps, ms, vs = [], [], []
        for b, (n, L) in enumerate(zip(NS, counts)):
            p = np.zeros(L, _DT[dt][0])
            p[:n] = _random(dt, n, 50 + b)
            ps.append(_dev(p, dt))
            ms.append(torch.zeros(L // world, dtype=_DT[dt][1], device="cuda"))
            vs.append(torch.zeros(L // world, dtype=_DT[dt][1], device="cuda"))
        ex.set_timing(True)
        for s, lr in enumerate(EX_LRS):
            gs = []
            for b, (n, L) in enumerate(zip(NS, counts)):
                g = np.zeros(L, _DT[dt][0])
                g[:n] = _grid(dt, n, 7000 + 100 * s + 10 * b + rank)
                gs.append(_dev(g, dt))
            ex.adam_step_(ps, gs, ms, vs, [_ex_hyper(dt, lr, s + 1)] * len(NS))
        torch.cuda.synchronize()
        times[rank] = ex.phase_times()
        ex.set_timing(False)
        got_p[rank] = [_host(p, dt) for p in ps]
        got_m[rank] = [_host(m, dt) for m in ms]
        got_v[rank] = [_host(v, dt) for v in vs]

    loopback.loop_ranks(world, body)
    for r in range(world):
        for b, (wp, wm, wv) in enumerate(want):
            assert _same(got_p[r][b], wp, dt), ("param", r, b)
            q = counts[b] // world
            assert _same(got_m[r][b], wm[r * q:(r + 1) * q], dt), ("exp_avg shard", r, b)
            assert _same(got_v[r][b], wv[r * q:(r + 1) * q], dt), ("exp_avg_sq shard", r, b)
        t = times[r]
        assert t["calls"] == len(EX_LRS) and t["untimed_calls"] == 0, t
        assert t["epilogue"] > 0, t


# ---- the optimizer -----------------------------------------------------------

def _state_arrays(opt, ps, dt):
    sb = opt.state_buffers()
    assert all(sb[p]["step"] == cpu.STEPS for p in ps)
    return ([cpu.to_numpy(sb[p]["exp_avg"], dt) for p in ps],
            [cpu.to_numpy(sb[p]["exp_avg_sq"], dt) for p in ps])


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_optimizer_world2_bit_exact(dt):
    """tests/test_sharded_adam.py's gloo model on the GPU over two loopback
    ranks; parameter 1 has no gradient on step 1 (updated as with zeros)."""
    world, skip = 2, (1, 1)
    want_p, want_m, want_v = cpu.reference_run(dt, world, skip=skip)
    got = {}

    def body(rank, ex):
        ps, opt = cpu.make_optimizer(dt, ex, device="cuda")
        cpu.run_steps(ps, opt, dt, world, rank, device="cuda", skip=skip)
        assert len(opt.state) == 0
        m, v = _state_arrays(opt, ps, dt)
        torch.cuda.synchronize()
        got[rank] = ([cpu.to_numpy(p, dt) for p in ps], m, v)

    loopback.loop_ranks(world, body)
    for r in range(world):
        for j in range(len(want_p)):
            assert _same(got[r][0][j], want_p[j], dt), ("param", r, j)
            assert _same(got[r][1][j].reshape(-1), want_m[j], dt), ("exp_avg", r, j)
            assert _same(got[r][2][j].reshape(-1), want_v[j], dt), ("exp_avg_sq", r, j)


def test_optimizer_world1_native_and_default_same_bits():
    """No process group: a NativeExchange over a one-rank librccl
    communicator (the collectives run), a plain NativeExchange() (world 1 on
    the built-in transport: the update over the whole buckets) and the
    default collective.Exchange() give the same bits (and adam_ref's)."""
    from kungfu_amd.exchange import NativeExchange
    dt = "f32"
    outs = []
    for make in (loopback.rccl1_exchange, NativeExchange, lambda: None):
        ex = make()
        ps, opt = cpu.make_optimizer(dt, ex, device="cuda")
        cpu.run_steps(ps, opt, dt, 1, 0, device="cuda")
        m, v = _state_arrays(opt, ps, dt)
        torch.cuda.synchronize()
        outs.append(([cpu.to_numpy(p, dt) for p in ps], m, v))
        if ex is not None:
            ex.close()
    want_p, want_m, want_v = cpu.reference_run(dt, 1)
    for j in range(len(want_p)):
        for got_p, got_m, got_v in outs:
            assert _same(got_p[j], want_p[j], dt), ("param", j)
            assert _same(got_m[j].reshape(-1), want_m[j], dt), ("exp_avg", j)
            assert _same(got_v[j].reshape(-1), want_v[j], dt), ("exp_avg_sq", j)
