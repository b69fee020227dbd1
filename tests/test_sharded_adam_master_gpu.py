"""The sharded Adam / AdamW step with fp32 master weights on the GPU, bit for
bit against tests/adam_master_ref.py: the batched update kernel alone, its
narrowing on a grid of ties, the native exchange's reduce-scatter -> update ->
all-gather over the loopback transport, and
ShardedAdamOptimizer(master_weights=True) end to end."""
import ctypes

import numpy as np
import pytest
import torch

import adam_master_ref
import adam_ref
import loopback
import sweep16
import test_sharded_adam_gpu as gpu
import test_sharded_adam_master as cpu

pytestmark = pytest.mark.gpu

# dt -> (torch dtype, KungFu_Datatype)
_DT16 = {"bf16": (torch.bfloat16, cpu.BF16), "f16": (torch.float16, cpu.F16)}

# kf_adam_master.hip's launch shape, pinned to the source by
# tests/test_sharded_adam_master.py
MASTER_SEG, BLOCK, ELTS, UNROLL = cpu.MASTER_SEG, cpu.BLOCK, cpu.ELTS, cpu.UNROLL


def _dev16(a, dt):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int16).copy()).cuda().view(_DT16[dt][0])


def _host16(t, dt):
    a = t.detach().cpu().contiguous().view(torch.int16).numpy().copy()
    return a.view(adam_master_ref.STORAGE[dt])


def _dev32(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32).copy()).cuda()


def _host32(t):
    return t.detach().cpu().contiguous().numpy().copy()


def _store16(x, dt):
    return adam_master_ref.narrow(np.asarray(x, np.float32), dt)


def _same16(got, want, dt):
    """Bit equality; NaNs are compared by position."""
    gn = np.isnan(adam_master_ref.widen(got, dt))
    wn = np.isnan(adam_master_ref.widen(want, dt))
    return np.array_equal(gn, wn) and np.array_equal(got.view(np.uint16)[~gn],
                                                     want.view(np.uint16)[~wn])


def _same32(got, want):
    return gpu._same(got, want, "f32")


def _g_specials(dt):
    """16-bit gradients: signed zeros, +-inf, NaN, the largest finite values
    and the smallest and largest subnormals, as bit patterns."""
    if dt == "bf16":
        bits = [0x0000, 0x8000, 0x7F80, 0xFF80, 0x7FC0, 0x7F7F, 0xFF7F, 0x0001, 0x8001, 0x007F, 0x807F]
    else:
        bits = [0x0000, 0x8000, 0x7C00, 0xFC00, 0x7E00, 0x7BFF, 0xFBFF, 0x0001, 0x8001, 0x03FF, 0x83FF]
    return np.array(bits, np.uint16).view(adam_master_ref.STORAGE[dt])


# tails of 1, 3, 1, 2, 1, 0 and 3 elements below the unit of 4; 1021 is a
# ragged tile alone, 4096 one full tile, 100003 full tiles and a ragged one
SIZES = (1, 3, 5, 6, 1021, 4096, 100003)
N_ONES = MASTER_SEG + 8  # with SIZES: more one-element segments than one launch's table


def _fill(dt, sizes):
    """[(g16, master, m, v)]: standard-normal g, master and m; v over every
    fp32 binade with zeros and subnormals (tests/test_sharded_adam_gpu.py)."""
    return [(_store16(np.random.default_rng(2000 + i).standard_normal(n), dt),
             gpu._random("f32", n, 1000 + i), gpu._random("f32", n, 3000 + i),
             gpu._random_v("f32", n, 4000 + i)) for i, n in enumerate(sizes)]


def _segments(dt):
    """SIZES, then N_ONES one-element segments. The special gradients sit at
    the start of the 4096 segment (a vector body), at the end of the 1021, 6
    and 100003 ones (their scalar tails and the units before them) and, one
    each, in the one-element segments (scalar tails alone)."""
    sp = _g_specials(dt)
    k = len(sp)
    assert k <= N_ONES
    segs = _fill(dt, SIZES + (1,) * N_ONES)
    for i, seg in enumerate(segs):
        g, n = seg[0], seg[0].size
        if n == 4096:
            g[:k] = sp
        elif n in (1021, 100003):
            g[-k:] = sp
            g[-2 * k:-k] = sp[::-1]  # every special in another lane of the unit
        elif n == 6:
            g[:] = sp[[2, 4, 5, 7, 1, 3]]
        elif n == 1 and i >= len(SIZES) and i - len(SIZES) < k:
            g[0] = sp[i - len(SIZES)]
    return segs


def _rows_segments(dt):
    """Three equal segments of two tiles and a 3-element tail: the rows grid."""
    n = 2 * BLOCK * UNROLL * ELTS + 3
    blocks = [max(-(-(n // ELTS) // (BLOCK * UNROLL)), 1)] * 3
    assert len(blocks) > 1 and max(blocks) * len(blocks) <= 2 * sum(blocks)  # launch_master's `rows`
    return _fill(dt, (n,) * 3)


@pytest.fixture(scope="module")
def segments():
    return {dt: (_segments(dt), _rows_segments(dt)) for dt in _DT16}


@pytest.mark.parametrize("np_", [0, 1, 3, 8])
@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_kernel_bit_exact(segments, dt, np_):
    from kungfu_amd import ops
    for which, segs in enumerate(segments[dt]):
        assert which == 1 or len(segs) > MASTER_SEG + len(SIZES)
        base_g = [_dev16(seg[0], dt) for seg in segs]
        base_f = [[_dev32(a) for a in seg[1:]] for seg in segs]
        for row, (wd, decoupled) in enumerate(cpu.ROWS):
            for step in (1, 7):
                hs = [adam_ref.hyper(1e-2 / (1 + (i % 3)), weight_decay=wd, decoupled=decoupled,
                                     step=step) for i in range(len(segs))]
                gs = [g.clone() for g in base_g]
                ws, ms, vs = ([f[j].clone() for f in base_f] for j in range(3))
                # the old parameter values are never read: any bits will do
                ps = [torch.full_like(g, 7.0) for g in gs]
                ops.adam_master_update_batch_(ps, gs, ws, ms, vs, hs, np_=np_)
                torch.cuda.synchronize()
                for i, (seg, h) in enumerate(zip(segs, hs)):
                    wp, ww, wm, wv = adam_master_ref.step(seg[1], seg[0], seg[2], seg[3], dt, h, np_)
                    where = (dt, np_, which, row, step, i, seg[0].size)
                    assert _same32(_host32(ws[i]), ww), ("master",) + where
                    assert _same16(_host16(ps[i], dt), wp, dt), ("param",) + where
                    assert _same16(_host16(gs[i], dt), seg[0], dt), ("grad was written",) + where
                    assert _same32(_host32(ms[i]), wm), ("exp_avg",) + where
                    assert _same32(_host32(vs[i]), wv), ("exp_avg_sq",) + where


def test_other_dtypes_are_refused():
    from kungfu_amd import _lib
    lib = _lib.load()
    x = [torch.zeros(8, device="cuda") for _ in range(5)]
    one = [_lib.ptr_array([t.data_ptr()]) for t in x]
    cnt = (ctypes.c_size_t * 1)(8)
    h = _lib.adam_hyper_array([adam_ref.hyper(1e-3)])
    for dt in (cpu.F32, cpu.F64):
        assert lib.kf_adam_master_update_batch(*one, cnt, 1, dt, 0, h, None) == cpu.ERR_DTYPE


# ---- the narrowing ------------------------------------------------------------

# the grid of fp32 masters around every rounding boundary of dt, shared with
# the LAMB apply pass's narrowing test (tests/test_sweep16_gpu.py)
_narrowing_grid = sweep16.narrowing_grid


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_narrowing_grid(dt):
    """Zero g, m and v: the master passes through unchanged (p + (-0)), both
    signs of zero included, and params16 is its RNE narrowing."""
    from kungfu_amd import ops
    grid = _narrowing_grid(dt)
    assert grid.size % ELTS == 3
    want = adam_master_ref.narrow(grid, dt)
    # the restatement agrees that this is a pass-through
    h = adam_ref.hyper(1e-3)
    z = np.zeros(grid.size, np.float32)
    rp, rw, rm, rv = adam_master_ref.step(grid, adam_master_ref.narrow(z, dt), z, z, dt, h)
    assert _same32(rw, grid) and _same16(rp, want, dt) and not rm.any() and not rv.any()
    # one long segment (vector bodies and a tail), then the first 64 and the
    # last 64 patterns as one-element segments (scalar tails alone)
    near = np.float32([1.0 + 2.0 ** -8, 1.0 + 2.0 ** -11, 65520.0, 65519.996, 2.0 ** -25, 2.0 ** -140])
    ones = np.concatenate([np.arange(64), np.arange(grid.size - 64, grid.size),
                           np.flatnonzero(grid == 0), np.flatnonzero(np.isin(np.abs(grid), near)),
                           np.flatnonzero(~np.isfinite(grid))])
    masters = [grid] + [grid[i:i + 1] for i in ones]
    ws = [_dev32(a) for a in masters]
    ps = [torch.full((a.size,), 7.0, dtype=_DT16[dt][0], device="cuda") for a in masters]
    gs, ms, vs = ([torch.zeros(a.size, dtype=d, device="cuda") for a in masters]
                  for d in (_DT16[dt][0], torch.float32, torch.float32))
    ops.adam_master_update_batch_(ps, gs, ws, ms, vs, [h] * len(masters))
    torch.cuda.synchronize()
    for i, a in enumerate(masters):
        got = _host16(ps[i], dt)
        w16 = adam_master_ref.narrow(a, dt)
        bad = np.flatnonzero(got.view(np.uint16) != w16.view(np.uint16))
        bad = [j for j in bad if not np.isnan(a[j])]
        assert not bad, (dt, i, [(float(a[j]), hex(int(got.view(np.uint16)[j])),
                                  hex(int(w16.view(np.uint16)[j]))) for j in bad[:8]])
        assert _same16(got, w16, dt), (dt, i)
        assert _same32(_host32(ws[i]), a), ("master changed", dt, i)
        assert not _host32(ms[i]).any() and not _host32(vs[i]).any()
    # -0 is preserved, in the vector body and alone
    neg0 = np.flatnonzero((grid == 0) & np.signbit(grid))
    assert neg0.size and all(_host16(ps[0], dt).view(np.uint16)[neg0] == 0x8000)


# ---- native exchange over the loopback transport -----------------------------

NS = gpu.NS
EX_LRS = gpu.EX_LRS
# Both 16-bit types take the all-to-all and the rank-order fold under "auto"
# (kf_exchange.hip resolve_algo): the fold rounds the average to 16 bits and
# the update divides by nothing. The loopback transport has no 16-bit
# reduce-scatter; the update's own / world after a reduce-scatter runs through
# librccl at world 1 below (test_optimizer_world1_...), and test_kernel_bit_exact
# covers np = 1, 3 and 8.


def _ex_hyper(dt, lr, step):
    """AdamW's decay for bf16, Adam's L2 for f16."""
    return adam_ref.hyper(lr, weight_decay=1e-2, decoupled=(dt == "bf16"), step=step)


def _grid16(dt, n, seed):
    """Multiples of 1/4 in [-8, 8]: their sums over the ranks are exact in
    every order a transport may add in, in either 16-bit format."""
    return _store16(np.random.default_rng(seed).integers(-32, 33, n) / 4.0, dt)


def _bucket(dt, n, L, seed):
    p = np.zeros(L, np.float32)
    p[:n] = np.random.default_rng(seed).standard_normal(n)
    return _store16(p, dt)


def _exchange_reference(dt, world, counts):
    """Per bucket (params16, master, exp_avg, exp_avg_sq) after the steps, on
    the padded length: the cross-rank sum is rounded to 16 bits exactly where
    the exchange rounds it."""
    from oracle import oracle
    out = []
    for b, (n, L) in enumerate(zip(NS, counts)):
        p = _bucket(dt, n, L, 50 + b)
        w = adam_master_ref.widen(p, dt)
        m, v = np.zeros(L, np.float32), np.zeros(L, np.float32)
        for s, lr in enumerate(EX_LRS):
            gr = []
            for r in range(world):
                g = np.zeros(L, np.float32)
                g[:n] = adam_master_ref.widen(_grid16(dt, n, 7000 + 100 * s + 10 * b + r), dt)
                gr.append(_store16(g, dt))
            g16 = oracle.reduce_avg(gr, dt, world)
            p, w, m, v = adam_master_ref.step(w, g16, m, v, dt, _ex_hyper(dt, lr, s + 1))
        out.append((p, w, m, v))
    return out


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("world", [2, 3, 4])
def test_native_exchange_adam_master_step(world, dt):
    from kungfu_amd.collective import padded_count
    counts = [padded_count(n, world, 2) for n in NS]
    want = _exchange_reference(dt, world, counts)
    got = {}
    times = {}

    def body(rank, ex):
        if world == 2 and rank == 0:  # refused before any collective is queued
            from kungfu_amd import _lib
            x = torch.zeros(64, device="cuda")
            one, null = _lib.ptr_array([x.data_ptr()]), _lib.ptr_array([0])
            h = _lib.adam_hyper_array([adam_ref.hyper(1e-3)])
            call = ex.lib.kf_exchange_adam_master_batch
            odd, even = (ctypes.c_size_t * 1)(3), (ctypes.c_size_t * 1)(32)
            assert call(ex._h, one, one, one, one, one, odd, 1, _DT16[dt][1], h, 0, None) == 3
            assert call(ex._h, one, one, null, one, one, even, 1, _DT16[dt][1], h, 0, None) == 3
            assert b"master shard" in ex.lib.kf_exchange_last_error()
            assert call(ex._h, one, one, None, one, one, even, 1, _DT16[dt][1], h, 0, None) == 3
            assert call(ex._h, one, one, one, one, one, even, 1, cpu.F32, h, 0, None) == 1
        ps, ws, ms, vs = [], [], [], []
        for b, (n, L) in enumerate(zip(NS, counts)):
            p = _bucket(dt, n, L, 50 + b)
            q = L // world
            ps.append(_dev16(p, dt))
            ws.append(_dev32(adam_master_ref.widen(p, dt)[rank * q:(rank + 1) * q]))
            ms.append(torch.zeros(q, device="cuda"))
            vs.append(torch.zeros(q, device="cuda"))
        ex.set_timing(True)
        for s, lr in enumerate(EX_LRS):
            gs = []
            for b, (n, L) in enumerate(zip(NS, counts)):
                g = np.zeros(L, np.float32)
                g[:n] = adam_master_ref.widen(_grid16(dt, n, 7000 + 100 * s + 10 * b + rank), dt)
                gs.append(_dev16(_store16(g, dt), dt))
            ex.adam_master_step_(ps, gs, ws, ms, vs, [_ex_hyper(dt, lr, s + 1)] * len(NS))
        torch.cuda.synchronize()
        times[rank] = ex.phase_times()
        ex.set_timing(False)
        got[rank] = ([_host16(p, dt) for p in ps], [_host32(w) for w in ws],
                     [_host32(m) for m in ms], [_host32(v) for v in vs])

    loopback.loop_ranks(world, body)
    for r in range(world):
        for b, (wp, ww, wm, wv) in enumerate(want):
            q = counts[b] // world
            assert _same16(got[r][0][b], wp, dt), ("param", r, b)
            assert _same16(got[r][0][b], got[0][0][b], dt), ("ranks differ", r, b)
            assert _same32(got[r][1][b], ww[r * q:(r + 1) * q]), ("master shard", r, b)
            assert _same32(got[r][2][b], wm[r * q:(r + 1) * q]), ("exp_avg shard", r, b)
            assert _same32(got[r][3][b], wv[r * q:(r + 1) * q]), ("exp_avg_sq shard", r, b)
            # the invariant: the gathered parameters are the narrowed masters
            mine = got[r][0][b][r * q:(r + 1) * q]
            assert _same16(mine, adam_master_ref.narrow(got[r][1][b], dt), dt), ("invariant", r, b)
        t = times[r]
        assert t["calls"] == len(EX_LRS) and t["untimed_calls"] == 0, t
        assert t["epilogue"] > 0, t


# ---- the optimizer -----------------------------------------------------------

def _collect(ps, opt):
    sb = opt.state_buffers()
    torch.cuda.synchronize()
    return ps, {p: {k: (t.cpu() if torch.is_tensor(t) else t) for k, t in b.items()}
                for p, b in sb.items()}


def test_optimizer_world2_bit_exact():
    """tests/test_sharded_adam_master.py's model (a bf16 group and an f32
    group) on the GPU over two loopback ranks; parameter 1 has no gradient on
    step 1 (updated as with zeros)."""
    world, skip = 2, (1, 1)
    want = cpu.reference_run(world, skip=skip)
    got = {}

    def body(rank, ex):
        ps, opt = cpu.make_optimizer(ex, device="cuda")
        cpu.run_steps(ps, opt, world, rank, device="cuda", skip=skip)
        assert len(opt.state) == 0
        got[rank] = _collect(ps, opt)

    loopback.loop_ranks(world, body)
    for r in range(world):
        cpu.check_against_reference(*got[r], want)


@pytest.mark.parametrize("dt16", ["bf16", "f16"])
def test_optimizer_world1_native_and_default_same_bits(dt16):
    """A NativeExchange over a one-rank librccl communicator under "auto"
    (all-to-all and fold) and under "rs" (reduce-scatter, the update divides
    by the world itself), a plain NativeExchange() (the update over the whole
    buckets) and the default collective.Exchange() give the same bits, and
    adam_master_ref's."""
    from kungfu_amd.exchange import NativeExchange
    want = cpu.reference_run(1, dt16=dt16)
    rccl1_rs = lambda: loopback.rccl1_exchange(algo="rs")  # noqa: E731  reduce-scatter, then / 1
    for make in (loopback.rccl1_exchange, rccl1_rs, NativeExchange, lambda: None):
        ex = make()
        ps, opt = cpu.make_optimizer(ex, device="cuda", dt16=dt16)
        cpu.run_steps(ps, opt, 1, 0, device="cuda", dt16=dt16)
        cpu.check_against_reference(*_collect(ps, opt), want, dt16=dt16)
        if ex is not None:
            ex.close()


def test_small_updates_reach_the_parameter():
    """tests/test_sharded_adam_master.py's motivating case on the device:
    p = 1.0 in bf16, g = 1.0, lr = 1e-3, 50 steps. With master weights the
    parameter ends at 0.94921875; without, it never leaves 1.0."""
    from kungfu_amd.optimizers import ShardedAdamOptimizer
    end = {}
    for flag in (True, False):
        p = torch.nn.Parameter(torch.ones(13, dtype=torch.bfloat16, device="cuda"))
        opt = ShardedAdamOptimizer(torch.optim.Adam([p], lr=1e-3), master_weights=flag)
        for _ in range(50):
            p.grad = torch.ones_like(p)
            opt.step()
        torch.cuda.synchronize()
        end[flag] = p.detach().float().cpu()
    assert torch.equal(end[True], torch.full((13,), 0.94921875)), end[True]
    assert torch.equal(end[False], torch.ones(13)), end[False]
