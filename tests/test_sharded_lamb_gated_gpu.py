"""The LAMB step under a gate on the GPU, bit for bit against
tests/lamb_gated_ref.py: the two gated moments kernels (every dtype, one rows
grid each, the no-op gate against the ungated kernels), the skip on pre-filled
buffers, the gated trust kernel and apply run, the whole step over the
loopback transport and a one-rank librccl communicator, and
ShardedLAMBOptimizer(gate=...) end to end on a two-layer f16 model. Data and
helpers are tests/test_sharded_adam_gpu.py's, tests/test_sharded_lamb_gpu.py's
and tests/test_large_launch_gpu.py's."""
import numpy as np
import pytest
import torch

import lamb_gated_ref as gref
import lamb_ref
import large_launch as ll
import loopback
import step_gate_ref
import test_large_launch_gpu as tl
import test_sharded_adam_gated as gated
import test_sharded_adam_gpu as ag
import test_sharded_lamb_gated as cg
import test_sharded_lamb_gpu as lg

pytestmark = pytest.mark.gpu

LAMB_SEG, LAMB_MASTER_SEG = lg.LAMB_SEG, lg.LAMB_MASTER_SEG
BETAS = (0.9, 0.999)
MULS = (1.0, 2.0 ** -16, 0.37)
GUARD = 24  # elements beyond every count that must stay as they were
_NP = {"f32": np.float32, "f64": np.float64, "bf16": np.uint16, "f16": np.uint16}
_TORCH = {"f32": torch.float32, "f64": torch.float64, "bf16": torch.bfloat16, "f16": torch.float16}
_INT = {2: (np.int16, torch.int16), 4: (np.int32, torch.int32), 8: (np.int64, torch.int64)}


def _hyper(wd):
    """The hyper of a gated call: one for every segment, no step."""
    return {"lr": 1e-2, "betas": BETAS, "eps": 1e-6, "weight_decay": wd}


def _gate_state(mul, step, skip=0):
    """(reference gate, reference state, device gate, device states) as a
    verdict with lr = 1 would leave them after `step` applied steps, with
    grad_mul = mul; the kernels read group 1 of two."""
    from kungfu_amd import ops
    g = dict(gref.new_gate(), skip=skip, grad_mul=np.float32(mul))
    st = gref.scalars_of({"lr": 1e-2, "betas": BETAS, "step": step})
    dg, ds = ops.new_step_gate("cuda"), ops.new_step_states("cuda", 2)
    gated.write_gate(dg, g)
    gated.write_states(ds, [gref.new_state(), st])
    return g, st, dg, ds


class Flat:
    """One role's segments in one allocation: every segment starts on a 16-byte
    boundary and has at least GUARD elements of a fill pattern after it.
    arrays[i] None: counts[i] elements of the pattern (an output)."""

    def __init__(self, arrays, counts, dt, fill_seed=None):
        self.dt, self.counts = dt, list(counts)
        t = np.dtype(_NP[dt])
        per16 = 16 // t.itemsize
        self.offs, cur = [], per16
        for n in counts:
            self.offs.append(cur)
            cur = -(-(cur + n + GUARD) // per16) * per16
        if fill_seed is None:
            self.host = np.full(cur, 0x4321 if t.kind == "u" else 7.0, t)
        else:  # distinct bytes per buffer
            self.host = np.random.default_rng(fill_seed).integers(
                0, 256, cur * t.itemsize, dtype=np.uint8).view(t).copy()
        for a, o in zip(arrays, self.offs):
            if a is not None:
                self.host[o:o + a.size] = a
        it = _INT[t.itemsize]
        self.t = torch.from_numpy(self.host.view(it[0]).copy()).cuda().view(_TORCH[dt])
        assert self.t.data_ptr() % 16 == 0

    def views(self):
        return [self.t[o:o + n] for o, n in zip(self.offs, self.counts)]

    def got(self):
        t = np.dtype(_NP[self.dt])
        return self.t.detach().cpu().view(_INT[t.itemsize][1]).numpy().view(t).copy()

    def check(self, want, what):
        """Segment i holds want[i] bit for bit (NaNs by position; want None:
        nothing was written) and every other element is as it was."""
        exp = self.host.copy()
        for w, o, n in zip(want or [], self.offs, self.counts):
            assert w.size == n
            exp[o:o + n] = w
        got = self.got()
        if exp.dtype.kind == "f":
            assert lg._same(got, exp), what
        else:
            assert np.array_equal(got, exp), what


def _counts(unit):
    """0, 1, 7, 8, 9 elements, one full tile (256 * 4 16-byte units), one tile
    + 1 and two tiles with a ragged remainder."""
    tile = 256 * 4 * unit
    return [0, 1, 7, 8, 9, tile, tile + 1, 2 * tile + 100 * unit + min(3, unit - 1)]


def _segments(dt, n_ones):
    """[(p, g, m, v)] in dt's numpy form ("f32" / "f64") for _counts, then
    n_ones one-element segments: tests/test_sharded_adam_gpu.py's random data,
    its all-binade v and its IEEE specials at the start of the full tile, at
    the end of the tile + 1 segment (its scalar tail and the units before it)
    and, as many as there are such segments, in the one-element segments."""
    unit = 4 if dt == "f32" else 2
    counts = _counts(unit) + [1] * n_ones
    sp = ag._specials(dt)
    k = len(sp[0])
    segs = ag._fill(dt, counts)
    tile = 256 * 4 * unit
    first_one = len(counts) - n_ones
    for i, seg in enumerate(segs):
        n = seg[0].size
        for a, s in zip(seg, sp):
            if n == tile:
                a[:k] = s
            elif n == tile + 1:
                a[-k:] = s
            elif i >= first_one and i - first_one < k:
                a[0] = s[i - first_one]
    return counts, segs


@pytest.fixture(scope="module")
def segments():
    return {"f32": _segments("f32", LAMB_SEG + 1), "f64": _segments("f64", LAMB_SEG + 1),
            "master": _segments("f32", LAMB_MASTER_SEG + 1)}


def _g16(segs, dt):
    """The f32 gradients narrowed to 16 bits, plus the format's own largest
    finite value and smallest subnormal."""
    g16 = [lamb_ref.narrow16(seg[1], dt) for seg in segs]
    big = 0x7F7F if dt == "bf16" else 0x7BFF
    tile = next(i for i, g in enumerate(g16) if g.size == 256 * 4 * 4)
    g16[tile][40:44] = (big, big | 0x8000, 0x0001, 0x8001)
    return g16


# ---- the gated moments kernels against the reference ---------------------------------

@pytest.mark.parametrize("np_", [0, 3])
@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_gated_moments_bit_exact(segments, dt, np_):
    from kungfu_amd import ops
    counts, segs = segments[dt]
    assert counts.count(1) - 1 == LAMB_SEG + 1 > LAMB_SEG  # more than one launch's table
    for wd in (0.0, 1e-2):
        for mul, step in zip(MULS, (1, 7, 3)):
            g, st, dg, ds = _gate_state(mul, step)
            P, G, M, V = (Flat([seg[j] for seg in segs], counts, dt) for j in range(4))
            U = Flat([None] * len(counts), counts, dt)
            ops.lamb_moments_batch_gated_(P.views(), G.views(), M.views(), V.views(), U.views(),
                                          _hyper(wd), dg, ds, group=1, np_=np_)
            torch.cuda.synchronize()
            want = [gref.moments(*seg, np.zeros_like(seg[0]), dt, _hyper(wd), g, st, np_)
                    for seg in segs]
            where = (dt, np_, wd, mul)
            for j, (buf, what) in enumerate(((M, "exp_avg"), (V, "exp_avg_sq"), (U, "update"))):
                buf.check([w[j] for w in want], (what,) + where)
            P.check(None, ("param was written",) + where)
            G.check(None, ("grad was written",) + where)


@pytest.mark.parametrize("np_", [0, 3])
@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_gated_master_moments_bit_exact(segments, dt, np_):
    from kungfu_amd import ops
    counts, segs = segments["master"]
    assert counts.count(1) - 1 == LAMB_MASTER_SEG + 1 > LAMB_MASTER_SEG
    g16 = _g16(segs, dt)
    for wd in (0.0, 1e-2):
        for mul, step in zip(MULS, (1, 7, 3)):
            g, st, dg, ds = _gate_state(mul, step)
            G = Flat(g16, counts, dt)
            W, M, V = (Flat([seg[j] for seg in segs], counts, "f32") for j in (0, 2, 3))
            U = Flat([None] * len(counts), counts, "f32")
            ops.lamb_master_moments_batch_gated_(G.views(), W.views(), M.views(), V.views(),
                                                 U.views(), _hyper(wd), dg, ds, group=1, np_=np_)
            torch.cuda.synchronize()
            want = [gref.moments(seg[0], lamb_ref.widen16(g16[i], dt), seg[2], seg[3],
                                 np.zeros_like(seg[0]), "f32", _hyper(wd), g, st, np_)
                    for i, seg in enumerate(segs)]
            where = (dt, np_, wd, mul)
            for j, (buf, what) in enumerate(((M, "exp_avg"), (V, "exp_avg_sq"), (U, "update"))):
                buf.check([w[j] for w in want], (what,) + where)
            W.check(None, ("master was written",) + where)
            G.check(None, ("grad was written",) + where)


# ---- one rows-grid launch per moments kernel -------------------------------------------

def _rows_gate(skip):
    wd = 1e-2
    return (_hyper(wd),) + _gate_state(0.37, 5, skip)


@pytest.mark.parametrize("skip", [0, 1])
@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_gated_moments_rows_grid(dt, skip):
    from kungfu_amd import ops
    dev = torch.device("cuda:0")
    counts, segs = tl._update_data("lamb-" + dt, "rows", dt, 26)
    assert ll.multi_tile_rows(counts, *ll.UPDATE_KERNELS["lamb-" + dt][1:]) == (True, True)
    h, g, st, dg, ds = _rows_gate(skip)
    p, gr, m, v = tl._seat(segs, counts, dt, dev)
    u = tl.Seated([None] * len(counts), counts, dt, dev)
    ops.lamb_moments_batch_gated_(p.views(), gr.views(), m.views(), v.views(), u.views(), h, dg, ds,
                                  group=1, np_=tl.UPDATE_NP)
    torch.cuda.synchronize()
    want = [gref.moments(*seg, np.zeros_like(seg[0]), dt, h, g, st, tl.UPDATE_NP) for seg in segs]
    for j, (buf, what) in enumerate(((m, "exp_avg"), (v, "exp_avg_sq"), (u, "update"))):
        buf.check(None if skip else [w[j] for w in want], (what, dt, skip))
    p.check(None, ("param", dt, skip))
    gr.check(None, ("grad", dt, skip))


@pytest.mark.parametrize("skip", [0, 1])
@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_gated_master_moments_rows_grid(dt, skip):
    from kungfu_amd import ops
    dev = torch.device("cuda:0")
    counts, segs = tl._master_data("lamb_master-" + dt, "rows", dt, 27)
    h, g, st, dg, ds = _rows_gate(skip)
    gr = tl.Seated([seg[1] for seg in segs], counts, dt, dev)
    w, m, v = (tl.Seated([seg[j] for seg in segs], counts, "f32", dev) for j in (0, 2, 3))
    u = tl.Seated([None] * len(counts), counts, "f32", dev)
    ops.lamb_master_moments_batch_gated_(gr.views(), w.views(), m.views(), v.views(), u.views(), h,
                                         dg, ds, group=1, np_=tl.UPDATE_NP)
    torch.cuda.synchronize()
    want = [gref.moments(sw_, lamb_ref.widen16(sg, dt), sm, sv, np.zeros_like(sw_), "f32", h, g, st,
                         tl.UPDATE_NP) for sw_, sg, sm, sv in segs]
    for j, (buf, what) in enumerate(((m, "exp_avg"), (v, "exp_avg_sq"), (u, "update"))):
        buf.check(None if skip else [x[j] for x in want], (what, dt, skip))
    w.check(None, ("master", dt, skip))
    gr.check(None, ("grad", dt, skip))


# ---- the no-op gate: the ungated kernels' bits -------------------------------------------

@pytest.mark.parametrize("dt", ["f32", "f64", "bf16", "f16"])
def test_noop_gate_is_the_ungated_kernel(segments, dt):
    """skip 0, grad_mul 1 and a state seeded to the hyper's bias corrections:
    exp_avg, exp_avg_sq and the update are the ungated kernel's, bit for bit."""
    from kungfu_amd import ops
    master = dt in ("bf16", "f16")
    counts, segs = segments["master" if master else dt]
    cdt = "f32" if master else dt
    g16 = _g16(segs, dt) if master else None
    for wd in (0.0, 1e-2):
        for np_, step in ((0, 1), (3, 7)):
            _, _, dg, ds = _gate_state(1.0, step)
            outs = []
            for with_gate in (True, False):
                G = Flat(g16, counts, dt) if master else Flat([s[1] for s in segs], counts, dt)
                P, M, V = (Flat([seg[j] for seg in segs], counts, cdt) for j in (0, 2, 3))
                U = Flat([None] * len(counts), counts, cdt)
                hs = [lamb_ref.hyper(1e-2, betas=BETAS, eps=1e-6, weight_decay=wd, step=step)] * \
                    len(counts)
                if master and with_gate:
                    ops.lamb_master_moments_batch_gated_(G.views(), P.views(), M.views(), V.views(),
                                                         U.views(), _hyper(wd), dg, ds, group=1,
                                                         np_=np_)
                elif master:
                    ops.lamb_master_moments_batch_(G.views(), P.views(), M.views(), V.views(),
                                                   U.views(), hs, np_=np_)
                elif with_gate:
                    ops.lamb_moments_batch_gated_(P.views(), G.views(), M.views(), V.views(),
                                                  U.views(), _hyper(wd), dg, ds, group=1, np_=np_)
                else:
                    ops.lamb_moments_batch_(P.views(), G.views(), M.views(), V.views(), U.views(),
                                            hs, np_=np_)
                outs.append((M, V, U))
            torch.cuda.synchronize()
            for a, b, what in zip(outs[0], outs[1], ("exp_avg", "exp_avg_sq", "update")):
                assert lg._same(a.got(), b.got()), (what, dt, wd, np_, step)


# ---- the skip on pre-filled buffers ---------------------------------------------------------

def _bytes(t):
    return t.detach().cpu().contiguous().view(torch.uint8).numpy().copy()


@pytest.mark.parametrize("dt", ["f32", "f64", "bf16", "f16"])
def test_skip_leaves_every_buffer(segments, dt):
    """The moments, trust and apply passes under skip = 1: exp_avg,
    exp_avg_sq, the update, the parameters, the master, the 16-bit parameters,
    nlr and ratio are byte for byte what they were."""
    from kungfu_amd import ops
    master = dt in ("bf16", "f16")
    counts, _ = segments["master" if master else dt]
    cdt = "f32" if master else dt
    _, _, dg, ds = _gate_state(0.37, 2, skip=1)
    none = [None] * len(counts)
    G = Flat(none, counts, dt, fill_seed=1)
    P, M, V, U = (Flat(none, counts, cdt, fill_seed=2 + j) for j in range(4))
    P16 = Flat(none, counts, dt, fill_seed=9) if master else None
    bufs = [b for b in (G, P, M, V, U, P16) if b is not None]
    T = len(counts)
    f64 = dict(dtype=torch.float64, device="cuda")
    nlr, ratio = torch.full((T,), -0.25, **f64), torch.full((T,), 3.0, **f64)
    sq = torch.rand(2 * 2 * T, **f64) + 0.5
    group_of = torch.zeros(T, dtype=torch.int32, device="cuda")
    before = [_bytes(b.t) for b in bufs] + [_bytes(nlr), _bytes(ratio)]
    if master:
        ops.lamb_master_moments_batch_gated_(G.views(), P.views(), M.views(), V.views(), U.views(),
                                             _hyper(1e-2), dg, ds, group=1, np_=3)
    else:
        ops.lamb_moments_batch_gated_(P.views(), G.views(), M.views(), V.views(), U.views(),
                                      _hyper(1e-2), dg, ds, group=1, np_=3)
    ops.lamb_trust_update_gated_(sq, 2, group_of, [{"lr": 0.1, "adapt": True}], nlr, ratio, dg,
                                 trust_clip=1.5)
    plan = ops.LambApplyPlan(P.views(), U.views(), list(range(T)), T,
                             P16.views() if master else None)
    plan.run(nlr, gate=dg)
    torch.cuda.synchronize()
    after = [_bytes(b.t) for b in bufs] + [_bytes(nlr), _bytes(ratio)]
    for i, (a, b) in enumerate(zip(before, after)):
        assert np.array_equal(a, b), (dt, i)
    # the same calls with skip = 0 do write: the test sees what it looks for
    _, _, dg0, ds0 = _gate_state(0.37, 2, skip=0)
    ops.lamb_trust_update_gated_(sq, 2, group_of, [{"lr": 0.1, "adapt": True}], nlr, ratio, dg0,
                                 trust_clip=1.5)
    plan.run(nlr, gate=dg0)
    torch.cuda.synchronize()
    assert not np.array_equal(_bytes(nlr), before[-2]) and not np.array_equal(_bytes(P.t), before[1])
    plan.close()


# ---- the gated trust kernel --------------------------------------------------------------------

@pytest.mark.parametrize("ngroup", [1, 20])
@pytest.mark.parametrize("world,T", [(1, 1), (3, 1), (1, 300), (3, 300)])
def test_gated_trust_kernel_bit_exact(world, T, ngroup):
    from kungfu_amd import ops
    rng = np.random.default_rng(100 * world + T + ngroup)
    sq = np.exp2(rng.uniform(-40, 40, (world, 2 * T)))
    if T > 8:
        sq[:, 0] = 0.0
        sq[:, T + 1] = 0.0
        sq[world - 1, 3] = np.inf
        sq[0, T + 4] = np.inf
        sq[0, 6] = np.nan
    group_of = rng.integers(0, ngroup, T).astype(np.int32)
    dsq = torch.from_numpy(sq.reshape(-1).copy()).cuda()
    dgo = torch.from_numpy(group_of).cuda()
    f64 = dict(dtype=torch.float64, device="cuda")
    for clip in (0.0, 1.5):
        groups = [{"lr": 1e-3 * (j + 1), "adapt": j % 2 == 0} for j in range(ngroup)]
        lrs, adapts = [groups[j]["lr"] for j in group_of], [groups[j]["adapt"] for j in group_of]
        old = (np.full(T, 9.0), np.full(T, 8.0))
        for skip in (0, 1):
            g, _, dg, _ = _gate_state(0.37, 2, skip=skip)
            nlr, ratio = torch.full((T,), 9.0, **f64), torch.full((T,), 8.0, **f64)
            ops.lamb_trust_update_gated_(dsq, world, dgo, groups, nlr, ratio, dg, trust_clip=clip)
            torch.cuda.synchronize()
            want = gref.trust(sq, lrs, adapts, *old, g, clip)
            assert lg._same(nlr.cpu().numpy(), want[0]), (world, T, ngroup, clip, skip)
            assert lg._same(ratio.cpu().numpy(), want[1]), (world, T, ngroup, clip, skip)
            if skip:
                assert np.array_equal(want[0], old[0]) and np.array_equal(want[1], old[1])
                continue
            # unskipped: the ungated kernel's bits
            nlr2, ratio2 = torch.full((T,), 9.0, **f64), torch.full((T,), 8.0, **f64)
            ops.lamb_trust_update_(dsq, world, dgo, groups, nlr2, ratio2, trust_clip=clip)
            torch.cuda.synchronize()
            assert lg._same(nlr.cpu().numpy(), nlr2.cpu().numpy())
            assert lg._same(ratio.cpu().numpy(), ratio2.cpu().numpy())


# ---- the gated apply run ---------------------------------------------------------------------------

def _apply_layout(unit):
    """[(start, length)]: every element offset 0..8 from a 16-byte boundary
    with lengths 1, 9, one tile - 1 and one tile + 1 elements."""
    tile = 256 * 4 * unit
    pieces, cur = [], 16
    for off in range(9):
        for n in (1, 9, tile - 1, tile + 1):
            start = cur + off
            pieces.append((start, n))
            cur = -(-(start + n + lg.GUARD) // 16) * 16 + 16
    return pieces, cur


@pytest.mark.parametrize("dt", ["f32", "f64", "bf16", "f16"])
def test_gated_apply_bit_exact(dt):
    from kungfu_amd import ops
    master = dt in ("bf16", "f16")
    cdt = "f32" if master else dt
    C = lamb_ref.COMPUTE[cdt]
    pieces, total = _apply_layout(2 if dt == "f64" else 4)
    rng = np.random.default_rng(5)
    T = 7
    p = rng.standard_normal(total).astype(C)
    u = rng.standard_normal(total).astype(C)
    u[pieces[5][0]] = np.inf
    u[pieces[2][0]:pieces[2][0] + 3] = (np.nan, -0.0, 0.0)
    p[pieces[6][0]] = -0.0
    nlr = -np.exp2(rng.uniform(-12, 2, T))
    nlr[3] = -0.0
    p16 = rng.integers(0, 0x7000, total).astype(np.uint16)
    tensors = [i % T for i in range(len(pieces))]
    dnlr = torch.from_numpy(nlr).cuda()
    want, want16 = p.copy(), p16.copy()
    for (s, n), t in zip(pieces, tensors):
        want[s:s + n] = lamb_ref.apply(p[s:s + n], u[s:s + n], nlr[t], cdt)
        want16[s:s + n] = lamb_ref.narrow16(want[s:s + n], dt) if master else 0
    outs = {}
    for how in ("gated", "skipped", "ungated"):
        dp, du = ag._dev(p, cdt), ag._dev(u, cdt)
        d16 = lg._dev16(p16, dt) if master else None
        plan = ops.LambApplyPlan([dp[s:s + n] for s, n in pieces], [du[s:s + n] for s, n in pieces],
                                 tensors, T, [d16[s:s + n] for s, n in pieces] if master else None)
        if how == "ungated":
            plan.run(dnlr)
        else:
            g, _, dg, _ = _gate_state(0.37, 2, skip=int(how == "skipped"))
            plan.run(dnlr, gate=dg)
        torch.cuda.synchronize()
        outs[how] = (ag._host(dp, cdt), lg._host16(d16) if master else None)
        assert ag._host(du, cdt).tobytes() == u.tobytes(), ("update was written", how)
        plan.close()
    # the whole buffers: the elements around every piece keep their bits
    assert lg._same(outs["gated"][0], want), dt
    assert outs["skipped"][0].tobytes() == p.tobytes(), "a skipped run wrote the parameters"
    assert lg._same(outs["ungated"][0], outs["gated"][0])
    if master:
        assert np.array_equal(outs["gated"][1], want16), dt
        assert np.array_equal(outs["skipped"][1], p16), "a skipped run wrote the 16-bit parameters"
        assert np.array_equal(outs["ungated"][1], outs["gated"][1])


# ---- the whole step ----------------------------------------------------------------------------------

SCALES = [1024.0, 1024.0, 512.0, 512.0]  # cg.body_gated asserts the reference gives these


def _run_gated_model(world, rank, ex):
    """tests/test_sharded_lamb_gated.py's model on the GPU: per step the
    device's (p, u) norm sums and a snapshot around the skipped step; at the
    end the parameters, the state, the ratios, the gate and the step states."""
    ps, opt = cg.g_optimizer(ex, device="cuda")
    opt._kf_build_sharded()
    sums, snaps = [], {}
    for s in range(cg.G_STEPS):
        cg.g_run(ps, opt, world, rank, SCALES, "cuda", first_step=s, steps=1)
        sums.append([L["sq"].cpu().numpy().reshape(world, -1).copy() for L in opt._kf_lamb])
        if s in (cg.G_BAD - 1, cg.G_BAD):
            snaps[s] = cg._snapshot(ps, opt)
    sb = opt.state_buffers()
    ratios = opt.last_trust_ratios()
    torch.cuda.synchronize()
    none = {"exp_avg": torch.zeros(0), "exp_avg_sq": torch.zeros(0), "step": None}
    k = len(cg.NUMELS)
    return {"p": [cg.lamb.to_numpy(p) for p in ps],
            "m": [sb.get(p, none)["exp_avg"].cpu().numpy().reshape(-1) for p in ps],
            "v": [sb.get(p, none)["exp_avg_sq"].cpu().numpy().reshape(-1) for p in ps],
            "w": [sb.get(p, {"master": torch.zeros(0)})["master"].cpu().numpy().reshape(-1)
                  if j >= k else None for j, p in enumerate(ps)],
            "steps": {sb[p]["step"] for p in ps if p in sb},
            "ratio": [ratios[p] for p in ps], "sums": sums, "snaps": snaps,
            "gate": gated.read_gate(opt._kf_gate), "states": gated.read_states(opt._kf_gstates),
            "accessors": (opt.skipped_steps(), opt.applied_steps(), opt.loss_scale_value(),
                          opt.last_grad_norm()),
            "cuts": cg.lamb.model_cuts(opt, world)}


def _check_gated_model(got, world):
    """Every rank against lamb_gated_ref run on the unsharded tensors with the
    device's own (p, u) norm sums, as in §17; the verdict's sums are exact."""
    want = cg.g_reference(world, got[0]["cuts"], sums=got[0]["sums"])
    assert want["scales"] == SCALES and want["gate"]["skipped"] == 1
    assert sum(1 for n in want["norms"] if np.isfinite(n) and n > 1.0) >= 1  # the clip was active
    assert want["norms"][cg.G_SMALL] < 1.0
    for r in range(world):
        g = got[r]
        for a, b in zip(g["sums"], got[0]["sums"]):
            for x, y in zip(a, b):
                assert np.array_equal(x, y, equal_nan=True), ("ranks disagree on the sums", r)
        for j in range(len(want["p"])):
            assert lg._same(g["p"][j], want["p"][j]), ("param", r, j)
            assert lg._same(g["m"][j], want["m"][j]), ("exp_avg", r, j)
            assert lg._same(g["v"][j], want["v"][j]), ("exp_avg_sq", r, j)
            if want["w"][j] is not None:
                assert lg._same(g["w"][j], want["w"][j]), ("master", r, j)
            assert g["ratio"][j] == want["ratio"][j], ("ratio", r, j)
        assert g["steps"] == {cg.G_STEPS - 1}
        for f in step_gate_ref.GATE_FIELDS:
            a = np.asarray(g["gate"][f])
            assert a.tobytes() == np.asarray(want["gate"][f]).astype(a.dtype).tobytes(), (f, r)
        for j, st in enumerate(want["states"]):
            for f in step_gate_ref.STATE_FIELDS:
                a = np.asarray(g["states"][j][f])
                assert a.tobytes() == np.asarray(st[f]).astype(a.dtype).tobytes(), (f, j, r)
        assert g["accessors"][:3] == (1, cg.G_STEPS - 1, float(want["gate"]["loss_scale"]))
        assert g["accessors"][3] == want["gate"]["grad_norm"]
        # the skipped step: parameters, state, u, nlr, ratio and the step states stood still
        a, b = g["snaps"][cg.G_BAD - 1], g["snaps"][cg.G_BAD]
        for x, y in zip(a[0], b[0]):
            assert x.tobytes() == y.tobytes(), ("param moved on a skip", r)
        for j in a[1]:
            for f in a[1][j]:
                if f != "step":
                    assert a[1][j][f].tobytes() == b[1][j][f].tobytes(), (f, j, r)
            assert a[1][j]["step"] == b[1][j]["step"] == cg.G_BAD
        for x, y in zip(a[2], b[2]):
            assert all(p.tobytes() == q.tobytes() for p, q in zip(x, y)), ("u moved on a skip", r)
        for x, y in zip(a[3], b[3]):
            assert x[0].tobytes() == y[0].tobytes() and x[1].tobytes() == y[1].tobytes()
        assert a[4].tobytes() == b[4].tobytes(), ("a step state moved on a skip", r)


@pytest.mark.parametrize("world", [2, 3])
def test_whole_gated_step_over_loopback(world):
    got = {}

    def body(rank, ex):
        got[rank] = _run_gated_model(world, rank, ex)

    loopback.loop_ranks(world, body)
    _check_gated_model(got, world)


def test_whole_gated_step_world1_rccl():
    """A one-rank librccl communicator: the collectives run."""
    ex = loopback.rccl1_exchange()
    got = {0: _run_gated_model(1, 0, ex)}
    ex.close()
    _check_gated_model(got, 1)


# ---- ShardedLAMBOptimizer(gate=...) on a model --------------------------------------------------------

def _two_layer_gated(ex, world, rank, steps=5, bad=2):
    """A two-layer f16 model under gate={"max_grad_norm": 1.0, "loss_scale":
    "dynamic"}; step `bad` gets one inf in a gradient on the last rank."""
    torch.manual_seed(0)
    model = torch.nn.Sequential(torch.nn.Linear(9, 17), torch.nn.Tanh(),
                                torch.nn.Linear(17, 3)).cuda().half()
    from kungfu_amd.torch.optimizers import ShardedLAMBOptimizer
    decay = [p for n, p in model.named_parameters() if n.endswith("weight")]
    plain = [p for n, p in model.named_parameters() if n.endswith("bias")]
    opt = ShardedLAMBOptimizer(
        torch.optim.AdamW([{"params": decay, "weight_decay": 1e-2},
                           {"params": plain, "weight_decay": 0.0}], lr=1e-2, eps=1e-6),
        model.named_parameters(), exchange=ex, bucket_bytes=256, master_weights=True,
        gate={"max_grad_norm": 1.0, "loss_scale": "dynamic"})
    gen = torch.Generator().manual_seed(100 + rank)
    log = []
    for s in range(steps):
        x = torch.randn(8, 9, generator=gen).cuda().half()
        y = torch.randn(8, 3, generator=gen).cuda()
        opt.zero_grad()
        loss = ((model(x).float() - y) ** 2).mean()
        opt.scale_loss(loss).backward()
        if s == bad and rank == world - 1:
            decay[0].grad[0, 0] = float("inf")
        before = [p.detach().clone() for p in model.parameters()]
        scale = opt.loss_scale_value()
        skipped = opt.skipped_steps()
        opt.step()
        was_skipped = opt.skipped_steps() - skipped
        moved = any(not torch.equal(a, p.detach()) for a, p in zip(before, model.parameters()))
        log.append((was_skipped, moved, scale, opt.loss_scale_value(), opt.last_grad_norm()))
    ratios = opt.last_trust_ratios()
    counts = (opt.skipped_steps(), opt.applied_steps())
    torch.cuda.synchronize()
    return [p.detach().cpu().numpy().copy() for p in model.parameters()], \
        [ratios[p] for p in model.parameters()], log, counts


def _check_two_layer(out, steps=5, bad=2):
    ps, ratios, log, (skipped, applied) = out
    assert all(np.isfinite(p.astype(np.float32)).all() for p in ps)
    assert skipped + applied == steps and skipped >= 1 and applied >= 2
    for s, (was_skipped, moved, scale, scale_after, norm) in enumerate(log):
        assert was_skipped in (0, 1)
        if was_skipped:  # nothing moved, the scale backed off
            assert not moved and scale_after == scale / 2 and not np.isfinite(norm), (s, log)
        else:
            assert moved and scale_after == scale and np.isfinite(norm), (s, log)
    assert log[bad][0] == 1, log
    assert ratios[1] == 1.0 and ratios[3] == 1.0                     # the biases: no decay
    assert ratios[0] != 1.0 and ratios[2] != 1.0 and all(np.isfinite(ratios))


def test_gated_optimizer_two_layer_f16_model():
    """World 1 on a plain NativeExchange and on the default
    collective.Exchange: the same bits. World 2 over loopback: both ranks end
    with the same parameters. The overflow step is skipped on every one."""
    from kungfu_amd.exchange import NativeExchange
    outs = []
    for make in (NativeExchange, lambda: None):
        ex = make()
        outs.append(_two_layer_gated(ex, 1, 0))
        if ex is not None:
            ex.close()
    for o in outs:
        _check_two_layer(o)
    for a, b in zip(outs[0][0], outs[1][0]):
        assert lg._same(a, b)
    got = {}

    def body(rank, ex):
        got[rank] = _two_layer_gated(ex, 2, rank)

    loopback.loop_ranks(2, body)
    for r in (0, 1):
        _check_two_layer(got[r])
    for a, b in zip(got[0][0], got[1][0]):
        assert lg._same(a, b)
    assert got[0][1] == got[1][1] and got[0][3] == got[1][3]
