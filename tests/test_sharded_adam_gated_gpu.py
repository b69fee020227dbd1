"""The gated sharded Adam / AdamW step on the GPU, bit for bit against
tests/step_gate_ref.py: the gated update kernels alone (every dtype, the
no-op gate against the ungated kernels, the skip), the gate kernel alone,
non-finite detection through the real norm pass, the native exchange's two
halves over the loopback transport and a one-rank librccl communicator, and
ShardedAdamOptimizer(max_grad_norm, loss_scale) end to end. Shapes and helpers
are tests/test_sharded_adam_gpu.py's and tests/test_sharded_adam_master_gpu.py's."""
import numpy as np
import pytest
import torch

import adam_ref
import loopback
import step_gate_ref as ref
import test_sharded_adam as cpu
import test_sharded_adam_gpu as gpu
import test_sharded_adam_master_gpu as mgpu

pytestmark = pytest.mark.gpu

PLAIN = ("f32", "bf16", "f64")
MASTER = ("bf16", "f16")
MULS = (1.0, 2.0 ** -16, 0.37)
# the hyper of a gated call: one for every segment, no step
BETAS = (0.9, 0.999)


def _hyper(row):
    wd, decoupled = cpu.ROWS[row]
    return {"lr": 1e-2, "betas": BETAS, "eps": 1e-8, "weight_decay": wd, "decoupled": decoupled}


def _gate_state(mul, step, skip=0, lr=1e-2):
    """(reference gate, reference state) as a verdict would leave them after
    `step` applied steps, with grad_mul = mul."""
    g = ref.new_gate()
    g["skip"], g["grad_mul"] = skip, np.float32(mul)
    st = ref.scalars_of(adam_ref.hyper(lr, betas=BETAS, step=step))
    return g, st


def _dev_gate(g):
    from kungfu_amd import _lib
    a = np.zeros(1, _lib.step_gate_dtype())
    for k in ref.GATE_FIELDS:
        a[k] = g[k]
    return torch.from_numpy(a.view(np.uint8).copy()).cuda()


def _dev_states(states):
    from kungfu_amd import _lib
    a = np.zeros(len(states), _lib.step_state_dtype())
    for j, st in enumerate(states):
        for k in ref.STATE_FIELDS:
            a[k][j] = st[k]
    return torch.from_numpy(a.view(np.uint8).copy()).cuda()


@pytest.fixture(scope="module")
def segments():
    return {dt: (gpu._segments(dt), gpu._rows_segments(dt)) for dt in PLAIN}


@pytest.fixture(scope="module")
def master_segments():
    return {dt: (mgpu._segments(dt), mgpu._rows_segments(dt)) for dt in MASTER}


# ---- the gated kernels against the reference -----------------------------------

@pytest.mark.parametrize("np_", [0, 3])
@pytest.mark.parametrize("dt", PLAIN)
def test_gated_kernel_bit_exact(segments, dt, np_):
    from kungfu_amd import ops
    for which, segs in enumerate(segments[dt]):
        base = [[gpu._dev(a, dt) for a in seg] for seg in segs]
        for row in range(len(cpu.ROWS)):
            h = _hyper(row)
            for mul, step in zip(MULS, (1, 7, 3)):
                g, st = _gate_state(mul, step)
                # group 1 of two: the kernel reads its own group's state
                dg, ds = _dev_gate(g), _dev_states([ref.new_state(), st])
                ps, gs, ms, vs = ([seg[j].clone() for seg in base] for j in range(4))
                ops.adam_update_batch_gated_(ps, gs, ms, vs, h, dg, ds, group=1, np_=np_)
                torch.cuda.synchronize()
                for i, seg in enumerate(segs):
                    wp, wm, wv = ref.update(*seg, dt, h, g, st, np_)
                    where = (dt, np_, which, row, mul, i, seg[0].size)
                    assert gpu._same(gpu._host(ps[i], dt), wp, dt), ("param",) + where
                    assert gpu._same(gpu._host(gs[i], dt), seg[1], dt), ("grad written",) + where
                    assert gpu._same(gpu._host(ms[i], dt), wm, dt), ("exp_avg",) + where
                    assert gpu._same(gpu._host(vs[i], dt), wv, dt), ("exp_avg_sq",) + where


@pytest.mark.parametrize("np_", [0, 3])
@pytest.mark.parametrize("dt", MASTER)
def test_gated_master_kernel_bit_exact(master_segments, dt, np_):
    from kungfu_amd import ops
    for which, segs in enumerate(master_segments[dt]):
        base_g = [mgpu._dev16(seg[0], dt) for seg in segs]
        base_f = [[mgpu._dev32(a) for a in seg[1:]] for seg in segs]
        for row in range(len(cpu.ROWS)):
            h = _hyper(row)
            for mul, step in zip(MULS, (1, 7, 3)):
                g, st = _gate_state(mul, step)
                dg, ds = _dev_gate(g), _dev_states([st])
                gs = [x.clone() for x in base_g]
                ws, ms, vs = ([f[j].clone() for f in base_f] for j in range(3))
                ps = [torch.full_like(x, 7.0) for x in gs]
                ops.adam_master_update_batch_gated_(ps, gs, ws, ms, vs, h, dg, ds, np_=np_)
                torch.cuda.synchronize()
                for i, seg in enumerate(segs):
                    wp, ww, wm, wv = ref.update_master(seg[1], seg[0], seg[2], seg[3], dt, h, g, st,
                                                       np_)
                    where = (dt, np_, which, row, mul, i, seg[0].size)
                    assert mgpu._same32(mgpu._host32(ws[i]), ww), ("master",) + where
                    assert mgpu._same16(mgpu._host16(ps[i], dt), wp, dt), ("param",) + where
                    assert mgpu._same16(mgpu._host16(gs[i], dt), seg[0], dt), ("grad written",) + where
                    assert mgpu._same32(mgpu._host32(ms[i]), wm), ("exp_avg",) + where
                    assert mgpu._same32(mgpu._host32(vs[i]), wv), ("exp_avg_sq",) + where


# ---- the no-op gate: the ungated kernels' bits ----------------------------------

@pytest.mark.parametrize("dt", PLAIN)
def test_noop_gate_is_the_ungated_kernel(segments, dt):
    from kungfu_amd import ops
    for segs in segments[dt]:
        base = [[gpu._dev(a, dt) for a in seg] for seg in segs]
        for row, (wd, decoupled) in enumerate(cpu.ROWS):
            for np_, step in ((0, 1), (3, 7)):
                g, st = _gate_state(1.0, step)
                a = [[seg[j].clone() for seg in base] for j in range(4)]
                b = [[seg[j].clone() for seg in base] for j in range(4)]
                ops.adam_update_batch_gated_(*a, _hyper(row), _dev_gate(g), _dev_states([st]),
                                             np_=np_)
                hs = [adam_ref.hyper(1e-2, betas=BETAS, weight_decay=wd, decoupled=decoupled,
                                     step=step)] * len(segs)
                ops.adam_update_batch_(*b, hs, np_=np_)
                torch.cuda.synchronize()
                for j, what in enumerate(("param", "grad", "exp_avg", "exp_avg_sq")):
                    for i in range(len(segs)):
                        assert gpu._same(gpu._host(a[j][i], dt), gpu._host(b[j][i], dt), dt), \
                            (what, dt, row, np_, i)


@pytest.mark.parametrize("dt", MASTER)
def test_noop_gate_is_the_ungated_master_kernel(master_segments, dt):
    from kungfu_amd import ops
    for segs in master_segments[dt]:
        base_g = [mgpu._dev16(seg[0], dt) for seg in segs]
        base_f = [[mgpu._dev32(x) for x in seg[1:]] for seg in segs]
        for row, (wd, decoupled) in enumerate(cpu.ROWS):
            for np_, step in ((0, 1), (3, 7)):
                g, st = _gate_state(1.0, step)
                outs = []
                for gated in (True, False):
                    gs = [x.clone() for x in base_g]
                    ws, ms, vs = ([f[j].clone() for f in base_f] for j in range(3))
                    ps = [torch.full_like(x, 7.0) for x in gs]
                    if gated:
                        ops.adam_master_update_batch_gated_(ps, gs, ws, ms, vs, _hyper(row),
                                                            _dev_gate(g), _dev_states([st]), np_=np_)
                    else:
                        hs = [adam_ref.hyper(1e-2, betas=BETAS, weight_decay=wd,
                                             decoupled=decoupled, step=step)] * len(segs)
                        ops.adam_master_update_batch_(ps, gs, ws, ms, vs, hs, np_=np_)
                    outs.append((ps, ws, ms, vs))
                torch.cuda.synchronize()
                for i in range(len(segs)):
                    assert mgpu._same16(mgpu._host16(outs[0][0][i], dt),
                                        mgpu._host16(outs[1][0][i], dt), dt), ("param", dt, row, i)
                    for j, what in ((1, "master"), (2, "exp_avg"), (3, "exp_avg_sq")):
                        assert mgpu._same32(mgpu._host32(outs[0][j][i]),
                                            mgpu._host32(outs[1][j][i])), (what, dt, row, np_, i)


# ---- the skip -------------------------------------------------------------------

def _bytes(t):
    return t.detach().cpu().contiguous().view(torch.uint8).numpy().copy()


def _pattern(t, seed):
    """Distinct bytes per buffer: a skipped step must leave every one alone."""
    n = t.numel() * t.element_size()
    a = np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)
    return torch.from_numpy(a).cuda().view(t.dtype)


@pytest.mark.parametrize("dt", PLAIN)
def test_skip_leaves_every_buffer(segments, dt):
    from kungfu_amd import ops
    g, st = _gate_state(0.37, 2, skip=1)
    for segs in segments[dt]:
        bufs = [[_pattern(gpu._dev(a, dt), 17 * i + j) for i, seg in enumerate(segs)
                 for a in [seg[j]]] for j in range(4)]
        before = [[_bytes(t) for t in col] for col in bufs]
        ops.adam_update_batch_gated_(*bufs, _hyper(1), _dev_gate(g), _dev_states([st]), np_=3)
        torch.cuda.synchronize()
        for col, was in zip(bufs, before):
            for t, w in zip(col, was):
                assert np.array_equal(_bytes(t), w), (dt, t.numel())


@pytest.mark.parametrize("dt", MASTER)
def test_skip_leaves_every_master_buffer(master_segments, dt):
    from kungfu_amd import ops
    g, st = _gate_state(0.37, 2, skip=1)
    for segs in master_segments[dt]:
        ps = [_pattern(mgpu._dev16(seg[0], dt), 5 * i) for i, seg in enumerate(segs)]
        gs = [_pattern(mgpu._dev16(seg[0], dt), 5 * i + 1) for i, seg in enumerate(segs)]
        ws, ms, vs = ([_pattern(mgpu._dev32(seg[1]), 5 * i + 2 + j) for i, seg in enumerate(segs)]
                      for j in range(3))
        cols = (ps, gs, ws, ms, vs)
        before = [[_bytes(t) for t in col] for col in cols]
        ops.adam_master_update_batch_gated_(*cols, _hyper(2), _dev_gate(g), _dev_states([st]),
                                            np_=3)
        torch.cuda.synchronize()
        for col, was in zip(cols, before):
            for t, w in zip(col, was):
                assert np.array_equal(_bytes(t), w), (dt, t.numel())


# ---- the gate kernel ------------------------------------------------------------

def _read(dg, ds):
    from kungfu_amd import ops
    return ops.read_step_gate(dg), ops.read_step_states(ds)


def _same_scalar(a, b):
    a, b = np.asarray(a), np.asarray(b).astype(np.asarray(a).dtype)
    if a.dtype.kind == "f":
        return (np.isnan(a) and np.isnan(b)) or a.tobytes() == b.tobytes()
    return a == b


def _check_gate(dg, ds, g, states, where):
    got_g, got_s = _read(dg, ds)
    for k in ref.GATE_FIELDS:
        assert _same_scalar(got_g[k], g[k]), (k, got_g[k], g[k]) + where
    for j, st in enumerate(states):
        for k in ref.STATE_FIELDS:
            assert _same_scalar(got_s[k][j], st[k]), (k, j, got_s[k][j], st[k]) + where


GROUPS2 = [{"lr": 1e-3, "betas": (0.9, 0.999)}, {"lr": 3e-2, "betas": (0.8, 0.95)}]


@pytest.mark.parametrize("world,nplan", [(1, 1), (3, 1), (1, 3), (3, 3)])
def test_gate_kernel_bit_exact(world, nplan):
    """Finite, +inf and NaN totals; a norm below and above max_norm; max_norm
    0; mixed np_k; a growth step and a backoff step."""
    from kungfu_amd import ops
    rng = np.random.default_rng(100 * world + nplan)
    nps = [0, 3, 4][:nplan]
    cases = []
    for kind in ("small", "large", "inf", "nan"):
        sq = rng.uniform(0.01, 1.0, (world, nplan)) * (1e-3 if kind == "small" else 1e9)
        if kind == "inf":
            sq[world - 1, nplan - 1] = np.inf
        if kind == "nan":
            sq[0, 0] = np.nan
        for max_norm in (0.0, 1.0):
            cases.append((kind, sq, max_norm))
    for scale0, interval in ((1.0, 0), (65536.0, 2)):
        g, states = ref.new_gate(scale0), [ref.new_state(betas=h["betas"]) for h in GROUPS2]
        dg = ops.new_step_gate("cuda", scale0)
        ds = ops.new_step_states("cuda", 2)
        for i, (kind, sq, max_norm) in enumerate(cases):
            kw = dict(max_norm=max_norm, growth_factor=2.0, backoff_factor=0.5,
                      growth_interval=interval)
            ref.gate_update(sq, nps, GROUPS2, states, g, **kw)
            ops.step_gate_update_(torch.from_numpy(sq.reshape(-1).copy()).cuda(), world, nps,
                                  GROUPS2, ds, dg, **kw)
            _check_gate(dg, ds, g, states, (world, nplan, scale0, i, kind, max_norm))
        # both rules were seen: clipping on and off, growth and backoff
        assert g["skipped"] == 4 and g["applied"] == 4
        if interval:
            assert g["loss_scale"] != np.float32(scale0)


def test_gate_kernel_pows_stand_still_on_a_skip():
    """Two groups with different lr and betas over 5 calls, the third one a
    skip: neither the pows nor the step advance on it."""
    from kungfu_amd import ops
    g, states = ref.new_gate(1024.0), [ref.new_state(betas=h["betas"]) for h in GROUPS2]
    dg, ds = ops.new_step_gate("cuda", 1024.0), ops.new_step_states("cuda", 2)
    for i in range(5):
        sq = np.array([[4.0 + i, 9.0], [1.0, np.inf if i == 2 else 16.0]])
        groups = [dict(h, lr=h["lr"] * (1 + i)) for h in GROUPS2]
        kw = dict(max_norm=1.0, growth_factor=2.0, backoff_factor=0.5, growth_interval=2)
        before = [dict(st) for st in states]
        ref.gate_update(sq, [2, 0], groups, states, g, **kw)
        ops.step_gate_update_(torch.from_numpy(sq.reshape(-1).copy()).cuda(), 2, [2, 0], groups, ds,
                              dg, **kw)
        _check_gate(dg, ds, g, states, (i,))
        if i == 2:
            assert g["skip"] == 1 and states == before
    assert [st["step"] for st in states] == [4, 4] and g["skipped"] == 1
    assert states[0]["beta1_pow"] == 0.9 * 0.9 * 0.9 * 0.9


def test_gate_kernel_many_plans_and_groups():
    """More plans and groups than one launch's kernel arguments hold."""
    from kungfu_amd import ops
    nplan, ngroup, world = 150, 37, 2
    rng = np.random.default_rng(5)
    nps = [int(x) for x in rng.integers(0, 4, nplan)]
    groups = [{"lr": 1e-3 * (j + 1), "betas": (0.9 - 0.01 * j, 0.999 - 0.001 * j)}
              for j in range(ngroup)]
    g, states = ref.new_gate(8.0), [ref.new_state() for _ in groups]
    dg, ds = ops.new_step_gate("cuda", 8.0), ops.new_step_states("cuda", ngroup)
    for i in range(3):
        sq = rng.uniform(0.0, 2.0, (world, nplan))
        if i == 1:
            sq[1, 140] = np.nan
        ref.gate_update(sq, nps, groups, states, g, max_norm=0.5)
        ops.step_gate_update_(torch.from_numpy(sq.reshape(-1).copy()).cuda(), world, nps, groups,
                              ds, dg, max_norm=0.5)
        _check_gate(dg, ds, g, states, (i,))
    assert g["skipped"] == 1 and states[-1]["step"] == 2


# ---- non-finite detection through the real norm pass ------------------------------

_TORCH = {"f32": torch.float32, "f64": torch.float64, "bf16": torch.bfloat16, "f16": torch.float16}


@pytest.mark.parametrize("dt", ["f16", "bf16", "f32"])
def test_norm_pass_sees_every_non_finite_gradient(dt):
    """One +-inf or NaN in a vector body, a scalar tail or a one-element
    segment sets skip; the largest finite values do not."""
    from kungfu_amd import ops
    sizes = (4096, 1021, 1)
    big = float(torch.finfo(_TORCH[dt]).max)
    tensors = [torch.zeros(n, dtype=_TORCH[dt], device="cuda") for n in sizes]
    plan = ops.SegNorm(tensors)
    out = torch.empty(len(sizes) + 1, dtype=torch.float64, device="cuda")
    verdicts = {}
    spots = ((0, 100), (1, 1020), (2, 0))  # a vector body, a scalar tail, a segment of one
    for name, val in (("+inf", np.inf), ("-inf", -np.inf), ("nan", np.nan), ("max", big),
                      ("-max", -big)):
        for seg, at in spots:
            for t in tensors:
                t.zero_()
            tensors[seg][at] = val
            if name.endswith("max"):  # every spot at once, and their neighbours
                for s2, a2 in spots:
                    tensors[s2][a2] = val
            plan.run("sq", out=out)
            dg, ds = ops.new_step_gate("cuda", 65536.0), ops.new_step_states("cuda", 1)
            ops.step_gate_update_(out[len(sizes):], 1, [0], GROUPS2[:1], ds, dg, max_norm=1.0)
            got, st = _read(dg, ds)
            verdicts[(name, seg)] = int(got["skip"])
            assert int(st["step"][0]) == (0 if got["skip"] else 1)
    for (name, seg), skip in verdicts.items():
        assert skip == (0 if name.endswith("max") else 1), (dt, name, seg, verdicts)


# ---- the native exchange's two halves over the loopback transport -----------------

NS = gpu.NS
X_LRS = (1e-2, 5e-3, 2e-2)
X_BAD = 1            # the step whose f32 gradient carries an inf, on the last rank only
X_SCALE0, X_MAX_NORM = 1024.0, 1.0
X_RULE = dict(growth_factor=2.0, backoff_factor=0.5, growth_interval=2)
# group 0: f16 with master weights, AdamW (all-to-all and fold under "auto": np = 0);
# group 1: f32, Adam with L2 decay (reduce-scatter: np = world)
X_GROUPS = ({"dt": "f16", "lr_mul": 1.0, "betas": (0.9, 0.999), "weight_decay": 1e-2,
             "decoupled": True},
            {"dt": "f32", "lr_mul": 0.5, "betas": (0.8, 0.95), "weight_decay": 1e-2,
             "decoupled": False})


def _x_hyper(g, lr):
    return {"lr": lr * g["lr_mul"], "betas": g["betas"], "eps": 1e-8,
            "weight_decay": g["weight_decay"], "decoupled": g["decoupled"]}


def _x_store(x, dt):
    return mgpu._store16(x, dt) if dt == "f16" else np.asarray(x, np.float32)


def _x_widen(a, dt):
    return ref.adam_master_ref.widen(a, dt) if dt == "f16" else a


def _x_grad(dt, n, L, seed, scale, bad):
    """A padded gradient bucket: multiples of 1/4 in [-8, 8] times the loss
    scale (a power of two), so every sum over ranks and of squares is exact."""
    g = np.zeros(L, np.float32)
    g[:n] = np.random.default_rng(seed).integers(-32, 33, n) / 4.0 * scale
    if bad:
        g[n // 2] = np.inf
    return _x_store(g, dt)


def _x_param(dt, n, L, seed):
    p = np.zeros(L, np.float32)
    p[:n] = np.random.default_rng(seed).standard_normal(n)
    return _x_store(p, dt)


def _x_counts(world):
    from kungfu_amd.collective import padded_count
    return [[padded_count(n, world, 2 if g["dt"] == "f16" else 4) for n in NS] for g in X_GROUPS]


def _x_reference(world, nps):
    """Per step: (per group per bucket (p, w, m, v), gate, states), from
    step_gate_ref; nps[g] is what group g's update still divides by."""
    from oracle import oracle
    counts = _x_counts(world)
    cur = []
    for gi, g in enumerate(X_GROUPS):
        rows = []
        for b, (n, L) in enumerate(zip(NS, counts[gi])):
            p = _x_param(g["dt"], n, L, 50 + 10 * gi + b)
            rows.append([p, _x_widen(p, g["dt"]).astype(np.float32), np.zeros(L, np.float32),
                         np.zeros(L, np.float32)])
        cur.append(rows)
    gate = ref.new_gate(X_SCALE0)
    states = [ref.new_state() for _ in X_GROUPS]
    out = []
    for s, lr in enumerate(X_LRS):
        scale = float(gate["loss_scale"])
        red, sq = [], []
        for gi, g in enumerate(X_GROUPS):
            rs, tot = [], 0.0
            for b, (n, L) in enumerate(zip(NS, counts[gi])):
                ins = [_x_grad(g["dt"], n, L, 7000 + 1000 * gi + 100 * s + 10 * b + r, scale,
                               s == X_BAD and gi == 1 and b == 1 and r == world - 1)
                       for r in range(world)]
                if nps[gi] == 0:   # the fold: the average, rounded to the dtype
                    x = oracle.reduce_avg(ins, g["dt"], world)
                else:              # a reduce-scatter: the sum (exact on this grid)
                    with np.errstate(invalid="ignore"):
                        x = np.sum(np.stack(ins).astype(np.float64), axis=0).astype(np.float32)
                rs.append(x)
                tot += ref.sum_sq([x])
            red.append(rs)
            sq.append(tot)
        hs = [_x_hyper(g, lr) for g in X_GROUPS]
        ref.gate_update([sq], nps, hs, states, gate, max_norm=X_MAX_NORM, **X_RULE)
        for gi, g in enumerate(X_GROUPS):
            for b, row in enumerate(cur[gi]):
                if g["dt"] == "f16":
                    p, w, m, v = ref.update_master(row[1], red[gi][b], row[2], row[3], "f16", hs[gi],
                                                   gate, states[gi], nps[gi])
                    cur[gi][b] = [row[0] if p is None else p, w, m, v]
                else:
                    p, m, v = ref.update(row[0], red[gi][b], row[2], row[3], "f32", hs[gi], gate,
                                         states[gi], nps[gi])
                    cur[gi][b] = [p, p, m, v]
        out.append(([[list(r) for r in rows] for rows in cur], dict(gate),
                    [dict(st) for st in states], scale))
    return out


def _x_run(rank, ex, world, scales, got):
    """Three gated steps of the two groups through the exchange's halves."""
    from kungfu_amd import ops
    counts = _x_counts(world)
    P, G, W, M, V = [], [], [], [], []
    for gi, g in enumerate(X_GROUPS):
        dt = g["dt"]
        ps = [_x_param(dt, n, L, 50 + 10 * gi + b) for b, (n, L) in enumerate(zip(NS, counts[gi]))]
        q = [L // world for L in counts[gi]]
        P.append([mgpu._dev16(p, dt) if dt == "f16" else mgpu._dev32(p) for p in ps])
        G.append([torch.zeros_like(t) for t in P[-1]])
        W.append([mgpu._dev32(_x_widen(p, dt)[rank * n:(rank + 1) * n]) for p, n in zip(ps, q)]
                 if dt == "f16" else None)
        M.append([torch.zeros(n, device="cuda") for n in q])
        V.append([torch.zeros(n, device="cuda") for n in q])
    gate, states = ops.new_step_gate("cuda", X_SCALE0), ops.new_step_states("cuda", len(X_GROUPS))
    # one plan per dtype (here: per group), over the fixed shard addresses
    plans = [ops.SegNorm(ex.grad_shards_(G[gi])) for gi in range(len(X_GROUPS))]
    outs = [torch.zeros(len(NS) + 1, dtype=torch.float64, device="cuda") for _ in X_GROUPS]
    sq = torch.zeros(len(X_GROUPS), dtype=torch.float64, device="cuda")
    sq_all = torch.zeros(len(X_GROUPS) * world, dtype=torch.float64, device="cuda")
    nps_seen = None
    for s, lr in enumerate(X_LRS):
        for gi, g in enumerate(X_GROUPS):
            for b, (n, L) in enumerate(zip(NS, counts[gi])):
                a = _x_grad(g["dt"], n, L, 7000 + 1000 * gi + 100 * s + 10 * b + rank, scales[s],
                            s == X_BAD and gi == 1 and b == 1 and rank == world - 1)
                G[gi][b].copy_(mgpu._dev16(a, "f16") if g["dt"] == "f16" else mgpu._dev32(a))
        nps = [ex.reduce_shards_(G[gi]) for gi in range(len(X_GROUPS))]
        assert nps_seen in (None, nps)
        nps_seen = nps
        for gi, plan in enumerate(plans):
            plan.run("sq", out=outs[gi])
            sq[gi:gi + 1].copy_(outs[gi][-1:])
        ex.gather_doubles_(sq, sq_all)
        hs = [_x_hyper(g, lr) for g in X_GROUPS]
        ops.step_gate_update_(sq_all, world, nps, hs, states, gate, max_norm=X_MAX_NORM, **X_RULE)
        for gi in range(len(X_GROUPS)):
            ex.adam_gated_step_(P[gi], G[gi], W[gi], M[gi], V[gi], hs[gi], nps[gi], gate, states, gi)
        torch.cuda.synchronize()
        snap = []
        for gi, g in enumerate(X_GROUPS):
            if g["dt"] == "f16":
                snap.append([(mgpu._host16(p, "f16"), mgpu._host32(w), mgpu._host32(m), mgpu._host32(v))
                             for p, w, m, v in zip(P[gi], W[gi], M[gi], V[gi])])
            else:
                snap.append([(mgpu._host32(p), None, mgpu._host32(m), mgpu._host32(v))
                             for p, m, v in zip(P[gi], M[gi], V[gi])])
        got.setdefault(rank, []).append((snap, _read(gate, states), nps))
    for plan in plans:
        plan.close()


def _x_check(world, got):
    nps = got[0][0][2]
    want = _x_reference(world, nps)
    counts = _x_counts(world)
    for r in range(world):
        for s, ((snap, (gg, gs), nps_r), (cur, gate, states, _)) in enumerate(zip(got[r], want)):
            assert nps_r == nps
            for k in ref.GATE_FIELDS:
                assert _same_scalar(gg[k], gate[k]), ("gate", k, r, s, gg[k], gate[k])
            for j, st in enumerate(states):
                for k in ref.STATE_FIELDS:
                    assert _same_scalar(gs[k][j], st[k]), ("state", k, j, r, s)
            for gi, g in enumerate(X_GROUPS):
                for b, ((p, w, m, v), (wp, ww, wm, wv)) in enumerate(zip(snap[gi], cur[gi])):
                    q = counts[gi][b] // world
                    mine = slice(r * q, (r + 1) * q)
                    where = (r, s, gi, b)
                    if g["dt"] == "f16":
                        assert mgpu._same16(p, wp, "f16"), ("param",) + where
                        assert mgpu._same32(w, ww[mine]), ("master shard",) + where
                    else:
                        assert mgpu._same32(p, wp), ("param",) + where
                    assert mgpu._same32(m, wm[mine]), ("exp_avg shard",) + where
                    assert mgpu._same32(v, wv[mine]), ("exp_avg_sq shard",) + where
        # the skipped step: nothing but the loss scale and the counters has moved
        a, b = got[r][X_BAD - 1], got[r][X_BAD]
        assert b[1][0]["skip"] == 1 and b[1][0]["skipped"] == 1 and b[1][0]["applied"] == X_BAD
        assert float(b[1][0]["loss_scale"]) == X_SCALE0 / 2
        for gi in range(len(X_GROUPS)):
            for x, y in zip(a[0][gi], b[0][gi]):
                for u, v in zip(x, y):
                    assert u is None or u.tobytes() == v.tobytes(), ("moved on a skip", r, gi)
        for k in ref.STATE_FIELDS:
            assert a[1][1][k].tobytes() == b[1][1][k].tobytes(), ("state moved on a skip", k)
    return nps


def _x_scales(world, nps):
    return [w[3] for w in _x_reference(world, nps)]


@pytest.mark.parametrize("world", [2, 3])
def test_native_exchange_gated_step_over_loopback(world):
    """f16 takes the all-to-all and the fold (np = 0), f32 the loopback's
    reduce-scatter (np = world): two plans with different np_k."""
    nps = [0, world]
    scales = _x_scales(world, nps)
    got = {}
    loopback.loop_ranks(world, lambda rank, ex: _x_run(rank, ex, world, scales, got))
    assert _x_check(world, got) == nps


def test_native_exchange_gated_step_rccl1():
    """World 1 through librccl itself: the f32 group's reduce-scatter, np = 1."""
    nps = [0, 1]
    scales = _x_scales(1, nps)
    got = {}
    ex = loopback.rccl1_exchange()
    _x_run(0, ex, 1, scales, got)
    ex.close()
    assert _x_check(1, got) == nps


def test_native_exchange_gated_refusals():
    """The up-front checks of both halves, before any collective."""
    import ctypes
    from kungfu_amd import _lib, ops

    def body(rank, ex):
        if rank:
            return
        x = torch.zeros(64, device="cuda")
        one, null = _lib.ptr_array([x.data_ptr()]), _lib.ptr_array([0])
        h = _lib.adam_hyper_array([adam_ref.hyper(1e-3)])
        gate, st = ops.new_step_gate("cuda"), ops.new_step_states("cuda", 1)
        odd, even = (ctypes.c_size_t * 1)(3), (ctypes.c_size_t * 1)(32)
        np_ = ctypes.c_int(-7)
        red = ex.lib.kf_exchange_reduce_shards_batch
        assert red(ex._h, one, odd, 1, cpu.F32, 0, ctypes.byref(np_), None) == 3
        assert red(ex._h, null, even, 1, cpu.F32, 0, ctypes.byref(np_), None) == 3
        assert red(ex._h, one, even, 1, cpu.F32, 0, None, None) == 3
        assert red(ex._h, one, even, 1, 0x10408, 0, ctypes.byref(np_), None) == 1  # i32
        assert np_.value == -7
        upd = ex.lib.kf_exchange_adam_gated_batch
        args = lambda **kw: [kw.get(k, d) for k, d in (  # noqa: E731
            ("p", one), ("g", one), ("w", None), ("m", one), ("v", one), ("cnt", even), ("nb", 1),
            ("dt", cpu.F32), ("np", 0), ("h", h), ("gate", gate.data_ptr()),
            ("st", st.data_ptr()), ("s", None))]
        assert upd(ex._h, *args(cnt=odd)) == 3
        assert upd(ex._h, *args(m=null)) == 3
        assert upd(ex._h, *args(gate=None)) == 3
        assert upd(ex._h, *args(st=None)) == 3
        assert upd(ex._h, *args(np=-1)) == 3
        assert upd(ex._h, *args(dt=cpu.F16)) == 1           # f16 needs master shards
        assert upd(ex._h, *args(w=one, dt=cpu.F32)) == 1    # master shards need 16 bits
        assert upd(ex._h, *args(w=null, dt=cpu.BF16)) == 3
        assert b"master shard" in ex.lib.kf_exchange_last_error()

    loopback.loop_ranks(2, body)


# ---- the optimizer ------------------------------------------------------------

def test_gated_optimizer_world1_every_exchange():
    """ShardedAdamOptimizer(master_weights=True, max_grad_norm=1.0,
    loss_scale=dynamic) on a two-layer f16 model with one overflow step:
    tests/test_sharded_adam_gated.py's body on the device, over a plain
    NativeExchange (the update over the whole buckets), a one-rank librccl
    communicator and the default collective.Exchange."""
    import test_sharded_adam_gated as gated
    from kungfu_amd.collective import Exchange
    from kungfu_amd.exchange import NativeExchange
    for make in (NativeExchange, loopback.rccl1_exchange, Exchange):
        made = []

        def make_exchange():
            if not made:
                made.append(make())
            return made[0]

        gated.body_gated(0, 1, make_exchange, "cuda")
        if hasattr(made[0], "close"):
            made[0].close()


def test_gated_optimizer_world2_over_loopback():
    import test_sharded_adam_gated as gated
    loopback.loop_ranks(2, lambda rank, ex: gated.body_gated(rank, 2, lambda: ex, "cuda"))
