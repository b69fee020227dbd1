"""ShardedLAMBOptimizer(gate=...) without a GPU: the numpy
restatement of the step under a gate (tests/lamb_gated_ref.py) pinned to
lamb_ref, measured against torch's clip_grad_norm_ + a torch-tensor LAMB, the
construction rules, the declarations, exports and argument checks of the new C
entries (no device touched), and the optimizer end to end over a CPU epilogue
at world 1 and over gloo at worlds 2 and 3."""
import ctypes
import os
import re
import sys
import tempfile
import traceback

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import cpu_epilogue
import lamb_gated_ref as gref
import lamb_ref
import step_gate_ref
import test_sharded_adam_gated as gated
import test_sharded_lamb as lamb
from procs import hung_msg, join_all

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
ROWS = lamb.ROWS
OK, ERR_DTYPE, ERR_ARG = lamb.OK, lamb.ERR_DTYPE, lamb.ERR_ARG
F32, I32, F16, BF16, F64 = lamb.F32, lamb.I32, lamb.F16, lamb.BF16, lamb.F64

# The largest |torch - lamb_gated_ref| measured for (p, m, v) on the data of
# test_gated_restatement_against_torch, per row (DESIGN.md §19's table). p is
# one unit in the last place of the largest elements, as in §17; m and v are
# far below §17's because two of the four gradients are clipped to norm 1 and
# two are smaller still (§16). The test's bounds are four times these.
MEASURED = {(0.0, False): (2.0 ** -22, 1.25 * 2.0 ** -31, 1.125 * 2.0 ** -43),
            (0.0, True): (2.0 ** -22, 1.25 * 2.0 ** -31, 1.125 * 2.0 ** -43),
            (1e-2, False): (2.0 ** -22, 1.25 * 2.0 ** -31, 1.125 * 2.0 ** -43)}


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ---- the restatement -------------------------------------------------------------

def _segment(dt, n=4099):
    C = gref.COMPUTE[dt]
    rng = np.random.default_rng(5)
    p, g, m, u = (rng.standard_normal(n).astype(C) for _ in range(4))
    v = np.square(rng.standard_normal(n)).astype(C)
    return p, g, m, v, u


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_restatement_is_lamb_ref(dt):
    """With skip = 0, grad_mul = 1 and lamb_ref's own scalars as the step
    state, lamb_gated_ref's moments, trust and apply are lamb_ref's, bit for
    bit (x * 1 is x); with skip = 1 every array comes back unchanged."""
    p, g, m, v, u = _segment(dt)
    skip = dict(gref.no_gate(), skip=1)
    for wd in (0.0, 1e-2):
        for np_, step in ((0, 1), (3, 7), (4, 2)):
            h = lamb_ref.hyper(1e-2, weight_decay=wd, step=step)
            want = lamb_ref.moments(p, g, m, v, dt, h, np_)
            got = gref.moments(p, g, m, v, u, dt, h, gref.no_gate(), gref.scalars_of(h), np_)
            for a, b in zip(got, want):
                assert same_bits(a, b), (dt, wd, np_, step)
            kept = gref.moments(p, g, m, v, u, dt, h, skip, gref.scalars_of(h), np_)
            for a, b in zip(kept, (m, v, u)):
                assert same_bits(a, b) and a is not b
    sq = np.random.default_rng(6).random((3, 8)) + 0.5
    lrs, adapts = [0.1, 0.2, 0.3, 0.4], [True, False, True, True]
    old = (np.arange(4.0), np.arange(4.0) + 7)
    for clip in (0.0, 0.9):
        want = lamb_ref.trust(sq, lrs, adapts, clip)
        got = gref.trust(sq, lrs, adapts, *old, gref.no_gate(), clip)
        assert same_bits(got[0], want[0]) and same_bits(got[1], want[1])
        kept = gref.trust(sq, lrs, adapts, *old, skip, clip)
        assert same_bits(kept[0], old[0]) and same_bits(kept[1], old[1])
    assert same_bits(gref.apply(p, u, -0.03, dt, gref.no_gate()), lamb_ref.apply(p, u, -0.03, dt))
    assert same_bits(gref.apply(p, u, -0.03, dt, skip), p)
    if dt == "f32":
        p16 = lamb_ref.narrow16(p, "f16")
        w, q = gref.apply_master(p, p16, u, -0.03, "f16", gref.no_gate())
        assert same_bits(w, lamb_ref.apply(p, u, -0.03, "f32")) and \
            same_bits(q, lamb_ref.narrow16(w, "f16"))
        w, q = gref.apply_master(p, p16, u, -0.03, "f16", skip)
        assert same_bits(w, p) and same_bits(q, p16)
    # the whole of E to G through step_tensors
    h = lamb_ref.hyper(1e-2, weight_decay=1e-2, step=3)
    cuts = [[(0, 1000), (1000, p.size)]]
    want = lamb_ref.step_tensors([p], [g], [m], [v], dt, [h], cuts, 1.7)
    got = gref.step_tensors([p], [g], [m], [v], [u], dt, [h], [gref.scalars_of(h)], gref.no_gate(),
                            cuts, np.zeros(1), np.ones(1), 1.7)
    for a, b in zip(got[:3], want[:3]):
        assert same_bits(a[0], b[0])
    assert same_bits(got[5], want[3])
    kept = gref.step_tensors([p], [g], [m], [v], [u], dt, [h], [gref.scalars_of(h)], skip, cuts,
                             np.zeros(1), np.ones(1), 1.7)
    for a, b in zip(kept, ([p], [m], [v], [u])):
        assert same_bits(a[0], b[0])
    assert same_bits(kept[4], np.zeros(1)) and same_bits(kept[5], np.ones(1))


def test_lr_one_identity():
    """D's rule: a step state advanced with lr = 1 holds nss = -(1 / (1 -
    beta1_pow)), so the gated kernel's rb1 = -nss is the ungated kernel's
    (C)(1 / bias_correction1) bit for bit, in f32 and in f64, for steps 1 to
    50 at betas (0.9, 0.999) where the running product equals beta ** step,
    and s2 likewise."""
    gate, st = gref.new_gate(), [gref.new_state()]
    h = {"lr": 0.37, "betas": (0.9, 0.999)}
    agree = 0
    for t in range(1, 51):
        gref.verdict([[1.0]], [0], [h], st, gate)
        assert st[0]["step"] == t
        for dt, C in (("f32", np.float32), ("f64", np.float64)):
            s2, rb1 = gref.state_scalars(st[0], dt)
            assert rb1.dtype == C and s2.dtype == C
            # the state's own products: always
            assert rb1 == C(1.0 / (1.0 - st[0]["beta1_pow"]))
            assert s2 == C(np.sqrt(1.0 - st[0]["beta2_pow"]))
            assert rb1 == -(C(st[0]["nss_f64"])) and rb1 == -C(-(1.0 / (1.0 - st[0]["beta1_pow"])))
            if st[0]["beta1_pow"] == 0.9 ** t:  # then also the host's scalars
                want = gref.scalars_of(dict(h, step=t))
                assert rb1 == C(1.0 / (1.0 - 0.9 ** t)) == gref.state_scalars(want, dt)[1]
                agree += 1
    assert agree >= 20, agree
    # lamb_ref's rb1 at lr = 1 is what scalars_of states
    for t in (1, 3, 50):
        st1 = gref.scalars_of({"lr": 5.0, "betas": (0.9, 0.999), "step": t})
        assert st1["nss_f64"] == -(1.0 / (1.0 - 0.9 ** t))
        assert np.float32(-st1["nss"]) == np.float32(1.0 / (1.0 - 0.9 ** t))


# ---- against torch ------------------------------------------------------------------

def _torch_lamb_step(p, g, m, v, lr, wd, adapt, step, betas=(0.9, 0.999), eps=1e-6):
    """tests/test_sharded_lamb.py's torch-tensor LAMB (apex FusedLAMB's
    formulation, bias correction on), restated; the clipping comes before it."""
    b1, b2 = betas
    m.mul_(b1).add_(g, alpha=1 - b1)
    v.mul_(b2).addcmul_(g, g, value=1 - b2)
    u = (m / (1 - b1 ** step)) / ((v / (1 - b2 ** step)).sqrt() + eps)
    if wd != 0:
        u = u + wd * p
    wn, un = p.double().norm(), u.double().norm()
    ratio = float(wn / un) if adapt and wn > 0 and un > 0 else 1.0
    p.add_(u, alpha=-lr * ratio)


@pytest.mark.parametrize("wd,always_adapt", ROWS)
def test_gated_restatement_against_torch(wd, always_adapt):
    """lamb_gated_ref (verdict, then E to G) against torch on CPU:
    clip_grad_norm_(max_norm = 1) followed by the torch-tensor LAMB above, on
    DESIGN.md §17's inputs (100003 standard-normal elements, 4 steps, lr
    changed every step). The gradients are scaled by (0.001, 1, 0.002, 3) as
    in §16: their norms are about 0.32, 316, 0.63 and 949, so the clip is
    active on steps 2 and 4 and idle on 1 and 3. A fifth gradient, in second
    place, carries one inf: both sides skip it, and the steps after it use the
    step counts of an uninterrupted run. Not bit-exact, for §17's reasons and
    because torch computes the norm and the clip factor in fp32. MEASURED has
    the largest absolute differences of (p, m, v) after the 4 applied steps;
    each bound is four times the measured value."""
    n = 100003
    lrs = (1e-3, 7e-4, 5e-4, 2e-3, 1e-4)
    scales = (0.001, None, 1.0, 0.002, 3.0)
    rng = np.random.default_rng(7)
    p0 = rng.standard_normal(n).astype(np.float32)
    grads = []
    for s in scales:
        g = rng.standard_normal(n).astype(np.float32)
        if s is None:
            g[n // 3] = np.inf
        else:
            g = (g * np.float32(s)).astype(np.float32)
        grads.append(g)
    adapt = wd != 0 or always_adapt
    tp = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    tm, tv = torch.zeros(n), torch.zeros(n)
    p, m, v, u = p0.copy(), np.zeros(n, np.float32), np.zeros(n, np.float32), np.zeros(n, np.float32)
    nlr, ratio = np.zeros(1), np.ones(1)
    gate, st = gref.new_gate(), [gref.new_state()]
    clipped, applied = [], 0
    for lr, g in zip(lrs, grads):
        tp.grad = torch.from_numpy(g.copy())
        norm = torch.nn.utils.clip_grad_norm_([tp], 1.0, foreach=False)
        if bool(torch.isfinite(norm)):
            applied += 1
            with torch.no_grad():
                _torch_lamb_step(tp, tp.grad, tm, tv, lr, wd, adapt, applied)
        h = dict(lamb_ref.hyper(lr, weight_decay=wd, adapt=adapt))
        gref.verdict([[step_gate_ref.sum_sq([g])]], [0], [h], st, gate, max_norm=1.0)
        assert gate["skip"] == int(not bool(torch.isfinite(norm)))
        if not gate["skip"]:
            assert abs(gate["grad_norm"] - float(norm)) <= 1e-5 * float(norm)
            clipped.append(float(gate["grad_mul"]) < 1.0)
        (p,), (m,), (v,), (u,), nlr, ratio = gref.step_tensors(
            [p], [g], [m], [v], [u], "f32", [h], st, gate, [[(0, n)]], nlr, ratio)
    assert clipped == [False, True, False, True] and gate["skipped"] == 1 and st[0]["step"] == 4
    diffs = [float(np.max(np.abs(a - b))) for a, b in
             ((tp.detach().numpy(), p), (tm.numpy(), m), (tv.numpy(), v))]
    print("max |torch - lamb_gated_ref| after 4 applied steps (p, m, v): %.6g %.6g %.6g"
          % tuple(diffs))
    for d, measured, what in zip(diffs, MEASURED[(wd, always_adapt)], "pmv"):
        assert d <= 4 * measured, (what, d, measured)


# ---- construction ------------------------------------------------------------------------

def _gated_exchange():
    from kungfu_amd.collective import Exchange
    return Exchange(epilogue=CpuLambGatedEpilogue())


def test_construction_rules():
    from kungfu_amd import optimizers as kopt
    from kungfu_amd.torch import optimizers as topt
    lin = torch.nn.Linear(5, 3)
    new = lambda **kw: kopt.ShardedLAMBOptimizer(  # noqa: E731
        torch.optim.AdamW(lin.parameters(), lr=1e-3), **kw)
    # refused forms of gate=
    for bad in ({}, [], "dynamic", 1.0, True, ("max_grad_norm", 1.0), {"max_norm": 1.0},
                {"max_grad_norm": 1.0, "scale": 2.0}, {"max_grad_norm": None},
                {"max_grad_norm": None, "loss_scale": None}):
        with pytest.raises(ValueError, match="gate"):
            new(gate=bad)
    for bad in (0, -1.0, float("inf"), float("nan"), "1.0", True):
        with pytest.raises(ValueError, match="ShardedLAMBOptimizer: max_grad_norm"):
            new(gate={"max_grad_norm": bad})
    for bad in (0, -2.0, float("inf"), float("nan"), "static", True, {"scale": 2.0},
                {"init_scale": 0}, {"growth_interval": -1}, {"growth_interval": 2.5},
                {"backoff_factor": "half"}):
        with pytest.raises(ValueError, match="ShardedLAMBOptimizer: loss_scale"):
            new(gate={"loss_scale": bad})
    # Adam's texts are its own still
    with pytest.raises(ValueError, match="ShardedAdamOptimizer: max_grad_norm"):
        kopt.ShardedAdamOptimizer(torch.optim.AdamW(lin.parameters(), lr=1e-3), max_grad_norm=0)
    # the old keywords are still refused, and point to gate=
    for kw in ({"max_grad_norm": 1.0}, {"loss_scale": "dynamic"}):
        with pytest.raises(ValueError, match="gated") as e:
            new(**kw)
        assert "gate=" in str(e.value)
    # accepted forms, and their rules
    static = {"init_scale": 1.0, "growth_factor": 1.0, "backoff_factor": 1.0, "growth_interval": 0}
    o = new(gate={"max_grad_norm": 2})
    assert o._kf_gated and o._kf_max_norm == 2.0 and o._kf_rule == static
    o = new(gate={"loss_scale": 128})
    assert o._kf_gated and o._kf_max_norm == 0.0 and o._kf_rule == dict(static, init_scale=128.0)
    o = new(gate={"loss_scale": "dynamic"})
    assert o._kf_rule == {"init_scale": 65536.0, "growth_factor": 2.0, "backoff_factor": 0.5,
                          "growth_interval": 2000}
    o = new(gate={"max_grad_norm": 1.0, "loss_scale": {"growth_interval": 7}})
    assert o._kf_max_norm == 1.0 and o._kf_rule["growth_interval"] == 7
    o = new(gate={"max_grad_norm": 0.5, "loss_scale": None})
    assert o._kf_gated and o._kf_rule == static
    # without a gate: today's path, and the accessors raise with the optimizer's name
    o = new()
    assert not o._kf_gated
    for call in (o.loss_scale_value, o.skipped_steps, o.applied_steps, o.last_grad_norm,
                 o.scaler_state, lambda: o.load_scaler_state({"loss_scale": 1.0, "good_steps": 0}),
                 lambda: o.scale_loss(torch.ones(()))):
        with pytest.raises(ValueError, match=r"ShardedLAMBOptimizer\.\w+( \w+)? needs gate="):
            call()
    # an exchange without the half-step methods is refused, gated or not
    with pytest.raises(ValueError, match="gather_params_"):
        new(exchange=lamb._NoGatherExchange(), gate={"max_grad_norm": 1.0})
    # f16 without master weights stays a TypeError under a gate
    p = torch.nn.Parameter(torch.zeros(8, dtype=torch.float16))
    o = kopt.ShardedLAMBOptimizer(torch.optim.Adam([p], lr=1e-3), exchange=_gated_exchange(),
                                  gate={"max_grad_norm": 1.0, "loss_scale": "dynamic"})
    p.grad = torch.zeros_like(p)
    with pytest.raises(TypeError, match="master_weights=True"):
        o.step()
    # through the torch-style constructor's **kwargs; scale_loss before the first step
    q = torch.nn.Parameter(torch.ones(8, dtype=torch.float16))
    o = topt.ShardedLAMBOptimizer(torch.optim.AdamW([q], lr=1e-3), [("q", q)], master_weights=True,
                                  exchange=_gated_exchange(), gate={"loss_scale": 4.0})
    assert o._kf_gated and o.loss_scale_value() == 4.0
    assert float(o.scale_loss(torch.tensor(1.5))) == 6.0
    assert "gate" in topt.ShardedLAMBOptimizer.__doc__
    doc = kopt.ShardedLAMBOptimizer.__doc__
    for words in ("gate: None, or a dict", '"max_grad_norm"', '"loss_scale"', "scale_loss()",
                  "skipped_steps()", "load_scaler_state()", "is skipped", "running",
                  "Non-finite gradients are not skipped", "behaviour without a gate",
                  "overlap=True", "hierarchical"):
        assert words in doc, words


# ---- declarations, exports, argument errors (no device) -------------------------------------

NEW_ENTRIES = ("kf_lamb_moments_batch_gated", "kf_lamb_master_moments_batch_gated",
               "kf_lamb_trust_update_gated", "kf_lamb_apply_run_gated")
NEW_KERNELS = ("lamb_moments_gated_kernel", "lamb_master_moments_gated_kernel",
               "lamb_trust_gated_kernel", "lamb_apply_gated_kernel",
               "lamb_master_apply_gated_kernel")


def test_entries_declared_and_exported():
    from kungfu_amd import _lib, collective, ops
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "kungfu_amd.h")).read()
    assert "LAMB under a gate" in hdr
    for name in NEW_ENTRIES:
        assert re.search(r"^int %s\(" % name, hdr, re.M), name
        assert name in _lib.EXPORTED and getattr(lib, name) is not None
    for name in ("lamb_moments_batch_gated_", "lamb_master_moments_batch_gated_",
                 "lamb_trust_update_gated_"):
        assert callable(getattr(ops, name))
    for name in ("lamb_moments_gated_", "lamb_master_moments_gated_", "lamb_trust_update_gated_"):
        assert callable(getattr(collective.HipEpilogue, name))
    src = open(os.path.join(ROOT, "kungfu_amd", "csrc", "kf_lamb.hip")).read()
    for k in NEW_KERNELS:
        assert re.search(r"\b%s\(" % k, src), k
    assert src.count("if (adam_gate_load(gate, st, gt)) return;") == 2
    assert src.count("__builtin_amdgcn_sched_barrier(0);") == 2  # the two tile loops, shared
    assert "asm" not in src
    math = open(os.path.join(ROOT, "kungfu_amd", "csrc", "kf_lamb_math.hpp")).read()
    # the one inserted operation, directly after the /np
    assert re.search(r"g\[i\] = SgdDiv<T, DIV>::run\(g\[i\], d\);\s*if constexpr \(GATE::on\) \{\s*"
                     r"#pragma unroll\s*for \(int i = 0; i < H; \+\+i\) g\[i\] = g\[i\] \* gate\.mul;",
                     math)
    assert "return -gate.nss;" in math and "typename GATE = AdamNoGate" in math


def test_gated_entries_arg_errors():
    """Every check of the new entries comes before any HIP call."""
    from kungfu_amd import _lib
    lib = _lib.load()
    pa = _lib.ptr_array
    cnt = lambda *v: (ctypes.c_size_t * len(v))(*v)  # noqa: E731
    h = _lib.adam_hyper_array([lamb_ref.hyper(1e-3)])
    h[0].bias_correction1 = h[0].bias_correction2 = float("nan")  # ignored by the gated entries
    five = (pa([16]), pa([32]), pa([48]), pa([64]), pa([80]))
    for fn, good, bad in ((lib.kf_lamb_moments_batch_gated, F32, (F16, BF16, I32)),
                          (lib.kf_lamb_master_moments_batch_gated, F16, (F32, F64, I32))):
        call = lambda t, c, nb, dt=good, np_=0, hyper=h, gate=96, st=128: \
            fn(*t, c, nb, dt, np_, hyper, gate, st, None)  # noqa: E731
        assert call((None,) * 5, None, 0) == OK
        assert call((None,) * 5, None, 0, gate=None, st=None) == OK
        assert call(five, cnt(0), 1) == OK
        assert call(five, cnt(4), -1) == ERR_ARG
        assert call(five, cnt(4), 1, gate=None) == ERR_ARG
        assert b"gate" in lib.kf_last_error() and b"_gated" in lib.kf_last_error()
        assert call(five, cnt(4), 1, st=None) == ERR_ARG
        for i in range(5):
            t = list(five)
            t[i] = None
            assert call(t, cnt(4), 1) == ERR_ARG, i
            t[i] = pa([0])
            assert call(t, cnt(4), 1) == ERR_ARG, i
            t[i] = pa([16 * (i + 1) + 8])
            assert call(t, cnt(4), 1) == ERR_ARG, i
            assert b"16-byte" in lib.kf_last_error() and b"_gated" in lib.kf_last_error()
        assert call(five, None, 1) == ERR_ARG and call(five, cnt(4), 1, hyper=None) == ERR_ARG
        assert call(five, cnt(4), 1, np_=-1) == ERR_ARG
        for dt in bad:
            assert call(five, cnt(4), 1, dt=dt) == ERR_DTYPE, hex(dt)
    groups = (_lib.LambGroup * 1)()
    trust = lib.kf_lamb_trust_update_gated
    assert trust(8, 0, 1, 8, groups, 1, 0.0, 8, 8, 96, None) == ERR_ARG   # world < 1
    assert trust(8, 1, 0, 8, groups, 1, 0.0, 8, 8, 96, None) == ERR_ARG   # no tensor
    assert trust(8, 1, 1, 8, groups, 0, 0.0, 8, 8, 96, None) == ERR_ARG   # no group
    assert trust(None, 1, 1, 8, groups, 1, 0.0, 8, 8, 96, None) == ERR_ARG
    assert trust(8, 1, 1, 8, None, 1, 0.0, 8, 8, 96, None) == ERR_ARG
    assert trust(8, 1, 1, 8, groups, 1, 0.0, None, 8, 96, None) == ERR_ARG
    assert trust(8, 1, 1, 8, groups, 1, float("nan"), 8, 8, 96, None) == ERR_ARG
    assert trust(8, 1, 1, 8, groups, 1, 0.0, 8, 8, None, None) == ERR_ARG  # no gate
    assert b"kf_lamb_trust_update_gated" in lib.kf_last_error()
    run = lib.kf_lamb_apply_run_gated
    assert run(None, 8, 96, None) == ERR_ARG
    assert run(1 << 12, None, 96, None) == ERR_ARG
    assert run(1 << 12, 8, None, None) == ERR_ARG
    assert b"kf_lamb_apply_run_gated" in lib.kf_last_error()


# ---- the optimizer: an f32 group and an f16 master group, an overflow step -----------------

class _CpuGatedApply(lamb._CpuApply):
    def run(self, nlr, gate=None):
        if gate is not None and gated.read_gate(gate)["skip"]:
            return
        super().run(nlr)


class CpuLambGatedEpilogue(lamb.CpuLambEpilogue, gated.CpuGatedEpilogue):
    """test_sharded_lamb's and test_sharded_adam_gated's CPU epilogues plus the
    gated LAMB passes, from lamb_gated_ref. The gate and the step states are
    the same bytes as on the device, in CPU tensors."""

    def sq_norm_plan(self, tensors):  # the gated one: 16-bit gradient shards too
        return gated.CpuGatedEpilogue._Plan(tensors)

    def _gated_moments(self, wide_g, ps, ms, vs, us, hyper, gate, states, group, np_):
        g, st = gated.read_gate(gate), gated.read_states(states)[group]
        for p, gr, m, v, u in zip(ps, wide_g, ms, vs, us):
            dt = "f64" if p.dtype == torch.float64 else "f32"
            new = gref.moments(p.numpy(), gr, m.numpy().copy(), v.numpy().copy(), u.numpy().copy(),
                               dt, hyper, g, st, np_)
            for t, a in zip((m, v, u), new):
                t.numpy()[...] = a
        return us

    def lamb_moments_gated_(self, params, grads, exp_avgs, exp_avg_sqs, updates, hyper, gate,
                            states, group, np_):
        assert "step" not in hyper
        return self._gated_moments([g.numpy() for g in grads], params, exp_avgs, exp_avg_sqs,
                                   updates, hyper, gate, states, group, np_)

    def lamb_master_moments_gated_(self, grads16, masters, exp_avgs, exp_avg_sqs, updates, hyper,
                                   gate, states, group, np_):
        assert "step" not in hyper
        wide = [lamb_ref.widen16(cpu_epilogue._np(g).view(np.uint16),
                                 "bf16" if g.dtype == torch.bfloat16 else "f16") for g in grads16]
        return self._gated_moments(wide, masters, exp_avgs, exp_avg_sqs, updates, hyper, gate,
                                   states, group, np_)

    def lamb_trust_update_gated_(self, sq, world, group_of, groups, nlr, ratio, gate,
                                 trust_clip=0.0):
        if gated.read_gate(gate)["skip"]:
            return nlr
        return self.lamb_trust_update_(sq, world, group_of, groups, nlr, ratio, trust_clip)

    def lamb_apply_plan(self, params, updates, tensors, ntensor, params16=None):
        return _CpuGatedApply(params, updates, tensors, ntensor, params16)


# test_sharded_lamb's model (NUMELS as f32, group 0; NUMELS as f16 with master
# weights, group 1) with betas whose cube is the running product
# (test_sharded_adam_gated's), a dynamic loss scale and a clip at norm 1. The
# gradients are integers in [-8, 8] times world / 4 times the loss scale (a
# power of two): every sum over the ranks, the division by the world and every
# sum of squares are exact in any order, so the verdict's reference needs no
# knowledge of which rank holds which shard. Step G_BAD carries one inf on
# the last rank only; step G_SMALL is scaled by 2^-8 and is not clipped.
NUMELS = lamb.NUMELS
G_HYPER = ({"lr": 0.05, "weight_decay": 1e-2, "betas": (0.9, 0.999), "eps": 1e-6},
           {"lr": 0.02, "weight_decay": 0.0, "betas": (0.8, 0.95), "eps": 1e-6})
G_SCALE = {"init_scale": 1024.0, "growth_interval": 2}
G_STEPS, G_BAD, G_SMALL, G_MAX_NORM = 4, 1, 3, 1.0
G_GATE = {"max_grad_norm": G_MAX_NORM, "loss_scale": dict(G_SCALE)}
TRUST_CLIP, BUCKET_BYTES = lamb.TRUST_CLIP, lamb.BUCKET_BYTES


def g_grads(world, step, scale, sixteen="f16"):
    """[rank][param]: the scaled gradients as the backward pass of
    scale_loss(loss) would leave them."""
    k = len(NUMELS)
    mul = np.float32(world / 4.0) * np.float32(scale) * np.float32(2.0 ** -8 if step == G_SMALL else 1)
    out = []
    for r in range(world):
        rng = np.random.default_rng(11 + 100 * step + r)
        gs = [rng.integers(-8, 9, n).astype(np.float32) * mul for n in NUMELS * 2]
        if step == G_BAD and r == world - 1:
            gs[k + 2][5] = np.inf
        out.append(gs[:k] + [lamb_ref.narrow16(g, sixteen) for g in gs[k:]])
    return out


def g_optimizer(exchange, device="cpu", sixteen="f16", gate=G_GATE, arrays=None):
    from kungfu_amd.optimizers import ShardedLAMBOptimizer
    arrays = lamb.model_arrays(sixteen) if arrays is None else arrays
    ps = [torch.nn.Parameter(lamb.to_torch(a, sixteen).to(device)) for a in arrays]
    k = len(NUMELS)
    groups = [dict(G_HYPER[0], params=ps[:k]), dict(G_HYPER[1], params=ps[k:])]
    kw = {} if gate is None else {"gate": gate}
    opt = ShardedLAMBOptimizer(torch.optim.AdamW(groups, lr=0.1), exchange=exchange,
                               bucket_bytes=BUCKET_BYTES, master_weights=True,
                               trust_clip=TRUST_CLIP, **kw)
    return ps, opt


def g_run(ps, opt, world, rank, scales, device="cpu", first_step=0, steps=G_STEPS, sixteen="f16"):
    """`scales`: the reference's loss scale per step (asserted against the
    device's on the way)."""
    for s in range(first_step, first_step + steps):
        if opt._kf_gated:
            assert float(opt.scale_loss(torch.ones((), device=device))) == scales[s]
        for p, g in zip(ps, g_grads(world, s, scales[s], sixteen)[rank]):
            p.grad = lamb.to_torch(g, sixteen).to(device)
        opt.step()
        lamb.schedule(opt)


_G_REFERENCE = {}


def g_reference(world, cuts, steps=G_STEPS, sixteen="f16", sums=None):
    """The model after `steps` steps by lamb_gated_ref on the unsharded
    tensors: oracle.reduce_avg of the ranks' gradients, one verdict per step
    over the two dtypes' plans, the lr halved after every step, the (p, u) norm
    sums taken per shard (cuts: test_sharded_lamb.model_cuts') and added in
    rank order, or the device's own (sums[step][group] of [world][2T]).
    Computed once per CPU case and shared; callers leave it unchanged."""
    key = (world, steps, sixteen)
    if sums is None and key in _G_REFERENCE:
        return _G_REFERENCE[key]
    from oracle import oracle
    k = len(NUMELS)
    arrs = lamb.model_arrays(sixteen)
    w = [a.copy() for a in arrs[:k]] + [lamb_ref.widen16(a, sixteen) for a in arrs[k:]]
    ms, vs, us = ([np.zeros(a.size, np.float32) for a in w] for _ in range(3))
    nlr, ratio = [np.zeros(k), np.zeros(k)], [np.ones(k), np.ones(k)]
    rule = dict(growth_factor=2.0, backoff_factor=0.5, growth_interval=G_SCALE["growth_interval"])
    gate, states = gref.new_gate(G_SCALE["init_scale"]), [gref.new_state() for _ in G_HYPER]
    scales, norms, lr_scale = [], [], 1.0
    for s in range(steps):
        scales.append(float(gate["loss_scale"]))
        gr = g_grads(world, s, scales[-1], sixteen)
        avg = []
        for j in range(2 * k):
            ins = [np.ascontiguousarray(gr[r][j]) for r in range(world)]
            if j < k:
                avg.append(oracle.reduce_avg(ins, "f32", world))
            else:
                ins = [x.view(np.float16) if sixteen == "f16" else x for x in ins]
                a = oracle.reduce_avg(ins, sixteen, world)
                avg.append(lamb_ref.widen16(np.asarray(a).view(np.uint16), sixteen))
        hs = [lamb_ref.hyper(h["lr"] * lr_scale, betas=h["betas"], eps=h["eps"],
                             weight_decay=h["weight_decay"]) for h in G_HYPER]
        # one plan per dtype, in group order; their sums of squares are exact
        sq = [[step_gate_ref.sum_sq(avg[:k]), step_gate_ref.sum_sq(avg[k:])]]
        gref.verdict(sq, [0, 0], hs, states, gate, max_norm=G_MAX_NORM, **rule)
        norms.append(gate["grad_norm"])
        for gi, idx in enumerate((list(range(0, k)), list(range(k, 2 * k)))):
            new = gref.step_tensors(
                [w[j] for j in idx], [avg[j] for j in idx], [ms[j] for j in idx],
                [vs[j] for j in idx], [us[j] for j in idx], "f32", [hs[gi]] * k, [states[gi]] * k,
                gate, cuts[gi], nlr[gi], ratio[gi], TRUST_CLIP,
                sums=None if sums is None else sums[s][gi])
            for i, j in enumerate(idx):
                w[j], ms[j], vs[j], us[j] = new[0][i], new[1][i], new[2][i], new[3][i]
            nlr[gi], ratio[gi] = new[4], new[5]
        lr_scale *= 0.5
    out = {"p": w[:k] + [lamb_ref.narrow16(a, sixteen) for a in w[k:]], "m": ms, "v": vs,
           "w": [None] * k + w[k:], "ratio": [float(x) for x in ratio[0]] + [float(x) for x in ratio[1]],
           "gate": gate, "states": states, "scales": scales, "norms": norms}
    if sums is None:
        _G_REFERENCE[key] = out
    return out


def g_check(ps, opt, want, steps):
    """Parameters, ratios, state, master, gate and step states, bit for bit."""
    sb = opt.state_buffers()
    assert set(sb) == {p for p in ps if p.numel()}
    ratios = opt.last_trust_ratios()
    for j, p in enumerate(ps):
        assert same_bits(lamb.to_numpy(p), want["p"][j]), ("param", j)
        assert ratios[p] == want["ratio"][j], ("ratio", j)
        if p.numel() == 0:
            continue
        assert sb[p]["step"] == steps
        assert same_bits(sb[p]["exp_avg"].cpu().numpy().reshape(-1), want["m"][j]), ("m", j)
        assert same_bits(sb[p]["exp_avg_sq"].cpu().numpy().reshape(-1), want["v"][j]), ("v", j)
        if want["w"][j] is not None:
            assert same_bits(sb[p]["master"].cpu().numpy().reshape(-1), want["w"][j]), ("w", j)
    got = gated.read_gate(opt._kf_gate)
    for f in step_gate_ref.GATE_FIELDS:
        a, b = np.asarray(got[f]), np.asarray(want["gate"][f]).astype(np.asarray(got[f]).dtype)
        assert a.tobytes() == b.tobytes(), (f, got[f], want["gate"][f])
    got_s = gated.read_states(opt._kf_gstates)
    for j, st in enumerate(want["states"]):
        for f in step_gate_ref.STATE_FIELDS:
            a, b = np.asarray(got_s[j][f]), np.asarray(st[f]).astype(np.asarray(got_s[j][f]).dtype)
            assert a.tobytes() == b.tobytes(), (f, j, got_s[j][f], st[f])
    g = want["gate"]
    assert opt.skipped_steps() == g["skipped"] and opt.applied_steps() == g["applied"]
    assert opt.loss_scale_value() == float(g["loss_scale"])
    assert opt.last_grad_norm() == g["grad_norm"]
    assert opt.scaler_state() == {"loss_scale": float(g["loss_scale"]),
                                  "good_steps": g["good_steps"]}
    return sb


def _snapshot(ps, opt):
    sb = opt.state_buffers()
    return ([lamb.to_numpy(p) for p in ps],
            {j: {f: (x if f == "step" else lamb.to_numpy(x)) for f, x in sb[p].items()}
             for j, p in enumerate(ps) if p in sb},
            [[lamb.to_numpy(u) for u in G["u"]] for G in opt._kf_groups],
            [(lamb.to_numpy(L["nlr"]), lamb.to_numpy(L["ratio"])) for L in opt._kf_lamb],
            lamb.to_numpy(opt._kf_gstates))


def body_gated(rank, world, make_exchange=_gated_exchange, device="cpu"):
    """What the CPU and the GPU end-to-end tests share: the gated run against
    the reference, the skipped step, the checkpoint round trip."""
    ps, opt = g_optimizer(make_exchange(), device)
    opt._kf_build_sharded()
    cuts = lamb.model_cuts(opt, world)
    want = g_reference(world, cuts)
    scales = want["scales"]
    assert scales == [1024.0, 1024.0, 512.0, 512.0] and want["gate"]["skipped"] == 1
    assert float(want["gate"]["loss_scale"]) == 1024.0  # growth after two good steps
    # the clip: active wherever the norm is above 1, idle on the small step
    assert all(n > 1.0 for s, n in enumerate(want["norms"]) if s not in (G_BAD, G_SMALL))
    assert want["norms"][G_SMALL] < 1.0 and not np.isfinite(want["norms"][G_BAD])
    # the step before the bad one, then the bad one: nothing but the loss
    # scale and the counters moves
    g_run(ps, opt, world, rank, scales, device, steps=G_BAD)
    before = _snapshot(ps, opt)
    g_run(ps, opt, world, rank, scales, device, first_step=G_BAD, steps=1)
    after = _snapshot(ps, opt)
    assert opt.skipped_steps() == 1 and opt.applied_steps() == G_BAD
    assert opt.loss_scale_value() == 512.0 and not np.isfinite(opt.last_grad_norm())
    for j in range(len(ps)):
        assert same_bits(before[0][j], after[0][j]), ("param moved on a skip", j)
        for f in before[1].get(j, {}):
            if f == "step":
                assert before[1][j][f] == after[1][j][f] == G_BAD
            else:
                assert same_bits(before[1][j][f], after[1][j][f]), (f, j)
    for a, b in zip(before[2], after[2]):
        assert all(same_bits(x, y) for x, y in zip(a, b)), "u moved on a skip"
    for a, b in zip(before[3], after[3]):
        assert same_bits(a[0], b[0]) and same_bits(a[1], b[1]), "nlr / ratio moved on a skip"
    assert same_bits(before[4], after[4]), "a step state moved on a skip"
    g_run(ps, opt, world, rank, scales, device, first_step=G_BAD + 1, steps=G_STEPS - G_BAD - 1)
    assert len(opt.state) == 0
    sb = g_check(ps, opt, want, G_STEPS - 1)
    k = len(NUMELS)
    assert all(want["ratio"][j] == 1.0 for j in range(k, 2 * k))     # no decay: no adapting
    assert any(want["ratio"][j] not in (1.0, TRUST_CLIP) for j in range(k))
    # save, reload into a fresh optimizer, and both go on with the same bits
    sc = opt.scaler_state()
    qs, opt2 = g_optimizer(make_exchange(), device, arrays=[lamb.to_numpy(p) for p in ps])
    for g2, g in zip(opt2.param_groups, opt.param_groups):
        g2["lr"] = g["lr"]
    opt2.load_state_buffers({q: sb[p] for p, q in zip(ps, qs) if p in sb})
    opt2.load_scaler_state(sc)
    assert opt2.scaler_state() == sc and opt2.skipped_steps() == 0
    assert {b["step"] for b in opt2.state_buffers().values()} == {G_STEPS - 1}
    more = g_reference(world, cuts, G_STEPS + 1)
    g_run(ps, opt, world, rank, more["scales"], device, first_step=G_STEPS, steps=1)
    g_run(qs, opt2, world, rank, more["scales"], device, first_step=G_STEPS, steps=1)
    g_check(ps, opt, more, G_STEPS)
    sb1, sb2 = opt.state_buffers(), opt2.state_buffers()
    for j, (p, q) in enumerate(zip(ps, qs)):
        assert same_bits(lamb.to_numpy(p), lamb.to_numpy(q)), ("reload", j)
        for f in sb1.get(p, {}):
            if f == "step":
                assert sb1[p][f] == sb2[q][f] == G_STEPS
            else:
                assert same_bits(lamb.to_numpy(sb1[p][f]), lamb.to_numpy(sb2[q][f])), (f, j)


def test_reload_pows_are_the_running_products_here():
    """body_gated's reload compares bit for bit: for these betas and three
    applied steps Python's beta ** 3 is the running product."""
    for h in G_HYPER:
        for b in h["betas"]:
            assert b ** 3 == b * b * b


def test_ungated_path_is_untouched():
    """gate=None: the optimizer calls today's epilogue methods and none of the
    gated ones, and its result is test_sharded_lamb's reference's bits."""
    called = []

    class Spy(CpuLambGatedEpilogue):
        def __getattribute__(self, name):
            if name.startswith("lamb_") or name == "step_gate_update_":
                called.append(name)
            return object.__getattribute__(self, name)

    from kungfu_amd.collective import Exchange
    ps, opt = lamb.make_optimizer(Exchange(epilogue=Spy()))
    assert not opt._kf_gated
    for s in range(lamb.STEPS):
        lamb.set_grads(ps, 1, 0, s)
        opt.step()
        lamb.schedule(opt)
    assert called and not [n for n in called if "gated" in n or n == "step_gate_update_"]
    lamb.check_against_reference(ps, opt, lamb.reference_run(1, cuts=lamb.model_cuts(opt, 1)))


def test_world1_gated_optimizer_and_checkpoint():
    """The whole of body_gated in this process: no process group, world 1."""
    body_gated(0, 1)


def _entry(rank, world, store, errq):
    sys.path[:0] = [ROOT, HERE]
    try:
        dist.init_process_group("gloo", init_method="file://" + store, rank=rank,
                                world_size=world)
        import test_sharded_lamb_gated as mod
        mod.body_gated(rank, world)
        dist.barrier()
    except Exception:
        errq.put("rank %d: %s" % (rank, traceback.format_exc()))
        raise
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_gated_optimizer_over_gloo(world):
    ctx = mp.get_context("spawn")
    errq = ctx.SimpleQueue()
    store = os.path.join(tempfile.mkdtemp(prefix="kflambg"), "store")
    procs = [ctx.Process(target=_entry, args=(r, world, store, errq)) for r in range(world)]
    for p in procs:
        p.start()
    hung = join_all(procs, 600)
    errs = []
    while not errq.empty():
        errs.append(errq.get())
    assert not errs, "\n".join(errs)
    assert not hung and all(p.exitcode == 0 for p in procs), hung_msg(hung, [p.exitcode for p in procs])
