"""ShardedAdamOptimizer(master_weights=True) without a GPU: the numpy
restatement (tests/adam_master_ref.py) on the case that motivates it and
against torch.optim.Adam / AdamW on an fp32 copy, the construction rules, the
argument checks of both C entries (no device touched), and the whole
reduce-scatter -> update -> all-gather step with its checkpoint path over gloo
with a CPU epilogue."""
import ctypes
import os
import sys
import tempfile
import traceback

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import adam_master_ref
import adam_ref
import cpu_epilogue
import test_sharded_adam as base
from procs import hung_msg, join_all

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

ROWS = base.ROWS

# The largest |torch - adam_master_ref| measured for (master, m, v) on the data
# of test_restatement_against_torch, per row: one to three units in the last
# place of the largest elements (2^-22 = 2.38e-7, 2^-23 = 1.19e-7,
# 2^-29 = 1.86e-9, 3 * 2^-29 = 5.59e-9). The arithmetic is adam_ref's f32 path
# and DESIGN.md §14's table for it was the expectation; on these bf16-rounded
# inputs the master is one place worse than §14's p in two rows and v is
# 3 * 2^-29 where §14 has 2^-28. The test's bounds are four times these.
MEASURED = {(0.0, False): (2.0 ** -22, 2.0 ** -23, 2.0 ** -29),
            (1e-2, False): (2.0 ** -22, 2.0 ** -23, 3 * 2.0 ** -29),
            (1e-2, True): (2.0 ** -22, 2.0 ** -23, 2.0 ** -29)}


# ---- the restatement ---------------------------------------------------------

def test_updates_below_half_an_ulp_accumulate_in_the_master():
    """p = 1.0, g = 1.0, lr = 1e-3, default betas, 50 steps. Every update is
    below half a bf16 ulp of 1.0 (2^-9): adam_ref's bf16 path rounds each one
    away and stays at exactly 1.0; the master reaches 0.95000064 and the
    parameter is its narrowing, 0.94921875."""
    one = adam_ref.f32_to_bf16_bits(np.ones(1, np.float32))
    p, m, v = one.copy(), np.zeros(1, np.uint16), np.zeros(1, np.uint16)
    w, wm, wv = np.ones(1, np.float32), np.zeros(1, np.float32), np.zeros(1, np.float32)
    p16 = one.copy()
    for t in range(1, 51):
        h = adam_ref.hyper(1e-3, step=t)
        p, m, v = adam_ref.step(p, one, m, v, "bf16", h)
        p16, w, wm, wv = adam_master_ref.step(w, one, wm, wv, "bf16", h)
    assert adam_ref.bf16_bits_to_f32(p)[0] == 1.0
    assert abs(float(w[0]) - 0.95000064) < 1e-7, float(w[0])
    assert p16.dtype == np.uint16 and p16[0] == adam_ref.f32_to_bf16_bits(w)[0]
    assert adam_ref.bf16_bits_to_f32(p16)[0] == 0.94921875


def test_narrow_and_widen():
    """The restatement's own codecs: ties go to even, overflow to inf, -0 stays."""
    x = np.array([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 0, 0, -0.0], np.float32)
    x.view(np.uint32)[2:4] = (0x7F7F8000, 0x7F7F7FFF)  # the tie above the largest bf16, one ulp below
    assert adam_master_ref.narrow(x, "bf16").tolist() == [0x3F80, 0x3F82, 0x7F80, 0x7F7F, 0x8000]
    y = np.array([1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 65520.0, 65519.996, -0.0], np.float32)
    got = adam_master_ref.narrow(y, "f16")
    assert got.view(np.uint16).tolist() == [0x3C00, 0x3C02, 0x7C00, 0x7BFF, 0x8000]
    for dt in ("bf16", "f16"):
        a = np.arange(0, 0x7C00, 7, dtype=np.uint16).view(adam_master_ref.STORAGE[dt])
        back = adam_master_ref.narrow(adam_master_ref.widen(a, dt), dt)
        assert np.array_equal(back.view(np.uint16), a.view(np.uint16)), dt


@pytest.mark.parametrize("wd,decoupled", ROWS)
def test_restatement_against_torch(wd, decoupled):
    """adam_master_ref against torch.optim.Adam / AdamW(foreach=False) on CPU,
    run on an fp32 copy of the parameters with the bf16-rounded gradients
    widened: DESIGN.md §14's inputs (100003 standard-normal elements, 4 steps,
    lr changed every step, the three decay rows). Not bit-exact, for §14's
    reasons (torch's lerp, its fused a + alpha*b). The largest absolute
    differences measured for (master, m, v): 2.38e-7, 1.19e-7, 1.86e-9 with no
    decay; 2.38e-7, 1.19e-7, 5.59e-9 with Adam's L2 decay; 2.38e-7, 1.19e-7,
    1.86e-9 with AdamW's (MEASURED; §14's table for the same arithmetic was the
    expectation). Each bound is four times the measured value. The parameter is the narrowing of the master by
    construction; that is asserted too."""
    n, lrs = 100003, (1e-3, 5e-4, 2e-3, 1e-4)
    rng = np.random.default_rng(7)
    p16 = adam_ref.f32_to_bf16_bits(rng.standard_normal(n).astype(np.float32))
    grads = [adam_ref.f32_to_bf16_bits(rng.standard_normal(n).astype(np.float32)) for _ in lrs]
    w = adam_master_ref.widen(p16, "bf16")
    tp = torch.nn.Parameter(torch.from_numpy(w.copy()))
    cls = torch.optim.AdamW if decoupled else torch.optim.Adam
    opt = cls([tp], lr=lrs[0], weight_decay=wd, foreach=False)
    m, v = np.zeros(n, np.float32), np.zeros(n, np.float32)
    for i, (lr, g) in enumerate(zip(lrs, grads)):
        opt.param_groups[0]["lr"] = lr
        tp.grad = torch.from_numpy(adam_master_ref.widen(g, "bf16"))
        opt.step()
        h = adam_ref.hyper(lr, weight_decay=wd, decoupled=decoupled, step=i + 1)
        p16, w, m, v = adam_master_ref.step(w, g, m, v, "bf16", h)
    st = opt.state[tp]
    diffs = [float(np.max(np.abs(a - b))) for a, b in
             ((tp.detach().numpy(), w), (st["exp_avg"].numpy(), m), (st["exp_avg_sq"].numpy(), v))]
    print("max |torch - adam_master_ref| after 4 steps (master, m, v): %.3g %.3g %.3g" % tuple(diffs))
    for d, measured, what in zip(diffs, MEASURED[(wd, decoupled)], "wmv"):
        assert d <= 4 * measured, (what, d, measured)
    assert np.array_equal(p16, adam_ref.f32_to_bf16_bits(w))


# ---- construction ------------------------------------------------------------

class _NoMasterExchange:
    world, rank = 1, 0

    def all_reduce_(self, buckets, **kw):
        return buckets

    def adam_step_(self, *a):
        return None


def test_construction_rules():
    from kungfu_amd import optimizers as kopt
    from kungfu_amd.collective import Exchange
    from kungfu_amd.torch import optimizers as topt
    seen = []

    class Ep(cpu_epilogue.CpuEpilogue):
        def adam_master_update_(self, params16, grads16, masters, ms, vs, hypers, np_):
            seen.append((params16[0].dtype, masters[0].dtype, ms[0].dtype, vs[0].dtype))

    # False: everything as before, f16 refused on the first step
    p = torch.nn.Parameter(torch.zeros(8, dtype=torch.float16))
    o = kopt.ShardedAdamOptimizer(torch.optim.Adam([p], lr=1e-3), master_weights=False)
    p.grad = torch.zeros_like(p)
    with pytest.raises(TypeError, match="f32, bf16 and f64"):
        o.step()
    # True: bf16 and f16 are taken, through adam_master_update_ with fp32 shards
    for dtype in (torch.bfloat16, torch.float16):
        for cls in (torch.optim.Adam, torch.optim.AdamW):
            p = torch.nn.Parameter(torch.ones(8, dtype=dtype))
            o = kopt.ShardedAdamOptimizer(cls([p], lr=1e-3), exchange=Exchange(epilogue=Ep()),
                                          master_weights=True)
            assert isinstance(o, cls) and len(o.state) == 0 and o.state_buffers() == {}
            p.grad = torch.ones_like(p)
            o.step()
            assert seen[-1] == (dtype,) + (torch.float32,) * 3
            G = o._kf_groups[0]
            assert G["w"][0].dtype == torch.float32 and G["w"][0][:8].eq(1).all()
            assert torch.equal(G["w"][0], G["pb"].buckets[0].float())  # the bucket, widened
    # through the torch-style constructor's **kwargs
    p = torch.nn.Parameter(torch.ones(8, dtype=torch.float16))
    o = topt.ShardedAdamOptimizer(torch.optim.AdamW([p], lr=1e-3), [("p", p)],
                                  exchange=Exchange(epilogue=Ep()), master_weights=True)
    p.grad = torch.ones_like(p)
    o.step()
    assert seen[-1][0] == torch.float16
    assert "master_weights" in topt.ShardedAdamOptimizer.__doc__
    # an exchange without adam_master_step_: refused at construction, only with the flag
    lin = torch.nn.Linear(5, 3)
    with pytest.raises(ValueError, match="adam_master_step_"):
        kopt.ShardedAdamOptimizer(torch.optim.Adam(lin.parameters(), lr=1e-3),
                                  exchange=_NoMasterExchange(), master_weights=True)
    kopt.ShardedAdamOptimizer(torch.optim.Adam(lin.parameters(), lr=1e-3),
                              exchange=_NoMasterExchange())
    for cls in (torch.optim.Adam, torch.optim.AdamW):
        for option in ("amsgrad", "maximize", "differentiable"):
            with pytest.raises(ValueError, match=option):
                kopt.ShardedAdamOptimizer(cls(lin.parameters(), lr=1e-3, **{option: True}),
                                          master_weights=True)
    with pytest.raises(TypeError):
        kopt.ShardedAdamOptimizer(torch.optim.SGD(lin.parameters(), lr=0.1), master_weights=True)
    doc = kopt.ShardedAdamOptimizer.__doc__
    for words in ("master_weights=True", "no loss scaling", "gradients finite", "narrowing of its master",
                  "overlap=True", "hierarchical"):
        assert words in doc, words


# ---- the launch shape ----------------------------------------------------------

# kf_adam_master.hip: segments per launch, threads per block, elements per
# unit, units per lane per tile
MASTER_SEG, BLOCK, ELTS, UNROLL = 32, 256, 4, 4


def test_launch_constants_pinned():
    """What tests/test_sharded_adam_master_gpu.py sizes its segments by."""
    import re
    src = open(os.path.join(ROOT, "kungfu_amd", "csrc", "kf_adam_master.hip")).read()
    assert int(re.search(r"constexpr int kAdamMasterSeg\s*=\s*(\d+);", src).group(1)) == MASTER_SEG
    assert int(re.search(r"constexpr int kAdamMasterBlock\s*=\s*(\d+);", src).group(1)) == BLOCK
    assert int(re.search(r"#define KF_ADAM_MASTER_ELTS (\d+)", src).group(1)) == ELTS
    assert "#define KF_ADAM_MASTER_UNROLL (16 / KF_ADAM_MASTER_ELTS)" in src and 16 // ELTS == UNROLL
    # the grid rule is the shared planner's (tests/test_update_plan.py runs it)
    assert '#include "kf_update_batch.hpp"' in src and "plan_update_batch<AdamMasterArgs>(" in src
    hdr = open(os.path.join(ROOT, "kungfu_amd", "csrc", "kf_update_batch.hpp")).read()
    assert "const bool rows = a.nseg > 1 && widest * a.nseg <= 2 * blocks;" in hdr
    names = open(os.path.join(ROOT, "kungfu_amd", "csrc", "Makefile")).read()
    assert re.search(r"^NAMES\s*:=.*\bkf_adam_master\b", names, re.M)


# ---- C ABI argument errors (no device) --------------------------------------

OK, ERR_DTYPE, ERR_ARG = base.OK, base.ERR_DTYPE, base.ERR_ARG
F32, I32, F16, BF16, F64, BOOL = base.F32, base.I32, base.F16, base.BF16, base.F64, base.BOOL


def test_adam_master_update_batch_arg_errors():
    """Every check of kf_adam_master_update_batch comes before any HIP call."""
    from kungfu_amd import _lib
    lib = _lib.load()
    pa = _lib.ptr_array
    cnt = lambda *v: (ctypes.c_size_t * len(v))(*v)  # noqa: E731
    plain = _lib.adam_hyper_array([adam_ref.hyper(1e-3)])

    def call(p16, g16, ws, ms, vs, counts, nb, dt=BF16, np_=0, hyper=plain):
        return lib.kf_adam_master_update_batch(p16, g16, ws, ms, vs, counts, nb, dt, np_, hyper,
                                               None)

    five = (pa([16]), pa([32]), pa([48]), pa([64]), pa([80]))
    assert call(None, None, None, None, None, None, 0) == OK           # nb == 0
    assert call(*five, cnt(0), 1) == OK                                # an empty segment
    assert call(*([pa([0])] * 5), cnt(0), 1) == OK
    assert call(*five, cnt(0), 1, dt=F16) == OK
    assert call(*five, cnt(4), -1) == ERR_ARG                          # nb < 0
    assert b"kf_adam_master_update_batch" in lib.kf_last_error()
    for i in range(5):                                                 # null tables
        t = list(five)
        t[i] = None
        assert call(*t, cnt(4), 1) == ERR_ARG, i
    assert call(*five, None, 1) == ERR_ARG
    assert call(*five, cnt(4), 1, hyper=None) == ERR_ARG
    for i in range(5):
        t = list(five)
        t[i] = pa([0])                                                 # null pointer, count > 0
        assert call(*t, cnt(4), 1) == ERR_ARG, i
        t[i] = pa([16 * (i + 1) + 8])                                  # off the 16-byte boundary
        assert call(*t, cnt(4), 1) == ERR_ARG, i
        assert b"16-byte" in lib.kf_last_error()
    assert call(*five, cnt(4), 1, np_=-1) == ERR_ARG
    zero1 = _lib.adam_hyper_array([adam_ref.hyper(1e-3, betas=(1.0, 0.999))])
    zero2 = _lib.adam_hyper_array([adam_ref.hyper(1e-3, betas=(0.9, 1.0))])
    neg = _lib.adam_hyper_array([adam_ref.hyper(1e-3)])
    neg[0].bias_correction2 = -0.5
    nan = _lib.adam_hyper_array([adam_ref.hyper(1e-3)])
    nan[0].bias_correction1 = float("nan")
    for h in (zero1, zero2, neg, nan):                                 # bias corrections <= 0
        assert call(*five, cnt(4), 1, hyper=h) == ERR_ARG
        assert b"kf_adam_master_update_batch" in lib.kf_last_error()
    for dt in (F32, F64, I32, BOOL, 0x00108, 0x12345):
        assert call(*five, cnt(4), 1, dt=dt) == ERR_DTYPE, hex(dt)
    assert b"kf_adam_master_update_batch" in lib.kf_last_error()


def test_exchange_adam_master_batch_needs_an_exchange():
    """Without a device there is no exchange to hand over: the null handle is
    refused before anything else (tests/test_sharded_adam_master_gpu.py makes
    the other checks on a loopback group)."""
    from kungfu_amd import _lib
    lib = _lib.load()
    pa = _lib.ptr_array
    h = _lib.adam_hyper_array([adam_ref.hyper(1e-3)])
    cnt = (ctypes.c_size_t * 1)(8)
    for dt in (BF16, F16, F32, F64):
        assert lib.kf_exchange_adam_master_batch(None, pa([16]), pa([32]), pa([48]), pa([64]),
                                                 pa([80]), cnt, 1, dt, h, 0, None) == ERR_ARG
    assert lib.kf_exchange_adam_master_batch(None, None, None, None, None, None, None, 0, BF16, h,
                                             0, None) == ERR_ARG
    assert b"kf_exchange_adam_master_batch" in lib.kf_exchange_last_error()


# ---- a bf16 group and an f32 group, worlds 1, 2 and 3 ---------------------------

class CpuAdamMasterEpilogue(base.CpuAdamEpilogue):
    """base.CpuAdamEpilogue plus the master-weights update, from adam_master_ref."""

    def adam_master_update_(self, params16, grads16, masters, exp_avgs, exp_avg_sqs, hypers, np_):
        for p, g, w, m, v, h in zip(params16, grads16, masters, exp_avgs, exp_avg_sqs, hypers):
            dt = cpu_epilogue._DT[p.dtype]
            assert w.dtype == m.dtype == v.dtype == torch.float32
            new = adam_master_ref.step(w.numpy().copy(), np.ascontiguousarray(cpu_epilogue._np(g)),
                                       m.numpy().copy(), v.numpy().copy(), dt, h, np_)
            for a, n in zip((cpu_epilogue._np(p), w.numpy(), m.numpy(), v.numpy()), new):
                a[...] = n
        return params16


SHAPES, GROUPS, GROUP_HYPER, STEPS = base.SHAPES, base.GROUPS, base.GROUP_HYPER, base.STEPS
DTS = ("bf16", "bf16", "f32")  # per parameter: group 0 is 16-bit, group 1 is f32


def param_dts(dt16):
    return tuple(dt16 if d == "bf16" else d for d in DTS)


def model_arrays(dt16="bf16"):
    return [_arrays(base.model_arrays("f32"), d)[j] for j, d in enumerate(param_dts(dt16))]


def _arrays(f32_arrays, dt):
    if dt == "f32":
        return f32_arrays
    return [adam_master_ref.narrow(a, dt) for a in f32_arrays]


def grad_arrays(world, step, dt16="bf16"):
    """[rank][param], base.grad_arrays' grid (exact sums) in each parameter's dtype."""
    f32 = base.grad_arrays("f32", world, step)
    return [[_arrays(gs, d)[j] for j, d in enumerate(param_dts(dt16))] for gs in f32]


def to_torch(a, dt):
    if dt == "f16":
        return torch.from_numpy(np.ascontiguousarray(a).copy())
    return base.to_torch(a, dt)


def to_numpy(t, dt):
    if dt == "f16":
        return t.detach().cpu().contiguous().numpy().copy()
    return base.to_numpy(t, dt)


_REFERENCE = {}


def reference_run(world, steps=STEPS, dt16="bf16", skip=None):
    """(params, masters, exp_avgs, exp_avg_sqs) after `steps` steps of AdamW
    with the lr halved after every step: adam_master_ref on the 16-bit
    parameters (masters[j] is None for the f32 one), adam_ref on the f32 one,
    both on oracle.reduce_avg of the ranks' gradients, which rounds the
    average to the gradients' dtype as the exchange's fold does. Computed once
    per case and shared; callers leave it unchanged."""
    key = (world, steps, dt16, skip)
    if key in _REFERENCE:
        return _REFERENCE[key]
    from oracle import oracle
    dts = param_dts(dt16)
    ps = model_arrays(dt16)
    ws = [adam_master_ref.widen(a, d).reshape(-1) if d != "f32" else None for a, d in zip(ps, dts)]
    ms = [np.zeros(a.size, np.float32) for a in ps]
    vs = [np.zeros(a.size, np.float32) for a in ps]
    lr_scale = 1.0
    for s in range(steps):
        gr = grad_arrays(world, s, dt16)
        for gi, idx in enumerate(GROUPS):
            h = dict(GROUP_HYPER[gi], decoupled=True, step=s + 1)
            h["lr"] = h["lr"] * lr_scale
            for j in idx:
                ins = [np.ascontiguousarray(gr[r][j].reshape(-1)) for r in range(world)]
                if skip == (s, j):
                    ins = [np.zeros_like(x) for x in ins]
                avg = oracle.reduce_avg(ins, dts[j], world)
                if ws[j] is None:
                    p, ms[j], vs[j] = adam_ref.step(ps[j].reshape(-1), avg, ms[j], vs[j], "f32", h)
                else:
                    p, ws[j], ms[j], vs[j] = adam_master_ref.step(ws[j], avg, ms[j], vs[j], dts[j], h)
                ps[j] = p.reshape(SHAPES[j])
        lr_scale *= 0.5
    _REFERENCE[key] = (ps, ws, ms, vs)
    return _REFERENCE[key]


def make_optimizer(exchange, device="cpu", master_weights=True, dt16="bf16", arrays=None):
    from kungfu_amd.optimizers import ShardedAdamOptimizer
    arrays = model_arrays(dt16) if arrays is None else arrays
    ps = [torch.nn.Parameter(to_torch(a, d).to(device)) for a, d in zip(arrays, param_dts(dt16))]
    groups = [dict(GROUP_HYPER[gi], params=[ps[j] for j in idx]) for gi, idx in enumerate(GROUPS)]
    return ps, ShardedAdamOptimizer(torch.optim.AdamW(groups, lr=0.1), exchange=exchange,
                                    master_weights=master_weights)


def run_steps(ps, opt, world, rank, device="cpu", first_step=0, steps=STEPS, dt16="bf16", skip=None):
    for s in range(first_step, first_step + steps):
        gr = grad_arrays(world, s, dt16)[rank]
        for j, (p, d) in enumerate(zip(ps, param_dts(dt16))):
            p.grad = None if skip == (s, j) else to_torch(gr[j], d).to(device)
        opt.step()
        for g in opt.param_groups:
            g["lr"] = g["lr"] * 0.5


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def check_against_reference(ps, sb, want, dt16="bf16", steps=STEPS):
    """Parameters, masters and both states against reference_run's, and the
    invariant: every 16-bit parameter is the narrowing of its gathered master."""
    want_p, want_w, want_m, want_v = want
    assert set(sb) == set(ps)
    for j, (p, d) in enumerate(zip(ps, param_dts(dt16))):
        assert same_bits(to_numpy(p, d), want_p[j]), ("param", j)
        b = sb[p]
        assert b["step"] == steps
        assert b["exp_avg"].dtype == b["exp_avg_sq"].dtype == torch.float32
        assert b["exp_avg"].shape == p.shape and b["exp_avg_sq"].shape == p.shape
        assert same_bits(b["exp_avg"].cpu().numpy().reshape(-1), want_m[j]), ("exp_avg", j)
        assert same_bits(b["exp_avg_sq"].cpu().numpy().reshape(-1), want_v[j]), ("exp_avg_sq", j)
        if d == "f32":
            assert "master" not in b
            continue
        w = b["master"]
        assert w.dtype == torch.float32 and w.shape == p.shape
        assert same_bits(w.cpu().numpy().reshape(-1), want_w[j]), ("master", j)
        assert same_bits(adam_master_ref.narrow(w.cpu().numpy(), d), to_numpy(p, d)), ("invariant", j)


def _clone_optimizer(ps, opt, exchange, device="cpu"):
    """A fresh optimizer over copies of the parameters, with opt's current lrs."""
    ps2, opt2 = make_optimizer(exchange, device, arrays=[to_numpy(p, d) for p, d in zip(ps, DTS)])
    for g2, g in zip(opt2.param_groups, opt.param_groups):
        g2["lr"] = g["lr"]
    return ps2, opt2


def body_sharded(rank, world):
    from kungfu_amd.collective import Exchange
    ps, opt = make_optimizer(Exchange(epilogue=CpuAdamMasterEpilogue()))
    run_steps(ps, opt, world, rank)
    assert len(opt.state) == 0
    sb = opt.state_buffers()
    check_against_reference(ps, sb, reference_run(world))
    if world > 1:  # every rank's parameters are bit-identical
        flat = torch.cat([torch.from_numpy(to_numpy(p, d).reshape(-1).view(
            np.int16 if d == "bf16" else np.int32).astype(np.int32)) for p, d in zip(ps, DTS)])
        allf = [torch.empty_like(flat) for _ in range(world)]
        dist.all_gather(allf, flat)
        for f in allf:
            assert torch.equal(f, flat)
    # the f32 group: the same bits as without the flag
    qs, plain = make_optimizer(Exchange(epilogue=CpuAdamMasterEpilogue()), master_weights=False)
    run_steps(qs, plain, world, rank)
    pb = plain.state_buffers()
    assert same_bits(to_numpy(ps[2], "f32"), to_numpy(qs[2], "f32"))
    for k in ("exp_avg", "exp_avg_sq"):
        assert same_bits(sb[ps[2]][k].numpy(), pb[qs[2]][k].numpy()), k
    assert pb[qs[0]]["exp_avg"].dtype == torch.bfloat16 and "master" not in pb[qs[0]]
    # checkpoint round trip: a fresh optimizer takes the buffers and goes on
    # as the uninterrupted one does
    ps2, opt2 = _clone_optimizer(ps, opt, Exchange(epilogue=CpuAdamMasterEpilogue()))
    opt2.load_state_buffers({q: sb[p] for p, q in zip(ps, ps2)})
    sb2 = opt2.state_buffers()
    for p, q in zip(ps, ps2):
        assert set(sb2[q]) == set(sb[p])
        for k in set(sb[p]) - {"step"}:
            assert same_bits(sb2[q][k].numpy(), sb[p][k].numpy()), k
    # without "master": the master is the current parameters widened again
    ps3, opt3 = _clone_optimizer(ps, opt, Exchange(epilogue=CpuAdamMasterEpilogue()))
    opt3.load_state_buffers({q: {k: t for k, t in sb[p].items() if k != "master"}
                             for p, q in zip(ps, ps3)})
    sb3 = opt3.state_buffers()
    for j, (p, q) in enumerate(zip(ps, ps3)):
        if DTS[j] != "f32":
            assert same_bits(sb3[q]["master"].numpy(), adam_master_ref.widen(to_numpy(p, DTS[j]), DTS[j]))
            assert same_bits(sb3[q]["exp_avg"].numpy(), sb[p]["exp_avg"].numpy())
    run_steps(ps, opt, world, rank, first_step=STEPS, steps=1)
    run_steps(ps2, opt2, world, rank, first_step=STEPS, steps=1)
    for j, (p, q) in enumerate(zip(ps, ps2)):
        assert same_bits(to_numpy(p, DTS[j]), to_numpy(q, DTS[j])), ("after the round trip", j)
    check_against_reference(ps2, opt2.state_buffers(), reference_run(world, STEPS + 1), steps=STEPS + 1)


def test_world1_mixed_groups_and_checkpoint():
    """The whole of body_sharded in this process: no process group, world 1."""
    body_sharded(0, 1)


def test_world1_f16_group():
    """f16 parameters through the optimizer (no GPU: the CPU epilogue)."""
    from kungfu_amd.collective import Exchange
    ps, opt = make_optimizer(Exchange(epilogue=CpuAdamMasterEpilogue()), dt16="f16")
    run_steps(ps, opt, 1, 0, dt16="f16")
    assert ps[0].dtype == torch.float16
    check_against_reference(ps, opt.state_buffers(), reference_run(1, dt16="f16"), dt16="f16")


def _entry(rank, world, store, errq):
    sys.path[:0] = [ROOT, HERE]
    try:
        dist.init_process_group("gloo", init_method="file://" + store, rank=rank,
                                world_size=world)
        import test_sharded_adam_master as mod
        mod.body_sharded(rank, world)
        dist.barrier()
    except Exception:
        errq.put("rank %d: %s" % (rank, traceback.format_exc()))
        raise
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_adam_master_over_gloo(world):
    ctx = mp.get_context("spawn")
    errq = ctx.SimpleQueue()
    store = os.path.join(tempfile.mkdtemp(prefix="kfadamw"), "store")
    procs = [ctx.Process(target=_entry, args=(r, world, store, errq)) for r in range(world)]
    for p in procs:
        p.start()
    hung = join_all(procs, 600)
    errs = []
    while not errq.empty():
        errs.append(errq.get())
    assert not errs, "\n".join(errs)
    assert not hung and all(p.exitcode == 0 for p in procs), hung_msg(hung, [p.exitcode for p in procs])
