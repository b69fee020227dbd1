"""ShardedAdamOptimizer without a GPU: the numpy restatement of the update
(tests/adam_ref.py) against torch.optim.Adam / AdamW, the optimizer's
construction rules, the C ABI's argument checks (no device touched), and the
whole reduce-scatter -> update -> all-gather step over gloo with a CPU
epilogue."""
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

import adam_ref
import cpu_epilogue
from procs import hung_msg, join_all

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

# (weight_decay, decoupled): no decay, Adam's L2, AdamW's decoupled decay
ROWS = [(0.0, False), (1e-2, False), (1e-2, True)]

# The largest |torch - adam_ref| measured for (p, m, v) on the data of
# test_restatement_against_torch, per row: one or two units in the last place
# of the largest elements (2^-23 = 1.19e-7, 2^-22 = 2.38e-7, 2^-29 = 1.86e-9,
# 2^-28 = 3.73e-9). The test's bounds are four times these.
MEASURED = {(0.0, False): (2.0 ** -23, 2.0 ** -23, 2.0 ** -29),
            (1e-2, False): (2.0 ** -22, 2.0 ** -23, 2.0 ** -28),
            (1e-2, True): (2.0 ** -23, 2.0 ** -23, 2.0 ** -29)}


# ---- the restatement against torch ------------------------------------------

@pytest.mark.parametrize("wd,decoupled", ROWS)
def test_restatement_against_torch(wd, decoupled):
    """adam_ref against torch.optim.Adam / AdamW(foreach=False) on CPU, f32.
    Not bit-exact: torch's exp_avg is a lerp and its CPU kernels fuse
    a + alpha*b. On standard-normal data the largest absolute differences
    after these 4 steps were, for (p, m, v): 1.19e-7, 1.19e-7, 1.86e-9 with no
    decay; 2.38e-7, 1.19e-7, 3.73e-9 with Adam's L2 decay; 1.19e-7, 1.19e-7,
    1.86e-9 with AdamW's (MEASURED). Each bound is four times the measured
    value. This pins the restatement, not the kernel."""
    n, lrs = 100003, (1e-3, 5e-4, 2e-3, 1e-4)
    rng = np.random.default_rng(7)
    p0 = rng.standard_normal(n).astype(np.float32)
    grads = [rng.standard_normal(n).astype(np.float32) for _ in lrs]
    tp = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    cls = torch.optim.AdamW if decoupled else torch.optim.Adam
    opt = cls([tp], lr=lrs[0], weight_decay=wd, foreach=False)
    p, m, v = p0.copy(), np.zeros(n, np.float32), np.zeros(n, np.float32)
    for i, (lr, g) in enumerate(zip(lrs, grads)):
        opt.param_groups[0]["lr"] = lr
        tp.grad = torch.from_numpy(g.copy())
        opt.step()
        p, m, v = adam_ref.step(p, g, m, v, "f32",
                                adam_ref.hyper(lr, weight_decay=wd, decoupled=decoupled, step=i + 1))
    st = opt.state[tp]
    diffs = [float(np.max(np.abs(a - b))) for a, b in
             ((tp.detach().numpy(), p), (st["exp_avg"].numpy(), m), (st["exp_avg_sq"].numpy(), v))]
    print("max |torch - adam_ref| after 4 steps (p, m, v): %.3g %.3g %.3g" % tuple(diffs))
    for d, measured, what in zip(diffs, MEASURED[(wd, decoupled)], "pmv"):
        assert d <= 4 * measured, (what, d, measured)


# ---- construction ------------------------------------------------------------

def _lin():
    torch.manual_seed(0)
    return torch.nn.Linear(5, 3)


class _NoAdamExchange:
    world, rank = 1, 0

    def all_reduce_(self, buckets, **kw):
        return buckets

    def sgd_step_(self, *a):
        return None


def test_construction_rules():
    from kungfu_amd import optimizers as kopt
    from kungfu_amd.torch import optimizers as topt
    assert "ShardedAdamOptimizer" in topt.__all__
    m = _lin()
    for cls in (torch.optim.Adam, torch.optim.AdamW):
        o = kopt.ShardedAdamOptimizer(cls(m.parameters(), lr=1e-3))
        assert isinstance(o, torch.optim.Adam) or cls is torch.optim.AdamW
        assert isinstance(o, cls)
        assert o._kf_decoupled == (cls is torch.optim.AdamW)
        assert len(o.state) == 0
        assert o.state_buffers() == {}
        torch.optim.lr_scheduler.StepLR(o, step_size=1)  # takes it for an optimizer
    o = kopt.ShardedAdamOptimizer(torch.optim.Adam(m.parameters(), lr=1e-3))
    assert isinstance(o, torch.optim.Adam)
    o2 = topt.ShardedAdamOptimizer(torch.optim.Adam(m.parameters(), lr=1e-3), m.named_parameters())
    assert isinstance(o2, torch.optim.Adam) and len(o2.state) == 0
    for other in (torch.optim.SGD(m.parameters(), lr=0.1), torch.optim.RMSprop(m.parameters()),
                  torch.optim.Adamax(m.parameters())):
        with pytest.raises(TypeError):
            kopt.ShardedAdamOptimizer(other)
    for cls in (torch.optim.Adam, torch.optim.AdamW):
        for option in ("amsgrad", "maximize", "differentiable"):
            with pytest.raises(ValueError, match=option):
                kopt.ShardedAdamOptimizer(cls(m.parameters(), lr=1e-3, **{option: True}))
    with pytest.raises(ValueError, match="adam_step_"):
        kopt.ShardedAdamOptimizer(torch.optim.Adam(m.parameters(), lr=1e-3),
                                  exchange=_NoAdamExchange())
    # ShardedSGDOptimizer still refuses Adam
    with pytest.raises(TypeError):
        kopt.ShardedSGDOptimizer(torch.optim.Adam(m.parameters(), lr=1e-3))
    doc = kopt.ShardedAdamOptimizer.__doc__
    for words in ("zero gradient", "p.grad does not hold", "overlap=True", "hierarchical",
                  "not torch's\n        lerp", "f16", "amsgrad", "single-tensor"):
        assert words in doc, words


def test_f16_parameters_are_refused():
    from kungfu_amd import optimizers as kopt
    p = torch.nn.Parameter(torch.zeros(8, dtype=torch.float16))
    o = kopt.ShardedAdamOptimizer(torch.optim.Adam([p], lr=1e-3))
    p.grad = torch.zeros_like(p)
    with pytest.raises(TypeError, match="f32, bf16 and f64"):
        o.step()


def test_tensor_lr_and_step_counter():
    """float() is taken of the hyperparameters (torch allows a tensor lr), and
    every bucket group counts its own steps from 1."""
    from kungfu_amd import optimizers as kopt
    from kungfu_amd.collective import Exchange
    seen = []

    class Ep(cpu_epilogue.CpuEpilogue):
        def adam_update_(self, params, grads, ms, vs, hypers, np_):
            seen.append([dict(h) for h in hypers])

    a, b = (torch.nn.Parameter(torch.ones(4)) for _ in range(2))
    o = kopt.ShardedAdamOptimizer(
        torch.optim.AdamW([{"params": [a], "lr": torch.tensor(0.5)}, {"params": [b]}], lr=0.25,
                          betas=(0.8, 0.9), eps=1e-6, weight_decay=0.125),
        exchange=Exchange(epilogue=Ep()))
    for _ in range(2):
        a.grad, b.grad = torch.ones(4), torch.ones(4)
        o.step()
    assert [[h["step"] for h in call] for call in seen] == [[1], [1], [2], [2]]
    h = seen[0][0]
    assert type(h["lr"]) is float and h["lr"] == 0.5 and seen[1][0]["lr"] == 0.25
    assert h["betas"] == (0.8, 0.9) and h["eps"] == 1e-6 and h["weight_decay"] == 0.125
    assert h["decoupled"] is True


# ---- the launch shape ----------------------------------------------------------

# kf_adam.hip: segments per launch, threads per block, 16-B vectors per lane
ADAM_SEG, BLOCK, UNROLL = 24, 256, 4


def test_launch_constants_pinned():
    """What tests/test_sharded_adam_gpu.py sizes its segments by."""
    import re
    src = open(os.path.join(ROOT, "kungfu_amd", "csrc", "kf_adam.hip")).read()
    assert int(re.search(r"constexpr int kAdamSeg\s*=\s*(\d+);", src).group(1)) == ADAM_SEG
    assert int(re.search(r"constexpr int kAdamBlock\s*=\s*(\d+);", src).group(1)) == BLOCK
    assert int(re.search(r"#define KF_ADAM_UNROLL (\d+)", src).group(1)) == UNROLL
    # the grid rule is the shared planner's (tests/test_update_plan.py runs it)
    assert '#include "kf_update_batch.hpp"' in src and "plan_update_batch<AdamBatchArgs<C>>(" in src
    hdr = open(os.path.join(ROOT, "kungfu_amd", "csrc", "kf_update_batch.hpp")).read()
    assert "const bool rows = a.nseg > 1 && widest * a.nseg <= 2 * blocks;" in hdr


# ---- C ABI argument errors (no device) --------------------------------------

OK, ERR_DTYPE, ERR_ARG = 0, 1, 3
F32, I32, F16, BF16, F64, BOOL = 0x20408, 0x10408, 0x20208, 0x20209, 0x20808, 0x30108


def test_adam_update_batch_arg_errors():
    """Every check of kf_adam_update_batch comes before any HIP call."""
    from kungfu_amd import _lib
    lib = _lib.load()
    pa = _lib.ptr_array
    cnt = lambda *v: (ctypes.c_size_t * len(v))(*v)  # noqa: E731
    plain = _lib.adam_hyper_array([adam_ref.hyper(1e-3)])

    def call(params, grads, ms, vs, counts, nb, dt=F32, np_=0, hyper=plain):
        return lib.kf_adam_update_batch(params, grads, ms, vs, counts, nb, dt, np_, hyper, None)

    four = (pa([16]), pa([32]), pa([48]), pa([64]))
    assert call(None, None, None, None, None, 0) == OK                 # nb == 0
    assert call(*four, cnt(0), 1) == OK                                # an empty segment
    assert call(pa([0]), pa([0]), pa([0]), pa([0]), cnt(0), 1) == OK
    assert call(*four, cnt(4), -1) == ERR_ARG                          # nb < 0
    for i in range(4):                                                 # null tables
        t = list(four)
        t[i] = None
        assert call(*t, cnt(4), 1) == ERR_ARG, i
    assert call(*four, None, 1) == ERR_ARG
    assert call(*four, cnt(4), 1, hyper=None) == ERR_ARG
    for i in range(4):
        t = list(four)
        t[i] = pa([0])                                                 # null pointer, count > 0
        assert call(*t, cnt(4), 1) == ERR_ARG, i
        t[i] = pa([16 * (i + 1) + 8])                                  # off the 16-byte boundary
        assert call(*t, cnt(4), 1) == ERR_ARG, i
    assert call(*four, cnt(4), 1, np_=-1) == ERR_ARG
    zero1 = _lib.adam_hyper_array([adam_ref.hyper(1e-3, betas=(1.0, 0.999))])
    zero2 = _lib.adam_hyper_array([adam_ref.hyper(1e-3, betas=(0.9, 1.0))])
    neg = _lib.adam_hyper_array([adam_ref.hyper(1e-3)])
    neg[0].bias_correction2 = -0.5
    nan = _lib.adam_hyper_array([adam_ref.hyper(1e-3)])
    nan[0].bias_correction1 = float("nan")
    assert zero1[0].bias_correction1 == 0 and zero2[0].bias_correction2 == 0
    for h in (zero1, zero2, neg, nan):                                 # bias corrections <= 0
        assert call(*four, cnt(4), 1, hyper=h) == ERR_ARG
        assert b"kf_adam_update_batch" in lib.kf_last_error()
    for dt in (F16, I32, BOOL, 0x00108, 0x12345):
        assert call(*four, cnt(4), 1, dt=dt) == ERR_DTYPE, hex(dt)
    assert b"kf_adam_update_batch" in lib.kf_last_error()


def test_adam_hyper_array_takes_the_bias_corrections_in_double():
    from kungfu_amd import _lib
    h = _lib.adam_hyper_array([adam_ref.hyper(1e-3, betas=(0.9, 0.999), eps=1e-8,
                                              weight_decay=0.01, decoupled=True, step=7)])[0]
    assert (h.lr, h.beta1, h.beta2, h.eps, h.weight_decay) == (1e-3, 0.9, 0.999, 1e-8, 0.01)
    assert h.bias_correction1 == 1.0 - 0.9 ** 7 and h.bias_correction2 == 1.0 - 0.999 ** 7
    assert h.decoupled == 1
    assert ctypes.sizeof(_lib.AdamHyper) == 64


def test_exchange_adam_batch_needs_an_exchange():
    """Without a device there is no exchange to hand over: the null handle is
    refused before anything else (the counts % world check needs a world;
    tests/test_sharded_adam_gpu.py makes it on a loopback group)."""
    from kungfu_amd import _lib
    lib = _lib.load()
    pa = _lib.ptr_array
    h = _lib.adam_hyper_array([adam_ref.hyper(1e-3)])
    cnt = (ctypes.c_size_t * 1)(4)
    assert lib.kf_exchange_adam_batch(None, pa([16]), pa([32]), pa([48]), pa([64]), cnt, 1, F32,
                                      h, 0, None) == ERR_ARG
    assert lib.kf_exchange_adam_batch(None, None, None, None, None, None, 0, F32, h, 0,
                                      None) == ERR_ARG


# ---- gloo, worlds 2 and 3 ----------------------------------------------------

class CpuAdamEpilogue(cpu_epilogue.CpuEpilogue):
    """cpu_epilogue.CpuEpilogue plus the Adam update, from adam_ref."""

    def adam_update_(self, params, grads, exp_avgs, exp_avg_sqs, hypers, np_):
        for p, g, m, v, h in zip(params, grads, exp_avgs, exp_avg_sqs, hypers):
            dt = cpu_epilogue._DT[p.dtype]
            arrs = [cpu_epilogue._np(x) for x in (p, g, m, v)]
            new = adam_ref.step(*[np.ascontiguousarray(a) for a in arrs], dt, h, np_)
            for a, n in zip((arrs[0], arrs[2], arrs[3]), new):
                a[...] = n
        return params


SHAPES = ((7, 5), (5,), (3, 5))
GROUPS = ((0, 1), (2,))  # parameter indices of the two param groups
GROUP_HYPER = ({"lr": 0.1, "weight_decay": 1e-2, "betas": (0.9, 0.999), "eps": 1e-8},
               {"lr": 0.05, "weight_decay": 0.0, "betas": (0.8, 0.99), "eps": 1e-6})
STEPS = 3
DECOUPLED = {"f32": False, "bf16": True}  # Adam for f32, AdamW for bf16
_TORCH = {"f32": torch.float32, "bf16": torch.bfloat16}


def model_arrays(dt, seed=3):
    """Initial parameters (the same on every rank), in dt's numpy form."""
    rng = np.random.default_rng(seed)
    out = []
    for shp in SHAPES:
        a = rng.standard_normal(shp).astype(np.float32)
        out.append(adam_ref.f32_to_bf16_bits(a) if dt == "bf16" else a)
    return out


def grad_arrays(dt, world, step, seed=11):
    """[rank][param]: multiples of 1/4 in [-8, 8], so that the sum over the
    ranks is exact in every order a transport may add in."""
    out = []
    for r in range(world):
        rng = np.random.default_rng(seed + 100 * step + r)
        gs = []
        for shp in SHAPES:
            a = (rng.integers(-32, 33, shp) / 4.0).astype(np.float32)
            gs.append(adam_ref.f32_to_bf16_bits(a) if dt == "bf16" else a)
        out.append(gs)
    return out


def to_torch(a, dt):
    if dt == "bf16":
        return torch.from_numpy(np.ascontiguousarray(a).view(np.int16).copy()).view(torch.bfloat16)
    return torch.from_numpy(a.copy())


def to_numpy(t, dt):
    t = t.detach().cpu().contiguous()
    if dt == "bf16":
        return t.view(torch.int16).numpy().view(np.uint16).copy()
    return t.numpy().copy()


_REFERENCE = {}


def reference_run(dt, world, steps=STEPS, skip=None):
    """(params, exp_avgs, exp_avg_sqs) after `steps` steps: adam_ref applied
    to oracle.reduce_avg of the ranks' gradients, lr halved after every step.
    skip = (step, param): that parameter has no gradient there (zeros).
    Computed once per case and shared; callers leave it unchanged."""
    key = (dt, world, steps, skip)
    if key in _REFERENCE:
        return _REFERENCE[key]
    from oracle import oracle
    ps = model_arrays(dt)
    zeros = lambda a: np.zeros(a.size, a.dtype)  # noqa: E731  (+0 in every format)
    ms, vs = [zeros(a) for a in ps], [zeros(a) for a in ps]
    lr_scale = 1.0
    for s in range(steps):
        gr = grad_arrays(dt, world, s)
        for gi, idx in enumerate(GROUPS):
            h = dict(GROUP_HYPER[gi], decoupled=DECOUPLED[dt], step=s + 1)
            h["lr"] = h["lr"] * lr_scale
            for j in idx:
                ins = [np.ascontiguousarray(gr[r][j].reshape(-1)) for r in range(world)]
                if skip == (s, j):
                    ins = [np.zeros_like(x) for x in ins]
                avg = oracle.reduce_avg(ins, dt, world)
                p, ms[j], vs[j] = adam_ref.step(ps[j].reshape(-1), avg, ms[j], vs[j], dt, h)
                ps[j] = p.reshape(SHAPES[j])
        lr_scale *= 0.5
    _REFERENCE[key] = (ps, ms, vs)
    return _REFERENCE[key]


def _torch_optimizer(dt, groups):
    cls = torch.optim.AdamW if DECOUPLED[dt] else torch.optim.Adam
    return cls(groups, lr=0.1)


def make_optimizer(dt, exchange, device="cpu"):
    from kungfu_amd.optimizers import ShardedAdamOptimizer
    ps = [torch.nn.Parameter(to_torch(a, dt).to(device)) for a in model_arrays(dt)]
    groups = [dict(GROUP_HYPER[gi], params=[ps[j] for j in idx]) for gi, idx in enumerate(GROUPS)]
    return ps, ShardedAdamOptimizer(_torch_optimizer(dt, groups), exchange=exchange)


def run_steps(ps, opt, dt, world, rank, device="cpu", skip=None, first_step=0, steps=STEPS):
    for s in range(first_step, first_step + steps):
        gr = grad_arrays(dt, world, s)[rank]
        for j, p in enumerate(ps):
            p.grad = None if skip == (s, j) else to_torch(gr[j], dt).to(device)
        opt.step()
        for g in opt.param_groups:
            g["lr"] = g["lr"] * 0.5


def _bits(t, dt):
    return t.view(torch.int16 if dt == "bf16" else torch.int32)


def body_sharded(rank, world):
    from kungfu_amd.collective import Exchange
    from kungfu_amd.optimizers import ShardedAdamOptimizer
    for dt in ("f32", "bf16"):
        ex = Exchange(epilogue=CpuAdamEpilogue())
        ps, opt = make_optimizer(dt, ex)
        run_steps(ps, opt, dt, world, rank)
        assert len(opt.state) == 0
        want_p, want_m, want_v = reference_run(dt, world)
        for j, p in enumerate(ps):
            assert np.array_equal(to_numpy(p, dt), want_p[j]), (dt, "param", j)
        # every rank's parameters are bit-identical
        flat = torch.cat([torch.from_numpy(to_numpy(p, dt).reshape(-1).view(
            np.int16 if dt == "bf16" else np.int32).astype(np.int32)) for p in ps])
        allf = [torch.empty_like(flat) for _ in range(world)]
        dist.all_gather(allf, flat)
        for f in allf:
            assert torch.equal(f, flat), dt
        sb = opt.state_buffers()
        assert set(sb) == set(ps)
        for j, p in enumerate(ps):
            assert sb[p]["step"] == STEPS
            assert sb[p]["exp_avg"].shape == p.shape and sb[p]["exp_avg_sq"].shape == p.shape
            assert np.array_equal(to_numpy(sb[p]["exp_avg"], dt).reshape(-1), want_m[j]), (dt, "m", j)
            assert np.array_equal(to_numpy(sb[p]["exp_avg_sq"], dt).reshape(-1), want_v[j]), (dt, "v", j)
        # load_state_buffers round-trips: a fresh optimizer over the same
        # parameters takes the state and goes on as the first one does
        ps2 = [torch.nn.Parameter(p.detach().clone()) for p in ps]
        at = {id(p): i for i, p in enumerate(ps)}
        groups = [dict(g, params=[ps2[at[id(p)]] for p in g["params"]]) for g in opt.param_groups]
        opt2 = ShardedAdamOptimizer(_torch_optimizer(dt, groups),
                                    exchange=Exchange(epilogue=CpuAdamEpilogue()))
        loaded = {ps2[at[id(p)]]: b for p, b in sb.items()}
        with pytest.raises(ValueError, match="step"):
            opt2.load_state_buffers({q: dict(b, step=b["step"] + (q is ps2[0])) for q, b in loaded.items()})
        opt2.load_state_buffers(loaded)
        sb2 = opt2.state_buffers()
        for p, q in zip(ps, ps2):
            assert sb2[q]["step"] == STEPS
            for k in ("exp_avg", "exp_avg_sq"):
                assert torch.equal(_bits(sb2[q][k], dt), _bits(sb[p][k], dt)), (dt, k)
        run_steps(ps, opt, dt, world, rank, first_step=STEPS, steps=1)
        run_steps(ps2, opt2, dt, world, rank, first_step=STEPS, steps=1)
        for p, q in zip(ps, ps2):
            assert np.array_equal(to_numpy(p, dt), to_numpy(q, dt)), dt
        # a group whose parameters are all absent is left as it is; a
        # parameter missing from a loaded group gets zeros
        before = opt2.state_buffers()
        opt2.load_state_buffers({ps2[0]: before[ps2[0]]})
        after = opt2.state_buffers()
        assert torch.equal(_bits(after[ps2[2]]["exp_avg"], dt), _bits(before[ps2[2]]["exp_avg"], dt))
        assert torch.equal(_bits(after[ps2[0]]["exp_avg_sq"], dt), _bits(before[ps2[0]]["exp_avg_sq"], dt))
        assert not after[ps2[1]]["exp_avg"].any() and not after[ps2[1]]["exp_avg_sq"].any()


def _entry(rank, world, store, errq):
    sys.path[:0] = [ROOT, HERE]
    try:
        dist.init_process_group("gloo", init_method="file://" + store, rank=rank,
                                world_size=world)
        import test_sharded_adam as mod
        mod.body_sharded(rank, world)
        dist.barrier()
    except Exception:
        errq.put("rank %d: %s" % (rank, traceback.format_exc()))
        raise
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_adam_over_gloo(world):
    ctx = mp.get_context("spawn")
    errq = ctx.SimpleQueue()
    store = os.path.join(tempfile.mkdtemp(prefix="kfadam"), "store")
    procs = [ctx.Process(target=_entry, args=(r, world, store, errq)) for r in range(world)]
    for p in procs:
        p.start()
    hung = join_all(procs, 600)
    errs = []
    while not errq.empty():
        errs.append(errq.get())
    assert not errs, "\n".join(errs)
    assert not hung and all(p.exitcode == 0 for p in procs), hung_msg(hung, [p.exitcode for p in procs])
