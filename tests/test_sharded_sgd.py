"""ShardedSGDOptimizer without a GPU: the numpy restatement of the update
(tests/sgd_ref.py) against torch.optim.SGD, the optimizer's construction
rules, the C ABI's argument checks (no device touched), and the whole
reduce-scatter -> update -> all-gather step over gloo with a CPU epilogue."""
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

import cpu_epilogue
import sgd_ref
from procs import hung_msg, join_all

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

# (momentum, dampening, weight_decay, nesterov)
ROWS = [(0.0, 0.0, 0.0, False), (0.9, 0.0, 0.0, False), (0.9, 0.0, 1e-2, True),
        (0.9, 0.1, 5e-4, False)]


# ---- the restatement against torch ------------------------------------------

@pytest.mark.parametrize("mu,damp,wd,nesterov", ROWS)
def test_restatement_against_torch(mu, damp, wd, nesterov):
    """sgd_ref against torch.optim.SGD(foreach=False) on CPU, f32. Not
    bit-exact: torch's CPU kernels fuse a + alpha*b. On standard-normal data
    the largest absolute difference after these 4 steps was 4.8e-7 for every
    row; the bound is four times that. This pins the restatement, not the
    kernel."""
    n, lrs = 100003, (0.1, 0.05, 0.2, 0.01)
    rng = np.random.default_rng(7)
    p0 = rng.standard_normal(n).astype(np.float32)
    grads = [rng.standard_normal(n).astype(np.float32) for _ in lrs]
    tp = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    opt = torch.optim.SGD([tp], lr=lrs[0], momentum=mu, dampening=damp, weight_decay=wd,
                          nesterov=nesterov, foreach=False)
    p, m = p0.copy(), (np.zeros(n, np.float32) if mu else None)
    for i, (lr, g) in enumerate(zip(lrs, grads)):
        opt.param_groups[0]["lr"] = lr
        tp.grad = torch.from_numpy(g.copy())
        opt.step()
        p, m = sgd_ref.step(p, g, m, "f32", sgd_ref.hyper(lr, mu, damp, wd, nesterov, i == 0))
    diff = float(np.max(np.abs(tp.detach().numpy() - p)))
    print("max |torch - sgd_ref| after 4 steps: %.3g" % diff)
    np.testing.assert_allclose(tp.detach().numpy(), p, rtol=0, atol=2e-6)
    if mu:
        np.testing.assert_allclose(opt.state[tp]["momentum_buffer"].numpy(), m, rtol=0, atol=2e-6)


# ---- construction ------------------------------------------------------------

def _lin():
    torch.manual_seed(0)
    return torch.nn.Linear(5, 3)


class _NoSgdExchange:
    world, rank = 1, 0

    def all_reduce_(self, buckets, **kw):
        return buckets


def test_construction_rules():
    from kungfu_amd import optimizers as kopt
    from kungfu_amd.torch import optimizers as topt
    assert "ShardedSGDOptimizer" in topt.__all__
    m = _lin()
    o = kopt.ShardedSGDOptimizer(torch.optim.SGD(m.parameters(), lr=0.1, momentum=0.9))
    assert isinstance(o, torch.optim.SGD)
    assert len(o.state) == 0
    assert o.momentum_buffers() == {}
    torch.optim.lr_scheduler.StepLR(o, step_size=1)  # takes it for an optimizer
    o2 = topt.ShardedSGDOptimizer(torch.optim.SGD(m.parameters(), lr=0.1), m.named_parameters())
    assert isinstance(o2, torch.optim.SGD) and len(o2.state) == 0
    with pytest.raises(TypeError):
        kopt.ShardedSGDOptimizer(torch.optim.Adam(m.parameters(), lr=0.1))
    with pytest.raises(ValueError, match="maximize"):
        kopt.ShardedSGDOptimizer(torch.optim.SGD(m.parameters(), lr=0.1, maximize=True))
    with pytest.raises(ValueError, match="differentiable"):
        kopt.ShardedSGDOptimizer(torch.optim.SGD(m.parameters(), lr=0.1, differentiable=True))
    with pytest.raises(ValueError, match="sgd_step_"):
        kopt.ShardedSGDOptimizer(torch.optim.SGD(m.parameters(), lr=0.1),
                                 exchange=_NoSgdExchange())
    doc = kopt.ShardedSGDOptimizer.__doc__
    for words in ("zero gradient", "p.grad does not hold", "overlap=True", "hierarchical"):
        assert words in doc, words


# ---- C ABI argument errors (no device) --------------------------------------

OK, ERR_DTYPE, ERR_ARG = 0, 1, 3
F32, I32, F16, BF16, F64 = 0x20408, 0x10408, 0x20208, 0x20209, 0x20808


def test_sgd_update_batch_arg_errors():
    """Every check of kf_sgd_update_batch comes before any HIP call."""
    from kungfu_amd import _lib
    lib = _lib.load()
    pa = _lib.ptr_array
    cnt = lambda *v: (ctypes.c_size_t * len(v))(*v)  # noqa: E731
    plain = _lib.sgd_hyper_array([sgd_ref.hyper(0.1)])
    mom = _lib.sgd_hyper_array([sgd_ref.hyper(0.1, 0.9)])

    def call(params, grads, moms, counts, nb, dt=F32, np_=0, hyper=plain):
        return lib.kf_sgd_update_batch(params, grads, moms, counts, nb, dt, np_, hyper, None)

    assert call(None, None, None, None, 0) == OK                       # nb == 0
    assert call(pa([16]), pa([32]), None, cnt(0), 1) == OK            # an empty segment
    assert call(pa([0]), pa([0]), None, cnt(0), 1, hyper=mom) == OK
    assert call(pa([16]), pa([32]), None, cnt(4), -1) == ERR_ARG      # nb < 0
    assert call(None, pa([32]), None, cnt(4), 1) == ERR_ARG           # null tables
    assert call(pa([16]), None, None, cnt(4), 1) == ERR_ARG
    assert call(pa([16]), pa([32]), None, None, 1) == ERR_ARG
    assert call(pa([16]), pa([32]), None, cnt(4), 1, hyper=None) == ERR_ARG
    assert call(pa([0]), pa([32]), None, cnt(4), 1) == ERR_ARG        # null pointer, count > 0
    assert call(pa([16]), pa([0]), None, cnt(4), 1) == ERR_ARG
    assert call(pa([24]), pa([32]), None, cnt(4), 1) == ERR_ARG       # off the 16-byte boundary
    assert call(pa([16]), pa([36]), None, cnt(4), 1) == ERR_ARG
    assert call(pa([16]), pa([32]), pa([56]), cnt(4), 1, hyper=mom) == ERR_ARG
    assert call(pa([16]), pa([32]), None, cnt(4), 1, np_=-1) == ERR_ARG
    assert call(pa([16]), pa([32]), pa([0]), cnt(4), 1, hyper=mom) == ERR_ARG  # momentum, no buffer
    assert call(pa([16]), pa([32]), None, cnt(4), 1, hyper=mom) == ERR_ARG
    for dt in (I32, 0x00108, 0x30108, 0x12345):
        assert call(pa([16]), pa([32]), None, cnt(4), 1, dt=dt) == ERR_DTYPE
    assert b"kf_sgd_update_batch" in lib.kf_last_error()


def test_exchange_sgd_batch_needs_an_exchange():
    """Without a device there is no exchange to hand over: the null handle is
    refused before anything else (the counts % world check needs a world;
    tests/test_sharded_sgd_gpu.py makes it on a loopback group)."""
    from kungfu_amd import _lib
    lib = _lib.load()
    pa = _lib.ptr_array
    h = _lib.sgd_hyper_array([sgd_ref.hyper(0.1)])
    cnt = (ctypes.c_size_t * 1)(4)
    assert lib.kf_exchange_sgd_batch(None, pa([16]), pa([32]), None, cnt, 1, F32, h, 0, None) == ERR_ARG
    assert lib.kf_exchange_sgd_batch(None, None, None, None, None, 0, F32, h, 0, None) == ERR_ARG


# ---- gloo, worlds 2 and 3 ----------------------------------------------------

class CpuSgdEpilogue(cpu_epilogue.CpuEpilogue):
    """cpu_epilogue.CpuEpilogue plus the SGD update, from sgd_ref."""

    def sgd_update_(self, params, grads, moms, hypers, np_):
        for p, g, m, h in zip(params, grads, moms, hypers):
            dt = cpu_epilogue._DT[p.dtype]
            pa, ga = cpu_epilogue._np(p), cpu_epilogue._np(g)
            ma = cpu_epilogue._np(m) if m is not None else None
            np2, nm = sgd_ref.step(np.ascontiguousarray(pa), np.ascontiguousarray(ga),
                                   None if ma is None else np.ascontiguousarray(ma), dt, h, np_)
            pa[...] = np2
            if ma is not None and float(h.get("momentum", 0.0)) != 0:
                ma[...] = nm
        return params


SHAPES = ((7, 5), (5,), (3, 5))
GROUPS = ((0, 1), (2,))  # parameter indices of the two param groups
GROUP_HYPER = ({"lr": 0.1, "weight_decay": 1e-2, "momentum": 0.9, "nesterov": True},
               {"lr": 0.05, "weight_decay": 0.0, "momentum": 0.9, "dampening": 0.1})
STEPS = 3
_TORCH = {"f32": torch.float32, "bf16": torch.bfloat16}


def model_arrays(dt, seed=3):
    """Initial parameters (the same on every rank), in dt's numpy form."""
    rng = np.random.default_rng(seed)
    out = []
    for shp in SHAPES:
        a = rng.standard_normal(shp).astype(np.float32)
        out.append(sgd_ref.f32_to_bf16_bits(a) if dt == "bf16" else a)
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
            gs.append(sgd_ref.f32_to_bf16_bits(a) if dt == "bf16" else a)
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


def reference_run(dt, world, steps=STEPS, skip=None):
    """(params, momenta) after `steps` steps: sgd_ref applied to
    oracle.reduce_avg of the ranks' gradients, lr halved after every step.
    skip = (step, param): that parameter has no gradient there (zeros)."""
    from oracle import oracle
    ps = model_arrays(dt)
    ms = [None] * len(ps)
    lr_scale = 1.0
    for s in range(steps):
        gr = grad_arrays(dt, world, s)
        for gi, idx in enumerate(GROUPS):
            h = dict(GROUP_HYPER[gi], first=(s == 0))
            h["lr"] = h["lr"] * lr_scale
            for j in idx:
                ins = [np.ascontiguousarray(gr[r][j].reshape(-1)) for r in range(world)]
                if skip == (s, j):
                    ins = [np.zeros_like(x) for x in ins]
                avg = oracle.reduce_avg(ins, dt, world)
                p, m = sgd_ref.step(ps[j].reshape(-1), avg, ms[j], dt, h)
                ps[j], ms[j] = p.reshape(SHAPES[j]), m
        lr_scale *= 0.5
    return ps, ms


def make_optimizer(dt, exchange, device="cpu"):
    from kungfu_amd.optimizers import ShardedSGDOptimizer
    ps = [torch.nn.Parameter(to_torch(a, dt).to(device)) for a in model_arrays(dt)]
    groups = [dict(GROUP_HYPER[gi], params=[ps[j] for j in idx]) for gi, idx in enumerate(GROUPS)]
    return ps, ShardedSGDOptimizer(torch.optim.SGD(groups, lr=0.1), exchange=exchange)


def run_steps(ps, opt, dt, world, rank, device="cpu", skip=None, first_step=0, steps=STEPS):
    for s in range(first_step, first_step + steps):
        gr = grad_arrays(dt, world, s)[rank]
        for j, p in enumerate(ps):
            p.grad = None if skip == (s, j) else to_torch(gr[j], dt).to(device)
        opt.step()
        for g in opt.param_groups:
            g["lr"] = g["lr"] * 0.5


def body_sharded(rank, world):
    from kungfu_amd.collective import Exchange
    for dt in ("f32", "bf16"):
        ex = Exchange(epilogue=CpuSgdEpilogue())
        ps, opt = make_optimizer(dt, ex)
        run_steps(ps, opt, dt, world, rank)
        assert len(opt.state) == 0
        want_p, want_m = reference_run(dt, world)
        for j, p in enumerate(ps):
            assert np.array_equal(to_numpy(p, dt), want_p[j]), (dt, "param", j)
        # every rank's parameters are bit-identical
        flat = torch.cat([torch.from_numpy(to_numpy(p, dt).reshape(-1).view(
            np.int16 if dt == "bf16" else np.int32).astype(np.int32)) for p in ps])
        allf = [torch.empty_like(flat) for _ in range(world)]
        dist.all_gather(allf, flat)
        for f in allf:
            assert torch.equal(f, flat), dt
        mb = opt.momentum_buffers()
        assert set(mb) == set(ps)
        for j, p in enumerate(ps):
            assert mb[p].shape == p.shape
            assert np.array_equal(to_numpy(mb[p], dt).reshape(-1), want_m[j]), (dt, "momentum", j)
        # load_momentum_buffers round-trips: a fresh optimizer over the same
        # parameters takes the buffers and goes on as the first one does
        ps2 = [torch.nn.Parameter(p.detach().clone()) for p in ps]
        from kungfu_amd.optimizers import ShardedSGDOptimizer
        at = {id(p): i for i, p in enumerate(ps)}
        groups = [dict(g, params=[ps2[at[id(p)]] for p in g["params"]]) for g in opt.param_groups]
        opt2 = ShardedSGDOptimizer(torch.optim.SGD(groups, lr=0.1),
                                   exchange=Exchange(epilogue=CpuSgdEpilogue()))
        opt2.load_momentum_buffers({ps2[at[id(p)]]: b for p, b in mb.items()})
        mb2 = opt2.momentum_buffers()
        for p, q in zip(ps, ps2):
            assert torch.equal(mb2[q].view(torch.int16 if dt == "bf16" else torch.int32),
                               mb[p].view(torch.int16 if dt == "bf16" else torch.int32))
        run_steps(ps, opt, dt, world, rank, first_step=STEPS, steps=1)
        run_steps(ps2, opt2, dt, world, rank, first_step=STEPS, steps=1)
        for p, q in zip(ps, ps2):
            assert np.array_equal(to_numpy(p, dt), to_numpy(q, dt)), dt


def _entry(rank, world, store, errq):
    sys.path[:0] = [ROOT, HERE]
    try:
        dist.init_process_group("gloo", init_method="file://" + store, rank=rank,
                                world_size=world)
        import test_sharded_sgd as mod
        mod.body_sharded(rank, world)
        dist.barrier()
    except Exception:
        errq.put("rank %d: %s" % (rank, traceback.format_exc()))
        raise
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_sgd_over_gloo(world):
    ctx = mp.get_context("spawn")
    errq = ctx.SimpleQueue()
    store = os.path.join(tempfile.mkdtemp(prefix="kfsgd"), "store")
    procs = [ctx.Process(target=_entry, args=(r, world, store, errq)) for r in range(world)]
    for p in procs:
        p.start()
    hung = join_all(procs, 600)
    errs = []
    while not errq.empty():
        errs.append(errq.get())
    assert not errs, "\n".join(errs)
    assert not hung and all(p.exitcode == 0 for p in procs), hung_msg(hung, [p.exitcode for p in procs])
