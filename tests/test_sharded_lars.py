"""ShardedLARSOptimizer without a GPU: tests/lars_ref.py against torch.optim.SGD,
the C entries' argument checks, the optimizer's refusals, and the whole step over
tests/adam8_cpu.py's in-process loopback with a numpy epilogue."""
import ctypes
import types

import numpy as np
import pytest
import torch

import adam8_cpu
import cpu_epilogue
import lars_ref
from adam8_cpu import to_numpy, to_torch

ERR_ARG = 3
F32, I32, F16 = 0x20408, 0x10408, 0x20208
MEASURED = 2.0 ** -50  # the largest |torch - lars_ref| of the rows below


@pytest.mark.parametrize("momentum,dampening,nesterov,wd", [
    (0.0, 0.0, False, 0.0), (0.9, 0.0, False, 1e-4), (0.9, 0.1, False, 1e-4),
    (0.9, 0.0, True, 1e-4), (0.8, 0.0, True, 0.0)])
def test_restatement_against_torch(momentum, dampening, nesterov, wd):
    """lars_ref in f64 against torch.optim.SGD(foreach=False) in f64 fed
    ratio * (g + wd * p) with weight_decay=0, over 5 steps. Tensor 0 adapts;
    tensors 1, 2 and 3 have ratio 1 through adapt off, a zero parameter norm
    and a zero gradient norm. Not bit-exact: torch may fuse add_(alpha=). The
    largest deviation measured is 2^-50 = 8.88e-16 (momentum 0.9 alone; 2^-51
    on the other rows); the bound is 8 times it."""
    n, rng = 1009, np.random.default_rng(5)
    ps = [rng.standard_normal(n) for _ in range(4)]
    ps[2] = np.zeros(n)
    hs = [lars_ref.hyper(0.1, momentum, dampening, wd, nesterov, first=True, trust_coefficient=0.02,
                         adapt=a) for a in (True, False, True, True)]
    ms = [np.zeros(n) for _ in ps]
    tps = [torch.from_numpy(p.copy()).requires_grad_() for p in ps]
    opts = [torch.optim.SGD([tp], lr=0.1, momentum=momentum, dampening=dampening,
                            nesterov=nesterov, foreach=False) for tp in tps]
    for step in range(5):
        gs = [rng.standard_normal(n) for _ in ps]
        gs[3] = np.zeros(n)
        for h, o in zip(hs, opts):
            h["first"], h["lr"] = step == 0, 0.1 * 0.5 ** step
            o.param_groups[0]["lr"] = h["lr"]
        ps2, ms, ratios = lars_ref.step_tensors(ps, gs, ms, "f64", hs)
        # both branches of the ratio, on the restatement's own values
        assert ratios[0] != 1.0 and np.isfinite(ratios[0]) and ratios[1] == ratios[3] == 1.0
        assert step > 0 or ratios[2] == 1.0
        for tp, o, p, g, r in zip(tps, opts, ps, gs, ratios):
            tp.grad = torch.from_numpy(r * (g + wd * p))
            o.step()
        ps = ps2
    worst = max(float(np.max(np.abs(tp.detach().numpy() - p))) for tp, p in zip(tps, ps))
    print("max |torch - lars_ref| after 5 steps: %.3g" % worst)
    assert worst <= 8 * MEASURED


def test_lars_c_entries_arg_errors():
    """Every check of the LARS entries comes before any HIP call."""
    from kungfu_amd import _lib
    lib, pa = _lib.load(), _lib.ptr_array
    cnt = (ctypes.c_size_t * 1)(4)
    groups = _lib.lars_group_array([lars_ref.hyper(0.1)])
    good = [8, 1, 1, 8, groups, 1, 0, 8, 8, None]
    # null sq, world < 1, null group_of, null groups, ngroup < 1, np < 0, null coef, null ratio
    for i, bad in ((0, None), (1, 0), (3, None), (4, None), (5, 0), (6, -1), (7, None), (8, None)):
        assert lib.kf_lars_trust_update(*good[:i], bad, *good[i + 1:]) == ERR_ARG, i

    def refused(code, p=16, g=32, m=48, p16=None, counts=cnt, tensor=0, dt=F32):
        tensors = (ctypes.c_int * 1)(tensor)
        made = lib.kf_lars_apply_create(p and pa([p]), pa([g]), pa([m]), p16 and pa([p16]), counts,
                                        tensors, 1, 1, dt)
        return not made and code in lib.kf_last_error().decode()

    assert refused("KF_ERR_ARG", p=None) and refused("KF_ERR_ARG", counts=None)   # null tables
    assert refused("KF_ERR_DTYPE", dt=I32) and refused("KF_ERR_DTYPE", dt=F16)    # F16: no params16
    assert refused("KF_ERR_DTYPE", p16=64)                                      # params16 with f32
    assert refused("offset", p=20) and refused("offset", g=36) and refused("offset", m=52)
    assert refused("offset", p16=66, dt=F16) and refused("KF_ERR_ARG", tensor=1)
    assert lib.kf_lars_apply_run(None, 8, 0, None) == ERR_ARG


def test_construction_rules_and_refusals():
    from kungfu_amd import optimizers as kopt
    from kungfu_amd.torch import optimizers as topt
    assert "ShardedLARSOptimizer" in topt.__all__
    m = torch.nn.Linear(5, 3)
    p16 = [torch.nn.Parameter(torch.zeros(8, dtype=t)) for t in (torch.bfloat16, torch.float16)]

    def sgd(params=None, **options):
        o = torch.optim.SGD(params or m.parameters(), lr=0.1, momentum=0.9)
        o.param_groups[0].update(options)
        return o

    no_gather = types.SimpleNamespace(world=1, rank=0, reduce_shards_=0, grad_shards_=0,
                                      gather_doubles_=0)
    o = topt.ShardedLARSOptimizer(sgd(), m.named_parameters(), always_adapt=True)
    assert isinstance(o, torch.optim.SGD) and len(o.state) == 0 and o._kf_always_adapt is True
    assert o.momentum_buffers() == {} and o.last_trust_ratios() == {}
    kopt.ShardedLARSOptimizer(sgd(p16), master_weights=True)
    for error, word, opt, kw in (
            (TypeError, "torch.optim.SGD", torch.optim.Adam(m.parameters()), {}),
            (ValueError, "maximize", sgd(maximize=True), {}),
            (ValueError, "differentiable", sgd(differentiable=True), {}),
            (TypeError, "master_weights=True", sgd(p16[:1]), {}),
            (TypeError, "master_weights=True", sgd(p16[1:]), {}),
            (ValueError, "gather_params_", sgd(), {"exchange": no_gather}),
            (ValueError, "trust_coefficient", sgd(), {"trust_coefficient": 0}),
            (ValueError, "trust_coefficient", sgd(), {"trust_coefficient": float("nan")}),
            (ValueError, "eps", sgd(), {"eps": -1e-9})):
        with pytest.raises(error, match=word):
            kopt.ShardedLARSOptimizer(opt, **kw)


# the model: an adapting and a non-adapting group of NUMELS each, in two padded buckets each
NUMELS = [1000, 5, 0, 1031, 7]
BUCKET_ELTS = 1500
GROUP_HYPER = ({"lr": 0.05, "momentum": 0.9, "dampening": 0.0, "nesterov": True, "weight_decay": 1e-2},
               {"lr": 0.02, "momentum": 0.8, "dampening": 0.1, "nesterov": False, "weight_decay": 0.0})
TRUST = 0.02


def _arr(t):  # a CPU tensor's values as numpy (bf16 widened)
    return lars_ref.widen16(cpu_epilogue._np(t), "bf16") if t.dtype == torch.bfloat16 else t.numpy()


class CpuLarsEpilogue(cpu_epilogue.CpuEpilogue):
    """Plus the LARS passes, from lars_ref. used: every step's (gathered sums [world][2T],
    np); fed: those of another run (a device adds in another order) to use instead."""

    def __init__(self, fed=()):
        self.fed, self.used = iter(fed), []

    def sq_norm_plan(self, tensors):
        def run(mode, out):
            sq = [lars_ref.sq_sum(_arr(t)) for t in tensors]
            out.copy_(torch.tensor(sq + [float(np.sum(sq))], dtype=torch.float64))
        return types.SimpleNamespace(run=run)

    def lars_trust_update_(self, sq, world, group_of, groups, coef, ratio, np_=0):
        self.used.append(next(self.fed, (sq.numpy().reshape(world, -1).copy(), np_)))
        c = lars_ref.trust(self.used[-1][0], [groups[j] for j in group_of.tolist()],
                           self.used[-1][1])
        coef.copy_(torch.from_numpy(c.reshape(-1)))
        ratio.copy_(torch.from_numpy(c[:, 0].copy()))

    def lars_apply_plan(self, params, grads, moms, tensors, ntensor, params16=None):
        def run(coef, np_):
            for p, g, m, t, p16 in zip(params, grads, moms, tensors, params16 or [None] * len(moms)):
                a, mom = p.numpy(), m.numpy()
                a[...], mom[...] = lars_ref.apply(a.copy(), _arr(g), mom.copy(),
                                                  coef.numpy()[6 * t:6 * t + 6], "f32", np_)
                if p16 is not None:
                    cpu_epilogue._np(p16).view(np.uint16)[...] = lars_ref.narrow16(a, "bf16")
        return types.SimpleNamespace(run=run)


def model_arrays(kind):
    """Both groups' initial parameters; tensor 1 of each group is all zeros."""
    out = adam8_cpu.model_arrays(kind, 3) + adam8_cpu.model_arrays(kind, 4)
    for j in (1, len(NUMELS) + 1):
        out[j] = np.zeros_like(out[j])
    return out


def grad_arrays(world, step):
    """[rank][param] f32, exact in bf16; every world averages to the same values."""
    a, b = adam8_cpu.grad_arrays(world, step, seed=11), adam8_cpu.grad_arrays(world, step, seed=12)
    return [x + y for x, y in zip(a, b)]


def make_optimizer(exchange, kind, device="cpu"):
    from kungfu_amd.optimizers import ShardedLARSOptimizer
    ps = [torch.nn.Parameter(to_torch(a, kind).to(device)) for a in model_arrays(kind)]
    k = len(NUMELS)
    groups = [dict(GROUP_HYPER[0], params=ps[:k]), dict(GROUP_HYPER[1], params=ps[k:])]
    opt = ShardedLARSOptimizer(torch.optim.SGD(groups, lr=0.1), exchange=exchange,
                               bucket_bytes=BUCKET_ELTS * ps[0].element_size(),
                               master_weights=kind != "f32", trust_coefficient=TRUST)
    return ps, opt


def feed(ps, opt, kind, world, rank, s, device="cpu"):
    """Step s's gradients and lr (halved s times)."""
    for g, h in zip(opt.param_groups, GROUP_HYPER):
        g["lr"] = h["lr"] * 0.5 ** s
    for p, g in zip(ps, grad_arrays(world, s)[rank]):
        p.grad = to_torch(adam8_cpu.narrow(g, kind), kind).to(device)


def snapshot(ps, opt):
    """Parameters, momentum and master buffers (in parameter order) and ratios."""
    ratios = opt.last_trust_ratios()
    return ([to_numpy(p) for p in ps], [to_numpy(t) for t in opt.momentum_buffers().values()],
            [to_numpy(t) for t in opt.master_buffers().values()], [ratios[p] for p in ps])


def run_ranks(world, kind, steps, load=None, fed=()):
    """On the numpy epilogue, from the snapshot `load` -> ({rank: snapshot}, rank 0's used)."""
    got, used = {}, {}

    def body(rank, ex):
        ps, opt = make_optimizer(ex, kind)
        live = [p for p in ps if p.numel()]
        for p, a in zip(ps, load[0] if load else ()):
            p.data.copy_(to_torch(a, kind))
        if load:
            opt.load_momentum_buffers({p: torch.from_numpy(a) for p, a in zip(live, load[1])})
            opt.load_master_buffers({p: torch.from_numpy(a) for p, a in zip(live, load[2])})
        for s in steps:
            feed(ps, opt, kind, world, rank, s)
            opt.step()
        assert len(opt.state) == 0 and sum(len(G["pb"].buckets) for G in opt._kf_groups) == 4
        got[rank], used[rank] = snapshot(ps, opt), ex.epilogue.used

    adam8_cpu.loop_ranks(world, body, epilogue=lambda: CpuLarsEpilogue(fed))
    return got, used[0]


def reference_run(kind, steps, used):
    """snapshot()'s tuple by lars_ref on the unsharded tensors and the steps' gathered sums."""
    k = len(NUMELS)
    w = [adam8_cpu.widen(a, kind) for a in model_arrays(kind)]
    ms = [np.zeros(a.size, np.float32) for a in w]
    for i, (s, (sq, np_)) in enumerate(zip(steps, used)):
        gs = [g * np.float32(max(np_, 1)) for g in grad_arrays(1, s)[0]]  # before the / np
        hs = [lars_ref.hyper(**dict(h, lr=h["lr"] / 2 ** s), first=i == 0, trust_coefficient=TRUST)
              for h in GROUP_HYPER for _ in range(k)]
        assert np.allclose(sq.sum(0), [lars_ref.sq_sum(a) for a in w + gs], rtol=2.0 ** -40)
        w, ms, ratios = lars_ref.step_tensors(w, gs, ms, "f32", hs, np_, sums=sq)
    assert all(r == 1.0 for r in ratios[k:]) and ratios[0] != 1.0 and ratios[3] != 1.0
    live = [j for j, n in enumerate(NUMELS * 2) if n]
    return ([adam8_cpu.narrow(a, kind) for a in w], [ms[j] for j in live],
            [w[j] for j in live] if kind != "f32" else [], list(ratios))


def assert_same(got, want):
    for a, b, what in zip(got, want, ("params", "momentum", "master", "ratios")):
        assert len(a) == len(b), what
        for j, (x, y) in enumerate(zip(a, b)):
            assert np.asarray(x).tobytes() == np.asarray(y).tobytes(), (what, j)


@pytest.mark.parametrize("worlds", [(1,), (2,), (4,), (2, 4)])
@pytest.mark.parametrize("kind", ["f32", "bf16"])
def test_sharded_lars_against_reference(kind, worlds):
    """4 steps, bit for bit; (2, 4): momentum (and master) saved after step 2
    at world 2 and resumed at world 4."""
    got, used = None, []
    for world, steps in zip(worlds, np.array_split(range(4), len(worlds))):
        got, more = run_ranks(world, kind, list(steps), load=got and got[0])
        used += more
    want = reference_run(kind, range(4), used)
    for r in got:
        assert_same(got[r], want)
    assert len(got[0][2]) == (0 if kind == "f32" else 8)
