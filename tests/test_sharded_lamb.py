"""ShardedLAMBOptimizer without a GPU: the numpy restatement of the step
(tests/lamb_ref.py) against a straightforward torch-tensor LAMB, the piece
builder, the optimizer's construction rules, the C ABI's argument checks (no
device touched), and the whole step over gloo with a numpy epilogue."""
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
import lamb_ref
from procs import hung_msg, join_all

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

OK, ERR_DTYPE, ERR_ARG = 0, 1, 3
F32, I32, F16, BF16, F64 = 0x20408, 0x10408, 0x20208, 0x20209, 0x20808

# kf_lamb.hip: segments per launch of the two moments kernels
LAMB_SEG, LAMB_MASTER_SEG = 24, 32


def test_launch_constants_pinned():
    """What tests/test_sharded_lamb_gpu.py sizes its segments by."""
    src = open(os.path.join(ROOT, "kungfu_amd", "csrc", "kf_lamb.hip")).read()
    assert int(re.search(r"constexpr int kLambSeg\s*=\s*(\d+);", src).group(1)) == LAMB_SEG
    assert int(re.search(r"constexpr int kLambMasterSeg\s*=\s*(\d+);", src).group(1)) == \
        LAMB_MASTER_SEG
    assert "plan_update_batch<LambArgs<C, NSEG>>(" in src and '#include "kf_lamb_math.hpp"' in src
    # kf_adam_math.hpp's update is not LAMB's: the shared header is its own
    math = open(os.path.join(ROOT, "kungfu_amd", "csrc", "kf_lamb_math.hpp")).read()
    assert "lamb_math" in math and '#include "kf_adam_math.hpp"' in math


# ---- the restatement against a torch-tensor LAMB -------------------------------

# (weight_decay, always_adapt)
ROWS = [(0.0, False), (0.0, True), (1e-2, False)]

# The largest |torch - lamb_ref| measured for (p, m, v) on the data of
# test_restatement_against_torch, per row. The test's bounds
# are four times these.
MEASURED = {(0.0, False): (2.0 ** -22, 2.0 ** -24, 2.0 ** -29),
            (0.0, True): (2.0 ** -22, 2.0 ** -24, 2.0 ** -29),
            (1e-2, False): (2.0 ** -22, 2.0 ** -24, 2.0 ** -29)}


def _torch_lamb_step(p, g, m, v, lr, wd, adapt, step, betas=(0.9, 0.999), eps=1e-6):
    """LAMB on torch tensors as apex FusedLAMB states it (bias correction on,
    no gradient clipping), written the plain way."""
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
def test_restatement_against_torch(wd, always_adapt):
    """lamb_ref against the torch-tensor LAMB above on CPU, f32, on the data
    of tests/test_sharded_adam.py's restatement test. Not
    bit-exact: torch fuses a + alpha*b, divides v by the bias correction
    before the sqrt, and takes its norms its own way. MEASURED has the largest
    absolute differences after these 4 steps; each bound is four times the
    measured value. This pins the restatement, not the kernel."""
    n, lrs = 100003, (1e-3, 5e-4, 2e-3, 1e-4)
    rng = np.random.default_rng(7)
    p0 = rng.standard_normal(n).astype(np.float32)
    grads = [rng.standard_normal(n).astype(np.float32) for _ in lrs]
    adapt = wd != 0 or always_adapt
    tp, tm, tv = torch.from_numpy(p0.copy()), torch.zeros(n), torch.zeros(n)
    p, m, v = p0.copy(), np.zeros(n, np.float32), np.zeros(n, np.float32)
    for i, (lr, g) in enumerate(zip(lrs, grads)):
        _torch_lamb_step(tp, torch.from_numpy(g.copy()), tm, tv, lr, wd, adapt, i + 1)
        h = lamb_ref.hyper(lr, weight_decay=wd, step=i + 1, adapt=adapt)
        (p,), (m,), (v,), _ = lamb_ref.step_tensors([p], [g], [m], [v], "f32", [h], [[(0, n)]])
    diffs = [float(np.max(np.abs(a - b))) for a, b in
             ((tp.numpy(), p), (tm.numpy(), m), (tv.numpy(), v))]
    print("max |torch - lamb_ref| after 4 steps (p, m, v): %.3g %.3g %.3g" % tuple(diffs))
    for d, measured, what in zip(diffs, MEASURED[(wd, always_adapt)], "pmv"):
        assert d <= 4 * measured, (what, d, measured)


# ---- the piece builder -----------------------------------------------------------

NUMELS = [5, 0, 1031, 7, 2050, 3]


def test_piece_builder_covers_every_element_once():
    from kungfu_amd.collective import GradBuckets
    from kungfu_amd.optimizers import lamb_pieces
    world = 3
    gb = GradBuckets(NUMELS, torch.float32, "cpu", world, bucket_bytes=6000)
    assert len(gb.buckets) >= 2
    seen = [np.zeros(b.numel(), np.int64) for b in gb.buckets]
    owner = [np.full(b.numel(), -1, np.int64) for b in gb.buckets]
    ranks_of = {t: [] for t in range(len(NUMELS))}
    for r in range(world):
        pieces = lamb_pieces(gb, world, r)
        assert len({t for t, _, _, _ in pieces}) == len(pieces)  # at most one per tensor
        for t, b, off, n in pieces:
            q = gb.buckets[b].numel() // world
            assert n > 0 and 0 <= off and off + n <= q
            seen[b][r * q + off:r * q + off + n] += 1
            owner[b][r * q + off:r * q + off + n] = t
            ranks_of[t].append(r)
    for t, (v, n) in enumerate(zip(gb.views, NUMELS)):
        for b, bucket in enumerate(gb.buckets):
            lo = bucket.data_ptr()
            if n and lo <= v.data_ptr() < lo + bucket.numel() * 4:
                s = (v.data_ptr() - lo) // 4
                assert (seen[b][s:s + n] == 1).all() and (owner[b][s:s + n] == t).all(), t
    for b, span in enumerate(gb.spans):
        assert seen[b][:span].sum() == span and not seen[b][span:].any()  # padding in none
    assert ranks_of[1] == []                    # the zero-element tensor
    assert ranks_of[2] == [0, 1, 2]             # straddles every shard boundary
    assert ranks_of[3] == [2]                   # wholly on another rank than 0
    starts = {(t, off) for r in range(world) for t, _, off, _ in lamb_pieces(gb, world, r)}
    assert (2, 5) in starts                     # an element offset that is no 16-byte multiple


# ---- construction and refusals ----------------------------------------------------

def _lin():
    torch.manual_seed(0)
    return torch.nn.Linear(5, 3)


class _NoGatherExchange:
    world, rank = 1, 0

    def reduce_shards_(self, *a):
        return 1

    def grad_shards_(self, *a):
        return []

    def gather_doubles_(self, *a):
        return None


def test_construction_rules_and_refusals():
    from kungfu_amd import optimizers as kopt
    from kungfu_amd.torch import optimizers as topt
    assert "ShardedLAMBOptimizer" in topt.__all__
    m = _lin()
    for cls in (torch.optim.Adam, torch.optim.AdamW):
        o = kopt.ShardedLAMBOptimizer(cls(m.parameters(), lr=1e-3))
        assert isinstance(o, cls) and len(o.state) == 0
        assert o.state_buffers() == {} and o.last_trust_ratios() == {}
        torch.optim.lr_scheduler.StepLR(o, step_size=1)  # takes it for an optimizer
    o = topt.ShardedLAMBOptimizer(torch.optim.Adam(m.parameters(), lr=1e-3), m.named_parameters(),
                                  trust_clip=1.0, always_adapt=True)
    assert o._kf_trust_clip == 1.0 and o._kf_always_adapt is True
    for other in (torch.optim.SGD(m.parameters(), lr=0.1), torch.optim.Adamax(m.parameters())):
        with pytest.raises(TypeError):
            kopt.ShardedLAMBOptimizer(other)
    for option in ("amsgrad", "maximize", "capturable", "differentiable"):
        a = torch.optim.Adam(m.parameters(), lr=1e-3)
        a.param_groups[0][option] = True
        with pytest.raises(ValueError, match=option):
            kopt.ShardedLAMBOptimizer(a)
    for kw in ({"max_grad_norm": 1.0}, {"loss_scale": "dynamic"}):
        with pytest.raises(ValueError, match="gated"):
            kopt.ShardedLAMBOptimizer(torch.optim.Adam(m.parameters(), lr=1e-3), **kw)
    with pytest.raises(TypeError):
        kopt.ShardedLAMBOptimizer(torch.optim.Adam(m.parameters(), lr=1e-3), overlap=True)
    for clip in (0, -1.0, float("inf"), float("nan"), True, "1"):
        with pytest.raises(ValueError, match="trust_clip"):
            kopt.ShardedLAMBOptimizer(torch.optim.Adam(m.parameters(), lr=1e-3), trust_clip=clip)
    with pytest.raises(ValueError, match="gather_params_"):
        kopt.ShardedLAMBOptimizer(torch.optim.Adam(m.parameters(), lr=1e-3),
                                  exchange=_NoGatherExchange())
    doc = kopt.ShardedLAMBOptimizer.__doc__
    for words in ("trust_clip", "always_adapt", "Non-finite gradients are not skipped",
                  "overlap=True", "hierarchical", "master_weights", "last_trust_ratios"):
        assert words in doc, words


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_16_bit_parameters_need_master_weights(dtype):
    from kungfu_amd import optimizers as kopt
    p = torch.nn.Parameter(torch.zeros(8, dtype=dtype))
    o = kopt.ShardedLAMBOptimizer(torch.optim.Adam([p], lr=1e-3))
    p.grad = torch.zeros_like(p)
    with pytest.raises(TypeError, match="master_weights=True"):
        o.step()


# ---- C ABI argument errors (no device) ----------------------------------------------

def test_lamb_c_entries_arg_errors():
    """Every check of the LAMB entries comes before any HIP call."""
    from kungfu_amd import _lib
    lib = _lib.load()
    pa = _lib.ptr_array
    cnt = lambda *v: (ctypes.c_size_t * len(v))(*v)  # noqa: E731
    plain = _lib.adam_hyper_array([lamb_ref.hyper(1e-3)])
    five = (pa([16]), pa([32]), pa([48]), pa([64]), pa([80]))
    for fn, good, bad in ((lib.kf_lamb_moments_batch, F32, (F16, BF16, I32)),
                          (lib.kf_lamb_master_moments_batch, F16, (F32, F64, I32))):
        call = lambda t, c, nb, dt=good, np_=0, h=plain: fn(*t, c, nb, dt, np_, h, None)  # noqa: E731
        assert call((None,) * 5, None, 0) == OK
        assert call(five, cnt(0), 1) == OK
        assert call(five, cnt(4), -1) == ERR_ARG
        for i in range(5):
            t = list(five)
            t[i] = None
            assert call(t, cnt(4), 1) == ERR_ARG, i
            t[i] = pa([0])
            assert call(t, cnt(4), 1) == ERR_ARG, i
            t[i] = pa([16 * (i + 1) + 8])
            assert call(t, cnt(4), 1) == ERR_ARG, i
        assert call(five, None, 1) == ERR_ARG and call(five, cnt(4), 1, h=None) == ERR_ARG
        assert call(five, cnt(4), 1, np_=-1) == ERR_ARG
        zero = _lib.adam_hyper_array([lamb_ref.hyper(1e-3, betas=(1.0, 0.999))])
        assert call(five, cnt(4), 1, h=zero) == ERR_ARG
        for dt in bad:
            assert call(five, cnt(4), 1, dt=dt) == ERR_DTYPE, hex(dt)
    groups = (_lib.LambGroup * 1)()
    trust = lib.kf_lamb_trust_update
    assert trust(8, 0, 1, 8, groups, 1, 0.0, 8, 8, None) == ERR_ARG   # world < 1
    assert trust(8, 1, 0, 8, groups, 1, 0.0, 8, 8, None) == ERR_ARG   # no tensor
    assert trust(8, 1, 1, 8, groups, 0, 0.0, 8, 8, None) == ERR_ARG   # no group
    assert trust(None, 1, 1, 8, groups, 1, 0.0, 8, 8, None) == ERR_ARG
    assert trust(8, 1, 1, 8, groups, 1, float("nan"), 8, 8, None) == ERR_ARG
    create = lib.kf_lamb_apply_create
    ints = lambda *v: (ctypes.c_int * len(v))(*v)  # noqa: E731
    assert not create(pa([16]), pa([32]), None, cnt(4), ints(0), 1, 1, I32)      # dtype
    assert not create(pa([16]), pa([32]), None, cnt(4), ints(0), 1, 1, F16)      # no params16
    assert not create(pa([16]), pa([36]), None, cnt(4), ints(0), 1, 1, F32)      # offsets differ
    assert not create(pa([16]), pa([32]), pa([66]), cnt(4), ints(0), 1, 1, F16)  # p16 offset
    assert not create(pa([16]), pa([32]), None, cnt(4), ints(1), 1, 1, F32)      # tensor index
    assert not create(pa([18]), pa([34]), None, cnt(4), ints(0), 1, 1, F32)      # element alignment
    assert b"kf_lamb_apply_create" in lib.kf_last_error()
    assert lib.kf_lamb_apply_run(None, 8, None) == ERR_ARG
    assert lib.kf_exchange_gather_params_batch(None, pa([16]), cnt(4), 1, F32, None) == ERR_ARG


# ---- the model of the gloo and GPU tests ----------------------------------------------

GROUP_HYPER = ({"lr": 0.05, "weight_decay": 1e-2, "betas": (0.9, 0.999), "eps": 1e-6},
               {"lr": 0.02, "weight_decay": 0.0, "betas": (0.8, 0.99), "eps": 1e-6})
STEPS = 3
TRUST_CLIP = 1.7
BUCKET_BYTES = 6000
_T16 = {"f16": torch.float16, "bf16": torch.bfloat16}


def model_arrays(sixteen, seed=3):
    """Initial parameters: NUMELS as f32 (group 0), then NUMELS as 16-bit
    patterns (group 1)."""
    rng = np.random.default_rng(seed)
    a = [rng.standard_normal(n).astype(np.float32) for n in NUMELS]
    b = [lamb_ref.narrow16(rng.standard_normal(n).astype(np.float32), sixteen) for n in NUMELS]
    return a + b


def grad_arrays(world, step, sixteen, seed=11):
    """[rank][param]: multiples of 1/4 in [-8, 8], so that the sum over the
    ranks is exact in every order a transport may add in."""
    out = []
    for r in range(world):
        rng = np.random.default_rng(seed + 100 * step + r)
        gs = [(rng.integers(-32, 33, n) / 4.0).astype(np.float32) for n in NUMELS * 2]
        out.append(gs[:len(NUMELS)] + [lamb_ref.narrow16(g, sixteen) for g in gs[len(NUMELS):]])
    return out


def to_torch(a, sixteen):
    if a.dtype == np.uint16:
        return torch.from_numpy(a.view(np.int16).copy()).view(_T16[sixteen])
    return torch.from_numpy(a.copy())


def to_numpy(t):
    t = t.detach().cpu().contiguous()
    if t.element_size() == 2:
        return t.view(torch.int16).numpy().view(np.uint16).copy()
    return t.numpy().copy()


def make_optimizer(exchange, device="cpu", sixteen="f16"):
    from kungfu_amd.optimizers import ShardedLAMBOptimizer
    ps = [torch.nn.Parameter(to_torch(a, sixteen).to(device)) for a in model_arrays(sixteen)]
    k = len(NUMELS)
    groups = [dict(GROUP_HYPER[0], params=ps[:k]), dict(GROUP_HYPER[1], params=ps[k:])]
    opt = ShardedLAMBOptimizer(torch.optim.AdamW(groups, lr=0.1), exchange=exchange,
                               bucket_bytes=BUCKET_BYTES, master_weights=True,
                               trust_clip=TRUST_CLIP)
    return ps, opt


def set_grads(ps, world, rank, step, device="cpu", sixteen="f16"):
    for p, g in zip(ps, grad_arrays(world, step, sixteen)[rank]):
        p.grad = to_torch(g, sixteen).to(device)


def schedule(opt):
    for g in opt.param_groups:
        g["lr"] = g["lr"] * 0.5


def model_cuts(opt, world):
    """Per bucket group: cuts[t] = [(start, stop) of tensor t's piece on rank
    r, for r in rank order], from the optimizer's own buckets."""
    from kungfu_amd.optimizers import lamb_pieces
    out = []
    for G in opt._kf_groups:
        gb = G["pb"]
        cuts = [[(0, 0)] * world for _ in G["ps"]]
        for r in range(world):
            for t, b, off, n in lamb_pieces(gb, world, r):
                bucket = gb.buckets[b]
                s = (gb.views[t].data_ptr() - bucket.data_ptr()) // bucket.element_size()
                a = r * (bucket.numel() // world) + off - s
                cuts[t][r] = (a, a + n)
        out.append(cuts)
    return out


_REFERENCE = {}


def reference_run(world, sixteen="f16", steps=STEPS, sums=None, cuts=None):
    """The model after `steps` steps by lamb_ref on the unsharded tensors:
    oracle.reduce_avg of the ranks' gradients, the lr halved after every step,
    the norm sums taken per shard (cuts: model_cuts') and added in rank order,
    or the device's own (sums[step][group] of [world][2T]), which are then
    also compared with the host's (sum_checks: device, host, elements).
    Computed once per CPU case and shared; callers leave it unchanged."""
    key = (world, sixteen, steps)
    if sums is None and key in _REFERENCE:
        return _REFERENCE[key]
    from oracle import oracle
    k = len(NUMELS)
    arrs = model_arrays(sixteen)
    w = [a.copy() for a in arrs[:k]] + [lamb_ref.widen16(a, sixteen) for a in arrs[k:]]
    ms, vs = [np.zeros(a.size, np.float32) for a in w], [np.zeros(a.size, np.float32) for a in w]
    ratios, checks, lr_scale = [1.0] * (2 * k), [], 1.0
    for s in range(steps):
        gr = grad_arrays(world, s, sixteen)
        for gi, idx in enumerate((range(0, k), range(k, 2 * k))):
            dt = "f32" if gi == 0 else sixteen
            avg = []
            for j in idx:
                ins = [np.ascontiguousarray(gr[r][j]) for r in range(world)]
                if gi == 1:
                    ins = [x.view(np.float16) if sixteen == "f16" else x for x in ins]
                a = oracle.reduce_avg(ins, dt, world)
                avg.append(a if gi == 0 else lamb_ref.widen16(np.asarray(a).view(np.uint16), sixteen))
            h = lamb_ref.hyper(GROUP_HYPER[gi]["lr"] * lr_scale, betas=GROUP_HYPER[gi]["betas"],
                               eps=GROUP_HYPER[gi]["eps"],
                               weight_decay=GROUP_HYPER[gi]["weight_decay"], step=s + 1)
            idx = list(idx)
            dev = None if sums is None else sums[s][gi]
            if dev is not None:  # the device's sums against the host's, before they are used
                _, _, us = zip(*[lamb_ref.moments(w[j], avg[i], ms[j], vs[j], "f32", h)
                                 for i, j in enumerate(idx)])
                for i, j in enumerate(idx):
                    for r, (a, b) in enumerate(cuts[gi][i]):
                        checks.append((dev[r][i], lamb_ref.sq_sum(w[j][a:b]), b - a))
                        checks.append((dev[r][k + i], lamb_ref.sq_sum(us[i][a:b]), b - a))
            new_p, new_m, new_v, ratio = lamb_ref.step_tensors(
                [w[j] for j in idx], avg, [ms[j] for j in idx], [vs[j] for j in idx], "f32",
                [h] * k, cuts[gi], TRUST_CLIP, sums=dev)
            for i, j in enumerate(idx):
                w[j], ms[j], vs[j], ratios[j] = new_p[i], new_m[i], new_v[i], float(ratio[i])
        lr_scale *= 0.5
    out = {"p": w[:k] + [lamb_ref.narrow16(a, sixteen) for a in w[k:]], "m": ms, "v": vs,
           "w": [None] * k + w[k:], "ratio": ratios, "sum_checks": checks}
    if sums is None:
        _REFERENCE[key] = out
    return out


# ---- gloo, worlds 1, 2 and 3 ------------------------------------------------------------

class _CpuNorm:
    def __init__(self, tensors):
        self.tensors = list(tensors)

    def run(self, mode, out):
        assert mode == "sq" and out.numel() == len(self.tensors) + 1
        sq = [lamb_ref.sq_sum(t.numpy()) for t in self.tensors]
        out.copy_(torch.tensor(sq + [float(np.sum(sq))], dtype=torch.float64))
        return out


class _CpuApply:
    def __init__(self, params, updates, tensors, ntensor, params16):
        self.rows = list(zip(params, updates, tensors, params16 or [None] * len(params)))
        self.ntensor = ntensor

    def run(self, nlr):
        assert nlr.numel() == self.ntensor
        for p, u, t, p16 in self.rows:
            a = p.numpy()
            a[...] = lamb_ref.apply(a.copy(), u.numpy(), float(nlr[t]),
                                    "f64" if p.dtype == torch.float64 else "f32")
            if p16 is not None:
                dt = "bf16" if p16.dtype == torch.bfloat16 else "f16"
                cpu_epilogue._np(p16).view(np.uint16)[...] = lamb_ref.narrow16(a, dt)


class CpuLambEpilogue(cpu_epilogue.CpuEpilogue):
    """cpu_epilogue.CpuEpilogue plus the LAMB passes, from lamb_ref."""

    def sq_norm_plan(self, tensors):
        return _CpuNorm(tensors)

    def lamb_moments_(self, params, grads, exp_avgs, exp_avg_sqs, updates, hypers, np_):
        for p, g, m, v, u, h in zip(params, grads, exp_avgs, exp_avg_sqs, updates, hypers):
            dt = "f64" if p.dtype == torch.float64 else "f32"
            new = lamb_ref.moments(p.numpy(), g.numpy(), m.numpy().copy(), v.numpy().copy(), dt, h,
                                   np_)
            for t, a in zip((m, v, u), new):
                t.numpy()[...] = a
        return updates

    def lamb_master_moments_(self, grads16, masters, exp_avgs, exp_avg_sqs, updates, hypers, np_):
        for g, w, m, v, u, h in zip(grads16, masters, exp_avgs, exp_avg_sqs, updates, hypers):
            dt = "bf16" if g.dtype == torch.bfloat16 else "f16"
            wide = lamb_ref.widen16(cpu_epilogue._np(g).view(np.uint16), dt)
            new = lamb_ref.moments(w.numpy(), wide, m.numpy().copy(), v.numpy().copy(), "f32", h,
                                   np_)
            for t, a in zip((m, v, u), new):
                t.numpy()[...] = a
        return updates

    def lamb_trust_update_(self, sq, world, group_of, groups, nlr, ratio, trust_clip=0.0):
        T = group_of.numel()
        gs = [groups[j] for j in group_of.tolist()]
        a, b = lamb_ref.trust(sq.numpy().reshape(world, 2 * T), [g["lr"] for g in gs],
                              [g["adapt"] for g in gs], trust_clip)
        nlr.copy_(torch.from_numpy(a))
        ratio.copy_(torch.from_numpy(b))
        return nlr

    def lamb_apply_plan(self, params, updates, tensors, ntensor, params16=None):
        return _CpuApply(params, updates, tensors, ntensor, params16)


def _state(opt, ps):
    sb = opt.state_buffers()
    assert set(sb) == {p for p in ps if p.numel()}
    return sb


def check_against_reference(ps, opt, want):
    sb = _state(opt, ps)
    ratios = opt.last_trust_ratios()
    for j, p in enumerate(ps):
        assert np.array_equal(to_numpy(p), want["p"][j]), ("param", j)
        assert ratios[p] == want["ratio"][j], ("ratio", j)
        if p.numel() == 0:
            assert ratios[p] == 1.0
            continue
        assert sb[p]["step"] == STEPS
        assert np.array_equal(sb[p]["exp_avg"].numpy().reshape(-1), want["m"][j]), ("m", j)
        assert np.array_equal(sb[p]["exp_avg_sq"].numpy().reshape(-1), want["v"][j]), ("v", j)
        if want["w"][j] is not None:
            assert np.array_equal(sb[p]["master"].numpy().reshape(-1), want["w"][j]), ("w", j)
    return sb


def body_sharded(rank, world):
    from kungfu_amd.collective import Exchange
    ps, opt = make_optimizer(Exchange(epilogue=CpuLambEpilogue()))
    for s in range(STEPS):
        set_grads(ps, world, rank, s)
        opt.step()
        schedule(opt)
    assert len(opt.state) == 0
    assert sum(len(G["pb"].buckets) for G in opt._kf_groups) >= 4
    want = reference_run(world, cuts=model_cuts(opt, world))
    sb = check_against_reference(ps, opt, want)
    k = len(NUMELS)
    assert all(want["ratio"][j] == 1.0 for j in range(k, 2 * k))     # no decay: no adapting
    assert any(want["ratio"][j] not in (1.0, TRUST_CLIP) for j in range(k))
    # state_buffers -> load_state_buffers -> continue equals the uninterrupted run
    ps2, opt2 = make_optimizer(Exchange(epilogue=CpuLambEpilogue()))
    for p, q in zip(ps, ps2):
        q.data.copy_(p.data)
    for g, g2 in zip(opt.param_groups, opt2.param_groups):
        g2["lr"] = g["lr"]
    opt2.load_state_buffers({q: sb[p] for p, q in zip(ps, ps2) if p in sb})
    for o, qs in ((opt, ps), (opt2, ps2)):
        set_grads(qs, world, rank, STEPS)
        o.step()
    sb1, sb2 = _state(opt, ps), _state(opt2, ps2)
    for p, q in zip(ps, ps2):
        assert np.array_equal(to_numpy(p), to_numpy(q))
        for key in sb1.get(p, {}):
            if key == "step":
                assert sb1[p][key] == sb2[q][key] == STEPS + 1
            else:
                assert np.array_equal(to_numpy(sb1[p][key]), to_numpy(sb2[q][key])), key


def test_sharded_lamb_world1_cpu_epilogue():
    """No process group: collective.Exchange at world 1."""
    body_sharded(0, 1)


def _entry(rank, world, store, errq):
    sys.path[:0] = [ROOT, HERE]
    try:
        dist.init_process_group("gloo", init_method="file://" + store, rank=rank,
                                world_size=world)
        import test_sharded_lamb as mod
        mod.body_sharded(rank, world)
        dist.barrier()
    except Exception:
        errq.put("rank %d: %s" % (rank, traceback.format_exc()))
        raise
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_lamb_over_gloo(world):
    ctx = mp.get_context("spawn")
    errq = ctx.SimpleQueue()
    store = os.path.join(tempfile.mkdtemp(prefix="kflamb"), "store")
    procs = [ctx.Process(target=_entry, args=(r, world, store, errq)) for r in range(world)]
    for p in procs:
        p.start()
    hung = join_all(procs, 600)
    errs = []
    while not errq.empty():
        errs.append(errq.get())
    assert not errs, "\n".join(errs)
    assert not hung and all(p.exitcode == 0 for p in procs), hung_msg(hung, [p.exitcode for p in procs])
