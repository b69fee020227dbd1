"""ShardedAdamOptimizer(stochastic_rounding=True) without a GPU: the numpy
restatement (tests/adam_sr_ref.py) on its own contract (Philox known answers,
sr on every bf16 pattern), the optimizer's construction rules, the C ABI's
argument checks (no device touched), the two stalls of the round-to-nearest
path and their absence under stochastic rounding, and the whole step over gloo
with a numpy epilogue at worlds 1, 2 and 3, ungated and gated."""
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
import adam_sr_ref as ref
import cpu_epilogue
import step_gate_ref
import test_sharded_adam_gated as gated
from oracle.oracle import bf16_bits_to_f32, f32_to_bf16_bits
from procs import hung_msg, join_all

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

OK, ERR_DTYPE, ERR_ARG = 0, 1, 3
F32, I32, F16, BF16, F64 = 0x20408, 0x10408, 0x20208, 0x20209, 0x20808

# kf_adam_sr.hip: segments per launch
SR_SEG = 32


# ---- the restatement on its own contract ---------------------------------------

def test_philox_known_answers():
    for (c0, c1, key), (a, b) in ref.PHILOX_KAT:
        ga, gb = ref.philox2x32_10(c0, c1, key)
        assert (int(ga), int(gb)) == (a, b), (hex(c0), hex(int(ga)), hex(int(gb)))
    # arrays of counters give what the scalars give
    c0 = np.array([k[0][0] for k in ref.PHILOX_KAT[:1]] * 3 + [5], np.uint64)
    ga, _ = ref.philox2x32_10(c0, 0, 0)
    assert int(ga[0]) == int(ga[2]) == 0xFF1DAE59 and int(ga[3]) != int(ga[0])


def _all_bf16():
    return np.arange(65536, dtype=np.uint32).astype(np.uint16)


def test_sr_keeps_every_bf16_value():
    """A value that is exactly a bf16 is returned unchanged for every r (the
    NaNs are made quiet, as the round-to-nearest narrowing does)."""
    bits = _all_bf16()
    x = bf16_bits_to_f32(bits)
    want = f32_to_bf16_bits(x)
    finite = (bits & 0x7FFF) < 0x7F80
    assert np.array_equal(want[finite], bits[finite])
    for r in (0, 0xFFFF):
        assert np.array_equal(ref.sr(x, np.full(65536, r)), want), r


def test_sr_between_neighbours():
    """r = 0 truncates; r = 0xffff rounds away from zero unless the low half
    is zero; a carry into the exponent is kept (the top binade reaches inf)."""
    hi = _all_bf16().astype(np.uint32)
    finite = (hi & 0x7FFF) < 0x7F80
    hi = hi[finite]
    for low in (1, 0x7FFF, 0x8000, 0xFFFF):
        x = ((hi << 16) | low).view(np.float32)
        assert np.array_equal(ref.sr(x, np.zeros(hi.size, np.uint32)), hi.astype(np.uint16)), low
        up = ref.sr(x, np.full(hi.size, 0xFFFF))
        assert np.array_equal(up, (hi + 1).astype(np.uint16)), low
        # the probability of going up is low / 2^16: r >= 2^16 - low goes up
        edge = 0x10000 - low
        assert np.array_equal(ref.sr(x, np.full(hi.size, edge)), (hi + 1).astype(np.uint16))
        assert np.array_equal(ref.sr(x, np.full(hi.size, edge - 1)), hi.astype(np.uint16))
    top = np.array([0x7F7F0001, 0xFF7F0001], np.uint32).view(np.float32)
    assert list(ref.sr(top, np.array([0xFFFF, 0xFFFF]))) == [0x7F80, 0xFF80]


def test_sr_nan_and_inf_pass_through():
    pats = np.array([0x7F800000, 0xFF800000, 0x7F800001, 0x7FC00000, 0xFFFFFFFF, 0x7F80FFFF,
                     0xFFBF0001], np.uint32)
    x = pats.view(np.float32)
    want = f32_to_bf16_bits(x)
    assert list(want[:2]) == [0x7F80, 0xFF80] and all((w & 0x7FFF) > 0x7F80 for w in want[2:])
    for r in (0, 1, 0x7FFF, 0x8000, 0xFFFF):
        assert np.array_equal(ref.sr(x, np.full(pats.size, r)), want), r


def test_random_bits_are_a_function_of_the_element_index():
    """Any split of a range gives the bits of the whole; an odd base takes the
    pair's second word."""
    rp, rv = ref.random_bits(0, 64, 7, 9)
    for base in (8, 24, 33):
        a, b = ref.random_bits(base, 16, 7, 9)
        assert np.array_equal(a, rp[base:base + 16]) and np.array_equal(b, rv[base:base + 16])
    a, b = ref.philox2x32_10(np.array([2]), 7, 9)
    assert rp[4] == int(a[0]) >> 16 and rv[5] == int(b[0]) & 0xFFFF
    hi, _ = ref.random_bits((1 << 33) - 8, 8, 7, 9)
    lo, _ = ref.random_bits((1 << 32) - 8, 8, 7, 9)
    assert not np.array_equal(hi, lo)  # bit 32 of the element index counts


def test_stream_and_key_words():
    from kungfu_amd import optimizers as kopt
    assert ref.splitmix64(0) == 0xE220A8397B1DCDAF       # SplitMix64's first output from 0
    for seed, g, b in ((0, 0, 0), (1, 2, 3), ((1 << 64) - 1, 5, 70000)):
        assert kopt.sr_stream_word(seed, g, b) == ref.stream_word(seed, g, b) < 1 << 32
        assert kopt.splitmix64(seed) == ref.splitmix64(seed)
    words = {ref.stream_word(0, g, b) for g in range(4) for b in range(4)}
    assert len(words) == 16
    assert ref.key_word((1 << 32) + 5) == 5


# ---- construction and refusals ----------------------------------------------------

def _lin(dtype=torch.bfloat16):
    torch.manual_seed(0)
    return torch.nn.Linear(5, 3).to(dtype)


class _NoGatherExchange:
    world, rank = 1, 0

    def adam_step_(self, *a):
        return None

    def adam_master_step_(self, *a):
        return None

    def reduce_shards_(self, *a):
        return 1

    def grad_shards_(self, *a):
        return []


def test_construction_rules_and_refusals():
    from kungfu_amd import optimizers as kopt
    from kungfu_amd.torch import optimizers as topt
    m = _lin()
    adam = lambda: torch.optim.Adam(m.parameters(), lr=1e-3)  # noqa: E731
    o = kopt.ShardedAdamOptimizer(adam())
    assert o._kf_sr is False
    o = topt.ShardedAdamOptimizer(adam(), m.named_parameters(), stochastic_rounding=True,
                                  sr_seed=(1 << 64) - 1)
    assert o._kf_sr is True and o._kf_sr_seed == (1 << 64) - 1 and o.state_buffers() == {}
    o = kopt.ShardedAdamOptimizer(adam(), stochastic_rounding=True, max_grad_norm=1.0)
    assert o._kf_sr and o._kf_gated
    with pytest.raises(ValueError, match="alternatives"):
        kopt.ShardedAdamOptimizer(adam(), stochastic_rounding=True, master_weights=True)
    for seed in (-1, 1 << 64, 1.0, "0", None, True):
        with pytest.raises(ValueError, match="sr_seed"):
            kopt.ShardedAdamOptimizer(adam(), stochastic_rounding=True, sr_seed=seed)
    with pytest.raises(ValueError, match="gather_params_"):
        kopt.ShardedAdamOptimizer(adam(), exchange=_NoGatherExchange(), stochastic_rounding=True)
    kopt.ShardedAdamOptimizer(adam(), exchange=_NoGatherExchange())  # not needed without the flag
    doc = kopt.ShardedAdamOptimizer.__doc__
    for words in ("stochastic_rounding=True", "sr_seed", "0x9E3779B97F4A7C15",
                  "0xBF58476D1CE4E5B9", "0x94D049BB133111EB", "identical bit for bit for any world",
                  "may round up to inf", "What is stochastic", "What is not", "sr_draw"):
        assert words in doc, words


def test_f16_stays_a_type_error():
    from kungfu_amd import optimizers as kopt
    p = torch.nn.Parameter(torch.zeros(8, dtype=torch.float16))
    o = kopt.ShardedAdamOptimizer(torch.optim.Adam([p], lr=1e-3), stochastic_rounding=True)
    p.grad = torch.zeros_like(p)
    with pytest.raises(TypeError, match="f32, bf16 and f64"):
        o.step()


# ---- C ABI argument errors (no device) ----------------------------------------------

def test_sources_pinned():
    src = open(os.path.join(ROOT, "kungfu_amd", "csrc", "kf_adam_sr.hip")).read()
    assert "constexpr int kAdamSrSeg   = %d;" % SR_SEG in src
    assert "plan_update_batch<AdamSrArgs>(" in src and '#include "kf_adam_math.hpp"' in src
    assert "adam_math<float, DIV, DECAY, H, f32x2>" in src
    assert "v_prng" not in src and "cvt_sr" not in src
    mk = open(os.path.join(ROOT, "kungfu_amd", "csrc", "Makefile")).read()
    assert " kf_adam_sr " in mk
    from kungfu_amd import _lib
    for name in ("kf_adam_sr_update_batch", "kf_adam_sr_update_batch_gated"):
        assert name in _lib.EXPORTED


def test_sr_entries_arg_errors():
    """Every check of the two entries comes before any HIP call."""
    from kungfu_amd import _lib
    lib = _lib.load()
    pa = _lib.ptr_array
    cnt = lambda *v: (ctypes.c_size_t * len(v))(*v)  # noqa: E731
    u64 = lambda *v: (ctypes.c_uint64 * len(v))(*v)  # noqa: E731
    u32 = lambda *v: (ctypes.c_uint32 * len(v))(*v)  # noqa: E731
    plain = _lib.adam_hyper_array([adam_ref.hyper(1e-3)])
    four = (pa([16]), pa([32]), pa([48]), pa([64]))

    def ungated(t, c, nb, dt=BF16, np_=0, h=plain, bases=u64(0), streams=u32(0)):
        return lib.kf_adam_sr_update_batch(*t, c, bases, streams, nb, dt, np_, h, 7, None)

    def gated_(t, c, nb, dt=BF16, np_=0, h=plain, bases=u64(0), streams=u32(0), gate=96, st=128):
        return lib.kf_adam_sr_update_batch_gated(*t, c, bases, streams, nb, dt, np_, h, 7, gate, st,
                                                 None)

    for call, name in ((ungated, b"kf_adam_sr_update_batch"),
                       (gated_, b"kf_adam_sr_update_batch_gated")):
        assert call((None,) * 4, None, 0, bases=None, streams=None) == OK
        assert call(four, cnt(0), 1) == OK
        assert call(four, cnt(8), -1) == ERR_ARG
        for i in range(4):
            t = list(four)
            t[i] = None
            assert call(t, cnt(8), 1) == ERR_ARG, i
            t[i] = pa([0])
            assert call(t, cnt(8), 1) == ERR_ARG, i
            t[i] = pa([16 * (i + 1) + 8])
            assert call(t, cnt(8), 1) == ERR_ARG, i
        assert call(four, None, 1) == ERR_ARG and call(four, cnt(8), 1, h=None) == ERR_ARG
        assert call(four, cnt(8), 1, bases=None) == ERR_ARG
        assert call(four, cnt(8), 1, streams=None) == ERR_ARG
        assert call(four, cnt(8), 1, np_=-1) == ERR_ARG
        for dt in (F32, F64, F16, I32):
            assert call(four, cnt(8), 1, dt=dt) == ERR_DTYPE, hex(dt)
        for base in (1, 4, 12, (1 << 33) + 4):
            assert call(four, cnt(8), 1, bases=u64(base)) == ERR_ARG, base
        assert call(four, cnt(16), 1, bases=u64((1 << 33) - 8)) == ERR_ARG   # past 2^33
        assert call(four, cnt(1), 1, bases=u64(1 << 33)) == ERR_ARG
        assert call(four, cnt((1 << 33) + 1), 1) == ERR_ARG
        assert call(four, cnt(0), 1, bases=u64(3)) == OK                     # an empty segment
        assert name + b":" in lib.kf_last_error()
    zero = _lib.adam_hyper_array([adam_ref.hyper(1e-3, betas=(1.0, 0.999))])
    assert ungated(four, cnt(8), 1, h=zero) == ERR_ARG
    assert gated_(four, cnt(8), 1, gate=None) == ERR_ARG
    assert gated_(four, cnt(8), 1, st=None) == ERR_ARG
    assert lib.kf_adam_sr_narrow(None, None, None, 0, None) == OK
    assert lib.kf_adam_sr_narrow(None, 16, 32, 4, None) == ERR_ARG
    assert lib.kf_adam_sr_narrow(18, 16, 32, 4, None) == ERR_ARG


# ---- the numpy epilogue -----------------------------------------------------------------

class CpuSrEpilogue(gated.CpuGatedEpilogue):
    """The CPU epilogues of the other sharded Adam tests plus the two
    stochastic-rounding updates, from adam_sr_ref."""

    def adam_sr_update_(self, params, grads, ms, vs, hypers, np_, bases, streams, key):
        for p, g, m, v, h, base, stream in zip(params, grads, ms, vs, hypers, bases, streams):
            assert p.dtype == torch.bfloat16 and base % 8 == 0
            arrs = [cpu_epilogue._np(x) for x in (p, g, m, v)]
            new = ref.step(*[np.ascontiguousarray(a) for a in arrs], h, base, stream, key, np_)
            for a, n in zip((arrs[0], arrs[2], arrs[3]), new):
                a[...] = n
        return params

    def adam_sr_update_gated_(self, params, grads, ms, vs, hyper, gate, states, group, np_, bases,
                              streams, key):
        g_, st = gated.read_gate(gate), gated.read_states(states)[group]
        for p, g, m, v, base, stream in zip(params, grads, ms, vs, bases, streams):
            arrs = [cpu_epilogue._np(x) for x in (p, g, m, v)]
            new = ref.step_gated(*[np.ascontiguousarray(a) for a in arrs], hyper, g_, st, base,
                                 stream, key, np_)
            for a, n in zip((arrs[0], arrs[2], arrs[3]), new):
                a[...] = n
        return params


def cpu_exchange():
    from kungfu_amd.collective import Exchange
    return Exchange(epilogue=CpuSrEpilogue())


def bf16_param(bits, device="cpu"):
    t = torch.from_numpy(np.ascontiguousarray(bits).view(np.int16).copy()).view(torch.bfloat16)
    return torch.nn.Parameter(t.to(device))


def bits_of(t):
    return t.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16).copy()


# ---- the flag off: the present bits -------------------------------------------------------

def test_flag_off_gives_the_present_bits_on_a_bf16_model():
    from kungfu_amd.optimizers import ShardedAdamOptimizer
    rng = np.random.default_rng(5)
    p0 = f32_to_bf16_bits(rng.standard_normal(1000).astype(np.float32))
    g0 = f32_to_bf16_bits(rng.standard_normal(1000).astype(np.float32))
    outs = []
    for kw in ({}, {"stochastic_rounding": False, "sr_seed": 99}):
        p = bf16_param(p0)
        opt = ShardedAdamOptimizer(torch.optim.Adam([p], lr=1e-2), exchange=cpu_exchange(), **kw)
        p.grad = bf16_param(g0).data
        opt.step()
        assert not any(G["sr"] for G in opt._kf_groups)
        assert "sr_draw" not in opt.state_buffers()[p]
        outs.append(bits_of(p))
    z = np.zeros(1000, np.uint16)
    want = adam_ref.step(p0, g0, z, z, "bf16", adam_ref.hyper(1e-2, step=1))[0]
    assert np.array_equal(outs[0], want) and np.array_equal(outs[1], want)


# ---- the two stalls ------------------------------------------------------------------------

STALL_N = 4096
ONE = 0x3F80  # bf16 1.0


def _stall_optimizer(sr, lr=2.0 ** -11):
    from kungfu_amd.optimizers import ShardedAdamOptimizer
    p = bf16_param(np.full(STALL_N, ONE, np.uint16))
    kw = {"stochastic_rounding": True, "sr_seed": 1} if sr else {}
    return p, ShardedAdamOptimizer(torch.optim.Adam([p], lr=lr), exchange=cpu_exchange(), **kw)


def test_small_updates_stall_under_rne_and_not_under_sr():
    """p = 1, g = 1, lr = 2^-11 (an eighth of an ulp of p below 1), 64 steps.
    Round-to-nearest leaves p exactly 1; with stochastic rounding the mean of
    4096 elements lies within 6 standard errors of f32 Adam's p. The standard
    error is the numpy reference's own: std(p_ref) / sqrt(n)."""
    steps, lr = 64, 2.0 ** -11
    ones = np.full(STALL_N, ONE, np.uint16)
    # f32 Adam, and the restatement with the optimizer's words
    pf, mf, vf = (np.ones(1, np.float32), np.zeros(1, np.float32), np.zeros(1, np.float32))
    pr, mr, vr = ones.copy(), np.zeros(STALL_N, np.uint16), np.zeros(STALL_N, np.uint16)
    stream = ref.stream_word(1, 0, 0)
    for t in range(1, steps + 1):
        h = adam_ref.hyper(lr, step=t)
        pf, mf, vf = adam_ref.step(pf, np.ones(1, np.float32), mf, vf, "f32", h)
        pr, mr, vr = ref.step(pr, ones, mr, vr, h, 0, stream, ref.key_word(t), 1)
    want = float(pf[0])
    assert abs(want - 0.96875) < 1e-5
    pr = bf16_bits_to_f32(pr).astype(np.float64)
    se = pr.std() / np.sqrt(STALL_N)
    print("reference: mean %.6f, f32 Adam %.6f, standard error %.3g" % (pr.mean(), want, se))
    assert 0 < se < 1e-3 and abs(pr.mean() - want) <= 6 * se
    p, opt = _stall_optimizer(sr=False)
    for _ in range(steps):
        p.grad = torch.ones_like(p)
        opt.step()
    assert np.array_equal(bits_of(p), ones), "round-to-nearest moved p"
    p, opt = _stall_optimizer(sr=True)
    for _ in range(steps):
        p.grad = torch.ones_like(p)
        opt.step()
    got = bf16_bits_to_f32(bits_of(p)).astype(np.float64)
    print("optimizer: mean %.6f" % got.mean())
    assert abs(got.mean() - want) <= 6 * se, (got.mean(), want, se)


def test_exp_avg_sq_never_decays_under_rne_and_does_under_sr():
    """v = 1 and 512 zero-gradient steps at beta2 = 0.999: round-to-nearest
    leaves v exactly 1; with stochastic rounding the mean of 4096 elements lies
    within 6 standard errors (the reference's own) of 0.999^512."""
    steps, lr = 512, 2.0 ** -11
    ones, zeros = np.full(STALL_N, ONE, np.uint16), np.zeros(STALL_N, np.uint16)
    want = 0.999 ** steps
    pr, mr, vr = ones.copy(), zeros.copy(), ones.copy()
    stream = ref.stream_word(1, 0, 0)
    for t in range(1, steps + 1):
        pr, mr, vr = ref.step(pr, zeros, mr, vr, adam_ref.hyper(lr, step=t), 0, stream,
                              ref.key_word(t), 1)
    vr = bf16_bits_to_f32(vr).astype(np.float64)
    se = vr.std() / np.sqrt(STALL_N)
    print("reference: mean %.6f, 0.999^512 %.6f, standard error %.3g" % (vr.mean(), want, se))
    assert 0 < se < 2e-3 and abs(vr.mean() - want) <= 6 * se
    got = {}
    for sr in (False, True):
        p, opt = _stall_optimizer(sr)
        opt.load_state_buffers({p: {"step": 0, "exp_avg": torch.zeros(STALL_N, dtype=torch.bfloat16),
                                    "exp_avg_sq": torch.ones(STALL_N, dtype=torch.bfloat16)}})
        for _ in range(steps):
            p.grad = torch.zeros_like(p)
            opt.step()
        got[sr] = bits_of(opt.state_buffers()[p]["exp_avg_sq"])
        assert np.array_equal(bits_of(p), ones)  # a zero gradient moves no parameter
    assert np.array_equal(got[False], ones), "round-to-nearest let v decay"
    mean = bf16_bits_to_f32(got[True]).astype(np.float64).mean()
    print("optimizer: mean %.6f" % mean)
    assert abs(mean - want) <= 6 * se, (mean, want, se)


# ---- the model of the gloo and GPU tests ------------------------------------------------------
#
# Group 0 is f32 (today's path), group 1 bf16 (stochastic rounding), the same
# tensor sizes in both, in buckets of 6000 bytes: three f32 buckets, two bf16
# ones. The gradients are multiples of 3/2 in [-48, 48]: their sum over 1, 2
# or 3 ranks, its average and every sum of squares are exact in any order, so
# the reference needs no knowledge of which rank holds which shard.

NUMELS = [5, 0, 1031, 7, 2050, 3]
GROUP_HYPER = ({"lr": 0.05, "weight_decay": 1e-2, "betas": (0.9, 0.999), "eps": 1e-8},
               {"lr": 0.02, "weight_decay": 1e-2, "betas": (0.8, 0.99), "eps": 1e-6})
STEPS, BAD = 4, 1
SEED = 0x123456789ABCDEF
BUCKET_BYTES = 6000
MAX_NORM = 40.0


def model_arrays(seed=3):
    rng = np.random.default_rng(seed)
    a = [rng.standard_normal(n).astype(np.float32) for n in NUMELS]
    b = [f32_to_bf16_bits(rng.standard_normal(n).astype(np.float32)) for n in NUMELS]
    return a + b


def grad_arrays(world, step, bad=False, seed=11):
    """[rank][param]; `bad`: step BAD carries one inf on the last rank, in the
    bf16 group."""
    out = []
    k = len(NUMELS)
    for r in range(world):
        rng = np.random.default_rng(seed + 100 * step + r)
        gs = [(rng.integers(-32, 33, n) * 1.5).astype(np.float32) for n in NUMELS * 2]
        if bad and step == BAD and r == world - 1:
            gs[k + 4][17] = np.inf
        out.append(gs[:k] + [f32_to_bf16_bits(g) for g in gs[k:]])
    return out


def to_torch(a):
    if a.dtype == np.uint16:
        return torch.from_numpy(a.view(np.int16).copy()).view(torch.bfloat16)
    return torch.from_numpy(a.copy())


def to_numpy(t):
    t = t.detach().cpu().contiguous()
    return bits_of(t) if t.element_size() == 2 else t.numpy().copy()


def make_optimizer(exchange, device="cpu", gate=False, arrays=None):
    from kungfu_amd.optimizers import ShardedAdamOptimizer
    arrays = model_arrays() if arrays is None else arrays
    ps = [torch.nn.Parameter(to_torch(a).to(device)) for a in arrays]
    k = len(NUMELS)
    groups = [dict(GROUP_HYPER[0], params=ps[:k]), dict(GROUP_HYPER[1], params=ps[k:])]
    kw = {"max_grad_norm": MAX_NORM} if gate else {}
    opt = ShardedAdamOptimizer(torch.optim.AdamW(groups, lr=0.1), exchange=exchange,
                               bucket_bytes=BUCKET_BYTES, stochastic_rounding=True, sr_seed=SEED,
                               **kw)
    return ps, opt


def run_steps(ps, opt, world, rank, device="cpu", first=0, steps=STEPS, bad=False):
    for s in range(first, first + steps):
        for p, g in zip(ps, grad_arrays(world, s, bad)[rank]):
            p.grad = to_torch(g).to(device)
        opt.step()
        for g in opt.param_groups:
            g["lr"] = g["lr"] * 0.5


def bucket_layout():
    """[[tensor indices of bucket b]] of the bf16 group: GradBuckets' greedy
    grouping, which does not depend on the world."""
    from kungfu_amd.collective import GradBuckets
    return GradBuckets._groups_greedy(NUMELS, BUCKET_BYTES // 2)


_REFERENCE = {}


def reference_run(world, steps=STEPS, gate=False):
    """The model after `steps` steps: adam_ref (f32 group) and adam_sr_ref on
    the unsharded bf16 buckets with base 0, on oracle.reduce_avg of the ranks'
    gradients, the lr halved after every step; with `gate`, step_gate_ref's
    verdict under MAX_NORM, step BAD skipped. Computed once per case and
    shared; callers leave it unchanged."""
    key = (world, steps, gate)
    if key in _REFERENCE:
        return _REFERENCE[key]
    from oracle import oracle
    k = len(NUMELS)
    arrs = model_arrays()
    p = [a.copy() for a in arrs]
    m = [np.zeros(a.size, a.dtype) for a in arrs]
    v = [np.zeros(a.size, a.dtype) for a in arrs]
    layout = bucket_layout()
    assert len(layout) == 2
    g_, states = step_gate_ref.new_gate(), [step_gate_ref.new_state(betas=h["betas"])
                                            for h in GROUP_HYPER]
    lr_scale, applied = 1.0, 0
    for s in range(steps):
        gr = grad_arrays(world, s, gate)
        avg = [oracle.reduce_avg([np.ascontiguousarray(gr[r][j]) for r in range(world)],
                                 "f32" if j < k else "bf16", world) for j in range(2 * k)]
        avg = [np.asarray(a).view(np.uint16) if j >= k else np.asarray(a, np.float32)
               for j, a in enumerate(avg)]
        hs = [dict(h, decoupled=True, lr=h["lr"] * lr_scale, step=applied + 1) for h in GROUP_HYPER]
        if gate:
            # one plan per dtype; the f32 shards hold the sum until the update
            # divides it (a reduce-scatter), the bf16 ones the average (the fold)
            sums = [np.sum([gr[r][j] for r in range(world)], axis=0, dtype=np.float32)
                    for j in range(k)]
            sq = [[step_gate_ref.sum_sq(sums), step_gate_ref.sum_sq(avg[k:], "bf16")]]
            nps = [world, 0] if world > 1 else [1, 1]
            step_gate_ref.gate_update(sq, nps, hs, states, g_, max_norm=MAX_NORM)
        draw = ref.key_word(s + 1)
        if gate:
            for j in range(k):
                p[j], m[j], v[j] = step_gate_ref.update(p[j], sums[j], m[j], v[j], "f32", hs[0], g_,
                                                        states[0], world)
        else:
            for j in range(k):
                p[j], m[j], v[j] = adam_ref.step(p[j], avg[j], m[j], v[j], "f32", hs[0])
        for b, idx in enumerate(layout):
            cat = [np.concatenate([x[k + t] for t in idx]) for x in (p, avg, m, v)]
            stream = ref.stream_word(SEED, 1, b)
            if gate:
                new = ref.step_gated(*cat, hs[1], g_, states[1], 0, stream, draw)
            else:
                new = ref.step(*cat, hs[1], 0, stream, draw)
            off = 0
            for t in idx:
                n = NUMELS[t]
                p[k + t], m[k + t], v[k + t] = (x[off:off + n].copy() for x in new)
                off += n
        if not (gate and g_["skip"]):
            applied += 1
        lr_scale *= 0.5
    _REFERENCE[key] = {"p": p, "m": m, "v": v, "applied": applied, "draw": steps, "gate": dict(g_)}
    return _REFERENCE[key]


def check_against_reference(ps, opt, want):
    sb = opt.state_buffers()
    assert set(sb) == {p for p in ps if p.numel()}
    k = len(NUMELS)
    for j, p in enumerate(ps):
        assert np.array_equal(to_numpy(p), want["p"][j]), ("param", j)
        if p.numel() == 0:
            continue
        assert sb[p]["step"] == want["applied"]
        assert ("sr_draw" in sb[p]) == (j >= k)
        if j >= k:
            assert sb[p]["sr_draw"] == want["draw"]
        assert np.array_equal(to_numpy(sb[p]["exp_avg"]).reshape(-1), want["m"][j]), ("m", j)
        assert np.array_equal(to_numpy(sb[p]["exp_avg_sq"]).reshape(-1), want["v"][j]), ("v", j)
    return sb


def body_sharded(rank, world, make_exchange=cpu_exchange, device="cpu", gate=False):
    """What the CPU and the GPU end-to-end tests share: the run against the
    reference on the unsharded buckets (the same reference bits whatever the
    world holds of them), and state_buffers -> load_state_buffers -> continue
    against the uninterrupted run. With `gate`, step BAD is skipped on the
    device and still advances the draw."""
    ps, opt = make_optimizer(make_exchange(), device, gate)
    if gate:
        run_steps(ps, opt, world, rank, device, steps=BAD, bad=True)
        before = [to_numpy(p) for p in ps], opt.state_buffers()
        run_steps(ps, opt, world, rank, device, first=BAD, steps=1, bad=True)
        after = [to_numpy(p) for p in ps], opt.state_buffers()
        assert opt.skipped_steps() == 1 and opt.applied_steps() == BAD
        for j, p in enumerate(ps):
            assert before[0][j].tobytes() == after[0][j].tobytes(), ("param moved on a skip", j)
            for key in ("exp_avg", "exp_avg_sq") if p.numel() else ():
                assert to_numpy(before[1][p][key]).tobytes() == to_numpy(after[1][p][key]).tobytes()
            if p.numel():
                assert before[1][p]["step"] == after[1][p]["step"] == BAD
        k = len(NUMELS)
        assert before[1][ps[k]]["sr_draw"] == BAD and after[1][ps[k]]["sr_draw"] == BAD + 1
        run_steps(ps, opt, world, rank, device, first=BAD + 1, steps=STEPS - BAD - 1, bad=True)
    else:
        run_steps(ps, opt, world, rank, device)
    assert len(opt.state) == 0
    assert [len(G["pb"].buckets) for G in opt._kf_groups] == [3, 2]
    assert [G["sr"] for G in opt._kf_groups] == [False, True]
    want = reference_run(world, gate=gate)
    assert want["applied"] == (STEPS - 1 if gate else STEPS)
    sb = check_against_reference(ps, opt, want)
    # the world-invariance claim: the reference of any world with the same
    # averaged gradients is the same computation; worlds 1 and 2 average
    # these gradients exactly, so their references are not the same numbers,
    # but each is matched bit for bit on the shards of its world
    # state_buffers -> load_state_buffers -> continue equals the uninterrupted run
    ps2, opt2 = make_optimizer(make_exchange(), device, gate, arrays=[to_numpy(p) for p in ps])
    for g, g2 in zip(opt.param_groups, opt2.param_groups):
        g2["lr"] = g["lr"]
    opt2.load_state_buffers({q: sb[p] for p, q in zip(ps, ps2) if p in sb})
    for o, qs in ((opt, ps), (opt2, ps2)):
        run_steps(qs, o, world, rank, device, first=STEPS, steps=1, bad=gate)
    check_against_reference(ps, opt, reference_run(world, STEPS + 1, gate))
    sb1, sb2 = opt.state_buffers(), opt2.state_buffers()
    for p, q in zip(ps, ps2):
        assert np.array_equal(to_numpy(p), to_numpy(q))
        for key in sb1.get(p, {}):
            if key in ("step", "sr_draw"):
                assert sb1[p][key] == sb2[q][key]
            else:
                assert np.array_equal(to_numpy(sb1[p][key]), to_numpy(sb2[q][key])), key


def test_load_without_sr_draw_takes_the_step():
    ps, opt = make_optimizer(cpu_exchange())
    run_steps(ps, opt, 1, 0, steps=2)
    sb = opt.state_buffers()
    ps2, opt2 = make_optimizer(cpu_exchange(), arrays=[to_numpy(p) for p in ps])
    opt2.load_state_buffers({q: {k: x for k, x in sb[p].items() if k != "sr_draw"}
                             for p, q in zip(ps, ps2) if p in sb})
    assert [G["draw"] for G in opt2._kf_groups] == [0, 2]
    k = len(NUMELS)
    bad = {q: dict(sb[p]) for p, q in zip(ps, ps2) if p in sb}
    bad[ps2[k]]["sr_draw"] = 7
    with pytest.raises(ValueError, match="sr_draw"):
        opt2.load_state_buffers(bad)


def test_same_averaged_gradients_same_bits_in_every_world():
    """The references of worlds 1, 2 and 3 on gradients whose average is the
    same in every world agree bit for bit: nothing in the reference (and so in
    what each world is matched against) depends on the world. Rank r's
    gradient is the average itself."""
    layout = bucket_layout()
    rng = np.random.default_rng(2)
    n = sum(NUMELS[t] for t in layout[0])
    p = f32_to_bf16_bits(rng.standard_normal(n).astype(np.float32))
    g = f32_to_bf16_bits(rng.standard_normal(n).astype(np.float32))
    z = np.zeros(n, np.uint16)
    h = adam_ref.hyper(1e-2, step=1)
    whole = ref.step(p, g, z, z, h, 0, 5, 1)
    for world in (2, 3):
        q = -(-n // (8 * world)) * 8  # a shard of the padded bucket
        parts = [ref.step(p[r * q:(r + 1) * q], g[r * q:(r + 1) * q], z[r * q:(r + 1) * q],
                          z[r * q:(r + 1) * q], h, r * q, 5, 1) for r in range(world)]
        for i in range(3):
            assert np.array_equal(np.concatenate([x[i] for x in parts]), whole[i]), (world, i)


def test_world1_cpu_epilogue():
    """No process group: collective.Exchange at world 1."""
    body_sharded(0, 1)


def test_world1_cpu_epilogue_gated():
    body_sharded(0, 1, gate=True)


def _entry(rank, world, store, errq):
    sys.path[:0] = [ROOT, HERE]
    try:
        dist.init_process_group("gloo", init_method="file://" + store, rank=rank,
                                world_size=world)
        import test_sharded_adam_sr as mod
        mod.body_sharded(rank, world)
        mod.body_sharded(rank, world, gate=True)
        dist.barrier()
    except Exception:
        errq.put("rank %d: %s" % (rank, traceback.format_exc()))
        raise
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_adam_sr_over_gloo(world):
    ctx = mp.get_context("spawn")
    errq = ctx.SimpleQueue()
    store = os.path.join(tempfile.mkdtemp(prefix="kfadamsr"), "store")
    procs = [ctx.Process(target=_entry, args=(r, world, store, errq)) for r in range(world)]
    for p in procs:
        p.start()
    hung = join_all(procs, 600)
    errs = []
    while not errq.empty():
        errs.append(errq.get())
    assert not errs, "\n".join(errs)
    assert not hung and all(p.exitcode == 0 for p in procs), hung_msg(hung, [p.exitcode for p in procs])
