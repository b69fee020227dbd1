"""The gated sharded Adam / AdamW step (max_grad_norm, loss_scale; DESIGN.md
§16) without a GPU: the numpy restatement (tests/step_gate_ref.py) pinned to
adam_ref, measured against torch's clip_grad_norm_ + Adam / AdamW and against
torch.amp.GradScaler, the construction rules, the source pins and exports of
the new kernels and entries, their argument checks (no device touched), and
ShardedAdamOptimizer(max_grad_norm, loss_scale) end to end over a CPU epilogue
at world 1 and over gloo."""
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

import adam_master_ref
import adam_ref
import cpu_epilogue
import step_gate_ref as ref
import test_sharded_adam as base
import test_sharded_adam_master as master
from procs import hung_msg, join_all

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
ROWS = base.ROWS

# The largest |torch - step_gate_ref| measured for (p, m, v) on the data of
# test_gated_restatement_against_torch, per row: DESIGN.md §16's table
# (2^-22 = 2.38e-7, 2^-23 = 1.19e-7, 1.25 * 2^-31 = 5.82e-10, 2^-29 = 1.86e-9,
# 1.125 * 2^-43 = 1.28e-13, 2^-40 = 9.09e-13). p is one or two units in the
# last place of the largest elements, as in §14; m and v are far below §14's
# because two of the four gradients are clipped to norm 1 and two are smaller
# still. The test's bounds are four times these.
MEASURED = {(0.0, False): (2.0 ** -22, 1.25 * 2.0 ** -31, 1.125 * 2.0 ** -43),
            (1e-2, False): (2.0 ** -23, 2.0 ** -29, 2.0 ** -40),
            (1e-2, True): (2.0 ** -22, 1.25 * 2.0 ** -31, 1.125 * 2.0 ** -43)}


# ---- the restatement ---------------------------------------------------------

def _random(dt, n, seed, square=False):
    """Standard-normal values (squared for an exp_avg_sq) in dt's numpy form."""
    x = np.random.default_rng(seed).standard_normal(n)
    x = x * x if square else x
    return adam_ref.f32_to_bf16_bits(x.astype(np.float32)) if dt == "bf16" else \
        x.astype(adam_ref.STORAGE[dt])


def _no_gate():
    g = ref.new_gate()
    g["grad_mul"] = np.float32(1.0)
    return g


@pytest.mark.parametrize("dt", ["f32", "bf16", "f64"])
def test_rest_is_adam_ref(dt):
    """step_gate_ref.update with grad_mul = 1 and adam_ref's own scalars is
    adam_ref.step, bit for bit: what `update` restates of it is restated
    right. (x * 1 is x, and rounding a value of the type to the type is the
    identity.)"""
    n = 4099
    seg = (_random(dt, n, 1), _random(dt, n, 2), _random(dt, n, 3), _random(dt, n, 4, square=True))
    for wd, decoupled in ROWS:
        for np_, step in ((0, 1), (3, 7), (4, 2)):
            h = adam_ref.hyper(1e-2, weight_decay=wd, decoupled=decoupled, step=step)
            want = adam_ref.step(*seg, dt, h, np_)
            got = ref.update(*seg, dt, h, _no_gate(), ref.scalars_of(h), np_)
            for a, b in zip(got, want):
                assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), (dt, wd, decoupled, np_)


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_rest_is_adam_master_ref(dt):
    n = 4099
    g16 = adam_master_ref.narrow(np.random.default_rng(5).standard_normal(n), dt)
    w, m, v = _random("f32", n, 1), _random("f32", n, 3), _random("f32", n, 4, square=True)
    for wd, decoupled in ROWS:
        h = adam_ref.hyper(1e-2, weight_decay=wd, decoupled=decoupled, step=3)
        want = adam_master_ref.step(w, g16, m, v, dt, h, 3)
        got = ref.update_master(w, g16, m, v, dt, h, _no_gate(), ref.scalars_of(h), 3)
        for a, b in zip(got, want):
            assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), (dt, wd, decoupled)


def test_skip_returns_the_inputs():
    g = _no_gate()
    g["skip"] = 1
    a = [np.arange(5, dtype=np.float32) + i for i in range(4)]
    p, m, v = ref.update(*a, "f32", adam_ref.hyper(1e-2), g, ref.new_state())
    assert np.array_equal(p, a[0]) and np.array_equal(m, a[2]) and np.array_equal(v, a[3])
    p16, w, m, v = ref.update_master(a[0], a[1].astype(np.float16), a[2], a[3], "f16",
                                     adam_ref.hyper(1e-2), g, ref.new_state())
    assert p16 is None and np.array_equal(w, a[0])


def test_running_products_are_the_contract():
    """The bias corrections are running products in double. After t applied
    steps they may differ from beta ** t in the last places; a skip does not
    advance them."""
    g, st = ref.new_gate(), [ref.new_state()]
    h = [{"lr": 1e-3, "betas": (0.9, 0.999)}]
    prod1 = prod2 = 1.0
    for t in range(1, 200):
        sq = [[np.inf if t % 7 == 0 else 1.0]]
        ref.gate_update(sq, [0], h, st, g)
        if t % 7:
            prod1, prod2 = prod1 * 0.9, prod2 * 0.999
        assert st[0]["beta1_pow"] == prod1 and st[0]["beta2_pow"] == prod2
    assert st[0]["step"] == 199 - 199 // 7 == g["applied"] and g["skipped"] == 199 // 7
    assert abs(st[0]["beta2_pow"] - 0.999 ** st[0]["step"]) <= 1e-13
    # resumed: seeded with Python's pow
    assert ref.new_state(5, (0.9, 0.999))["beta1_pow"] == 0.9 ** 5


# ---- against torch ------------------------------------------------------------

@pytest.mark.parametrize("wd,decoupled", ROWS)
def test_gated_restatement_against_torch(wd, decoupled):
    """step_gate_ref (verdict, then gated update) against torch on CPU:
    clip_grad_norm_(max_norm = 1) followed by torch.optim.Adam / AdamW
    (foreach=False), on DESIGN.md §14's inputs (100003 standard-normal
    elements, 4 steps, lr changed every step). The gradients are scaled by
    (0.001, 1, 0.002, 3): their norms are about 0.32, 316, 0.63 and 949, so
    the clip is active on steps 2 and 4 and idle on 1 and 3. A fifth gradient,
    in second place, carries one inf: both sides skip it (torch as GradScaler
    does: no optimizer step), and the steps after it use the step counts of
    an uninterrupted run. Not bit-exact, for §14's reasons and because torch
    computes the norm and the clip factor in fp32. The largest absolute
    differences measured for (p, m, v): 2.38e-7, 5.82e-10, 1.28e-13 with no
    decay; 1.19e-7, 1.86e-9, 9.09e-13 with Adam's L2 decay; 2.38e-7, 5.82e-10,
    1.28e-13 with AdamW's (MEASURED). Each bound is four times the measured
    value."""
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
    tp = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    cls = torch.optim.AdamW if decoupled else torch.optim.Adam
    opt = cls([tp], lr=lrs[0], weight_decay=wd, foreach=False)
    p, m, v = p0.copy(), np.zeros(n, np.float32), np.zeros(n, np.float32)
    gate, st = ref.new_gate(), [ref.new_state()]
    clipped = []
    for lr, g in zip(lrs, grads):
        opt.param_groups[0]["lr"] = lr
        tp.grad = torch.from_numpy(g.copy())
        norm = torch.nn.utils.clip_grad_norm_([tp], 1.0, foreach=False)
        if bool(torch.isfinite(norm)):
            opt.step()
        h = {"lr": lr, "betas": (0.9, 0.999), "eps": 1e-8, "weight_decay": wd,
             "decoupled": decoupled}
        ref.gate_update([[ref.sum_sq([g])]], [0], [h], st, gate, max_norm=1.0)
        assert gate["skip"] == int(not bool(torch.isfinite(norm)))
        if not gate["skip"]:
            assert abs(gate["grad_norm"] - float(norm)) <= 1e-5 * float(norm)
            clipped.append(float(gate["grad_mul"]) < 1.0)
        p, m, v = ref.update(p, g, m, v, "f32", h, gate, st[0])
    assert clipped == [False, True, False, True] and gate["skipped"] == 1 and st[0]["step"] == 4
    ts = opt.state[tp]
    assert int(ts["step"]) == 4
    diffs = [float(np.max(np.abs(a - b))) for a, b in
             ((tp.detach().numpy(), p), (ts["exp_avg"].numpy(), m), (ts["exp_avg_sq"].numpy(), v))]
    print("max |torch - step_gate_ref| after 4 applied steps (p, m, v): %.3g %.3g %.3g"
          % tuple(diffs))
    for d, measured, what in zip(diffs, MEASURED[(wd, decoupled)], "pmv"):
        assert d <= 4 * measured, (what, d, measured)


def test_loss_scale_sequence_is_grad_scalers():
    """A skip, growth_interval good steps (the last one grows the scale), two
    skips in a row, one more good step: the loss scale equals
    torch.amp.GradScaler's _scale, and the growth tracker its _growth_tracker,
    after every step."""
    interval = 3
    found = [1] + [0] * interval + [1, 1, 0]
    scaler = torch.amp.GradScaler("cpu", init_scale=65536.0, growth_factor=2.0, backoff_factor=0.5,
                                  growth_interval=interval)
    tp = torch.nn.Parameter(torch.ones(3))
    opt = torch.optim.SGD([tp], lr=0.1)
    gate, st = ref.new_gate(65536.0), [ref.new_state()]
    seen = []
    for bad in found:
        scaler.scale(torch.tensor(1.0))
        tp.grad = torch.full((3,), float("inf") if bad else 1.0)
        scaler.step(opt)
        scaler.update()
        ref.gate_update([[np.inf if bad else 3.0]], [0], [{"lr": 0.1}], st, gate,
                        growth_factor=2.0, backoff_factor=0.5, growth_interval=interval)
        assert gate["skip"] == bad
        assert gate["loss_scale"].dtype == np.float32
        assert float(gate["loss_scale"]) == float(scaler._scale), (seen, bad)
        assert gate["good_steps"] == int(scaler._growth_tracker)
        seen.append(float(gate["loss_scale"]))
    assert seen == [32768.0] * interval + [65536.0, 32768.0, 16384.0, 16384.0]
    # growth_interval 0 never grows; a static scale (backoff 1) never moves
    gate = ref.new_gate(8.0)
    for bad in (0, 0, 1, 0):
        ref.gate_update([[np.inf if bad else 1.0]], [0], [], [], gate)
    assert float(gate["loss_scale"]) == 8.0 and gate["skipped"] == 1 and gate["applied"] == 3
    # the scale does not grow to inf (GradScaler keeps the finite one)
    gate = ref.new_gate(2.0 ** 127)
    ref.gate_update([[1.0]], [0], [], [], gate, growth_factor=2.0, growth_interval=1)
    assert float(gate["loss_scale"]) == 2.0 ** 127 and gate["good_steps"] == 0


# ---- construction ---------------------------------------------------------------

class _NoGatedExchange:
    world, rank = 1, 0

    def all_reduce_(self, buckets, **kw):
        return buckets

    def adam_step_(self, *a):
        return None

    def adam_master_step_(self, *a):
        return None


def test_construction_rules():
    from kungfu_amd import optimizers as kopt
    from kungfu_amd.torch import optimizers as topt
    lin = torch.nn.Linear(5, 3)
    new = lambda **kw: kopt.ShardedAdamOptimizer(  # noqa: E731
        torch.optim.AdamW(lin.parameters(), lr=1e-3), **kw)
    for bad in (0, -1.0, float("inf"), float("nan"), "1.0", True):
        with pytest.raises(ValueError, match="max_grad_norm"):
            new(max_grad_norm=bad)
    for bad in (0, -2.0, float("inf"), float("nan"), "static", True, {"scale": 2.0},
                {"init_scale": 0}, {"growth_interval": -1}, {"growth_interval": 2.5},
                {"backoff_factor": "half"}):
        with pytest.raises(ValueError, match="loss_scale"):
            new(loss_scale=bad)
    # an exchange without the gated methods: refused at construction, only when gated
    for kw in ({"max_grad_norm": 1.0}, {"loss_scale": "dynamic"}):
        with pytest.raises(ValueError, match="reduce_shards_"):
            new(exchange=_NoGatedExchange(), **kw)
    o = new(exchange=_NoGatedExchange())
    assert not o._kf_gated
    for call in (o.loss_scale_value, o.skipped_steps, o.scaler_state,
                 lambda: o.scale_loss(torch.ones(()))):
        with pytest.raises(ValueError, match="max_grad_norm or loss_scale"):
            call()
    # the rules of the three forms
    assert new(max_grad_norm=2)._kf_rule == {"init_scale": 1.0, "growth_factor": 1.0,
                                             "backoff_factor": 1.0, "growth_interval": 0}
    assert new(loss_scale=128)._kf_rule["init_scale"] == 128.0
    assert new(loss_scale=128)._kf_rule["growth_interval"] == 0
    assert new(loss_scale="dynamic")._kf_rule == {"init_scale": 65536.0, "growth_factor": 2.0,
                                                  "backoff_factor": 0.5, "growth_interval": 2000}
    assert new(loss_scale={"growth_interval": 7})._kf_rule["growth_interval"] == 7
    assert new(loss_scale="dynamic")._kf_max_norm == 0.0 and new(max_grad_norm=0.5)._kf_max_norm == 0.5
    # f16 without master weights stays a TypeError, gated or not
    p = torch.nn.Parameter(torch.zeros(8, dtype=torch.float16))
    o = kopt.ShardedAdamOptimizer(torch.optim.Adam([p], lr=1e-3), max_grad_norm=1.0,
                                  loss_scale="dynamic", exchange=_gated_exchange())
    p.grad = torch.zeros_like(p)
    with pytest.raises(TypeError, match="f32, bf16 and f64"):
        o.step()
    # through the torch-style constructor's **kwargs
    q = torch.nn.Parameter(torch.ones(8, dtype=torch.float16))
    o = topt.ShardedAdamOptimizer(torch.optim.AdamW([q], lr=1e-3), [("q", q)], master_weights=True,
                                  exchange=_gated_exchange(), max_grad_norm=1.0, loss_scale=4.0)
    assert o._kf_gated and o.loss_scale_value() == 4.0
    assert float(o.scale_loss(torch.tensor(1.5))) == 6.0
    for words in ("max_grad_norm", "loss_scale"):
        assert words in topt.ShardedAdamOptimizer.__doc__
    doc = kopt.ShardedAdamOptimizer.__doc__
    for words in ("max_grad_norm", "loss_scale", "scale_loss", "clip_grad_norm_", "GradScaler",
                  "Clipping without a loss scale skips such steps too", "running products",
                  "skipped_steps()", "load_scaler_state()"):
        assert words in doc, words


# ---- source pins and exports ---------------------------------------------------

def _src(name):
    return open(os.path.join(ROOT, "kungfu_amd", "csrc", name)).read()


def test_sources_pinned():
    adam, mst, math_, gate = (_src(n) for n in ("kf_adam.hip", "kf_adam_master.hip",
                                                 "kf_adam_math.hpp", "kf_step_gate.hip"))
    # new kernels beside the parents, through the parents' bodies and planner
    assert "adam_update_gated_kernel(AdamBatchArgs<typename SgdElt<T>::C> a, Div np, int div," in adam
    assert "adam_master_gated_kernel(AdamMasterArgs a, Div np, int div," in mst
    assert "adam_update_kernel(AdamBatchArgs<typename SgdElt<T>::C> a, Div np, int div)" in adam
    assert "adam_master_kernel(AdamMasterArgs a, Div np, int div)" in mst
    for src in (adam, mst):
        assert src.count("__builtin_amdgcn_sched_barrier(0);") == 1  # one tile loop, shared
        assert "if (adam_gate_load(gate, st, gt)) return;" in src
        assert "asm" not in src
    # the one inserted operation, directly after the /np
    assert re.search(r"g\[i\] = SgdDiv<T, DIV>::run\(g\[i\], d\);\s*if constexpr \(GATE::on\) \{\s*"
                     r"#pragma unroll\s*for \(int i = 0; i < H; \+\+i\) g\[i\] = E::rnd\(g\[i\] \* gate\.mul\);",
                     math_)
    assert "const int skip = gate->skip;" in math_ and "return skip != 0;" in math_
    # the verdict: one lane, correctly rounded fp64, no pow, no atomics
    assert "if (threadIdx.x != 0 || blockIdx.x != 0) return;" in gate
    for word in ("__dsqrt_rn", "__ddiv_rn", "__dadd_rn", "__dmul_rn", "__fmul_rn"):
        assert word in gate, word
    code = re.sub(r"//.*", "", gate)  # the header comment says what is absent
    for word in ("pow(", "atomic", "asm"):
        assert word not in code, word
    names = open(os.path.join(ROOT, "kungfu_amd", "csrc", "Makefile")).read()
    assert re.search(r"^NAMES\s*:=.*\bkf_step_gate\b", names, re.M)


NEW_ENTRIES = ("kf_step_gate_update", "kf_adam_update_batch_gated",
               "kf_adam_master_update_batch_gated", "kf_exchange_reduce_shards_batch",
               "kf_exchange_adam_gated_batch", "kf_exchange_all_gather_doubles")


def test_entries_declared_and_exported():
    from kungfu_amd import _lib, ops
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "kungfu_amd.h")).read()
    for name in NEW_ENTRIES:
        assert re.search(r"^int %s\(" % name, hdr, re.M), name
        assert name in _lib.EXPORTED and getattr(lib, name) is not None
    for name in ("step_gate_update_", "adam_update_batch_gated_", "adam_master_update_batch_gated_"):
        assert callable(getattr(ops, name))
    # the two device structs as the header declares them, field for field
    for struct, cname in ((_lib.StepGate, "kf_step_gate"), (_lib.StepState, "kf_step_state")):
        body = re.search(r"typedef struct \{([^}]*)\} %s;" % cname, hdr).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = re.findall(r"(\w+)\s+(\w+);", body)
        ctype = {"int32_t": ctypes.c_int32, "float": ctypes.c_float, "double": ctypes.c_double,
                 "uint64_t": ctypes.c_uint64, "int64_t": ctypes.c_int64}
        assert [(n, ctype[t]) for t, n in fields] == list(struct._fields_), cname
    assert ctypes.sizeof(_lib.StepGate) == 48 and ctypes.sizeof(_lib.StepState) == 48
    assert _lib.StepGate.loss_scale.offset == 8  # ShardedAdamOptimizer.scale_loss reads it there
    assert tuple(n for n, _ in _lib.StepGate._fields_) == ref.GATE_FIELDS
    assert tuple(n for n, _ in _lib.StepState._fields_) == ref.STATE_FIELDS


OK, ERR_DTYPE, ERR_ARG = base.OK, base.ERR_DTYPE, base.ERR_ARG
F32, F16, BF16, F64 = base.F32, base.F16, base.BF16, base.F64


def test_gated_entries_arg_errors():
    """Every check of the new entries comes before any HIP call."""
    from kungfu_amd import _lib
    lib = _lib.load()
    pa = _lib.ptr_array
    cnt = lambda *v: (ctypes.c_size_t * len(v))(*v)  # noqa: E731
    h = _lib.adam_hyper_array([adam_ref.hyper(1e-3)])
    h[0].bias_correction1 = h[0].bias_correction2 = float("nan")  # ignored by the gated entries
    four, five = (pa([16]), pa([32]), pa([48]), pa([64])), (pa([16]), pa([32]), pa([48]), pa([64]), pa([80]))
    plain = lambda *a, dt=F32, np_=0, hyper=h, gate=96, st=128: \
        lib.kf_adam_update_batch_gated(*a, dt, np_, hyper, gate, st, None)  # noqa: E731
    mst = lambda *a, dt=BF16, np_=0, hyper=h, gate=96, st=128: \
        lib.kf_adam_master_update_batch_gated(*a, dt, np_, hyper, gate, st, None)  # noqa: E731
    for call, tabs in ((plain, four), (mst, five)):
        nulls = (None,) * len(tabs)
        assert call(*nulls, None, 0) == OK                              # nb == 0
        assert call(*tabs, cnt(0), 1) == OK                             # an empty segment
        assert call(*tabs, cnt(4), -1) == ERR_ARG
        assert call(*tabs, cnt(4), 1, gate=None) == ERR_ARG
        assert call(*tabs, cnt(4), 1, st=None) == ERR_ARG
        assert b"gate" in lib.kf_last_error()
        assert call(*tabs, cnt(4), 1, hyper=None) == ERR_ARG
        assert call(*tabs, cnt(4), 1, np_=-1) == ERR_ARG
        for i in range(len(tabs)):
            t = list(tabs)
            t[i] = pa([16 * (i + 1) + 8])
            assert call(*t, cnt(4), 1) == ERR_ARG, i
            assert b"16-byte" in lib.kf_last_error() and b"_gated" in lib.kf_last_error()
    assert plain(*four, cnt(4), 1, dt=F16) == ERR_DTYPE
    assert mst(*five, cnt(4), 1, dt=F32) == ERR_DTYPE
    # the verdict
    G = _lib.StepGroup * 1
    gate = lambda sq=8, world=1, nplan=1, nps=(ctypes.c_int * 1)(0), groups=G(), states=64, ng=1, \
        growth=2.0, backoff=0.5, interval=2, g=96: lib.kf_step_gate_update(  # noqa: E731
            sq, world, nplan, nps, groups, states, ng, 1.0, growth, backoff, interval, g, None)
    for kw in ({"sq": None}, {"nps": None}, {"g": None}, {"world": 0}, {"nplan": 0}, {"ng": -1},
               {"groups": None}, {"states": None}, {"interval": -1}, {"growth": 0.0},
               {"backoff": float("nan")}, {"nps": (ctypes.c_int * 1)(-1)}):
        assert gate(**kw) == ERR_ARG, kw
        assert b"kf_step_gate_update" in lib.kf_last_error()
    # the exchange's halves need an exchange
    np_ = ctypes.c_int(0)
    assert lib.kf_exchange_reduce_shards_batch(None, pa([16]), cnt(8), 1, F32, 0,
                                               ctypes.byref(np_), None) == ERR_ARG
    assert lib.kf_exchange_adam_gated_batch(None, pa([16]), pa([32]), None, pa([48]), pa([64]),
                                            cnt(8), 1, F32, 0, h, 96, 128, None) == ERR_ARG
    assert b"kf_exchange_adam_gated_batch" in lib.kf_exchange_last_error()
    assert lib.kf_exchange_all_gather_doubles(None, 8, 16, 1, None) == ERR_ARG


# ---- the optimizer: a two-layer f16 model, an overflow step --------------------

class CpuGatedEpilogue(master.CpuAdamMasterEpilogue):
    """master.CpuAdamMasterEpilogue plus the gated step's device work, from
    step_gate_ref: the gate and the step states are the same bytes as on the
    device, in CPU tensors."""

    class _Plan:
        def __init__(self, tensors):
            self.tensors = list(tensors)

        def run(self, mode, out):
            assert mode == "sq" and out.numel() == len(self.tensors) + 1
            sq = [ref.sum_sq([cpu_epilogue._np(t)], cpu_epilogue._DT[t.dtype]) for t in self.tensors]
            tot = 0.0
            for s in sq:
                tot += s
            out.copy_(torch.tensor(sq + [tot], dtype=torch.float64))
            return out

    def sq_norm_plan(self, tensors):
        return self._Plan(tensors)

    def step_gate_update_(self, sq, world, nps, groups, states, gate, **rule):
        g, sts = read_gate(gate), read_states(states)
        ref.gate_update(sq.numpy().reshape(world, len(nps)), nps, groups, sts[:len(groups)], g,
                        **rule)
        write_gate(gate, g)
        write_states(states, sts)

    def adam_update_gated_(self, params, grads, ms, vs, hyper, gate, states, group, np_):
        g, st = read_gate(gate), read_states(states)[group]
        for p, gr, m, v in zip(params, grads, ms, vs):
            dt = cpu_epilogue._DT[p.dtype]
            arrs = [cpu_epilogue._np(x) for x in (p, gr, m, v)]
            new = ref.update(*[np.ascontiguousarray(a) for a in arrs], dt, hyper, g, st, np_)
            for a, n in zip((arrs[0], arrs[2], arrs[3]), new):
                a[...] = n

    def adam_master_update_gated_(self, params16, grads16, ws, ms, vs, hyper, gate, states, group,
                                  np_):
        g, st = read_gate(gate), read_states(states)[group]
        for p, gr, w, m, v in zip(params16, grads16, ws, ms, vs):
            dt = cpu_epilogue._DT[p.dtype]
            new = ref.update_master(w.numpy().copy(), np.ascontiguousarray(cpu_epilogue._np(gr)),
                                    m.numpy().copy(), v.numpy().copy(), dt, hyper, g, st, np_)
            if new[0] is None:
                continue
            for a, n in zip((cpu_epilogue._np(p), w.numpy(), m.numpy(), v.numpy()), new):
                a[...] = n


def read_gate(t):
    from kungfu_amd import ops
    a = ops.read_step_gate(t)
    return {k: (a[k].copy() if a[k].dtype.kind == "f" and a[k].dtype.itemsize == 4 else a[k].item())
            for k in ref.GATE_FIELDS}


def read_states(t):
    from kungfu_amd import ops
    a = ops.read_step_states(t)
    return [{k: (a[k][j].copy() if a[k].dtype.itemsize == 4 else a[k][j].item())
             for k in ref.STATE_FIELDS} for j in range(a.shape[0])]


def write_gate(t, g):
    from kungfu_amd import _lib
    a = np.zeros(1, _lib.step_gate_dtype())
    for k in ref.GATE_FIELDS:
        a[k] = g[k]
    t.copy_(torch.from_numpy(a.view(np.uint8).copy()))


def write_states(t, states):
    from kungfu_amd import _lib
    a = np.zeros(len(states), _lib.step_state_dtype())
    for j, st in enumerate(states):
        for k in ref.STATE_FIELDS:
            a[k][j] = st[k]
    t.copy_(torch.from_numpy(a.view(np.uint8).copy()))


def _gated_exchange():
    from kungfu_amd.collective import Exchange
    return Exchange(epilogue=CpuGatedEpilogue())


# Two layers, f16, one parameter group each (two bucket groups): AdamW with
# its own lr and betas per layer. The gradients are multiples of 1/4 in
# [-8, 8] times the loss scale, a power of two: every sum over the ranks and
# every sum of squares is exact in any order, so the reference needs no
# knowledge of which rank holds which shard. Step BAD carries one inf on the
# last rank only.
M_SHAPES = ((7, 5), (3, 7))
M_HYPER = ({"lr": 0.1, "weight_decay": 1e-2, "betas": (0.9, 0.999), "eps": 1e-8},
           {"lr": 0.05, "weight_decay": 0.0, "betas": (0.8, 0.95), "eps": 1e-6})
M_SCALE = {"init_scale": 1024.0, "growth_interval": 2}
M_STEPS, M_BAD, M_MAX_NORM = 4, 1, 1.0


def m_params(dt="f16"):
    rng = np.random.default_rng(3)
    return [adam_master_ref.narrow(rng.standard_normal(s).astype(np.float32), dt) for s in M_SHAPES]


def m_grads(world, step, scale, dt="f16"):
    """[rank][layer]: the scaled gradients as the backward pass of
    scale_loss(loss) would leave them."""
    out = []
    for r in range(world):
        rng = np.random.default_rng(11 + 100 * step + r)
        gs = [(rng.integers(-32, 33, s) / 4.0).astype(np.float32) * np.float32(scale)
              for s in M_SHAPES]
        if step == M_BAD and r == world - 1:
            gs[1].reshape(-1)[5] = np.inf
        out.append([adam_master_ref.narrow(g, dt) for g in gs])
    return out


_M_REFERENCE = {}


def m_reference(world, steps=M_STEPS, dt="f16"):
    """(params16, masters, ms, vs, gate, states, scales) after `steps` steps,
    from step_gate_ref on oracle.reduce_avg of the ranks' gradients; computed
    once per case and shared, callers leave it unchanged."""
    key = (world, steps, dt)
    if key in _M_REFERENCE:
        return _M_REFERENCE[key]
    from oracle import oracle
    ps = m_params(dt)
    ws = [adam_master_ref.widen(a, dt).reshape(-1) for a in ps]
    ms = [np.zeros(a.size, np.float32) for a in ps]
    vs = [np.zeros(a.size, np.float32) for a in ps]
    rule = dict(growth_factor=2.0, backoff_factor=0.5, **{k: v for k, v in M_SCALE.items()
                                                           if k != "init_scale"})
    gate, states = ref.new_gate(M_SCALE["init_scale"]), [ref.new_state() for _ in ps]
    scales, lr_scale = [], 1.0
    for s in range(steps):
        scales.append(float(gate["loss_scale"]))
        gr = m_grads(world, s, scales[-1], dt)
        avg = [oracle.reduce_avg([np.ascontiguousarray(gr[r][j].reshape(-1)) for r in range(world)],
                                 dt, world) for j in range(len(ps))]
        hs = [dict(h, decoupled=True, lr=h["lr"] * lr_scale) for h in M_HYPER]
        # one dtype, so one plan: its sum of squares is exact
        ref.gate_update([[ref.sum_sq(avg)]], [0], hs, states, gate, max_norm=M_MAX_NORM, **rule)
        for j in range(len(ps)):
            p, ws[j], ms[j], vs[j] = ref.update_master(ws[j], avg[j], ms[j], vs[j], dt, hs[j], gate,
                                                       states[j])
            if p is not None:
                ps[j] = p.reshape(M_SHAPES[j])
        lr_scale *= 0.5
    _M_REFERENCE[key] = (ps, ws, ms, vs, gate, states, scales)
    return _M_REFERENCE[key]


def m_optimizer(exchange, device="cpu", dt="f16", gated=True, arrays=None):
    from kungfu_amd.optimizers import ShardedAdamOptimizer
    tt = {"f16": torch.float16, "bf16": torch.bfloat16}[dt]
    arrays = m_params(dt) if arrays is None else arrays
    ps = [torch.nn.Parameter(master.to_torch(a, dt).to(device)) for a in arrays]
    assert ps[0].dtype == tt
    groups = [dict(h, params=[p]) for h, p in zip(M_HYPER, ps)]
    kw = dict(max_grad_norm=M_MAX_NORM, loss_scale=dict(M_SCALE)) if gated else {}
    return ps, ShardedAdamOptimizer(torch.optim.AdamW(groups, lr=0.1), exchange=exchange,
                                    master_weights=True, **kw)


def m_run(ps, opt, world, rank, scales, device="cpu", first_step=0, steps=M_STEPS, dt="f16"):
    """`scales`: the reference's loss scale per step, what scale_loss would
    have multiplied the loss by (asserted against the device's on the way)."""
    for s in range(first_step, first_step + steps):
        if opt._kf_gated:
            assert float(opt.scale_loss(torch.ones((), device=device))) == scales[s]
        gr = m_grads(world, s, scales[s], dt)[rank]
        for p, g in zip(ps, gr):
            p.grad = master.to_torch(g, dt).to(device)
        opt.step()
        for g in opt.param_groups:
            g["lr"] = g["lr"] * 0.5


def m_check(ps, opt, want, dt="f16", steps=M_STEPS - 1):
    want_p, want_w, want_m, want_v, gate, states, _ = want
    sb = opt.state_buffers()
    for j, p in enumerate(ps):
        b = sb[p]
        assert master.same_bits(master.to_numpy(p, dt), want_p[j]), ("param", j)
        assert b["step"] == steps == states[j]["step"]
        assert master.same_bits(b["master"].cpu().numpy().reshape(-1), want_w[j]), ("master", j)
        assert master.same_bits(b["exp_avg"].cpu().numpy().reshape(-1), want_m[j]), ("exp_avg", j)
        assert master.same_bits(b["exp_avg_sq"].cpu().numpy().reshape(-1), want_v[j]), ("exp_avg_sq", j)
    got = read_gate(opt._kf_gate)
    for k in ref.GATE_FIELDS:
        a, b = np.asarray(got[k]), np.asarray(gate[k]).astype(np.asarray(got[k]).dtype)
        assert a.tobytes() == b.tobytes(), (k, got[k], gate[k])
    got_s = read_states(opt._kf_gstates)
    for j, st in enumerate(states):
        for k in ref.STATE_FIELDS:
            a, b = np.asarray(got_s[j][k]), np.asarray(st[k]).astype(np.asarray(got_s[j][k]).dtype)
            assert a.tobytes() == b.tobytes(), (k, j, got_s[j][k], st[k])
    assert opt.skipped_steps() == gate["skipped"] and opt.applied_steps() == gate["applied"]
    assert opt.loss_scale_value() == float(gate["loss_scale"])
    assert opt.last_grad_norm() == gate["grad_norm"]
    assert opt.scaler_state() == {"loss_scale": float(gate["loss_scale"]),
                                  "good_steps": gate["good_steps"]}


def body_gated(rank, world, make_exchange=_gated_exchange, device="cpu"):
    """What the CPU and the GPU end-to-end tests share: the gated run against
    the reference, the skipped step, the checkpoint round trip, and the
    ungated optimizer's unchanged bits."""
    want = m_reference(world)
    scales = want[6]
    assert scales == [1024.0, 1024.0, 512.0, 512.0] and want[4]["skipped"] == 1  # backoff at BAD
    assert float(want[4]["loss_scale"]) == 1024.0                                # growth after two
    ps, opt = m_optimizer(make_exchange(), device)
    # the step before the bad one, then the bad one: nothing but the loss
    # scale and the counters moves
    m_run(ps, opt, world, rank, scales, device, steps=M_BAD)
    before = ([master.to_numpy(p, "f16") for p in ps], opt.state_buffers())
    m_run(ps, opt, world, rank, scales, device, first_step=M_BAD, steps=1)
    after = ([master.to_numpy(p, "f16") for p in ps], opt.state_buffers())
    assert opt.skipped_steps() == 1 and opt.applied_steps() == M_BAD
    assert opt.loss_scale_value() == 512.0 and not np.isfinite(opt.last_grad_norm())
    for j, p in enumerate(ps):
        assert master.same_bits(before[0][j], after[0][j]), ("param moved on a skip", j)
        assert before[1][p]["step"] == after[1][p]["step"] == M_BAD
        for k in ("master", "exp_avg", "exp_avg_sq"):
            assert master.same_bits(before[1][p][k].cpu().numpy(), after[1][p][k].cpu().numpy()), (k, j)
    m_run(ps, opt, world, rank, scales, device, first_step=M_BAD + 1, steps=M_STEPS - M_BAD - 1)
    m_check(ps, opt, want)
    assert opt.skipped_steps() == 1 and opt.state_buffers()[ps[0]]["step"] == 3
    # save, reload into a fresh optimizer, and both go on with the same bits
    sb, sc = opt.state_buffers(), opt.scaler_state()
    qs, opt2 = m_optimizer(make_exchange(), device, arrays=[master.to_numpy(p, "f16") for p in ps])
    for g2, g in zip(opt2.param_groups, opt.param_groups):
        g2["lr"] = g["lr"]
    opt2.load_state_buffers({q: sb[p] for p, q in zip(ps, qs)})
    opt2.load_scaler_state(sc)
    assert opt2.scaler_state() == sc and opt2.skipped_steps() == 0
    assert [b["step"] for b in opt2.state_buffers().values()] == [3, 3]
    more = m_reference(world, M_STEPS + 1)
    m_run(ps, opt, world, rank, more[6], device, first_step=M_STEPS, steps=1)
    m_run(qs, opt2, world, rank, more[6], device, first_step=M_STEPS, steps=1)
    m_check(ps, opt, more, steps=M_STEPS)
    sb1, sb2 = opt.state_buffers(), opt2.state_buffers()
    for j, (p, q) in enumerate(zip(ps, qs)):
        # the reloaded pows are Python's beta ** 3, the running products'
        # bits here: the continued run agrees bit for bit
        assert master.same_bits(master.to_numpy(p, "f16"), master.to_numpy(q, "f16")), ("reload", j)
        for k in ("master", "exp_avg", "exp_avg_sq"):
            assert master.same_bits(sb1[p][k].cpu().numpy(), sb2[q][k].cpu().numpy()), (k, j)
    # both keywords None: today's path, today's bits
    rs, plain = m_optimizer(make_exchange(), device, gated=False)
    assert not plain._kf_gated
    ones = [1.0] * M_STEPS
    m_run(rs, plain, world, rank, ones, device, steps=1)
    gr = m_grads(world, 0, 1.0)
    from oracle import oracle
    for j, p in enumerate(rs):
        avg = oracle.reduce_avg([np.ascontiguousarray(gr[r][j].reshape(-1)) for r in range(world)],
                                "f16", world)
        w0 = adam_master_ref.widen(m_params()[j], "f16").reshape(-1)
        z = np.zeros(w0.size, np.float32)
        want_p = adam_master_ref.step(w0, avg, z, z, "f16",
                                      dict(M_HYPER[j], decoupled=True, step=1))[0]
        assert master.same_bits(master.to_numpy(p, "f16").reshape(-1), want_p), ("ungated", j)


def test_reload_pows_are_the_running_products_here():
    """body_gated's reload compares bit for bit: for these betas and three
    applied steps Python's beta ** 3 is the running product."""
    for h in M_HYPER:
        for b in h["betas"]:
            assert b ** 3 == b * b * b
    assert 0.99 ** 3 != 0.99 * 0.99 * 0.99  # not so in general: the last place may differ


def test_world1_gated_optimizer_and_checkpoint():
    """The whole of body_gated in this process: no process group, world 1."""
    body_gated(0, 1)


def _entry(rank, world, store, errq):
    sys.path[:0] = [ROOT, HERE]
    try:
        dist.init_process_group("gloo", init_method="file://" + store, rank=rank,
                                world_size=world)
        import test_sharded_adam_gated as mod
        mod.body_gated(rank, world)
        dist.barrier()
    except Exception:
        errq.put("rank %d: %s" % (rank, traceback.format_exc()))
        raise
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()


def test_gated_optimizer_over_gloo():
    world = 2
    ctx = mp.get_context("spawn")
    errq = ctx.SimpleQueue()
    store = os.path.join(tempfile.mkdtemp(prefix="kfgated"), "store")
    procs = [ctx.Process(target=_entry, args=(r, world, store, errq)) for r in range(world)]
    for p in procs:
        p.start()
    hung = join_all(procs, 600)
    errs = []
    while not errq.empty():
        errs.append(errq.get())
    assert not errs, "\n".join(errs)
    assert not hung and all(p.exitcode == 0 for p in procs), hung_msg(hung, [p.exitcode for p in procs])
