"""The refusals of the batched update entries and of their ops wrappers, with
their full texts and their order. Every check driven here comes before the
first HIP call (C entries) or before the device check (wrappers), so nothing
needs a GPU.

A C entry's ladder is driven one rung at a time; then, for every pair of
adjacent rungs, one call trips both and the earlier rung's text must win."""
import ctypes

import pytest
import torch

from kungfu_amd import _lib, ops

OK, ERR_DTYPE, ERR_ARG = 0, 1, 3
F32, I32, F16, BF16, F64 = 0x20408, 0x10408, 0x20208, 0x20209, 0x20808
GATE, STATE = 4096, 8192  # never dereferenced: every call here ends before a launch


def pa(ptrs):
    return _lib.ptr_array(ptrs)


def cnt(*v):
    return (ctypes.c_size_t * len(v))(*v)


def u64(*v):
    return (ctypes.c_uint64 * len(v))(*v)


def u32(*v):
    return (ctypes.c_uint32 * len(v))(*v)


def hyper(n=2, bias2=None):
    h = _lib.adam_hyper_array([{"lr": 1e-3, "step": 1}] * n)
    if bias2 is not None:
        for b, x in enumerate(bias2):
            h[b].bias_correction2 = x
    return h


# entry -> (pointer tables, a dtype it takes, one it refuses, the refusal's text,
#           whether the dtype is checked before the tables (LAMB))
ADAM_FAMILIES = {
    "kf_adam_update_batch": (
        4, F32, F16, "f32, bf16 and f64 only (eps = 1e-8 is 0 in f16: 0 / 0 where v == 0)", False),
    "kf_adam_master_update_batch": (
        5, BF16, F32, "bf16 and f16 parameters only (f32 and f64 take kf_adam_update_batch)",
        False),
    "kf_adam_sr_update_batch": (
        4, BF16, F32, "bf16 only (f32 and f64 take kf_adam_update_batch; f16 the master path)",
        False),
    "kf_adam8_update_batch": (
        6, F32, BF16, "f32 only (bf16 and f16 take kf_adam8_master_update_batch)", False),
    "kf_adam8_master_update_batch": (
        7, F16, F32, "bf16 and f16 parameters only (f32 takes kf_adam8_update_batch)", False),
    "kf_lamb_moments_batch": (
        5, F64, BF16, "f32 and f64 only (bf16 and f16 take kf_lamb_master_moments_batch)", True),
    "kf_lamb_master_moments_batch": (
        5, BF16, F64, "bf16 and f16 gradients only (f32 and f64 take kf_lamb_moments_batch)",
        True),
}
GATED_DTYPE_TEXT = {  # where the gated entry's text names the gated sibling
    "kf_lamb_moments_batch":
        "f32 and f64 only (bf16 and f16 take kf_lamb_master_moments_batch_gated)",
    "kf_lamb_master_moments_batch":
        "bf16 and f16 gradients only (f32 and f64 take kf_lamb_moments_batch_gated)",
}
CASES = [(e, g) for e in ADAM_FAMILIES for g in (False, True)]


class Entry:
    """One C entry, called with keyword overrides of a legal two-segment call."""

    def __init__(self, base, gated):
        self.ntab, self.dt, self.bad_dt, self.dtype_text, self.dtype_first = ADAM_FAMILIES[base]
        if gated:
            self.dtype_text = GATED_DTYPE_TEXT.get(base, self.dtype_text)
        self.name = base + ("_gated" if gated else "")
        self.gated, self.sr, self.b8 = gated, "_sr_" in base, "adam8" in base
        self.fn = getattr(_lib.load(), self.name)
        self.n16 = self.ntab - 2 if self.b8 else self.ntab  # the 16-byte aligned tables

    def tables(self):
        """Two segments per table, every pointer 16-byte aligned and distinct."""
        return [[1024 * (i + 1), 1024 * (i + 1) + 512] for i in range(self.ntab)]

    def __call__(self, tabs=None, counts=(64, 192), nb=2, dt=None, np_=0, hyper_=True,
                 gate=GATE, state=STATE, bases=(0, 64), streams=(1, 2), null=()):
        """null: indices of tables passed as NULL; ntab is counts, ntab + 1 the
        hyper, ntab + 2 / + 3 the stochastic-rounding bases / streams."""
        tabs = [pa(t) for t in (self.tables() if tabs is None else tabs)]
        tabs = [None if i in null else t for i, t in enumerate(tabs)]
        counts = None if self.ntab in null else cnt(*counts)
        h = None if self.ntab + 1 in null or hyper_ is None else \
            (hyper() if hyper_ is True else hyper_)
        args = tabs + [counts]
        if self.sr:
            args += [None if self.ntab + 2 in null else u64(*bases),
                     None if self.ntab + 3 in null else u32(*streams)]
        args += [nb, self.dt if dt is None else dt, np_, h]
        if self.sr:
            args.append(7)
        if self.gated:
            args += [gate, state]
        return self.fn(*args, None)

    def refused(self, code, what, **kw):
        rc = self(**kw)
        text = _lib.load().kf_last_error().decode()
        name = {ERR_ARG: "KF_ERR_ARG", ERR_DTYPE: "KF_ERR_DTYPE"}[code]
        assert (rc, text) == (code, "%s: %s: %s" % (name, self.name, what)), kw

    def with_ptr(self, table, seg, ptr):
        t = self.tables()
        t[table][seg] = ptr
        return t

    @property
    def align16_text(self):
        return "parameter, gradient and codes pointers must be 16-byte aligned" if self.b8 else \
            "pointers must be 16-byte aligned"


@pytest.mark.parametrize("base,gated", CASES)
def test_entry_refusals_one_at_a_time(base, gated):
    e = Entry(base, gated)
    e.refused(ERR_ARG, "nb < 0", nb=-1)
    assert e(nb=0) == OK
    assert e(nb=0, null=range(e.ntab + 4), gate=None, state=None) == OK
    assert e(counts=(0, 0)) == OK                      # empty segments: nothing is launched
    assert e(counts=(0, 0), tabs=[[0, 8]] * e.ntab) == OK
    if gated:
        e.refused(ERR_ARG, "null gate or step state", gate=None)
        e.refused(ERR_ARG, "null gate or step state", state=None)
    for i in range(e.ntab + (4 if e.sr else 2)):       # every table, counts, hyper, bases, streams
        e.refused(ERR_ARG, "null table", null=(i,))
    for dt in (e.bad_dt, I32, 0x12345):
        e.refused(ERR_DTYPE, e.dtype_text, dt=dt)
    e.refused(ERR_ARG, "np < 0", np_=-1)
    for i in range(e.ntab):
        for seg in (0, 1):
            e.refused(ERR_ARG, "null pointer in a non-empty segment", tabs=e.with_ptr(i, seg, 0))
    for i in range(e.n16):
        e.refused(ERR_ARG, e.align16_text, tabs=e.with_ptr(i, 1, 1024 * (i + 1) + 520))
    if e.b8:
        e.refused(ERR_ARG, "counts must be multiples of 64 (a block)", counts=(64, 200))
        for i in (e.ntab - 2, e.ntab - 1):
            e.refused(ERR_ARG, "scales pointers must be 4-byte aligned",
                      tabs=e.with_ptr(i, 0, 1024 * (i + 1) + 2))
    if not gated:  # a gated call's bias corrections are the device's: never refused
        for bad in (0.0, -0.5, float("nan")):
            e.refused(ERR_ARG, "bias corrections must be > 0", hyper_=hyper(bias2=(1.0, bad)))
        h = hyper()
        h[0].bias_correction1 = 0.0
        e.refused(ERR_ARG, "bias corrections must be > 0", hyper_=h)
    if e.sr:
        e.refused(ERR_ARG, "bases must be multiples of 8 elements", bases=(0, 68))
        e.refused(ERR_ARG, "base + count must be at most 2^33", bases=(0, (1 << 33) - 64))
        e.refused(ERR_ARG, "base + count must be at most 2^33", bases=((1 << 33) + 8, 64))


@pytest.mark.parametrize("base,gated", CASES)
def test_entry_refusals_keep_their_order(base, gated):
    """Two adjacent rungs tripped in one call: the earlier one's text."""
    e = Entry(base, gated)
    bad_h = hyper(bias2=(0.0, 0.0))
    e.refused(ERR_ARG, "nb < 0", nb=-1, gate=None, null=(0,), dt=e.bad_dt, np_=-1)
    assert e(nb=0, gate=None, null=(0,), dt=e.bad_dt, np_=-1) == OK
    if gated:
        e.refused(ERR_ARG, "null gate or step state", gate=None, null=(0,), dt=e.bad_dt)
        e.refused(ERR_ARG, "null gate or step state", state=None, null=(e.ntab + 1,),
                  dt=e.bad_dt)
    if e.dtype_first:
        e.refused(ERR_DTYPE, e.dtype_text, dt=e.bad_dt, null=(0,), np_=-1)
        e.refused(ERR_DTYPE, e.dtype_text, dt=e.bad_dt, null=(e.ntab + 1,))
        e.refused(ERR_ARG, "null table", null=(e.ntab - 1,), np_=-1)
    else:
        e.refused(ERR_ARG, "null table", null=(e.ntab - 1,), dt=e.bad_dt)
        e.refused(ERR_ARG, "null table", null=(e.ntab + 1,), dt=e.bad_dt)
        e.refused(ERR_DTYPE, e.dtype_text, dt=e.bad_dt, np_=-1)
    first = "counts must be multiples of 64 (a block)" if e.b8 else \
        "null pointer in a non-empty segment"
    e.refused(ERR_ARG, "np < 0", np_=-1, tabs=e.with_ptr(0, 0, 0), counts=(72, 192))
    if e.b8:
        e.refused(ERR_ARG, first, counts=(72, 192), tabs=e.with_ptr(0, 0, 0))
    # within one segment: null pointer, 16-byte alignment, [4-byte], bias, [bases]
    t = e.with_ptr(e.n16 - 1, 0, 0)
    t[0][0] += 8
    e.refused(ERR_ARG, "null pointer in a non-empty segment", tabs=t)
    t = e.with_ptr(e.n16 - 1, 0, 1024 * e.n16 + 8)
    if e.b8:
        t[e.ntab - 1][0] += 2
        e.refused(ERR_ARG, e.align16_text, tabs=t, hyper_=bad_h)
        e.refused(ERR_ARG, "scales pointers must be 4-byte aligned",
                  tabs=e.with_ptr(e.ntab - 1, 0, 1024 * e.ntab + 2), hyper_=bad_h)
    else:
        e.refused(ERR_ARG, e.align16_text, tabs=t, hyper_=bad_h, bases=(4, 64))
    if not gated:
        if e.sr:
            e.refused(ERR_ARG, "bias corrections must be > 0", hyper_=bad_h, bases=(4, 64))
        # across segments: all of segment 0 comes before anything of segment 1
        e.refused(ERR_ARG, "bias corrections must be > 0", hyper_=hyper(bias2=(0.0, 1.0)),
                  tabs=e.with_ptr(0, 1, 0))
    if e.sr:
        e.refused(ERR_ARG, "bases must be multiples of 8 elements", bases=((1 << 33) + 4, 64))
        e.refused(ERR_ARG, "bases must be multiples of 8 elements", bases=(4, 64),
                  tabs=e.with_ptr(0, 1, 0))
    # an empty segment is not looked at
    e.refused(ERR_ARG, "null pointer in a non-empty segment", counts=(0, 192),
              tabs=[[8, 0]] + e.tables()[1:])


def sgd_call(params=(1024, 1536), grads=(2048, 2560), moms=(3072, 3584), counts=(64, 192), nb=2,
             dt=F32, np_=0, momentum=(0.9, 0.9), null=()):
    h = _lib.sgd_hyper_array([{"lr": 0.1, "momentum": m} for m in momentum])
    args = [pa(params), pa(grads), None if moms is None else pa(moms), cnt(*counts), nb, dt, np_,
            h]
    args = [None if i in null else a for i, a in enumerate(args)]
    return _lib.load().kf_sgd_update_batch(*args, None)


def sgd_refused(code, what, **kw):
    rc = sgd_call(**kw)
    name = {ERR_ARG: "KF_ERR_ARG", ERR_DTYPE: "KF_ERR_DTYPE"}[code]
    assert (rc, _lib.load().kf_last_error().decode()) == \
        (code, "%s: kf_sgd_update_batch: %s" % (name, what)), kw


def test_sgd_entry_refusals():
    sgd_refused(ERR_ARG, "nb < 0", nb=-1)
    assert sgd_call(nb=0, null=(0, 1, 2, 3, 7)) == OK
    assert sgd_call(counts=(0, 0)) == OK
    for i in (0, 1, 3, 7):
        sgd_refused(ERR_ARG, "null table", null=(i,))
    for dt in (I32, 0x12345):
        sgd_refused(ERR_DTYPE, "f32, f16, bf16 and f64 only", dt=dt)
    sgd_refused(ERR_ARG, "np < 0", np_=-1)
    sgd_refused(ERR_ARG, "null pointer in a non-empty segment", params=(1024, 0))
    sgd_refused(ERR_ARG, "null pointer in a non-empty segment", grads=(0, 2560))
    sgd_refused(ERR_ARG, "momentum != 0 needs a momentum buffer", moms=(3072, 0))
    sgd_refused(ERR_ARG, "momentum != 0 needs a momentum buffer", moms=None)
    assert sgd_call(moms=None, momentum=(0.0, 0.0), counts=(0, 0)) == OK
    for kw in (dict(params=(1032, 1536)), dict(grads=(2048, 2568)), dict(moms=(3072, 3592)),
               dict(moms=(3080, 3584), momentum=(0.0, 0.0))):
        sgd_refused(ERR_ARG, "pointers must be 16-byte aligned", **kw)


def test_sgd_entry_refusals_keep_their_order():
    sgd_refused(ERR_ARG, "nb < 0", nb=-1, null=(0,), dt=I32, np_=-1)
    assert sgd_call(nb=0, null=(0,), dt=I32, np_=-1) == OK
    sgd_refused(ERR_ARG, "null table", null=(1,), dt=I32)
    sgd_refused(ERR_DTYPE, "f32, f16, bf16 and f64 only", dt=I32, np_=-1)
    sgd_refused(ERR_ARG, "np < 0", np_=-1, params=(0, 1536))
    sgd_refused(ERR_ARG, "null pointer in a non-empty segment", params=(0, 1536), moms=(0, 3584))
    sgd_refused(ERR_ARG, "momentum != 0 needs a momentum buffer", moms=(0, 3584),
                grads=(2056, 2560))
    sgd_refused(ERR_ARG, "pointers must be 16-byte aligned", grads=(2056, 2560), params=(1024, 0))
    sgd_refused(ERR_ARG, "null pointer in a non-empty segment", counts=(0, 192),
                params=(8, 0))


# -- the ops wrappers: what is refused before the device check -----------------

def seg(dtype=torch.float32, n=(64, 192)):
    return [torch.zeros(k, dtype=dtype) for k in n]


H = {"lr": 1e-3, "step": 1}
GATED = dict(gate=None, states=None)  # never looked at before the device check

# wrapper -> (tensor tables, the text of a table-length mismatch, what an empty call returns:
#             the index of the returned table)
WRAPPERS = {
    "sgd_update_batch_": (3, "one grad, momentum and hyper per param segment", 0),
    "adam_update_batch_": (4, "one grad, exp_avg, exp_avg_sq and hyper per param segment", 0),
    "adam_master_update_batch_": (
        5, "one grad, master, exp_avg, exp_avg_sq and hyper per param segment", 0),
    "adam_update_batch_gated_": (4, "one grad, exp_avg and exp_avg_sq per param segment", 0),
    "adam_master_update_batch_gated_": (
        5, "one grad, master, exp_avg and exp_avg_sq per param segment", 0),
    "adam_sr_update_batch_": (
        4, "one grad, exp_avg, exp_avg_sq, base and stream word per param segment", 0),
    "adam_sr_update_batch_gated_": (
        4, "one grad, exp_avg, exp_avg_sq, base and stream word per param segment", 0),
    "adam8_update_batch_": (
        6, "one grad, codes and scales tensor of each state per param segment", 0),
    "adam8_update_batch_gated_": (
        6, "one grad, codes and scales tensor of each state per param segment", 0),
    "adam8_master_update_batch_": (
        7, "one grad, codes and scales tensor of each state and a master per param segment", 0),
    "adam8_master_update_batch_gated_": (
        7, "one grad, codes and scales tensor of each state and a master per param segment", 0),
    "lamb_moments_batch_": (
        5, "one grad, exp_avg, exp_avg_sq, update and hyper per param segment", 4),
    "lamb_master_moments_batch_": (
        5, "one master, exp_avg, exp_avg_sq, update and hyper per gradient segment", 4),
    "lamb_moments_batch_gated_": (
        5, "one grad, exp_avg, exp_avg_sq and update per param segment", 4),
    "lamb_master_moments_batch_gated_": (
        5, "one master, exp_avg, exp_avg_sq and update per gradient segment", 4),
}


def wrapper_call(name, tables, nhyper=None, **kw):
    """The wrapper on `tables`, with hypers (nhyper of them, default one per
    segment) or the one hyper and a gate, and SR's bases, streams and key."""
    fn, gated, sr = getattr(ops, name), name.endswith("gated_"), "_sr_" in name
    n = len(tables[0])
    args = list(tables) + ([H, None, None] if gated else [[H] * (n if nhyper is None else nhyper)])
    if sr:
        args += [kw.pop("bases", [64 * i for i in range(n)]),
                 kw.pop("streams", list(range(n))), kw.pop("key", 7)]
    return fn(*args, **kw)


def raises(text, name, *a, **kw):
    with pytest.raises(ValueError) as err:
        wrapper_call(name, *a, **kw)
    assert str(err.value) == text


@pytest.mark.parametrize("name", sorted(WRAPPERS))
def test_wrapper_refusals_before_the_device_check(name):
    ntab, words, ret = WRAPPERS[name]
    gated, sr = name.endswith("gated_"), "_sr_" in name
    tables = [seg() for _ in range(ntab)]
    raises("kungfu_amd device ops need GPU tensors (got cpu)", name, tables)
    for i in range(1, ntab):                           # a table one segment short
        short = [t[:1] if k == i else t for k, t in enumerate(tables)]
        raises("%s: %s" % (name, words), name, short)
    short0 = [tables[0][:1]] + tables[1:]
    if not gated:                                      # one hyper too few
        lone = "%s: one hyper per param segment" % name if sr or "adam8" in name else \
            "%s: %s" % (name, words)
        raises(lone, name, tables, nhyper=1)
        if sr or "adam8" in name:                      # the hypers are counted first
            raises(lone, name, [t[:1] if k == 1 else t for k, t in enumerate(tables)], nhyper=1)
    raises("%s: %s" % (name, words), name, short0)
    empty = [[] for _ in range(ntab)]
    out = wrapper_call(name, empty)
    assert out == [] and out is not empty[ret]         # the empty call: a new empty list
    if sr:
        text = "%s: key and stream words are 32-bit, bases 64-bit unsigned" % name
        for kw in (dict(key=-1), dict(key=1 << 32), dict(streams=[0, 1 << 32]),
                   dict(streams=[-1, 0]), dict(bases=[0, 1 << 64]), dict(bases=[-8, 0])):
            raises(text, name, tables, **kw)
        raises(text, name, empty, key=1 << 32)         # ranges come before the empty return
        raises("%s: %s" % (name, words), name, tables, bases=[0], key=-1)
        raises("%s: %s" % (name, words), name, tables, streams=[0, 1, 2])


def test_sgd_wrapper_takes_no_momentum_table():
    assert ops.sgd_update_batch_([], [], None, []) == []
    with pytest.raises(ValueError) as err:
        ops.sgd_update_batch_(seg(), seg(), None, [H])
    assert str(err.value) == "sgd_update_batch_: one grad, momentum and hyper per param segment"
    with pytest.raises(ValueError) as err:
        ops.sgd_update_batch_(seg(), seg(), None, [H, H])
    assert str(err.value) == "kungfu_amd device ops need GPU tensors (got cpu)"


@pytest.mark.parametrize("name", ["lamb_trust_update_", "lamb_trust_update_gated_"])
def test_trust_wrapper_refuses_cpu_tensors(name):
    f64 = dict(dtype=torch.float64)
    args = [torch.zeros(4, **f64), 1, torch.zeros(2, dtype=torch.int32),
            [{"lr": 1.0, "adapt": True}], torch.zeros(2, **f64), torch.zeros(2, **f64)]
    if name.endswith("gated_"):
        args.append(torch.zeros(64, dtype=torch.uint8))
    with pytest.raises(ValueError) as err:
        getattr(ops, name)(*args)
    assert str(err.value) == "kungfu_amd device ops need GPU tensors (got cpu)"
