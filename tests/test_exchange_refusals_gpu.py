"""The up-front refusals of the native exchange's batch entries
(kungfu_amd/csrc/kf_exchange.hip), with their codes, their full texts
(kf_exchange_last_error) and their order, over two loopback ranks with rank 0
acting: every call here ends before the first collective, so rank 1 has
nothing to do. Buffers are 64-element f32 tensors, two buckets per table.

A ladder is driven one rung at a time; then, for every pair of adjacent rungs,
one call trips both and the earlier rung's text must win
(tests/test_update_refusals.py does the same for the update entries)."""
import ctypes

import pytest
import torch

import loopback

pytestmark = pytest.mark.gpu

OK, ERR_DTYPE, ERR_OP, ERR_ARG = 0, 1, 2, 3
F32, F64, F16, BF16, I32, U16, I16 = 0x20408, 0x20808, 0x20208, 0x20209, 0x10408, 0x208, 0x10208
NOT_A_DTYPE = 0x12345
SUM, MIN, PROD = 0, 1, 3
AUTO, RS, A2A, RS_AVG = 0, 1, 2, 3
COUNTS = (64, 32)     # both multiples of the world; shards of 128 and 64 bytes
ODD = (64, 3)         # bucket 1 is no multiple of the world
SHARD4 = (64, 2)      # bucket 1's shard is 4 bytes: it cannot start 16-byte aligned
NP_UNTOUCHED = -7

NOT_MULTIPLE = "counts must be multiples of the world (padded buckets, no tails)"
ALIGN16 = "buckets and their shards must start 16-byte aligned"
FLOATS = "f32, f16, bf16 and f64 only"
BOTH_STATES = "every non-empty bucket needs both state shards"
MASTER_SHARD = "every non-empty bucket needs its master shard"
BIAS = "bias corrections must be > 0"

# entry -> (the keys of its arguments after the exchange, in order; "t<i>" is
# pointer table i), the dtype of its legal call
ENTRIES = {
    "kf_exchange_sgd_batch":
        ("t0 t1 t2 counts nb dt hyper algo stream", F32),
    "kf_exchange_adam_batch":
        ("t0 t1 t2 t3 counts nb dt hyper algo stream", F32),
    "kf_exchange_adam_master_batch":
        ("t0 t1 t2 t3 t4 counts nb dt hyper algo stream", BF16),
    "kf_exchange_adam_gated_batch":
        ("t0 t1 t2 t3 t4 counts nb dt np hyper gate state stream", BF16),
    "kf_exchange_reduce_shards_batch":
        ("t0 counts nb dt algo npp stream", F32),
    "kf_exchange_gather_params_batch":
        ("t0 counts nb dt stream", F32),
    "kf_exchange_all_reduce_batch":
        ("t0 t1 counts nb dt op average algo stream", F32),
    "kf_exchange_sma_batch":
        ("t0 t1 counts nb dt alpha algo stream", F32),
}


class Entry:
    """One C entry, called with keyword overrides of a legal two-bucket call.
    The legal call itself is never made: it would start a collective."""

    def __init__(self, ex, name, pool, gate, state):
        from kungfu_amd import _lib
        keys, self.dt = ENTRIES[name]
        self.name, self.keys, self.lib = name, keys.split(), ex.lib
        self.fn = getattr(ex.lib, name)
        self.ntab = sum(k.startswith("t") for k in self.keys)
        self.np = ctypes.c_int(NP_UNTOUCHED)
        self.pool = pool
        mk = _lib.sgd_hyper_array if "sgd" in name else _lib.adam_hyper_array
        self.defaults = dict(
            ex=ex._h, counts=COUNTS, nb=2, dt=self.dt, algo=AUTO, stream=None, op=SUM, average=0,
            alpha=0.5, np=0, npp=ctypes.byref(self.np), gate=gate, state=state,
            hyper=mk([{"lr": 0.1, "momentum": 0.9, "step": 1}] * 2))

    def tables(self):
        """Two buckets per table: distinct 64-element f32 buffers, 256 bytes apart."""
        return [[self.pool + 256 * (2 * i + b) for b in (0, 1)] for i in range(self.ntab)]

    def ptr(self, table, bucket, ptr=0, off=None):
        """Keywords that replace one pointer (off: move it by so many bytes)."""
        t = self.tables()[table]
        t[bucket] = t[bucket] + off if off is not None else ptr
        return {"t%d" % table: t}

    def __call__(self, **kw):
        from kungfu_amd import _lib
        v = dict(self.defaults, **{"t%d" % i: t for i, t in enumerate(self.tables())})
        v.update(kw)
        args = []
        for k in ["ex"] + self.keys:
            a = v[k]
            if a is not None and k.startswith("t"):
                a = _lib.ptr_array(a)
            elif a is not None and k == "counts":
                a = (ctypes.c_size_t * len(a))(*a)
            args.append(a)
        return self.fn(*args)

    def refused(self, code, what, prefix=True, **kw):
        rc = self(**kw)
        text = self.lib.kf_exchange_last_error().decode()
        assert (rc, text) == (code, (self.name + ": " if prefix else "") + what), kw
        assert self.np.value == NP_UNTOUCHED, kw

    def nulls(self):
        """Every argument that an empty call may leave out."""
        return {k: None for k in self.keys if k.startswith("t") or k in ("counts", "hyper")}


def adam_hyper(bias1=(0.1, 0.1), bias2=(0.1, 0.1)):
    from kungfu_amd import _lib
    h = _lib.adam_hyper_array([{"lr": 1e-3, "step": 1}] * 2)
    for b in (0, 1):
        h[b].bias_correction1, h[b].bias_correction2 = bias1[b], bias2[b]
    return h


def sgd_hyper(momentum):
    from kungfu_amd import _lib
    return _lib.sgd_hyper_array([{"lr": 0.1, "momentum": m} for m in momentum])


# ---- the shard entries' shared rungs ---------------------------------------------

def shard_rungs_one_at_a_time(e, buckets, aligned):
    """null bucket (tables `buckets`), divisibility, 16-byte alignment (tables
    `aligned`, and the shard's size)."""
    for i in buckets:
        for b in (0, 1):
            e.refused(ERR_ARG, "null bucket", **e.ptr(i, b))
    e.refused(ERR_ARG, NOT_MULTIPLE, counts=ODD)
    e.refused(ERR_ARG, NOT_MULTIPLE, counts=(3, 32))
    for i in aligned:
        for b in (0, 1):
            e.refused(ERR_ARG, ALIGN16, **e.ptr(i, b, off=8))
    e.refused(ERR_ARG, ALIGN16, counts=SHARD4)


def sgd_ladder(e):
    e.refused(ERR_ARG, "bad arguments", ex=None)
    e.refused(ERR_ARG, "bad arguments", nb=-1)
    for dt in (I32, U16, NOT_A_DTYPE):
        e.refused(ERR_DTYPE, FLOATS, dt=dt)
    assert e(nb=0) == OK and e(nb=0, **e.nulls()) == OK and e(nb=0, t2=None, algo=9) == OK
    for k in ("t0", "t1", "counts", "hyper"):
        e.refused(ERR_ARG, "null table", **{k: None})
    for algo in (-1, 4):
        e.refused(ERR_ARG, "unknown algo", prefix=False, algo=algo)
    shard_rungs_one_at_a_time(e, (0, 1), (0, 1, 2))
    needs = "momentum != 0 needs a momentum shard"
    e.refused(ERR_ARG, needs, t2=None)
    e.refused(ERR_ARG, needs, **e.ptr(2, 1))
    e.refused(ERR_ARG, needs, hyper=sgd_hyper((0.0, 0.5)), **e.ptr(2, 1))
    # a momentum shard that is not used is still looked at
    e.refused(ERR_ARG, ALIGN16, hyper=sgd_hyper((0.0, 0.0)), **e.ptr(2, 0, off=8))
    # order
    e.refused(ERR_ARG, "bad arguments", nb=-1, dt=I32)
    e.refused(ERR_DTYPE, FLOATS, nb=0, dt=I32)
    e.refused(ERR_DTYPE, FLOATS, dt=I32, hyper=None)
    e.refused(ERR_ARG, "null table", hyper=None, **e.ptr(0, 0))
    # every bucket's pointers come before the algo and before any bucket's count
    e.refused(ERR_ARG, "null bucket", algo=9, **e.ptr(1, 1))
    e.refused(ERR_ARG, "null bucket", counts=(3, 32), **e.ptr(1, 1))
    e.refused(ERR_ARG, "unknown algo", prefix=False, algo=9, counts=(3, 32))
    e.refused(ERR_ARG, NOT_MULTIPLE, counts=(3, 32), **e.ptr(2, 0))
    e.refused(ERR_ARG, needs, t0=[e.tables()[0][0] + 8, e.tables()[0][1]], **e.ptr(2, 0))
    # all of bucket 0 comes before bucket 1's count
    e.refused(ERR_ARG, ALIGN16, counts=ODD, **e.ptr(0, 0, off=8))
    e.refused(ERR_ARG, NOT_MULTIPLE, counts=ODD, **e.ptr(2, 1))
    # an empty bucket is not looked at
    e.refused(ERR_ARG, NOT_MULTIPLE, counts=(0, 3), t0=[0, e.tables()[0][1]],
              t2=[8, e.tables()[2][1]])


def adam_ladder(e, master, gated):
    """kf_exchange_adam_batch, _adam_master_batch and _adam_gated_batch (with
    master shards: table 2; without: table 2 is NULL)."""
    m, v = (3, 4) if master or gated else (2, 3)
    base = dict(t2=None, dt=F32) if gated and not master else {}

    def refused(code, what, prefix=True, **kw):
        e.refused(code, what, prefix, **dict(base, **kw))

    if gated:
        refused(ERR_ARG, "null gate", gate=None)
        refused(ERR_ARG, "null gate", gate=None, ex=None)
        refused(ERR_ARG, "null gate", gate=None, nb=-1, state=None)
    refused(ERR_ARG, "bad arguments", ex=None)
    refused(ERR_ARG, "bad arguments", nb=-1)
    if gated:
        refused(ERR_ARG, "no step state, or np < 0", state=None)
        refused(ERR_ARG, "no step state, or np < 0", np=-1)
        refused(ERR_ARG, "bad arguments", nb=-1, state=None)
        refused(ERR_ARG, "no step state, or np < 0", np=-1, dt=I32)
    if master:
        bad_dts, dtype_text = (F32, F64, I32, NOT_A_DTYPE), "bf16 and f16 only"
    else:
        bad_dts, dtype_text = (F16, I32, NOT_A_DTYPE), "f32, bf16 and f64 only"
    for dt in bad_dts:
        refused(ERR_DTYPE, dtype_text, dt=dt)
    assert e(nb=0, **base) == OK and e(nb=0, **dict(e.nulls(), dt=base.get("dt", e.dt))) == OK
    tabs = [i for i in range(e.ntab) if master or not gated or i != 2]
    for k in ["t%d" % i for i in tabs] + ["counts", "hyper"]:
        if not (gated and k == "t2"):  # no master table: the gated entry's other path
            refused(ERR_ARG, "null table", **{k: None})
    if not gated:
        for algo in (-1, 4):
            refused(ERR_ARG, "unknown algo", prefix=False, algo=algo)
    for i in (0, 1):
        for b in (0, 1):
            refused(ERR_ARG, "null bucket", **e.ptr(i, b))
    refused(ERR_ARG, NOT_MULTIPLE, counts=ODD)
    refused(ERR_ARG, NOT_MULTIPLE, counts=(3, 32))
    for i in (m, v):
        for b in (0, 1):
            refused(ERR_ARG, BOTH_STATES, **e.ptr(i, b))
    if master:
        for b in (0, 1):
            refused(ERR_ARG, MASTER_SHARD, **e.ptr(2, b))
    for i in tabs:
        for b in (0, 1):
            refused(ERR_ARG, ALIGN16, **e.ptr(i, b, off=8))
    refused(ERR_ARG, ALIGN16, counts=SHARD4)
    if not gated:  # a gated call's bias corrections are the device's: never looked at
        for bad in (0.0, -0.5, float("nan")):
            refused(ERR_ARG, BIAS, hyper=adam_hyper(bias2=(0.1, bad)))
        refused(ERR_ARG, BIAS, hyper=adam_hyper(bias1=(0.0, 0.1)))
    # order
    bad_h = adam_hyper(bias2=(0.0, 0.1))
    refused(ERR_ARG, "bad arguments", nb=-1, dt=bad_dts[0])
    refused(ERR_DTYPE, dtype_text, nb=0, dt=bad_dts[0])
    refused(ERR_DTYPE, dtype_text, dt=bad_dts[0], hyper=None)
    if gated:
        refused(ERR_ARG, "null table", hyper=None, **e.ptr(0, 0))
    else:
        refused(ERR_ARG, "null table", hyper=None, algo=9)
        refused(ERR_ARG, "unknown algo", prefix=False, algo=9, **e.ptr(0, 0))
    refused(ERR_ARG, "null bucket", counts=(3, 32), **e.ptr(1, 0))
    refused(ERR_ARG, NOT_MULTIPLE, counts=(3, 32), **e.ptr(m, 0))
    if master:
        refused(ERR_ARG, BOTH_STATES, **dict(e.ptr(v, 0), **e.ptr(2, 0)))
        refused(ERR_ARG, MASTER_SHARD, **dict(e.ptr(2, 0), **e.ptr(0, 0, off=8)))
    else:
        refused(ERR_ARG, BOTH_STATES, **dict(e.ptr(v, 0), **e.ptr(0, 0, off=8)))
    if not gated:
        refused(ERR_ARG, ALIGN16, hyper=bad_h, **e.ptr(1, 0, off=8))
        # all of bucket 0 comes before anything of bucket 1
        refused(ERR_ARG, BIAS, hyper=bad_h, **e.ptr(0, 1))
    refused(ERR_ARG, ALIGN16, counts=ODD, **e.ptr(0, 0, off=8))
    # an empty bucket is not looked at
    refused(ERR_ARG, NOT_MULTIPLE, counts=(0, 3), t0=[0, e.tables()[0][1]],
            t1=[8, e.tables()[1][1]])


def reduce_shards_ladder(e):
    e.refused(ERR_ARG, "bad arguments", ex=None)
    e.refused(ERR_ARG, "bad arguments", nb=-1)
    e.refused(ERR_ARG, "bad arguments", npp=None)
    for dt in (I32, U16, NOT_A_DTYPE):
        e.refused(ERR_DTYPE, FLOATS, dt=dt)
    for algo in (-1, 4):
        e.refused(ERR_ARG, "unknown algo", prefix=False, algo=algo)
    for k in ("t0", "counts"):
        e.refused(ERR_ARG, "null table", **{k: None})
    shard_rungs_one_at_a_time(e, (0,), (0,))
    # order
    e.refused(ERR_ARG, "bad arguments", npp=None, dt=I32)
    e.refused(ERR_DTYPE, FLOATS, dt=I32, algo=9)
    e.refused(ERR_DTYPE, FLOATS, dt=I32, algo=9, nb=0)
    e.refused(ERR_ARG, "unknown algo", prefix=False, algo=9, t0=None)
    e.refused(ERR_ARG, "unknown algo", prefix=False, algo=9, nb=0)
    e.refused(ERR_ARG, "null table", counts=None, t0=[0, 0])
    e.refused(ERR_ARG, "null bucket", counts=(3, 32), **e.ptr(0, 0))
    e.refused(ERR_ARG, NOT_MULTIPLE, counts=(3, 32), **e.ptr(0, 0, off=8))
    e.refused(ERR_ARG, ALIGN16, counts=ODD, **e.ptr(0, 0, off=8))
    e.refused(ERR_ARG, NOT_MULTIPLE, counts=(0, 3), t0=[8, e.tables()[0][1]])
    # the empty call: np is what a non-empty call would report, over this
    # transport's reduce-scatter (the world) or after a fold or ncclAvg (0)
    for dt, algo, want in ((F32, AUTO, 2), (F64, AUTO, 2), (F16, AUTO, 0), (BF16, AUTO, 0),
                           (F32, RS, 2), (BF16, RS, 2), (F32, A2A, 0), (F32, RS_AVG, 0)):
        for kw in ({}, e.nulls()):
            e.np.value = NP_UNTOUCHED
            assert e(nb=0, dt=dt, algo=algo, **kw) == OK
            assert e.np.value == want, (dt, algo)
    e.np.value = NP_UNTOUCHED


def gather_params_ladder(e):
    e.refused(ERR_ARG, "bad arguments", ex=None)
    e.refused(ERR_ARG, "bad arguments", nb=-1)
    for dt in (I32, U16, NOT_A_DTYPE):
        e.refused(ERR_DTYPE, FLOATS, dt=dt)
    assert e(nb=0) == OK and e(nb=0, **e.nulls()) == OK
    for k in ("t0", "counts"):
        e.refused(ERR_ARG, "null table", **{k: None})
    shard_rungs_one_at_a_time(e, (0,), (0,))
    # order
    e.refused(ERR_ARG, "bad arguments", nb=-1, dt=I32)
    e.refused(ERR_DTYPE, FLOATS, dt=I32, nb=0)
    e.refused(ERR_DTYPE, FLOATS, dt=I32, t0=None)
    e.refused(ERR_ARG, "null table", counts=None, t0=[0, 0])
    e.refused(ERR_ARG, "null bucket", counts=(3, 32), **e.ptr(0, 0))
    e.refused(ERR_ARG, NOT_MULTIPLE, counts=(3, 32), **e.ptr(0, 0, off=8))
    e.refused(ERR_ARG, ALIGN16, counts=ODD, **e.ptr(0, 0, off=8))
    e.refused(ERR_ARG, NOT_MULTIPLE, counts=(0, 3), t0=[8, e.tables()[0][1]])


def bucket_args_rungs(e, op_too):
    """check_bucket_args: what kf_exchange_all_reduce_batch and _sma_batch share."""
    def refused(code, what, **kw):
        e.refused(code, what, prefix=False, **kw)

    refused(ERR_ARG, "bad arguments", ex=None)
    refused(ERR_ARG, "bad arguments", nb=-1)
    for k in ("t0", "t1", "counts"):
        refused(ERR_ARG, "bad arguments", **{k: None})
    refused(ERR_DTYPE, "unsupported dtype", dt=NOT_A_DTYPE)
    for i in (0, 1):
        for b in (0, 1):
            refused(ERR_ARG, "null bucket", **e.ptr(i, b))
    assert e(nb=0) == OK and e(nb=0, **e.nulls()) == OK and e(nb=0, algo=9) == OK
    assert e(nb=0, dt=I32) == OK
    for algo in (-1, 4):
        refused(ERR_ARG, "unknown algo", algo=algo)
    # order
    refused(ERR_ARG, "bad arguments", nb=-1, dt=NOT_A_DTYPE)
    refused(ERR_ARG, "bad arguments", t0=None, dt=NOT_A_DTYPE)
    refused(ERR_DTYPE, "unsupported dtype", dt=NOT_A_DTYPE, nb=0)
    refused(ERR_DTYPE, "unsupported dtype", dt=NOT_A_DTYPE, **e.ptr(0, 0))
    refused(ERR_ARG, "null bucket", algo=9, **e.ptr(1, 1))
    # an empty bucket is not looked at
    refused(ERR_ARG, "unknown algo", algo=9, counts=(0, 3), t0=[0, e.tables()[0][1]])
    if op_too:
        refused(ERR_DTYPE, "unsupported dtype", dt=NOT_A_DTYPE, op=7)


def all_reduce_ladder(e):
    def refused(code, what, **kw):
        e.refused(code, what, prefix=False, **kw)

    bucket_args_rungs(e, op_too=True)
    for op in (4, 7, -1):
        refused(ERR_OP, "unsupported op", op=op)
    for op in (MIN, PROD):
        refused(ERR_OP, "fp16 supports SUM only", dt=F16, op=op)
    average = "average needs SUM on a float dtype"
    refused(ERR_OP, average, average=1, op=MIN)
    refused(ERR_OP, average, average=1, dt=I32)
    no_rs = "no reduce-scatter type for this dtype"
    for dt in (U16, I16):
        for algo in (RS, RS_AVG):
            refused(ERR_DTYPE, no_rs, dt=dt, algo=algo)
    # order
    refused(ERR_OP, "unsupported op", op=7, dt=F16)
    refused(ERR_OP, "unsupported op", op=7, nb=0)
    refused(ERR_OP, "fp16 supports SUM only", dt=F16, op=MIN, average=1)
    refused(ERR_OP, average, average=1, dt=I32, **e.ptr(0, 0))
    refused(ERR_ARG, "null bucket", dt=U16, algo=RS, **e.ptr(0, 0))


def sma_ladder(e):
    def refused(code, what, **kw):
        e.refused(code, what, prefix=False, **kw)

    bucket_args_rungs(e, op_too=False)
    for dt in (I32, U16):
        refused(ERR_DTYPE, "SMA needs a float dtype", dt=dt)
    # order: the buckets, the empty return, the dtype, the algo
    refused(ERR_ARG, "null bucket", dt=I32, **e.ptr(0, 0))
    refused(ERR_DTYPE, "SMA needs a float dtype", dt=I32, algo=9)


LADDERS = {
    "kf_exchange_sgd_batch": sgd_ladder,
    "kf_exchange_adam_batch": lambda e: adam_ladder(e, master=False, gated=False),
    "kf_exchange_adam_master_batch": lambda e: adam_ladder(e, master=True, gated=False),
    "kf_exchange_adam_gated_batch":
        lambda e: (adam_ladder(e, master=True, gated=True),
                   adam_ladder(e, master=False, gated=True)),
    "kf_exchange_reduce_shards_batch": reduce_shards_ladder,
    "kf_exchange_gather_params_batch": gather_params_ladder,
    "kf_exchange_all_reduce_batch": all_reduce_ladder,
    "kf_exchange_sma_batch": sma_ladder,
}


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_exchange_entry_refusals_and_their_order(name):
    from kungfu_amd import ops

    def body(rank, ex):
        if rank:
            return
        bufs = torch.zeros(2 * 5 * 64, device="cuda")  # 5 tables x 2 buckets x 64 f32
        gate, st = ops.new_step_gate("cuda"), ops.new_step_states("cuda", 1)
        assert bufs.data_ptr() % 256 == 0
        LADDERS[name](Entry(ex, name, bufs.data_ptr(), gate.data_ptr(), st.data_ptr()))

    loopback.loop_ranks(2, body)
