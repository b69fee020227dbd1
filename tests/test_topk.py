"""The top-k gradient wire without a device."""
import ctypes

import pytest

import topk_ref as ref
from kungfu_amd import _lib, ops
from kungfu_amd.exchange import GRAD_WIRES, NativeExchange
from test_mx8 import ERR_ARG, ERR_DTYPE, F32, F64, OK, cnt, pa


def test_names_and_piece_bytes():
    lib = _lib.load()
    assert all(n in _lib.EXPORTED and getattr(lib, n) for n in (
        "kf_topk_piece_bytes", "kf_topk_pack_ef_batch", "kf_topk_fold_batch",
        "kf_exchange_reduce_shards_topk_batch"))
    assert ops.TOPK_BLOCK == ref.BLOCK == 64 and "topk" in GRAD_WIRES
    for k in ref.KS:
        for q in (0, 64, 192, 2112):
            assert lib.kf_topk_piece_bytes(q, k) == ops.topk_piece_bytes(q, k) == ref.piece_bytes(q, k) \
                == -(-5 * k * (q // 64) // 16) * 16
    assert lib.kf_topk_piece_bytes(1 << 26, 8) * 8 == 5 << 26 and lib.kf_topk_piece_bytes(64, 3) == 0
    with pytest.raises(ValueError, match="k must be"):
        ops.topk_piece_bytes(64, 3)


# (what differs from a good call, status, a piece of the text) in the documented order; a second fault lies further right
LADDER = (
    ({"nb": -1, "a": None}, ERR_ARG, b"nb < 0"), ({"a": None}, ERR_ARG, b"null table"),
    ({"b": None, "dt": F64}, ERR_ARG, b"null table"), ({"c": None}, ERR_ARG, b"null table"),
    ({"dt": F64}, ERR_DTYPE, b"f32, bf16 and f16"), ({"dt": F64, "world": 0}, ERR_DTYPE, b"f16"),
    ({"world": 0}, ERR_ARG, b"[1, 16]"), ({"world": 17, "c": cnt(64 * 17), "k": 3}, ERR_ARG, b"[1, 16]"),
    ({"k": 3}, ERR_ARG, b"k must be"), ({"k": 0, "a": pa([0])}, ERR_ARG, b"k must be"),
    ({"k": 16, "c": cnt(96)}, ERR_ARG, b"k must be"),
    ({"a": pa([0])}, ERR_ARG, b"null pointer"), ({"b": pa([0]), "c": cnt(96)}, ERR_ARG, b"null pointer"),
    ({"c": cnt(96)}, ERR_ARG, b"multiples of 64"), ({"a": pa([8]), "c": cnt(32)}, ERR_ARG, b"multiples of 64"),
    ({"a": pa([72])}, ERR_ARG, b"16-byte"), ({"b": pa([136])}, ERR_ARG, b"16-byte"),
)
PACK_OWN = (({"r": None}, ERR_ARG, b"null table"), ({"r": pa([0])}, ERR_ARG, b"null residual"),
            ({"r": pa([264])}, ERR_ARG, b"residuals must be 16-byte"),
            ({"r": pa([0]), "c": cnt(96)}, ERR_ARG, b"multiples of 64"),
            ({"r": None, "k": 5}, ERR_ARG, b"k must be"),
            ({"world": 2, "c": cnt(192)}, ERR_ARG, b"multiples of 64"))  # q = 96
FOLD_OWN = (({"np_": -1}, ERR_ARG, b"np < 0"), ({"np_": -1, "k": 3}, ERR_ARG, b"k must be"),
            ({"np_": -1, "a": pa([0])}, ERR_ARG, b"np < 0"))


def pack(a=pa([64]), r=pa([256]), b=pa([128]), c=cnt(64), nb=1, world=1, dt=F32, k=4):
    return _lib.load().kf_topk_pack_ef_batch(a, r, b, c, nb, world, dt, k, None)


def fold(a=pa([64]), b=pa([128]), c=cnt(64), nb=1, world=1, dt=F32, np_=0, k=4):
    return _lib.load().kf_topk_fold_batch(a, b, c, nb, world, dt, np_, k, None)


@pytest.mark.parametrize("call,name,cases", (
    (pack, b"kf_topk_pack_ef_batch", LADDER + PACK_OWN),
    (fold, b"kf_topk_fold_batch", LADDER + FOLD_OWN)), ids=("pack", "fold"))
def test_refusals_in_their_documented_order(call, name, cases):
    lib = _lib.load()
    assert call(a=None, b=None, c=None, nb=0) == OK and call(c=cnt(0)) == OK  # an empty bucket is not looked at
    for kw, rc, text in cases:
        assert call(**kw) == rc, kw
        assert name in lib.kf_last_error() and text in lib.kf_last_error(), kw


def test_exchange_entry_refuses_a_bad_k_and_a_null_exchange():
    lib, np_ = _lib.load(), ctypes.c_int(7)
    for k, text in ((3, b"k must be"), (4, b"bad arguments")):
        args = (None, pa([64]), pa([256]), cnt(64), 1, F32, k, ctypes.byref(np_), None)
        assert lib.kf_exchange_reduce_shards_topk_batch(*args) == ERR_ARG and np_.value == 7
        assert b"kf_exchange_reduce_shards_topk_batch: " + text in lib.kf_exchange_last_error()


def test_set_grad_wire_options():
    ex = NativeExchange.__new__(NativeExchange)  # the setter needs no communicator
    assert ex.set_grad_wire("topk", error_feedback=True) is ex and ex._wire_k == 4
    assert ex.set_grad_wire("topk", error_feedback=True, k=8).grad_residuals() == [] and ex._wire_k == 8
    for kw in ({"k": 3}, {"k": 0}, {"k": True}, {"k": 2.5}, {"k": "4"}):
        with pytest.raises(ValueError, match="grad_wire k"):
            ex.set_grad_wire("topk", error_feedback=True, **kw)
    for wire in ("mx8", "sign1", None):  # k is this wire's alone
        with pytest.raises(ValueError, match="grad_wire k"):
            ex.set_grad_wire(wire, error_feedback=wire is not None, k=2)
    for kw in ({}, {"error_feedback": False, "k": 2}, {"rounding": "stochastic"},
               {"error_feedback": True, "rounding": "stochastic"}):
        with pytest.raises(ValueError, match="grad_wire"):
            ex.set_grad_wire("topk", **kw)
    assert ex.set_grad_wire("sign1", error_feedback=True, k=4) is ex and ex.set_grad_wire(None) is ex
