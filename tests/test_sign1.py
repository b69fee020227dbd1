"""The 1-bit gradient wire without a device: the piece size,
the C entries' refusals in their documented order, set_grad_wire's options,
and the property of the restatement that bounds the residual."""
import ctypes

import numpy as np
import pytest

import sign1_ref as ref
from kungfu_amd import _lib
from kungfu_amd.exchange import GRAD_WIRES, NativeExchange
from test_mx8 import ERR_ARG, ERR_DTYPE, F32, F64, OK, cnt, pa


def test_piece_bytes():
    lib = _lib.load()
    for q in (0, 64, 128, 960, 1024, 1 << 26):
        assert lib.kf_sign1_piece_bytes(q) == ref.piece_bytes(q) == -(-(q // 8 + q // 16) // 16) * 16
    assert lib.kf_sign1_piece_bytes(64) == 16 and lib.kf_sign1_piece_bytes(1 << 26) * 16 == 3 << 26


# (arguments that differ from a good call, status, a piece of kf_last_error's text), in the
# documented order: dtype, then the world, then a bucket's own faults, then the residuals
LADDER = (
    ({"nb": -1}, ERR_ARG, b"nb < 0"), ({"a": None}, ERR_ARG, b"null table"),
    ({"b": None}, ERR_ARG, b"null table"), ({"c": None}, ERR_ARG, b"null table"),
    ({"dt": F64}, ERR_DTYPE, b"f32, bf16 and f16"), ({"dt": F64, "world": 0}, ERR_DTYPE, b"f16"),
    ({"world": 0}, ERR_ARG, b"[1, 16]"), ({"world": 17, "c": cnt(64 * 17)}, ERR_ARG, b"[1, 16]"),
    ({"world": 0, "a": pa([0])}, ERR_ARG, b"[1, 16]"),
    ({"a": pa([0])}, ERR_ARG, b"null pointer"), ({"b": pa([0])}, ERR_ARG, b"null pointer"),
    ({"c": cnt(96)}, ERR_ARG, b"multiples of 64"), ({"a": pa([8]), "c": cnt(32)}, ERR_ARG, b"multiples of 64"),
    ({"a": pa([72])}, ERR_ARG, b"16-byte"), ({"b": pa([136])}, ERR_ARG, b"16-byte"),
)
PACK_OWN = (({"r": None}, ERR_ARG, b"null table"), ({"r": pa([0])}, ERR_ARG, b"null residual"),
            ({"r": pa([264])}, ERR_ARG, b"residuals must be 16-byte"),
            ({"r": pa([0]), "c": cnt(96)}, ERR_ARG, b"multiples of 64"),
            ({"r": None, "dt": F64}, ERR_DTYPE, b"f16"),
            ({"world": 2, "c": cnt(192)}, ERR_ARG, b"multiples of 64"))  # q = 96


def pack(a=pa([64]), r=pa([256]), b=pa([128]), c=cnt(64), nb=1, world=1, dt=F32):
    return _lib.load().kf_sign1_pack_ef_batch(a, r, b, c, nb, world, dt, None)


def fold(a=pa([64]), b=pa([128]), c=cnt(64), nb=1, world=1, dt=F32, np_=0):
    return _lib.load().kf_sign1_fold_batch(a, b, c, nb, world, dt, np_, None)


@pytest.mark.parametrize("call,name,cases", (
    (pack, b"kf_sign1_pack_ef_batch", LADDER + PACK_OWN),
    (fold, b"kf_sign1_fold_batch", LADDER + (({"np_": -1}, ERR_ARG, b"np < 0"),))), ids=("pack", "fold"))
def test_refusals_in_their_documented_order(call, name, cases):
    lib = _lib.load()
    assert call(a=None, b=None, c=None, nb=0) == OK and call(c=cnt(0)) == OK  # an empty bucket is not looked at
    for kw, rc, text in cases:
        assert call(**kw) == rc, kw
        assert name in lib.kf_last_error() and text in lib.kf_last_error(), kw


def test_exchange_entry_refuses_a_null_exchange():
    lib, np_ = _lib.load(), ctypes.c_int(7)
    assert lib.kf_exchange_reduce_shards_sign1_batch(None, pa([64]), pa([256]), cnt(64), 1, F32,
                                                     ctypes.byref(np_), None) == ERR_ARG
    assert b"kf_exchange_reduce_shards_sign1_batch" in lib.kf_exchange_last_error() and np_.value == 7


def test_set_grad_wire_options():
    ex = NativeExchange.__new__(NativeExchange)  # the setter needs no communicator
    assert "sign1" in GRAD_WIRES
    assert ex.set_grad_wire("sign1", error_feedback=True) is ex and ex.grad_residuals() == []
    assert ex.set_grad_wire("sign1", error_feedback=True, rounding="nearest", seed=3) is ex
    for kw in ({}, {"rounding": "stochastic"}, {"error_feedback": False},
               {"error_feedback": True, "rounding": "stochastic"}, {"error_feedback": True, "seed": -1}):
        with pytest.raises(ValueError, match="grad_wire"):
            ex.set_grad_wire("sign1", **kw)
    assert ex.set_grad_wire(None) is ex


def test_the_compressor_is_a_contraction():
    """Per block |s - d|^2 = |s|^2 - |s|_1^2 / 64 <= |s|^2 (in float64 over
    the restatement's f32 output), with a slack of 64 f32 ulps of |s|^2 for
    the f32 tree; and r' is s - d."""
    rng = np.random.default_rng(27)
    g = np.ldexp(rng.standard_normal(256 * 64), rng.integers(-60, 60, 256).repeat(64)).astype(np.float32)
    r = (g * rng.uniform(-2, 2, g.size)).astype(np.float32)
    piece, res = ref.pack_ef(g, r)
    s, d = (g + r).astype(np.float64).reshape(-1, 64), ref.unpack(piece, g.size).astype(np.float64).reshape(-1, 64)
    ss = (s * s).sum(axis=1)
    assert (((s - d) ** 2).sum(axis=1) <= ss + 64 * np.spacing(ss.astype(np.float32))).all()
    assert (np.sign(d) == np.sign(s)).all() and np.array_equal(res.reshape(-1, 64), (s - d).astype(np.float32))
    # the scale is the mean of |s| within the tree's six roundings
    assert np.allclose(np.abs(d[:, 0]), np.abs(s).mean(axis=1), rtol=2.0 ** -20, atol=0)
