"""The MXFP8 gradient wire without a device: the numpy
restatement's known answers and error bound, the piece size, and every
argument refusal of the C entries (all come before any HIP call)."""
import ctypes

import numpy as np
import pytest

import mx8_ref
from kungfu_amd import _lib
from kungfu_amd.base import DataType
from kungfu_amd.exchange import NativeExchange

OK, ERR_DTYPE, ERR_ARG = 0, 1, 3
F32, F64, I32 = int(DataType.F32), int(DataType.F64), int(DataType.I32)
f32 = np.float32


def bits(u):
    return np.array([u], np.uint32).view(np.float32)[0]


# the block's largest element -> (scale byte, its code)
KNOWN = [
    (f32(448), 128, 0x76), (f32(449), 128, 0x76), (f32(1.75), 120, 0x76),
    (np.nextafter(f32(1.75), f32(2)), 120, 0x76), (np.nextafter(f32(1.75), f32(0)), 119, 0x7E),
    (f32(2.0 ** -126), 0, 0x40), (bits(1), 0, 0x00), (bits(0x7F7FFFFF), 247, 0x78),
    (f32(np.nan), 255, 0x00), (f32(np.inf), 255, 0x00), (f32(0), 0, 0x00), (f32(-0.0), 0, 0x80),
]


@pytest.mark.parametrize("big,scale,code", KNOWN)
def test_pack_known_answers(big, scale, code):
    x = np.zeros(32, np.float32)
    x[5] = big
    p = mx8_ref.pack(x)
    assert p.size == 48 and (p[32], p[5]) == (scale, code) and not p[33:].any()
    if np.isfinite(big):
        assert abs(float(big)) * 2.0 ** (127 - scale) <= 448
        assert not mx8_ref.unpack(p)[np.arange(32) != 5].any()
    else:
        assert np.isnan(mx8_ref.unpack(p)).all()


def test_error_bound_over_the_exponent_range():
    rng = np.random.default_rng(7)
    for k in list(range(-149, 127, 5)) + [126]:
        x = (rng.standard_normal(64 * 32) * 2.0 ** k).astype(np.float32)  # flushes, saturates: fine
        x = x[np.isfinite(x.reshape(-1, 32)).all(axis=1).repeat(32)]
        p = mx8_ref.pack(x)
        X = np.repeat(2.0 ** (p[x.size:x.size + x.size // 32].astype(np.float64) - 127), 32)
        err = np.abs(mx8_ref.unpack(p).astype(np.float64) - x)
        assert (err <= np.maximum(np.abs(x.astype(np.float64)) * 2.0 ** -4, X * 2.0 ** -10)).all(), k


def pa(vals):
    return _lib.ptr_array(vals)


def cnt(*v):
    return (ctypes.c_size_t * len(v))(*v)


def test_piece_bytes_and_refusals():
    lib = _lib.load()
    for q in (0, 32, 64, 480, 512, 544, 2208, 1 << 26):
        assert lib.kf_mx8_piece_bytes(q) == mx8_ref.piece_bytes(q) == -(-(q + q // 32) // 16) * 16
    assert lib.kf_mx8_piece_bytes(32) == 48

    def pack(a=pa([64]), b=pa([128]), c=cnt(64), nb=1, world=1, dt=F32):
        return lib.kf_mx8_pack_batch(a, b, c, nb, world, dt, None)

    def fold(a=pa([64]), b=pa([128]), c=cnt(64), nb=1, world=1, dt=F32, np_=0):
        return lib.kf_mx8_fold_batch(a, b, c, nb, world, dt, np_, None)

    for call, name in ((pack, b"kf_mx8_pack_batch"), (fold, b"kf_mx8_fold_batch")):
        assert call(None, None, None, nb=0) == OK
        assert call(c=cnt(0)) == OK                      # an empty bucket is not looked at
        for kw, rc, text in (
                ({"nb": -1}, ERR_ARG, b"nb < 0"), ({"a": None}, ERR_ARG, b"null table"),
                ({"b": None}, ERR_ARG, b"null table"), ({"c": None}, ERR_ARG, b"null table"),
                ({"dt": F64}, ERR_DTYPE, b"f32, bf16 and f16"), ({"dt": I32}, ERR_DTYPE, b"f16"),
                ({"world": 0}, ERR_ARG, b"[1, 16]"), ({"world": 17, "c": cnt(64 * 17)}, ERR_ARG, b"[1, 16]"),
                ({"a": pa([0])}, ERR_ARG, b"null pointer"), ({"b": pa([0])}, ERR_ARG, b"null pointer"),
                ({"c": cnt(48)}, ERR_ARG, b"multiples of 32"), ({"a": pa([72])}, ERR_ARG, b"16-byte"),
                ({"b": pa([136])}, ERR_ARG, b"16-byte"),
                # the documented order: dtype before world before a bucket's own faults
                ({"dt": F64, "world": 0}, ERR_DTYPE, b"f16"), ({"world": 0, "a": pa([0])}, ERR_ARG, b"[1, 16]"),
                ({"a": pa([8]), "c": cnt(48)}, ERR_ARG, b"multiples of 32")):
            assert call(**kw) == rc, (name, kw)
            assert name in lib.kf_last_error() and text in lib.kf_last_error(), (name, kw)
    assert pack(world=2, c=cnt(96)) == ERR_ARG           # q = 48
    assert fold(np_=-1) == ERR_ARG and b"np < 0" in lib.kf_last_error()
    np_ = ctypes.c_int(7)
    assert lib.kf_exchange_reduce_shards_mx8_batch(None, pa([64]), cnt(64), 1, F32,
                                                   ctypes.byref(np_), None) == ERR_ARG
    assert b"kf_exchange_reduce_shards_mx8_batch" in lib.kf_exchange_last_error() and np_.value == 7


def test_set_grad_wire_refuses_unknown_wires():
    ex = NativeExchange.__new__(NativeExchange)  # the setter needs no communicator
    assert ex.set_grad_wire("mx8") is ex and ex.set_grad_wire(None) is ex
    for bad in ("fp8", "MX8", 8, ""):
        with pytest.raises(ValueError, match="grad_wire"):
            ex.set_grad_wire(bad)
