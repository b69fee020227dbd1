"""The MXFP8 wire's error-feedback and stochastic-rounding packs without a
device: the restatement's known answers and two properties,
the C entries' refusals in their documented order, set_grad_wire's options."""
import ctypes

import numpy as np
import pytest

import mx8_ef_sr_ref as ref
import mx8_ref
from kungfu_amd import _lib
from kungfu_amd.exchange import NativeExchange
from test_mx8 import ERR_ARG, ERR_DTYPE, F32, F64, OK, cnt, f32, pa


def up(v, k=1):
    """v, k f32 steps away from zero"""
    return (np.array([v], f32).view(np.int32) + np.int32(k)).view(f32)[0]


# (element, draw, code) in one block whose largest element, 430, gives the scale 2^0
SR_KNOWN = [
    (18, 0, 0x59), (18, 0xFFFF, 0x59),                # an E4M3 value: whatever the draw
    (up(18), 0, 0x59), (up(18), 0xFFFF, 0x59),        # 1 + 0xffff0 stays below 2^20
    (up(18, 16), 0xFFFF, 0x5A), (up(18, 16), 0xFFFE, 0x59),
    (2.0 ** -6, 0, 0x08), (2.0 ** -6, 0xFFFF, 0x08),  # the smallest normal code, by the first formula
    (up(2.0 ** -6, -1), 0, 0x07), (up(2.0 ** -6, -1), 0xFFFF, 0x08),
    (2.0 ** -10, 0x7FFF, 0x00), (2.0 ** -10, 0x8000, 0x01), (-2.0 ** -10, 0x8000, 0x81),
    (2.0 ** -30, 0xFFFF, 0x00), (-2.0 ** -30, 0xFFFF, 0x80),
    (430, 0, 0x7D), (430, 0xFFFF, 0x7E), (-430, 0x9000, 0xFE), (-430, 0x8FFF, 0xFD),
    (-0.0, 0xFFFF, 0x80), (0.0, 0xFFFF, 0x00),
]


def test_pack_sr_known_answers():
    x = np.zeros(32, f32)
    x[:len(SR_KNOWN)] = [v for v, _, _ in SR_KNOWN]
    r = np.zeros(32, np.uint32)
    r[:len(SR_KNOWN)] = [d for _, d, _ in SR_KNOWN]
    p = ref.pack_sr(x, 0, 0, 0, 0, 0, r16=r)
    assert p[32] == 127 and p[:len(SR_KNOWN)].tolist() == [c for _, _, c in SR_KNOWN]
    for k in (-100, 100):  # the same codes at another scale
        assert (ref.pack_sr(np.ldexp(x, k), 0, 0, 0, 0, 0, r16=r)[:32] == p[:32]).all()
    x[9] = np.inf
    bad = ref.pack_sr(x, 0, 0, 0, 0, 0, r16=r)
    assert bad[32] == 255 and not bad[:32].any()
    # the generator's draws: the element index counts from the bucket's start; every input matters
    d = [ref.draws(*a) for a in ((5, 1, 2, 3, 0, 96), (5, 1, 2, 3, 32, 64), (5, 0, 2, 3, 0, 96),
                                 (5, 1, 1, 3, 0, 96), (5, 1, 2, 4, 0, 96), (6, 1, 2, 3, 0, 96))]
    assert (d[0][32:] == d[1]).all() and all((d[0] != o).any() for o in d[2:])


def test_pack_sr_is_unbiased():
    """Over K = 1024 steps the mean of unpack(pack_sr(x)) is within ulp / 8 of
    x: one draw's deviation is at most ulp / 2, the mean's ulp / 64, eight of
    those the bound (ulp: the spacing of E4M3 values around x at its scale)."""
    K, rng = 1024, np.random.default_rng(11)
    x = np.ldexp(rng.standard_normal(512), rng.integers(-20, 20, 16).repeat(32)).astype(f32)
    X = np.ldexp(1.0, mx8_ref.scales(x).astype(np.int64) - 127).repeat(32)
    ulp = X * np.maximum(2.0 ** (np.frexp(np.abs(x) / X)[1] - 1), 2.0 ** -6) / 8
    mean = sum(mx8_ref.unpack(ref.pack_sr(x, 7, k, 0, 0, 0)).astype(np.float64) for k in range(K)) / K
    assert (np.abs(mean - x) <= ulp / 8).all()


def test_pack_ef_sends_what_it_dropped():
    """For a constant g with 1 <= |g| < 2 the f64 sum of unpack(pack_ef) over K
    steps is K g - r_K within K f32 roundings of |g| (2^-23 |g| each): the add
    g + r rounds once per step, |g + r| < 2 |g|, and s - d is exact."""
    K, rng = 64, np.random.default_rng(12)
    g = (rng.uniform(1, 2, 256) * rng.choice([-1, 1], 256)).astype(f32)
    r, total = np.zeros(256, f32), np.zeros(256)
    for _ in range(K):
        piece, r = ref.pack_ef(g, r)
        total += mx8_ref.unpack(piece)
    assert r.any() and (np.abs(total - (K * g.astype(np.float64) - r)) <= K * 2.0 ** -23 * np.abs(g)).all()


def test_refusals_in_their_documented_order():
    lib = _lib.load()

    def ef(a=pa([64]), r=pa([256]), b=pa([128]), c=cnt(64), nb=1, world=1, dt=F32):
        return lib.kf_mx8_pack_ef_batch(a, r, b, c, nb, world, dt, None)

    def sr(a=pa([64]), b=pa([128]), c=cnt(64), nb=1, world=1, dt=F32, rank=0, bucket0=0):
        return lib.kf_mx8_pack_sr_batch(a, b, c, nb, world, dt, 1, 2, rank, bucket0, None)

    shared = (({"nb": -1}, ERR_ARG, b"nb < 0"), ({"a": None}, ERR_ARG, b"null table"),
              ({"dt": F64}, ERR_DTYPE, b"f32, bf16 and f16"), ({"world": 0}, ERR_ARG, b"[1, 16]"),
              ({"a": pa([0])}, ERR_ARG, b"null pointer"), ({"c": cnt(48)}, ERR_ARG, b"multiples of 32"),
              ({"b": pa([136])}, ERR_ARG, b"16-byte"))
    own = {ef: (({"r": None}, b"null table"), ({"r": pa([0])}, b"null residual"),
                ({"r": pa([264])}, b"residuals must be 16-byte"),
                ({"r": pa([0]), "c": cnt(48)}, b"multiples of 32"), ({"r": None, "dt": F64}, b"f16")),
           sr: (({"rank": -1}, b"rank"), ({"rank": 2, "world": 2, "c": cnt(128)}, b"rank"),
                ({"bucket0": -1}, b"bucket0"), ({"rank": 1, "c": cnt(48)}, b"multiples of 32"),
                ({"rank": 1, "world": 0}, b"[1, 16]"))}
    assert ef(None, None, None, None, nb=0) == OK and sr(None, None, None, nb=0) == OK
    for call, name in ((ef, b"kf_mx8_pack_ef_batch"), (sr, b"kf_mx8_pack_sr_batch")):
        assert call(c=cnt(0)) == OK  # an empty bucket is not looked at
        cases = list(shared) + [(kw, ERR_DTYPE if b"f16" in text else ERR_ARG, text)
                                for kw, text in own[call]]
        for kw, rc, text in cases:
            assert call(**kw) == rc, (name, kw)
            assert name in lib.kf_last_error() and text in lib.kf_last_error(), (name, kw)
    np_ = ctypes.c_int(7)
    for fn, args in ((lib.kf_exchange_reduce_shards_mx8_ef_batch, (pa([256]),)),
                     (lib.kf_exchange_reduce_shards_mx8_sr_batch, ())):
        extra = (1, 2) if not args else ()
        assert fn(None, pa([64]), *args, cnt(64), 1, F32, *extra, ctypes.byref(np_), None) == ERR_ARG
        assert b"bad arguments" in lib.kf_exchange_last_error() and np_.value == 7


def test_set_grad_wire_options():
    ex = NativeExchange.__new__(NativeExchange)  # the setter needs no communicator
    assert ex.set_grad_wire("mx8", error_feedback=True) is ex and ex.grad_residuals() == []
    assert ex.set_grad_wire("mx8", rounding="stochastic", seed=2 ** 64 - 1) is ex
    assert ex.set_grad_wire("mx8", rounding="nearest") is ex and ex.set_grad_wire(None) is ex
    for kw in ({"wire": "mx8", "error_feedback": True, "rounding": "stochastic"},
               {"wire": None, "error_feedback": True}, {"wire": None, "rounding": "stochastic"},
               {"wire": "mx8", "rounding": "up"}, {"wire": "mx8", "seed": -1}, {"wire": "mx8", "seed": 1.0}):
        with pytest.raises(ValueError, match="grad_wire"):
            ex.set_grad_wire(**kw)
    ex.reset_grad_residuals()
