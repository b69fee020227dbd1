"""numpy restatement of the block-wise 8-bit Adam state (include/kungfu_amd.h
"8-bit block-wise state"); what tests/test_sharded_adam8*.py
measure the device code against. This file is the format's definition.

A block is 64 consecutive f32 values. Its state is 64 uint8 codes and one f32
scale `a`, the element of largest magnitude with its sign:

    mag = max|x_j|;  a = +mag if some x_j == +mag else -mag
    a = NaN (0x7FC00000) if any x_j is NaN
    y_j = 0 if a == 0 else x_j / a               (one correctly rounded division)
    code_j = #{k : mid[k] < y_j}                 (NaN y: 0)
    x_j' = T[code_j] * a                         (one f32 multiply)

T is one of two sorted tables of 256 f32 values (TABLES[0]: signed, exp_avg;
TABLES[1]: unsigned, exp_avg_sq), mid[k] = f32((f64(T[k]) + f64(T[k+1])) / 2).

The step: dequantize m and v, adam_ref's f32 update (or step_gate_ref's gated
one) on them, quantize the new m and v; the parameter comes from the
unquantized new m and v.
"""
import numpy as np

import adam_master_ref
import adam_ref
import step_gate_ref

BLOCK = 64
SIGNED, UNSIGNED = 0, 1
NAN_BITS = 0x7FC00000
# the largest round-trip error of a block, relative to |a|: half the widest
# interval of the top decade
D = (0.9 / 128, 0.9 / 256)
ZERO_CODE = (127, 0)  # the code of 0.0


def _decades(n_of):
    out = []
    for i in range(7):
        n = n_of(i)
        b = [0.1 + 0.9 * k / n for k in range(n + 1)]
        out += [10.0 ** (i - 6) * (b[k] + b[k + 1]) / 2 for k in range(n)]
    return out


def _tables():
    s = _decades(lambda i: 2 ** i)
    u = _decades(lambda i: 2 ** (i + 1))
    ts = np.array(sorted([-x for x in s] + [0.0] + s + [1.0]), np.float64).astype(np.float32)
    tu = np.array(sorted([0.0] + u + [1.0]), np.float64).astype(np.float32)
    assert ts.size == 256 and tu.size == 256
    return ts, tu


TABLES = _tables()
MIDS = tuple(((t[:-1].astype(np.float64) + t[1:].astype(np.float64)) / 2).astype(np.float32)
             for t in TABLES)


def scales_of(x):
    """The signed scale of every block of x (x.size a multiple of 64)."""
    x = np.asarray(x, np.float32).reshape(-1, BLOCK)
    with np.errstate(invalid="ignore"):
        mag = np.max(np.abs(x), axis=1)  # propagates NaN
        pos = np.any(x == mag[:, None], axis=1)
        a = np.where(pos, mag, -mag).astype(np.float32)
    nan = np.isnan(x).any(axis=1)
    a[nan] = np.array([NAN_BITS], np.uint32).view(np.float32)[0]
    return a


def quantize(x, which):
    """(codes uint8[n], scales f32[n / 64])."""
    x = np.ascontiguousarray(x, np.float32)
    assert x.ndim == 1 and x.size % BLOCK == 0
    a = scales_of(x)
    ae = np.repeat(a, BLOCK)
    with np.errstate(over="ignore", invalid="ignore", under="ignore", divide="ignore"):
        y = np.where(ae == 0, np.float32(0), x / ae).astype(np.float32)
    codes = np.searchsorted(MIDS[which], y, side="left")
    codes[np.isnan(y)] = 0
    return codes.astype(np.uint8), a


def dequantize(codes, scales, which):
    codes = np.asarray(codes, np.uint8)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        return (TABLES[which][codes] * np.repeat(np.asarray(scales, np.float32), BLOCK)).astype(
            np.float32)


def zero_state(n, which):
    assert n % BLOCK == 0
    return np.full(n, ZERO_CODE[which], np.uint8), np.zeros(n // BLOCK, np.float32)


def step(p, g, mc, vc, ms, vs, h, np_=0):
    """One update of f32 parameters. Returns (p', mc', vc', ms', vs')."""
    m, v = dequantize(mc, ms, SIGNED), dequantize(vc, vs, UNSIGNED)
    p, m, v = adam_ref.step(np.asarray(p, np.float32), np.asarray(g, np.float32), m, v, "f32", h,
                            np_)
    return (p,) + _pack(m, v)


def step_gated(p, g, mc, vc, ms, vs, h, gate, state, np_=0):
    """step under a gate; a skipped step returns copies of everything."""
    if gate["skip"]:
        return tuple(np.array(x, copy=True) for x in (p, mc, vc, ms, vs))
    m, v = dequantize(mc, ms, SIGNED), dequantize(vc, vs, UNSIGNED)
    p, m, v = step_gate_ref.update(np.asarray(p, np.float32), np.asarray(g, np.float32), m, v,
                                   "f32", h, gate, state, np_)
    return (p,) + _pack(m, v)


def step_master(master, g16, mc, vc, ms, vs, dt, h, np_=0):
    """The update of bf16 / f16 parameters through their fp32 master. Returns
    (p16', master', mc', vc', ms', vs')."""
    m, v = dequantize(mc, ms, SIGNED), dequantize(vc, vs, UNSIGNED)
    p16, w, m, v = adam_master_ref.step(master, g16, m, v, dt, h, np_)
    return (p16, w) + _pack(m, v)


def step_master_gated(master, g16, mc, vc, ms, vs, dt, h, gate, state, np_=0):
    """step_master under a gate; p16' is None on a skipped step."""
    if gate["skip"]:
        return (None,) + tuple(np.array(x, copy=True) for x in (master, mc, vc, ms, vs))
    m, v = dequantize(mc, ms, SIGNED), dequantize(vc, vs, UNSIGNED)
    p16, w, m, v = step_gate_ref.update_master(master, g16, m, v, dt, h, gate, state, np_)
    return (p16, w) + _pack(m, v)


def _pack(m, v):
    mc, ms = quantize(m, SIGNED)
    vc, vs = quantize(v, UNSIGNED)
    return mc, vc, ms, vs
