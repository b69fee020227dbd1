"""numpy restatement of the stochastic-rounding Adam / AdamW update of bf16
parameters (include/kungfu_amd.h "Adam, stochastic rounding");
what tests/test_sharded_adam_sr*.py measure the device code against.

    widen p, g, m, v                                   exact
    (p', m', v') = adam_ref.step(..., "f32", h, np_)   the master path's arithmetic
    p = sr(p', r_p);  m = rne(m');  v = sr(v', r_v)

    sr(x, r) = (bits(x) + r) >> 16 for finite x; inf and NaN as rne narrows them
    (a, b) = philox2x32_10((base + i) >> 1, stream, key)
    w = (base + i) & 1 ? b : a;  r_p = w >> 16;  r_v = w & 0xffff

The gated update is step_gate_ref.update's f32 path with the same narrowing.
bf16 arrays travel as uint16 bit patterns, as in adam_ref.
"""
import numpy as np

import adam_ref
import step_gate_ref
from oracle.oracle import bf16_bits_to_f32, f32_to_bf16_bits

PHILOX_M, PHILOX_W = 0xD256D193, 0x9E3779B9
MASK32, MASK64 = 0xFFFFFFFF, (1 << 64) - 1

# (c0, c1, key) -> (a, b): the known answers of the contract
PHILOX_KAT = (((0x00000000, 0x00000000, 0x00000000), (0xFF1DAE59, 0x6CD10DF2)),
              ((0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF), (0x2C3F628B, 0xAB4FD7AD)),
              ((0x243F6A88, 0x85A308D3, 0x13198A2E), (0xDD7CE038, 0xF62A4C12)))


def philox2x32_10(c0, c1, key):
    """Philox2x32-10 on arrays (or scalars) of counters: (a, b) as uint32."""
    c0 = np.asarray(c0, np.uint64) & np.uint64(MASK32)
    c1 = np.broadcast_to(np.asarray(c1, np.uint64) & np.uint64(MASK32), c0.shape).copy()
    k = int(key) & MASK32
    for _ in range(10):
        prod = np.uint64(PHILOX_M) * c0            # below 2^64: both factors are 32-bit
        hi, lo = prod >> np.uint64(32), prod & np.uint64(MASK32)
        c0, c1 = hi ^ np.uint64(k) ^ c1, lo
        k = (k + PHILOX_W) & MASK32
    return c0.astype(np.uint32), c1.astype(np.uint32)


def sr(x, r):
    """x: float32 array, r: 16-bit random words -> bf16 bit patterns (uint16)."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    r = np.asarray(r).astype(np.uint64)
    assert (r < 65536).all()
    finite = (u & np.uint64(0x7FFFFFFF)) < np.uint64(0x7F800000)
    out = (((u + r) & np.uint64(MASK32)) >> np.uint64(16)).astype(np.uint16)
    return np.where(finite, out, f32_to_bf16_bits(x)).astype(np.uint16)


def random_bits(base, n, stream, key):
    """(r_p, r_v) of elements base .. base + n."""
    e = np.uint64(base) + np.arange(n, dtype=np.uint64)
    a, b = philox2x32_10(e >> np.uint64(1), stream, key)
    w = np.where((e & np.uint64(1)) != 0, b, a).astype(np.uint32)
    return (w >> np.uint32(16)).astype(np.uint32), (w & np.uint32(0xFFFF)).astype(np.uint32)


def _narrow(pw, mw, vw, base, stream, key):
    rp, rv = random_bits(base, pw.size, stream, key)
    return sr(pw, rp), f32_to_bf16_bits(mw), sr(vw, rv)


def step(p, g, m, v, h, base, stream, key, np_=0):
    """One update of one segment. p, g, m, v: uint16 bf16 bits. Returns
    (p', m', v') as new uint16 arrays."""
    pw, mw, vw = adam_ref.step(bf16_bits_to_f32(p), bf16_bits_to_f32(g), bf16_bits_to_f32(m),
                               bf16_bits_to_f32(v), "f32", h, np_)
    return _narrow(pw, mw, vw, base, stream, key)


def step_gated(p, g, m, v, h, gate, state, base, stream, key, np_=0):
    """The gated update: a skipped step returns copies."""
    if gate["skip"]:
        return p.copy(), m.copy(), v.copy()
    pw, mw, vw = step_gate_ref.update(bf16_bits_to_f32(p), bf16_bits_to_f32(g),
                                      bf16_bits_to_f32(m), bf16_bits_to_f32(v), "f32", h, gate,
                                      state, np_)
    return _narrow(pw, mw, vw, base, stream, key)


def splitmix64(x):
    z = (int(x) + 0x9E3779B97F4A7C15) & MASK64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
    return z ^ (z >> 31)


def stream_word(sr_seed, group_index, bucket_index):
    return splitmix64(splitmix64(sr_seed) ^ ((group_index << 32) | bucket_index)) & MASK32


def key_word(draw):
    return int(draw) & MASK32
