"""The MXFP8 wire's error-feedback and stochastic-rounding packs (include/
kungfu_amd.h) restated in numpy over tests/mx8_ref.py."""
import numpy as np

import mx8_ref
from adam_sr_ref import MASK32, philox2x32_10, splitmix64

BLOCK = mx8_ref.BLOCK


def pack_ef(x, r):
    """One piece with error feedback: (the piece of x + r, the new residual)."""
    with np.errstate(all="ignore"):
        s = np.asarray(x, np.float32) + np.asarray(r, np.float32)
        piece = mx8_ref.pack(s)
        out = s - mx8_ref.unpack(piece, s.size)
    out[np.repeat(mx8_ref.scales(s) == 255, BLOCK)] = 0.0
    return piece, out


def draws(seed, step, rank, bucket, base, n):
    """The 16-bit draws of the bucket's elements base .. base + n."""
    w = splitmix64(splitmix64(splitmix64(seed) ^ step) ^ (rank << 32 | bucket))
    i = np.uint64(base) + np.arange(n, dtype=np.uint64)
    a, b = philox2x32_10(i >> np.uint64(2), w >> 32, w & MASK32)
    four = np.stack([a >> 16, a & 0xFFFF, b >> 16, b & 0xFFFF])
    return four[(i & np.uint64(3)).astype(np.int64), np.arange(n)].astype(np.uint32)


def pack_sr(x, seed, step, rank, bucket, base, r16=None):
    """One piece, rounded stochastically; x starts at element `base` of bucket
    `bucket`. r16: draws to use in place of the generator's."""
    x = np.ascontiguousarray(x, np.float32)
    q, s = x.size, mx8_ref.scales(x)
    r = (draws(seed, step, rank, bucket, base, q) if r16 is None
         else np.broadcast_to(np.asarray(r16, np.uint32), (q,))) << np.uint32(4)
    with np.errstate(all="ignore"):
        y = np.ldexp(x.astype(np.float64), -np.repeat(s.astype(np.int64) - 127, BLOCK)).astype(np.float32)
        t = np.abs(y)
        small = ((t * np.float32(2.0 ** 29)).astype(np.int64) + r) >> 20
    mag = np.where(t >= np.float32(2.0 ** -6), ((t.view(np.uint32).astype(np.int64) + r) >> 20) - 960, small)
    codes = (x.view(np.uint32) >> 31 << 7 | mag).astype(np.uint8)
    codes[np.repeat(s == 255, BLOCK)] = 0
    out = np.zeros(mx8_ref.piece_bytes(q), np.uint8)
    out[:q], out[q:q + q // BLOCK] = codes, s
    return out
