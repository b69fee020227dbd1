"""numpy restatement of Lion and its sign code format (include/kungfu_amd.h
"Lion"), the definition tests/test_sharded_lion*.py measure
against. "f32" arrays are float32; "bf16" arrays travel as uint16 bit patterns
(adam_ref's way), are widened exactly, m' narrows round-to-nearest-even and p
by adam_sr_ref.sr with r_p of element base + i. c1, c2, dk, nlr: double
arithmetic, cast once. A piece of q elements is q / 16 little-endian dwords,
element i in bits 2 * (i % 16) of dword i // 16, zero dwords to the next 16 bytes.
"""
import numpy as np

import adam_sr_ref
from oracle.oracle import bf16_bits_to_f32, f32_to_bf16_bits

QNAN = {"f32": np.uint32(0x7FC00000), "bf16": np.uint16(0x7FC0)}


def hyper(lr, betas=(0.9, 0.99), weight_decay=0.0):
    return {"lr": lr, "betas": betas, "weight_decay": weight_decay}


def sign_bytes(q):
    return -(-(q // 16 * 4) // 16) * 16


def _scalars(h):
    b1, b2 = (float(b) for b in h["betas"])
    lr, wd = float(h["lr"]), float(h.get("weight_decay", 0.0))
    f = np.float32
    return f(b1), f(1.0 - b1), f(b2), f(1.0 - b2), f(1.0 - lr * wd), f(-lr), wd != 0


def _wide(x, dt):
    return bf16_bits_to_f32(x) if dt == "bf16" else np.asarray(x, np.float32)


def _moments(g, m, dt, h, np_):
    """(c, m') as float32 arrays."""
    b1, c1, b2, c2, _, _, _ = _scalars(h)
    with np.errstate(all="ignore"):
        gw, mw = _wide(g, dt), _wide(m, dt)
        if np_ > 0:
            gw = gw / np.float32(np_)
        return (b1 * mw) + (c1 * gw), (b2 * mw) + (c2 * gw)


def _narrow_m(mn, dt):
    return f32_to_bf16_bits(mn) if dt == "bf16" else mn.astype(np.float32)


def signs(g, m, dt, h, np_=0):
    """(m', the piece's codes as uint32 dwords, padding included)."""
    c, mn = _moments(g, m, dt, h, np_)
    code = np.where(c > 0, 1, np.where(c < 0, 3, np.where(c == c, 0, 2))).astype(np.uint32)
    words = np.zeros(sign_bytes(code.size) // 4, np.uint32)
    shifted = code << (2 * (np.arange(code.size, dtype=np.uint32) % 16))
    np.bitwise_or.at(words, np.arange(code.size) // 16, shifted)
    return _narrow_m(mn, dt), words


def codes_of(words, n):
    i = np.arange(n)
    return (words[i // 16] >> (2 * (i % 16)).astype(np.uint32)) & np.uint32(3)


def apply(p, words, dt, h, base=0, stream=0, key=0):
    """p after the codes; bf16 draws r_p for elements base .. base + n."""
    _, _, _, _, dk, nlr, decay = _scalars(h)
    k = codes_of(np.asarray(words, np.uint32), len(p))
    with np.errstate(all="ignore"):
        x = _wide(p, dt)
        if decay:
            x = dk * x
        y = np.where(k == 1, x + nlr, np.where(k == 3, x - nlr, x)).astype(np.float32)
    if dt == "f32":
        # a choice of bits: code 0 without decay keeps p's, a signalling NaN's too
        keep = np.asarray(p, np.float32).view(np.uint32) if not decay else y.view(np.uint32)
        out = np.where(k == 0, keep, y.view(np.uint32))
        return np.where(k == 2, QNAN["f32"], out).astype(np.uint32).view(np.float32)
    rp, _ = adam_sr_ref.random_bits(base, len(p), stream, key)
    out = adam_sr_ref.sr(y, rp)
    if not decay:
        out = np.where(k == 0, np.asarray(p, np.uint16), out)
    return np.where(k == 2, QNAN["bf16"], out).astype(np.uint16)


def update(p, g, m, dt, h, np_=0, base=0, stream=0, key=0):
    """The dense update, (p', m'), from c itself: no code is formed."""
    _, _, _, _, dk, nlr, decay = _scalars(h)
    c, mn = _moments(g, m, dt, h, np_)
    bits = np.uint32 if dt == "f32" else np.uint16
    old = np.asarray(p).view(bits)
    with np.errstate(all="ignore"):
        x = _wide(p, dt)
        x = dk * x if decay else x
        y = np.where(c > 0, x + nlr, np.where(c < 0, x - nlr, x)).astype(np.float32)
    if dt == "f32":
        new = y.view(np.uint32)
    else:
        new = adam_sr_ref.sr(y, adam_sr_ref.random_bits(base, len(old), stream, key)[0])
    if not decay:
        new = np.where(c == 0, old, new)
    new = np.where(c != c, QNAN[dt], new).astype(bits)
    return (new.view(np.float32) if dt == "f32" else new), _narrow_m(mn, dt)
