"""The 1-bit gradient wire (include/kungfu_amd.h) restated in
numpy. A block is 64 elements; a piece is q // 8 bytes of sign bits (LSB
first), q // 64 f32 scales and zeros up to the next 16 bytes."""
import numpy as np

import mx8_ref

BLOCK = 64
NAN = np.uint32(0x7FC00000)  # the scale word of a block that is not finite
widen, TORCH = mx8_ref.widen, mx8_ref.TORCH


def piece_bytes(q):
    return (q // 8 + q // 16 + 15) // 16 * 16


def block_sums(s):
    """sum |s| per block as a pairwise tree of adjacent elements, in f32"""
    a = np.abs(np.ascontiguousarray(s, np.float32)).reshape(-1, BLOCK)
    with np.errstate(all="ignore"):
        while a.shape[1] > 1:
            a = a[:, 0::2] + a[:, 1::2]
    return a[:, 0]


def pack_ef(g, r):
    """One piece: the f32 gradients g and residuals r (a multiple of 64
    elements) -> (the piece's bytes, the new residuals)."""
    with np.errstate(all="ignore"):
        s = np.ascontiguousarray(g, np.float32) + np.ascontiguousarray(r, np.float32)
        a = block_sums(s)
        ok = np.isfinite(a)
        scale = np.where(ok, (a * np.float32(2.0 ** -6)).view(np.uint32), NAN).astype(np.uint32)
        sign = s.view(np.uint32) >> 31
        d = (np.repeat(scale, BLOCK) | (sign << 31)).astype(np.uint32).view(np.float32)
        res = np.where(np.repeat(ok, BLOCK), s - d, np.float32(0)).astype(np.float32)
    sign[~np.repeat(ok, BLOCK)] = 0
    q = s.size
    out = np.zeros(piece_bytes(q), np.uint8)
    out[:q // 8] = np.packbits(sign.astype(np.uint8), bitorder="little")
    out[q // 8:q // 8 + q // 16] = scale.view(np.uint8)
    return out, res


def unpack(piece, q):
    """The f32 values of one piece of q elements (3 and 4 blocks are both 48
    bytes: the length does not tell)."""
    piece = np.asarray(piece, np.uint8)
    sign = np.unpackbits(piece[:q // 8], bitorder="little").astype(np.uint32)
    scale = np.repeat(piece[q // 8:q // 8 + q // 16].copy().view(np.uint32), BLOCK)
    ok = (scale & 0x7F800000) != 0x7F800000
    return np.where(ok, scale | (sign << 31), NAN).astype(np.uint32).view(np.float32)


def fold(pieces, np_, kind, q):
    """mx8_ref.fold over 1-bit pieces: added in f32 in rank order, / np_
    (np_ > 0), narrowed once (its divide and narrowing, restated)."""
    import torch
    s = None
    with np.errstate(all="ignore"):
        for piece in pieces:
            v = unpack(piece, q)
            s = v if s is None else (s + v).astype(np.float32)
        if np_:
            s = (s / np.float32(np_)).astype(np.float32)
    if kind != "bf16":
        return torch.from_numpy(s).to(TORCH[kind])
    u = s.view(np.uint32).astype(np.uint64)
    h = np.where(np.isnan(s), (u >> 16) | 0x40, (u + 0x7FFF + ((u >> 16) & 1)) >> 16)
    return torch.from_numpy(h.astype(np.uint16).view(np.int16)).view(torch.bfloat16)
