"""The top-k gradient wire (include/kungfu_amd.h) restated in numpy: per block of 64
elements k f32 values in selection order, then as many index bytes, then zeros up to the next 16 bytes."""
import numpy as np

import mx8_ref

BLOCK, KS = 64, (1, 2, 4, 8)
widen, TORCH = mx8_ref.widen, mx8_ref.TORCH


def piece_bytes(q, k):
    return (5 * k * (q // BLOCK) + 15) // 16 * 16


def pack_ef(g, r, k):
    """One piece: f32 gradients g and residuals r (whole blocks) -> (its bytes, the new residuals)"""
    with np.errstate(all="ignore"):
        s = np.ascontiguousarray(g, np.float32) + np.ascontiguousarray(r, np.float32)
    bits = s.view(np.uint32).reshape(-1, BLOCK)
    key = (bits & 0x7FFFFFFF).astype(np.int64)
    order = np.argsort(-key, axis=1, kind="stable")[:, :k]  # the largest key, then the smallest index
    taken = np.zeros(bits.shape, bool)
    np.put_along_axis(taken, order, True, axis=1)
    res = np.where(taken | ~np.isfinite(s.reshape(-1, BLOCK)), np.uint32(0), bits)
    n = order.size
    out = np.zeros(piece_bytes(s.size, k), np.uint8)
    out[:4 * n] = np.take_along_axis(bits, order, axis=1).ravel().view(np.uint8)
    out[4 * n:5 * n] = order.ravel().astype(np.uint8)
    return out, res.ravel().view(np.float32)


def pack_pieces(g, r, q, world, k):  # a bucket's pieces; r, its residuals, is updated in place
    cuts = [slice(j * q, (j + 1) * q) for j in range(world)]
    done = [pack_ef(g[c], r[c], k) for c in cuts]
    for c, (_, res) in zip(cuts, done):
        r[c] = res
    return [p for p, _ in done]


def fold(pieces, np_, kind, q, k):
    """Added in f32 in rank order into zeros; sign1_ref.fold's divide and narrowing."""
    import torch
    n = q // BLOCK * k
    s = np.zeros(q, np.float32)
    at = np.repeat(np.arange(q // BLOCK) * BLOCK, k)
    with np.errstate(all="ignore"):
        for piece in pieces:
            piece = np.asarray(piece, np.uint8)
            np.add.at(s, at + (piece[4 * n:5 * n] & 63), piece[:4 * n].copy().view(np.float32))
        if np_:
            s = (s / np.float32(np_)).astype(np.float32)
    if kind != "bf16":
        return torch.from_numpy(s).to(TORCH[kind])
    u = s.view(np.uint32).astype(np.uint64)
    h = np.where(np.isnan(s), (u >> 16) | 0x40, (u + 0x7FFF + ((u >> 16) & 1)) >> 16)
    return torch.from_numpy(h.astype(np.uint16).view(np.int16)).view(torch.bfloat16)
