"""The MXFP8 gradient wire (include/kungfu_amd.h) restated in
numpy; torch's CPU float8_e4m3fn cast is the element conversion. A piece is
q codes, q // 32 scale bytes and zeros up to the next 16 bytes."""
import numpy as np
import torch

BLOCK = 32
TORCH = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}


def piece_bytes(q):
    return (q + q // BLOCK + 15) // 16 * 16


def widen(t):
    """A torch tensor of any of the three dtypes as f32 numpy (exact)."""
    return t.detach().cpu().to(torch.float32).numpy()


def scales(x):
    """The scale byte of every block of the f32 array x."""
    mag = (np.ascontiguousarray(x, np.float32).view(np.uint32) & 0x7FFFFFFF).reshape(-1, BLOCK)
    mag = mag.max(axis=1).astype(np.int64)
    e = np.clip(((mag + 0x00200000) >> 23) - 135, -127, 127)
    return np.where(mag >= 0x7F800000, 255, e + 127).astype(np.uint8)


def pack(x):
    """One piece: the f32 array x (a multiple of 32 elements) packed."""
    x = np.ascontiguousarray(x, np.float32)
    q, s = x.size, scales(x)
    e = np.repeat(s.astype(np.int64) - 127, BLOCK)
    with np.errstate(all="ignore"):
        # exact wherever it matters: what f32 cannot hold is below 2^-126 and rounds to +-0
        y = np.ldexp(x.astype(np.float64), -e).astype(np.float32)
    y[np.repeat(s == 255, BLOCK)] = 0.0
    codes = torch.from_numpy(y).to(torch.float8_e4m3fn).view(torch.uint8).numpy()
    out = np.zeros(piece_bytes(q), np.uint8)
    out[:q], out[q:q + q // BLOCK] = codes, s
    return out


def unpack(piece, q=None):
    """The f32 values of one piece."""
    piece = np.asarray(piece, np.uint8)
    if q is None:
        q = next(n for n in range(0, piece.size + 1, BLOCK) if piece_bytes(n) == piece.size)
    v = torch.from_numpy(piece[:q].copy()).view(torch.float8_e4m3fn).to(torch.float32).numpy()
    s = np.repeat(piece[q:q + q // BLOCK], BLOCK)
    with np.errstate(all="ignore"):
        out = np.ldexp(v.astype(np.float64), s.astype(np.int64) - 127).astype(np.float32)
    out[s == 255] = np.float32(np.nan)
    return out


def fold(packed_pieces, np_, dtype):
    """The ranks' pieces of one shard added in f32 in rank order, one add at a
    time, / np_ (np_ > 0), narrowed once: a torch tensor of `dtype`."""
    s = None
    with np.errstate(all="ignore"):
        for piece in packed_pieces:
            v = unpack(piece)
            s = v if s is None else (s + v).astype(np.float32)
        if np_:
            s = (s / np.float32(np_)).astype(np.float32)
    if dtype != "bf16":
        return torch.from_numpy(s).to(TORCH[dtype])
    # f32_to_bf16's recipe (kf_reduce_kernels.hpp): RNE; a NaN keeps its sign and upper payload
    u = s.view(np.uint32).astype(np.uint64)
    h = np.where(np.isnan(s), (u >> 16) | 0x40, (u + 0x7FFF + ((u >> 16) & 1)) >> 16)
    return torch.from_numpy(h.astype(np.uint16).view(np.int16)).view(torch.bfloat16)


def roundtrip(t, world=1):
    """unpack(pack(.)) of every piece of the bucket t (its tail untouched), in
    t's dtype: what a gradient looks like after the wire at np = 1."""
    x = widen(t).copy()
    q = x.size // world
    for j in range(world):
        x[j * q:(j + 1) * q] = unpack(pack(x[j * q:(j + 1) * q]), q)
    return torch.from_numpy(x).to(t.dtype)
