"""Inputs for the IEEE-special tests of the fused epilogues (the /np average
and the SMA blend) and of the bf16 plain ops: pools of special values, fills
that carry them to every region of a launch, and the bit comparison.

No test functions: tests/test_epilogue_specials.py checks this module and the
oracle on the CPU, tests/test_epilogue_specials_gpu.py runs the kernels.

bf16 is carried as uint16 bit patterns, as in the other tests.
"""
import functools
import zlib

import numpy as np

import golden_io

DTS = ("f32", "f64", "f16", "bf16")
NP = {"f32": np.float32, "f64": np.float64, "f16": np.float16, "bf16": np.uint16}
# (exponent bits, mantissa bits)
FORMAT = {"f32": (8, 23), "f64": (11, 52), "f16": (5, 10), "bf16": (8, 7)}
UINT = {2: np.uint16, 4: np.uint32, 8: np.uint64}

# tile of the single-launch kernels and of the batch at k >= 2: 256 lanes x 4
# 16-byte vectors; the k = 1 batch takes 2 per lane
TILE_VECS = 1024
TILE_VECS_BATCH_K1 = 512


def itemsize(dt):
    return np.dtype(NP[dt]).itemsize


def pool_bits(dt):
    """The pool as Python ints, -0 first: for each magnitude (0, smallest
    subnormal, 3x smallest subnormal (with the former: ties when halved),
    largest subnormal, smallest normal, 1, largest finite, largest finite / 2,
    inf) the negative then the positive value, and one quiet NaN."""
    ebits, mbits = FORMAT[dt]
    sign = 1 << (ebits + mbits)
    inf = ((1 << ebits) - 1) << mbits
    fmax = inf - 1
    mags = [0, 1, 3, (1 << mbits) - 1, 1 << mbits, ((1 << (ebits - 1)) - 1) << mbits,
            fmax, fmax - (1 << mbits), inf]
    return [s | m for m in mags for s in (sign, 0)] + [inf | (1 << (mbits - 1))]


@functools.lru_cache(maxsize=None)
def pool(dt):
    """The pool as a read-only array of the dtype's storage type."""
    u = np.array(pool_bits(dt), dtype=UINT[itemsize(dt)])
    a = u.view(NP[dt])
    a.setflags(write=False)
    return a


def f32_to_bf16_bits(a):
    from oracle import oracle
    return oracle.f32_to_bf16_bits(a)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(UINT[a.itemsize])


def is_nan(dt, a):
    if dt == "bf16":
        return (np.asarray(a) & 0x7FFF) > 0x7F80
    return np.isnan(a)


def is_neg_zero(dt, a):
    ebits, mbits = FORMAT[dt]
    return bits(a) == (1 << (ebits + mbits))


# the last BACK elements of an input are laid out from the end, so that the
# scalar tail sees the same values as the scalar head
BACK = 8


@functools.lru_cache(maxsize=None)
def fill(dt, n, j):
    """Input j of a fold over n elements (read-only, cached).

    With m the position counted from the front (from the back for the last
    min(BACK, n // 2) elements) and L the pool's length (19, a prime):
      m odd:        a standard-normal value (ordinary rounding);
      m % 4 == 0:   pool[(q + j * (q // L)) % L], q = m // 4: input j cycles
                    the pool shifted by j once per period, so over L * L
                    periods inputs j and j' (j != j' mod L) show every ordered
                    pair of pool values;
      m % 4 == 2:   pool[(m // 4) % L], the same value in every input: x + x
                    (overflow at the largest finite, -0 + -0 = -0, ...).
    Element 0 and element n - 1 are -0 in every input."""
    p = pool(dt)
    L = p.size
    pos = np.arange(n)
    back = n - 1 - pos
    m = np.where(back < min(BACK, n // 2), back, pos)
    q = m // 4
    rng = np.random.default_rng(zlib.crc32(("epi" + dt).encode()) + j)
    normal = rng.standard_normal(n)
    if dt == "bf16":
        normal = f32_to_bf16_bits(normal.astype(np.float32))
    else:
        normal = normal.astype(NP[dt])
    pairs = p[(q + (j % L) * (q // L)) % L]
    diag = p[q % L]
    out = np.where(m % 2 == 1, normal, np.where(m % 4 == 0, pairs, diag)).astype(NP[dt])
    out.setflags(write=False)
    return out


def shapes(dt):
    """The element counts every case uses, E = elements per 16-byte vector:
    one element; less than a vector; a vector and one; exactly one tile; a
    tile, a ragged tile of 300 vectors and a tail of E - 1."""
    E = 16 // itemsize(dt)
    return (1, E - 1, E + 1, TILE_VECS * E, TILE_VECS * E + 300 * E + (E - 1))


# The SMA blend's placements, (name, offset of v, offset of the sum) in
# elements past a 16-byte boundary: aligned; both one element past alignment
# (a head of E - 1); v one past and the sum at another residue.
SMA_PLACEMENTS = (("aligned", 0, 0), ("co1", 1, 1), ("mixed", 1, 0))
SMA_BATCH_BUCKETS = 20  # 16 + 4: two launches of the batch kernel


def sma_batch_layout(dt):
    """Bucket b of the batched SMA blend: (n, placement). The five shapes in
    turn, each meeting every placement."""
    s = shapes(dt)
    return [(s[b % len(s)], SMA_PLACEMENTS[(b % len(s) + b // len(s)) % len(SMA_PLACEMENTS)])
            for b in range(SMA_BATCH_BUCKETS)]


def regions(ptr_residue_bytes, n, isz, tile_vecs=TILE_VECS):
    """Index sets of a launch over n elements whose OUTPUT pointer is
    ptr_residue_bytes past a 16-byte boundary, as the host plan and the kernel
    body split them: the scalar head (up to the output's 16-byte boundary),
    the full tiles of tile_vecs vectors, the ragged last tile, and the scalar
    tail after the last whole vector."""
    assert 0 <= ptr_residue_bytes < 16 and ptr_residue_bytes % isz == 0
    E = 16 // isz
    head = 0 if ptr_residue_bytes == 0 else (16 - ptr_residue_bytes) // isz
    head = min(head, n)
    nvec = (n - head) // E
    nfull = (nvec // tile_vecs) * tile_vecs
    vend = head + nvec * E
    return {"head": np.arange(0, head),
            "full": np.arange(head, head + nfull * E),
            "ragged": np.arange(head + nfull * E, vend),
            "tail": np.arange(vend, n)}


def mismatches(dt, got, want):
    """Indices at which got and want differ, with golden_io.same_bits_or_nan's
    meaning: NaNs are compared by position (an x86 reference and the GPU
    differ in the sign of a generated NaN), everything else by bits."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype
    ng, nw = is_nan(dt, got), is_nan(dt, want)
    bad = (ng != nw) | (~ng & ~nw & (bits(got) != bits(want)))
    return np.flatnonzero(bad)


def same(dt, got, want):
    if dt != "bf16":
        ok = golden_io.same_bits_or_nan(got, want)
        assert ok == (mismatches(dt, got, want).size == 0)
        return ok
    return mismatches(dt, got, want).size == 0


def describe(dt, got, want, reg=None, limit=4):
    """A short account of the mismatches for an assertion message: how many,
    in which regions, and the first few as (index, got bits, want bits)."""
    idx = mismatches(dt, got, want)
    if idx.size == 0:
        return ""
    where = ""
    if reg is not None:
        where = " in " + "+".join(k for k, v in reg.items() if np.intersect1d(v, idx).size)
    g, w = bits(got), bits(want)
    return "%d wrong%s: %s" % (idx.size, where,
                               ["%d: %#x != %#x" % (i, g[i], w[i]) for i in idx[:limit]])
