"""Shapes for the kernel schedules that only large launches select
(tests/test_large_launch.py pins and checks them on the CPU,
tests/test_large_launch_gpu.py runs them).

The host code picks a kernel's schedule from the size of the launch: the
runtime-k fold's one-vector-in-flight loads from 2048 blocks, grid-stride past
a block cap, the segmented norm's fold with eight loads in flight past 1792
partials, the SGD update as a rows grid for segments of about equal length.
The serial and the batched schedules give the same bits by design, so no
output shows which one ran: a shape reaches a path because of the numbers
below. They restate the host code's launch arithmetic (kf_capi.hip grid_for /
make_plan / launch_batch_kc, kf_segnorm.hip kf_segnorm_create, kf_sgd.hip
launch_sgd); tests/test_large_launch.py reads the same constants out of the
sources, so a retune fails there and does not silently empty the GPU tests.

The Adam, master-weight, gated, stochastic-rounding and LAMB moments kernels
share the SGD update's planner (kf_update_batch.hpp plan_update_batch), which
update_plan restates for one table; their rows shapes are ROWS_TILES and
ROWS_WITH_TAIL_ONLY (update_shape).
"""
import numpy as np

# ---- the constants the shapes rest on (pinned by tests/test_large_launch.py) --
BLOCK = 256               # kBlock, KF_BATCH_BLOCK, kNormBlock, kSgdBlock
UNROLL = 4                # Geometry::unroll, KF_BATCH_UNROLL, the SMA kernels
BATCH_UNROLL_K1 = 2       # KF_BATCH_UNROLL_K1
SERIAL_MIN_BLOCKS = 2048  # kSerialMinBlocks
BATCH_SERIAL_MIN_BLOCKS = 2048  # KF_BATCH_SERIAL_MIN_BLOCKS
BATCH_SEG = 16            # kBatchSeg
BATCH_SEG1 = 64           # kBatchSeg1
GRID_CAP = 1 << 20        # Geometry::grid_cap
NORM_UNROLL_SQ = 8        # kNormUnrollSq
NORM_UNROLL_VAR = 4       # kNormUnrollVar
SEG_MAX_BLOCKS = 2048     # kSegMaxBlocks
FOLD_G = 8                # segnorm_fold_kernel's G
SGD_SEG = 32              # kSgdSeg
SGD_UNROLL = 4            # KF_SGD_UNROLL

TILE = BLOCK * UNROLL                       # 16-B vectors per reduce / SMA / SGD tile
SQ_TILE = BLOCK * NORM_UNROLL_SQ            # vectors per SQ tile (32 KiB)
VAR_TILE = BLOCK * NORM_UNROLL_VAR          # vectors per VAR tile
SEG_BYTES_PER_BLOCK = SQ_TILE * 16          # kBytesPerBlock

ITEMSIZE = {"u8": 1, "i8": 1, "f16": 2, "bf16": 2, "u16": 2, "f32": 4, "i32": 4, "f64": 8}


def epv(dt):
    """Elements per 16-B vector."""
    return 16 // ITEMSIZE[dt]


def ceil_div(a, b):
    return -(-a // b)


# ---- reduce / SMA: kf_capi.hip make_plan and grid_for -------------------------

def plan(n, dt, out_residue=0):
    """(head, nvec, nedge) of a bucket of n elements whose OUTPUT starts
    out_residue elements past a 16-B boundary (make_plan)."""
    e = epv(dt)
    head = 0 if out_residue % e == 0 else e - out_residue % e
    head = min(head, n)
    nvec = (n - head) // e
    return head, nvec, head + (n - head - nvec * e)


def blocks_for(nvec, nedge=0, unroll=UNROLL, cap=GRID_CAP):
    """grid_for: one block per tile up to the cap, enough blocks for the
    scalar edges, at least one."""
    return max(min(ceil_div(nvec, BLOCK * unroll), cap), ceil_div(nedge, BLOCK), 1)


def tiles_for(nvec, unroll=UNROLL):
    return ceil_div(nvec, BLOCK * unroll)


def count(dt, tiles=0, vecs=0, head=0, tail=0):
    """Elements of a bucket of `tiles` full tiles and `vecs` more vectors with
    `head` scalars before and `tail` scalars after the vector body."""
    e = epv(dt)
    assert head < e and tail < e
    return head + (tiles * TILE + vecs) * e + tail


class Launch:
    """One reduce_kernel launch as the host shapes it."""

    def __init__(self, n, dt, k, out_residue=0, cap=GRID_CAP):
        self.n, self.dt, self.k = n, dt, k
        self.head, self.nvec, self.nedge = plan(n, dt, out_residue)
        self.blocks = blocks_for(self.nvec, self.nedge, UNROLL, cap)
        self.tiles = tiles_for(self.nvec)
        self.serial = k >= 3 and self.blocks >= SERIAL_MIN_BLOCKS
        self.strides = self.tiles > self.blocks
        self.ragged = self.nvec % TILE != 0


def single_shape(name, dt, residue):
    """The single-launch shapes: S_lo (2047 blocks, the control), S_at (2048,
    all tiles full), S_rag (2049, last tile ragged). With residue != 0 the
    output starts that many elements past a 16-B boundary, which gives
    E - residue head scalars; the same number of tail scalars follows."""
    e = epv(dt)
    edge = 0 if residue % e == 0 else e - residue % e
    tiles, vecs = {"S_lo": (2047, 0), "S_at": (2048, 0), "S_rag": (2048, 300),
                   "S_stride": (2060, 300)}[name]
    return count(dt, tiles, vecs, edge, edge)


def input_offset(j, dt):
    """Input j starts this many elements past a 16-B boundary (the layout of
    test_gpu_parity.test_k_fold_inputs_at_other_residues)."""
    return (3 * j + 1) % epv(dt)


# single-launch cases: (dtype, k, op or "avg")
SINGLE_CASES = [
    ("f32", 3, "sum"), ("f32", 8, "sum"), ("f32", 3, "min"), ("f32", 3, "prod"),
    ("f32", 4, "avg"), ("f32", 5, "avg"),
    ("bf16", 4, "sum"), ("bf16", 4, "max"), ("bf16", 4, "avg"), ("bf16", 16, "sum"),
    ("f16", 3, "sum"), ("f16", 3, "avg"),
    ("u8", 6, "sum"), ("u8", 6, "min"), ("u8", 6, "max"), ("u8", 6, "prod"),
    ("i8", 3, "min"), ("i8", 3, "max"),
    ("i32", 3, "sum"),
    ("f64", 3, "sum"), ("f64", 3, "avg"),
]
THRESHOLD_CASES = [("f32", 3), ("bf16", 4)]   # S_at and S_lo, SUM, co-aligned
STRIDE_SERIAL_CAP = 2048
STRIDE_SERIAL_CASES = [("f32", 3), ("bf16", 4)]

# the vector body the grid-stride calls share: 14 tiles, the last ragged
STRIDE_NVEC = 13 * TILE + 300
STRIDE_CAPS = (3, 1)


# ---- the batched launch: kf_capi.hip launch_batch_kc ---------------------------

def batch_buckets(dt):
    """[(count, misaligned)] of the twenty ragged buckets. Buckets 0..16 hold
    sixteen non-empty buckets and an empty one: the first launch, whose blocks
    total at least 2048. Buckets 17..19 are the second launch. The last four
    buckets (16..19) are small. Every other bucket starts one element past a
    16-B boundary (all its pointers: one residue, so it stays in the batch)."""
    e = epv(dt)
    c = lambda *a, **kw: count(dt, *a, **kw)  # noqa: E731
    counts = [
        c(1900, 300, tail=e - 1),      # 0: the bulk of the launch
        1,                             # 1
        c(150),                        # 2
        7,                             # 3
        c(1),                          # 4: one exact tile
        c(1, 1),                       # 5: a tile and one vector
        0,                             # 6: empty, takes no slot
        c(3, 5, tail=min(3, e - 1)),   # 7
        c(2),                          # 8
        c(0, 1),                       # 9: one vector
        33,                            # 10
        c(0, TILE - 1),                # 11: one vector short of a tile
        4099,                          # 12
        c(7, 255, tail=1),             # 13
        c(0, 0, tail=e - 1),           # 14: tail only
        c(1, 2),                       # 15
        c(0, 3, tail=1),               # 16
        c(2, 1),                       # 17
        5,                             # 18
        c(1, 0, tail=e - 1),           # 19
    ]
    return [(n, b % 2 == 1) for b, n in enumerate(counts)]


def equal_buckets(dt):
    """Sixteen equal buckets of 128 tiles + 5 vectors + a tail: 129 blocks
    each on a rows grid."""
    e = epv(dt)
    return [(count(dt, 128, 5, tail=min(3, e - 1)), False)] * 16


def stride_buckets(dt):
    """The batch under a lowered cap: 14 tiles (the last ragged), 2 tiles,
    3 tiles + a ragged one, a tail alone."""
    e = epv(dt)
    counts = [count(dt, 13, 300, tail=e - 1), count(dt, 2), count(dt, 3, 77, tail=1),
              count(dt, 0, 0, tail=e - 1)]
    return [(n, b % 2 == 1) for b, n in enumerate(counts)]


def stride_equal_buckets(dt):
    """Four equal buckets of 7 tiles: a rows grid, at most `cap` blocks a row."""
    return [(count(dt, 7), False)] * 4


class BatchLaunch:
    def __init__(self):
        self.buckets, self.blocks, self.tiles = [], [], []

    @property
    def total(self):
        return sum(self.blocks)

    @property
    def rows(self):
        return len(self.blocks) > 1 and len(set(self.blocks)) == 1

    @property
    def grid(self):
        return (self.blocks[0], len(self.blocks)) if self.rows else (self.total, 1)

    def serial(self, k):
        return k >= 3 and self.total >= BATCH_SERIAL_MIN_BLOCKS

    @property
    def strides(self):
        return any(t > b for t, b in zip(self.tiles, self.blocks))


def batch_launches(buckets, dt, k, cap=GRID_CAP):
    """The launches kf_bucket_reduce_batch makes of [(count, misaligned)]:
    empty buckets take no slot, a launch holds kBatchSeg buckets (kBatchSeg1
    at k = 1), a bucket has one block per tile up to the cap."""
    unroll = BATCH_UNROLL_K1 if k == 1 else UNROLL
    per = BATCH_SEG1 if k == 1 else BATCH_SEG
    out, cur = [], BatchLaunch()
    for b, (n, mis) in enumerate(buckets):
        if n == 0:
            continue
        _, nvec, nedge = plan(n, dt, 1 if mis else 0)
        cur.buckets.append(b)
        cur.blocks.append(blocks_for(nvec, nedge, unroll, cap))
        cur.tiles.append(tiles_for(nvec, unroll))
        if len(cur.buckets) == per:
            out.append(cur)
            cur = BatchLaunch()
    if cur.buckets:
        out.append(cur)
    return out


def flat_layout(buckets, dt, gap=None):
    """Element offsets of [(count, misaligned)] in one flat buffer that starts
    on a 16-B boundary: every bucket starts on one, or one element past it,
    with at least `gap` (default: one vector) poisoned elements before the
    first bucket, between neighbours and after the last. Returns (offsets,
    total)."""
    e = epv(dt)
    gap = e if gap is None else gap
    offs, cur = [], gap
    for n, mis in buckets:
        cur += (-cur) % e + (1 if mis else 0)
        offs.append(cur)
        cur += n + gap
    return offs, cur + (-cur) % e + e


# ---- segmented norms: kf_segnorm.hip kf_segnorm_create ---------------------------

def seg_blocks(n, dt, cap=SEG_MAX_BLOCKS):
    """Blocks of a segment of n elements: one per 32 KiB of `a`, up to the cap."""
    return min(ceil_div(n * ITEMSIZE[dt], SEG_BYTES_PER_BLOCK), cap)


def seg_tiles(n, dt, residue, var=False):
    """Tiles the segment's blocks share; `residue`: elements past a 16-B
    boundary at which it starts."""
    _, nvec, _ = plan(n, dt, residue)
    return ceil_div(nvec, VAR_TILE if var else SQ_TILE)


def seg_stride_counts(dt):
    """Segments for the SQ stride under a lowered cap: empty, one element, one
    SQ tile + 1 element, exactly 3 tiles, 5 tiles + 300 vectors + edges."""
    e = epv(dt)
    return [0, 1, SQ_TILE * e + 1, 3 * SQ_TILE * e, (5 * SQ_TILE + 300) * e + 2 * (e - 1)]


SEG_STRIDE_CAPS = (1, 3)
WIDE_TILES = 2100          # 65.6 MiB: past the fold's 1792 partials and the default cap
WIDE_CAP = 4096            # KUNGFU_AMD_SEGNORM_MAX_BLOCKS for the second plan
WIDE_BEFORE, WIDE_AFTER = 1000, 4099   # the random neighbours


def wide_count(dt):
    return WIDE_TILES * SQ_TILE * epv(dt)


def fold_lanes(partials):
    """Per lane of segnorm_fold_kernel, for a segment of `partials` blocks:
    (rounds of the eight-loads-at-a-time loop, loads of the one-at-a-time
    loop after it), two lists of 256."""
    wide, rem = [], []
    for lane in range(BLOCK):
        i, w, r = lane, 0, 0
        while i + (FOLD_G - 1) * BLOCK < partials:
            i += FOLD_G * BLOCK
            w += 1
        while i < partials:
            i += BLOCK
            r += 1
        wide.append(w)
        rem.append(r)
    return wide, rem


def dyadic_sq(n, seed):
    """m with |m| <= 8: the SQ data is m / 4."""
    return np.random.default_rng(seed).integers(-8, 9, n, dtype=np.int8)


def dyadic_var(n, seed):
    """(j, m) with |j| <= 32 and |m| <= 4: a = j / 16, b = m / 4, so
    a - b * b = (j - m * m) / 16."""
    rng = np.random.default_rng(seed)
    return rng.integers(-32, 33, n, dtype=np.int8), rng.integers(-4, 5, n, dtype=np.int8)


def exact_sq_sum(m):
    """sum (m / 4)^2, from the integer sum."""
    m = m.astype(np.int64)
    return float(int(np.dot(m, m))) / 16.0


def exact_var_sum(j, m):
    """sum ((j - m * m) / 16)^2, from the integer sum."""
    d = j.astype(np.int64) - m.astype(np.int64) ** 2
    return float(int(np.dot(d, d))) / 256.0


TOTAL_NSEG = 600           # three LDS rounds of segnorm_total_kernel, the last with 88


# ---- the SGD update: kf_sgd.hip launch_sgd ------------------------------------------

SGD_ROWS_TILES = (5, 4, 5, 3)
SGD_FLAT_TILES = (5, 1, 1, 1)


def sgd_counts(dt, tiles):
    """Segments of `tiles` tiles, each short by 100 vectors, with a scalar
    tail of 3 elements (1 for f64, whose vector holds two)."""
    e = epv(dt)
    return [(t * TILE - 100) * e + min(3, e - 1) for t in tiles]


def sgd_grid(counts, dt):
    """(rows, widest, blocks per segment) of one kf_sgd_update_batch launch."""
    e = epv(dt)
    blocks = [max(ceil_div(n // e, BLOCK * SGD_UNROLL), 1) for n in counts if n]
    assert len(blocks) <= SGD_SEG
    widest, total = max(blocks), sum(blocks)
    rows = len(blocks) > 1 and widest * len(blocks) <= 2 * total
    return rows, widest, blocks


# ---- the Adam-family updates: kf_update_batch.hpp plan_update_batch ----------------------

PLAN_BLOCK_CAP = 0x400000    # blocks of one segment; beyond, they stride over the tiles
PLAN_GRID_CAP = 0x7FFFFF     # blocks of one launch

ROWS_TILES = SGD_ROWS_TILES


def update_plan(counts, unit, tile_units, nseg):
    """The launches plan_update_batch makes of one table of `counts`:
    [(rows, widest, [blocks per segment])]. A unit is `unit` elements, a tile
    `tile_units` units; one block per tile, at least one (a tail alone), at
    most PLAN_BLOCK_CAP; rows when nseg > 1 and widest * nseg <= 2 * blocks; a
    launch is flushed at `nseg` segments and before PLAN_GRID_CAP blocks.
    Empty segments take no entry."""
    out, cur = [], []

    def flush():
        if cur:
            widest, total = max(cur), sum(cur)
            out.append((len(cur) > 1 and widest * len(cur) <= 2 * total, widest, list(cur)))
            del cur[:]
    for n in counts:
        if n == 0:
            continue
        nblk = min(max(ceil_div(n // unit, tile_units), 1), PLAN_BLOCK_CAP)
        if sum(cur) + nblk > PLAN_GRID_CAP:
            flush()
        cur.append(nblk)
        if len(cur) == nseg:
            flush()
    flush()
    return out


def multi_tile_rows(counts, unit, tile_units, nseg):
    """Does a launch of these counts run a rows grid with a segment of more
    than one tile? (and, if so, does a row have blocks past its last tile)"""
    hit = [p for p in update_plan(counts, unit, tile_units, nseg) if p[0] and p[1] > 1]
    return bool(hit), any(min(p[2]) < p[1] for p in hit)


def update_counts(unit, tile_units, tiles):
    """Segments of `tiles` tiles, each short by 100 units, with a scalar tail
    of 3 elements (unit - 1 where a unit holds fewer)."""
    return [(t * tile_units - 100) * unit + min(3, unit - 1) for t in tiles]


def tail_only_counts(unit, tile_units):
    """ROWS_WITH_TAIL_ONLY: three segments of 2 tiles and one of unit - 1
    elements, a row whose only work is block 0's scalar tail."""
    return update_counts(unit, tile_units, (2, 2, 2)) + [unit - 1]


# kernel -> (source file, elements per unit, units per tile, segments per
# launch); the numbers are pinned to the sources by tests/test_large_launch.py
UPDATE_KERNELS = {
    "adam-f32": ("kf_adam.hip", 4, 1024, 24), "adam-bf16": ("kf_adam.hip", 8, 1024, 24),
    "adam-f64": ("kf_adam.hip", 2, 1024, 24),
    "master-bf16": ("kf_adam_master.hip", 4, 1024, 32), "master-f16": ("kf_adam_master.hip", 4, 1024, 32),
    "sr-bf16": ("kf_adam_sr.hip", 8, 1024, 32),
    "lamb-f32": ("kf_lamb.hip", 4, 1024, 24), "lamb-f64": ("kf_lamb.hip", 2, 1024, 24),
    "lamb_master-bf16": ("kf_lamb.hip", 4, 1024, 32), "lamb_master-f16": ("kf_lamb.hip", 4, 1024, 32),
}
UPDATE_SHAPES = ("rows", "tail_only")


def update_shape(kernel, shape):
    _, unit, tile, _ = UPDATE_KERNELS[kernel]
    return update_counts(unit, tile, ROWS_TILES) if shape == "rows" else tail_only_counts(unit, tile)
