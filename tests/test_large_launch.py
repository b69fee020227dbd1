"""The shapes of tests/test_large_launch_gpu.py reach the schedules they are
there for. No output shows which schedule a launch ran (they give the same
bits by design), so this is the evidence: the thresholds and tile constants
are read out of the sources and pinned, and every GPU case's shape is checked
for the property the case exists for. A retune of a threshold fails here; move
the shapes in tests/large_launch.py with it."""
import os
import re

import numpy as np
import pytest

import large_launch as ll
from oracle.oracle import bf16_bits_to_f32, f32_to_bf16_bits

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "kungfu_amd", "csrc")


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _int(text, pattern):
    """The one integer `pattern` captures in `text` (C literals: 2048, 1 << 20)."""
    found = re.findall(pattern, text)
    assert len(found) == 1, (pattern, found)
    m = re.fullmatch(r"(\d+)\s*<<\s*(\d+)", found[0].strip())
    return int(m.group(1)) << int(m.group(2)) if m else int(found[0])


# ---- 1. the constants -----------------------------------------------------------

def test_reduce_constants_pinned():
    capi, hpp = _src("kf_capi.hip"), _src("kf_reduce_kernels.hpp")
    assert _int(capi, r"constexpr unsigned kSerialMinBlocks\s*=\s*(\d+);") == ll.SERIAL_MIN_BLOCKS == 2048
    assert _int(capi, r"#define KF_BATCH_SERIAL_MIN_BLOCKS (\d+)") == ll.BATCH_SERIAL_MIN_BLOCKS == 2048
    assert "kBatchSerialMinBlocks = KF_BATCH_SERIAL_MIN_BLOCKS;" in capi
    assert _int(capi, r"constexpr int kBlock\s*=\s*(\d+);") == ll.BLOCK == 256
    assert _int(capi, r"#define KF_BATCH_BLOCK (\d+)") == ll.BLOCK
    assert _int(capi, r"int unroll\s*=\s*(\d+);") == ll.UNROLL == 4
    assert _int(capi, r"int grid_cap = ([^;]+);  // blocks; grid-stride beyond") == ll.GRID_CAP == 1 << 20
    assert _int(capi, r"#define KF_BATCH_UNROLL (\d+)") == ll.UNROLL
    assert _int(capi, r"#define KF_BATCH_UNROLL_K1 (\d+)") == ll.BATCH_UNROLL_K1 == 2
    # the runtime-k fold (KC == 0) takes four vectors per lane like k <= 2
    assert "constexpr int U = KC == 0 || KC <= 2 ? 4 : KC <= 4 ? 2 : 1;" in capi
    # the flag: runtime k only, by the launch's block count
    assert "const int serial = KC == 0 && g >= kSerialMinBlocks ? 1 : 0;" in capi
    assert "a.serial       = KC == 0 && blocks >= kBatchSerialMinBlocks ? 1 : 0;" in capi
    # the SMA kernels' tile and the peers fold's one vector per lane
    assert capi.count("grid_for(p.nvec, ned, 4)") == 2
    assert "sma_kernel<T, C, kBlock, 4>" in capi and "sma_batch_kernel<T, C, kBlock, 4>" in capi
    assert "const unsigned g = grid_for(p.nvec, ned, 1);" in capi
    assert _int(hpp, r"constexpr int kBatchSeg\s*=\s*(\d+);") == ll.BATCH_SEG == 16
    assert _int(hpp, r"constexpr int kBatchSeg1\s*=\s*(\d+);") == ll.BATCH_SEG1 == 64
    # what the flag selects
    assert "if (LOADNT && serial) {" in hpp and "ld_vec_serial<W>(sj, v0 + u * BLOCK)" in hpp


def test_segnorm_constants_pinned():
    seg = _src("kf_segnorm.hip")
    assert _int(seg, r"constexpr int kNormBlock\s*=\s*(\d+);") == ll.BLOCK
    assert _int(seg, r"constexpr int kNormUnrollSq\s*=\s*(\d+);") == ll.NORM_UNROLL_SQ == 8
    assert _int(seg, r"constexpr int kNormUnrollVar\s*=\s*(\d+);") == ll.NORM_UNROLL_VAR == 4
    assert _int(seg, r"constexpr unsigned kSegMaxBlocks\s*=\s*(\d+);") == ll.SEG_MAX_BLOCKS == 2048
    assert _int(seg, r"constexpr int G\s*=\s*(\d+);") == ll.FOLD_G == 8
    assert "kBytesPerBlock = static_cast<size_t>(kNormBlock) * kNormUnrollSq * 16;" in seg
    assert ll.SEG_BYTES_PER_BLOCK == 32 << 10
    assert 'std::getenv("KUNGFU_AMD_SEGNORM_MAX_BLOCKS")' in seg
    # the total's LDS rounds are kNormBlock values each
    assert "for (int base = 0; base < nseg; base += kNormBlock) {" in seg


def test_sgd_constants_pinned():
    sgd = _src("kf_sgd.hip")
    assert _int(sgd, r"constexpr int kSgdSeg\s*=\s*(\d+);") == ll.SGD_SEG == 32
    assert _int(sgd, r"constexpr int kSgdBlock\s*=\s*(\d+);") == ll.BLOCK
    assert _int(sgd, r"#define KF_SGD_UNROLL (\d+)") == ll.SGD_UNROLL == 4
    # the grid rule is the shared planner's (tests/test_update_plan.py runs it)
    assert '#include "kf_update_batch.hpp"' in sgd and "plan_update_batch<SgdBatchArgs<C>>(" in sgd
    assert "const bool rows = a.nseg > 1 && widest * a.nseg <= 2 * blocks;" in \
        _src("kf_update_batch.hpp")


# ---- 2. the reduce family's shapes -------------------------------------------------

@pytest.mark.parametrize("dt", sorted({c[0] for c in ll.SINGLE_CASES}))
def test_single_launch_shapes(dt):
    e = ll.epv(dt)
    ks = sorted({k for d, k, _ in ll.SINGLE_CASES if d == dt})
    assert min(ks) >= 3  # runtime k: KC == 0
    for k in ks:
        rag = ll.Launch(ll.single_shape("S_rag", dt, 1), dt, k, out_residue=1)
        assert rag.nvec == 2048 * 1024 + 300 and rag.blocks == 2049 and rag.tiles == 2049
        assert rag.serial and rag.ragged and not rag.strides
        assert rag.head == e - 1 and rag.nedge == 2 * (e - 1)
        # inputs 2..k-1 are the serially loaded ones; at least one of them is
        # off the output's residue (E = 2 has two residues only)
        assert any(ll.input_offset(j, dt) != 1 for j in range(2, k)) or e == 2
        assert all(0 <= ll.input_offset(j, dt) < e for j in range(k))
    assert 2048 * 1024 * 16 == 32 << 20  # 32 MiB per input: the smallest serial launch


@pytest.mark.parametrize("dt,k", ll.THRESHOLD_CASES)
def test_threshold_shapes(dt, k):
    at = ll.Launch(ll.single_shape("S_at", dt, 0), dt, k)
    lo = ll.Launch(ll.single_shape("S_lo", dt, 0), dt, k)
    assert at.blocks == 2048 and at.serial and not at.ragged and at.nedge == 0
    assert lo.blocks == 2047 and not lo.serial and not lo.ragged and lo.nedge == 0
    assert at.nvec == 2048 * 1024 and lo.nvec == 2047 * 1024


@pytest.mark.parametrize("dt,k", ll.STRIDE_SERIAL_CASES)
def test_serial_and_stride_shape(dt, k):
    n = ll.single_shape("S_stride", dt, 1)
    s = ll.Launch(n, dt, k, out_residue=1, cap=ll.STRIDE_SERIAL_CAP)
    assert s.nvec == 2060 * 1024 + 300 and s.tiles == 2061 and s.blocks == 2048
    assert s.serial and s.strides and s.ragged
    # uncapped it would not stride
    assert not ll.Launch(n, dt, k, out_residue=1).strides


@pytest.mark.parametrize("dt,k", [("f32", 3), ("f32", 5), ("bf16", 8), ("u8", 5)])
def test_batch_shapes(dt, k):
    buckets = ll.batch_buckets(dt)
    assert len(buckets) == 20
    assert [b for b, (n, _) in enumerate(buckets) if n == 0] == [6]
    assert all(mis == (b % 2 == 1) for b, (_, mis) in enumerate(buckets))
    first, second = ll.batch_launches(buckets, dt, k)
    assert first.buckets == [b for b in range(17) if b != 6] and len(first.buckets) == ll.BATCH_SEG
    assert second.buckets == [17, 18, 19]
    # this launch's buckets total at least 2048 blocks and the next launch's fewer
    assert first.total >= ll.BATCH_SERIAL_MIN_BLOCKS and first.serial(k)
    assert second.total < ll.BATCH_SERIAL_MIN_BLOCKS and not second.serial(k)
    assert not first.rows and not second.rows  # a block finds its bucket in the table
    assert first.blocks[0] == 1901 and first.tiles[0] == 1901 and first.blocks[2] == 150
    assert not first.strides
    # no single bucket reaches the threshold: the flag is the launch's, not a bucket's
    assert max(first.blocks) < ll.BATCH_SERIAL_MIN_BLOCKS
    # the last four buckets are small
    assert all(n <= ll.count(dt, 2, 1) for n, _ in buckets[16:])
    # the poisoned layout keeps every bucket's residue
    offs, total = ll.flat_layout(buckets, dt)
    e = ll.epv(dt)
    for (n, mis), o in zip(buckets, offs):
        assert o % e == (1 if mis else 0)
    ends = [o + n for (n, _), o in zip(buckets, offs)]
    assert all(a < b for a, b in zip(ends, offs[1:])) and ends[-1] < total


def test_equal_batch_shape():
    buckets = ll.equal_buckets("f32")
    (launch,) = ll.batch_launches(buckets, "f32", 3)
    assert launch.rows and launch.grid == (129, 16)
    assert launch.total == 2064 >= ll.BATCH_SERIAL_MIN_BLOCKS and launch.serial(3)
    assert launch.grid[1] < 32  # below the XCD-by-XCD hand-out: the bucket is blockIdx.y
    _, nvec, nedge = ll.plan(buckets[0][0], "f32")
    assert nvec == 128 * 1024 + 5 and nedge == 3


@pytest.mark.parametrize("cap", ll.STRIDE_CAPS)
def test_grid_stride_shapes(cap):
    nvec = ll.STRIDE_NVEC
    assert ll.tiles_for(nvec) == 14 and nvec % ll.TILE == 300
    for dt, k in (("f32", 1), ("bf16", 2), ("f32", 3), ("u8", 8)):
        n = ll.count(dt, 13, 300, ll.epv(dt) - 1, ll.epv(dt) - 1)
        s = ll.Launch(n, dt, k, out_residue=1, cap=cap)
        assert s.blocks == cap and s.tiles == 14 and s.strides and not s.serial
        assert s.nedge <= ll.BLOCK  # the edges fit block 0
    # the peers fold: one vector per lane, 54 blocks uncapped
    assert ll.blocks_for(nvec, 6, unroll=1) == 54
    assert ll.blocks_for(nvec, 6, unroll=1, cap=cap) == cap
    assert ll.ceil_div(nvec, cap * ll.BLOCK) == {3: 18, 1: 54}[cap]
    # the batch: a table grid whose buckets stride, and a rows grid of `cap` a row
    for k in (1, 2, 3):
        (ragged,) = ll.batch_launches(ll.stride_buckets("f32"), "f32", k, cap)
        # (at cap 1 every bucket has one block: equal counts, so rows there too)
        assert ragged.rows == (cap == 1) and ragged.strides
        assert ragged.blocks == [cap, min(cap, 4 // (1 if k == 1 else 2)), cap, 1]
        (equal,) = ll.batch_launches(ll.stride_equal_buckets("f32"), "f32", k, cap)
        assert equal.rows and equal.grid == (cap, 4) and equal.strides
    assert ll.batch_launches(ll.stride_equal_buckets("f32"), "f32", 3, 3)[0].tiles == [7] * 4


# ---- 3. segmented norms ----------------------------------------------------------------

@pytest.mark.parametrize("dt", ["f32", "f16", "bf16", "f64"])
@pytest.mark.parametrize("cap", ll.SEG_STRIDE_CAPS)
def test_segnorm_stride_shapes(dt, cap):
    import test_monitor_gpu as mon
    counts = ll.seg_stride_counts(dt)
    e = ll.epv(dt)
    assert counts[:2] == [0, 1] and counts[3] * ll.ITEMSIZE[dt] == 3 * (32 << 10)
    offs, _ = mon.layout(counts, dt)
    res = [o % e for o in offs]
    assert res == [k % e for k in range(5)]
    blocks = [ll.seg_blocks(n, dt, cap) for n in counts]
    sq = [ll.seg_tiles(n, dt, r) for n, r in zip(counts, res)]
    assert blocks[:2] == [0, 1]
    assert blocks[2:] == [min(2, cap), min(3, cap), min(6, cap)]
    # SQ strides under the cap: more tiles than blocks (uncapped: one each)
    # (the tile + 1 element segment is one tile and an edge: uncapped, its
    # second block finds no tile)
    assert sq[2:] == [1, 3, 6]
    assert sq[4] > blocks[4] and (sq[3] > blocks[3] or cap == 3)
    assert [ll.seg_tiles(n, dt, r, var=True) for n, r in zip(counts, res)][2:] == [2, 6, 11]
    assert [ll.seg_blocks(n, dt) for n in counts][2:] == [2, 3, 6]
    # the last segment's last tile is ragged
    _, nvec, _ = ll.plan(counts[4], dt, res[4])
    assert nvec % ll.SQ_TILE != 0


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_wide_segment_shape(dt):
    import test_monitor_gpu as mon
    n = ll.wide_count(dt)
    assert n * ll.ITEMSIZE[dt] == 2100 * (32 << 10)  # 65.6 MiB
    counts = [ll.WIDE_BEFORE, n, ll.WIDE_AFTER]
    offs, _ = mon.layout(counts, dt)
    res = offs[1] % ll.epv(dt)
    assert ll.seg_blocks(ll.WIDE_BEFORE, dt) == 1  # the fold's b0 is not zero
    assert ll.seg_tiles(n, dt, res) == 2100 and ll.seg_tiles(n, dt, res, var=True) == 4200
    # default cap: 2048 blocks, 52 take a second SQ tile; the wide loop once per lane
    assert ll.seg_blocks(n, dt) == 2048 and 2100 - 2048 == 52
    wide, rem = ll.fold_lanes(2048)
    assert set(wide) == {1} and set(rem) == {0}
    # cap 4096: 2100 blocks; the wide loop, then the remainder loop in 52 lanes
    assert ll.seg_blocks(n, dt, ll.WIDE_CAP) == 2100
    wide, rem = ll.fold_lanes(2100)
    assert set(wide) == {1} and rem == [1] * 52 + [0] * 204
    # 1792 partials are the fewest that enter the wide loop at all (56 MiB)
    assert max(ll.fold_lanes(1792)[0]) == 0 and ll.fold_lanes(1793)[0][0] == 1
    assert 1792 * (32 << 10) == 56 << 20


def test_total_rounds_shape():
    assert ll.TOTAL_NSEG == 600 and ll.ceil_div(600, ll.BLOCK) == 3 and 600 - 2 * ll.BLOCK == 88


# ---- 4. the dyadic inputs are exact -------------------------------------------------------

def test_dyadic_inputs_are_exact():
    # SQ: x = m / 4, |m| <= 8: every value a bf16 (and f32) number, every
    # square a multiple of 2^-4 no larger than 4
    m = np.arange(-8, 9, dtype=np.int64)
    x = (m / 4.0).astype(np.float32)
    assert np.array_equal(x.astype(np.float64) * 4, m)
    assert np.array_equal(bf16_bits_to_f32(f32_to_bf16_bits(x)), x)
    assert np.array_equal((x.astype(np.float64) ** 2) * 16, m * m)
    # VAR (f32): a = j / 16, b = m / 4; fl(b * b) and fl(a - b * b) are exact
    j = np.arange(-32, 33, dtype=np.int64)[:, None]
    mb = np.arange(-4, 5, dtype=np.int64)[None, :]
    a, b = (j / 16.0).astype(np.float32), (mb / 4.0).astype(np.float32)
    assert np.array_equal(a.astype(np.float64) * 16, j) and np.array_equal(b.astype(np.float64) * 4, mb)
    p = (b * b).astype(np.float32)
    assert np.array_equal(p.astype(np.float64) * 16, mb * mb)
    d = (a - p).astype(np.float32)
    assert np.array_equal(d.astype(np.float64) * 16, j - mb * mb)
    assert np.array_equal((d.astype(np.float64) ** 2) * 256, (j - mb * mb) ** 2)
    # every partial sum is a multiple of 2^-8 below 2^53 * 2^-8: fp64 adds
    # them without rounding in any order
    most = max(ll.wide_count("f32"), ll.wide_count("bf16"))
    assert most * int(((j - mb * mb) ** 2).max()) < 2 ** 53
    assert most * 64 * 16 < 2 ** 53
    # the generators stay inside those ranges, and the integer sums restate them
    ms = ll.dyadic_sq(10007, 1)
    jv, mv = ll.dyadic_var(10007, 2)
    assert abs(ms.astype(int)).max() == 8 and abs(jv.astype(int)).max() == 32
    assert abs(mv.astype(int)).max() == 4
    assert ll.exact_sq_sum(ms) == float(np.sum((ms / 4.0) ** 2))
    assert ll.exact_var_sum(jv, mv) == float(np.sum(((jv / 16.0) - (mv / 4.0) ** 2) ** 2))


# ---- 5. the SGD update's grids ---------------------------------------------------------------

@pytest.mark.parametrize("dt", ["f32", "f16", "bf16", "f64"])
def test_sgd_shapes(dt):
    e = ll.epv(dt)
    counts = ll.sgd_counts(dt, ll.SGD_ROWS_TILES)
    rows, widest, blocks = ll.sgd_grid(counts, dt)
    # rows grid: widest * nseg <= 2 * blocks; 5 wide, multi-tile, unequal lengths
    assert rows and widest == 5 and blocks == [5, 4, 5, 3]
    assert widest * 4 <= 2 * sum(blocks)
    assert widest - blocks[3] == 2  # two blocks of the last row have no tile
    for n, t in zip(counts, ll.SGD_ROWS_TILES):
        assert (n // e) % ll.TILE == ll.TILE - 100 and 0 < n % e < e  # ragged last tile, a tail
        assert ll.ceil_div(n // e, ll.TILE) == t
    rows, widest, blocks = ll.sgd_grid(ll.sgd_counts(dt, ll.SGD_FLAT_TILES), dt)
    assert not rows and blocks == [5, 1, 1, 1]  # the control: the 1-D table


# ---- 6. the Adam-family updates' rows grids ------------------------------------------------

def test_update_planner_pinned():
    hpp = _src("kf_update_batch.hpp")
    assert "size_t nblk = (n / elts + tile - 1) / tile;  // one block per tile" in hpp
    assert "if (nblk < 1) nblk = 1;" in hpp
    assert "if (nblk > 0x400000u) nblk = 0x400000u;" in hpp and ll.PLAN_BLOCK_CAP == 0x400000
    assert "if (blocks + nblk > 0x7fffffu) {" in hpp and ll.PLAN_GRID_CAP == 0x7FFFFF
    assert "const bool rows = a.nseg > 1 && widest * a.nseg <= 2 * blocks;" in hpp
    assert "if (++a.nseg == NSEG) {" in hpp and "if (n == 0) continue;" in hpp
    # the restatement on the planner's edges
    assert ll.update_plan([0, 5, 0], 4, 1024, 24) == [(False, 1, [1])]
    assert ll.update_plan([4096 * 3] * 25, 4, 1024, 24) == [(True, 3, [3] * 24), (False, 3, [3])]
    assert ll.update_plan([4 * 1024 * (ll.PLAN_BLOCK_CAP + 7)], 4, 1024, 24)[0][2] == [ll.PLAN_BLOCK_CAP]
    big = 4 * 1024 * ll.PLAN_BLOCK_CAP
    assert [p[2] for p in ll.update_plan([big, big, 4096], 4, 1024, 24)] == \
        [[ll.PLAN_BLOCK_CAP], [ll.PLAN_BLOCK_CAP, 1]]
    assert ll.update_plan([4096 * 5, 4096, 4096, 4096], 4, 1024, 24) == [(False, 5, [5, 1, 1, 1])]
    # and it is the SGD restatement's rule
    for dt in ("f32", "f16", "bf16", "f64"):
        for tiles in (ll.SGD_ROWS_TILES, ll.SGD_FLAT_TILES):
            counts = ll.sgd_counts(dt, tiles)
            assert ll.update_counts(ll.epv(dt), ll.TILE, tiles) == counts
            (plan,) = ll.update_plan(counts, ll.epv(dt), ll.TILE, ll.SGD_SEG)
            assert plan == ll.sgd_grid(counts, dt)


def test_update_kernel_constants_pinned():
    """UPDATE_KERNELS' numbers against every source file."""
    adam, master = _src("kf_adam.hip"), _src("kf_adam_master.hip")
    sr, lamb = _src("kf_adam_sr.hip"), _src("kf_lamb.hip")
    k = ll.UPDATE_KERNELS
    for dt in ("f32", "bf16", "f64"):
        assert k["adam-" + dt] == ("kf_adam.hip", ll.epv(dt), ll.BLOCK * 4, 24)
    assert _int(adam, r"constexpr int kAdamSeg\s*=\s*(\d+);") == 24
    assert _int(adam, r"constexpr int kAdamBlock\s*=\s*(\d+);") == ll.BLOCK
    assert _int(adam, r"#define KF_ADAM_UNROLL (\d+)") == 4
    assert "counts, nb, SgdVec<T>::N, static_cast<size_t>(kAdamBlock) * kAdamUnroll," in adam
    for dt in ("bf16", "f16"):
        assert k["master-" + dt] == ("kf_adam_master.hip", 4, ll.BLOCK * 4, 32)
        assert k["lamb_master-" + dt] == ("kf_lamb.hip", 4, ll.BLOCK * 4, 32)
    assert _int(master, r"constexpr int kAdamMasterSeg\s*=\s*(\d+);") == 32
    assert _int(master, r"constexpr int kAdamMasterBlock\s*=\s*(\d+);") == ll.BLOCK
    assert _int(master, r"#define KF_ADAM_MASTER_ELTS (\d+)") == 4
    assert "#define KF_ADAM_MASTER_UNROLL (16 / KF_ADAM_MASTER_ELTS)" in master
    assert "counts, nb, kAdamMasterElts, static_cast<size_t>(kAdamMasterBlock) * kAdamMasterUnroll," \
        in master
    assert k["sr-bf16"] == ("kf_adam_sr.hip", 8, ll.BLOCK * 4, 32)
    assert _int(sr, r"constexpr int kAdamSrSeg\s*=\s*(\d+);") == 32
    assert _int(sr, r"constexpr int kAdamSrBlock\s*=\s*(\d+);") == ll.BLOCK
    assert _int(sr, r"#define KF_ADAM_SR_UNROLL (\d+)") == 4
    assert _int(sr, r"constexpr int kAdamSrElts\s*=\s*(\d+);") == 8
    assert "counts, nb, kAdamSrElts, static_cast<size_t>(kAdamSrBlock) * kAdamSrUnroll," in sr
    for dt in ("f32", "f64"):
        assert k["lamb-" + dt] == ("kf_lamb.hip", ll.epv(dt), ll.BLOCK * 4, 24)
    assert _int(lamb, r"constexpr int kLambSeg\s*=\s*(\d+);") == 24
    assert _int(lamb, r"constexpr int kLambMasterSeg\s*=\s*(\d+);") == 32
    assert _int(lamb, r"constexpr int kLambBlock\s*=\s*(\d+);") == ll.BLOCK
    assert _int(lamb, r"constexpr int kLambUnroll\s*=\s*(\d+);") == 4
    assert "counts, nb, SgdVec<C>::N, static_cast<size_t>(kLambBlock) * kLambUnroll," in lamb
    # every kernel's own tile loop, tail and idle blocks, over the shared lookup
    for src, n in ((adam, 2), (master, 2), (sr, 2), (lamb, 1)):
        assert src.count("batch_segment(a, blk, nblk)") == n
        assert "for (size_t t = blk; t < ntiles; t += nblk) {" in src and "if (blk == 0 && ti < n) {" in src


@pytest.mark.parametrize("kernel", sorted(ll.UPDATE_KERNELS))
def test_update_rows_shapes(kernel):
    _, unit, tile, nseg = ll.UPDATE_KERNELS[kernel]
    counts = ll.update_shape(kernel, "rows")
    (plan,) = ll.update_plan(counts, unit, tile, nseg)
    assert plan == (True, 5, [5, 4, 5, 3])
    for n, t in zip(counts, ll.ROWS_TILES):
        assert (n // unit) % tile == tile - 100 and 0 < n % unit < unit  # ragged last tile, a tail
        assert ll.ceil_div(n // unit, tile) == t
    assert ll.multi_tile_rows(counts, unit, tile, nseg) == (True, True)
    counts = ll.update_shape(kernel, "tail_only")
    (plan,) = ll.update_plan(counts, unit, tile, nseg)
    assert plan == (True, 2, [2, 2, 2, 1])
    # the short segment's row: `widest` blocks and no tile, block 0's tail alone
    assert counts[3] == unit - 1 and counts[3] // unit == 0 and plan[1] == 2
    assert ll.ceil_div(counts[3] // unit, tile) == 0 and (unit - 1 == 1) == kernel.endswith("f64")
    assert [ll.ceil_div(n // unit, tile) for n in counts[:3]] == [2, 2, 2]


def test_what_the_existing_kernel_tests_launch():
    """The record: which shapes of the kernel-level tests of the Adam family
    select a rows grid with a segment of more than one tile (first flag), and
    whether a row then has blocks past its last tile (second flag).

    The Adam, master-weight and gated tests reach rows with two-tile segments
    through _rows_segments (three equal segments: every block has a tile).
    Two launches do have rows with idle blocks: the first table of the bf16
    Adam sweep (tests/sweep16.py adam_sweep, ungated, np and step as swept)
    and the three cuts of test_sharded_adam_sr_gpu.test_split_invariance
    (ungated, np = 0). Neither LAMB moments test, no gated or master-weight
    launch and no launch of the stochastic-rounding kernel with np > 0 or a
    gate does."""
    import sweep16 as sw
    import test_sharded_adam_gpu as ag
    import test_sharded_adam_master_gpu as mg
    import test_sharded_adam_sr_gpu as srg
    import test_sharded_lamb_gpu as lg
    k = ll.UPDATE_KERNELS
    record = {}
    for dt in ("f32", "bf16", "f64"):
        _, unit, tile, nseg = k["adam-" + dt]
        rows_n = 2 * ag.BLOCK * ag.UNROLL * unit + 3
        record["adam-" + dt] = [ll.multi_tile_rows(c, unit, tile, nseg)
                                for c in (ag.SIZES + (1,) * ag.N_ONES, (rows_n,) * 3)]
    for dt in ("bf16", "f16"):
        _, unit, tile, nseg = k["master-" + dt]
        rows_n = 2 * mg.BLOCK * mg.UNROLL * mg.ELTS + 3
        record["master-" + dt] = [ll.multi_tile_rows(c, unit, tile, nseg)
                                  for c in (mg.SIZES + (1,) * mg.N_ONES, (rows_n,) * 3)]
    _, unit, tile, nseg = k["sr-bf16"]
    record["sr-bf16"] = [ll.multi_tile_rows(c, unit, tile, nseg) for c in
                         (srg.SIZES + (1,) * srg.N_ONES, (8 * 129, srg.TILE + 56, srg.SIZES[-1] - 8 * 129 - srg.TILE - 56),
                          (4096, 1011))]
    for name, ones in (("lamb-f32", lg.LAMB_SEG), ("lamb-f64", lg.LAMB_SEG),
                       ("lamb_master-bf16", lg.LAMB_MASTER_SEG)):
        _, unit, tile, nseg = k[name]
        record[name] = [ll.multi_tile_rows(lg.SIZES + (1,) * (ones + 8), unit, tile, nseg)]
    for name, kernel, s in (("adam-bf16", "adam", sw.adam_sweep(0, 1)),
                            ("master-bf16", "master", sw.master_sweep("bf16", 0, 1)),
                            ("sr-bf16", "adam_sr", sw.sr_sweep(0, 1)),
                            ("lamb_master-bf16", "lamb_master", sw.lamb_master_sweep("bf16", 0, 0.0))):
        unit, tile, nseg = sw.kernels()[kernel]
        assert (unit, tile, nseg) == k[name][1:]
        record[name].append(ll.multi_tile_rows(s.layout.n.tolist(), unit, tile, nseg))
    print(record)
    none, equal, idle = (False, False), (True, False), (True, True)
    assert record == {
        # (SIZES and one-element segments, _rows_segments[, the 16-bit sweep's layout])
        "adam-f32": [none, equal], "adam-f64": [none, equal],
        # the sweep's first table: 12 long segments and 12 tails, 10 x 24 <= 2 * 132
        "adam-bf16": [none, equal, idle],
        "master-bf16": [none, equal, none], "master-f16": [none, equal],
        # (SIZES, test_split_invariance's three cuts in one launch: 1, 2 and 2
        # blocks, test_high_bases, the sweep)
        "sr-bf16": [none, idle, none, none],
        "lamb-f32": [none], "lamb-f64": [none], "lamb_master-bf16": [none, none]}
