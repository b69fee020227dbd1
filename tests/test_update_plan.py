"""The launch planner the optimizer-update kernels share
(kungfu_amd/csrc/kf_update_batch.hpp plan_update_batch), on the CPU:
tests/c/test_update_plan.cpp includes the header's host part alone, is built
with the host compiler under AddressSanitizer and UBSan, and prints the
launches it is asked to make. The two grid limits (0x400000 blocks per
segment, 0x7fffff per launch) need billions of elements on a GPU; here the
counts are plain numbers."""
import os
import subprocess

import pytest

import large_launch as ll

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))

UNIT, TILE, NSEG = 4, 1024, 32   # elements per unit, units per tile, table size
CAP, LIMIT = 0x400000, 0x7fffff  # blocks per segment, blocks per launch


@pytest.fixture(scope="module")
def binary(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("plan") / "test_update_plan")
    subprocess.run(["g++", "-std=c++17", "-g", "-Wall", "-Wextra", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(ROOT, "kungfu_amd", "csrc"),
                    os.path.join(ROOT, "tests", "c", "test_update_plan.cpp"), "-o", out],
                   check=True)
    return out


def plan(binary, counts, fail_at=-1):
    """(rc, [(grid_x, grid_y, nseg, blk0, segment indices)]) of one call."""
    r = subprocess.run([binary, str(fail_at)] + [str(n) for n in counts],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and not r.stderr, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert lines[-1].startswith("rc ")
    launches = []
    for line in lines[:-1]:
        head, blk0, segs = (list(map(int, part.split())) for part in line.split("|"))
        launches.append((head[0], head[1], head[2], blk0, segs))
    return int(lines[-1].split()[1]), launches


def tiles(t):
    """Elements of a segment of t tiles, short by 100 units (large_launch's
    sgd_counts) and with a tail."""
    return (t * TILE - 100) * UNIT + 3


def agrees_with_sgd_grid(counts, launch):
    """large_launch.sgd_grid is the same rule for f32 (4 elements per unit,
    tiles of 256 * 4 units) and one table."""
    assert (UNIT, TILE, NSEG) == (ll.epv("f32"), ll.BLOCK * ll.SGD_UNROLL, ll.SGD_SEG)
    rows, widest, blocks = ll.sgd_grid(counts, "f32")
    gx, gy, nseg, blk0, _ = launch
    assert (gx, gy) == ((widest, len(blocks)) if rows else (sum(blocks), 1))
    assert nseg == len(blocks)
    assert blk0 == [sum(blocks[:i]) for i in range(len(blocks) + 1)]


@pytest.mark.parametrize("counts", [[], [0], [0, 0, 0]])
def test_nothing_to_do(binary, counts):
    assert plan(binary, counts) == (0, [])


def test_one_element(binary):
    rc, launches = plan(binary, [1])
    assert rc == 0 and launches == [(1, 1, 1, [0, 1], [0])]
    agrees_with_sgd_grid([1], launches[0])


def test_table_full(binary):
    rc, launches = plan(binary, [1] * 33)
    assert rc == 0 and len(launches) == 2
    assert launches[0] == (1, 32, 32, list(range(33)), list(range(32)))  # rows of one block
    assert launches[1] == (1, 1, 1, [0, 1], [32])
    agrees_with_sgd_grid([1] * 32, launches[0])


def test_flat_grid(binary):
    counts = [tiles(t) for t in ll.SGD_FLAT_TILES]
    assert counts == ll.sgd_counts("f32", ll.SGD_FLAT_TILES)
    rc, launches = plan(binary, counts)
    # rows would need 5 * 4 = 20 blocks, and 20 > 2 * 8
    assert rc == 0 and launches == [(8, 1, 4, [0, 5, 6, 7, 8], [0, 1, 2, 3])]
    agrees_with_sgd_grid(counts, launches[0])


def test_rows_grid(binary):
    counts = [tiles(t) for t in ll.SGD_ROWS_TILES]
    assert counts == ll.sgd_counts("f32", ll.SGD_ROWS_TILES)
    rc, launches = plan(binary, counts)
    # 5 * 4 = 20 <= 2 * 17
    assert rc == 0 and launches == [(5, 4, 4, [0, 5, 9, 14, 17], [0, 1, 2, 3])]
    agrees_with_sgd_grid(counts, launches[0])


def test_empty_segment_takes_no_slot(binary):
    counts = [tiles(2), 0, tiles(3)]
    rc, launches = plan(binary, counts)
    assert rc == 0 and launches == [(3, 2, 2, [0, 2, 5], [0, 2])]
    agrees_with_sgd_grid(counts, launches[0])


def test_segment_cap(binary):
    rc, launches = plan(binary, [(CAP + 5) * TILE * UNIT])
    assert rc == 0 and launches == [(CAP, 1, 1, [0, CAP], [0])]


def test_launch_limit_splits(binary):
    n = CAP * TILE * UNIT
    rc, launches = plan(binary, [n, n])
    assert 2 * CAP > LIMIT
    assert rc == 0 and launches == [(CAP, 1, 1, [0, CAP], [0]), (CAP, 1, 1, [0, CAP], [1])]


def test_launch_limit_is_inclusive(binary):
    rc, launches = plan(binary, [(CAP - 1) * TILE * UNIT, CAP * TILE * UNIT])
    assert CAP - 1 + CAP == LIMIT  # exactly the limit: not above it
    assert rc == 0 and launches == [(CAP, 2, 2, [0, CAP - 1, LIMIT], [0, 1])]


def test_first_error_stops(binary):
    rc, launches = plan(binary, [1] * 33, fail_at=0)
    assert rc == 7 and len(launches) == 1 and launches[0][:3] == (1, 32, 32)
    rc, launches = plan(binary, [1] * 33, fail_at=1)  # the final flush's status
    assert rc == 7 and len(launches) == 2
