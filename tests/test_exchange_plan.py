"""The arithmetic of the exchange's batch schedule
(kungfu_amd/csrc/kf_exchange_plan.hpp plan_workspace and split_groups), on the
CPU: tests/c/test_exchange_plan.cpp includes the header alone, is built with
the host compiler under AddressSanitizer and UBSan, and prints the workspace
layout and the pipeline's groups it is asked for. The expected values are the
two rules restated here, and cases worked out by hand."""
import os
import subprocess

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
STEP = 256  # every workspace region starts at a multiple of this many bytes


@pytest.fixture(scope="module")
def binary(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("plan") / "test_exchange_plan")
    subprocess.run(["g++", "-std=c++17", "-g", "-Wall", "-Wextra", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "kungfu_amd", "csrc"),
                    os.path.join(ROOT, "tests", "c", "test_exchange_plan.cpp"), "-o", out],
                   check=True)
    return out


def plan(binary, counts, world=4, sz=4, a2a=False, G=1):
    """((bytes, shard offsets, tail offsets), cuts) of one call."""
    r = subprocess.run([binary, str(world), str(sz), str(int(a2a)), str(G)] +
                       [str(n) for n in counts], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and not r.stderr, r.stdout + r.stderr
    ws, groups = r.stdout.splitlines()
    head, shards, tails = (list(map(int, part.split())) for part in ws[3:].split("|"))
    assert ws.startswith("ws ") and groups.startswith("groups ") and len(head) == 1
    return (head[0], shards, tails), list(map(int, groups.split()[1:]))


def want_workspace(counts, world, sz, a2a):
    """The layout rule: per bucket the received shards (all-to-all only), then
    the gathered tails, each region at the next 256-byte step."""
    need, shards, tails = 0, [], []
    for n in counts:
        q, t = divmod(n, world)
        shards.append(need if a2a and q else 0)
        need += -(-q * world * sz // STEP) * STEP if a2a and q else 0
        tails.append(need if t else 0)
        need += -(-t * world * sz // STEP) * STEP if t else 0
    return need, shards, tails


def want_groups(counts, G):
    """The split rule: a group closes at the first bucket that brings the
    running count to its share, while every later group can still get one."""
    nb = len(counts)
    cuts, acc, G = [0], 0, min(G, nb)
    for b, n in enumerate(counts):
        acc += n
        want = G - len(cuts)
        if want > 0 and nb - b - 1 >= want and acc * G >= sum(counts) * len(cuts):
            cuts.append(b + 1)
    return cuts + [nb] if nb else cuts


def check_groups(counts, G, cuts):
    """Non-empty, consecutive, covering [0, nb), at most min(G, nb) of them."""
    nb = len(counts)
    assert cuts[0] == 0 and cuts[-1] == nb
    assert all(a < b for a, b in zip(cuts, cuts[1:]))
    assert len(cuts) - 1 <= min(G, nb)
    assert cuts == want_groups(counts, G)


def test_empty_call(binary):
    for a2a in (False, True):
        assert plan(binary, [], a2a=a2a, G=4) == ((0, [], []), [0])


def test_one_bucket(binary):
    # 10 f32 over 4 ranks: shards of 2 (4 x 8 = 32 bytes), a tail of 2
    assert plan(binary, [10]) == ((256, [0], [0]), [0, 1])
    assert plan(binary, [10], a2a=True, G=4) == ((512, [0], [256]), [0, 1])
    # 1024 f32: no tail; the received shards are the whole bucket's bytes
    assert plan(binary, [1024]) == ((0, [0], [0]), [0, 1])
    assert plan(binary, [1024], a2a=True) == ((4096, [0], [0]), [0, 1])


def test_counts_below_the_world_are_tails_only(binary):
    for a2a in (False, True):
        assert plan(binary, [3, 0, 1], a2a=a2a)[0] == (512, [0, 0, 0], [0, 0, 256])


@pytest.mark.parametrize("a2a", [False, True])
def test_shards_and_tails_under_each_algorithm(binary, a2a):
    counts = [1000 * 3 + 2, 7, 3 * 4096 + 1, 3 * 100]
    got, _ = plan(binary, counts, world=3, sz=2, a2a=a2a)
    assert got == want_workspace(counts, 3, 2, a2a)
    if a2a:  # shards of 1000, 2, 4096, 100 bf16 from 3 ranks; tails of 2, 1, 1, 0
        assert got == (6144 + 256 + 256 + 256 + 24576 + 256 + 768,
                       [0, 6400, 6912, 31744], [6144, 6656, 31488, 0])
    else:
        assert got == (768, [0, 0, 0, 0], [0, 256, 512, 0])


@pytest.mark.parametrize("world,sz", [(1, 4), (2, 1), (8, 8), (16, 2)])
def test_layout_agrees_with_the_rule(binary, world, sz):
    counts = [0, 1, world - 1, world, world + 1, 255 * world, 256 * world + 3, 10 ** 9 + 7]
    for a2a in (False, True):
        got, _ = plan(binary, counts, world=world, sz=sz, a2a=a2a)
        assert got == want_workspace(counts, world, sz, a2a)
        assert all(off % STEP == 0 for off in got[1] + got[2]) and got[0] % STEP == 0


def test_more_groups_than_buckets(binary):
    assert plan(binary, [10, 10], G=5)[1] == [0, 1, 2]
    assert plan(binary, [7], G=4)[1] == [0, 1]


def test_one_huge_bucket_first(binary):
    assert plan(binary, [1000, 1, 1, 1], G=2)[1] == [0, 1, 4]
    assert plan(binary, [1000, 1, 1, 1], G=3)[1] == [0, 1, 2, 4]


def test_one_huge_bucket_last(binary):
    # no earlier bucket reaches a share: the call stays one group
    assert plan(binary, [1, 1, 1, 1000], G=2)[1] == [0, 4]
    assert plan(binary, [1, 1, 1, 1000], G=3)[1] == [0, 4]


def test_all_equal_buckets(binary):
    assert plan(binary, [5, 5, 5, 5], G=1)[1] == [0, 4]
    assert plan(binary, [5, 5, 5, 5], G=2)[1] == [0, 2, 4]
    assert plan(binary, [5, 5, 5, 5], G=4)[1] == [0, 1, 2, 3, 4]
    assert plan(binary, [5] * 64, G=4)[1] == [0, 16, 32, 48, 64]


@pytest.mark.parametrize("G", [1, 2, 3, 4, 7, 100])
def test_groups_are_consecutive_and_cover_the_call(binary, G):
    for counts in ([1], [0, 0, 0], [3, 1, 4, 1, 5, 9, 2, 6], [1 << 40, 1, 1 << 40], [0, 0, 9, 0],
                   [5] * 13, list(range(20))):
        check_groups(counts, G, plan(binary, counts, G=G)[1])
