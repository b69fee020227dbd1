"""Pair averaging's host side (no GPU): the seqlock protocol over every
interleaving of a reader with a writer (pairavg_ref's model), the reference's
peer choice, constructor validation, the argument errors of the C ABI that
touch no device, and the numpy blend pinned against hand-computed cases."""
import ctypes
import itertools
import math
import os
import random
import subprocess

import numpy as np
import pytest
import torch

import pairavg_ref
from pairavg_ref import EMPTY, TORN, VALID

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
LIB = os.path.join(ROOT, "kungfu_amd", "libkungfu_amd.so")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "kungfu_amd", "csrc")],
                       check=True)
    from kungfu_amd import _lib
    return _lib.load()


# ---- the protocol, exhaustively ------------------------------------------

def _interleavings(slots, start):
    """One reader's pick / fetch / check at every position among a writer's
    three consecutive publishes (begin, copy half, copy half, end each), from
    a store that already holds `start` versions. Yields (reader, positions,
    latest seen at pick)."""
    nw = 12
    for pos in itertools.combinations(range(nw + 3), 3):
        st = pairavg_ref.Store(slots)
        w, r = pairavg_ref.Writer(st), pairavg_ref.Reader(st)
        for _ in range(start):
            w.publish()
        wsteps = [ph for _ in range(3) for ph in w.phases()]
        rsteps = r.phases()
        wi = ri = 0
        for i in range(nw + 3):
            if ri < 3 and i == pos[ri]:
                rsteps[ri]()
                ri += 1
            else:
                wsteps[wi]()
                wi += 1
        assert wi == nw and ri == 3 and st.latest == start + 3
        yield r, pos


@pytest.mark.parametrize("start", [0, 1, 2])
@pytest.mark.parametrize("slots", [2, 3])
def test_every_interleaving_gives_a_whole_version_or_nothing(slots, start):
    seen = {VALID: 0, TORN: 0, EMPTY: 0}
    mixed = cases = 0
    for r, pos in _interleavings(slots, start):
        cases += 1
        # exactly one outcome
        assert r.outcome in seen and sum(r.counters.values()) == 1
        assert r.counters[r.outcome] == 1
        seen[r.outcome] += 1
        if r.outcome == VALID:
            # one whole version: the one `latest` named at the pick
            assert len(set(r.staging)) == 1, (pos, r.staging)
            assert r.staging[0] >= r.version and r.staging[0] == r.version, (pos, r.staging)
        elif r.staging is not None and r.state is None and len(set(r.staging)) > 1:
            mixed += 1  # a half-written slot was read: it must not count as valid
        # no writer phase between pick and check: always valid once published
        if pos[2] - pos[0] == 2 and r.version > 0:
            assert r.outcome == VALID, pos
        if r.version == 0:
            assert r.outcome == EMPTY
    assert cases == math.comb(15, 3)
    # the enumeration reaches every path it is meant to judge
    assert seen[VALID]
    assert bool(seen[EMPTY]) == (start == 0)
    # a pull can only be torn if the slot of a version it can pick (the first
    # is max(start, 1)) is written again, `slots` versions later, within the
    # three publishes
    rewritten = max(start, 1) + slots <= start + 3
    assert bool(seen[TORN]) == rewritten and bool(mixed) == rewritten


def test_slots_minus_one_publishes_keep_a_pick_valid():
    """With S slots the S - 1 publishes after a pick go to other slots; the
    S-th rewrites the picked one."""
    for slots in (2, 3, 4):
        for extra, want in ((slots - 1, VALID), (slots, TORN)):
            st = pairavg_ref.Store(slots)
            w, r = pairavg_ref.Writer(st), pairavg_ref.Reader(st)
            w.publish()
            r.pick()
            for _ in range(extra):
                w.publish()
            r.fetch()
            assert r.check() == want
            if want == VALID:
                assert r.staging == [1] * st.width


# ---- peer choice ---------------------------------------------------------

def test_random_peer_is_the_reference_rule():
    from kungfu_amd.pairavg import random_peer
    rng = random.Random(7)
    assert all(random_peer(rng, 1, 0) == 0 for _ in range(20))
    for world in (2, 3, 8):
        for rank in range(world):
            assert all(random_peer(rng, world, rank) != rank for _ in range(200))
    # world 4, rank 1: t == 1 becomes 2, so rank 2 has p = 1/2, ranks 0 and 3 p = 1/4
    n = 8000
    rng = random.Random(12345)
    counts = [0] * 4
    for _ in range(n):
        counts[random_peer(rng, 4, 1)] += 1
    assert counts[1] == 0 and sum(counts) == n
    for peer, p in ((2, 0.5), (0, 0.25), (3, 0.25)):
        sd = math.sqrt(n * p * (1 - p))
        assert abs(counts[peer] - n * p) <= 5 * sd, (peer, counts)


# ---- constructor validation ----------------------------------------------

def _sgd(dtype=torch.float32):
    p = torch.nn.Parameter(torch.zeros(4, dtype=dtype), requires_grad=dtype.is_floating_point)
    return torch.optim.SGD([p], lr=0.1), p


@pytest.mark.parametrize("bad", [1, 0, -2])
def test_pair_averaging_rejects_fewer_than_two_slots(bad):
    from kungfu_amd.optimizers import PairAveragingOptimizer
    with pytest.raises(ValueError, match="slots"):
        PairAveragingOptimizer(_sgd()[0], slots=bad)


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64, torch.uint8])
def test_pair_averaging_rejects_integer_parameters(dtype):
    from kungfu_amd.optimizers import PairAveragingOptimizer
    opt, p = _sgd(dtype)
    with pytest.raises(ValueError, match="f32, f16, bf16 and f64"):
        PairAveragingOptimizer(opt, named_parameters=[("p", p)])


def test_pair_averaging_rejects_an_out_of_range_peer_at_the_step():
    from kungfu_amd.optimizers import PairAveragingOptimizer
    for bad in (1, -1):  # no process group: world 1, the only peer is 0
        opt = PairAveragingOptimizer(_sgd()[0], peer_selector=lambda step, rank, world: bad)
        with pytest.raises(ValueError, match="peer_selector"):
            opt.step()
        assert opt.last_target is None


def test_pair_averaging_wraps_and_exports():
    from kungfu_amd import optimizers as kopt
    from kungfu_amd.torch import optimizers as topt
    assert "PairAveragingOptimizer" in topt.__all__
    opt, p = _sgd()
    o = topt.PairAveragingOptimizer(opt, [("p", p)], slots=3, seed=5)
    assert isinstance(o, torch.optim.SGD)
    assert o._kf_slots == 3 and o.last_target is None
    assert o.pair_counters == dict(valid=0, torn=0, empty=0, published=0)
    with pytest.raises(TypeError):  # no exchange= / overlap=: RCCL plays no part
        kopt.PairAveragingOptimizer(_sgd()[0], exchange=None)
    with pytest.raises(TypeError):
        kopt.PairAveragingOptimizer(_sgd()[0], overlap=False)


def test_peer_model_store_rejects_bad_arguments():
    from kungfu_amd.pairavg import PeerModelStore
    with pytest.raises(ValueError, match="slots"):
        PeerModelStore([torch.zeros(4)], slots=1)
    with pytest.raises(ValueError, match="f32, f16, bf16 and f64"):
        PeerModelStore([torch.zeros(4, dtype=torch.int32)])


# ---- C ABI argument errors (no device) -----------------------------------

def _err(lib):
    return lib.kf_pairavg_last_error().decode()


def test_pairavg_create_arg_errors(lib):
    """Argument checks come before any HIP call (no device here)."""
    from kungfu_amd import _lib
    F32 = 0x20408
    lens = (ctypes.c_size_t * 2)(64, 64)
    ok = _lib.ptr_array([16, 32])
    # a null span pointer with a non-zero length
    assert lib.kf_pairavg_create(_lib.ptr_array([16, 0]), lens, 2, F32, 2, 1, 0) is None
    assert _err(lib).startswith("KF_ERR_ARG")
    # S < 2
    for slots in (1, 0, -1):
        assert lib.kf_pairavg_create(ok, lens, 2, F32, slots, 1, 0) is None
        assert _err(lib).startswith("KF_ERR_ARG") and "slots" in _err(lib)
    # rank >= world, negative rank, no world
    for world, rank in ((2, 2), (1, 1), (2, -1), (0, 0)):
        assert lib.kf_pairavg_create(ok, lens, 2, F32, 2, world, rank) is None
        assert _err(lib).startswith("KF_ERR_ARG") and "rank" in _err(lib)
    # no spans, null tables, a span off the 16-byte boundary, half an element
    assert lib.kf_pairavg_create(ok, lens, 0, F32, 2, 1, 0) is None
    assert _err(lib).startswith("KF_ERR_ARG")
    assert lib.kf_pairavg_create(None, lens, 2, F32, 2, 1, 0) is None
    assert _err(lib).startswith("KF_ERR_ARG")
    assert lib.kf_pairavg_create(_lib.ptr_array([16, 36]), lens, 2, F32, 2, 1, 0) is None
    assert _err(lib).startswith("KF_ERR_ARG")
    assert lib.kf_pairavg_create(ok, (ctypes.c_size_t * 2)(64, 6), 2, F32, 2, 1, 0) is None
    assert _err(lib).startswith("KF_ERR_ARG")
    # integers have no blend
    assert lib.kf_pairavg_create(ok, lens, 2, 0x10408, 2, 1, 0) is None
    assert _err(lib).startswith("KF_ERR_DTYPE")
    # a misaligned slot base; a misaligned control base
    ctrl = _lib.ptr_array([8, 16])
    assert lib.kf_pairavg_set_peers(None, _lib.ptr_array([16, 40]), ctrl, 2) == 3
    assert _err(lib).startswith("KF_ERR_ARG") and "slot base" in _err(lib)
    assert lib.kf_pairavg_set_peers(None, ok, _lib.ptr_array([8, 12]), 2) == 3
    assert _err(lib).startswith("KF_ERR_ARG") and "control base" in _err(lib)
    # every call on no plan
    for name in ("publish", "publish_begin", "publish_copy", "publish_end", "blend"):
        assert getattr(lib, "kf_pairavg_" + name)(None, None) == 3, name
    for name in ("pull_average", "pick", "fetch", "check"):
        assert getattr(lib, "kf_pairavg_" + name)(None, 0, None) == 3, name
    assert lib.kf_pairavg_counters(None, 8, None) == 3
    assert lib.kf_pairavg_local(None, None, None, None) == 3
    assert _err(lib).startswith("KF_ERR_ARG")
    lib.kf_pairavg_destroy(None)


# ---- the blend yardstick, by hand ----------------------------------------

def test_ref_blend_by_hand():
    from oracle.oracle import bf16_bits_to_f32, f32_to_bf16_bits
    blend = pairavg_ref.blend
    fmax = np.finfo(np.float32).max
    # f32: the add overflows before the halving can bring it back
    r = blend(np.array([fmax, 3.0], np.float32), np.array([fmax, 1.0], np.float32), "f32")
    assert r.dtype == np.float32 and np.isinf(r[0]) and r[0] > 0 and r[1] == 2.0
    # f32 subnormals, d = 2^-149: (d + 2d) / 2 = 1.5 d, a tie, rounds to the even 2 d;
    # (d + 0) / 2 = 0.5 d, a tie, rounds to the even 0; (2d + 4d) / 2 = 3 d exactly
    d = np.float32(2.0 ** -149)
    v = np.array([d, d, 2 * d], np.float32)
    o = np.array([2 * d, 0, 4 * d], np.float32)
    r = blend(v, o, "f32")
    assert r.tolist() == [float(2 * d), 0.0, float(3 * d)]
    # f64 is the same recipe
    assert blend(np.array([1.0]), np.array([2.0 ** -52]), "f64")[0] == 0.5 + 2.0 ** -53
    # f16: 65504 + 65504 overflows to inf
    r = blend(np.array([65504, 1], np.float16), np.array([65504, 2], np.float16), "f16")
    assert r.dtype == np.float16 and np.isinf(r[0]) and float(r[1]) == 1.5
    # f16: 1 + (1 + 2^-10) = 2 + 2^-10 is a tie at 2's spacing 2^-9 -> 2, halved 1
    assert float(blend(np.array([1], np.float16), np.array([1 + 2.0 ** -10], np.float16),
                       "f16")[0]) == 1.0
    # bf16: a sum keeps the mean's significand (a factor of two), so rounding
    # after the add can differ from one rounding of the exact mean only at
    # the ends of the range. v = max = 0x7f7f, o = 2^127 = 0x7f00: the exact
    # mean 2^127 * (1.5 - 2^-8) rounds once to 2^127 * 1.5 = 0x7f40 (a tie, to
    # even), but the sum 2^128 * (1.5 - 2^-8) overflows and the blend is inf.
    v = np.array([0x7F7F], np.uint16)
    o = np.array([0x7F00], np.uint16)
    exact_mean = (float(bf16_bits_to_f32(v)[0]) + float(bf16_bits_to_f32(o)[0])) / 2
    once = f32_to_bf16_bits(np.array([exact_mean], np.float32))
    assert once[0] == 0x7F40
    r = blend(v, o, "bf16")
    assert r.dtype == np.uint16 and r[0] == 0x7F80 and r[0] != once[0]
    # bf16 away from the limits: 1 + (1 + 2^-7) = 2 + 2^-7, a tie at 2^-6 -> 2, halved 1
    r = blend(np.array([0x3F80], np.uint16), np.array([0x3F81], np.uint16), "bf16")
    assert r[0] == 0x3F80
