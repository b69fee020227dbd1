"""Pair averaging on the device (kungfu_amd/pairavg.py, kf_pairavg_*): ranks
are processes sharing cuda:0 over gloo, as in tests/test_p2p.py. Every result
is compared bit for bit with pairavg_ref.blend; every ordering between ranks
in the scripted tests is a host barrier after a device sync (nothing waits on
the device for a peer)."""
import os
import sys
import traceback

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp
from procs import hung_msg, join_all

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

pytestmark = pytest.mark.gpu

# shorter than one 16-byte vector, a ragged tail, exactly one tile of
# 256 x 4 vectors (f32), many tiles with a tail
SIZES = [1, 3, 1021, 4096, 100003]
# more spans than KF_MAX_SEGMENTS: a second launch per phase
MANY = SIZES + [1] * 17

_DT = {
    "f32": (torch.float32, np.float32, np.uint32, torch.int32),
    "f64": (torch.float64, np.float64, np.uint64, torch.int64),
    "f16": (torch.float16, np.float16, np.uint16, torch.int16),
    "bf16": (torch.bfloat16, None, np.uint16, torch.int16),
}


def _bits(a, dt):
    return np.ascontiguousarray(a).view(_DT[dt][2])


def _to_torch(a, dt, dev):
    tdt, _, u, ti = _DT[dt]
    signed = _bits(a, dt).view(np.dtype("i%d" % np.dtype(u).itemsize))
    return torch.from_numpy(signed.copy()).to(dev).view(tdt)


def _to_numpy(t, dt):
    tdt, npt, u, ti = _DT[dt]
    raw = t.detach().contiguous().view(ti).cpu().numpy().view(u)
    return raw if npt is None else raw.view(npt)


def _cast(x64, dt):
    """fp64 values -> T's representation (bf16 as uint16 bits)."""
    if dt == "bf16":
        from oracle.oracle import f32_to_bf16_bits
        return f32_to_bf16_bits(x64.astype(np.float32))
    return x64.astype(_DT[dt][1])


def _random(dt, n, seed):
    return _cast(np.random.default_rng(seed).standard_normal(n), dt)


def _specials(dt):
    """(v, o) pairs at fixed positions: signed zeros, inf, NaN, the largest
    finite value, subnormals."""
    if dt == "bf16":
        big, sub, one = 0x7F7F, 0x0001, 0x3F80
        inf, nan, nz = 0x7F80, 0x7FC0, 0x8000
        neg = lambda b: b ^ 0x8000  # noqa: E731
        pairs = [(0, nz), (nz, nz), (inf, one), (inf, neg(inf)), (nan, one), (one, nan),
                 (big, big), (big, neg(big)), (sub, sub), (sub, 0), (neg(sub), 0), (sub, 0x0002),
                 (big, 0x7F00)]
        v, o = zip(*pairs)
        return np.array(v, np.uint16), np.array(o, np.uint16)
    t = _DT[dt][1]
    fi = np.finfo(t)
    big, sub = fi.max, fi.smallest_subnormal
    pairs = [(0.0, -0.0), (-0.0, -0.0), (np.inf, 1.0), (np.inf, -np.inf), (np.nan, 1.0),
             (1.0, np.nan), (big, big), (big, -big), (sub, sub), (sub, 0.0), (-sub, 0.0),
             (sub, 2 * sub), (big, big / 2)]
    v, o = zip(*pairs)
    return np.array(v, t), np.array(o, t)


def _same(got, want, dt):
    """Bit equality; NaNs are compared by position."""
    if dt == "bf16":
        from oracle.oracle import bf16_bits_to_f32
        gn, wn = np.isnan(bf16_bits_to_f32(got)), np.isnan(bf16_bits_to_f32(want))
    else:
        gn, wn = np.isnan(got), np.isnan(want)
    if not np.array_equal(gn, wn):
        return False
    return np.array_equal(_bits(got, dt)[~gn], _bits(want, dt)[~wn])


# ---- 1. world 1, single process, every dtype -----------------------------

@pytest.mark.parametrize("dt", ["f32", "f16", "bf16", "f64"])
def test_world1_publish_pull_blend_is_bit_exact(dt):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import pairavg_ref
    from kungfu_amd.pairavg import PeerModelStore
    dev = torch.device("cuda:0")
    sv, so = _specials(dt)
    old = [_random(dt, n, 10 + i) for i, n in enumerate(MANY)]
    new = [_random(dt, n, 500 + i) for i, n in enumerate(MANY)]
    k = len(sv)
    old[4][:k], new[4][:k] = so, sv          # the specials meet in the vector body
    old[4][-3:], new[4][-3:] = so[:3], sv[:3]  # and in the scalar tail
    old[2][-k:], new[2][-k:] = so, sv
    spans = [_to_torch(a, dt, dev) for a in old]
    store = PeerModelStore(spans)
    assert store.world == 1 and store.rank == 0
    try:
        # a pull before any publish: nothing to fetch, nothing changes
        store.pull_average_(0)
        assert store.counters() == dict(valid=0, torn=0, empty=1, published=0)
        for t, a in zip(spans, old):
            assert np.array_equal(_bits(_to_numpy(t, dt), dt), _bits(a, dt))
        store.publish()
        for t, a in zip(spans, new):
            t.copy_(_to_torch(a, dt, dev))
        store.pull_average_(0)
        assert store.counters() == dict(valid=1, torn=0, empty=1, published=1)
        for i, (t, a, b) in enumerate(zip(spans, new, old)):
            want = pairavg_ref.blend(a, b, dt)
            got = _to_numpy(t, dt)
            assert _same(got, want, dt), (dt, i, MANY[i])
        with pytest.raises(ValueError):
            store.pull_average_(1)
    finally:
        store.close()


# ---- multi-process scaffolding (tests/test_p2p.py's) ---------------------

def _run(target, world, *args):
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    errq = ctx.SimpleQueue()
    ps = [ctx.Process(target=target, args=(r, world, port, errq) + args) for r in range(world)]
    for p in ps:
        p.start()
    hung = join_all(ps, 240)
    errs = []
    while not errq.empty():
        errs.append(errq.get())
    assert not errs, "\n".join(errs)
    assert not hung and all(p.exitcode == 0 for p in ps), hung_msg(hung, [p.exitcode for p in ps])


def _init(rank, world, port):
    sys.path[:0] = [ROOT, HERE]
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    return dist


def _meet(dist):
    torch.cuda.synchronize()
    dist.barrier()


# ---- 2. worlds 2 and 3 in lock step --------------------------------------

def _lockstep_body(rank, world, port, errq):
    try:
        dist = _init(rank, world, port)
        import pairavg_ref
        from kungfu_amd.pairavg import PeerModelStore
        dev = torch.device("cuda:0")
        dt = "f32"

        def data(rnd, r):
            return [_random(dt, n, 10000 * rnd + 100 * r + i) for i, n in enumerate(SIZES)]

        spans = [torch.zeros(n, device=dev) for n in SIZES]
        store = PeerModelStore(spans)
        peer = (rank + 1) % world
        for rnd in range(3):  # three versions: both slots are reused
            for t, a in zip(spans, data(rnd, rank)):
                t.copy_(_to_torch(a, dt, dev))
            store.publish()
            _meet(dist)
            store.pull_average_(peer)
            torch.cuda.synchronize()
            for i, (t, a, b) in enumerate(zip(spans, data(rnd, rank), data(rnd, peer))):
                assert _same(_to_numpy(t, dt), pairavg_ref.blend(a, b, dt), dt), (rnd, i)
            _meet(dist)
        assert store.counters() == dict(valid=3, torn=0, empty=0, published=3)
        store.close()
        dist.destroy_process_group()
    except Exception:
        errq.put("rank %d: %s" % (rank, traceback.format_exc()))


@pytest.mark.parametrize("world", [2, 3])
def test_lockstep_pull_from_next_rank_is_bit_exact(world):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    _run(_lockstep_body, world)


# ---- 3. torn and empty paths through the phase entry points --------------

def _phases_body(rank, world, port, errq):
    """Rank 0 reads, rank 1 writes, two slots; turn(who, fn) lets one rank act
    and then both meet (device sync, host barrier).

    With version n in slot n % S, a writer that has only begun its next
    publish holds the lock of a slot OTHER than `latest`'s, so a whole pull
    that starts then is not torn: before the first version it is empty (a0),
    afterwards it gets the previous version whole. A pull meets an odd lock
    only when the writer has come round to the picked slot again, which the
    phase entry points script in (a)."""
    try:
        dist = _init(rank, world, port)
        import pairavg_ref
        from kungfu_amd.pairavg import PeerModelStore
        dev = torch.device("cuda:0")
        dt = "f32"
        sizes = [3, 1021, 40007]
        spans = [torch.zeros(n, device=dev) for n in sizes]
        store = PeerModelStore(spans, slots=2)

        def data(tag):
            return [_random(dt, n, 7000 + 10 * tag + i) for i, n in enumerate(sizes)]

        def put(tag):
            for t, a in zip(spans, data(tag)):
                t.copy_(_to_torch(a, dt, dev))

        def turn(who, fn):
            if rank == who:
                fn()
            _meet(dist)

        def expect(mine, theirs, counters):
            """Rank 0's variables: data(mine), blended with data(theirs) or
            untouched (theirs None); and its counters."""
            if rank == 0:
                torch.cuda.synchronize()
                for i, (t, a) in enumerate(zip(spans, data(mine))):
                    want = a if theirs is None else pairavg_ref.blend(a, data(theirs)[i], dt)
                    assert _same(_to_numpy(t, dt), want, dt), (mine, theirs, i)
                c = store.counters()
                assert (c["valid"], c["torn"], c["empty"]) == counters, c
            _meet(dist)

        def rest_of_pull():
            store._fetch(1)
            store._check_(1)
            store._blend()

        # (a0) the writer has only begun its first publish: nothing to pull yet
        turn(1, lambda: (put(101), store._publish_begin()))
        turn(0, lambda: (put(1), store.pull_average_(1)))
        expect(1, None, (0, 0, 1))
        turn(1, lambda: (store._publish_copy(), store._publish_end()))  # v1 = data(101)
        turn(0, lambda: store.pull_average_(1))
        expect(1, 101, (1, 0, 1))
        # (a) picked v1 (slot 1); the writer publishes v2 and is half way through
        # v3, in slot 1 again: its lock is odd at the check
        turn(0, lambda: (put(2), store._pick(1)))
        turn(1, lambda: (put(102), store.publish(), put(103), store._publish_begin(),
                         store._publish_copy()))
        turn(0, rest_of_pull)
        expect(2, None, (1, 1, 1))
        turn(1, store._publish_end)  # v3 = data(103)
        turn(0, lambda: store.pull_average_(1))
        expect(2, 103, (2, 1, 1))
        # (b) picked v3 (slot 1); S more versions: v5 has rewritten slot 1
        turn(0, lambda: (put(3), store._pick(1)))
        turn(1, lambda: (put(104), store.publish(), put(105), store.publish()))
        turn(0, rest_of_pull)
        expect(3, None, (2, 2, 1))
        # (c) picked v5 (slot 1); S - 1 more versions: v6 went to slot 0, and the
        # blend is with the version picked, not the newest
        turn(0, lambda: (put(4), store._pick(1)))
        turn(1, lambda: (put(106), store.publish()))
        turn(0, rest_of_pull)
        expect(4, 105, (3, 2, 1))
        if rank == 1:
            assert store.counters() == dict(valid=0, torn=0, empty=0, published=6)
        store.close()
        dist.destroy_process_group()
    except Exception:
        errq.put("rank %d: %s" % (rank, traceback.format_exc()))


def test_torn_and_empty_pulls_leave_the_variables_untouched():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    _run(_phases_body, 2)


# ---- 4. free running -----------------------------------------------------

def _free_body(rank, world, port, errq):
    try:
        dist = _init(rank, world, port)
        from kungfu_amd.optimizers import PairAveragingOptimizer
        dev = torch.device("cuda:0")
        shapes = [(1021,), (64, 33), (5,), (40007,)]
        params = [torch.nn.Parameter(torch.full(s, 2.0 ** rank, device=dev)) for s in shapes]
        # small buckets: the model is several spans
        opt = PairAveragingOptimizer(torch.optim.SGD(params, lr=0.0), bucket_bytes=8192, seed=1234)
        steps = 40
        for _ in range(steps):
            for p in params:
                p.grad = torch.zeros_like(p)
            opt.step()
        torch.cuda.synchronize()
        assert len(opt._kf_stores) == 1 and len(opt._kf_groups[0][1].buckets) > 1
        # every snapshot is a constant vector and so is every blend of two
        # (dyadic values, exact in fp32): any mix of two versions would show
        firsts = []
        for b, sp in zip(opt._kf_groups[0][1].buckets, opt._kf_groups[0][1].spans):
            h = b[:sp].cpu().numpy()
            assert (h == h[0]).all(), (rank, np.unique(h)[:8])
            assert 1.0 <= float(h[0]) <= 4.0
            firsts.append(float(h[0]))
        assert len(set(firsts)) == 1, firsts  # one store: the whole model is one version
        c = opt.pair_counters
        print("rank %d: value %r counters %r" % (rank, firsts[0], c), flush=True)
        assert c["valid"] + c["torn"] + c["empty"] == steps and c["published"] == steps + 1
        assert c["valid"] >= 1
        assert opt.last_target in [r for r in range(world) if r != rank]
        opt.close()
        dist.destroy_process_group()
    except Exception:
        errq.put("rank %d: %s" % (rank, traceback.format_exc()))


def test_free_running_ranks_never_mix_two_versions():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    _run(_free_body, 3)


# ---- 5. optimizer parity -------------------------------------------------

def _parity_body(rank, world, port, errq):
    """Both ranks replay both ranks: the blend in numpy (pairavg_ref.blend),
    the update by an unwrapped torch SGD on the same device (the same update
    kernel, so its rounding is not in question). A step pre-hook of the test
    holds every rank between its pull and its publish, and the loop holds
    them between steps: each pull then finds exactly what the peer published
    at the end of the previous step."""
    try:
        dist = _init(rank, world, port)
        import pairavg_ref
        from kungfu_amd.torch.optimizers import PairAveragingOptimizer
        dev = torch.device("cuda:0")
        dt = "f32"
        shapes = [("w", 1021), ("frozen", 7), ("b", 3)]
        with_grad = ("w", "b")

        def init(r):
            return {n: _random(dt, k, 31 * r + i) for i, (n, k) in enumerate(shapes)}

        def grad(step, r, n):
            k = dict(shapes)[n]
            return _random(dt, k, 900 + 50 * step + 7 * r + len(n))

        params = {n: torch.nn.Parameter(_to_torch(a, dt, dev)) for n, a in init(rank).items()}
        opt = PairAveragingOptimizer(torch.optim.SGD(list(params.values()), lr=0.1),
                                     list(params.items()),
                                     peer_selector=lambda step, rank, world: 1 - rank)
        opt.register_step_pre_hook(lambda *a, **k: _meet(dist))

        # the replay's state
        ref = [{n: torch.nn.Parameter(_to_torch(a, dt, dev)) for n, a in init(r).items()}
               for r in range(world)]
        sgd = [torch.optim.SGD(list(ref[r].values()), lr=0.1) for r in range(world)]
        pub = [init(r) for r in range(world)]

        for step in range(4):
            for n in with_grad:
                params[n].grad = _to_torch(grad(step, rank, n), dt, dev)
            assert params["frozen"].grad is None
            opt.step()
            _meet(dist)
            for r in range(world):
                for n in with_grad:
                    mixed = pairavg_ref.blend(_to_numpy(ref[r][n].data, dt), pub[1 - r][n], dt)
                    ref[r][n].data.copy_(_to_torch(mixed, dt, dev))
                    ref[r][n].grad = _to_torch(grad(step, r, n), dt, dev)
                sgd[r].step()
            pub = [{n: _to_numpy(ref[r][n].data, dt) for n, _ in shapes} for r in range(world)]
            for n, _ in shapes:
                assert _same(_to_numpy(params[n].data, dt), pub[rank][n], dt), (step, n)
            assert opt.last_target == 1 - rank
        assert _same(_to_numpy(params["frozen"].data, dt), init(rank)["frozen"], dt)
        assert opt.pair_counters == dict(valid=4, torn=0, empty=0, published=5)
        opt.close()
        dist.destroy_process_group()
    except Exception:
        errq.put("rank %d: %s" % (rank, traceback.format_exc()))


def test_optimizer_matches_a_replay_bit_for_bit():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    _run(_parity_body, 2)
