"""The gradient monitors on the GPU: the segmented squared-norm kernels
(kf_segnorm_*: bound, determinism, range, VAR, graph capture), the device
noise-scale update against the numpy restatement bit for bit, and both
monitoring optimizers at world 2 (two processes sharing cuda:0 over gloo,
as tests/test_configs_gpu.py runs its configs).

Bounds are derived, not measured (include/kungfu_amd.h): fp64 accumulation of
exact squares, |out[s] - exact| <= (n + 2) * 2^-53 * exact.
"""
import math
import os
import sys
import traceback

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import monitor_ref
from monitor_ref import bound, exact_sq, exact_var, left_sum, total_sqrt_bound
from oracle.oracle import f32_to_bf16_bits
from procs import hung_msg, join_all

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

pytestmark = pytest.mark.gpu

COUNTS = [0, 1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 4099, 65537, (1 << 20) + 7]
BIG = (1 << 20) + 7
DTYPES = ["f32", "f16", "bf16", "f64"]
NP = {"f32": np.float32, "f16": np.float16, "bf16": np.uint16, "f64": np.float64}
TORCH = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16,
         "f64": torch.float64}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def cast(x, dt):
    """fp64 values -> dt's host representation (bf16: uint16 bit patterns)."""
    if dt == "bf16":
        return f32_to_bf16_bits(x.astype(np.float32))
    return x.astype(NP[dt])


def to_dev(a, dt, dev):
    if dt == "bf16":
        return torch.from_numpy(a.view(np.int16)).to(dev).view(torch.bfloat16)
    return torch.from_numpy(a).to(dev)


def counts_for(nseg):
    """COUNTS cycled; the 1 Mi-element count at most twice per case."""
    out, big = [], 0
    for k in range(nseg):
        c = COUNTS[k % len(COUNTS)] if nseg > 1 else 4099
        if c == BIG:
            big += 1
            if big > 2:
                c = 257
        out.append(c)
    return out


def layout(counts, dt, shift=None):
    """Element offsets of the segments in one flat buffer: segment k starts at
    16-B residue k (+ shift.get(k, 0)) modulo the elements per 16 B, so every
    residue of the dtype occurs, with at least one poisoned element between
    neighbours. Returns (offsets, total)."""
    e = 16 // np.dtype(NP[dt]).itemsize
    offs, cur = [], 1
    for k, c in enumerate(counts):
        want = (k + (shift or {}).get(k, 0)) % e
        cur += (want - cur) % e
        offs.append(cur)
        cur += c + 1
    return offs, cur + e


def poisoned(total, dt):
    """A flat host buffer whose every element would wreck a sum that read it."""
    bad = np.array([np.inf if dt == "f16" else 1e30])
    return np.full(total, cast(bad, dt)[0], dtype=NP[dt])


def make_case(counts, dt, dev, seed, shift=None, square=False):
    offs, total = layout(counts, dt, shift)
    host = poisoned(total, dt)
    rng = np.random.default_rng(seed)
    segs = []
    for o, c in zip(offs, counts):
        x = rng.standard_normal(c)
        v = cast(x * x if square else x, dt)
        host[o:o + c] = v
        segs.append(v)
    flat = to_dev(host, dt, dev)
    views = [flat[o:o + c] for o, c in zip(offs, counts)]
    if len(counts) >= 16:  # every 16-B residue of the dtype occurs
        itemsize = host.dtype.itemsize
        seen = {(v.data_ptr() % 16) // itemsize for v, c in zip(views, counts) if c}
        assert seen == set(range(16 // itemsize)), seen
    return flat, views, segs


def check_bound(got, want, n, what):
    err = abs(got - want)
    print("%s: n=%d got=%.17g exact=%.17g rel=%.3g bound=%.3g"
          % (what, n, got, want, err / want if want else err, bound(n)))
    assert err <= bound(n) * want, what


# ---- 1. SQ: the bound, every residue, no over-read --------------------------

@pytest.mark.parametrize("nseg", [1, 16, 17, 65, 214])
@pytest.mark.parametrize("dt", DTYPES)
def test_sq_bound(dev, dt, nseg):
    from kungfu_amd import ops
    counts = counts_for(nseg)
    flat, views, segs = make_case(counts, dt, dev, seed=nseg)
    plan = ops.SegNorm(views)
    out = plan.run("sq")
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    plan.close()
    assert got.shape == (nseg + 1,) and got.dtype == np.float64
    for s, (seg, n) in enumerate(zip(segs, counts)):
        check_bound(float(got[s]), exact_sq(seg, dt), n, "%s seg %d" % (dt, s))
        if n == 0:
            assert got[s] == 0.0
    tot = left_sum(got[:nseg])
    assert got[nseg].tobytes() == np.float64(tot).tobytes()


# ---- 2. determinism, no stale state -----------------------------------------

def test_same_bits_whatever_ran_before(dev):
    from kungfu_amd import ops
    counts = counts_for(17)
    flat, views, _ = make_case(counts, "f32", dev, seed=5)
    plan = ops.SegNorm(views)
    out = torch.empty(18, dtype=torch.float64, device=dev)
    out.view(torch.uint8).fill_(0xFF)
    plan.run("sq", out=out)
    torch.cuda.synchronize()
    first = out.cpu().numpy().copy()
    assert np.isfinite(first).all()
    # a different, larger plan's data through in between (its workspace is
    # freed again, so the allocator may hand the same memory around), and the
    # output pre-filled with 0xFF bytes
    flat2, views2, _ = make_case(counts_for(65), "f32", dev, seed=6)
    other = ops.SegNorm(views2)
    other.run("sq")
    torch.cuda.synchronize()
    other.close()
    for _ in range(2):
        out.view(torch.uint8).fill_(0xFF)
        plan.run("sq", out=out)
        torch.cuda.synchronize()
        assert out.cpu().numpy().tobytes() == first.tobytes()
    # a second plan over the same bytes: the same bits
    again = ops.SegNorm(views)
    assert again.run("sq").cpu().numpy().tobytes() == first.tobytes()
    again.close()
    plan.close()


# ---- 3. range -----------------------------------------------------------------

def test_range_and_non_finite(dev):
    from kungfu_amd import ops
    big = np.full(4, 3e38, np.float32)
    tiny = np.full(1000, 1e-45, np.float32)
    assert tiny[0] > 0 and tiny[0] == np.float32(2.0 ** -149)  # the smallest subnormal
    rng = np.random.default_rng(3)
    plain = [rng.standard_normal(300).astype(np.float32) for _ in range(3)]
    with_inf = plain[1].copy()
    with_inf[17] = np.inf
    with_nan = plain[1].copy()
    with_nan[250] = np.nan
    segs = [big, tiny, plain[0], with_inf, plain[2], with_nan, plain[0]]
    ts = [torch.from_numpy(s).to(dev) for s in segs]
    plan = ops.SegNorm(ts)
    got = plan.run("sq").cpu().numpy()
    plan.close()
    assert got[0] == 4 * float(big[0]) ** 2 and np.isfinite(got[0])  # no fp32 overflow
    assert got[1] == 1000 * 2.0 ** -298 and got[1] > 0  # subnormals not flushed
    assert got[3] == np.inf
    assert np.isnan(got[5])
    for s in (2, 4, 6):  # the neighbours of the inf and the NaN
        check_bound(float(got[s]), exact_sq(segs[s], "f32"), 300, "neighbour %d" % s)
    assert np.isnan(got[7])


# ---- 4. VAR ---------------------------------------------------------------------

@pytest.mark.parametrize("dt", DTYPES)
def test_var_bound_and_total_sqrt(dev, dt):
    from kungfu_amd import ops
    counts = counts_for(17)
    # a: mean-of-squares-like (non-negative), b: gradient-like; segment 12
    # (4099 elements) has b one element off a's 16-B residue
    fa, va, sa = make_case(counts, dt, dev, seed=40, square=True)
    fb, vb, sb = make_case(counts, dt, dev, seed=41, shift={12: 1})
    assert va[12].data_ptr() % 16 != vb[12].data_ptr() % 16
    plan = ops.SegNorm(list(zip(va, vb)))
    got = plan.run("var").cpu().numpy()
    root = plan.run("var", total_sqrt=True).cpu().numpy()
    sq = plan.run("sq").cpu().numpy()  # a plan with b still runs SQ over a
    plan.close()
    exact = [exact_var(a, b, dt) for a, b in zip(sa, sb)]
    for s, n in enumerate(counts):
        check_bound(float(got[s]), exact[s], n, "%s var seg %d" % (dt, s))
        check_bound(float(sq[s]), exact_sq(sa[s], dt), n, "%s sq seg %d" % (dt, s))
    assert got[17].tobytes() == np.float64(left_sum(got[:17])).tobytes()
    assert root[:17].tobytes() == got[:17].tobytes()
    want = math.fsum(math.sqrt(e) for e in exact)
    rel = abs(float(root[17]) - want) / want
    print("%s total sqrt: got=%.17g want=%.17g rel=%.3g bound=%.3g"
          % (dt, root[17], want, rel, total_sqrt_bound(counts)))
    assert rel <= total_sqrt_bound(counts)


def test_var_needs_pairs(dev):
    from kungfu_amd import _lib, ops
    x = torch.ones(10, device=dev)
    plan = ops.SegNorm([x])
    with pytest.raises(_lib.KungFuAMDError, match="KF_ERR_ARG"):
        plan.run("var")
    with pytest.raises(_lib.KungFuAMDError, match="KF_ERR_ARG"):
        plan.run(7)
    plan.close()
    with pytest.raises(TypeError):
        ops.SegNorm([torch.ones(10, device=dev, dtype=torch.int32)])
    with pytest.raises(ValueError):
        ops.SegNorm([torch.ones(10)])  # a CPU tensor: no fallback


# ---- 5. kf_noise_scale_update -----------------------------------------------

def test_noise_scale_update_matches_ref_bits(dev):
    from kungfu_amd import ops
    rng = np.random.default_rng(9)
    state = torch.zeros(4, dtype=torch.float32, device=dev)
    want = np.zeros(4, np.float32)
    for step in range(5):
        big = float(rng.uniform(0.5, 3.0))
        small = big + float(rng.uniform(0.01, 2.0))
        ops.noise_scale_update_(torch.tensor(small, dtype=torch.float64, device=dev),
                                torch.tensor(big, dtype=torch.float64, device=dev),
                                32, 64, 0.9, state)
        want = monitor_ref.noise_scale_step(want, small, big, 32, 64, 0.9)
        got = state.cpu().numpy()
        print(step, got, want)
        assert got.tobytes() == want.tobytes(), step
    # one peer: bb == bs divides by zero; IEEE's inf / NaN, not an error
    st1 = torch.zeros(4, dtype=torch.float32, device=dev)
    ops.noise_scale_update_(torch.tensor(2.5, dtype=torch.float64, device=dev),
                            torch.tensor(1.5, dtype=torch.float64, device=dev), 32, 32, 0.9, st1)
    w1 = monitor_ref.noise_scale_step(np.zeros(4, np.float32), 2.5, 1.5, 32, 32, 0.9)
    g1 = st1.cpu().numpy()
    assert not np.isfinite(g1[:3]).all()
    assert np.array_equal(np.isnan(g1), np.isnan(w1))
    assert g1[~np.isnan(g1)].tobytes() == w1[~np.isnan(w1)].tobytes()


# ---- 6. graph capture -------------------------------------------------------

def test_segnorm_run_captures_and_replays(dev):
    """One SegNorm.run queued into a HIP graph on a side stream (as
    tests/test_gpu_parity.py does for the B2 ops) and replayed twice with
    the inputs changed in between: no allocation, no host sync inside."""
    from kungfu_amd import ops
    counts = counts_for(17)
    flat, views, segs = make_case(counts, "f32", dev, seed=60)
    plan = ops.SegNorm(views)
    out = torch.zeros(18, dtype=torch.float64, device=dev)
    plan.run("sq", out=out)  # eager once: code objects loaded before capture
    torch.cuda.synchronize()
    out.zero_()
    graph = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            plan.run("sq", out=out, stream=s)
    torch.cuda.synchronize()
    assert float(out.abs().sum()) == 0.0  # capture ran nothing
    for scale in (1.0, 3.0):
        if scale != 1.0:
            for v in views:
                v.mul_(scale)  # exact in fp32 only up to rounding: re-read below
        torch.cuda.synchronize()
        now = [v.cpu().numpy() for v in views]
        graph.replay()
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        for k, (seg, n) in enumerate(zip(now, counts)):
            check_bound(float(got[k]), exact_sq(seg, "f32"), n, "replay x%g seg %d" % (scale, k))
        assert got[17].tobytes() == np.float64(left_sum(got[:17])).tobytes()
    plan.close()


# ---- 7. the optimizers at world 2 ---------------------------------------------

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
    hung = join_all(ps, 300)
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


def _host(t):
    t = t.detach().cpu()
    if t.dtype == torch.bfloat16:
        return t.view(torch.int16).numpy().view(np.uint16)
    return t.numpy()


MODEL_F32 = [("f32", n) for n in (7, 64, 1000, 4097, 3)]
MODEL_MIXED = MODEL_F32 + [("bf16", 130), ("bf16", 2049)]


def _grad(model, r, step):
    """Rank r's gradients of one step, host representation, from a seed both
    ranks know."""
    rng = np.random.default_rng(1000 * step + r)
    return [cast(rng.standard_normal(n), dt) for dt, n in model]


def _params(model, dev):
    rng = np.random.default_rng(77)
    return [torch.nn.Parameter(to_dev(cast(rng.standard_normal(n), dt), dt, dev))
            for dt, n in model]


def _square(g, dt):
    """fl_T(g * g): the reduce kernel's PROD."""
    if dt == "bf16":
        f = monitor_ref.bf16_bits_to_f32(g)
        return f32_to_bf16_bits(f * f)
    return (g * g).astype(g.dtype)


def _monitors_body(rank, world, port, errq, mixed):
    try:
        dist = _init(rank, world, port)
        from kungfu_amd.collective import Exchange
        from kungfu_amd.optimizers import (MonitorGradientNoiseScaleOptimizer,
                                           MonitorGradientVarianceOptimizer,
                                           SynchronousSGDOptimizer)
        from oracle import oracle
        dev = torch.device("cuda:0")
        model = MODEL_MIXED if mixed else MODEL_F32
        ntotal = sum(n for _, n in model)

        def sgd(ps):
            return torch.optim.SGD(ps, lr=0.125)

        plain_p, ns_p, gv_p = (_params(model, dev) for _ in range(3))
        kw = dict(bucket_bytes=4096)
        plain = SynchronousSGDOptimizer(sgd(plain_p), average=True, exchange=Exchange(), **kw)
        ns = MonitorGradientNoiseScaleOptimizer(sgd(ns_p), 32, monitor_interval=2, alpha=0.9,
                                                exchange=Exchange(), **kw)
        gv = MonitorGradientVarianceOptimizer(sgd(gv_p), monitor_interval=2,
                                              exchange=Exchange(), **kw)
        ref_state = np.zeros(4, np.float32)
        for step in range(3):
            gs = [_grad(model, r, step) for r in range(world)]
            for ps in (plain_p, ns_p, gv_p):
                for p, g, (dt, _) in zip(ps, gs[rank], model):
                    p.grad = to_dev(g, dt, dev)
            before = _host(ns.noise_scale_state).copy()
            var_before = _host(gv.last_variances).copy()
            plain.step()
            ns.step()
            gv.step()
            torch.cuda.synchronize()
            if step == 0:  # several buckets per group, so the plans have several segments
                assert len(ns._kf_groups) == (2 if mixed else 1)
                assert len(ns._kf_groups[0][1].buckets) >= 3
            # the monitors disturb nothing: parameters bit-equal to plain S-SGD
            for i, (a, b, c) in enumerate(zip(plain_p, ns_p, gv_p)):
                assert _host(a).tobytes() == _host(b).tobytes(), (step, i)
                assert _host(a).tobytes() == _host(c).tobytes(), (step, i)
            state = _host(ns.noise_scale_state)
            if step == 1:  # not monitored: nothing moves
                assert state.tobytes() == before.tobytes()
                assert _host(gv.last_variances).tobytes() == var_before.tobytes()
                continue
            # the averaged gradient and the averaged squares, as the exchange
            # computes them (sum, / np; exact to restate at world 2)
            avg = [oracle.reduce_avg([gs[r][i] for r in range(world)], dt, world)
                   for i, (dt, _) in enumerate(model)]
            avg_sq = [oracle.reduce_avg([_square(gs[r][i], dt) for r in range(world)], dt, world)
                      for i, (dt, _) in enumerate(model)]
            for i, (p, (dt, _)) in enumerate(zip(ns_p, model)):  # the exchange itself
                assert _host(p.grad).tobytes() == avg[i].tobytes(), (step, i)
            # noise scale: both sums within the bound of the exact ones ...
            small = float(ns.last_sq_small.item())
            big = float(ns.last_sq_big.item())
            want_small = math.fsum(exact_sq(g, dt) for g, (dt, _) in zip(gs[rank], model))
            want_big = math.fsum(exact_sq(g, dt) for g, (dt, _) in zip(avg, model))
            check_bound(small, want_small, ntotal, "step %d sq_small" % step)
            check_bound(big, want_big, ntotal, "step %d sq_big" % step)
            # ... and the estimate bit-equal to the chain fed those two
            # observed values (the formula cancels: only this is meaningful)
            ref_state = monitor_ref.noise_scale_step(ref_state, small, big, 32, 32 * world, 0.9)
            assert state.tobytes() == ref_state.tobytes(), (step, state, ref_state)
            assert _host(ns.noise_scale).tobytes() == ref_state[2].tobytes()
            # variance: per-parameter sums, then the sum of their roots
            got = _host(gv.last_variances)
            exact = [exact_var(a, b, dt) for a, b, (dt, _) in zip(avg_sq, avg, model)]
            for i, (dt, n) in enumerate(model):
                check_bound(float(got[i]), exact[i], n, "step %d variance %d" % (step, i))
            want = math.fsum(math.sqrt(e) for e in exact)
            rel = abs(float(gv.variance.item()) - want) / want
            assert rel <= total_sqrt_bound([n for _, n in model]), (step, rel)
        dist.barrier()
        dist.destroy_process_group()
    except Exception:
        errq.put("rank %d: %s" % (rank, traceback.format_exc()))


@pytest.mark.parametrize("mixed", [False, True], ids=["f32", "f32+bf16"])
def test_monitoring_optimizers_world2(mixed):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    _run(_monitors_body, 2, mixed)
