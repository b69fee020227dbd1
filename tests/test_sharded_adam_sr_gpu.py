"""The stochastic-rounding Adam / AdamW step on the GPU, bit for bit against
tests/adam_sr_ref.py: the batched update kernel and its gated twin alone, the
narrowing over its whole domain, and ShardedAdamOptimizer(stochastic_rounding=
True) end to end over the loopback transport and a one-rank librccl
communicator."""
import numpy as np
import pytest
import torch

import adam_ref
import adam_sr_ref as ref
import loopback
import step_gate_ref
import test_sharded_adam as adam_cpu
import test_sharded_adam_gated as gated
import test_sharded_adam_gpu as ag
import test_sharded_adam_sr as cpu

pytestmark = pytest.mark.gpu

# kf_adam_sr.hip's launch shape: 256 lanes, 4 vectors of 8 elements per lane
SR_SEG = cpu.SR_SEG
TILE = 256 * 4 * 8
SIZES = (0, 1, 7, 8, 9, 1023, TILE, TILE + 1, 2 * TILE + 8 * 300 + 5)
N_ONES = SR_SEG + 8  # with SIZES: more one-element segments than one launch's table
PAD = 24             # elements beyond `count` that must keep their bytes
SENTINEL = 0x5A5A
KEY = 0x9ABCDEF1


def _dev_padded(bits):
    """The segment's `count` elements as a view of a buffer with PAD more."""
    full = np.concatenate([bits, np.full(PAD, SENTINEL, np.uint16)])
    t = ag._dev(full, "bf16")
    assert t.data_ptr() % 16 == 0
    return t, t[:bits.size]


def _segments():
    """[(p, g, m, v)] as bf16 bits: SIZES, then N_ONES one-element segments,
    with tests/test_sharded_adam_gpu.py's random data, its exp_avg_sq over
    every binade and its IEEE specials at the start of the one-tile segment
    (a vector body), at the end of the 1023 one (its scalar tail and the
    vectors before it) and in the one-element segments (scalar tails alone)."""
    sp = ag._specials("bf16")
    k = len(sp[0])
    assert k <= N_ONES
    segs = ag._fill("bf16", SIZES + (1,) * N_ONES)
    for i, seg in enumerate(segs):
        n = seg[0].size
        for a, s in zip(seg, sp):
            if n == TILE:
                a[:k] = s
            elif n == 1023:
                a[-k:] = s
            elif n == 1 and i >= len(SIZES) and i - len(SIZES) < k:
                a[0] = s[i - len(SIZES)]
    return segs


@pytest.fixture(scope="module")
def segments():
    segs = _segments()
    # a base and a stream word of its own per segment
    bases = [8 * (1000 * i + 3) for i in range(len(segs))]
    streams = [(0x01234567 * (i + 1)) & 0xFFFFFFFF for i in range(len(segs))]
    return segs, bases, streams


def _hypers(n, wd, decoupled, step=3):
    # a hyper of its own per segment: the lr differs
    return [adam_ref.hyper(1e-2 / (1 + (i % 3)), weight_decay=wd, decoupled=decoupled, step=step)
            for i in range(n)]


def _check_segments(segs, devs, want, where):
    for i, (seg, (fp, fg, fm, fv), w) in enumerate(zip(segs, devs, want)):
        n = seg[0].size
        at = where + (i, n)
        for name, full, exp in (("param", fp, w[0]), ("exp_avg", fm, w[1]), ("exp_avg_sq", fv, w[2])):
            got = ag._host(full, "bf16")
            assert ag._same(got[:n], exp, "bf16"), (name,) + at
            assert (got[n:] == SENTINEL).all(), (name + " written beyond count",) + at
        assert ag._host(fg, "bf16").tobytes() == \
            np.concatenate([seg[1], np.full(PAD, SENTINEL, np.uint16)]).tobytes(), ("grad",) + at


@pytest.mark.parametrize("wd,decoupled", adam_cpu.ROWS)
@pytest.mark.parametrize("np_", [0, 2, 3])
def test_kernel_bit_exact(segments, np_, wd, decoupled):
    from kungfu_amd import ops
    segs, bases, streams = segments
    assert len({(wd_ != 0, dec) for wd_, dec in adam_cpu.ROWS}) == 3  # the three decay modes
    assert sum(1 for s in segs if s[0].size == 1) > SR_SEG
    hs = _hypers(len(segs), wd, decoupled)
    devs = [[_dev_padded(a) for a in seg] for seg in segs]
    views = [[d[j][1] for d in devs] for j in range(4)]
    ops.adam_sr_update_batch_(*views, hs, bases, streams, KEY, np_=np_)
    torch.cuda.synchronize()
    want = [ref.step(*seg, h, b, s, KEY, np_) for seg, h, b, s in zip(segs, hs, bases, streams)]
    _check_segments(segs, [[d[j][0] for j in range(4)] for d in devs], want, (np_, wd, decoupled))
    # the narrowing was stochastic somewhere: not the round-to-nearest bits
    big = max(range(len(segs)), key=lambda i: segs[i][0].size)
    rne = adam_ref.f32_to_bf16_bits(adam_ref.step(
        *[adam_ref.bf16_bits_to_f32(a) for a in segs[big]], "f32", hs[big], np_)[0])
    assert not np.array_equal(rne, want[big][0])


def _run(segs, hs, bases, streams, key=KEY, np_=0):
    from kungfu_amd import ops
    ts = [[ag._dev(a, "bf16") for a in seg] for seg in segs]
    ops.adam_sr_update_batch_(*[[t[j] for t in ts] for j in range(4)], hs, bases, streams, key,
                              np_=np_)
    torch.cuda.synchronize()
    return [[ag._host(t[j], "bf16") for j in (0, 2, 3)] for t in ts]


def test_split_invariance():
    """One segment of n elements against the same data as three segments
    with bases (0, a, a + b), in one launch and in separate launches."""
    n, a, b = SIZES[-1], 8 * 129, TILE + 8 * 7
    (seg,) = ag._fill("bf16", (n,))
    h = adam_ref.hyper(1e-2, weight_decay=1e-2, step=2)
    (whole,) = _run([seg], [h], [0], [77])
    cuts = ((0, a), (a, a + b), (a + b, n))
    parts = [tuple(x[lo:hi].copy() for x in seg) for lo, hi in cuts]
    together = _run(parts, [h] * 3, [lo for lo, _ in cuts], [77] * 3)
    apart = [_run([p], [h], [lo], [77])[0] for p, (lo, _) in zip(parts, cuts)]
    want = ref.step(*seg, h, 0, 77, KEY)
    for j in range(3):
        assert whole[j].tobytes() == want[j].tobytes(), j
        for got in (together, apart):
            assert np.concatenate([g[j] for g in got]).tobytes() == whole[j].tobytes(), j
    # another stream word or key: other bits
    (other,) = _run([seg], [h], [0], [78])
    (later,) = _run([seg], [h], [0], [77], key=KEY + 1)
    assert other[0].tobytes() != whole[0].tobytes() and later[0].tobytes() != whole[0].tobytes()


def test_high_bases():
    """The base is only a number: the last 4096 elements below 2^33, and a
    segment that crosses element 2^32."""
    cases = (((1 << 33) - 4096, 4096), ((1 << 32) - 8, 8 + 1000 + 3))
    segs = ag._fill("bf16", tuple(n for _, n in cases))
    hs = _hypers(len(segs), 0.0, False)
    got = _run(segs, hs, [b for b, _ in cases], [5, 6])
    for seg, h, (base, n), s, g in zip(segs, hs, cases, (5, 6), got):
        want = ref.step(*seg, h, base, s, KEY)
        for j in range(3):
            assert ag._same(g[j], want[j], "bf16"), (base, j)
        # what an element index cut to 32 bits would have given is something else
        cut = (1 << 32) - (base & 0xFFFFFFFF) if base < (1 << 32) else 0
        low = [ref.step(*[a[lo:hi] for a in seg], h, (base + lo) & 0xFFFFFFFF, s, KEY)[0]
               for lo, hi in ((0, cut), (cut, n))]
        assert not np.array_equal(np.concatenate(low), want[0]), (base, "the reference ignores bit 32")


def _gate_tensors(gate, state):
    from kungfu_amd import ops
    g, st = ops.new_step_gate("cuda"), ops.new_step_states("cuda", 2)
    gated.write_gate(g, gate)
    gated.write_states(st, [step_gate_ref.new_state(), state])
    return g, st


@pytest.mark.parametrize("skip", [0, 1])
def test_gated_kernel(segments, skip):
    """Applied: grad_mul, s2 and nss are the device's. Skipped: every byte of
    p, m and v (and of g) stays."""
    from kungfu_amd import ops
    segs, bases, streams = segments
    h = adam_ref.hyper(1e-2, weight_decay=1e-2, decoupled=True, step=5)
    gate = dict(step_gate_ref.new_gate(), skip=skip, grad_mul=np.float32(0.37))
    state = step_gate_ref.scalars_of(h)
    g_t, st_t = _gate_tensors(gate, state)
    devs = [[_dev_padded(a) for a in seg] for seg in segs]
    views = [[d[j][1] for d in devs] for j in range(4)]
    ops.adam_sr_update_batch_gated_(*views, h, g_t, st_t, bases, streams, KEY, group=1, np_=3)
    torch.cuda.synchronize()
    want = [ref.step_gated(*seg, h, gate, state, b, s, KEY, 3)
            for seg, b, s in zip(segs, bases, streams)]
    fulls = [[d[j][0] for j in range(4)] for d in devs]
    _check_segments(segs, fulls, want, ("gated", skip))
    if skip:
        for seg, full in zip(segs, fulls):
            for a, t in zip(seg, full):
                assert ag._host(t, "bf16")[:a.size].tobytes() == a.tobytes()
    else:
        big = max(range(len(segs)), key=lambda i: segs[i][0].size)
        plain = ref.step(*segs[big], h, bases[big], streams[big], KEY, 3)
        assert not np.array_equal(plain[0], want[big][0])  # grad_mul took part


def test_narrowing_sweep():
    """The kernels' narrowing on all 65,536 high halves x five low halves x
    five random words, against sr(). The kernels narrow two values at a time,
    one to each half of a word: the grid runs twice, the second time moved on
    by one element, so that every case meets both halves."""
    from kungfu_amd import ops
    marks = np.array([0, 1, 0x7FFF, 0x8000, 0xFFFF], np.uint32)
    hi = np.arange(65536, dtype=np.uint32)
    x = ((hi[:, None, None] << 16) | marks[None, :, None]) + np.zeros((1, 1, 5), np.uint32)
    r = np.zeros((65536, 5, 1), np.uint32) + marks[None, None, :]
    x, r = np.ascontiguousarray(x).reshape(-1), np.ascontiguousarray(r).reshape(-1)
    assert x.size == r.size == 65536 * 25
    want = ref.sr(x.view(np.float32), r)
    for shift in (0, 1):
        xs, rs = np.concatenate([x[:shift], x]), np.concatenate([r[:shift], r])
        got = ops.adam_sr_narrow(torch.from_numpy(xs.view(np.int32)).cuda(),
                                 torch.from_numpy(rs.astype(np.uint16).view(np.int16)).cuda())
        got = got.cpu().numpy().view(np.uint16)[shift:]
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, [(shift, hex(int(x[i])), hex(int(r[i])), hex(int(got[i])),
                                hex(int(want[i]))) for i in bad[:8]]


# ---- the whole step -------------------------------------------------------------------

@pytest.mark.parametrize("world", [2, 3])
def test_whole_step_over_loopback(world):
    """tests/test_sharded_adam_sr.py's model (an f32 group beside a bf16 one)
    on the native exchange: the reference on the unsharded buckets, and the
    checkpoint round trip."""
    loopback.loop_ranks(world, lambda rank, ex: cpu.body_sharded(rank, world, lambda: ex, "cuda"))


def test_whole_step_gated_over_loopback():
    loopback.loop_ranks(2, lambda rank, ex: cpu.body_sharded(rank, 2, lambda: ex, "cuda", gate=True))


@pytest.mark.parametrize("gate", [False, True])
def test_whole_step_world1_through_librccl(gate):
    ex = loopback.rccl1_exchange()
    cpu.body_sharded(0, 1, lambda: ex, "cuda", gate=gate)
    ex.close()
