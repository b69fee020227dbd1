"""Every update entry captured into a graph and replayed (tests/capture.py):
the ungated entries over three replays on evolving state, the gated chains of
a world-1 Adam and LAMB step over six replays with the gate, the loss scale
and the step states left on the device in between, and the C entries with
their host tables overwritten after capture. A replay must give the bits of
an eager twin that made the same calls, and those of the CPU references
(tests/test_capture_replay.py holds the chains' builders)."""
import ctypes

import numpy as np
import pytest
import torch

import capture as cap
import lamb_ref
import monitor_ref
import step_gate_ref
import test_capture_replay as cr
from test_monitor_gpu import check_bound

pytestmark = pytest.mark.gpu

_F16, _BF16 = torch.float16, torch.bfloat16


def _same_scalar(a, b):
    a = np.asarray(a)
    b = np.asarray(b).astype(a.dtype)
    if a.dtype.kind == "f" and np.isnan(a) and np.isnan(b):
        return True
    return a.tobytes() == b.tobytes()


def _gate_bytes(scale):
    from kungfu_amd import _lib
    a = np.zeros(1, _lib.step_gate_dtype())
    a["loss_scale"] = scale
    return a.view(np.uint8)


def _state_bytes(states):
    from kungfu_amd import _lib
    a = np.zeros(len(states), _lib.step_state_dtype())
    for j, st in enumerate(states):
        for k in step_gate_ref.STATE_FIELDS:
            a[k][j] = st[k]
    return a.view(np.uint8)


def _check_gate(side, gate, states, where):
    from kungfu_amd import _lib
    got_g = cap.host(side.gate, np.uint8).view(_lib.step_gate_dtype())[0]
    got_s = cap.host(side.states, np.uint8).view(_lib.step_state_dtype())
    for k in step_gate_ref.GATE_FIELDS:
        assert _same_scalar(got_g[k], gate[k]), ("gate", k, got_g[k], gate[k]) + where
    for j, st in enumerate(states):
        for k in step_gate_ref.STATE_FIELDS:
            assert _same_scalar(got_s[k][j], st[k]), ("state", k, j, got_s[k][j], st[k]) + where


def _check_sq(got, segs, dt, where):
    """A norm run's nseg + 1 values: every segment within the documented bound
    of the exact sum (tests/test_monitor_gpu.py's check_bound), the total their
    left-to-right sum."""
    nseg = len(segs)
    assert got.shape == (nseg + 1,)
    for k, seg in enumerate(segs):
        want = monitor_ref.exact_sq(seg, dt)
        if np.isfinite(want):
            check_bound(float(got[k]), want, seg.size, "%s sq seg %d" % (where, k))
        else:
            assert got[k] == want, (where, k, got[k])
    with np.errstate(invalid="ignore", over="ignore"):
        assert _same_scalar(got[nseg], monitor_ref.left_sum(got[:nseg])), where


def _check_cols(side, cols, where):
    for c, arrays in cols.items():
        for i, (t, want) in enumerate(zip(side.cols[c], arrays)):
            got = cap.host(t, want.dtype)
            assert got.tobytes() == np.ascontiguousarray(want).tobytes(), (c, i, want.size) + where


def _moved(before, after, names, keep):
    """The names of the buffers outside `keep` whose bytes changed."""
    return [n for a, b, n in zip(before, after, names)
            if a.tobytes() != b.tobytes() and not n.startswith(keep)]


# ---- 2. the ungated entries: three replays on evolving state ---------------------------

NP_ = 3  # what the gradients are still to be divided by


def _layout(segs, rows, kernel):
    """A family's own segments arranged so that one call reaches every branch:
    an empty segment, then as many of `segs` as fill one launch's table (the
    family's ragged last tile among them), then `rows` (equal segments of more
    than a tile) with six more of `segs`: a second launch, on the rows grid.
    kernel = (unit, tile_units, nseg) of large_launch.update_plan."""
    import large_launch as ll
    nseg = kernel[2]
    live = [s for s in segs if s[0].size]
    assert len(live) >= nseg + 6
    empty = tuple(a[:0].copy() for a in live[0])
    out = [empty] + live[:nseg] + list(rows) + live[nseg:nseg + 6]
    counts = [s[0].size for s in out]
    plans = ll.update_plan(counts, *kernel)
    assert sum(1 for n in counts if n) > nseg and len(plans) >= 2  # at least two kernel nodes
    assert any(r and widest > 1 for r, widest, _ in plans), plans   # one of them a rows grid
    tile = kernel[0] * kernel[1]
    assert any(n > tile and n % tile for n in counts)               # a ragged last tile
    return out


def _rolled(gs, j):
    """The gradients of replay j: replay 1 has the family's own."""
    return [np.roll(g, 7 * (j - 1)) for g in gs]


class Side:
    """A side whose build(side, bufs) sets `cols` (name -> views) and run(stream)."""

    def __init__(self, build):
        self.bufs = cap.Guarded()
        build(self, self.bufs)

    def feed(self, gs):
        for t, g in zip(self.cols["g"], gs):
            cap.put(t, g)

    def work(self, stream):
        self.run(stream)


def _three_replays(build, gs, check_first, where=()):
    twins = cap.Twins(lambda: Side(build))
    for j in (1, 2, 3):
        twins.feed(lambda side: side.feed(_rolled(gs, j)))
        if j == 1:
            twins.capture()
        before = twins.cap.bufs.bytes()
        twins.replay(where)
        assert not cap.same_bytes(before, twins.cap.bufs.bytes()), ("nothing moved", j) + where
        if j == 1:
            check_first(twins.cap)
    return twins


def _update_case(names, arrays, dtypes, op_cols, call):
    """build() for a batched update: arrays[name] per segment, uploaded as
    dtypes.get(name); call(tables, stream) with the tables in op_cols' order."""
    def build(side, b):
        side.cols = {c: b.add_all(arrays[c], dtypes.get(c), name=c) for c in names}
        tables = [side.cols[c] for c in op_cols]
        side.run = lambda stream: call(tables, stream)
    return build


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_sgd_update_replays(dt):
    import large_launch as ll
    import sgd_ref
    import test_sharded_sgd_gpu as sg
    from kungfu_amd import ops
    unit = ll.epv(dt)
    n = 2 * ll.TILE * unit + 3
    rows = [tuple(sg._random(dt, n, 50 + 3 * i + j) for j in range(3)) for i in range(3)]
    segs = _layout(sg._segments(dt), rows, (unit, ll.TILE, ll.SGD_SEG))
    hs = [sgd_ref.hyper(0.1 / (1 + (i % 3)), 0.9, 0.0, 1e-2, i % 2 == 0, False)
          for i in range(len(segs))]
    arrays = {c: [s[j] for s in segs] for j, c in enumerate("pgm")}
    build = _update_case("pgm", arrays, {}, "pgm", lambda t, stream: ops.sgd_update_batch_(
        t[0], t[1], t[2], hs, np_=NP_, stream=stream))

    def check(side):
        for i, ((p, g, m), h) in enumerate(zip(segs, hs)):
            wp, wm = sgd_ref.step(p, g, m, dt, h, NP_)
            assert sg._same(cap.host(side.cols["p"][i], p.dtype), wp, dt), ("param", dt, i, p.size)
            assert sg._same(cap.host(side.cols["m"][i], m.dtype), wm, dt), ("momentum", dt, i)

    _three_replays(build, arrays["g"], check, (dt,))


def _adam_hypers(n, step=3):
    import adam_ref
    # a hyper of its own per segment: the lr and the decay mode differ
    return [adam_ref.hyper(1e-2 / (1 + (i % 3)), weight_decay=1e-2 if i % 3 else 0.0,
                           decoupled=i % 2 == 0, step=step) for i in range(n)]


@pytest.mark.parametrize("dt", ["f32", "bf16", "f64"])
def test_adam_update_replays(dt):
    import adam_ref
    import large_launch as ll
    import test_sharded_adam_gpu as ag
    from kungfu_amd import ops
    segs = _layout(ag._segments(dt), ag._rows_segments(dt), ll.UPDATE_KERNELS["adam-" + dt][1:])
    hs = _adam_hypers(len(segs))
    arrays = {c: [s[j] for s in segs] for j, c in enumerate("pgmv")}
    build = _update_case("pgmv", arrays, {}, "pgmv", lambda t, stream: ops.adam_update_batch_(
        *t, hs, np_=NP_, stream=stream))

    def check(side):
        for i, (seg, h) in enumerate(zip(segs, hs)):
            want = adam_ref.step(*seg, dt, h, NP_)
            for c, w in zip("pmv", want):
                assert ag._same(cap.host(side.cols[c][i], w.dtype), w, dt), (c, dt, i, seg[0].size)

    _three_replays(build, arrays["g"], check, (dt,))


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_adam_master_update_replays(dt):
    import adam_master_ref
    import large_launch as ll
    import test_sharded_adam_master_gpu as mg
    from kungfu_amd import ops
    segs = _layout(mg._segments(dt), mg._rows_segments(dt), ll.UPDATE_KERNELS["master-" + dt][1:])
    hs = _adam_hypers(len(segs))
    arrays = {c: [s[j] for s in segs] for j, c in enumerate("gwmv")}
    # the old 16-bit parameters are never read: any bits will do
    arrays["p16"] = [np.full(s[0].size, 0x4321, np.uint16).view(s[0].dtype) for s in segs]
    cols = ("p16", "g", "w", "m", "v")
    build = _update_case(cols, arrays, {}, cols, lambda t, stream: ops.adam_master_update_batch_(
        *t, hs, np_=NP_, stream=stream))

    def check(side):
        for i, (seg, h) in enumerate(zip(segs, hs)):
            wp, ww, wm, wv = adam_master_ref.step(seg[1], seg[0], seg[2], seg[3], dt, h, NP_)
            where = (dt, i, seg[0].size)
            assert mg._same16(cap.host(side.cols["p16"][i], wp.dtype), wp, dt), ("param",) + where
            for c, w in (("w", ww), ("m", wm), ("v", wv)):
                assert mg._same32(cap.host(side.cols[c][i], np.float32), w), (c,) + where

    _three_replays(build, arrays["g"], check, (dt,))


def test_adam_sr_update_replays():
    """The key is frozen at capture: every replay draws the same bits."""
    import adam_sr_ref
    import large_launch as ll
    import test_sharded_adam_gpu as ag
    import test_sharded_adam_sr_gpu as srg
    from kungfu_amd import ops
    kernel = ll.UPDATE_KERNELS["sr-bf16"][1:]
    rows = ag._fill("bf16", (2 * kernel[0] * kernel[1] + 3,) * 3)
    segs = _layout(srg._segments(), rows, kernel)
    hs = _adam_hypers(len(segs))
    bases = [8 * (1000 * i + 3) for i in range(len(segs))]
    words = [(0x01234567 * (i + 1)) & 0xFFFFFFFF for i in range(len(segs))]
    arrays = {c: [s[j] for s in segs] for j, c in enumerate("pgmv")}
    build = _update_case("pgmv", arrays, {}, "pgmv", lambda t, stream: ops.adam_sr_update_batch_(
        *t, hs, bases, words, srg.KEY, np_=NP_, stream=stream))
    def check(side):
        want = [adam_sr_ref.step(*seg, h, b, s, srg.KEY, NP_)
                for seg, h, b, s in zip(segs, hs, bases, words)]
        for i, w in enumerate(want):
            for c, x in zip("pmv", w):
                assert ag._same(cap.host(side.cols[c][i], np.uint16), x, "bf16"), (c, i, x.size)

    twins = _three_replays(build, arrays["g"], check)
    # the third replay is the reference's third step with that same key
    cur = [tuple(s) for s in segs]
    for j in (1, 2, 3):
        gs = _rolled(arrays["g"], j)
        cur = [(w[0], g, w[1], w[2]) for w, g in zip(
            [adam_sr_ref.step(p, g, m, v, h, b, s, srg.KEY, NP_)
             for (p, _, m, v), g, h, b, s in zip(cur, gs, hs, bases, words)], gs)]
    for i, (p, _, m, v) in enumerate(cur):
        for c, x in (("p", p), ("m", m), ("v", v)):
            assert ag._same(cap.host(twins.cap.cols[c][i], np.uint16), x, "bf16"), (c, i, "third")


@pytest.mark.parametrize("kind", ["f32", "bf16"])
def test_adam8_update_replays(kind):
    import test_sharded_adam8_gpu as a8
    from kungfu_amd import ops
    kernel = (4, a8.TILE // 4, a8.ADAM8_SEG)
    rows = a8._segments(kind, (2 * a8.TILE + 64,) * 3)
    segs = _layout(a8._segments(kind), rows, kernel)
    hs = _adam_hypers(len(segs))
    names = ("w" if kind != "f32" else "p", "g", "mc", "vc", "ms", "vs")
    arrays = {c: [s[j] for s in segs] for j, c in enumerate(names)}
    if kind == "f32":
        cols, fn = ("p", "g", "mc", "vc", "ms", "vs"), ops.adam8_update_batch_
    else:
        cols, fn = ("p16", "g", "w", "mc", "vc", "ms", "vs"), ops.adam8_master_update_batch_
        arrays["p16"] = [np.full(s[0].size, 0x4321, np.uint16) for s in segs]
    build = _update_case(cols, arrays, {}, cols,
                         lambda t, stream: fn(*t, hs, np_=NP_, stream=stream))

    def check(side):
        for i, (seg, h) in enumerate(zip(segs, hs)):
            want = a8._ref_step(seg, h, kind, NP_)
            where = (kind, i, seg[0].size)
            if kind != "f32":
                got16 = cap.host(side.cols["p16"][i], np.uint16)
                assert a8._same16(got16, want[0], kind), ("p16",) + where
                want = want[1:]
            got = {c: cap.host(side.cols[c][i], a.dtype) for c, a in zip(names, seg)}
            assert a8._same_f32(got[names[0]], want[0]), ("param",) + where
            assert np.array_equal(got["mc"], want[1]), ("exp_avg codes",) + where
            assert np.array_equal(got["vc"], want[2]), ("exp_avg_sq codes",) + where
            assert a8._same_f32(got["ms"], want[3]), ("exp_avg scales",) + where
            assert a8._same_f32(got["vs"], want[4]), ("exp_avg_sq scales",) + where

    _three_replays(build, arrays["g"], check, (kind,))


def test_adam8_codec_and_sr_narrow_replay():
    """adam8_quantize and adam8_dequantize with their results given, and
    adam_sr_narrow (whose result is the capture's own allocation)."""
    import adam8_ref
    import adam_sr_ref
    from kungfu_amd import ops
    n = 64 * 37
    rng = np.random.default_rng(21)
    xs = [(rng.standard_normal(n) * np.exp2(rng.integers(-30, 30, n))).astype(np.float32)
          for _ in range(3)]
    r = rng.integers(0, 65536, n).astype(np.uint16)

    def build(side, b):
        x = b.add(np.zeros(n, np.float32), name="x")
        mag = b.add(np.zeros(n, np.float32), name="|x|")  # table 1 holds exp_avg_sq: no sign
        side.cols = {"g": [x, mag]}
        src = (x, mag)
        codes = [b.add(np.zeros(n, np.uint8), name="codes%d" % w) for w in (0, 1)]
        scales = [b.add(np.zeros(n // 64, np.float32), name="scales%d" % w) for w in (0, 1)]
        outs = [b.add(np.zeros(n, np.float32), name="out%d" % w) for w in (0, 1)]
        xi, rr = x.view(torch.int32), b.add(r, torch.int16, name="r")
        side.outs = (codes, scales, outs)

        def run(stream):
            for w in (0, 1):
                ops.adam8_quantize(src[w], w, codes=codes[w], scales=scales[w], stream=stream)
                ops.adam8_dequantize(codes[w], scales[w], w, out=outs[w], stream=stream)
            side.narrowed = ops.adam_sr_narrow(xi, rr)
        side.run = run

    twins = cap.Twins(lambda: Side(build))
    for j, x in enumerate(xs):
        twins.feed(lambda side: side.feed([x, np.abs(x)]))
        if j == 0:
            twins.capture()
        twins.replay((j,))
        codes, scales, outs = twins.cap.outs
        for w in (0, 1):
            wc, ws = adam8_ref.quantize(np.abs(x) if w else x, w)
            assert np.array_equal(cap.host(codes[w], np.uint8), wc), (j, w)
            assert cap.host(scales[w], np.uint32).tobytes() == ws.view(np.uint32).tobytes(), (j, w)
            assert cap.host(outs[w], np.uint32).tobytes() == \
                adam8_ref.dequantize(wc, ws, w).view(np.uint32).tobytes(), (j, w)
        want = adam_sr_ref.sr(x, r)
        assert np.array_equal(cap.host(twins.cap.narrowed, np.uint16), want), j
        assert np.array_equal(cap.host(twins.eager.narrowed, np.uint16), want), j


@pytest.mark.parametrize("dt", ["f32", "f16"])
def test_lamb_step_replays(dt):
    """The ungated LAMB step in one graph: the moments pass (f32, or f16
    gradients on fp32 masters), the (p, u) norms, lamb_trust_update_ and
    LambApplyPlan.run."""
    import large_launch as ll
    import test_sharded_adam_gpu as ag
    import test_sharded_lamb_gpu as lg
    from kungfu_amd import ops
    master = dt != "f32"
    kernel = ll.UPDATE_KERNELS["lamb_master-f16" if master else "lamb-f32"][1:]
    rows = ag._fill("f32", (2 * kernel[0] * kernel[1] + 3,) * 3)
    segs = _layout(lg._segments("f32", kernel[2] + 8), rows, kernel)
    T = len(segs)
    hs = lg._hypers(T, 1e-2)
    group_of = np.array([t % 2 for t in range(T)], np.int32)
    groups = [{"lr": 1e-2, "adapt": True}, {"lr": 3e-3, "adapt": False}]
    arrays = {c: [s[j] for s in segs] for j, c in enumerate("pgmv")}
    if master:
        arrays["g"] = [lamb_ref.narrow16(g, dt) for g in arrays["g"]]
        arrays["p16"] = [np.full(s[0].size, 0x4321, np.uint16) for s in segs]
    arrays["u"] = [np.full(s[0].size, 7.0, np.float32) for s in segs]

    def build(side, b):
        names = ("p", "g", "m", "v", "u") + (("p16",) if master else ())
        side.cols = c = {k: b.add_all(arrays[k], _F16 if master and k in ("g", "p16") else None,
                                      name=k) for k in names}
        side.sq = b.add(np.zeros(2 * T + 1), name="sq")
        side.nlr, side.ratio = b.add(np.full(T, 9.0), name="nlr"), b.add(np.full(T, 9.0), name="ratio")
        dgo = b.add(group_of, name="group_of")
        side.norm = ops.SegNorm(c["p"] + c["u"])
        side.apply = ops.LambApplyPlan(c["p"], c["u"], range(T), T, c["p16"] if master else None)
        sums = side.sq[:2 * T]

        def run(stream):
            if master:
                ops.lamb_master_moments_batch_(c["g"], c["p"], c["m"], c["v"], c["u"], hs, np_=NP_,
                                               stream=stream)
            else:
                ops.lamb_moments_batch_(c["p"], c["g"], c["m"], c["v"], c["u"], hs, np_=NP_,
                                        stream=stream)
            side.norm.run("sq", out=side.sq, stream=stream)
            ops.lamb_trust_update_(sums, 1, dgo, groups, side.nlr, side.ratio, trust_clip=1.5,
                                   stream=stream)
            side.apply.run(side.nlr, stream=stream)
        side.run = run

    def check(side):
        sums = cap.host(side.sq, np.float64)[:2 * T]
        nlr, ratio = lamb_ref.trust(sums.reshape(1, -1), [groups[j]["lr"] for j in group_of],
                                    [groups[j]["adapt"] for j in group_of], 1.5)
        assert lg._same(cap.host(side.nlr, np.float64), nlr), "nlr"
        assert lg._same(cap.host(side.ratio, np.float64), ratio), "ratio"
        for i, (seg, h) in enumerate(zip(segs, hs)):
            g = lamb_ref.widen16(arrays["g"][i], dt) if master else seg[1]
            wm, wv, wu = lamb_ref.moments(seg[0], g, seg[2], seg[3], "f32", h, NP_)
            wp = lamb_ref.apply(seg[0], wu, nlr[i], "f32")
            where = (dt, i, seg[0].size)
            for c, w in (("p", wp), ("m", wm), ("v", wv), ("u", wu)):
                assert lg._same(cap.host(side.cols[c][i], np.float32), w), (c,) + where
            if master:
                assert np.array_equal(cap.host(side.cols["p16"][i], np.uint16),
                                      lamb_ref.narrow16(wp, dt)), ("p16",) + where

    twins = _three_replays(build, arrays["g"], check, (dt,))
    for side in (twins.eager, twins.cap):
        side.norm.close()
        side.apply.close()


def test_sma_blend_batch_replays():
    """More buckets than one launch's 16, an empty one among them; after the
    first replay also the bits of one sma_blend_ per bucket."""
    import test_sharded_sgd_gpu as sg
    from kungfu_amd import ops
    sizes = (0, 1, 3, 1021, 4096, 100003) + (1,) * 17
    assert sum(1 for n in sizes if n) > 16
    vs = [sg._random("bf16", n, 300 + i) for i, n in enumerate(sizes)]
    sums = [sg._random("bf16", n, 400 + i) for i, n in enumerate(sizes)]

    def build(side, b):
        side.cols = c = {"v": b.add_all(vs, name="v"), "g": b.add_all(sums, name="sum")}
        side.run = lambda stream: ops.sma_blend_batch_(c["v"], c["g"], 4, 0.1, stream=stream)

    def check(side):
        for i, (v, s) in enumerate(zip(vs, sums)):
            if v.size:
                one = ops.sma_blend_(sg._dev(v, "bf16"), sg._dev(s, "bf16"), 4, 0.1)
                assert cap.host(side.cols["v"][i], np.uint16).tobytes() == \
                    sg._host(one, "bf16").tobytes(), (i, v.size)

    _three_replays(build, sums, check)


def test_noise_scale_update_replays():
    """The EMA state advances on the device from replay to replay."""
    from kungfu_amd import ops
    rng = np.random.default_rng(9)
    want = np.zeros(4, np.float32)

    def build(side, b):
        side.small, side.big = b.add(np.zeros(1), name="small"), b.add(np.zeros(1), name="big")
        side.state = b.add(np.zeros(4, np.float32), name="state")
        side.run = lambda stream: ops.noise_scale_update_(side.small, side.big, 32, 64, 0.9,
                                                          side.state, stream=stream)

    twins = cap.Twins(lambda: Side(build))
    for j in range(4):
        big = float(rng.uniform(0.5, 3.0))
        small = big + float(rng.uniform(0.01, 2.0))

        def feed(side):
            cap.put(side.small, np.array([small]))
            cap.put(side.big, np.array([big]))
        twins.feed(feed)
        if j == 0:
            twins.capture()
        twins.replay((j,))
        want = monitor_ref.noise_scale_step(want, small, big, 32, 64, 0.9)
        assert cap.host(twins.cap.state, np.float32).tobytes() == want.tobytes(), (j, want)


def test_pair_average_world1_replays():
    """publish, new values into the spans, pull: the device-side version
    counter advances with every replay, and every pull finds the version the
    same replay published."""
    import pairavg_ref
    import test_pairavg_gpu as pg
    from kungfu_amd.pairavg import PeerModelStore
    dt = "f32"
    sizes = pg.MANY

    class Store:
        def __init__(self):
            self.bufs = b = cap.Guarded()
            self.spans = b.add_all([pg._random(dt, n, 10 + i) for i, n in enumerate(sizes)],
                                   name="span")
            self.new = b.add_all([np.zeros(n, np.float32) for n in sizes], name="new")
            self.store = PeerModelStore(self.spans)

        def work(self, stream):
            self.store.publish()
            for t, x in zip(self.spans, self.new):
                t.copy_(x)
            self.store.pull_average_(0)

    twins = cap.Twins(Store)
    cur = [pg._random(dt, n, 10 + i) for i, n in enumerate(sizes)]
    try:
        for j in (1, 2, 3):
            new = [pg._random(dt, n, 500 * j + i) for i, n in enumerate(sizes)]

            def feed(side):
                for t, a in zip(side.new, new):
                    cap.put(t, a)
            twins.feed(feed)
            if j == 1:
                twins.capture()
                assert twins.cap.store.counters() == dict(valid=0, torn=0, empty=0, published=0)
            twins.replay((j,))
            cur = [pairavg_ref.blend(a, b, dt) for a, b in zip(new, cur)]
            for i, (t, w) in enumerate(zip(twins.cap.spans, cur)):
                assert pg._same(cap.host(t, np.float32), w, dt), (j, i, sizes[i])
            for side in (twins.eager, twins.cap):
                assert side.store.counters() == dict(valid=j, torn=0, empty=0, published=j)
    finally:
        twins.eager.store.close()
        twins.cap.store.close()


# ---- 3. the gated chains -------------------------------------------------------------

class AdamSide:
    """One side's buffers of a gated Adam chain and the step it queues:
    SegNorm.run -> step_gate_update_ -> the gated update."""

    def __init__(self, name):
        from kungfu_amd import ops
        self.kind, self.dt, self.group, sizes = cr.ADAM_CHAINS[name]
        self.bufs = b = cap.Guarded()
        first = cr.adam_initial(name)
        self.cols = {c: b.add_all(first[c], name=c) for c in first}
        gdt = np.float32 if self.kind == "adam8" else cr.store(np.zeros(1), self.dt).dtype
        self.gdt = "f32" if self.kind == "adam8" else self.dt
        self.cols["g"] = b.add_all([np.zeros(n, gdt) for n in sizes], name="g")
        self.nseg = len(sizes)
        self.sq = b.add(np.zeros(self.nseg + 1), name="sq")
        self.total = self.sq[self.nseg:]
        self.gate = b.add(_gate_bytes(cr.SCALE0), name="gate")
        self.states = b.add(_state_bytes([step_gate_ref.new_state() for _ in cr.GROUPS]),
                            name="states")
        self.plan = ops.SegNorm(self.cols["g"])
        self.fn = {"plain": ops.adam_update_batch_gated_,
                   "master": ops.adam_master_update_batch_gated_,
                   "sr": ops.adam_sr_update_batch_gated_,
                   "adam8": ops.adam8_update_batch_gated_,
                   "adam8m": ops.adam8_master_update_batch_gated_}[self.kind]
        self.tables = [self.cols[c] for c in cr.COLS[self.kind]]
        self.extra = list(cr.sr_words(name)) + [cr.SR_KEY] if self.kind == "sr" else []

    def feed(self, gs):
        for t, g in zip(self.cols["g"], gs):
            cap.put(t, g)

    def work(self, stream):
        from kungfu_amd import ops
        self.plan.run("sq", out=self.sq, stream=stream)
        ops.step_gate_update_(self.total, 1, [0], cr.GROUPS, self.states, self.gate,
                              max_norm=cr.MAX_NORM, stream=stream, **cr.RULE)
        self.fn(*self.tables, cr.hyper(self.group), self.gate, self.states, *self.extra,
                group=self.group, stream=stream)


def _chain(name, ref, make, check):
    """Six replays of one captured step against the reference and the eager
    twin; check(side, gs, where) looks at what the step's norm runs gave and
    advances the reference with it."""
    twins = cap.Twins(make)
    side = twins.cap
    for s in range(cr.STEPS):
        where = (name, s)
        assert ref.scale == cr.SCALES_IN_FORCE[s]
        gs = ref.grads()
        twins.feed(lambda x: x.feed(gs))
        if s == 0:
            twins.capture()
        before = side.bufs.bytes()
        twins.replay(where)
        after = side.bufs.bytes()
        check(side, gs, where)
        _check_gate(side, ref.gate, ref.states, where)
        assert float(ref.gate["loss_scale"]) == cr.SCALES_AFTER[s]
        moved = _moved(before, after, side.bufs.names, ("g[", "sq", "gate"))
        if s == cr.BAD:  # nothing but the gate (and the norms) has moved
            assert ref.gate["skip"] == 1 and ref.gate["skipped"] == 1
            assert moved == [], where
        else:
            assert ref.gate["skip"] == 0 and "states" in moved
    assert ref.gate["applied"] == cr.STEPS - 1 and ref.states[0]["step"] == cr.STEPS - 1
    return twins


@pytest.mark.parametrize("name", list(cr.ADAM_CHAINS))
def test_gated_adam_chain_replays(name):
    ref = cr.AdamChain(name)
    assert sum(1 for n in ref.sizes if n) > cr.SEG[name]  # the update is at least two launches

    def check(side, gs, where):
        sq = cap.host(side.sq, np.float64)
        _check_sq(sq, gs, side.gdt, where)
        ref.step(gs, float(sq[-1]))
        _check_cols(side, ref.cols, where)

    twins = _chain(name, ref, lambda: AdamSide(name), check)
    for side in (twins.eager, twins.cap):
        side.plan.close()


class LambSide:
    """One side of a gated LAMB chain: gradient norm -> gate with every group's
    lr = 1 -> gated moments, a call per group -> the (p, u) norms -> gated
    trust -> gated apply."""

    def __init__(self, name):
        from kungfu_amd import ops
        ref = cr.LambChain(name)
        self.dt, self.master, self.T = ref.dt, ref.master, ref.T
        self.bufs = b = cap.Guarded()
        self.cols = {c: b.add_all(ref.cols[c], name=c) for c in ("p", "m", "v", "u")}
        if self.master:
            self.cols["p16"] = b.add_all(ref.cols["p16"], dtype=_BF16, name="p16")
        gdt = cr.store(np.zeros(1), self.dt).dtype
        self.cols["g"] = b.add_all([np.zeros(n, gdt) for n in ref.sizes], name="g")
        T = self.T
        self.sqg = b.add(np.zeros(T + 1), name="sq_g")
        self.sqpu = b.add(np.zeros(2 * T + 1), name="sq_pu")
        self.nlr, self.ratio = b.add(ref.nlr, name="nlr"), b.add(ref.ratio, name="ratio")
        self.gate = b.add(_gate_bytes(cr.SCALE0), name="gate")
        self.states = b.add(_state_bytes([step_gate_ref.new_state() for _ in cr.GROUPS]),
                            name="states")
        self.group_of = b.add(np.array(ref.group_of, np.int32), name="group_of")
        self.gnorm = ops.SegNorm(self.cols["g"])
        self.punorm = ops.SegNorm(self.cols["p"] + self.cols["u"])
        self.apply = ops.LambApplyPlan(self.cols["p"], self.cols["u"], range(T), T,
                                       self.cols["p16"] if self.master else None)
        self.calls = []
        for grp in range(len(cr.GROUPS)):
            mine = [t for t in range(T) if ref.group_of[t] == grp]
            order = ("g", "p", "m", "v", "u") if self.master else ("p", "g", "m", "v", "u")
            self.calls.append((grp, [[self.cols[c][t] for t in mine] for c in order]))
        self.total, self.sums = self.sqg[T:], self.sqpu[:2 * T]

    def feed(self, gs):
        for t, g in zip(self.cols["g"], gs):
            cap.put(t, g)

    def work(self, stream):
        from kungfu_amd import ops
        self.gnorm.run("sq", out=self.sqg, stream=stream)
        ops.step_gate_update_(self.total, 1, [0], [dict(g, lr=1.0) for g in cr.GROUPS],
                              self.states, self.gate, max_norm=cr.MAX_NORM, stream=stream,
                              **cr.RULE)
        moments = ops.lamb_master_moments_batch_gated_ if self.master else \
            ops.lamb_moments_batch_gated_
        for grp, tables in self.calls:
            moments(*tables, cr.lamb_hyper(grp), self.gate, self.states, group=grp, stream=stream)
        self.punorm.run("sq", out=self.sqpu, stream=stream)
        groups = [{"lr": g["lr"], "adapt": cr.lamb_hyper(j)["adapt"]}
                  for j, g in enumerate(cr.GROUPS)]
        ops.lamb_trust_update_gated_(self.sums, 1, self.group_of, groups, self.nlr, self.ratio,
                                     self.gate, trust_clip=cr.TRUST_CLIP, stream=stream)
        self.apply.run(self.nlr, stream=stream, gate=self.gate)


@pytest.mark.parametrize("name", list(cr.LAMB_CHAINS))
def test_gated_lamb_chain_replays(name):
    ref = cr.LambChain(name)
    mine = [n for t, n in enumerate(ref.sizes) if ref.group_of[t] == 0 and n]
    assert len(mine) > cr.SEG[name]  # group 0's moments call is at least two launches

    def check(side, gs, where):
        T = ref.T
        sq = cap.host(side.sqg, np.float64)
        _check_sq(sq, gs, ref.dt, where)
        p_before = [p.copy() for p in ref.cols["p"]]
        sums = cap.host(side.sqpu, np.float64)
        ref.step(gs, float(sq[-1]), sums[:2 * T])
        # the sums the reference was fed, against the exact ones: of the
        # parameters before the apply pass and of the updates
        _check_sq(sums, p_before + ref.cols["u"], "f32", where + ("p, u",))
        _check_cols(side, ref.cols, where)
        assert cap.host(side.nlr, np.float64).tobytes() == ref.nlr.tobytes(), ("nlr",) + where
        assert cap.host(side.ratio, np.float64).tobytes() == ref.ratio.tobytes(), ("ratio",) + where

    twins = _chain(name, ref, lambda: LambSide(name), check)
    assert (ref.ratio != 5.0).all()
    for side in (twins.eager, twins.cap):
        for plan in (side.gnorm, side.punorm, side.apply):
            plan.close()


# ---- 4. host tables are dead after the call --------------------------------------------

class DirectSide:
    """A direct call of one C entry. build(side, bufs) makes the buffers and
    returns call(stream_ptr) -> (status, [every host array passed])."""

    def __init__(self, build):
        self.bufs = cap.Guarded()
        self.call = build(self, self.bufs)
        self.host = []

    def work(self, stream):
        sp = (stream or torch.cuda.current_stream()).cuda_stream
        rc, self.host = self.call(sp)
        assert rc == 0, rc


def _dead_tables(build, replays=2):
    twins = cap.Twins(lambda: DirectSide(build))
    twins.capture()
    arrays = twins.cap.host
    assert arrays and all(isinstance(a, ctypes.Array) for a in arrays)
    for a in arrays:
        ctypes.memset(a, 0xFF, ctypes.sizeof(a))
    first = twins.cap.bufs.bytes()
    for _ in range(replays):
        twins.replay()
    assert not cap.same_bytes(first, twins.cap.bufs.bytes())  # the replays did something
    return twins


def _ptrs(views):
    from kungfu_amd import _lib
    return _lib.ptr_array([v.data_ptr() for v in views])


def _counts(views):
    return (ctypes.c_size_t * len(views))(*[v.numel() for v in views])


def _adam_hyper_array(n, step=3):
    from kungfu_amd import _lib
    return _lib.adam_hyper_array([dict(cr.hyper(i % 2), lr=1e-2 / (1 + i % 3), step=step)
                                  for i in range(n)])


def test_sgd_host_tables_are_dead_after_the_call():
    from kungfu_amd import _lib
    import sgd_ref
    sizes = cr.ADAM_CHAINS["master-f16"][3]
    assert sum(1 for n in sizes if n) > 32

    def build(side, b):
        cols = [b.add_all([np.random.default_rng(100 * j + i).standard_normal(n).astype(np.float32)
                           for i, n in enumerate(sizes)], name=c) for j, c in enumerate("pgm")]
        lib = _lib.load()

        def call(sp):
            host = [_ptrs(c) for c in cols] + [_counts(cols[0]), _lib.sgd_hyper_array(
                [sgd_ref.hyper(0.1 / (1 + i % 3), 0.9, 0.0, 1e-2, i % 2 == 0) for i in range(len(sizes))])]
            rc = lib.kf_sgd_update_batch(host[0], host[1], host[2], host[3], len(sizes), cr.adam_cpu.F32,
                                         3, host[4], sp)
            return rc, host
        return call

    _dead_tables(build)


def _fixed_gate(b):
    """A gate and two step states as a verdict leaves them at step 5."""
    gate = _gate_bytes(1024.0).copy().view(_gate_dtype())
    gate["grad_mul"] = np.float32(0.37)
    states = [step_gate_ref.scalars_of(dict(cr.GROUPS[j], step=5)) for j in range(2)]
    return b.add(gate.view(np.uint8), name="gate"), b.add(_state_bytes(states), name="states")


def _gate_dtype():
    from kungfu_amd import _lib
    return _lib.step_gate_dtype()


def test_adam_gated_host_tables_are_dead_after_the_call():
    from kungfu_amd import _lib
    name = "adam-f32"
    sizes = cr.ADAM_CHAINS[name][3]
    gs = cr.grads(name, sizes, "f32", 0, 1.0)

    def build(side, b):
        first = dict(cr.adam_initial(name), g=gs)
        cols = [b.add_all(first[c], name=c) for c in cr.COLS["plain"]]
        gate, states = _fixed_gate(b)
        lib = _lib.load()

        def call(sp):
            host = [_ptrs(c) for c in cols] + [_counts(cols[0]),
                                                _lib.adam_hyper_array([dict(cr.hyper(1), step=1)])]
            rc = lib.kf_adam_update_batch_gated(
                *host[:4], host[4], len(sizes), cr.adam_cpu.F32, 2, host[5], gate.data_ptr(),
                states.data_ptr() + ctypes.sizeof(_lib.StepState), sp)
            return rc, host
        return call

    _dead_tables(build)


def test_adam_sr_host_tables_are_dead_after_the_call():
    from kungfu_amd import _lib
    name = "sr"
    sizes = cr.ADAM_CHAINS[name][3]
    gs = cr.grads(name, sizes, "bf16", 0, 1.0)
    bases, words = cr.sr_words(name)

    def build(side, b):
        first = dict(cr.adam_initial(name), g=gs)
        cols = [b.add_all(first[c], name=c) for c in cr.COLS["sr"]]
        lib = _lib.load()

        def call(sp):
            n = len(sizes)
            host = [_ptrs(c) for c in cols] + [_counts(cols[0]), (ctypes.c_uint64 * n)(*bases),
                                                (ctypes.c_uint32 * n)(*words), _adam_hyper_array(n)]
            rc = lib.kf_adam_sr_update_batch(*host[:7], n, cr.adam_cpu.BF16, 2, host[7], cr.SR_KEY,
                                             sp)
            return rc, host
        return call

    _dead_tables(build)


def test_adam8_host_tables_are_dead_after_the_call():
    from kungfu_amd import _lib
    name = "adam8"
    sizes = cr.ADAM_CHAINS[name][3]
    gs = cr.grads(name, sizes, "f32", 0, 1.0)

    def build(side, b):
        first = dict(cr.adam_initial(name), g=gs)
        cols = [b.add_all(first[c], name=c) for c in cr.COLS["adam8"]]
        lib = _lib.load()

        def call(sp):
            n = len(sizes)
            host = [_ptrs(c) for c in cols] + [_counts(cols[0]), _adam_hyper_array(n)]
            rc = lib.kf_adam8_update_batch(*host[:7], n, cr.adam_cpu.F32, 2, host[7], sp)
            return rc, host
        return call

    _dead_tables(build)


def test_step_gate_host_tables_are_dead_after_the_call():
    """More plans than one launch's 64 and more groups than its 16."""
    from kungfu_amd import _lib
    nplan, ngroup, world = 150, 37, 2
    rng = np.random.default_rng(5)
    nps = [int(x) for x in rng.integers(0, 4, nplan)]
    sq = rng.uniform(0.0, 2.0, (world, nplan))

    def build(side, b):
        dsq = b.add(sq, name="sq")
        gate = b.add(_gate_bytes(8.0), name="gate")
        states = b.add(_state_bytes([step_gate_ref.new_state() for _ in range(ngroup)]),
                       name="states")
        side.gate, side.states = gate, states
        lib = _lib.load()

        def call(sp):
            garr = (_lib.StepGroup * ngroup)()
            for j, a in enumerate(garr):
                a.lr, a.beta1, a.beta2 = 1e-3 * (j + 1), 0.9 - 0.01 * j, 0.999 - 0.001 * j
            host = [(ctypes.c_int * nplan)(*nps), garr]
            rc = lib.kf_step_gate_update(dsq.data_ptr(), world, nplan, host[0], host[1],
                                         states.data_ptr(), ngroup, 0.5, 2.0, 0.5, 2,
                                         gate.data_ptr(), sp)
            return rc, host
        return call

    twins = _dead_tables(build, replays=3)
    # and the replays are the reference's three verdicts
    groups = [{"lr": 1e-3 * (j + 1), "betas": (0.9 - 0.01 * j, 0.999 - 0.001 * j)}
              for j in range(ngroup)]
    g, states = step_gate_ref.new_gate(8.0), [step_gate_ref.new_state() for _ in groups]
    for _ in range(3):
        step_gate_ref.gate_update(sq, nps, groups, states, g, max_norm=0.5, growth_factor=2.0,
                                  backoff_factor=0.5, growth_interval=2)
    _check_gate(twins.cap, g, states, ("three replays",))
    assert g["applied"] == 3 and float(g["loss_scale"]) == 16.0


def test_lamb_trust_host_tables_are_dead_after_the_call():
    """More groups than one launch's 16."""
    from kungfu_amd import _lib
    T, ngroup, world = 300, 20, 2
    rng = np.random.default_rng(7)
    sq = np.exp2(rng.uniform(-40, 40, (world, 2 * T)))
    group_of = rng.integers(0, ngroup, T).astype(np.int32)
    assert set(group_of) == set(range(ngroup))
    groups = [(1e-3 * (j + 1), j % 2 == 0) for j in range(ngroup)]

    def build(side, b):
        dsq, dgo = b.add(sq, name="sq"), b.add(group_of, name="group_of")
        nlr, ratio = b.add(np.full(T, 9.0), name="nlr"), b.add(np.full(T, 9.0), name="ratio")
        side.nlr, side.ratio = nlr, ratio
        lib = _lib.load()

        def call(sp):
            garr = (_lib.LambGroup * ngroup)()
            for a, (lr, adapt) in zip(garr, groups):
                a.lr, a.adapt = lr, int(adapt)
            rc = lib.kf_lamb_trust_update(dsq.data_ptr(), world, T, dgo.data_ptr(), garr, ngroup,
                                          1.5, nlr.data_ptr(), ratio.data_ptr(), sp)
            return rc, [garr]
        return call

    twins = cap.Twins(lambda: DirectSide(build))
    twins.capture()
    for a in twins.cap.host:
        ctypes.memset(a, 0xFF, ctypes.sizeof(a))
    twins.replay()
    want_nlr, want_ratio = lamb_ref.trust(sq, [groups[j][0] for j in group_of],
                                          [groups[j][1] for j in group_of], 1.5)
    assert cap.host(twins.cap.nlr, np.float64).tobytes() == want_nlr.tobytes()
    assert cap.host(twins.cap.ratio, np.float64).tobytes() == want_ratio.tobytes()
