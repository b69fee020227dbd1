"""The 8-bit block-wise Adam state on the GPU, bit for bit against
tests/adam8_ref.py: the update kernels, their gated and master twins, the
quantizer alone over its table's every boundary, and
ShardedAdamOptimizer(state_bits=8) end to end over the loopback transport and
a one-rank librccl communicator."""
import numpy as np
import pytest
import torch

import adam8_cpu as cpu
import adam8_ref as ref
import adam_ref
import loopback
import step_gate_ref
import sweep16
import test_sharded_adam as adam_cpu
import test_sharded_adam8 as cpu_tests
import test_sharded_adam_gated as gated

pytestmark = pytest.mark.gpu

# kf_adam8.hip's launch shape: 256 lanes, one unit of 4 elements per lane and tile
ADAM8_SEG = cpu_tests.ADAM8_SEG
TILE = cpu_tests.TILE
SIZES = (0, 64, 128, 64 * 15, 64 * 16, TILE - 64, TILE, TILE + 64, 2 * TILE + 64 * 37)
N_SMALL = ADAM8_SEG + 8   # with SIZES: more segments than one launch's table
PAD = 64                  # elements (and code bytes) beyond `count` that must keep their bytes
PAD_SCALES = 4
SENT8, SENT16, SENT32 = 0x5A, 0x5A5A, 0x5A5A5A5A
NP16 = {"bf16": np.uint16, "f16": np.float16}


def _dev(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint16:
        return torch.from_numpy(a.view(np.int16).copy()).view(torch.bfloat16).cuda()
    return torch.from_numpy(a.copy()).cuda()


def _host(t):
    t = t.detach().cpu().contiguous()
    if t.dtype == torch.bfloat16:
        return t.view(torch.int16).numpy().view(np.uint16).copy()
    return t.numpy().copy()


def _padded(a):
    """(the whole buffer, the segment's view): sentinel bytes follow the data."""
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint8:
        pad = np.full(PAD, SENT8, np.uint8)
    elif a.dtype == np.float32:
        pad = np.full(PAD, SENT32, np.uint32).view(np.float32)
    else:
        pad = np.full(PAD, SENT16, np.uint16).view(a.dtype)
    full = _dev(np.concatenate([a, pad]))
    assert full.data_ptr() % 16 == 0
    return full, full[:a.size]


def _padded_scales(a):
    full = _dev(np.concatenate([a, np.full(PAD_SCALES, SENT32, np.uint32).view(np.float32)]))
    return full, full[:a.size]


def _tail_is_sentinel(full, n):
    raw = _host(full)[n:]
    return bool((raw.view(np.uint8) == SENT8).all())


def _same_f32(got, want):
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    return sweep16.mismatches_float(got, want).size == 0


def _same16(got, want, kind):
    got, want = (np.ascontiguousarray(x).view(np.uint16) for x in (got, want))
    return sweep16.mismatches(kind, got, want).size == 0


def _binades(rng, n, lo, hi, signed):
    """n values (a multiple of 64): every block has a binade of its own from
    [lo, hi) for its largest elements, and its elements are spread over the
    table's seven decades below it, so that a block uses codes of every
    decade."""
    k = np.repeat(rng.integers(lo, hi, n // 64), 64)
    x = np.ldexp(rng.uniform(1.0, 2.0, n) * 10.0 ** -rng.uniform(0, 7, n), k).astype(np.float32)
    return x * rng.choice([-1.0, 1.0], n).astype(np.float32) if signed else x


def _segment(n, seed, kind="f32"):
    """(p or master, g, mc, vc, ms, vs): random parameters and gradients, the
    previous state ref.quantize of random m / v over every binade."""
    rng = np.random.default_rng(seed)
    p = rng.standard_normal(n).astype(np.float32)
    g = (rng.standard_normal(n) * np.exp(rng.uniform(-6, 2, n))).astype(np.float32)
    mc, ms = ref.quantize(_binades(rng, n, -60, 30, True), ref.SIGNED)
    vc, vs = ref.quantize(_binades(rng, n, -100, 40, False), ref.UNSIGNED)
    return [p, cpu.narrow(g, kind), mc, vc, ms, vs]


def _segments(kind="f32", sizes=None):
    sizes = SIZES + (64,) * N_SMALL if sizes is None else sizes
    return [_segment(n, 100 + i, kind) for i, n in enumerate(sizes)]


def _hypers(n, wd, decoupled, step=3):
    # a hyper of its own per segment: the lr differs
    return [adam_ref.hyper(1e-2 / (1 + (i % 3)), weight_decay=wd, decoupled=decoupled, step=step)
            for i in range(n)]


def _upload(segs, kind):
    """Per segment the device buffers [(full, view)] in the order p16 (master
    kinds only), g, p / master, mc, vc, ms, vs."""
    out = []
    for p, g, mc, vc, ms, vs in segs:
        row = []
        if kind != "f32":
            row.append(_padded(np.full(p.size, SENT16, np.uint16).view(NP16[kind])))
        row += [_padded(g), _padded(p), _padded(mc), _padded(vc), _padded_scales(ms),
                _padded_scales(vs)]
        out.append(row)
    return out


def _views(devs, kind):
    """The argument lists of ops.adam8_[master_]update_batch[_gated]_."""
    cols = list(zip(*[[v for _, v in row] for row in devs]))
    if kind == "f32":
        g, p, mc, vc, ms, vs = cols
        return [p, g, mc, vc, ms, vs]
    p16, g, w, mc, vc, ms, vs = cols
    return [p16, g, w, mc, vc, ms, vs]


def _check(segs, devs, want, kind, where, skipped=False):
    """want[i] = (p', mc', vc', ms', vs') or, for a master kind, (p16', w',
    ...). Nothing beyond the counts was written and the gradients kept their
    bytes."""
    for i, (seg, row, w) in enumerate(zip(segs, devs, want)):
        n = seg[0].size
        at = where + (i, n)
        if kind != "f32":
            full16, row = row[0][0], row[1:]
            got16 = _host(full16)
            if skipped or w[0] is None:
                assert (got16.view(np.uint16) == SENT16).all(), ("p16 written on a skip",) + at
            else:
                assert _same16(got16[:n], w[0], kind), ("p16",) + at
                assert _same16(got16[:n], cpu.narrow(_host(row[1][0])[:n], kind), kind), \
                    ("p16 is not the narrowed master",) + at
            assert _tail_is_sentinel(full16, n), ("p16 written beyond count",) + at
            w = w[1:]
        (fg, _), (fp, _), (fmc, _), (fvc, _), (fms, _), (fvs, _) = row
        assert _host(fg)[:n].tobytes() == np.ascontiguousarray(seg[1]).tobytes(), ("grad",) + at
        assert _same_f32(_host(fp)[:n], w[0]), ("param",) + at
        assert np.array_equal(_host(fmc)[:n], w[1]), ("exp_avg codes",) + at
        assert np.array_equal(_host(fvc)[:n], w[2]), ("exp_avg_sq codes",) + at
        assert _same_f32(_host(fms)[:n // 64], w[3]), ("exp_avg scales",) + at
        assert _same_f32(_host(fvs)[:n // 64], w[4]), ("exp_avg_sq scales",) + at
        for name, full, m in (("grad", fg, n), ("param", fp, n), ("exp_avg codes", fmc, n),
                              ("exp_avg_sq codes", fvc, n), ("exp_avg scales", fms, n // 64),
                              ("exp_avg_sq scales", fvs, n // 64)):
            assert _tail_is_sentinel(full, m), (name + " written beyond count",) + at


def _ref_step(seg, h, kind, np_):
    p, g, mc, vc, ms, vs = seg
    if kind == "f32":
        return ref.step(p, g, mc, vc, ms, vs, h, np_)
    return ref.step_master(p, g, mc, vc, ms, vs, kind, h, np_)


@pytest.fixture(scope="module")
def segments():
    return {"f32": _segments("f32")}


@pytest.mark.parametrize("wd,decoupled", adam_cpu.ROWS)
@pytest.mark.parametrize("np_", [0, 2, 3])
def test_kernel_bit_exact(segments, np_, wd, decoupled):
    """SIZES and N_SMALL blocks alone: two launches, a 1-D grid with its
    search table. Per-segment hypers, sentinels beyond every count."""
    from kungfu_amd import ops
    segs = segments["f32"]
    assert sum(1 for s in segs if s[0].size) > ADAM8_SEG
    hs = _hypers(len(segs), wd, decoupled)
    devs = _upload(segs, "f32")
    ops.adam8_update_batch_(*_views(devs, "f32"), hs, np_=np_)
    torch.cuda.synchronize()
    want = [_ref_step(seg, h, "f32", np_) for seg, h in zip(segs, hs)]
    _check(segs, devs, want, "f32", (np_, wd, decoupled))
    # the data is worth the comparison: the largest segment's previous state
    # uses most codes of both tables, and the step moved it
    big = max(range(len(segs)), key=lambda i: segs[i][0].size)
    assert np.unique(segs[big][2]).size > 200 and np.unique(segs[big][3]).size > 200
    assert not np.array_equal(want[big][1], segs[big][2])


def test_rows_grid():
    """Five equal segments of TILE + 64: plan_update_batch's rows grid, two
    blocks a row, the second with one row of lanes at work."""
    from kungfu_amd import ops
    import large_launch
    counts = [TILE + 64] * 5
    (rows, widest, _), = large_launch.update_plan(counts, 4, TILE // 4, ADAM8_SEG)
    assert rows and widest == 2
    segs = _segments("f32", tuple(counts))
    hs = _hypers(5, 1e-2, True)
    devs = _upload(segs, "f32")
    ops.adam8_update_batch_(*_views(devs, "f32"), hs, np_=2)
    torch.cuda.synchronize()
    _check(segs, devs, [_ref_step(s, h, "f32", 2) for s, h in zip(segs, hs)], "f32", ("rows",))


# ---- blocks chosen to break the reduction ----------------------------------------

def _reduction_blocks():
    """(name, block of 64 f32 values)."""
    rng = np.random.default_rng(9)
    small = (rng.standard_normal(64) * 0.25).astype(np.float32)
    out = [("zeros", np.zeros(64, np.float32))]
    for pos in (0, 15, 16, 63):
        b = np.zeros(64, np.float32)
        b[pos] = -3.5 if pos % 2 else 2.25
        out.append(("single@%d" % pos, b))
    b = small.copy()
    b[5], b[40] = -2.0, 2.0
    out.append(("both signs of mag", b))
    b = small.copy()
    b[41] = -2.0
    out.append(("only -mag", b))
    out.append(("all equal", np.full(64, -0.75, np.float32)))
    out.append(("all equal +", np.full(64, 0.75, np.float32)))
    b = small.copy()
    b[33] = np.nan
    out.append(("one NaN", b))
    b = small.copy()
    b[17] = np.inf
    out.append(("one +inf", b))
    b = small.copy()
    b[62] = -np.inf
    out.append(("-inf and finite", b))
    b = small.copy()
    b[3] = 3e22   # its square times 1e-3 overflows f32
    out.append(("v overflows", b))
    b = np.zeros(64, np.float32)
    b[7] = -0.0
    out.append(("a -0 alone", b))
    return out


def test_reduction_blocks_through_the_quantizer():
    from kungfu_amd import ops
    blocks = _reduction_blocks()
    x = np.concatenate([b for _, b in blocks])
    for which in (ref.SIGNED, ref.UNSIGNED):
        src = x if which == ref.SIGNED else np.abs(x)
        codes, scales = ops.adam8_quantize(_dev(src), which)
        torch.cuda.synchronize()
        wc, ws = ref.quantize(src, which)
        got_c, got_s = _host(codes), _host(scales)
        for i, (name, _) in enumerate(blocks):
            assert got_s[i:i + 1].view(np.uint32)[0] == ws[i:i + 1].view(np.uint32)[0], \
                (name, which, got_s[i], ws[i])
            assert np.array_equal(got_c[64 * i:64 * i + 64], wc[64 * i:64 * i + 64]), (name, which)
    # the contract's own statements, on the reference's scales
    s = dict(zip([n for n, _ in blocks], ref.quantize(x, ref.SIGNED)[1]))
    assert s["both signs of mag"] == 2.0 and s["only -mag"] == -2.0
    assert s["all equal"] == -0.75 and s["zeros"] == 0 and not np.signbit(s["a -0 alone"])
    assert np.isnan(s["one NaN"]) and s["one +inf"] == np.inf and s["-inf and finite"] == -np.inf
    assert np.array([s["one NaN"]], np.float32).view(np.uint32)[0] == ref.NAN_BITS


@pytest.mark.parametrize("wd,decoupled", [(1e-2, False)])
def test_reduction_blocks_through_the_update(wd, decoupled):
    """The blocks as gradients on a zeroed state: the new exp_avg is c1 * g
    and the new exp_avg_sq c2 * g * g (plus the decay's share), block by
    block, and the one large gradient makes exp_avg_sq overflow."""
    from kungfu_amd import ops
    blocks = _reduction_blocks()
    n = 64 * len(blocks)
    g = np.concatenate([b for _, b in blocks])
    p = np.random.default_rng(4).standard_normal(n).astype(np.float32)
    seg = [p, g] + [x for w in (ref.SIGNED, ref.UNSIGNED) for x in ref.zero_state(n, w)]
    seg = [seg[0], seg[1], seg[2], seg[4], seg[3], seg[5]]  # p, g, mc, vc, ms, vs
    h = adam_ref.hyper(1e-2, weight_decay=wd, decoupled=decoupled, step=1)
    devs = _upload([seg], "f32")
    ops.adam8_update_batch_(*_views(devs, "f32"), [h])
    torch.cuda.synchronize()
    want = ref.step(*seg, h)
    k = [name for name, _ in blocks].index("v overflows")
    assert want[4][k] == np.inf
    _check([seg], devs, [want], "f32", ("blocks",))


# ---- the quantizer alone ---------------------------------------------------------------

def _boundary_inputs(which):
    t, mid = ref.TABLES[which], ref.MIDS[which]
    x = np.concatenate([t, mid, np.nextafter(mid, np.float32(-np.inf)),
                        np.nextafter(mid, np.float32(np.inf))]).astype(np.float32)
    assert x.size == 1021
    return x


@pytest.mark.parametrize("which", [ref.SIGNED, ref.UNSIGNED])
def test_quantizer_on_every_boundary(which):
    """Every table value, every midpoint and both f32 neighbours of every
    midpoint, each in a block with a 1.0 (so y is the value itself), and the
    whole again scaled by 2^-20 and 2^20 (exact)."""
    from kungfu_amd import ops
    x = _boundary_inputs(which)
    rng = np.random.default_rng(1)
    blocks = rng.uniform(0, 1, (x.size, 64)).astype(np.float32)
    blocks[:, 0] = x
    blocks[:, 1] = 1.0
    src = np.concatenate([blocks.reshape(-1) * np.float32(s) for s in (1.0, 2.0 ** -20, 2.0 ** 20)])
    codes, scales = ops.adam8_quantize(_dev(src), which)
    back = ops.adam8_dequantize(codes, scales, which)
    torch.cuda.synchronize()
    wc, ws = ref.quantize(src, which)
    assert np.array_equal(_host(codes), wc)
    assert _host(scales).tobytes() == ws.tobytes()
    assert _same_f32(_host(back), ref.dequantize(wc, ws, which))
    # what the inputs are there for: a table value has its own code, a
    # midpoint the lower one, its upper neighbour the higher one
    c0 = wc[:64 * x.size].reshape(-1, 64)[:, 0]
    assert np.array_equal(c0[:256], np.arange(256))
    assert np.array_equal(c0[256:511], np.arange(255))
    assert np.array_equal(c0[766:], np.arange(1, 256))
    assert np.array_equal(c0[511:766], np.arange(255))


@pytest.mark.parametrize("which", [ref.SIGNED, ref.UNSIGNED])
def test_quantizer_sweeps_every_bf16_pattern(which):
    """sweep16's 65,536 bf16 patterns widened to f32, once through: NaNs,
    infinities, subnormals and both zeros among them."""
    from kungfu_amd import ops
    src = sweep16.widen("bf16", sweep16.patterns())
    codes, scales = ops.adam8_quantize(_dev(src), which)
    back = ops.adam8_dequantize(codes, scales, which)
    torch.cuda.synchronize()
    wc, ws = ref.quantize(src, which)
    assert np.array_equal(_host(codes), wc)
    assert _same_f32(_host(scales), ws)
    assert np.array_equal(np.isnan(_host(scales)), np.isnan(ws))
    assert (_host(scales)[np.isnan(ws)].view(np.uint32) == ref.NAN_BITS).all()
    assert _same_f32(_host(back), ref.dequantize(wc, ws, which))


@pytest.mark.parametrize("which", [ref.SIGNED, ref.UNSIGNED])
def test_dequantize_every_code_and_special_scale(which):
    from kungfu_amd import ops
    scales = np.array([0.0, 1.0, -1.0, 2.0 ** -100, 2.0 ** 100, np.inf, np.nan, -2.0 ** -140],
                      np.float32)
    codes = np.tile(np.arange(256, dtype=np.uint8), scales.size)
    s = np.repeat(scales, 4)
    got = ops.adam8_dequantize(_dev(codes), _dev(s), which)
    torch.cuda.synchronize()
    assert _same_f32(_host(got), ref.dequantize(codes, s, which))


def test_codec_past_its_block_cap():
    """More than 1024 blocks of 256 lanes: the codec kernels stride."""
    from kungfu_amd import ops
    n = cpu_tests.CODEC_BLOCKS * 256 * 4 + 64 * 5
    rng = np.random.default_rng(6)
    src = _binades(rng, n, -30, 30, True)
    want = np.full(PAD, SENT8, np.uint8)
    codes_full, codes = _padded(np.zeros(n, np.uint8))
    scales_full, scales = _padded_scales(np.zeros(n // 64, np.float32))
    ops.adam8_quantize(_dev(src), ref.SIGNED, codes, scales)
    back_full, back = _padded(np.zeros(n, np.float32))
    ops.adam8_dequantize(codes, scales, ref.SIGNED, out=back)
    torch.cuda.synchronize()
    wc, ws = ref.quantize(src, ref.SIGNED)
    assert np.array_equal(_host(codes), wc) and _host(scales).tobytes() == ws.tobytes()
    assert np.array_equal(_host(codes_full)[n:], want)
    assert _tail_is_sentinel(scales_full, n // 64) and _tail_is_sentinel(back_full, n)
    assert _host(back).tobytes() == ref.dequantize(wc, ws, ref.SIGNED).tobytes()


# ---- split invariance, gated and master twins -----------------------------------------------

def _run(segs, hs, kind="f32", np_=0):
    from kungfu_amd import ops
    devs = _upload(segs, kind)
    f = ops.adam8_update_batch_ if kind == "f32" else ops.adam8_master_update_batch_
    f(*_views(devs, kind), hs, np_=np_)
    torch.cuda.synchronize()
    first = 2 if kind != "f32" else 1
    return [[_host(v) for _, v in row[first:]] for row in devs]


def test_split_invariance():
    """One segment against the same data cut at block multiples into three,
    in one launch and in three."""
    n, a, b = SIZES[-1], 64 * 9, TILE + 64 * 7
    seg = _segment(n, 77)
    h = adam_ref.hyper(1e-2, weight_decay=1e-2, step=2)
    (whole,) = _run([seg], [h])
    cuts = ((0, a), (a, a + b), (a + b, n))
    parts = [[x[lo:hi].copy() for x in seg[:4]] + [x[lo // 64:hi // 64].copy() for x in seg[4:]]
             for lo, hi in cuts]
    together = _run(parts, [h] * 3)
    apart = [_run([p], [h])[0] for p in parts]
    want = ref.step(*seg, h)
    for j in range(5):
        assert _same_f32(whole[j], want[j]) if whole[j].dtype == np.float32 else \
            np.array_equal(whole[j], want[j]), j
        for got in (together, apart):
            assert np.concatenate([g[j] for g in got]).tobytes() == whole[j].tobytes(), j


def _gate_tensors(gate, state):
    from kungfu_amd import ops
    g = ops.new_step_gate("cuda")
    gated.write_gate(g, gate)
    st = ops.new_step_states("cuda", 2)
    gated.write_states(st, [step_gate_ref.new_state(), state])
    return g, st


@pytest.mark.parametrize("kind", ["f32", "bf16"])
def test_gated_twins(kind):
    """A skipping gate leaves every byte; a passing one with grad_mul != 1 and
    the device's s2 / nss gives ref.step_gated's bits."""
    from kungfu_amd import ops
    sizes = (64, TILE + 64, 0, 64 * 16)
    h = adam_ref.hyper(1e-2, weight_decay=1e-2, decoupled=True, step=3)
    state = step_gate_ref.scalars_of(h)
    f = ops.adam8_update_batch_gated_ if kind == "f32" else ops.adam8_master_update_batch_gated_
    for mul, skip in ((0.37, 0), (2.0 ** -16, 0), (0.37, 1)):
        gate = sweep16.gate_of(mul, skip)
        g, st = _gate_tensors(gate, state)
        segs = _segments(kind, sizes)
        devs = _upload(segs, kind)
        f(*_views(devs, kind), h, g, st, group=1, np_=2)
        torch.cuda.synchronize()
        if kind == "f32":
            want = [ref.step_gated(*seg, h, gate, state, 2) for seg in segs]
        else:
            want = [ref.step_master_gated(*seg, kind, h, gate, state, 2) for seg in segs]
        _check(segs, devs, want, kind, (kind, mul, skip), skipped=bool(skip))
        if skip:  # every byte: the reference returned copies of its inputs
            for seg, w in zip(segs, want):
                assert w[-4].tobytes() == seg[2].tobytes() and w[-1].tobytes() == seg[5].tobytes()


@pytest.mark.parametrize("kind", ["bf16", "f16"])
@pytest.mark.parametrize("wd,decoupled", adam_cpu.ROWS)
def test_master_twins(kind, wd, decoupled):
    from kungfu_amd import ops
    segs = _segments(kind)
    hs = _hypers(len(segs), wd, decoupled)
    devs = _upload(segs, kind)
    ops.adam8_master_update_batch_(*_views(devs, kind), hs, np_=3)
    torch.cuda.synchronize()
    want = [_ref_step(seg, h, kind, 3) for seg, h in zip(segs, hs)]
    _check(segs, devs, want, kind, (kind, wd, decoupled))


# ---- end to end ------------------------------------------------------------------------------

def _cpu_run(kind, gate, resume_at=None):
    """The same optimizer on the numpy epilogue, on CPU tensors at world 1."""
    from kungfu_amd.collective import Exchange
    ps, opt = cpu.make_optimizer(Exchange(epilogue=cpu.CpuAdam8Epilogue()), kind, gate=gate)
    cpu.run_steps(ps, opt, kind, 1, 0, steps=4, gate=gate)
    return cpu.snapshot(ps, opt)


def _same_snapshot(a, b):
    (pa, sa), (pb, sb) = a, b
    assert len(pa) == len(pb) and set(sa) == set(sb)
    for j, (x, y) in enumerate(zip(pa, pb)):
        assert cpu.same_bits(x, y), ("param", j)
    for j in sa:
        assert set(sa[j]) == set(sb[j])
        for k in sa[j]:
            if isinstance(sa[j][k], np.ndarray):
                assert cpu.same_bits(sa[j][k], sb[j][k]), (k, j)
            else:
                assert sa[j][k] == sb[j][k], (k, j)


def _gpu_body(kind, gate, world, rank, ex, got):
    """Two steps, a checkpoint into a second optimizer on the same exchange,
    two more steps on both."""
    ps, opt = cpu.make_optimizer(ex, kind, device="cuda", gate=gate)
    cpu.run_steps(ps, opt, kind, world, rank, device="cuda", steps=2, gate=gate)
    params, state = cpu.snapshot(ps, opt)
    ps2, opt2 = cpu.make_optimizer(ex, kind, device="cuda", gate=gate, arrays=params)
    for g, g2 in zip(opt.param_groups, opt2.param_groups):
        g2["lr"] = g["lr"]
    cpu.load_snapshot(ps2, opt2, state, device="cuda")
    if gate:
        opt2.load_scaler_state(opt.scaler_state())
    for qs, o in ((ps, opt), (ps2, opt2)):
        cpu.run_steps(qs, o, kind, world, rank, device="cuda", first=2, steps=2, gate=gate)
    assert len(opt.state) == 0 and all(G["b8"] for G in opt._kf_groups)
    assert all(c.dtype == torch.uint8 for G in opt._kf_groups for c in G["m"] + G["v"])
    got[rank] = (cpu.snapshot(ps, opt), cpu.snapshot(ps2, opt2))


CASES = [("f32", False), ("bf16", True)]


@pytest.mark.parametrize("kind,gate", CASES)
def test_optimizer_over_loopback(kind, gate):
    """World 2 over the loopback transport against the optimizer on the numpy
    epilogue and against adam8_ref on the unsharded buckets; the resumed
    optimizer ends where the uninterrupted one does."""
    want, got = _cpu_run(kind, gate), {}
    loopback.loop_ranks(2, lambda rank, ex: _gpu_body(kind, gate, 2, rank, ex, got))
    ref_run = cpu.reference_run(kind, 4, gate)
    for r in range(2):
        for snap in got[r]:
            _same_snapshot(snap, want)
        for j, p in enumerate(got[r][0][0]):
            assert cpu.same_bits(p, ref_run["p"][j]), ("reference", j)


@pytest.mark.parametrize("kind,gate", CASES)
def test_optimizer_over_one_rank_rccl(kind, gate):
    want, got = _cpu_run(kind, gate), {}
    for make in (loopback.rccl1_exchange, lambda: None):
        ex = make()
        _gpu_body(kind, gate, 1, 0, ex, got)
        for snap in got[0]:
            _same_snapshot(snap, want)
        if ex is not None:
            ex.close()
