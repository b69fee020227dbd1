"""The kernel schedules that only large launches select, on the GPU against
the oracle: the runtime-k fold's one-vector-in-flight loads (single and
batched launches of 2048 blocks and more), grid-stride under a lowered block
cap, the segmented norm's strided SQ body, its fold's eight-loads-at-a-time
loop and its total's later LDS rounds, and the SGD, Adam, master-weight,
gated, stochastic-rounding and LAMB moments updates as rows grids of
multi-tile segments (42 cases of the Adam family, under a second together on
an MI355X, none above 0.1 s). What those 42 catch, measured on libraries with
one line changed: without the g * grad_mul multiply every applied gated case
fails, with p narrowed by r_v's bits every stochastic-rounding case. A change
that makes two blocks of a row do the same in-place work (the scalar tail on
the blocks after the first, `blk` for `blk == 0`; a row's blocks striding by
one less than the row's width) rewrites what the other block has read a
moment before, so it shows only where the blocks' timing lets it: 3 and 13
of the 42 failed, the stochastic-rounding cases among them every time (their
one-launch-per-segment half has a single block), while the sweeps of
tests/test_sweep16_gpu.py, whose tails-alone tables are rows grids one block
wide, fail on the first of the two throughout.

The shapes come from tests/large_launch.py; tests/test_large_launch.py shows
on the CPU that each reaches its path. Every reduce and blend output is
compared whole, bit for bit (NaNs by position), inside a poisoned buffer
whose other bytes must not change.

The tests under a lowered grid cap (the `capped` fixture) stay at the end of
this file: the cap is the library's process-wide launch geometry, and the
fixture puts the defaults back before anything else runs.
"""
import ctypes
import zlib

import numpy as np
import pytest

import golden_io
import large_launch as ll
import monitor_ref
import sgd_ref

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

POISON = 0xA5
ALPHA = 0.1


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib(dev):
    from kungfu_amd import _lib
    l = _lib.load()
    assert l.kf_device_count() > 0
    return l


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    oracle.build()
    return oracle


# ---- shared inputs -------------------------------------------------------------
# Four random arrays per element kind, made once and kept on the device. Input
# j of a launch is array j % 4 from a start that moves 257 vectors per round
# of four, so no two inputs of a launch hold the same data at an index.

POOL_ARRAYS = 4
POOL_ROUND = 257                      # vectors
POOL_VECS = 2100 * ll.TILE            # the longest flat layout and every round's start fit
KIND = {"u8": "bytes", "i8": "bytes", "i32": "bytes"}


class Pool:
    def __init__(self, dev):
        self.dev = dev
        self._host, self._dev = {}, {}

    def _make(self, kind, i):
        rng = np.random.default_rng(zlib.crc32(kind.encode()) + i)
        nbytes = (POOL_VECS + 4 * POOL_ROUND) * 16
        if kind == "bytes":
            return rng.integers(0, 256, nbytes, dtype=np.uint8)
        if kind == "f64":
            return rng.standard_normal(nbytes // 8)
        x = rng.standard_normal(nbytes // 4 if kind == "f32" else nbytes // 2, dtype=np.float32)
        if kind == "f32":
            return x
        if kind == "f16":
            return (x * 30).astype(np.float16)
        return (x.view(np.uint32) >> 16).astype(np.uint16)  # bf16: the top halves

    def host(self, dt):
        """The four host arrays, in dt's numpy type."""
        from oracle.oracle import NP
        kind = KIND.get(dt, dt)
        if kind not in self._host:
            self._host[kind] = [self._make(kind, i) for i in range(POOL_ARRAYS)]
        return [a.view(NP[dt]) for a in self._host[kind]]

    def device(self, dt):
        kind = KIND.get(dt, dt)
        if kind not in self._dev:
            self.host(dt)
            self._dev[kind] = [torch.from_numpy(a.view(np.uint8)).to(self.dev)
                               for a in self._host[kind]]
            assert all(t.data_ptr() % 16 == 0 for t in self._dev[kind])
        return self._dev[kind]

    def start(self, j, dt, offset):
        return (j // POOL_ARRAYS) * POOL_ROUND * ll.epv(dt) + offset

    def input(self, dt, j, n, offset):
        """(host slice, device address) of n elements of input j, `offset`
        elements past a 16-B boundary."""
        s = self.start(j, dt, offset)
        h = self.host(dt)[j % POOL_ARRAYS][s:s + n]
        assert h.size == n, "the pool is too short for this input"
        return h, self.device(dt)[j % POOL_ARRAYS].data_ptr() + s * ll.ITEMSIZE[dt]


@pytest.fixture(scope="module")
def pool(dev):
    p = Pool(dev)
    yield p
    p._dev.clear()
    p._host.clear()
    torch.cuda.empty_cache()


# ---- poisoned outputs ------------------------------------------------------------

def poisoned_bytes(nbytes, dev):
    return torch.full((nbytes,), POISON, dtype=torch.uint8, device=dev)


def out_buffer(n, dt, residue, dev):
    """A poisoned device buffer with room for n elements from `residue`
    elements past a 16-B boundary, a vector and more of poison on either
    side. Returns (buffer, index of the first output element)."""
    e, isz = ll.epv(dt), ll.ITEMSIZE[dt]
    pre = e + residue
    buf = poisoned_bytes((pre + n + 2 * e) * isz, dev)
    assert buf.data_ptr() % 16 == 0
    return buf, pre


def check_out(buf, pre, n, dt, want, what):
    """The n elements from `pre` equal `want` bit for bit (NaNs by position),
    and every other byte of the buffer is still poison."""
    from oracle.oracle import NP
    isz = ll.ITEMSIZE[dt]
    h = buf.cpu().numpy()
    assert (h[:pre * isz] == POISON).all(), ("wrote before the output", what)
    assert (h[(pre + n) * isz:] == POISON).all(), ("wrote past the output", what)
    got = h[pre * isz:(pre + n) * isz].copy().view(NP[dt])
    assert golden_io.same_bits_or_nan(got, np.asarray(want).view(NP[dt])), what


def stream():
    return torch.cuda.current_stream().cuda_stream


def reduce_call(lib, ptrs, k, out_ptr, n, dt, op, peers=False):
    from kungfu_amd import _lib
    from oracle.oracle import DT, OPS
    arr = _lib.ptr_array(ptrs)
    if peers:
        rc = lib.kf_bucket_reduce_peers(arr, k, out_ptr, n, DT[dt], 0 if op == "avg" else OPS[op],
                                        k if op == "avg" else 0, stream())
    elif op == "avg":
        rc = lib.kf_bucket_reduce_avg(arr, k, out_ptr, n, DT[dt], k, stream())
    else:
        rc = lib.kf_bucket_reduce(arr, k, out_ptr, n, DT[dt], OPS[op], stream())
    assert rc == 0, lib.kf_last_error()
    torch.cuda.synchronize()


def reference(orc, hs, dt, op):
    if op == "avg":
        return orc.reduce_avg(hs, dt, len(hs))
    return orc.reduce_k(hs, dt, op)


def run_single(lib, orc, pool, dev, dt, k, op, n, out_residue, in_residue=None, peers=False):
    """One launch over pool inputs into a poisoned buffer, against the oracle.
    in_residue None: input j starts ll.input_offset(j) past a 16-B boundary."""
    ins = [pool.input(dt, j, n, ll.input_offset(j, dt) if in_residue is None else in_residue)
           for j in range(k)]
    buf, pre = out_buffer(n, dt, out_residue, dev)
    reduce_call(lib, [p for _, p in ins], k, buf.data_ptr() + pre * ll.ITEMSIZE[dt], n, dt, op,
                peers=peers)
    check_out(buf, pre, n, dt, reference(orc, [h for h, _ in ins], dt, op), (dt, k, op, n))


# ---- A1. single launches of 2049 blocks: one vector in flight ------------------------

@pytest.mark.parametrize("dt,k,op", ll.SINGLE_CASES,
                         ids=["%s-k%d-%s" % c for c in ll.SINGLE_CASES])
def test_serial_fold_single_launch(lib, orc, pool, dev, dt, k, op):
    """S_rag: 2049 blocks, the last tile ragged, E - 1 head and tail scalars;
    the output one element past a 16-B boundary, input j (3j + 1) mod E past
    one, so the one-in-flight loads of inputs 2..k-1 run at unaligned
    addresses."""
    run_single(lib, orc, pool, dev, dt, k, op, ll.single_shape("S_rag", dt, 1), 1)


@pytest.mark.parametrize("shape", ["S_at", "S_lo"])
@pytest.mark.parametrize("dt,k", ll.THRESHOLD_CASES)
def test_serial_threshold_both_sides(lib, orc, pool, dev, dt, k, shape):
    """2048 blocks, all tiles full (the flag is on) and 2047 (the control: it
    is off), co-aligned, SUM."""
    run_single(lib, orc, pool, dev, dt, k, "sum", ll.single_shape(shape, dt, 0), 0, in_residue=0)


@pytest.fixture(scope="module")
def alias_reference(orc, pool):
    """The inputs and the oracle's fold both in-place cases share."""
    n = ll.single_shape("S_rag", "f32", 1)
    hs = [pool.input("f32", j, n, 1)[0] for j in range(4)]
    return n, hs, orc.reduce_k(hs, "f32", "sum")


@pytest.mark.parametrize("alias", [0, 2])
def test_serial_fold_in_place(lib, pool, dev, alias_reference, alias):
    """f32 k = 4, S_rag, every pointer one element past a 16-B boundary; the
    output is input 0, then input 2 (a serially loaded input)."""
    n, hs, want = alias_reference
    ptrs = [pool.input("f32", j, n, 1)[1] for j in range(4)]
    buf, pre = out_buffer(n, "f32", 1, dev)
    buf[pre * 4:(pre + n) * 4] = torch.from_numpy(hs[alias].view(np.uint8)).to(dev)
    ptrs[alias] = buf.data_ptr() + pre * 4
    reduce_call(lib, ptrs, 4, ptrs[alias], n, "f32", "sum")
    check_out(buf, pre, n, "f32", want, ("alias", alias))
    # the inputs that are not the output are as they were
    for j in range(4):
        if j != alias:
            s = pool.start(j, "f32", 1)
            kept = pool.device("f32")[j % POOL_ARRAYS][s * 4:(s + n) * 4]
            assert torch.equal(kept.cpu(), torch.from_numpy(hs[j].view(np.uint8))), j


# ---- A2. batched launches ----------------------------------------------------------------

def run_batch(lib, orc, pool, dev, buckets, dt, k, avg):
    """kf_bucket_reduce_batch over [(count, misaligned)] laid out in flat
    buffers (one per input, one poisoned for the outputs): every bucket
    against the oracle, every byte between the buckets unchanged."""
    from kungfu_amd import _lib
    from oracle.oracle import DT, NP
    isz = ll.ITEMSIZE[dt]
    offs, total = ll.flat_layout(buckets, dt)
    flats = [pool.input(dt, j, total, 0) for j in range(k)]
    out = poisoned_bytes(total * isz, dev)
    assert out.data_ptr() % 16 == 0
    ptrs = [fp + o * isz for o in offs for _, fp in flats]
    outs = [out.data_ptr() + o * isz for o in offs]
    rc = lib.kf_bucket_reduce_batch(
        _lib.ptr_array(ptrs), k, _lib.ptr_array(outs),
        (ctypes.c_size_t * len(buckets))(*[n for n, _ in buckets]), len(buckets), DT[dt], 0,
        k if avg else 0, stream())
    assert rc == 0, lib.kf_last_error()
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    for b, ((n, _), o) in enumerate(zip(buckets, offs)):
        if n == 0:
            continue
        hs = [fh[o:o + n] for fh, _ in flats]
        want = reference(orc, hs, dt, "avg" if avg else "sum")
        seg = got[o * isz:(o + n) * isz]
        assert golden_io.same_bits_or_nan(seg.copy().view(NP[dt]), want), (dt, k, avg, b, n)
        seg[:] = POISON
    assert (got == POISON).all(), "a byte outside the buckets changed"


@pytest.mark.parametrize("dt,k,avg", [("f32", 3, False), ("f32", 5, True), ("bf16", 8, True),
                                      ("u8", 5, False)])
def test_serial_fold_batched(lib, orc, pool, dev, dt, k, avg):
    """Twenty ragged buckets: the first launch (sixteen of them, 2077 blocks,
    none of 2048 alone) runs the one-in-flight schedule, the second (three
    small ones) does not."""
    run_batch(lib, orc, pool, dev, ll.batch_buckets(dt), dt, k, avg)


@pytest.mark.parametrize("avg", [False, True], ids=["sum", "avg"])
def test_serial_fold_batched_rows(lib, orc, pool, dev, avg):
    """Sixteen equal buckets of 129 blocks: a 129 x 16 rows grid, 2064 blocks."""
    run_batch(lib, orc, pool, dev, ll.equal_buckets("f32"), "f32", 3, avg)


# ---- B. segmented norms -------------------------------------------------------------------

def _segnorm(views, cap, monkeypatch):
    """A plan built under KUNGFU_AMD_SEGNORM_MAX_BLOCKS = cap (None: unset)."""
    from kungfu_amd import ops
    with monkeypatch.context() as m:
        if cap is None:
            m.delenv("KUNGFU_AMD_SEGNORM_MAX_BLOCKS", raising=False)
        else:
            m.setenv("KUNGFU_AMD_SEGNORM_MAX_BLOCKS", str(cap))
        return ops.SegNorm(views)


def _total_is_left_sum(got, nseg):
    assert got[nseg].tobytes() == np.float64(monitor_ref.left_sum(got[:nseg])).tobytes()


@pytest.fixture(scope="module")
def stride_cases(dev):
    """Per dtype: the a and b buffers of the stride segments and their exact
    sums, shared by both caps."""
    import test_monitor_gpu as mon
    cases = {}

    def get(dt):
        if dt not in cases:
            counts = ll.seg_stride_counts(dt)
            fa, va, sa = mon.make_case(counts, dt, dev, seed=70, square=True)
            fb, vb, sb = mon.make_case(counts, dt, dev, seed=71)
            cases[dt] = (counts, (fa, fb), va, vb,
                         [monitor_ref.exact_sq(a, dt) for a in sa],
                         [monitor_ref.exact_var(a, b, dt) for a, b in zip(sa, sb)])
        return cases[dt]

    yield get
    cases.clear()


@pytest.mark.parametrize("cap", ll.SEG_STRIDE_CAPS)
@pytest.mark.parametrize("dt", ["f32", "f16", "bf16", "f64"])
def test_segnorm_strides_under_cap(dev, stride_cases, monkeypatch, dt, cap):
    """Segments of 0, 1, an SQ tile + 1, exactly 3 tiles and 5 tiles + 300
    vectors + edges, at most `cap` blocks each: the SQ body strides over its
    tiles (VAR over twice as many). Each sum within the bound of the exact
    one; capped and uncapped plans add in different orders, so nothing is
    said about their bits."""
    import test_monitor_gpu as mon
    counts, _, va, vb, want_sq, want_var = stride_cases(dt)
    plan = _segnorm(list(zip(va, vb)), cap, monkeypatch)
    sq = plan.run("sq").cpu().numpy()
    var = plan.run("var").cpu().numpy()
    plan.close()
    for s, n in enumerate(counts):
        mon.check_bound(float(sq[s]), want_sq[s], n, "%s cap %d sq seg %d" % (dt, cap, s))
        mon.check_bound(float(var[s]), want_var[s], n, "%s cap %d var seg %d" % (dt, cap, s))
    assert sq[0] == 0.0 and var[0] == 0.0
    _total_is_left_sum(sq, len(counts))
    _total_is_left_sum(var, len(counts))


def _dyadic(ints, scale, dt):
    """ints * scale (a power of two; exact in fp32 and, for these ranges, in
    bf16) in dt's host representation."""
    x = ints.astype(np.float32) * np.float32(scale)
    return (x.view(np.uint32) >> 16).astype(np.uint16) if dt == "bf16" else x


@pytest.mark.parametrize("dt,mode", [("f32", "sq"), ("bf16", "sq"), ("f32", "var")])
def test_segnorm_wide_fold_exact(dev, monkeypatch, dt, mode):
    """One segment of 2100 SQ tiles (65.6 MiB) between two small random ones,
    two plans over the same bytes: 2048 blocks (52 take a second tile; the
    fold's eight-loads-at-a-time loop once in every lane) and, with the cap
    at 4096, 2100 blocks (that loop, then the one-at-a-time loop in 52
    lanes). The data are small dyadic numbers, every partial sum is exact in
    fp64 in any order, so the segment's sum EQUALS the integer sum."""
    import test_monitor_gpu as mon
    n = ll.wide_count(dt)
    counts = [ll.WIDE_BEFORE, n, ll.WIDE_AFTER]
    offs, total = mon.layout(counts, dt)
    rng = np.random.default_rng(80)
    ha, hb = mon.poisoned(total, dt), mon.poisoned(total, dt)
    small = {}
    for s in (0, 2):
        b = mon.cast(rng.standard_normal(counts[s]), dt)
        a = mon.cast(rng.standard_normal(counts[s]) ** 2, dt) if mode == "var" else b
        ha[offs[s]:offs[s] + counts[s]] = a
        hb[offs[s]:offs[s] + counts[s]] = b
        small[s] = (monitor_ref.exact_var(a, b, dt) if mode == "var"
                    else monitor_ref.exact_sq(a, dt))
    if mode == "sq":
        m = ll.dyadic_sq(n, 81)
        ha[offs[1]:offs[1] + n] = _dyadic(m, 0.25, dt)
        exact = ll.exact_sq_sum(m)
    else:
        j, m = ll.dyadic_var(n, 82)
        ha[offs[1]:offs[1] + n] = _dyadic(j, 0.0625, dt)
        hb[offs[1]:offs[1] + n] = _dyadic(m, 0.25, dt)
        exact = ll.exact_var_sum(j, m)
    assert exact > 0
    da = mon.to_dev(ha, dt, dev)
    va = [da[o:o + c] for o, c in zip(offs, counts)]
    if mode == "var":
        db = mon.to_dev(hb, dt, dev)
        views = [(x, db[o:o + c]) for x, o, c in zip(va, offs, counts)]
    else:
        views = va
    for cap in (None, ll.WIDE_CAP):
        plan = _segnorm(views, cap, monkeypatch)
        got = plan.run(mode).cpu().numpy()
        plan.close()
        print("%s %s cap %s: got=%.17g exact=%.17g" % (dt, mode, cap, got[1], exact))
        assert got[1] == exact, (dt, mode, cap, float(got[1]), exact)
        for s in (0, 2):
            mon.check_bound(float(got[s]), small[s], counts[s], "%s %s neighbour %d" % (dt, mode, s))
        _total_is_left_sum(got, 3)


def test_segnorm_total_three_rounds(dev):
    """600 segments: segnorm_total_kernel stages 256 + 256 + 88 values."""
    import test_monitor_gpu as mon
    from kungfu_amd import ops
    small = [c for c in mon.COUNTS if c <= 1023]
    nseg = ll.TOTAL_NSEG
    counts = [small[s % len(small)] for s in range(nseg)]
    _, views, segs = mon.make_case(counts, "f32", dev, seed=90)
    plan = ops.SegNorm(views)
    sq = plan.run("sq").cpu().numpy()
    root = plan.run("sq", total_sqrt=True).cpu().numpy()
    plan.close()
    for s in range(nseg):
        want = monitor_ref.exact_sq(segs[s], "f32")
        assert abs(sq[s] - want) <= monitor_ref.bound(counts[s]) * want, s
    _total_is_left_sum(sq, nseg)
    assert root[:nseg].tobytes() == sq[:nseg].tobytes()
    # both square roots are correctly rounded
    want = np.float64(monitor_ref.left_sum(np.sqrt(sq[:nseg])))
    assert root[nseg].tobytes() == want.tobytes()


# ---- C. the SGD update as rows -----------------------------------------------------------

_SGD_DT = {"f32": (torch.float32, np.int32), "f64": (torch.float64, np.int64),
           "f16": (torch.float16, np.int16), "bf16": (torch.bfloat16, np.int16)}


def _sgd_store(x, dt):
    if dt == "bf16":
        return sgd_ref.f32_to_bf16_bits(x.astype(np.float32))
    return x.astype(sgd_ref.STORAGE[dt])


def _sgd_dev(a, dt):
    tt, it = _SGD_DT[dt]
    return torch.from_numpy(a.view(it).copy()).cuda().view(tt)


def _sgd_host(t, dt):
    tt, it = _SGD_DT[dt]
    ti = {np.int16: torch.int16, np.int32: torch.int32, np.int64: torch.int64}[it]
    return t.detach().cpu().view(ti).numpy().view(sgd_ref.STORAGE[dt])


def _sgd_same(got, want, dt):
    if dt == "bf16":
        f = sgd_ref.bf16_bits_to_f32
        return golden_io.same_bits_or_nan(f(got), f(want))
    return golden_io.same_bits_or_nan(got, want)


@pytest.mark.parametrize("tiles", [ll.SGD_ROWS_TILES, ll.SGD_FLAT_TILES], ids=["rows", "table"])
@pytest.mark.parametrize("dt", ["f32", "f16", "bf16", "f64"])
def test_sgd_rows_grid_multi_tile(dev, dt, tiles):
    """Segments of 5, 4, 5 and 3 tiles (each short by 100 vectors, with a
    scalar tail): a rows grid 5 wide whose last row has two blocks without a
    tile; and 5, 1, 1, 1 tiles, the 1-D table grid, as the control."""
    from kungfu_amd import ops
    counts = ll.sgd_counts(dt, tiles)
    rng = np.random.default_rng(len(tiles) + sum(tiles))
    segs = [tuple(_sgd_store(rng.standard_normal(n), dt) for _ in range(3)) for n in counts]
    hs = [sgd_ref.hyper(0.1 / (1 + i), momentum=0.9, nesterov=True, weight_decay=1e-2,
                        first=False) for i in range(len(counts))]
    ps, gs, ms = ([_sgd_dev(s[i], dt) for s in segs] for i in range(3))
    assert all(t.data_ptr() % 16 == 0 for t in ps + gs + ms)
    ops.sgd_update_batch_(ps, gs, ms, hs, np_=3)
    torch.cuda.synchronize()
    for i, ((p, g, m), h) in enumerate(zip(segs, hs)):
        wp, wm = sgd_ref.step(p, g, m, dt, h, 3)
        assert _sgd_same(_sgd_host(ps[i], dt), wp, dt), ("param", dt, i)
        assert _sgd_same(_sgd_host(ms[i], dt), wm, dt), ("momentum", dt, i)
        assert _sgd_host(gs[i], dt).tobytes() == g.tobytes(), ("grad was written", dt, i)


# ---- D. the Adam-family updates as rows ---------------------------------------------------
# ROWS_TILES: segments of 5, 4, 5 and 3 tiles, a rows grid 5 wide whose rows
# have up to two blocks without a tile. ROWS_WITH_TAIL_ONLY: three segments of
# two tiles and one shorter than a unit, whose row does block 0's scalar tail
# and nothing else. Every role's segments sit in one poisoned allocation.

_BITS16 = ("bf16", "f16")
_TORCH = {"f32": torch.float32, "f64": torch.float64, "bf16": torch.bfloat16, "f16": torch.float16}
UPDATE_NP = 3
SR_KEY = 0x9ABCDEF1


def _as_dt(x, dt):
    """fp64 values in dt's travelling form: numpy's own type, or uint16 bits."""
    import sweep16 as sw
    if dt in _BITS16:
        return sw.narrow(dt, x.astype(np.float32))
    return x.astype({"f32": np.float32, "f64": np.float64}[dt])


def _f16(a, dt):
    """uint16 bits in the form adam_master_ref takes."""
    return a.view(np.float16) if dt == "f16" else a


class Seated:
    """One role's segments in one poisoned allocation: every segment starts on
    a 16-byte boundary with at least two vectors of poison after its last
    element. arrays[i] None: `counts[i]` elements of poison (an output)."""

    def __init__(self, arrays, counts, dt, dev):
        self.dt, self.isz, self.counts = dt, ll.ITEMSIZE[dt], counts
        self.offs, cur = [], 16
        for n in counts:
            self.offs.append(cur)
            cur += ll.ceil_div(n * self.isz, 16) * 16 + 32
        self.host = np.full(cur, POISON, np.uint8)
        for a, o in zip(arrays, self.offs):
            if a is not None:
                self.host[o:o + a.nbytes] = np.ascontiguousarray(a).view(np.uint8)
        self.t = torch.from_numpy(self.host.copy()).to(dev)
        assert self.t.data_ptr() % 16 == 0

    def views(self):
        return [self.t[o:o + n * self.isz].view(_TORCH[self.dt])
                for o, n in zip(self.offs, self.counts)]

    def check(self, want, what):
        """Segment i holds want[i] bit for bit (NaNs by position; want None:
        nothing at all was written) and every other byte is as it was."""
        import sweep16 as sw
        got = self.t.cpu().numpy()
        if want is None:
            assert np.array_equal(got, self.host), (what, "was written")
            return
        rest = got.copy()
        for i, (w, o, n) in enumerate(zip(want, self.offs, self.counts)):
            seg = got[o:o + n * self.isz]
            if self.dt in _BITS16:
                bad = sw.mismatches(self.dt, seg.view(np.uint16), np.ascontiguousarray(w).view(np.uint16))
            else:
                bad = sw.mismatches_float(seg.view(w.dtype), w)
            assert bad.size == 0, (what, i, n, bad.size, bad[:4].tolist(), bad[-1])
            rest[o:o + n * self.isz] = self.host[o:o + n * self.isz]
        assert np.array_equal(rest, self.host), (what, "a byte outside the segments changed")


def _update_data(kernel, shape, dt, seed):
    """(counts, [(p, g, m, v)]) of standard-normal p, g, m and squared-normal v."""
    counts = ll.update_shape(kernel, shape)
    rng = np.random.default_rng(seed)
    return counts, [tuple(_as_dt(rng.standard_normal(n) ** (2 if j == 3 else 1), dt)
                          for j in range(4)) for n in counts]


def _adam_hypers(n):
    """A hyper of its own per segment: lr, decay mode and step differ."""
    import adam_ref
    modes = ((0.0, False), (1e-2, False), (1e-2, True), (0.0, False))
    return [adam_ref.hyper(1e-2 / (1 + i), weight_decay=modes[i % 4][0], decoupled=modes[i % 4][1],
                           step=1 + 2 * i) for i in range(n)]


def _gate(skip):
    """(hyper, reference gate, reference state, device gate, device states):
    AdamW under a clip of 0.37 at step 5; the kernel reads group 1 of two."""
    import adam_ref
    import step_gate_ref
    import test_sharded_adam_gated as gated
    from kungfu_amd import ops
    h = adam_ref.hyper(1e-2, weight_decay=1e-2, decoupled=True, step=5)
    gate = dict(step_gate_ref.new_gate(), skip=skip, grad_mul=np.float32(0.37))
    state = step_gate_ref.scalars_of(h)
    g, st = ops.new_step_gate("cuda"), ops.new_step_states("cuda", 2)
    gated.write_gate(g, gate)
    gated.write_states(st, [step_gate_ref.new_state(), state])
    return h, gate, state, g, st


def _seat(segs, counts, dt, dev, roles=4):
    return [Seated([seg[j] for seg in segs], counts, dt, dev) for j in range(roles)]


@pytest.mark.parametrize("shape", ll.UPDATE_SHAPES)
@pytest.mark.parametrize("dt", ["f32", "bf16", "f64"])
def test_adam_rows_grid(dev, dt, shape):
    import adam_ref
    from kungfu_amd import ops
    counts, segs = _update_data("adam-" + dt, shape, dt, 11)
    hs = _adam_hypers(len(counts))
    p, g, m, v = _seat(segs, counts, dt, dev)
    ops.adam_update_batch_(p.views(), g.views(), m.views(), v.views(), hs, np_=UPDATE_NP)
    torch.cuda.synchronize()
    want = [adam_ref.step(*seg, dt, h, UPDATE_NP) for seg, h in zip(segs, hs)]
    for j, (buf, what) in enumerate(((p, "param"), (m, "exp_avg"), (v, "exp_avg_sq"))):
        buf.check([w[j] for w in want], (what, dt, shape))
    g.check(None, ("grad", dt, shape))


def _seat_master(segs, counts, dt, dev):
    """(p16 as poison, g16, fp32 master, m, v)."""
    g16 = Seated([seg[1] for seg in segs], counts, dt, dev)
    p16 = Seated([None] * len(counts), counts, dt, dev)
    return [p16, g16] + [Seated([seg[j] for seg in segs], counts, "f32", dev) for j in (0, 2, 3)]


def _master_data(kernel, shape, dt, seed):
    """fp32 master, m, v and a 16-bit gradient."""
    counts, segs = _update_data(kernel, shape, "f32", seed)
    return counts, [(seg[0], _as_dt(seg[1].astype(np.float64), dt), seg[2], seg[3]) for seg in segs]


@pytest.mark.parametrize("shape", ll.UPDATE_SHAPES)
@pytest.mark.parametrize("dt", _BITS16)
def test_adam_master_rows_grid(dev, dt, shape):
    import adam_master_ref
    from kungfu_amd import ops
    counts, segs = _master_data("master-" + dt, shape, dt, 12)
    hs = _adam_hypers(len(counts))
    bufs = _seat_master(segs, counts, dt, dev)
    ops.adam_master_update_batch_(*[b.views() for b in bufs], hs, np_=UPDATE_NP)
    torch.cuda.synchronize()
    want = [adam_master_ref.step(w, _f16(g, dt), m, v, dt, h, UPDATE_NP)
            for (w, g, m, v), h in zip(segs, hs)]
    for j, (k, what) in enumerate(((0, "param16"), (2, "master"), (3, "exp_avg"), (4, "exp_avg_sq"))):
        bufs[k].check([w[j] for w in want], (what, dt, shape))
    bufs[1].check(None, ("grad", dt, shape))


@pytest.mark.parametrize("skip", [0, 1])
@pytest.mark.parametrize("shape", ll.UPDATE_SHAPES)
@pytest.mark.parametrize("dt", ["f32", "bf16", "f64"])
def test_adam_gated_rows_grid(dev, dt, shape, skip):
    import step_gate_ref
    from kungfu_amd import ops
    counts, segs = _update_data("adam-" + dt, shape, dt, 13)
    h, gate, state, dg, ds = _gate(skip)
    p, g, m, v = _seat(segs, counts, dt, dev)
    ops.adam_update_batch_gated_(p.views(), g.views(), m.views(), v.views(), h, dg, ds, group=1,
                                 np_=UPDATE_NP)
    torch.cuda.synchronize()
    want = [step_gate_ref.update(*seg, dt, h, gate, state, UPDATE_NP) for seg in segs]
    for j, (buf, what) in enumerate(((p, "param"), (m, "exp_avg"), (v, "exp_avg_sq"))):
        buf.check(None if skip else [w[j] for w in want], (what, dt, shape, skip))
    g.check(None, ("grad", dt, shape, skip))


@pytest.mark.parametrize("skip", [0, 1])
@pytest.mark.parametrize("shape", ll.UPDATE_SHAPES)
@pytest.mark.parametrize("dt", _BITS16)
def test_adam_master_gated_rows_grid(dev, dt, shape, skip):
    import step_gate_ref
    from kungfu_amd import ops
    counts, segs = _master_data("master-" + dt, shape, dt, 14)
    h, gate, state, dg, ds = _gate(skip)
    bufs = _seat_master(segs, counts, dt, dev)
    ops.adam_master_update_batch_gated_(*[b.views() for b in bufs], h, dg, ds, group=1, np_=UPDATE_NP)
    torch.cuda.synchronize()
    want = [step_gate_ref.update_master(w, _f16(g, dt), m, v, dt, h, gate, state, UPDATE_NP)
            for w, g, m, v in segs]
    for j, (k, what) in enumerate(((0, "param16"), (2, "master"), (3, "exp_avg"), (4, "exp_avg_sq"))):
        bufs[k].check(None if skip else [w[j] for w in want], (what, dt, shape, skip))
    bufs[1].check(None, ("grad", dt, shape, skip))


@pytest.mark.parametrize("gated", [False, True], ids=["plain", "gated"])
@pytest.mark.parametrize("shape", ll.UPDATE_SHAPES)
def test_adam_sr_rows_grid(dev, shape, gated):
    """The rows launch against the reference, then the same data as one
    launch per segment (a 1-D grid each): the random bits depend on the
    element index alone, so the bits are the same."""
    import adam_sr_ref
    from kungfu_amd import ops
    dt = "bf16"
    counts, segs = _update_data("sr-bf16", shape, dt, 15)
    bases = [8 * (1000 * i + 3) for i in range(len(counts))]
    streams = [(0x01234567 * (i + 1)) & 0xFFFFFFFF for i in range(len(counts))]
    if gated:
        h, gate, state, dg, ds = _gate(0)
        want = [adam_sr_ref.step_gated(*seg, h, gate, state, b, s, SR_KEY, UPDATE_NP)
                for seg, b, s in zip(segs, bases, streams)]
    else:
        hs = _adam_hypers(len(counts))
        want = [adam_sr_ref.step(*seg, h, b, s, SR_KEY, UPDATE_NP)
                for seg, h, b, s in zip(segs, hs, bases, streams)]

    def run(which):
        bufs = _seat(segs, counts, dt, dev)
        cols = [b.views() for b in bufs]
        for idx in which:
            args = [[c[i] for i in idx] for c in cols]
            tabs = ([bases[i] for i in idx], [streams[i] for i in idx], SR_KEY)
            if gated:
                ops.adam_sr_update_batch_gated_(*args, h, dg, ds, *tabs, group=1, np_=UPDATE_NP)
            else:
                ops.adam_sr_update_batch_(*args, [hs[i] for i in idx], *tabs, np_=UPDATE_NP)
        torch.cuda.synchronize()
        return bufs
    together = run([list(range(len(counts)))])
    apart = run([[i] for i in range(len(counts))])
    for bufs, how in ((together, "rows"), (apart, "one launch per segment")):
        for j, (k, what) in enumerate(((0, "param"), (2, "exp_avg"), (3, "exp_avg_sq"))):
            bufs[k].check([w[j] for w in want], (what, shape, gated, how))
        bufs[1].check(None, ("grad", shape, gated, how))
    for a, b in zip(together, apart):
        assert torch.equal(a.t, b.t), (shape, gated, "the grid shows in the bits")


def _lamb_hypers(n):
    import lamb_ref
    return [lamb_ref.hyper(1e-2, betas=(0.9 - 0.1 * (i % 3), 0.999), eps=1e-6,
                           weight_decay=(0.0, 1e-2)[i % 2], step=1 + i) for i in range(n)]


@pytest.mark.parametrize("shape", ll.UPDATE_SHAPES)
@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_lamb_moments_rows_grid(dev, dt, shape):
    import lamb_ref
    from kungfu_amd import ops
    counts, segs = _update_data("lamb-" + dt, shape, dt, 16)
    hs = _lamb_hypers(len(counts))
    p, g, m, v = _seat(segs, counts, dt, dev)
    u = Seated([None] * len(counts), counts, dt, dev)
    ops.lamb_moments_batch_(p.views(), g.views(), m.views(), v.views(), u.views(), hs, np_=UPDATE_NP)
    torch.cuda.synchronize()
    want = [lamb_ref.moments(*seg, dt, h, UPDATE_NP) for seg, h in zip(segs, hs)]
    for j, (buf, what) in enumerate(((m, "exp_avg"), (v, "exp_avg_sq"), (u, "update"))):
        buf.check([w[j] for w in want], (what, dt, shape))
    p.check(None, ("param", dt, shape))
    g.check(None, ("grad", dt, shape))


@pytest.mark.parametrize("shape", ll.UPDATE_SHAPES)
@pytest.mark.parametrize("dt", _BITS16)
def test_lamb_master_moments_rows_grid(dev, dt, shape):
    import lamb_ref
    from kungfu_amd import ops
    counts, segs = _master_data("lamb_master-" + dt, shape, dt, 17)
    hs = _lamb_hypers(len(counts))
    g = Seated([seg[1] for seg in segs], counts, dt, dev)
    w, m, v = (Seated([seg[j] for seg in segs], counts, "f32", dev) for j in (0, 2, 3))
    u = Seated([None] * len(counts), counts, "f32", dev)
    ops.lamb_master_moments_batch_(g.views(), w.views(), m.views(), v.views(), u.views(), hs,
                                   np_=UPDATE_NP)
    torch.cuda.synchronize()
    want = [lamb_ref.moments(sw_, lamb_ref.widen16(sg, dt), sm, sv, "f32", h, UPDATE_NP)
            for (sw_, sg, sm, sv), h in zip(segs, hs)]
    for j, (buf, what) in enumerate(((m, "exp_avg"), (v, "exp_avg_sq"), (u, "update"))):
        buf.check([x[j] for x in want], (what, dt, shape))
    w.check(None, ("master", dt, shape))
    g.check(None, ("grad", dt, shape))


# ---- A3. grid-stride under a lowered block cap (keep these last) ---------------------------

_geometry = {"cap": None}


def _default_launch_check(lib, orc, pool, dev):
    n = ll.count("f32", 13, 300, 3, 3)
    run_single(lib, orc, pool, dev, "f32", 3, "sum", n, 1)


@pytest.fixture(scope="module")
def capped(request, lib, orc, pool, dev):
    """The library's grid cap lowered to request.param blocks (kf_set_geometry,
    process-wide) for the tests that name it, the defaults put back after
    them and one default-geometry launch checked against the oracle."""
    cap = request.param
    assert lib.kf_set_geometry(4, cap, 1, 0) == 0
    _geometry["cap"] = cap
    try:
        yield cap
    finally:
        rc = lib.kf_set_geometry(4, 1 << 20, 1, 0)
        _geometry["cap"] = None
    assert rc == 0
    _default_launch_check(lib, orc, pool, dev)


@pytest.fixture(autouse=True)
def _default_geometry_elsewhere(request):
    """No test but those that ask for the cap runs under it."""
    if "capped" not in request.fixturenames:
        assert _geometry["cap"] is None, "the grid cap of the stride tests is still set"


stride_caps = pytest.mark.parametrize("capped", ll.STRIDE_CAPS, indirect=True,
                                      ids=["cap%d" % c for c in ll.STRIDE_CAPS])


@stride_caps
@pytest.mark.parametrize("dt,k,op", [("f32", 1, "sum"), ("f32", 1, "avg"), ("bf16", 2, "max"),
                                     ("f32", 3, "sum"), ("u8", 8, "sum")])
def test_stride_reduce(lib, orc, pool, dev, capped, dt, k, op):
    """14 tiles on `cap` blocks. kf_bucket_reduce at k = 1 is a copy, so the
    k = 1 kernel is reached through kf_bucket_reduce_avg (x / 1) as well."""
    e = ll.epv(dt)
    run_single(lib, orc, pool, dev, dt, k, op, ll.count(dt, 13, 300, e - 1, e - 1), 1)


@stride_caps
@pytest.mark.parametrize("k,op", [(3, "sum"), (9, "avg")])
def test_stride_peers(lib, orc, pool, dev, capped, k, op):
    """The peers fold, one vector per lane: 54 blocks' work on `cap` blocks."""
    run_single(lib, orc, pool, dev, "f32", k, op, ll.count("f32", 13, 300, 3, 3), 1, peers=True)


@stride_caps
@pytest.mark.parametrize("k,avg", [(1, True), (2, False), (3, False)])
def test_stride_batch(lib, orc, pool, dev, capped, k, avg):
    """The batched launch: ragged buckets through the table, then four equal
    buckets of 7 tiles as a rows grid of `cap` blocks a row."""
    run_batch(lib, orc, pool, dev, ll.stride_buckets("f32"), "f32", k, avg)
    run_batch(lib, orc, pool, dev, ll.stride_equal_buckets("f32"), "f32", k, avg)


@stride_caps
@pytest.mark.parametrize("dt,np_", [("f32", 3), ("bf16", 4)])
def test_stride_sma(lib, orc, pool, dev, capped, dt, np_):
    """kf_sma_blend and kf_sma_blend_batch on `cap` blocks per bucket."""
    from kungfu_amd import _lib
    from oracle.oracle import DT, NP
    e, isz = ll.epv(dt), ll.ITEMSIZE[dt]
    n = ll.count(dt, 13, 300, e - 1, e - 1)
    (vh, _), (sh, sp) = pool.input(dt, 0, n, 1), pool.input(dt, 1, n, ll.input_offset(1, dt))
    buf, pre = out_buffer(n, dt, 1, dev)
    buf[pre * isz:(pre + n) * isz] = torch.from_numpy(vh.view(np.uint8)).to(dev)
    rc = lib.kf_sma_blend(buf.data_ptr() + pre * isz, sp, n, DT[dt], np_, ALPHA, stream())
    assert rc == 0, lib.kf_last_error()
    torch.cuda.synchronize()
    check_out(buf, pre, n, dt, orc.sma_blend(vh, sh, dt, np_, ALPHA), ("sma", dt))
    # the batch: the stride buckets in flat buffers, gaps between them
    buckets = ll.stride_buckets(dt)
    offs, total = ll.flat_layout(buckets, dt)
    (vf, _), (sf, sfp) = pool.input(dt, 2, total, 0), pool.input(dt, 3, total, 0)
    flat = poisoned_bytes(total * isz, dev)
    for (c, _), o in zip(buckets, offs):
        flat[o * isz:(o + c) * isz] = torch.from_numpy(vf[o:o + c].view(np.uint8)).to(dev)
    rc = lib.kf_sma_blend_batch(
        _lib.ptr_array([flat.data_ptr() + o * isz for o in offs]),
        _lib.ptr_array([sfp + o * isz for o in offs]),
        (ctypes.c_size_t * len(buckets))(*[c for c, _ in buckets]), len(buckets), DT[dt], np_,
        ALPHA, stream())
    assert rc == 0, lib.kf_last_error()
    torch.cuda.synchronize()
    got = flat.cpu().numpy()
    for b, ((c, _), o) in enumerate(zip(buckets, offs)):
        want = orc.sma_blend(vf[o:o + c], sf[o:o + c], dt, np_, ALPHA)
        seg = got[o * isz:(o + c) * isz]
        assert golden_io.same_bits_or_nan(seg.copy().view(NP[dt]), want), (dt, b)
        seg[:] = POISON
    assert (got == POISON).all(), "a byte outside the buckets changed"


@pytest.mark.parametrize("capped", [ll.STRIDE_SERIAL_CAP], indirect=True, ids=["cap2048"])
@pytest.mark.parametrize("dt,k", ll.STRIDE_SERIAL_CASES)
def test_serial_and_stride_together(lib, orc, pool, dev, capped, dt, k):
    """2061 tiles on 2048 blocks: the one-in-flight schedule, and thirteen
    blocks take a second tile."""
    run_single(lib, orc, pool, dev, dt, k, "sum", ll.single_shape("S_stride", dt, 1), 1)
