"""Every f16 and bf16 value through the element-wise kernels on the GPU, bit
for bit against the references (NaNs by position): the /np average, the
two-input plain ops, the SMA blend, the pair average, the segmented norm's
terms, and the SGD, Adam and master-weight Adam updates. The inputs, layouts
and references are tests/sweep16.py's; tests/test_sweep16.py asserts on the
CPU that every pattern passes through a full tile and through a scalar edge
of each kernel and that the references hold the overflows, subnormals,
underflows, -0s, NaNs and inexact results the cases exist for.

Every array sits in a buffer pre-filled with a guard pattern, at least one
16-byte vector of it before and after every segment, which must come back
unchanged; inputs that a kernel only reads must come back unchanged too.

What these cases catch that the hand-picked specials did not, measured on
libraries with one rounding site changed: PairElt<bf16_t>::avg without the
narrowing after the add fails test_pair_average[bf16] (540 elements, vector
body and tails: sums past the largest finite value that the halving brings
back); NormElt<f16_t>::var with a product that saturates instead of
overflowing fails test_segnorm_terms[f16-var] (16,386 segments of the b sweep
at a = 0 alone). Neither fails tests/test_pairavg_gpu.py or
tests/test_monitor_gpu.py. A plain f32_to_f16 of the f16 products (the -0
defect of the /np average's scalar edges) fails test_avg[f16] at every
power-of-two np, head and tail, and test_sgd_update[f16-4].

The kernels added after that sweep: the gated Adam updates (bf16, and bf16 /
f16 gradients on fp32 masters) at grad_mul = 2^-16 and 0.37, one call per
decay mode; the stochastic-rounding update (p, g, m and v through widen, the
fp32 update, sr(p'), rne(m'), sr(v'); one segment over element 2^32, one up
to 2^33) and its gated twin; LAMB's master moments pass; and the narrowing of
LAMB's master apply pass through its scalar heads, 16-byte units and scalar
tails. Measured on an MI355X: these 39 cases take 38 s (the 55 before them
32 s); the slowest are test_adam_update_gated_bf16 (1.3 to 2.1 s a case, three
calls each), test_adam_sr_update (1.3 to 1.5 s) and
test_adam_master_update_gated (0.7 to 0.9 s). With one line of a kernel
changed: without the g * grad_mul multiply every gated case fails; with p
narrowed by r_v's bits every stochastic-rounding case; with the scalar tail on
the blocks after the first (`blk` for `blk == 0`) every update case; with
truncation in the apply pass's narrowing test_lamb_master_apply_narrowing of
that type, in head, unit and tail.
"""
import ctypes

import numpy as np
import pytest

import sweep16 as sw

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

DTS = sw.DTS
TORCH = {"f16": torch.float16, "bf16": torch.bfloat16}


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


@pytest.fixture(scope="module", autouse=True)
def orc():
    from oracle import oracle
    oracle.build()
    return oracle


def stream():
    return torch.cuda.current_stream().cuda_stream


def c_array(ctype, values):
    """A ctypes array from a numpy array of addresses or counts."""
    a = np.ascontiguousarray(values, dtype=np.uint64)
    return (ctype * a.size).from_buffer_copy(a.tobytes())


class Placed:
    """One role's logical array over a Layout in a guarded device buffer:
    segment i starts `residues[i]` elements (default: the layout's) past a
    16-byte boundary. `logical` None: guard-filled (an output)."""

    def __init__(self, dev, lay, logical=None, residues=None, f32=False):
        self.lay = lay
        self.phys, self.pstart, self.size = lay.physical(residues)
        assert self.phys.min() >= sw.EPV and self.phys.max() < self.size - sw.EPV
        self.np_t, self.isz = (np.uint32, 4) if f32 else (np.uint16, 2)
        self.guard = sw.GUARD_F32 if f32 else sw.GUARD
        self.host = np.full(self.size, self.guard, self.np_t)
        self.used = np.zeros(self.size, bool)
        self.used[self.phys] = True
        if logical is not None:
            self.host[self.phys] = np.ascontiguousarray(logical).view(self.np_t)
        self.t = torch.from_numpy(self.host.view(np.int32 if f32 else np.int16).copy()).to(dev)
        assert self.t.data_ptr() % 16 == 0

    def load(self, logical):
        """Replace the contents in place (the pointers stay)."""
        self.host[self.phys] = np.ascontiguousarray(logical).view(self.np_t)
        self.t.copy_(torch.from_numpy(self.host.view(np.int32 if self.isz == 4 else np.int16)))

    def ptrs(self):
        return self.t.data_ptr() + self.isz * self.pstart.astype(np.uint64)

    def ptr(self, i=0):
        return int(self.ptrs()[i])

    def views(self, tdt):
        tv = self.t.view(tdt)
        return [tv[a:a + n] for a, n in zip(self.pstart.tolist(), self.lay.n.tolist())]

    def fetch(self):
        """(the logical array now on the device, whether every guard element
        still holds the guard)."""
        back = self.t.cpu().numpy().view(self.np_t)
        return back[self.phys], bool((back[~self.used] == self.guard).all())

    def unchanged(self):
        got, ok = self.fetch()
        return ok and np.array_equal(got, self.host[self.phys])


def check(fails, tag, s, role, placed):
    """placed's contents against the reference s.want[role]."""
    got, guards = placed.fetch()
    want = s.want[role]
    if want.dtype == np.uint16:
        bad = sw.mismatches(s.dt, got, want)
    else:
        bad = sw.mismatches_float(got.view(np.float32), want)
    if bad.size:
        regs = "+".join(sw.REGION_NAMES[r] for r in np.unique(s.layout.label[bad]))
        fails.append((tag, role, "%d wrong in %s" % (bad.size, regs),
                      [(int(i), hex(int(got[i])), hex(int(want.view(got.dtype)[i]))) for i in bad[:4]]))
    if not guards:
        fails.append((tag, role, "guard elements overwritten"))


# ---- a. the /np average ------------------------------------------------------------------

@pytest.mark.parametrize("np_", sw.AVG_NPS)
@pytest.mark.parametrize("dt", DTS)
def test_avg(lib, dev, dt, np_):
    from kungfu_amd import _lib
    from oracle.oracle import DT
    sweeps = sw.avg_sweeps(dt, np_)
    fails = []
    for place, _, ioff in sw.FLAT_PLACEMENTS:
        s = sweeps[place]
        x = Placed(dev, s.layout, s.inputs["x"], residues=[ioff(0)])
        out = Placed(dev, s.layout)
        rc = lib.kf_bucket_reduce_avg(_lib.ptr_array([x.ptr()]), 1, out.ptr(), s.layout.total,
                                      DT[dt], np_, stream())
        assert rc == 0, lib.kf_last_error()
        torch.cuda.synchronize()
        check(fails, place, s, "out", out)
        assert x.unchanged(), place
    s = sweeps["batch"]
    x, out = Placed(dev, s.layout, s.inputs["x"]), Placed(dev, s.layout)
    nb = len(s.layout.n)
    rc = lib.kf_bucket_reduce_batch(c_array(ctypes.c_void_p, x.ptrs()), 1,
                                    c_array(ctypes.c_void_p, out.ptrs()),
                                    c_array(ctypes.c_size_t, s.layout.n), nb, DT[dt], 0, np_, stream())
    assert rc == 0, lib.kf_last_error()
    torch.cuda.synchronize()
    check(fails, "batch", s, "out", out)
    assert x.unchanged()
    assert not fails, (len(fails), fails[:8])


# ---- b. the two-input plain ops -------------------------------------------------------

@pytest.mark.parametrize("dt,op", [(dt, op) for dt in DTS for op in sw.PAIR_OPS[dt]])
def test_pair_ops(lib, dev, dt, op):
    """Every pattern with every partner, in both operand orders. MIN, MAX and
    PROD take one launch per bucket inside the batch entry point."""
    from kungfu_amd import _lib
    from oracle.oracle import DT, OPS
    sweeps = sw.pair_sweeps(dt, op)
    fails = []
    for place, _, ioff in sw.FLAT_PLACEMENTS:
        s = sweeps[place]
        x = Placed(dev, s.layout, s.inputs["x"], residues=[ioff(0)])
        y = Placed(dev, s.layout, s.inputs["y"], residues=[ioff(1)])
        out = Placed(dev, s.layout)
        rc = lib.kf_bucket_reduce(_lib.ptr_array([x.ptr(), y.ptr()]), 2, out.ptr(), s.layout.total,
                                  DT[dt], OPS[op], stream())
        assert rc == 0, lib.kf_last_error()
        torch.cuda.synchronize()
        check(fails, place, s, "out", out)
        assert x.unchanged() and y.unchanged(), place
    s = sweeps["batch"]
    x, y = Placed(dev, s.layout, s.inputs["x"]), Placed(dev, s.layout, s.inputs["y"])
    out = Placed(dev, s.layout)
    ins = np.stack((x.ptrs(), y.ptrs()), axis=1).reshape(-1)  # bucket b's inputs at 2b, 2b + 1
    rc = lib.kf_bucket_reduce_batch(c_array(ctypes.c_void_p, ins), 2,
                                    c_array(ctypes.c_void_p, out.ptrs()),
                                    c_array(ctypes.c_size_t, s.layout.n), len(s.layout.n), DT[dt],
                                    OPS[op], 0, stream())
    assert rc == 0, lib.kf_last_error()
    torch.cuda.synchronize()
    check(fails, "batch", s, "out", out)
    assert x.unchanged() and y.unchanged()
    if op in ("min", "max"):  # an input's own bits, NaNs too
        got = out.fetch()[0]
        assert ((got == s.inputs["x"]) | (got == s.inputs["y"])).all()
    assert not fails, (len(fails), fails[:8])


# ---- c. the SMA blend --------------------------------------------------------------------

@pytest.mark.parametrize("np_,alpha", sw.SMA_CASES)
@pytest.mark.parametrize("dt", DTS)
def test_sma_blend(lib, dev, dt, np_, alpha):
    import epilogue_specials as es
    from oracle.oracle import DT
    sweeps = sw.sma_sweeps(dt, np_, alpha)
    fails = []
    for place, voff, soff in es.SMA_PLACEMENTS:
        s = sweeps[place]
        assert int(s.layout.res[0]) == voff
        v = Placed(dev, s.layout, s.inputs["v"])
        sm = Placed(dev, s.layout, s.inputs["s"], residues=[soff])
        rc = lib.kf_sma_blend(v.ptr(), sm.ptr(), s.layout.total, DT[dt], np_, alpha, stream())
        assert rc == 0, lib.kf_last_error()
        torch.cuda.synchronize()
        check(fails, place, s, "v", v)
        assert sm.unchanged(), place
    s = sweeps["batch"]
    v, sm = Placed(dev, s.layout, s.inputs["v"]), Placed(dev, s.layout, s.inputs["s"])
    rc = lib.kf_sma_blend_batch(c_array(ctypes.c_void_p, v.ptrs()), c_array(ctypes.c_void_p, sm.ptrs()),
                                c_array(ctypes.c_size_t, s.layout.n), len(s.layout.n), DT[dt], np_,
                                alpha, stream())
    assert rc == 0, lib.kf_last_error()
    torch.cuda.synchronize()
    check(fails, "batch", s, "v", v)
    assert sm.unchanged()
    assert not fails, (len(fails), fails[:8])


# ---- d. the pair average -----------------------------------------------------------------

@pytest.mark.parametrize("dt", DTS)
def test_pair_average(dev, dt):
    """Publish o, overwrite with v, pull: world 1, the rank averages with its
    own published model."""
    from kungfu_amd.pairavg import PeerModelStore
    s = sw.pairavg_sweep(dt)
    v = Placed(dev, s.layout, s.inputs["o"])
    store = PeerModelStore(v.views(TORCH[dt]))
    fails = []
    try:
        store.publish()
        v.load(s.inputs["v"])
        store.pull_average_(0)
        assert store.counters() == dict(valid=1, torn=0, empty=0, published=1)
        check(fails, "pull", s, "v", v)
    finally:
        store.close()
    assert not fails, fails


# ---- e. the segmented norm ---------------------------------------------------------------

def _bits64(a):
    return np.ascontiguousarray(a).view(np.uint64)


@pytest.mark.parametrize("mode", ["sq", "var"])
@pytest.mark.parametrize("dt", DTS)
def test_segnorm_terms(dev, dt, mode):
    """65,536 segments of 16 elements, one non-zero term each: out[s] is that
    term's square exactly. Plans: aligned; every segment one element along (7
    head elements, a vector, a tail element); for "var" also b one element
    along against an aligned a (the mismatched-residue load)."""
    from kungfu_amd import ops
    nseg, L, tdt = sw.NPAT, sw.SEG_LEN, TORCH[dt]
    size = nseg * L + 4 * sw.EPV
    bufs = {r: torch.empty(size, dtype=torch.int16, device=dev) for r in ("a", "b")}
    obuf = torch.empty(nseg + 1 + 8, dtype=torch.float64, device=dev)
    out = obuf[4:4 + nseg + 1]
    oguard = np.float64(-1.2345e300)

    def rows(role, res):
        return bufs[role].view(tdt)[sw.EPV + res:sw.EPV + res + nseg * L].view(nseg, L).unbind(0)

    placements = [(0, 0), (1, 1)] + ([(0, 1)] if mode == "var" else [])
    plans = {}
    fails = []
    try:
        for ra, rb in placements:
            a = rows("a", ra)
            plans[ra, rb] = ops.SegNorm(list(zip(a, rows("b", rb))) if mode == "var" else list(a))
        for cfg in [c for c in sw.segnorm_configs(dt) if c[0] == mode]:
            for (ra, rb), plan in plans.items():
                for rot in sw.SEG_ROTATIONS[ra]:
                    a, b, want, _ = sw.segnorm_case(dt, *cfg, rot)
                    host = {}
                    for role, arr, res in (("a", a, ra), ("b", b, rb)):
                        if arr is None:
                            continue
                        h = np.full(size, sw.GUARD, np.uint16)
                        h[sw.EPV + res:sw.EPV + res + nseg * L] = arr.reshape(-1)
                        host[role] = h
                        bufs[role].copy_(torch.from_numpy(h.view(np.int16)))
                    obuf.fill_(float(oguard))
                    plan.run(mode, out=out)
                    torch.cuda.synchronize()
                    back = obuf.cpu().numpy()
                    got = back[4:4 + nseg]
                    bad = sw.mismatches_float(got, want)
                    tag = (cfg, (ra, rb), rot)
                    if bad.size:
                        lab = sw.segnorm_regions(ra, mode)[sw.segnorm_position(rot)[bad]]
                        fails.append((tag, "%d wrong in %s" % (bad.size, "+".join(
                            sw.REGION_NAMES[r] for r in np.unique(lab))),
                            [(int(i), hex(int(_bits64(got)[i])), hex(int(_bits64(want)[i])))
                             for i in bad[:4]]))
                    assert (back[:4] == oguard).all() and (back[-4:] == oguard).all(), tag
                    for role, h in host.items():
                        assert np.array_equal(bufs[role].cpu().numpy().view(np.uint16), h), tag
    finally:
        for p in plans.values():
            p.close()
    assert not fails, (len(fails), fails[:8])


# ---- f, g, h. the update kernels -----------------------------------------------------------

def _run_update(dev, s, roles16, roles32, call, written):
    """Place every role, call the op on the segments' views, compare the
    written roles with the reference and the others with what went in."""
    tdt = TORCH[s.dt]
    placed = {r: Placed(dev, s.layout, s.inputs.get(r)) for r in roles16}
    placed.update({r: Placed(dev, s.layout, s.inputs.get(r), f32=True) for r in roles32})
    views = {r: placed[r].views(tdt) for r in roles16}
    views.update({r: placed[r].views(torch.float32) for r in roles32})
    hypers = [s.hypers[i] for i in s.hyper_of_seg]
    call(views, hypers)
    torch.cuda.synchronize()
    fails = []
    for r in roles16 + roles32:
        if r in written:
            check(fails, s.params, s, r, placed[r])
        else:
            assert placed[r].unchanged(), (r, "was written")
    assert not fails, (len(fails), fails[:8])


@pytest.mark.parametrize("np_", sw.SGD_NPS)
@pytest.mark.parametrize("dt", DTS)
def test_sgd_update(dev, dt, np_):
    from kungfu_amd import ops
    s = sw.sgd_sweep(dt, np_)
    _run_update(dev, s, ("p", "g", "m"), (),
                lambda v, h: ops.sgd_update_batch_(v["p"], v["g"], v["m"], h, np_=np_),
                written=("p", "m"))


@pytest.mark.parametrize("step", sw.ADAM_STEPS)
@pytest.mark.parametrize("np_", sw.ADAM_NPS)
def test_adam_update_bf16(dev, np_, step):
    from kungfu_amd import ops
    s = sw.adam_sweep(np_, step)
    _run_update(dev, s, ("p", "g", "m", "v"), (),
                lambda v, h: ops.adam_update_batch_(v["p"], v["g"], v["m"], v["v"], h, np_=np_),
                written=("p", "m", "v"))


@pytest.mark.parametrize("step", sw.ADAM_STEPS)
@pytest.mark.parametrize("np_", sw.ADAM_NPS)
@pytest.mark.parametrize("dt", DTS)
def test_adam_master_update(dev, dt, np_, step):
    from kungfu_amd import ops
    s = sw.master_sweep(dt, np_, step)
    _run_update(dev, s, ("p16", "g"), ("w", "m", "v"),
                lambda v, h: ops.adam_master_update_batch_(v["p16"], v["g"], v["w"], v["m"], v["v"],
                                                           h, np_=np_),
                written=("p16", "w", "m", "v"))


# ---- i, j. the gated updates --------------------------------------------------------------

def _gate_tensors(s):
    """The sweep's gate and step state on the device; the kernel reads group
    1 of two."""
    import step_gate_ref
    import test_sharded_adam_gated as gated
    from kungfu_amd import ops
    g, st = ops.new_step_gate("cuda"), ops.new_step_states("cuda", 2)
    gated.write_gate(g, s.gate)
    gated.write_states(st, [step_gate_ref.new_state(), s.state])
    return g, st


@pytest.mark.parametrize("mul", sw.GATED_MULS)
@pytest.mark.parametrize("step", sw.ADAM_STEPS)
@pytest.mark.parametrize("np_", sw.ADAM_NPS)
def test_adam_update_gated_bf16(dev, np_, step, mul):
    """One call per row of ROWS: the gated entry takes one hyper."""
    from kungfu_amd import ops
    for row in range(sw.NROWS):
        s = sw.gated_adam_sweep(np_, step, mul, row)
        g, st = _gate_tensors(s)
        _run_update(dev, s, ("p", "g", "m", "v"), (),
                    lambda v, h: ops.adam_update_batch_gated_(v["p"], v["g"], v["m"], v["v"], h[0],
                                                              g, st, group=1, np_=np_),
                    written=("p", "m", "v"))


@pytest.mark.parametrize("mul", sw.GATED_MULS)
@pytest.mark.parametrize("step", sw.ADAM_STEPS)
@pytest.mark.parametrize("np_", sw.ADAM_NPS)
@pytest.mark.parametrize("dt", DTS)
def test_adam_master_update_gated(dev, dt, np_, step, mul):
    from kungfu_amd import ops
    for row in range(sw.NROWS):
        s = sw.gated_master_sweep(dt, np_, step, mul, row)
        g, st = _gate_tensors(s)
        _run_update(dev, s, ("p16", "g"), ("w", "m", "v"),
                    lambda v, h: ops.adam_master_update_batch_gated_(
                        v["p16"], v["g"], v["w"], v["m"], v["v"], h[0], g, st, group=1, np_=np_),
                    written=("p16", "w", "m", "v"))


# ---- k. the stochastic-rounding update -------------------------------------------------------

@pytest.mark.parametrize("step", sw.ADAM_STEPS)
@pytest.mark.parametrize("np_", sw.ADAM_NPS)
def test_adam_sr_update(dev, np_, step):
    from kungfu_amd import ops
    s = sw.sr_sweep(np_, step)
    _run_update(dev, s, ("p", "g", "m", "v"), (),
                lambda v, h: ops.adam_sr_update_batch_(v["p"], v["g"], v["m"], v["v"], h,
                                                       s.bases.tolist(), s.streams.tolist(),
                                                       sw.SR_KEY, np_=np_),
                written=("p", "m", "v"))


def test_adam_sr_update_gated(dev):
    """The unscale: grad_mul = 2^-16, a row of ROWS per call."""
    from kungfu_amd import ops
    np_, step, mul = 3, sw.ADAM_STEPS[1], sw.GATED_MULS[0]
    for row in range(sw.NROWS):
        s = sw.sr_gated_sweep(np_, step, mul, row)
        g, st = _gate_tensors(s)
        _run_update(dev, s, ("p", "g", "m", "v"), (),
                    lambda v, h: ops.adam_sr_update_batch_gated_(
                        v["p"], v["g"], v["m"], v["v"], h[0], g, st, s.bases.tolist(),
                        s.streams.tolist(), sw.SR_KEY, group=1, np_=np_),
                    written=("p", "m", "v"))


# ---- l. LAMB's master moments pass -----------------------------------------------------------

@pytest.mark.parametrize("wd", sw.LAMB_WDS)
@pytest.mark.parametrize("np_", sw.LAMB_NPS)
@pytest.mark.parametrize("dt", DTS)
def test_lamb_master_moments(dev, dt, np_, wd):
    from kungfu_amd import ops
    s = sw.lamb_master_sweep(dt, np_, wd)
    _run_update(dev, s, ("g",), ("w", "m", "v", "u"),
                lambda v, h: ops.lamb_master_moments_batch_(v["g"], v["w"], v["m"], v["v"], v["u"],
                                                            h, np_=np_),
                written=("m", "v", "u"))


# ---- m. LAMB's master apply pass: the narrowing ------------------------------------------------

@pytest.mark.parametrize("dt", DTS)
def test_lamb_master_apply_narrowing(dev, dt):
    """The narrowing grid through the scalar heads, the 16-byte units and the
    scalar tails of the apply pass, u = 0 and a negative nlr: the fp32
    parameter comes back as it went in (-0 too), p16 is its round-to-nearest
    narrowing, and the guard words between the pieces of all three arrays
    keep their bits."""
    from kungfu_amd import ops
    c = sw.apply_case(dt)
    p = torch.from_numpy(c.p.view(np.int32).copy()).to(dev).view(torch.float32)
    u = torch.from_numpy(c.u.view(np.int32).copy()).to(dev).view(torch.float32)
    p16 = torch.from_numpy(np.full(c.size, sw.GUARD, np.uint16).view(np.int16)).to(dev).view(TORCH[dt])
    assert all(t.data_ptr() % 16 == 0 for t in (p, u, p16))

    def views(t):
        (a, n), (b, hrows), (cc, trows) = c.long, c.heads, c.tails
        return ([t[a:a + n]] + list(t[b:b + 16 * hrows].view(hrows, 16)[:, 1:8].unbind(0))
                + list(t[cc:cc + 8 * trows].view(trows, 8)[:, 0:3].unbind(0)))
    vp, vu, v16 = views(p), views(u), views(p16)
    assert len(vp) == len(c.pieces)
    for i in (0, 1, len(vp) - 1):  # the views are the pieces
        assert vp[i].data_ptr() == p.data_ptr() + 4 * c.pieces[i][0] and vp[i].numel() == c.pieces[i][1]
    plan = ops.LambApplyPlan(vp, vu, [0] * len(vp), 1, v16)
    try:
        plan.run(torch.tensor([sw.APPLY_NLR], dtype=torch.float64, device=dev))
        torch.cuda.synchronize()
    finally:
        plan.close()
    gp = p.cpu().numpy().view(np.uint32)
    g16 = p16.view(torch.int16).cpu().numpy().view(np.uint16)
    names = ("head", "unit", "tail")
    bad = sw.mismatches_float(gp.view(np.float32), c.p.view(np.float32))
    assert bad.size == 0, ("fp32 parameter", dt, sorted({names[r] for r in c.label[bad] if r >= 0}),
                           [(int(i), hex(int(gp[i])), hex(int(c.p[i]))) for i in bad[:8]])
    bad = sw.mismatches(dt, g16, c.want16)
    assert bad.size == 0, ("p16", dt, sorted({names[r] for r in c.label[bad] if r >= 0}),
                           [(int(i), hex(int(c.p[i])), hex(int(g16[i])), hex(int(c.want16[i])))
                            for i in bad[:8]])
    assert np.array_equal(u.cpu().numpy().view(np.uint32), c.u), "the update was written"
    # -0 went through all three paths
    neg0 = c.used & (c.p == 0x80000000)
    assert {int(r) for r in c.label[neg0]} == {0, 1, 2} and (g16[neg0] == 0x8000).all()
