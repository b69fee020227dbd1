"""What tests/test_sweep16_gpu.py relies on, checked on the CPU from the
inputs and the references alone (no device).

For every GPU case: each of the 65,536 patterns occurs in the swept role,
passes through a full-tile vector position and through a scalar edge (head or
tail) of the kernel under test, by the layout helpers of tests/sweep16.py; and
the reference's output holds the classes the case exists for (an overflow
from finite inputs, a subnormal, an underflow to zero, a -0, a NaN, an inexact
result). The two segmented-norm layouts have no full tile by design (segments
of 16 elements): there the vector position is one of the ragged tile's.

And every single-operation step of the references (add, multiply, subtract,
the /np division, the halving, the square root) is compared with exact
rational arithmetic rounded once to the 16-bit type, ties to even, on the
partner x partner grid and 4,096 random pairs per format.
"""
import math
from fractions import Fraction

import numpy as np
import pytest

import epilogue_specials
import sweep16 as sw

DTS = sw.DTS


@pytest.fixture(scope="module", autouse=True)
def orc():
    from oracle import oracle
    oracle.build()
    return oracle


def _holds_all(values, idx):
    return np.bincount(values[idx], minlength=sw.NPAT).all()


# ---- the values and the helpers --------------------------------------------------------

@pytest.mark.parametrize("dt", DTS)
def test_partners_are_what_they_say(dt):
    p = sw.partners(dt)
    f = sw.widen64(dt, p)
    ebits, mbits = sw.FORMAT[dt]
    emin = 2 - (1 << (ebits - 1))
    sub, tiny = 2.0 ** (emin - mbits), 2.0 ** emin
    big = (2.0 - 2.0 ** -mbits) * 2.0 ** ((1 << (ebits - 1)) - 1)
    third = f[-3]
    mags = [0.0, sub, tiny - sub, tiny, 1.0, 1.0 + 2.0 ** -mbits, big, big / 2, np.inf, third]
    assert p.size == 2 * len(mags) + 1 >= 21
    for i, m in enumerate(mags):
        assert f[2 * i] == m and f[2 * i + 1] == -m, (i, f[2 * i], m)
        assert not np.signbit(f[2 * i]) and np.signbit(f[2 * i + 1])
    assert np.isnan(f[-1]) and p[-1] & (1 << (mbits - 1))  # quiet
    # the value nearest 1/3 has a full significand: every other bit set
    assert abs(third - 1 / 3) <= 2.0 ** -(mbits + 3) and bin(int(p[-3]) & ((1 << mbits) - 1)).count("1") >= mbits // 2
    assert np.array_equal(sw.patterns(), np.arange(65536)) and sw.patterns().dtype == np.uint16
    if dt == "f16":  # numpy states the same values independently
        fi = np.finfo(np.float16)
        assert (sub, tiny, big) == (float(fi.smallest_subnormal), float(fi.tiny), float(fi.max))


def test_constants_are_the_sources():
    """The tile constants come out of the kernel sources; where another test
    helper states one by hand it agrees."""
    import large_launch as ll
    k = sw.kernels()
    assert k["reduce"][:2] == (8, ll.TILE) and k["batch"][:2] == (8, ll.TILE)
    assert k["batch_k1"] == (8, ll.BLOCK * ll.BATCH_UNROLL_K1, ll.BATCH_SEG1)
    assert k["batch"][2] == ll.BATCH_SEG
    assert k["segnorm_sq"][1] == ll.SQ_TILE and k["segnorm_var"][1] == ll.VAR_TILE
    assert k["sgd"] == (8, ll.BLOCK * ll.SGD_UNROLL, ll.SGD_SEG)
    assert k["reduce"][1] == epilogue_specials.TILE_VECS
    assert k["batch_k1"][1] == epilogue_specials.TILE_VECS_BATCH_K1


@pytest.mark.parametrize("kernel", ["reduce", "batch_k1", "master", "segnorm_var"])
def test_layout_against_the_kernels_index_arithmetic(kernel):
    """Layout.label against the kernels' own split, element by element:
    head = elements up to the 16-byte boundary, units from there, a tile full
    when its last unit exists."""
    unit, tile, _ = sw.kernels()[kernel]
    segs = [(0, 1), (1, 15), (0, unit - 1), (0, unit * tile), (3, unit * tile + 5 * unit + 9),
            (0, 2 * unit * tile + unit + 1), (7, 1), (1, 6)]
    if unit != sw.EPV:
        segs = [(0, n) for _, n in segs]  # no head without 16-byte units
    lay = sw.Layout(kernel, segs)
    assert lay.total == sum(n for _, n in segs)
    for i, (res, n) in enumerate(segs):
        head = min(n, (8 - res) % 8)
        nunit = (n - head) // unit
        want = []
        for j in range(n):
            if j < head:
                want.append(sw.HEAD)
            elif j >= head + nunit * unit:
                want.append(sw.TAIL)
            else:
                t = (j - head) // unit // tile
                want.append(sw.FULL if (t + 1) * tile <= nunit else sw.RAGGED)
        assert np.array_equal(lay.label[lay.seg(i)], want), (kernel, i)
        assert sw.regions(res, n, unit, tile) == tuple(want.count(r) for r in range(4))
    phys, pstart, size = lay.physical()
    assert np.array_equal(pstart % 8, lay.res) and np.unique(phys).size == lay.total
    used = np.zeros(size, bool)
    used[phys] = True
    # a whole guard vector before the first segment, between neighbours, after the last
    gaps = np.flatnonzero(np.diff(np.concatenate(([1], used.astype(np.int8), [1]))))
    assert ((gaps[1::2] - gaps[0::2]) >= 8).all() and not used[:8].any() and not used[-8:].any()
    other = lay.physical(residues=(lay.res + 3) % 8 if unit == 8 else None)[1]
    assert np.array_equal(other % 8, (lay.res + 3) % 8 if unit == 8 else lay.res)


def test_mismatches_tolerates_only_nan_payloads():
    for dt in DTS:
        p = sw.partners(dt)
        q = p.copy()
        q[-1] |= 0x8001  # another NaN
        assert sw.mismatches(dt, p, q).size == 0
        for i in (0, 16):  # +0 / -0, +inf / -inf: the sign matters
            q = p.copy()
            q[i] = p[i + 1]
            assert list(sw.mismatches(dt, p, q)) == [i]
        q = p.copy()
        q[-1] = p[4]  # a NaN against a number
        assert list(sw.mismatches(dt, p, q)) == [p.size - 1]
    a = np.array([0.0, -0.0, np.nan, 1.0], np.float32)
    b = np.array([-0.0, -0.0, -np.nan, 1.0], np.float32)
    assert list(sw.mismatches_float(a, b)) == [0]


# ---- coverage of every GPU case --------------------------------------------------------

def _classes(s, out_role, exact64=None):
    """The classes present in the reference's output."""
    dt, want = s.dt, s.want[out_role]
    ins = [a for a in s.inputs.values() if a.dtype == np.uint16]
    finite = np.logical_and.reduce([sw.is_finite(dt, a) for a in ins])
    nonzero = np.zeros(want.size, bool)
    for role, mask in s.swept:
        nonzero |= mask & ~sw.is_zero(s.inputs[role])
    got = set()
    for name, m in (("overflow", finite & sw.is_inf(dt, want)),
                    ("subnormal", sw.is_subnormal(dt, want)),
                    ("underflow", nonzero & finite & sw.is_zero(want)),
                    ("negzero", want == 0x8000),
                    ("nan", sw.is_nan(dt, want))):
        if m.any():
            got.add(name)
    if exact64 is not None:
        with np.errstate(all="ignore"):
            e = exact64({r: sw.widen64(dt, a) if a.dtype == np.uint16
                         else a.astype(np.float64) for r, a in s.inputs.items()})
        fin = sw.is_finite(dt, want) & np.isfinite(e)
        if (sw.widen64(dt, want)[fin] != e[fin]).any():
            got.add("inexact")
    return got


def _check_coverage(s, full=True, edge=True):
    lay = s.layout
    for role, mask in s.swept:
        x = s.inputs[role]
        assert _holds_all(x, np.flatnonzero(mask)), (s.name, role)
        if full:
            assert _holds_all(x, np.flatnonzero(mask & (lay.label == sw.FULL))), (s.name, role, "full")
        if edge:  # the tails, and the heads of a kernel that has them
            for reg in (sw.TAIL,) + ((sw.HEAD,) if lay.res.any() else ()):
                assert _holds_all(x, np.flatnonzero(mask & (lay.label == reg))), \
                    (s.name, role, sw.REGION_NAMES[reg])


def _check_flat_and_batch(sweeps):
    """The single launch at its three starts: every pattern in a full tile,
    and head and tail reached. The batch: a full tile, a scalar head and a
    scalar tail for every pattern, in every swept role."""
    for place in ("aligned", "co1", "mixed"):
        _check_coverage(sweeps[place], edge=False)
    assert (sweeps["aligned"].layout.label == sw.TAIL).sum() == 7
    assert (sweeps["co1"].layout.label == sw.HEAD).sum() == 7
    assert not np.array_equal(sweeps["aligned"].layout.physical()[0], sweeps["co1"].layout.physical()[0])
    b = sweeps["batch"]
    _check_coverage(b)
    lab = b.layout.label
    assert (lab == sw.HEAD).sum() >= sw.NPAT and (lab == sw.TAIL).sum() >= sw.NPAT
    assert len(b.layout.n) > 2 * b.layout.per_launch  # more than one launch


ALL_CLASSES = {"overflow", "subnormal", "underflow", "negzero", "nan", "inexact"}


@pytest.mark.parametrize("np_", sw.AVG_NPS)
@pytest.mark.parametrize("dt", DTS)
def test_avg_cases(dt, np_):
    """x / np of a finite x never overflows; np = 1 is the identity (no
    underflow, nothing inexact)."""
    sweeps = sw.avg_sweeps(dt, np_)
    _check_flat_and_batch(sweeps)
    need = {"subnormal", "negzero", "nan"} | ({"underflow", "inexact"} if np_ > 1 else set())
    for s in sweeps.values():
        assert need <= _classes(s, "out", lambda x: x["x"] / np_), (s.name, np_)
    assert any(n > 16 and n & (n - 1) for n in sw.AVG_NPS) and set(range(1, 9)) | {16} <= set(sw.AVG_NPS)


@pytest.mark.parametrize("dt,op", [(dt, op) for dt in DTS for op in sw.PAIR_OPS[dt]])
def test_pair_cases(dt, op):
    """Both operand orders; MIN and MAX return an input (nothing overflows,
    nothing is inexact; a non-zero pattern does meet a zero partner)."""
    sweeps = sw.pair_sweeps(dt, op)
    _check_flat_and_batch(sweeps)
    exact = {"sum": lambda x: x["x"] + x["y"], "prod": lambda x: x["x"] * x["y"]}.get(op)
    need = ALL_CLASSES if exact else {"subnormal", "underflow", "negzero", "nan"}
    for s in sweeps.values():
        assert need <= _classes(s, "out", exact), (s.name, s.layout.kernel)
    # every (pattern, partner) pair in both orders, in the vector body
    s = sweeps["aligned"]
    p = sw.partners(dt)
    rank = np.full(sw.NPAT, -1)
    rank[p] = np.arange(p.size)
    body = s.layout.label == sw.FULL
    for a, b, mask in (("x", "y", s.swept[0][1]), ("y", "x", s.swept[1][1])):
        m = mask & body
        key = s.inputs[a][m].astype(np.int64) * p.size + rank[s.inputs[b][m]]
        assert np.bincount(key, minlength=sw.NPAT * p.size).all(), (op, a)


def test_sma_parameters_are_the_epilogue_specials():
    import test_epilogue_specials_gpu as esg
    assert sw.SMA_CASES == esg.SMA_CASES


@pytest.mark.parametrize("np_,alpha", sw.SMA_CASES)
@pytest.mark.parametrize("dt", DTS)
def test_sma_cases(dt, np_, alpha):
    """One rounding of c1*v + c2*(s/np) computed in fp32: with c1 + c2/np < 1
    two finite inputs cannot overflow."""
    sweeps = sw.sma_sweeps(dt, np_, alpha)
    _check_flat_and_batch(sweeps)
    assert (1 - alpha) + alpha / np_ < 1
    exact = lambda x: (1 - alpha) * x["v"] + alpha * (x["s"] / np_)  # noqa: E731
    for s in sweeps.values():
        assert ALL_CLASSES - {"overflow"} <= _classes(s, "v", exact), s.name


@pytest.mark.parametrize("dt", DTS)
def test_pairavg_case(dt):
    s = sw.pairavg_sweep(dt)
    _check_coverage(s)
    assert not (s.layout.res != 0).any() and not (s.layout.label == sw.HEAD).any()
    assert ALL_CLASSES <= _classes(s, "v", lambda x: 0.5 * (x["v"] + x["o"]))


@pytest.mark.parametrize("dt", DTS)
def test_segnorm_cases(dt):
    """Pattern s sits at element (s + rot) % 16 of segment s. Aligned, both
    vectors of a segment see every pattern's residue class; one element along
    the segment is 7 head elements, one vector and one tail element, and the
    two rotations run there put every pattern into a scalar edge once and
    into the vector once."""
    for mode in ("sq", "var"):
        lab0, lab1 = sw.segnorm_regions(0, mode), sw.segnorm_regions(1, mode)
        assert (lab0 == sw.RAGGED).all()
        assert list(lab1) == [sw.HEAD] * 7 + [sw.RAGGED] * 8 + [sw.TAIL]
        assert sw.SEG_ROTATIONS == {0: (0,), 1: (0, 8)}
        edge = np.zeros(sw.NPAT, bool)
        vec = np.zeros(sw.NPAT, bool)
        for rot in sw.SEG_ROTATIONS[1]:
            lab = lab1[sw.segnorm_position(rot)]
            edge |= (lab == sw.HEAD) | (lab == sw.TAIL)
            vec |= lab == sw.RAGGED
        assert edge.all() and vec.all()
    seen = set()
    for mode, role, fixed in sw.segnorm_configs(dt):
        for rot in (0, 8):
            a, b, want, term = sw.segnorm_case(dt, mode, role, fixed, rot)
            x = a if role == "a" else b
            pos = sw.segnorm_position(rot)
            assert np.array_equal(x[np.arange(sw.NPAT), pos], sw.patterns())
            for y in (a, b):
                if y is not None:  # one non-zero term per segment at the most
                    z = y.copy()
                    z[np.arange(sw.NPAT), pos] = 0
                    assert not z.any()
            t64 = sw.widen64(dt, term)
            fin = np.isfinite(t64)
            assert np.array_equal(want[fin], t64[fin] ** 2)
            assert np.array_equal(np.isnan(want), np.isnan(t64)) and (want[np.isinf(t64)] == np.inf).all()
        if mode == "var":
            av = sw.widen64(dt, a[np.arange(sw.NPAT), pos])
            bv = sw.widen64(dt, b[np.arange(sw.NPAT), pos])
            finite = np.isfinite(av) & np.isfinite(bv)
            if (finite & sw.is_inf(dt, term)).any():
                seen.add("overflow")
            if sw.is_subnormal(dt, term).any():
                seen.add("subnormal")
            if (finite & (bv != 0) & sw.is_zero(term)).any():
                seen.add("underflow")
            if (term == 0x8000).any():
                seen.add("negzero")
            if sw.is_nan(dt, term).any():
                seen.add("nan")
            with np.errstate(all="ignore"):
                e = av - bv * bv
            ok = finite & sw.is_finite(dt, term)
            if (t64[ok] != e[ok]).any():
                seen.add("inexact")
    assert seen == ALL_CLASSES, seen
    # fl_T(b * b) over all b (a = 0): overflows from a finite b, non-zero
    # subnormal products, underflows to zero from a non-zero b
    _, b, _, term = sw.segnorm_case(dt, "var", "b", "zero", 0)
    bb = sw.patterns()
    fin = sw.is_finite(dt, bb)
    assert (fin & sw.is_inf(dt, term)).sum() == 16384
    assert sw.is_subnormal(dt, term).sum() == {"f16": 11438, "bf16": 1022}[dt]
    assert (fin & ~sw.is_zero(bb) & sw.is_zero(term)).sum() == {"f16": 4944, "bf16": 15360}[dt]
    # the largest b whose square is finite is where it says
    bm = sw.largest_finite_square(dt)
    f = sw.widen(dt, np.array([bm, bm + 1, sw.special(dt, "max")], np.uint16)).astype(np.float64)
    big = f[2]
    ulp = big * 2.0 ** -(sw.FORMAT[dt][1] + 1)
    assert f[0] ** 2 < big + ulp / 2 <= f[1] ** 2


def _check_update(s, out_roles, exact64=None):
    _check_coverage(s)
    lay = s.layout
    assert not lay.res.any() and not (lay.label == sw.HEAD).any()
    per = lay.per_launch
    assert len(lay.n) > 2 * per and len(s.hypers) == s.hyper_of_seg.max() + 1
    got = set()
    for r in out_roles:
        got |= _classes(s, r, exact64 if r == out_roles[0] else None)
    return got


def _sgd64(h, np_):
    def f(x):
        g = x["g"] / np_ if np_ else x["g"]
        g = g + h["weight_decay"] * x["p"]
        if h["momentum"]:
            m = g if h["first"] else h["momentum"] * x["m"] + (1 - h["dampening"]) * g
            g = g + h["momentum"] * m if h["nesterov"] else m
        return x["p"] - h["lr"] * g
    return f


@pytest.mark.parametrize("np_", sw.SGD_NPS)
@pytest.mark.parametrize("dt", DTS)
def test_sgd_cases(dt, np_):
    import test_sharded_sgd
    s = sw.sgd_sweep(dt, np_)
    assert len(s.hypers) == 2 * len(test_sharded_sgd.ROWS)
    assert [r for r, _ in s.swept] == ["g", "p"]

    def exact(x):  # row by row: each row's block is one stretch of the arrays
        n = s.layout.total // len(s.hypers)
        return np.concatenate([_sgd64(h, np_)({r: a[i * n:(i + 1) * n] for r, a in x.items()})
                               for i, h in enumerate(s.hypers)])
    assert ALL_CLASSES <= _check_update(s, ("p", "m"), exact)
    # the three partner settings meet every pattern in the body
    for role, mask in s.swept:
        other = "p" if role == "g" else "g"
        assert np.unique(s.inputs[other][mask & (s.layout.label == sw.FULL)]).size == 3


@pytest.mark.parametrize("step", sw.ADAM_STEPS)
@pytest.mark.parametrize("np_", sw.ADAM_NPS)
def test_adam_cases(np_, step):
    import test_sharded_adam
    s = sw.adam_sweep(np_, step)
    dt = "bf16"
    assert len(s.hypers) == len(test_sharded_adam.ROWS) and [r for r, _ in s.swept] == ["p", "g", "m", "v"]
    assert ALL_CLASSES - {"inexact"} <= _check_update(s, ("p", "m", "v"))
    # the settings the sweeps of v and g are there for
    one, zero = sw.special(dt, "one"), 0
    body = s.layout.label == sw.FULL
    masks = dict(s.swept)
    for role, fixed in (("v", {"p": one, "g": zero, "m": one}), ("g", {"p": one, "m": zero, "v": zero})):
        hit = masks[role] & body
        for r, val in fixed.items():
            hit = hit & (s.inputs[r] == val)
        assert _holds_all(s.inputs[role], np.flatnonzero(hit)), role
    # a result that differs from the unrounded fp64 update: v' of the g sweep
    g = sw.widen64(dt, s.inputs["g"])
    g = g / np_ if np_ else g
    sel = masks["g"] & (s.inputs["v"] == 0) & sw.is_finite(dt, s.want["v"])
    beta2 = s.hypers[0]["betas"][1]
    assert all(h["betas"][1] == beta2 for h in s.hypers)
    wd0 = np.repeat([h["weight_decay"] == 0 or h["decoupled"] for h in s.hypers],
                    s.layout.total // len(s.hypers))
    sel &= wd0  # g itself enters v
    with np.errstate(all="ignore"):
        assert (sw.widen64(dt, s.want["v"])[sel] != ((1 - beta2) * g * g)[sel]).any()


@pytest.mark.parametrize("step", sw.ADAM_STEPS)
@pytest.mark.parametrize("np_", sw.ADAM_NPS)
@pytest.mark.parametrize("dt", DTS)
def test_master_cases(dt, np_, step):
    """The state is fp32 and only the master is narrowed; an Adam step is
    bounded by the learning rate, so of the 16-bit classes the gradient sweep
    reaches only NaN (from an inf or NaN gradient) in p16 = narrow(master').
    What it does reach is every widened gradient in the fp32 m, v and master.
    The narrowing's subnormals, ties and overflow are
    tests/test_sharded_adam_master_gpu.py's grid."""
    s = sw.master_sweep(dt, np_, step)
    got = _check_update(s, ("p16",))
    assert "nan" in got, got
    assert len(sw.MASTER_TRIPLES) == 3
    body = s.layout.label == sw.FULL
    for t in sw.MASTER_TRIPLES:
        assert _holds_all(s.inputs["g"], np.flatnonzero(body & (s.inputs["w"] == np.float32(t[0]))))
    # fp32 results that an fp64 evaluation does not reproduce: m' = b1*m + c1*g
    h = s.hypers[0]
    g = sw.widen64(dt, s.inputs["g"])
    g = g / np_ if np_ else g
    n = s.layout.total // len(s.hypers)
    b1 = h["betas"][0]
    e = b1 * s.inputs["m"][:n].astype(np.float64) + (1 - b1) * g[:n]
    fin = np.isfinite(e)
    assert (s.want["m"][:n].astype(np.float64)[fin] != e[fin]).any()


# ---- the gated, stochastic-rounding and LAMB cases ---------------------------------------

def test_newer_kernels_constants_are_the_sources():
    import test_sharded_adam_sr
    import test_sharded_lamb
    k = sw.kernels()
    assert k["adam_sr"] == (8, 256 * 4, test_sharded_adam_sr.SR_SEG)
    assert k["lamb_master"] == (4, 256 * 4, test_sharded_lamb.LAMB_MASTER_SEG)
    assert k["lamb_apply"][:2] == (4, 256 * 4)
    assert sw.NROWS == len(sw.adam_hypers(1))
    assert sw.GATED_MULS == (2.0 ** -16, 0.37)


def _no_mul(dt, g):
    """Gradients on which a finite non-zero grad_mul cannot show: zeros,
    infinities and NaNs."""
    return sw.is_zero(g) | ~sw.is_finite(dt, g)


@pytest.mark.parametrize("mul", sw.GATED_MULS)
@pytest.mark.parametrize("step", sw.ADAM_STEPS)
@pytest.mark.parametrize("np_", sw.ADAM_NPS)
def test_gated_adam_cases(np_, step, mul):
    import adam_ref
    import test_sharded_adam
    dt = "bf16"
    decays = set()
    for row in range(sw.NROWS):
        s = sw.gated_adam_sweep(np_, step, mul, row)
        assert [r for r, _ in s.swept] == ["p", "g", "m", "v"] and len(s.hypers) == 1
        assert ALL_CLASSES - {"inexact"} <= _check_update(s, ("p", "m", "v"))
        h = s.hypers[0]
        assert (h["weight_decay"], h["decoupled"]) == test_sharded_adam.ROWS[row]
        decays.add((h["weight_decay"] != 0, h["decoupled"]))
        assert s.gate["skip"] == 0 and s.gate["grad_mul"] == np.float32(mul) != 1
        assert s.state["step"] == step
        # against the ungated update of the same inputs: other bits where the
        # multiply can show, the same where it cannot
        x = s.inputs
        ungated = adam_ref.step(x["p"], x["g"], x["m"], x["v"], dt, h, np_)
        masks = dict(s.swept)
        for r, a in zip(("p", "m", "v"), ungated):
            same = sw.mismatches(dt, s.want[r], a).size == 0
            assert not same, (r, row)
            quiet = _no_mul(dt, x["g"])
            assert sw.mismatches(dt, s.want[r][quiet], a[quiet]).size == 0, (r, row)
        assert (s.want["m"][masks["g"]] != ungated[1][masks["g"]]).any()
        if mul == 2.0 ** -16:
            # R(g * 2^-16) of a subnormal g is a zero: m' and v' of the g
            # sweep's setting (p, m, v) = (1, 0, 0) are zeros there
            sub = masks["g"] & sw.is_subnormal(dt, x["g"]) & (x["m"] == 0) & (x["v"] == 0)
            if not (h["weight_decay"] != 0 and not h["decoupled"]):  # L2 adds wd * p to g
                full = sub & (s.layout.label == sw.FULL)
                assert np.unique(x["g"][full]).size == 2 * 127 and (sub & ~full).any()
                assert sw.is_zero(s.want["m"][sub]).all() and sw.is_zero(s.want["v"][sub]).all()
    assert len(decays) == 3  # all three decay modes


def _subnormal_count(s, np_, mul):
    """Distinct swept gradient patterns whose product is an fp32 subnormal."""
    mask = dict(s.swept)["g"]
    g = s.inputs["g"][mask]
    return np.unique(g[sw.subnormal_products(s.dt, g, mul, np_)]).size


@pytest.mark.parametrize("mul", sw.GATED_MULS)
@pytest.mark.parametrize("step", sw.ADAM_STEPS)
@pytest.mark.parametrize("np_", sw.ADAM_NPS)
@pytest.mark.parametrize("dt", DTS)
def test_gated_master_cases(dt, np_, step, mul):
    """With grad_mul = 2^-16 every bf16 gradient below 2^-110 in magnitude,
    the subnormals (2 * 127 patterns) and sixteen binades of normal values
    (2 * 16 * 128), gives an exact, non-zero fp32-subnormal product: 4350
    patterns at np = 0. The smallest f16 value is 2^-24: no f16 gradient
    reaches that range."""
    import adam_master_ref
    for row in range(sw.NROWS):
        s = sw.gated_master_sweep(dt, np_, step, mul, row)
        got = _check_update(s, ("p16",))
        assert "nan" in got and len(s.hypers) == 1
        h, x = s.hypers[0], s.inputs
        ungated = adam_master_ref.step(x["w"], sw.store(dt, x["g"]), x["m"], x["v"], dt, h, np_)
        quiet = _no_mul(dt, x["g"])
        for r, a in zip(("w", "m", "v"), ungated[1:]):
            assert sw.mismatches_float(s.want[r], a).size, (r, row)
            assert sw.mismatches_float(s.want[r][quiet], a[quiet]).size == 0, (r, row)
        count = _subnormal_count(s, np_, mul)
        print("fp32-subnormal products:", dt, np_, mul, count)
        if dt == "f16":
            assert count == 0
            continue
        if mul != 2.0 ** -16:  # a bf16 subnormal is an fp32 subnormal as it stands
            assert count >= 2 * 127
            continue
        assert count == (4350 if np_ == 0 else count) and count >= 4350
        if h["weight_decay"] != 0 and not h["decoupled"]:
            continue  # L2 adds wd * master to the product
        # they reach m' = c1 * that product as non-zero subnormals (m = 0)
        hit = sw.subnormal_products(dt, x["g"], mul, np_) & (x["m"] == 0)
        body = hit & (s.layout.label == sw.FULL)
        tail = hit & (s.layout.label == sw.TAIL)
        tiny = np.finfo(np.float32).tiny
        for where in (body, tail):
            m = np.abs(s.want["m"][where])
            assert ((m > 0) & (m < tiny)).sum() > 1000


@pytest.mark.parametrize("step", sw.ADAM_STEPS)
@pytest.mark.parametrize("np_", sw.ADAM_NPS)
def test_sr_cases(np_, step):
    import adam_sr_ref
    s = sw.sr_sweep(np_, step)
    dt, lay = "bf16", s.layout
    assert [r for r, _ in s.swept] == ["p", "g", "m", "v"] and len(s.hypers) == sw.NROWS
    got = _check_update(s, ("p", "m", "v"))
    assert {"overflow", "subnormal", "negzero", "nan"} <= got, got
    # negative and NaN exp_avg_sq pass through the sqrt in a full tile and in a tail
    l2 = np.repeat([h["weight_decay"] != 0 and not h["decoupled"] for h in s.hypers],
                   lay.total // len(s.hypers))  # there wd * p joins the gradient
    neg_v = dict(s.swept)["v"] & (s.inputs["v"] > 0x8000) & (s.inputs["g"] == 0) & ~l2
    assert np.unique(s.inputs["v"][neg_v & (lay.label == sw.FULL)]).size == 0x7FFF
    assert np.unique(s.inputs["v"][neg_v & (lay.label == sw.TAIL)]).size > 10000  # every third tail
    for reg in (sw.FULL, sw.TAIL):
        assert sw.is_nan(dt, s.want["p"][neg_v & (lay.label == reg)]).all()
    # the tables: a base of its own (a multiple of 8) and a stream word of
    # its own per segment, one long segment over element 2^32, a tail alone
    # up to the last element a pair index can name
    b, st = s.bases, s.streams
    assert (b % 8 == 0).all() and np.unique(b).size == b.size and np.unique(st).size == st.size
    assert (b + lay.n <= 1 << 33).all() and st.max() < 1 << 32
    k = sw.SR_STRADDLES
    assert b[k] < 1 << 32 < b[k] + lay.n[k] and (lay.label[lay.seg(k)] == sw.FULL).any()
    cut = (1 << 32) - b[k]
    assert lay.label[lay.seg(k)][cut] == sw.FULL  # the crossing is inside a full tile
    assert b[-1] + 8 == 1 << 33 and lay.n[-1] == 7 and (lay.label[lay.seg(-1 % len(lay.n))] == sw.TAIL).all()
    # stochastic somewhere: not the round-to-nearest bits; and where p' (v')
    # is a bf16 already, that bf16 whatever the random word
    for r in ("p", "v"):
        wide = s.wide[r]
        rne = sw.narrow(dt, wide)
        fin = np.isfinite(wide)
        diff = fin & (s.want[r] != rne)
        assert diff.sum() > 1000, (r, diff.sum())
        exact = fin & ((wide.view(np.uint32) & 0xFFFF) == 0)
        assert exact.sum() > 1000 and (s.want[r][exact] == rne[exact]).all()
        # never further than one bf16 from the truncation
        trunc = (wide.view(np.uint32) >> 16).astype(np.uint16)
        assert ((s.want[r][fin] == trunc[fin]) | (s.want[r][fin] == trunc[fin] + 1)).all()
    assert sw.mismatches(dt, s.want["m"], sw.narrow(dt, s.wide["m"])).size == 0
    # the whole-layout narrowing is adam_sr_ref.step segment by segment
    rng = np.random.default_rng(np_ + 10 * step)
    nbody = 12
    pick = [0, k, 2, nbody, len(lay.n) - 1] + list(rng.integers(0, len(lay.n), 60))
    for i in pick:
        sl = lay.seg(int(i))
        h = s.hypers[s.hyper_of_seg[i]]
        want = adam_sr_ref.step(*(s.inputs[r][sl] for r in ("p", "g", "m", "v")), h, int(b[i]),
                                int(st[i]), sw.SR_KEY, np_)
        for r, a in zip(("p", "m", "v"), want):
            assert sw.mismatches(dt, s.want[r][sl], a).size == 0, (i, r)
            ok = ~sw.is_nan(dt, a)
            assert np.array_equal(s.want[r][sl][ok], a[ok])


def test_sr_gated_case():
    import adam_sr_ref
    np_, step, mul = 3, sw.ADAM_STEPS[1], sw.GATED_MULS[0]
    for row in range(sw.NROWS):
        s = sw.sr_gated_sweep(np_, step, mul, row)
        lay = s.layout
        _check_update(s, ("p", "m", "v"))
        count = _subnormal_count(s, np_, mul)
        print("fp32-subnormal products, SR:", row, count)
        assert count >= 4350
        plain = sw.sr_sweep(np_, step)
        n = lay.total
        sl = slice(row * n, (row + 1) * n)
        assert np.array_equal(plain.inputs["g"][sl], s.inputs["g"])
        assert sw.mismatches(s.dt, plain.want["m"][sl], s.want["m"]).size  # grad_mul took part
        for i in (0, sw.SR_STRADDLES, len(lay.n) - 1, len(lay.n) // 2):
            seg = lay.seg(i)
            want = adam_sr_ref.step_gated(*(s.inputs[r][seg] for r in ("p", "g", "m", "v")),
                                          s.hypers[0], s.gate, s.state, int(s.bases[i]),
                                          int(s.streams[i]), sw.SR_KEY, np_)
            for r, a in zip(("p", "m", "v"), want):
                assert sw.mismatches(s.dt, s.want[r][seg], a).size == 0, (row, i, r)


@pytest.mark.parametrize("wd", sw.LAMB_WDS)
@pytest.mark.parametrize("np_", sw.LAMB_NPS)
@pytest.mark.parametrize("dt", DTS)
def test_lamb_master_cases(dt, np_, wd):
    """Every widened gradient reaches the fp32 m, v and u through a full
    tile's 8-byte loads and through the scalar tail."""
    s = sw.lamb_master_sweep(dt, np_, wd)
    _check_coverage(s)
    lay = s.layout
    assert not lay.res.any() and len(lay.n) > 2 * lay.per_launch
    assert len(s.hypers) == len(sw.ADAM_STEPS) and all(h["weight_decay"] == wd for h in s.hypers)
    assert set(s.want) == {"m", "v", "u", "g"} and np.array_equal(s.want["g"], s.inputs["g"])
    body = lay.label == sw.FULL
    for t in sw.MASTER_TRIPLES:
        assert _holds_all(s.inputs["g"], np.flatnonzero(body & (s.inputs["w"] == np.float32(t[0]))))
    g = s.inputs["g"]
    bad = ~sw.is_finite(dt, g)
    assert np.isnan(s.want["u"][bad]).all() and np.isfinite(s.want["u"][~bad]).all()
    assert np.isinf(s.want["v"][sw.is_inf(dt, g)]).all()
    # the weight decay shows in u alone
    other = sw.lamb_master_sweep(dt, np_, sw.LAMB_WDS[1 - sw.LAMB_WDS.index(wd)])
    assert sw.mismatches_float(s.want["u"], other.want["u"]).size
    assert sw.mismatches_float(s.want["m"], other.want["m"]).size == 0


@pytest.mark.parametrize("dt", DTS)
def test_apply_narrowing_case(dt):
    """Every value of the narrowing grid passes through a scalar head, a
    16-byte unit and a scalar tail of the apply pass, by the kernel's own
    split of a piece."""
    c = sw.apply_case(dt)
    unit, tile, _ = sw.kernels()["lamb_apply"]
    grid = np.unique(c.grid)
    for reg in (sw.APPLY_HEAD, sw.APPLY_UNIT, sw.APPLY_TAIL):
        assert np.array_equal(np.unique(c.p[c.label == reg]), grid), reg
    # the kernel's split, piece by piece: head = elements up to the first index
    # at which the fp32 arrays (4 to 16 bytes) and p16 (8) are all aligned
    seen = set()
    for start, n in c.pieces[:1] + c.pieces[1::997] + c.pieces[-1:]:
        head = next(h for h in range(9) if (start + h) % 4 == 0 and (start + h) % 8 == 0)
        head = min(head, n)
        nunit = (n - head) // unit
        want = [sw.APPLY_HEAD] * head + [sw.APPLY_UNIT] * (nunit * unit) + \
            [sw.APPLY_TAIL] * (n - head - nunit * unit)
        assert np.array_equal(c.label[start:start + n], want), (start, n)
        seen.add((start % 8, n, head))
    n_long = c.long[1]
    assert seen == {(0, n_long, 0), (1, 7, 7), (0, 3, 0)}
    assert n_long // unit > tile and (n_long // unit) % tile and n_long % unit  # full, ragged, tail
    # pieces do not touch: a guard element before and after every one
    starts = np.array([s for s, _ in c.pieces])
    ends = starts + np.array([n for _, n in c.pieces])
    assert (np.diff(starts) > 0).all() and (starts[1:] > ends[:-1]).all()
    assert not c.used[starts - 1].any() and not c.used[ends].any() and c.used.sum() == (ends - starts).sum()
    assert not c.used[:8].any() and not c.used[-8:].any()
    # what the narrowing is there for: ties, 16-bit subnormal results, the
    # overflow to inf from a finite value, both zeros, NaN
    f = c.p.view(np.float32)[c.used]
    w16 = c.want16[c.used]
    back = sw.widen(dt, w16).astype(np.float64)
    fin = np.isfinite(f) & sw.is_finite(dt, w16)
    mag = (w16 & 0x7FFF).astype(np.uint16)
    up = sw.widen64(dt, mag + 1) - sw.widen64(dt, mag)
    down = sw.widen64(dt, mag) - sw.widen64(dt, np.maximum(mag, 1) - 1)
    with np.errstate(invalid="ignore"):  # inf - inf
        err = np.abs(f.astype(np.float64) - back) * 2
    tie = fin & (err > 0) & ((err == up) | (err == down))
    assert tie.sum() > 3 * 30000 and ((w16[tie] & 1) == 0).all()  # ties go to even
    assert sw.is_subnormal(dt, w16).any() and (np.isfinite(f) & sw.is_inf(dt, w16)).any()
    assert (w16 == 0x8000).any() and (w16 == 0).any() and sw.is_nan(dt, w16).any()
    assert sw.APPLY_NLR < 0


# ---- the references against exact rational arithmetic ----------------------------------

def _fields(dt, b):
    ebits, mbits = sw.FORMAT[dt]
    return b >> 15, (b >> mbits) & ((1 << ebits) - 1), b & ((1 << mbits) - 1)


def _frac(dt, b):
    """A finite pattern's value."""
    ebits, mbits = sw.FORMAT[dt]
    bias = (1 << (ebits - 1)) - 1
    s, e, m = _fields(dt, b)
    v = Fraction(m) * Fraction(2) ** (1 - bias - mbits) if e == 0 else \
        Fraction((1 << mbits) + m) * Fraction(2) ** (e - bias - mbits)
    return -v if s else v


def _round(dt, mag, neg):
    """|value| as a Fraction -> the nearest pattern, ties to even, beyond the
    largest finite value's half-ulp neighbour inf; the sign is `neg`."""
    ebits, mbits = sw.FORMAT[dt]
    emin = 2 - (1 << (ebits - 1))
    inf = ((1 << ebits) - 1) << mbits
    sign = 0x8000 if neg else 0
    if mag == 0:
        return sign
    e = mag.numerator.bit_length() - mag.denominator.bit_length()
    if Fraction(2) ** e > mag:
        e -= 1
    assert Fraction(2) ** e <= mag < Fraction(2) ** (e + 1)
    e = max(e, emin)
    scaled = mag / Fraction(2) ** (e - mbits)
    n = scaled.numerator // scaled.denominator
    rem = scaled - n
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and n & 1):
        n += 1
    bits = ((e - emin) << mbits) + n  # a carry out of the significand bumps the exponent
    return sign | min(bits, inf)


def _nan(dt):
    return sw.special(dt, "nan")


def _isnan(dt, b):
    return bool(sw.is_nan(dt, np.uint16(b)))


def _isinf(dt, b):
    return bool(sw.is_inf(dt, np.uint16(b)))


def x_add(dt, a, b):
    if _isnan(dt, a) or _isnan(dt, b):
        return _nan(dt)
    if _isinf(dt, a) or _isinf(dt, b):
        if _isinf(dt, a) and _isinf(dt, b) and (a ^ b) & 0x8000:
            return _nan(dt)
        return a if _isinf(dt, a) else b
    q = _frac(dt, a) + _frac(dt, b)
    if q == 0:  # an exact zero sum is +0 unless both terms are negative (both -0)
        return 0x8000 if (a & b & 0x8000) else 0
    return _round(dt, abs(q), q < 0)


def x_sub(dt, a, b):
    return x_add(dt, a, b ^ 0x8000)


def x_mul(dt, a, b):
    if _isnan(dt, a) or _isnan(dt, b):
        return _nan(dt)
    neg = bool((a ^ b) & 0x8000)
    if _isinf(dt, a) or _isinf(dt, b):
        if (a & 0x7FFF) == 0 or (b & 0x7FFF) == 0:
            return _nan(dt)
        return sw.special(dt, "inf") | (0x8000 if neg else 0)
    return _round(dt, abs(_frac(dt, a) * _frac(dt, b)), neg)


def x_div(dt, a, d):
    if _isnan(dt, a):
        return _nan(dt)
    if _isinf(dt, a):
        return a
    return _round(dt, abs(_frac(dt, a)) / d, bool(a & 0x8000))


def x_sqrt(dt, a):
    if _isnan(dt, a) or (a & 0x8000 and a & 0x7FFF):
        return _nan(dt)
    if _isinf(dt, a) or (a & 0x7FFF) == 0:
        return a
    q = _frac(dt, a)
    t = 80  # q * 4^t is an integer of far more bits than the format keeps
    X = q * 4 ** t
    assert X.denominator == 1
    r = math.isqrt(X.numerator)
    # an inexact root lies strictly between r and r + 1: r + 1/2 rounds as it does
    y = Fraction(2 * r + (0 if r * r == X.numerator else 1), 2 ** (t + 1))
    return _round(dt, y, False)


@pytest.fixture(scope="module")
def pairs():
    """dt -> (a, b): the partner x partner grid, then 4,096 random pairs."""
    out = {}
    for dt in DTS:
        p = sw.partners(dt)
        r = np.random.default_rng(1616).integers(0, 65536, (4096, 2)).astype(np.uint16)
        out[dt] = (np.concatenate((np.repeat(p, p.size), r[:, 0])),
                   np.concatenate((np.tile(p, p.size), r[:, 1])))
        assert out[dt][0].size >= p.size ** 2 + 4096
    return out


def _exact(fn, dt, *cols):
    return np.array([fn(dt, *(int(c) for c in row)) for row in zip(*cols)], np.uint16)


def _agree(dt, got, want, what):
    assert sw.mismatches(dt, got, want).size == 0, (what, sw.describe(dt, got, want))


@pytest.mark.parametrize("dt", DTS)
def test_exact_helpers_on_known_values(dt):
    s = lambda name: sw.special(dt, name)  # noqa: E731
    assert x_add(dt, s("max"), s("max")) == s("inf") and x_add(dt, s("one"), s("one") | 0x8000) == 0
    assert x_add(dt, 0x8000, 0x8000) == 0x8000 and x_add(dt, 0x8000, 0) == 0
    assert x_add(dt, s("min_sub"), s("min_sub")) == 2 and x_mul(dt, s("min_sub"), s("min_sub") | 0x8000) == 0x8000
    assert x_div(dt, 1, 2) == 0 and x_div(dt, 3, 2) == 2 and x_div(dt, 0x8001, 2) == 0x8000  # ties to even
    assert x_mul(dt, s("inf"), 0) == _nan(dt) and x_add(dt, s("inf"), s("inf") | 0x8000) == _nan(dt)
    four = s("one") + (2 << sw.FORMAT[dt][1])
    assert x_sqrt(dt, four) == s("one") + (1 << sw.FORMAT[dt][1]) and x_sqrt(dt, 0x8000) == 0x8000
    assert x_sqrt(dt, s("one") | 0x8000) == _nan(dt)
    # every pattern survives a round trip through its own value
    for b in list(range(0, 0x7C00 if dt == "f16" else 0x7F80, 97)) + [s("max"), s("max_sub")]:
        assert _round(dt, abs(_frac(dt, b)), False) == b


@pytest.mark.parametrize("dt", DTS)
def test_oracle_sum_and_prod_are_correctly_rounded(orc, pairs, dt):
    a, b = pairs[dt]
    got = sw.bits_of(orc.transform2(sw.store(dt, a), sw.store(dt, b), dt, "sum"))
    _agree(dt, got, _exact(x_add, dt, a, b), "sum")
    if dt == "bf16":
        got = orc.transform2(a, b, dt, "prod")
        _agree(dt, got, _exact(x_mul, dt, a, b), "prod")


@pytest.mark.parametrize("dt", DTS)
def test_oracle_division_by_np_is_correctly_rounded(orc, pairs, dt):
    a = np.concatenate((sw.partners(dt), pairs[dt][0][-4096:], np.arange(0, 64, dtype=np.uint16)))
    for np_ in sw.AVG_NPS:
        got = sw.bits_of(orc.reduce_avg([sw.store(dt, a)], dt, np_))
        _agree(dt, got, _exact(lambda d, x: x_div(d, x, np_), dt, a), np_)


@pytest.mark.parametrize("dt", DTS)
def test_pairavg_blend_is_two_correct_roundings(pairs, dt):
    import pairavg_ref
    a, b = pairs[dt]
    got = sw.bits_of(pairavg_ref.blend(sw.store(dt, a), sw.store(dt, b), dt))
    _agree(dt, got, _exact(lambda d, x, y: x_div(d, x_add(d, x, y), 2), dt, a, b), "blend")


@pytest.mark.parametrize("dt", DTS)
def test_var_terms_is_two_correct_roundings(pairs, dt):
    """fl(a - fl(b * b)): the multiply and the subtract."""
    import monitor_ref
    a, b = pairs[dt]
    with np.errstate(over="ignore", invalid="ignore"):
        got = sw.bits_of(monitor_ref.var_terms(sw.store(dt, a), sw.store(dt, b), dt))
    _agree(dt, got, _exact(lambda d, x, y: x_sub(d, x, x_mul(d, y, y)), dt, a, b), "var")


@pytest.mark.parametrize("dt", DTS)
def test_sqrt_through_fp32_is_correctly_rounded(pairs, dt):
    """adam_ref's R(sqrt(v)): numpy's fp32 sqrt narrowed."""
    a = np.concatenate((sw.partners(dt), pairs[dt][0][-4096:]))
    with np.errstate(invalid="ignore"):
        got = sw.narrow(dt, np.sqrt(sw.widen(dt, a)))
    _agree(dt, got, _exact(x_sqrt, dt, a), "sqrt")


@pytest.mark.parametrize("dt", DTS)
def test_sgd_ref_np_division_is_correctly_rounded(pairs, dt):
    """sgd_ref multiplies by 2^-k for a power-of-two np: the same value as the
    division. lr = 0 and p = 0 leave g / np to be read off the momentum of a
    first step."""
    import sgd_ref
    a = np.concatenate((sw.partners(dt), pairs[dt][0][-4096:]))
    zero = np.zeros(a.size, np.uint16)
    for np_ in (3, 4):
        h = sgd_ref.hyper(0.0, momentum=0.9, first=True)
        _, m = sgd_ref.step(sw.store(dt, zero), sw.store(dt, a), sw.store(dt, zero), dt, h, np_)
        _agree(dt, sw.bits_of(m), _exact(lambda d, x: x_div(d, x, np_), dt, a), np_)
