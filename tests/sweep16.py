"""Every f16 and bf16 value through the element-wise kernels: the inputs, the
layouts and the references of tests/test_sweep16.py (CPU: the coverage every
case exists for, and the references against exact rational arithmetic) and
tests/test_sweep16_gpu.py (the kernels, bit for bit).

A 16-bit type has 65,536 values, so a unary rounding step is run on all of
them and a binary step on all of them against a fixed partner set. A case is
a Sweep: segments in a Layout, one logical array per role, the reference's
output, and which elements hold the swept role. The Layout says which
elements a kernel treats as scalar head, full tile, ragged tile and scalar
tail; its tile constants are read out of the kernel sources.

Everything here travels as uint16 bit patterns; store() gives the numpy form
the references take (float16 for f16, the bits themselves for bf16). No torch
and no GPU is needed to import this module.
"""
import functools
import os
import re

import numpy as np

from oracle.oracle import bf16_bits_to_f32, f32_to_bf16_bits

DTS = ("f16", "bf16")
FORMAT = {"f16": (5, 10), "bf16": (8, 7)}  # (exponent bits, mantissa bits)
EPV = 8            # 16-bit elements per 16-byte vector
NPAT = 1 << 16
GUARD = 0xA5A5     # what the elements around every segment hold
GUARD_F32 = 0xA5A5A5A5

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "kungfu_amd", "csrc")


# ---- values -----------------------------------------------------------------

def patterns():
    return np.arange(NPAT, dtype=np.uint16)


def special(dt, name):
    """One named magnitude of the format as a bit pattern (positive)."""
    ebits, mbits = FORMAT[dt]
    inf = ((1 << ebits) - 1) << mbits
    one = ((1 << (ebits - 1)) - 1) << mbits
    return {"zero": 0, "min_sub": 1, "max_sub": (1 << mbits) - 1, "min_normal": 1 << mbits,
            "one": one, "above_one": one + 1, "max": inf - 1, "half_max": inf - 1 - (1 << mbits),
            "inf": inf, "nan": inf | (1 << (mbits - 1)),
            # the pattern nearest 1/3: exponent of 1/4, significand 0101..01(1)
            "third": int(bits_of(narrow(dt, np.array([1.0 / 3.0], np.float32)))[0])}[name]


PARTNER_NAMES = ("zero", "min_sub", "max_sub", "min_normal", "one", "above_one", "max",
                 "half_max", "inf", "third")


@functools.lru_cache(maxsize=None)
def partners(dt):
    """The fixed partner set: for each magnitude the positive then the
    negative value, and one quiet NaN (read-only)."""
    sign = 0x8000
    out = []
    for name in PARTNER_NAMES:
        b = special(dt, name)
        out += [b, b | sign]
    out.append(special(dt, "nan"))
    a = np.array(out, dtype=np.uint16)
    a.setflags(write=False)
    return a


def bits_of(a):
    return np.ascontiguousarray(a).view(np.uint16)


def store(dt, bits):
    """Bit patterns -> the numpy form the references take."""
    bits = np.ascontiguousarray(bits, dtype=np.uint16)
    return bits.view(np.float16) if dt == "f16" else bits


def widen(dt, bits):
    """Bit patterns -> float32 values (exact)."""
    if dt == "bf16":
        return bf16_bits_to_f32(bits)
    with np.errstate(invalid="ignore"):  # a signalling NaN among the patterns
        return store(dt, bits).astype(np.float32)


def widen64(dt, bits):
    with np.errstate(invalid="ignore"):
        return widen(dt, bits).astype(np.float64)


def narrow(dt, x):
    """float32 -> bit patterns, round to nearest even."""
    x = np.asarray(x, np.float32)
    if dt == "bf16":
        return f32_to_bf16_bits(x)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        return x.astype(np.float16).view(np.uint16)


def is_nan(dt, bits):
    ebits, mbits = FORMAT[dt]
    return (np.asarray(bits) & 0x7FFF) > (((1 << ebits) - 1) << mbits)


def is_inf(dt, bits):
    return (np.asarray(bits) & 0x7FFF) == special(dt, "inf")


def is_finite(dt, bits):
    return (np.asarray(bits) & 0x7FFF) < special(dt, "inf")


def is_subnormal(dt, bits):
    m = np.asarray(bits) & 0x7FFF
    return (m > 0) & (m < special(dt, "min_normal"))


def is_zero(bits):
    return (np.asarray(bits) & 0x7FFF) == 0


def mismatches(dt, got, want):
    """Indices at which two arrays of bit patterns differ: NaNs are compared
    by position (a generated NaN's sign and payload differ between an x86
    reference and the GPU), everything else bit for bit."""
    got, want = bits_of(got), bits_of(want)
    assert got.shape == want.shape, (got.shape, want.shape)
    ng, nw = is_nan(dt, got), is_nan(dt, want)
    return np.flatnonzero((ng != nw) | (~ng & ~nw & (got != want)))


def mismatches_float(got, want):
    """The same for float32 / float64 arrays."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype
    u = {4: np.uint32, 8: np.uint64}[got.itemsize]
    ng, nw = np.isnan(got), np.isnan(want)
    return np.flatnonzero((ng != nw) | (~ng & ~nw & (got.view(u) != want.view(u))))


def describe(dt, got, want, layout=None, limit=4):
    """A short account of the mismatches for an assertion message."""
    idx = mismatches(dt, got, want)
    if idx.size == 0:
        return ""
    where = ""
    if layout is not None:
        where = " in " + "+".join(REGION_NAMES[r] for r in np.unique(layout.label[idx]))
    g, w = bits_of(got), bits_of(want)
    return "%d wrong%s: %s" % (idx.size, where,
                               ["%d: %#06x != %#06x" % (i, g[i], w[i]) for i in idx[:limit]])


# ---- the kernels' tile constants, read out of the sources -------------------------

def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _int(text, pattern):
    found = re.findall(pattern, text)
    assert len(found) == 1, (pattern, found)
    return int(found[0])


@functools.lru_cache(maxsize=None)
def kernels():
    """name -> (elements per unit, units per tile, segments per launch or
    None): a unit is what one lane loads at once (a 16-byte vector of the
    16-bit stream; four elements for the master-weight update), a tile what
    one block does per round."""
    capi, seg = _src("kf_capi.hip"), _src("kf_segnorm.hip")
    sgd, adam, master = _src("kf_sgd.hip"), _src("kf_adam.hip"), _src("kf_adam_master.hip")
    pa, hpp = _src("kf_pairavg.hip"), _src("kf_reduce_kernels.hpp")
    block = _int(capi, r"constexpr int kBlock\s*=\s*(\d+);")
    bblock = _int(capi, r"#define KF_BATCH_BLOCK (\d+)")
    sma = _int(capi, r"sma_kernel<T, C, kBlock, (\d+)>")
    assert sma == _int(capi, r"sma_batch_kernel<T, C, kBlock, (\d+)>")
    assert capi.count("grid_for(p.nvec, ned, %d)" % sma) == 2
    nblock = _int(seg, r"constexpr int kNormBlock\s*=\s*(\d+);")
    elts = _int(master, r"#define KF_ADAM_MASTER_ELTS (\d+)")
    assert "#define KF_ADAM_MASTER_UNROLL (16 / KF_ADAM_MASTER_ELTS)" in master
    return {
        "reduce": (EPV, block * _int(capi, r"int unroll\s*=\s*(\d+);"), None),
        "batch_k1": (EPV, bblock * _int(capi, r"#define KF_BATCH_UNROLL_K1 (\d+)"),
                     _int(hpp, r"constexpr int kBatchSeg1\s*=\s*(\d+);")),
        "batch": (EPV, bblock * _int(capi, r"#define KF_BATCH_UNROLL (\d+)"),
                  _int(hpp, r"constexpr int kBatchSeg\s*=\s*(\d+);")),
        "sma": (EPV, block * sma, _int(hpp, r"constexpr int kBatchSeg\s*=\s*(\d+);")),
        "segnorm_sq": (EPV, nblock * _int(seg, r"constexpr int kNormUnrollSq\s*=\s*(\d+);"), None),
        "segnorm_var": (EPV, nblock * _int(seg, r"constexpr int kNormUnrollVar\s*=\s*(\d+);"), None),
        "sgd": (EPV, _int(sgd, r"constexpr int kSgdBlock\s*=\s*(\d+);")
                * _int(sgd, r"#define KF_SGD_UNROLL (\d+)"),
                _int(sgd, r"constexpr int kSgdSeg\s*=\s*(\d+);")),
        "adam": (EPV, _int(adam, r"constexpr int kAdamBlock\s*=\s*(\d+);")
                 * _int(adam, r"#define KF_ADAM_UNROLL (\d+)"),
                 _int(adam, r"constexpr int kAdamSeg\s*=\s*(\d+);")),
        "master": (elts, _int(master, r"constexpr int kAdamMasterBlock\s*=\s*(\d+);") * (16 // elts),
                   _int(master, r"constexpr int kAdamMasterSeg\s*=\s*(\d+);")),
        "pairavg": (EPV, _int(pa, r"constexpr int kPaBlock\s*=\s*(\d+);")
                    * _int(pa, r"constexpr int kPaUnroll\s*=\s*(\d+);"), None),
    }


# ---- layouts ------------------------------------------------------------------------

HEAD, FULL, RAGGED, TAIL = 0, 1, 2, 3
REGION_NAMES = ("head", "full", "ragged", "tail")


def regions(residue, n, unit, tile_units):
    """(head, full, ragged, tail) element counts of one segment of n elements
    that starts `residue` elements past a 16-byte boundary: the scalars up to
    the boundary, the whole tiles, the last tile's units, the scalars after
    the last whole unit. Kernels without a head take residue 0 only."""
    head = min(n, (EPV - residue) % EPV)
    units = (n - head) // unit
    full = units // tile_units * tile_units
    return head, full * unit, (units - full) * unit, n - head - units * unit


class Layout:
    """Segments [(residue, n)] of one kernel, end to end in one logical
    array. label[i] is the region of logical element i."""

    def __init__(self, kernel, segs):
        self.kernel = kernel
        self.unit, self.tile_units, self.per_launch = kernels()[kernel]
        self.res = np.array([r for r, _ in segs], dtype=np.int64)
        self.n = np.array([n for _, n in segs], dtype=np.int64)
        assert ((0 <= self.res) & (self.res < EPV)).all() and (self.n > 0).all()
        self.start = np.concatenate(([0], np.cumsum(self.n)))[:-1]
        self.total = int(self.n.sum())
        head = np.minimum(self.n, (EPV - self.res) % EPV)
        units = (self.n - head) // self.unit
        full = units // self.tile_units * self.tile_units
        local = np.arange(self.total) - np.repeat(self.start, self.n)
        h, f, u = (np.repeat(x, self.n) for x in (head, head + full * self.unit,
                                                  head + units * self.unit))
        self.label = np.where(local < h, HEAD, np.where(local < f, FULL,
                              np.where(local < u, RAGGED, TAIL))).astype(np.int8)
        self.label.setflags(write=False)

    def where(self, *regs):
        return np.flatnonzero(np.isin(self.label, regs))

    def seg(self, i):
        return slice(int(self.start[i]), int(self.start[i] + self.n[i]))

    def physical(self, residues=None):
        """(index of every logical element in one flat buffer, the buffer's
        length in elements): segment i starts `residues[i]` elements (default:
        its own) past a 16-byte boundary, with at least one vector of guard
        elements before it, between neighbours and after the last."""
        res = self.res if residues is None else np.asarray(residues, dtype=np.int64)
        slot = -(-(res + self.n) // EPV) * EPV + EPV
        pstart = EPV + np.concatenate(([0], np.cumsum(slot)))[:-1] + res
        phys = np.repeat(pstart - self.start, self.n) + np.arange(self.total)
        return phys, pstart, int(EPV + slot.sum())


def body_count(kernel, n):
    """The smallest segment length that has at least n elements in full tiles,
    then a ragged tile of 300 units and a scalar tail one short of a unit."""
    unit, tile, _ = kernels()[kernel]
    per = unit * tile
    return -(-n // per) * per + 300 * unit + unit - 1


def edge_segments(kernel, n, heads):
    """Segments that put at least n elements into scalar tails and, with
    `heads`, as many into scalar heads: tails alone (a segment one element
    short of a unit) and, with `heads`, every other segment 15 elements one
    past a boundary: a head of 7, one vector, no tail."""
    unit = kernels()[kernel][0]
    ntail = -(-n // (unit - 1))
    if not heads:
        return [(0, unit - 1)] * ntail
    nhead = -(-n // (EPV - 1))
    segs = []
    for i in range(max(ntail, nhead)):
        if i < ntail:
            segs.append((0, unit - 1))
        if i < nhead:
            segs.append((1, 2 * EPV - 1))
    return segs


def spread(layout, nstream):
    """For every logical element the index into a stream of `nstream` =
    Q * 65536 entries (entry q * 65536 + p: pattern p with partner setting q):
    the vector body walks the stream in order, so a body of nstream elements
    holds it whole; the scalar heads, and the scalar tails on their own, walk
    the patterns in order once per round of 65536 elements, pattern p with
    setting p + round * (Q / rounds) modulo Q: with two rounds a pattern meets
    both halves of the stream (both operand orders)."""
    assert nstream % NPAT == 0
    q = nstream // NPAT
    idx = np.empty(layout.total, dtype=np.int64)
    body = layout.where(FULL, RAGGED)
    idx[body] = np.arange(body.size) % nstream
    for reg in (HEAD, TAIL):
        edge = layout.where(reg)
        e = np.arange(edge.size)
        p = e % NPAT
        rounds = max(1, edge.size // NPAT)
        idx[edge] = ((p + (e // NPAT) * max(1, q // rounds)) % q) * NPAT + p
    return idx


class Sweep:
    """One case: `inputs` and `want` are {role: logical array} over `layout`
    (bit patterns; float32 for the master-weight state), `swept` is a list of
    (role, mask): the elements at which that role holds the swept pattern."""

    def __init__(self, name, dt, layout, inputs, want, swept, **params):
        self.name, self.dt, self.layout = name, dt, layout
        self.inputs, self.want, self.swept = inputs, want, swept
        self.params = params
        for a in list(inputs.values()) + list(want.values()):
            a.setflags(write=False)


def _orc():
    from oracle import oracle
    return oracle


# ---- a. the /np average ---------------------------------------------------------------

AVG_NPS = (1, 2, 3, 4, 5, 6, 7, 8, 16, 23)
# the three starts of the single-launch entry points, (name, output's residue,
# residue of input j): tests/test_epilogue_specials_gpu.py's placements
FLAT_PLACEMENTS = (("aligned", 0, lambda j: 0), ("co1", 1, lambda j: 1),
                   ("mixed", 1, lambda j: (2 + j) % EPV))


def _flat_and_batch(flat_kernel, batch_kernel, nstream, nedge=NPAT):
    """The layouts of one entry-point pair: the single launch at the three
    output residues, and the batch: one long segment and the edge segments."""
    n = body_count(flat_kernel, nstream)
    lay = {name: Layout(flat_kernel, [(res, n)]) for name, res, _ in FLAT_PLACEMENTS}
    lay["batch"] = Layout(batch_kernel, [(0, body_count(batch_kernel, nstream))]
                          + edge_segments(batch_kernel, nedge, heads=True))
    return lay


@functools.lru_cache(maxsize=None)
def avg_sweeps(dt, np_):
    out = {}
    for place, lay in _flat_and_batch("reduce", "batch_k1", NPAT).items():
        x = patterns()[spread(lay, NPAT)]
        want = bits_of(_orc().reduce_avg([store(dt, x)], dt, np_))
        out[place] = Sweep("avg", dt, lay, {"x": x}, {"out": want},
                           [("x", np.ones(lay.total, bool))], np=np_)
    return out


# ---- b. the two-input plain ops -----------------------------------------------------

PAIR_OPS = {"f16": ("sum",), "bf16": ("sum", "min", "max", "prod")}


def pair_stream(dt):
    """(swept, partner, order) of 2 * P * 65536 entries: every pattern with
    every partner, the pattern as the first operand (order 0), then as the
    second (order 1)."""
    p = partners(dt)
    sw = np.tile(patterns(), 2 * p.size)
    pt = np.tile(np.repeat(p, NPAT), 2)
    order = np.repeat(np.array([0, 1], np.int8), p.size * NPAT)
    return sw, pt, order


def _pair_roles(dt, lay):
    sw, pt, order = pair_stream(dt)
    idx = spread(lay, sw.size)
    sw, pt, first = sw[idx], pt[idx], order[idx] == 0
    return np.where(first, sw, pt), np.where(first, pt, sw), first


@functools.lru_cache(maxsize=None)
def pair_layouts(dt):
    return _flat_and_batch("reduce", "batch", 2 * partners(dt).size * NPAT, 2 * NPAT)


@functools.lru_cache(maxsize=1)
def pair_sweeps(dt, op):
    out = {}
    for place, lay in pair_layouts(dt).items():
        x, y, first = _pair_roles(dt, lay)
        want = bits_of(_orc().transform2(store(dt, x), store(dt, y), dt, op))
        out[place] = Sweep("pair_" + op, dt, lay, {"x": x, "y": y}, {"out": want},
                           [("x", first), ("y", ~first)], op=op)
    return out


# ---- c. the SMA blend -----------------------------------------------------------------

SMA_CASES = ((2, 0.1), (3, 0.25), (8, 0.1))  # tests/test_epilogue_specials_gpu.py's (np, alpha)

@functools.lru_cache(maxsize=None)
def sma_layouts(dt):
    return _flat_and_batch("sma", "sma", 2 * partners(dt).size * NPAT, 2 * NPAT)


@functools.lru_cache(maxsize=1)
def sma_sweeps(dt, np_, alpha):
    """v swept against the partners as the sum, then the sum swept against
    the partners as v."""
    out = {}
    for place, lay in sma_layouts(dt).items():
        v, s, first = _pair_roles(dt, lay)
        want = bits_of(_orc().sma_blend(store(dt, v), store(dt, s), dt, np_, alpha))
        out[place] = Sweep("sma", dt, lay, {"v": v, "s": s}, {"v": want},
                           [("v", first), ("s", ~first)], np=np_, alpha=alpha)
    return out


# ---- d. the pair average ---------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def pairavg_sweep(dt):
    """Spans start 16-byte aligned: one long span and tails alone. v is the
    local model at the pull, o the published one."""
    import pairavg_ref
    nstream = 2 * partners(dt).size * NPAT
    lay = Layout("pairavg", [(0, body_count("pairavg", nstream))]
                 + edge_segments("pairavg", 2 * NPAT, heads=False))
    v, o, first = _pair_roles(dt, lay)
    want = bits_of(pairavg_ref.blend(store(dt, v), store(dt, o), dt))
    return Sweep("pairavg", dt, lay, {"v": v, "o": o}, {"v": want}, [("v", first), ("o", ~first)])


# ---- e. the segmented norm -------------------------------------------------------------

SEG_LEN = 2 * EPV          # two vectors when aligned
SEG_ROTATIONS = {0: (0,), 1: (0, EPV)}  # start residue -> rotations run there


def segnorm_configs(dt):
    """[(mode, swept role, name of the fixed value)]: "sq" sweeps a; "var"
    sweeps b against five a values and a against three b values."""
    return ([("sq", "a", None)]
            + [("var", "b", a) for a in ("zero", "one", "max", "min_sub", "inf")]
            + [("var", "a", b) for b in ("zero", "one", "bmax")])


def largest_finite_square(dt):
    """The largest b whose square rounds to a finite value, as bits."""
    b = patterns()[:special(dt, "inf")]
    with np.errstate(over="ignore"):
        ok = is_finite(dt, narrow(dt, widen(dt, b) * widen(dt, b)))
    return int(b[ok].max())


def segnorm_position(rot):
    """Element of segment s that holds pattern s."""
    return (np.arange(NPAT) + rot) % SEG_LEN


def segnorm_regions(residue, mode):
    """label of the SEG_LEN elements of a segment that starts `residue`
    elements past a boundary."""
    return Layout("segnorm_" + mode, [(residue, SEG_LEN)]).label


@functools.lru_cache(maxsize=None)
def segnorm_case(dt, mode, role, fixed, rot):
    """(a, b, want): a and b as (65536, 16) bit patterns, pattern s (or the
    fixed partner) at element (s + rot) % 16 of segment s and zeros elsewhere;
    want[s] the fp64 square of the one term. b is None for "sq"."""
    import monitor_ref
    pos = segnorm_position(rot)
    rows = np.arange(NPAT)
    a = np.zeros((NPAT, SEG_LEN), np.uint16)
    b = None
    if mode == "sq":
        a[rows, pos] = patterns()
        term = patterns()
    else:
        b = np.zeros((NPAT, SEG_LEN), np.uint16)
        fv = largest_finite_square(dt) if fixed == "bmax" else special(dt, fixed)
        a[rows, pos] = patterns() if role == "a" else fv
        b[rows, pos] = patterns() if role == "b" else fv
        with np.errstate(over="ignore", invalid="ignore"):
            term = bits_of(monitor_ref.var_terms(store(dt, a[rows, pos]), store(dt, b[rows, pos]), dt))
        # every other term is fl(0 - fl(0 * 0)) = 0
    w = widen64(dt, term)
    with np.errstate(over="ignore", invalid="ignore"):
        want = w * w  # exact: at most 22 significand bits; inf -> inf, NaN -> NaN
    for x in (a, b, want, term):
        if x is not None:
            x.setflags(write=False)
    return a, b, want, term


# ---- f, g, h. the update kernels ---------------------------------------------------------

def _update_layout(kernel, ncombo_body, ncombo_edge):
    """Per hyper row: `ncombo_body` long segments (one per sweep and partner
    triple) and `ncombo_edge` runs of tails alone (one per sweep)."""
    segs = [(0, body_count(kernel, NPAT))] * ncombo_body
    edge = edge_segments(kernel, NPAT, heads=False)
    return segs + edge * ncombo_edge, len(edge)


def _fill_update(lay, nbody, nedge_segs, roles, sweeps, env):
    """Logical arrays {role: bits} for one hyper row's block of a layout: body
    segment c = (sweep i, triple t) holds the patterns in role sweeps[i] and
    env(sweeps[i], t)[role] in the others; edge run i holds the patterns in
    role sweeps[i] in order, segment j of it with triple j % 3."""
    arrs = {r: np.empty(lay.total, np.uint16) for r in roles}
    masks = {r: np.zeros(lay.total, bool) for r in roles}
    pat = patterns()
    for c in range(nbody):
        i, t = divmod(c, 3)
        sl = lay.seg(c)
        n = sl.stop - sl.start
        for r in roles:
            arrs[r][sl] = pat[np.arange(n) % NPAT] if r == sweeps[i] else env(sweeps[i], t)[r]
        masks[sweeps[i]][sl] = True
    for i, sw in enumerate(sweeps):
        lo = nbody + i * nedge_segs
        a, b = int(lay.start[lo]), int(lay.start[lo + nedge_segs - 1] + lay.n[lo + nedge_segs - 1])
        n = b - a
        segno = np.repeat(np.arange(nedge_segs), lay.n[lo:lo + nedge_segs])
        for r in roles:
            if r == sw:
                arrs[r][a:b] = pat[np.arange(n) % NPAT]
            else:
                vals = np.array([env(sw, t)[r] for t in range(3)], np.uint16)
                arrs[r][a:b] = vals[segno % 3]
        masks[sw][a:b] = True
    return arrs, masks


def _env16(dt, fixed0):
    """The three partner settings of a 16-bit update kernel: env(sweep, t) ->
    {role: bits}. Setting 0 is `fixed0[sweep]` where given."""
    s = lambda name, neg=False: special(dt, name) | (0x8000 if neg else 0)  # noqa: E731
    base = [{"p": s("one"), "g": s("zero"), "m": s("zero"), "v": s("zero")},
            {"p": s("third"), "g": s("one"), "m": s("one", True), "v": s("above_one")},
            {"p": s("max", True), "g": s("half_max"), "m": s("min_sub"), "v": s("max")}]

    def env(sweep, t):
        d = dict(base[t])
        if t == 0:
            d.update(fixed0.get(sweep, {}))
        return d
    return env


SGD_NPS = (0, 3, 4)
SGD_LR = 0.1


def sgd_hypers():
    """tests/test_sharded_sgd.py's rows, each as a first and a later step."""
    import sgd_ref
    import test_sharded_sgd
    return [sgd_ref.hyper(SGD_LR, mu, damp, wd, nesterov, first)
            for mu, damp, wd, nesterov in test_sharded_sgd.ROWS for first in (True, False)]


class UpdateSweep(Sweep):
    """A Sweep whose segments carry a hyper row each: hyper_of_seg[i] indexes
    `hypers`."""


def _update_sweep(name, kernel, dt, hypers, roles, sweeps, env, ref, **params):
    """One call's segments: for every hyper row the block of _fill_update."""
    nbody = 3 * len(sweeps)
    block_segs, nedge = _update_layout(kernel, nbody, len(sweeps))
    block = Layout(kernel, block_segs)
    arrs, masks = _fill_update(block, nbody, nedge, roles, sweeps, env)
    lay = Layout(kernel, block_segs * len(hypers))
    inputs = {r: np.tile(a, len(hypers)) for r, a in arrs.items()}
    swept = [(r, np.tile(masks[r], len(hypers))) for r in sweeps]
    want = {}
    for h, hyper in enumerate(hypers):
        sl = slice(h * block.total, (h + 1) * block.total)
        for r, a in ref({r: inputs[r][sl] for r in roles}, hyper).items():
            want.setdefault(r, []).append(a)
    want = {r: np.concatenate(v) for r, v in want.items()}
    sw = UpdateSweep(name, dt, lay, inputs, want, swept, **params)
    sw.hypers = hypers
    sw.hyper_of_seg = np.repeat(np.arange(len(hypers)), len(block_segs))
    return sw


@functools.lru_cache(maxsize=2)
def sgd_sweep(dt, np_):
    """g swept, then p swept."""
    import sgd_ref

    def ref(x, h):
        p, m = sgd_ref.step(store(dt, x["p"]), store(dt, x["g"]), store(dt, x["m"]), dt, h, np_)
        return {"p": bits_of(p), "m": bits_of(m), "g": x["g"]}
    return _update_sweep("sgd", "sgd", dt, sgd_hypers(), ("p", "g", "m"), ("g", "p"),
                         _env16(dt, {}), ref, np=np_)


ADAM_NPS = (0, 3)
ADAM_STEPS = (1, 7)
ADAM_LR = 1e-2


def adam_hypers(step):
    import adam_ref
    import test_sharded_adam
    return [adam_ref.hyper(ADAM_LR, weight_decay=wd, decoupled=dec, step=step)
            for wd, dec in test_sharded_adam.ROWS]


@functools.lru_cache(maxsize=2)
def adam_sweep(np_, step):
    """bf16: p, g, m and v swept in turn. Setting 0 of the v sweep is
    (p, g, m) = (1, 0, 1): every value through b2*v, the sqrt, the / s2, the
    + eps and the final divide; of the g sweep (p, m, v) = (1, 0, 0)."""
    import adam_ref
    dt = "bf16"
    one = special(dt, "one")

    def ref(x, h):
        p, m, v = adam_ref.step(x["p"], x["g"], x["m"], x["v"], dt, h, np_)
        return {"p": p, "m": m, "v": v, "g": x["g"]}
    return _update_sweep("adam", "adam", dt, adam_hypers(step), ("p", "g", "m", "v"),
                         ("p", "g", "m", "v"), _env16(dt, {"v": {"m": one}}), ref,
                         np=np_, step=step)


# fp32 (master, m, v) of the master-weight update's three settings
MASTER_TRIPLES = ((1.0, 0.0, 0.0), (1.0 / 3.0, -1.0, 1.0 + 2.0 ** -23), (-30000.25, 1e-8, 1e30))


@functools.lru_cache(maxsize=2)
def master_sweep(dt, np_, step):
    """g swept against three fp32 (master, m, v) triples. The long segments
    are one per triple; tail segment j has triple j % 3."""
    import adam_master_ref
    hypers = adam_hypers(step)
    block_segs, nedge = _update_layout("master", 3, 1)
    block = Layout("master", block_segs)
    g = np.empty(block.total, np.uint16)
    trip = np.empty(block.total, np.int64)
    for c in range(3):
        sl = block.seg(c)
        g[sl] = patterns()[np.arange(sl.stop - sl.start) % NPAT]
        trip[sl] = c
    a = int(block.start[3])
    g[a:] = patterns()[np.arange(block.total - a) % NPAT]
    trip[a:] = np.repeat(np.arange(nedge), block.n[3:]) % 3
    t32 = np.array(MASTER_TRIPLES, np.float32)
    w, m, v = (t32[trip, j] for j in range(3))
    lay = Layout("master", block_segs * len(hypers))
    want = {"p16": [], "w": [], "m": [], "v": []}
    for h in hypers:
        p16, w2, m2, v2 = adam_master_ref.step(w, store(dt, g), m, v, dt, h, np_)
        for k, x in zip(("p16", "w", "m", "v"), (bits_of(p16), w2, m2, v2)):
            want[k].append(x)
    want = {k: np.concatenate(x) for k, x in want.items()}
    want["g"] = np.tile(g, len(hypers))
    inputs = {"g": np.tile(g, len(hypers)), "w": np.tile(w, len(hypers)),
              "m": np.tile(m, len(hypers)), "v": np.tile(v, len(hypers))}
    sw = UpdateSweep("master", dt, lay, inputs, want, [("g", np.ones(lay.total, bool))],
                     np=np_, step=step)
    sw.hypers = hypers
    sw.hyper_of_seg = np.repeat(np.arange(len(hypers)), len(block_segs))
    return sw
