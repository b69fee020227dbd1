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

The update kernels: SGD, Adam (bf16) and master-weight Adam; their gated
twins at an unscale of 2^-16 and a clip of 0.37, one call per decay mode (the
gated entries take one hyper); the stochastic-rounding update and its gated
twin, every segment with an element base and a stream word of its own; LAMB's
master moments pass; and the narrowing of LAMB's master apply pass on the
grid of fp32 values around every 16-bit rounding boundary.
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
    sr, lamb = _src("kf_adam_sr.hip"), _src("kf_lamb.hip")
    # the gated kernels are launched by their parents' planner call, on its
    # grid and with its block: the "adam" and "master" geometry is theirs
    assert adam.count("plan_update_batch<") == 1 and master.count("plan_update_batch<") == 1
    assert "adam_update_gated_kernel<T><<<dim3(gx, gy), kAdamBlock, 0, s>>>" in adam
    assert "adam_update_kernel<T><<<dim3(gx, gy), kAdamBlock, 0, s>>>" in adam
    assert re.search(r"adam_master_gated_kernel<T>\s*<<<dim3\(gx, gy\), kAdamMasterBlock, 0, s>>>",
                     master)
    assert "adam_master_kernel<T><<<dim3(gx, gy), kAdamMasterBlock, 0, s>>>" in master
    assert adam.count("adam_body<T, decltype(DIV)::value, decltype(DECAY)::value>") == 2
    assert "plan_update_batch<" not in _src("kf_step_gate.hip")
    # so is the stochastic-rounding kernel's gated twin
    assert sr.count("plan_update_batch<") == 1 and \
        sr.count("<<<dim3(gx, gy), kAdamSrBlock, 0, s>>>") == 2
    assert "constexpr int kAdamSrUnroll = KF_ADAM_SR_UNROLL;" in sr
    # the LAMB master moments pass: 16-byte units of the fp32 compute type
    assert "counts, nb, SgdVec<C>::N, static_cast<size_t>(kLambBlock) * kLambUnroll," in lamb
    assert "return launch_moments<float, kLambMasterSeg>(masters, grads16," in lamb
    return {
        "adam_sr": (_int(sr, r"constexpr int kAdamSrElts\s*=\s*(\d+);"),
                    _int(sr, r"constexpr int kAdamSrBlock\s*=\s*(\d+);")
                    * _int(sr, r"#define KF_ADAM_SR_UNROLL (\d+)"),
                    _int(sr, r"constexpr int kAdamSrSeg\s*=\s*(\d+);")),
        "lamb_master": (16 // 4, _int(lamb, r"constexpr int kLambBlock\s*=\s*(\d+);")
                        * _int(lamb, r"constexpr int kLambUnroll\s*=\s*(\d+);"),
                        _int(lamb, r"constexpr int kLambMasterSeg\s*=\s*(\d+);")),
        # the apply pass's pieces: 16-byte units of fp32, one piece per table row
        "lamb_apply": (16 // 4, _int(lamb, r"constexpr int kLambBlock\s*=\s*(\d+);")
                       * _int(lamb, r"#define KF_LAMB_APPLY_UNROLL (\d+)")
                       * _int(lamb, r"#define KF_LAMB_APPLY_TILES (\d+)"), None),
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




def _master_block(kernel):
    """One hyper row's block of a gradient sweep against the fp32 triples:
    (segments, their Layout, g, (w, m, v)). The long segments are one per
    triple; tail segment j has triple j % 3."""
    block_segs, nedge = _update_layout(kernel, 3, 1)
    block = Layout(kernel, block_segs)
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
    return block_segs, block, g, tuple(t32[trip, j] for j in range(3))


def _master_sweep(name, kernel, dt, hypers, ref, **params):
    """g swept against the triples, one block per hyper row.
    ref(w, g, m, v, hyper) -> {role: array} over one block."""
    block_segs, block, g, (w, m, v) = _master_block(kernel)
    lay = Layout(kernel, block_segs * len(hypers))
    want = {}
    for h in hypers:
        for k, x in ref(w, g, m, v, h).items():
            want.setdefault(k, []).append(x)
    want = {k: np.concatenate(x) for k, x in want.items()}
    want["g"] = np.tile(g, len(hypers))
    inputs = {"g": np.tile(g, len(hypers)), "w": np.tile(w, len(hypers)),
              "m": np.tile(m, len(hypers)), "v": np.tile(v, len(hypers))}
    sw = UpdateSweep(name, dt, lay, inputs, want, [("g", np.ones(lay.total, bool))], **params)
    sw.hypers = hypers
    sw.hyper_of_seg = np.repeat(np.arange(len(hypers)), len(block_segs))
    return sw


@functools.lru_cache(maxsize=2)
def master_sweep(dt, np_, step):
    """g swept against three fp32 (master, m, v) triples. The long segments
    are one per triple; tail segment j has triple j % 3."""
    import adam_master_ref

    def ref(w, g, m, v, h):
        p16, w2, m2, v2 = adam_master_ref.step(w, store(dt, g), m, v, dt, h, np_)
        return {"p16": bits_of(p16), "w": w2, "m": m2, "v": v2}
    return _master_sweep("master", "master", dt, adam_hypers(step), ref, np=np_, step=step)


# ---- i, j. the gated updates ----------------------------------------------------------

# an unscale (every bf16 subnormal gradient times 2^-16 is an fp32 subnormal
# on the master and stochastic-rounding paths, and below half the smallest
# bf16 subnormal on the plain bf16 path), and a clip
GATED_MULS = (2.0 ** -16, 0.37)
NROWS = 3  # tests/test_sharded_adam.py's ROWS: the three decay modes


def gate_of(mul, skip=0):
    """A gate as a verdict leaves it, with grad_mul = mul."""
    import step_gate_ref
    g = step_gate_ref.new_gate()
    g["skip"], g["grad_mul"] = skip, np.float32(mul)
    return g


def _gated(s, h, mul):
    """The gate and the step state of a gated sweep: the state adam_ref's own
    scalars for h["step"] correspond to."""
    import step_gate_ref
    s.gate, s.state = gate_of(mul), step_gate_ref.scalars_of(h)
    return s


@functools.lru_cache(maxsize=NROWS)
def gated_adam_sweep(np_, step, mul, row):
    """adam_sweep's layout and settings for one row of ROWS (the gated entry
    takes one hyper for all segments), bf16."""
    import step_gate_ref
    dt = "bf16"
    h = adam_hypers(step)[row]
    gate, state = gate_of(mul), step_gate_ref.scalars_of(h)

    def ref(x, h):
        p, m, v = step_gate_ref.update(x["p"], x["g"], x["m"], x["v"], dt, h, gate, state, np_)
        return {"p": p, "m": m, "v": v, "g": x["g"]}
    s = _update_sweep("adam_gated", "adam", dt, [h], ("p", "g", "m", "v"), ("p", "g", "m", "v"),
                      _env16(dt, {"v": {"m": special(dt, "one")}}), ref,
                      np=np_, step=step, mul=mul, row=row)
    return _gated(s, h, mul)


@functools.lru_cache(maxsize=NROWS)
def gated_master_sweep(dt, np_, step, mul, row):
    """master_sweep's layout for one row of ROWS."""
    import step_gate_ref
    h = adam_hypers(step)[row]
    gate, state = gate_of(mul), step_gate_ref.scalars_of(h)

    def ref(w, g, m, v, h):
        p16, w2, m2, v2 = step_gate_ref.update_master(w, store(dt, g), m, v, dt, h, gate, state, np_)
        return {"p16": bits_of(p16), "w": w2, "m": m2, "v": v2}
    s = _master_sweep("master_gated", "master", dt, [h], ref, np=np_, step=step, mul=mul, row=row)
    return _gated(s, h, mul)


def subnormal_products(dt, g, mul, np_=0):
    """Which gradients (bit patterns) give a non-zero fp32-subnormal
    g / np * mul on the paths that compute in fp32 without narrowing."""
    with np.errstate(under="ignore", invalid="ignore", over="ignore"):
        x = widen(dt, g)
        if np_:
            x = x * np.float32(1.0 / np_) if np_ & (np_ - 1) == 0 else x / np.float32(np_)
        x = np.abs(x * np.float32(mul))
    return (x > 0) & (x < np.finfo(np.float32).tiny)


# ---- k. the stochastic-rounding update ----------------------------------------------------

SR_KEY = 0x9ABCDEF1
SR_STRADDLES = 1  # the segment (a long one) that holds element 2^32


def sr_tables(lay):
    """(bases, stream words) of a layout's segments: a base (a multiple of 8)
    and a stream word of its own for every segment; segment SR_STRADDLES
    crosses element 2^32 and the last segment (a tail alone) holds the last
    elements below 2^33."""
    nseg = len(lay.n)
    bases = 8 * (1000 * np.arange(nseg, dtype=np.int64) + 3)
    assert bases[-1] + lay.n.max() < 1 << 32
    bases[SR_STRADDLES] = (1 << 32) - 8 * 1001
    bases[-1] = (1 << 33) - 8
    streams = (0x01234567 * (np.arange(nseg, dtype=np.int64) + 1)) & 0xFFFFFFFF
    return bases, streams


def sr_narrow(lay, pw, mw, vw, bases, streams, key):
    """adam_sr_ref's narrowing of fp32 (p', m', v') over a whole layout at
    once: element i of segment s has index bases[s] + i and stream word
    streams[s]. tests/test_sweep16.py pins it to adam_sr_ref.step segment by
    segment."""
    import adam_sr_ref
    e = (np.repeat(bases - lay.start, lay.n) + np.arange(lay.total)).astype(np.uint64)
    a, b = adam_sr_ref.philox2x32_10(e >> np.uint64(1), np.repeat(streams, lay.n), key)
    w = np.where((e & np.uint64(1)) != 0, b, a).astype(np.uint32)
    return (adam_sr_ref.sr(pw, w >> np.uint32(16)), f32_to_bf16_bits(mw),
            adam_sr_ref.sr(vw, w & np.uint32(0xFFFF)))


def _sr_sweep(name, hypers, wide, **params):
    """adam_sweep's layout; wide(x, h) -> fp32 (p', m', v') of one row's
    block. s.wide keeps them beside the narrowed s.want."""
    dt = "bf16"

    def ref(x, h):
        pw, mw, vw = wide({r: bf16_bits_to_f32(x[r]) for r in ("p", "g", "m", "v")}, h)
        return {"p": pw, "m": mw, "v": vw}
    s = _update_sweep(name, "adam_sr", dt, hypers, ("p", "g", "m", "v"), ("p", "g", "m", "v"),
                      _env16(dt, {"v": {"m": special(dt, "one")}}), ref, **params)
    s.bases, s.streams = sr_tables(s.layout)
    s.wide = s.want
    p, m, v = sr_narrow(s.layout, s.wide["p"], s.wide["m"], s.wide["v"], s.bases, s.streams, SR_KEY)
    s.want = {"p": p, "m": m, "v": v, "g": s.inputs["g"]}
    for a in s.want.values():
        a.setflags(write=False)
    return s


@functools.lru_cache(maxsize=2)
def sr_sweep(np_, step):
    """p, g, m and v swept in turn through widen, the fp32 update, sr(p'),
    rne(m'), sr(v'); the three rows of ROWS in one call."""
    import adam_ref
    return _sr_sweep("adam_sr", adam_hypers(step),
                     lambda x, h: adam_ref.step(x["p"], x["g"], x["m"], x["v"], "f32", h, np_),
                     np=np_, step=step)


@functools.lru_cache(maxsize=NROWS)
def sr_gated_sweep(np_, step, mul, row):
    import step_gate_ref
    h = adam_hypers(step)[row]
    gate, state = gate_of(mul), step_gate_ref.scalars_of(h)
    s = _sr_sweep("adam_sr_gated", [h],
                  lambda x, h: step_gate_ref.update(x["p"], x["g"], x["m"], x["v"], "f32", h, gate,
                                                    state, np_),
                  np=np_, step=step, mul=mul, row=row)
    return _gated(s, h, mul)


# ---- l. LAMB's master moments pass --------------------------------------------------------

LAMB_NPS = (0, 3)
LAMB_WDS = (0.0, 1e-2)


def lamb_hypers(wd):
    """A first and a later step."""
    import lamb_ref
    return [lamb_ref.hyper(ADAM_LR, eps=1e-6, weight_decay=wd, step=t) for t in ADAM_STEPS]


@functools.lru_cache(maxsize=2)
def lamb_master_sweep(dt, np_, wd):
    """g swept against MASTER_TRIPLES as (master, m, v): m, v and u are
    written, the master and g only read."""
    import lamb_ref

    def ref(w, g, m, v, h):
        m2, v2, u = lamb_ref.moments(w, lamb_ref.widen16(g, dt), m, v, "f32", h, np_)
        return {"m": m2, "v": v2, "u": u}
    return _master_sweep("lamb_master", "lamb_master", dt, lamb_hypers(wd), ref, np=np_, wd=wd)


# ---- m. LAMB's master apply pass: the narrowing ---------------------------------------------

def narrowing_grid(dt):
    """fp32 masters around every rounding boundary of dt: for every positive
    finite 16-bit value, the exact tie between it and the next one (both
    parities of the last kept bit; above the largest finite value the tie
    narrows to inf: 65520 for f16), and one fp32 ulp either side of the tie;
    all of that negated; fp32 subnormals, values that narrow to 16-bit
    subnormals (in the ties already), +-0, +-inf, NaN, the fp32 extremes."""
    elts = kernels()["master"][0]
    top = special(dt, "max")
    lo = widen(dt, np.arange(0, top + 1, dtype=np.uint16)).astype(np.float64)
    hi = np.empty_like(lo)
    hi[:-1] = lo[1:]
    hi[-1] = 2.0 ** 128 if dt == "bf16" else 65536.0
    tie = ((lo + hi) / 2).astype(np.float32)
    assert np.array_equal(tie.astype(np.float64), (lo + hi) / 2)  # exact in fp32
    below = np.nextafter(tie, np.float32(0))
    above = np.nextafter(tie, np.float32(np.inf))
    extra = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, np.finfo(np.float32).max,
                      np.finfo(np.float32).smallest_subnormal, 2.0 ** -127, 2.0 ** -140,
                      65504.0, 65519.996, 65520.0, 65520.004, 2.0 ** -24, 2.0 ** -25,
                      2.0 ** -25 + 2.0 ** -48, 6.0e-8, 1.0, 1.0 + 2.0 ** -8, 1.0 + 2.0 ** -11],
                     np.float32)
    pos = np.concatenate([tie, below, above, lo.astype(np.float32), extra])
    grid = np.concatenate([pos, -pos])
    return grid[:grid.size - (grid.size % elts) + 3 - elts]  # a 3-element scalar tail


APPLY_HEAD, APPLY_UNIT, APPLY_TAIL = 0, 1, 2
APPLY_NLR = -0.01  # with u = 0: p + (nlr * 0) = p + (-0) = p, -0 included


def apply_regions(offset, n):
    """(head, unit, tail) element counts of a master-path piece of n elements
    that starts `offset` elements past a 16-byte boundary in all three of its
    arrays (kf_lamb_apply_create, apply_body): the head runs to the first
    index at which the fp32 arrays and the 16-bit one are all 16-byte aligned."""
    unit = kernels()["lamb_apply"][0]
    head = min(n, (-offset) % EPV)
    assert (offset + head) % unit == 0 or head == n
    units = (n - head) // unit
    return head, units * unit, n - head - units * unit


class ApplyCase:
    """The narrowing grid through the three paths of the master apply pass,
    in one flat buffer per array (element i of all three arrays is the same
    element; every buffer starts 16-byte aligned):

      long   one piece at offset 0: the grid's last three values, then the
             grid: every value in a 16-byte unit, a scalar tail after them
      heads  pieces of 7 at element 1 of rows of 16 elements: head = 7
      tails  pieces of 3 at element 0 of rows of 8: no unit, a tail of 3

    p: the fp32 image (bit patterns; GUARD_F32 outside the pieces), used: the
    pieces' elements, label: their region, pieces: [(start, n)]."""

    def __init__(self, dt):
        self.dt = dt
        grid = np.ascontiguousarray(narrowing_grid(dt)).view(np.uint32)
        self.grid = grid
        wrap = lambda k: np.concatenate([grid, grid[:(-grid.size) % k]]).reshape(-1, k)  # noqa: E731
        long = np.concatenate([grid[-3:], grid])
        heads, tails = wrap(7), wrap(3)
        self.long = (2 * EPV, long.size)
        b0 = -(-(self.long[0] + long.size + EPV) // 16) * 16
        self.heads = (b0, heads.shape[0])              # rows of 16 from b0, the piece at [1, 8)
        c0 = b0 + 16 * heads.shape[0]
        self.tails = (c0, tails.shape[0])              # rows of 8 from c0, the piece at [0, 3)
        self.size = c0 + 8 * tails.shape[0] + EPV
        self.p = np.full(self.size, GUARD_F32, np.uint32)
        self.label = np.full(self.size, -1, np.int8)
        self.pieces = [self.long]
        self.p[self.long[0]:self.long[0] + long.size] = long
        h, u, t = apply_regions(0, long.size)
        self.label[self.long[0]:self.long[0] + long.size] = np.repeat(
            [APPLY_HEAD, APPLY_UNIT, APPLY_TAIL], [h, u, t])
        for (start, rows), data, off in ((self.heads, heads, 1), (self.tails, tails, 0)):
            k = data.shape[1]
            stride = 16 if off else 8
            idx = start + off + stride * np.arange(rows)[:, None] + np.arange(k)[None, :]
            self.p[idx] = data
            h, u, t = apply_regions(off, k)
            self.label[idx] = np.repeat([APPLY_HEAD, APPLY_UNIT, APPLY_TAIL], [h, u, t])[None, :]
            self.pieces += [(int(s), k) for s in idx[:, 0]]
        self.used = self.label >= 0
        import lamb_ref
        self.u = np.where(self.used, np.uint32(0), np.uint32(GUARD_F32))
        self.want16 = np.where(self.used, lamb_ref.narrow16(self.p.view(np.float32), dt),
                               np.uint16(GUARD))
        for a in (self.p, self.u, self.want16, self.label, self.used):
            a.setflags(write=False)


@functools.lru_cache(maxsize=None)
def apply_case(dt):
    return ApplyCase(dt)
