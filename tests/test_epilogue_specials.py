"""The reference and the inputs of tests/test_epilogue_specials_gpu.py,
checked on the CPU (no device).

The oracle's /np average, SMA blend and bf16 two-input ops are compared, over
the special-value pools and fills of tests/epilogue_specials.py, with a second
statement of the same arithmetic in numpy. And the coverage the GPU test
relies on is asserted on the inputs themselves: every region of a launch
(scalar head, full tile, ragged tile, scalar tail) is reached, and every one
of them holds an element whose sum is exactly -0.
"""
import numpy as np
import pytest

import epilogue_specials as es

DTS = es.DTS
NPS = (1, 2, 3, 4, 8)
# output placements of the GPU test, as the output pointer's residue in
# elements past a 16-byte boundary
OUT_OFFSETS = (0, 1)


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    oracle.build()
    return oracle


# ---- the pools -------------------------------------------------------------

@pytest.mark.parametrize("dt", ["f32", "f64", "f16"])
def test_pool_is_what_it_says(dt):
    """The pools are built from bit fields; numpy's finfo states the same
    values independently."""
    p = es.pool(dt)
    fi = np.finfo(es.NP[dt])
    sub = fi.smallest_subnormal
    want = []
    for mag in (0.0, sub, 3 * sub, fi.tiny - sub, fi.tiny, 1.0, fi.max, fi.max / 2, np.inf):
        want += [-mag, mag]
    want = np.array(want, dtype=es.NP[dt])
    assert np.array_equal(es.bits(p[:-1]), es.bits(want))
    assert np.isnan(p[-1]) and p.size == 19
    # 3x the smallest subnormal and the smallest subnormal are ties when halved
    assert float(p[5]) / 2 == 1.5 * float(sub) and float(p[3]) / 2 == 0.5 * float(sub)


def test_bf16_pool_is_the_f32_pool_truncated(orc):
    """Every bf16 special is the top half of an fp32 pattern of the same
    class: widened it is (-)0, subnormal, smallest normal, 1, finite, inf, NaN."""
    p = es.pool("bf16")
    f = orc.bf16_bits_to_f32(p)
    tiny = np.finfo(np.float32).tiny
    want = [0.0, 2.0 ** -133, 3 * 2.0 ** -133, tiny - 2.0 ** -133, tiny, 1.0,
            float(np.float32(2.0 ** 127) * np.float32(2 - 2.0 ** -7)),
            float(np.float32(2.0 ** 126) * np.float32(2 - 2.0 ** -7)), np.inf]
    for i, mag in enumerate(want):
        assert f[2 * i] == -mag and f[2 * i + 1] == mag, (i, f[2 * i], mag)
        assert np.signbit(f[2 * i]) and not np.signbit(f[2 * i + 1])
    assert np.isnan(f[-1]) and p[-1] == 0x7FC0
    assert np.array_equal(orc.f32_to_bf16_bits(f[:-1]), p[:-1])  # exact both ways


# ---- the fills: what the GPU test relies on ---------------------------------

def _sum_is_neg_zero(dt, n, k):
    """Elements at which all k inputs are -0: the only way a sum is -0."""
    z = np.ones(n, dtype=bool)
    for j in range(k):
        z &= es.is_neg_zero(dt, es.fill(dt, n, j))
    return z


@pytest.mark.parametrize("dt", DTS)
def test_fill_reaches_every_region(dt):
    isz = es.itemsize(dt)
    E = 16 // isz
    shapes = es.shapes(dt)
    assert shapes == (1, E - 1, E + 1, 1024 * E, 1024 * E + 300 * E + E - 1)
    seen = {"head": 0, "full": 0, "ragged": 0, "tail": 0}
    for n in shapes:
        for off in OUT_OFFSETS:
            for tile in (es.TILE_VECS, es.TILE_VECS_BATCH_K1):
                reg = es.regions(off * isz, n, isz, tile)
                # a partition of [0, n), in order
                assert np.array_equal(np.concatenate(list(reg.values())), np.arange(n))
                # what the shape allows
                head = min(n, (E - off) % E)
                nvec = (n - head) // E
                assert reg["head"].size == head
                assert reg["full"].size == (nvec // tile) * tile * E
                assert reg["ragged"].size == (nvec % tile) * E
                assert reg["tail"].size == n - head - nvec * E
                for k in (1, 2):
                    nz = _sum_is_neg_zero(dt, n, k)
                    for name, idx in reg.items():
                        if idx.size:
                            seen[name] += 1
                            assert nz[idx].any(), (dt, n, off, tile, k, name)
    assert all(seen.values()), seen
    # the largest shape has a full tile, a ragged tile and a tail of E - 1
    # when aligned; one element past alignment the head takes those E - 1
    for tile in (es.TILE_VECS, es.TILE_VECS_BATCH_K1):
        sizes = {k: v.size for k, v in es.regions(0, shapes[-1], isz, tile).items()}
        assert sizes["head"] == 0 and sizes["tail"] == E - 1, sizes
        assert sizes["full"] and sizes["ragged"] == (1324 % tile) * E, sizes
        sizes = {k: v.size for k, v in es.regions(isz, shapes[-1], isz, tile).items()}
        assert sizes["head"] == E - 1 and sizes["tail"] == 0, sizes
        assert sizes["full"] and sizes["ragged"] == (1324 % tile) * E, sizes
    # and a tail behind a head: a vector and one, one element past alignment
    sizes = {k: v.size for k, v in es.regions(isz, E + 1, isz).items()}
    if E > 2:
        assert sizes == {"head": E - 1, "full": 0, "ragged": 0, "tail": 2}, sizes
    else:  # fp64: the two elements after the head are one vector
        assert sizes == {"head": 1, "full": 0, "ragged": 2, "tail": 0}, sizes


@pytest.mark.parametrize("dt", DTS)
def test_fill_has_every_ordered_pair_and_ordinary_values(dt):
    n = es.shapes(dt)[-1]
    L = es.pool(dt).size
    pb = [int(b) for b in es.bits(es.pool(dt))]
    for j0, j1 in ((0, 1), (1, 2), (0, 2), (1, 0)):
        x, y = es.bits(es.fill(dt, n, j0)), es.bits(es.fill(dt, n, j1))
        got = set(zip(x[::4].tolist(), y[::4].tolist()))
        assert {(a, b) for a in pb for b in pb} <= got, (dt, j0, j1)
    x = es.fill(dt, n, 0)
    odd = x[1:n - es.BACK:2]
    f = odd.astype(np.float64) if dt != "bf16" else None
    if f is not None:
        assert np.isfinite(f).all() and 0.5 < f.std() < 1.5  # standard normal
    assert len(set(es.bits(odd).tolist())) > odd.size // 4
    # the same value in every input at m % 4 == 2
    assert np.array_equal(es.bits(es.fill(dt, n, 0))[2::4], es.bits(es.fill(dt, n, 5))[2::4])
    assert L == 19


@pytest.mark.parametrize("dt", DTS)
def test_sma_batch_layout_meets_every_shape_and_placement(dt):
    lay = es.sma_batch_layout(dt)
    assert len(lay) == 20 > 16  # two launches
    assert {(n, p[0]) for n, p in lay} >= {(n, p[0]) for n in es.shapes(dt)
                                           for p in es.SMA_PLACEMENTS}
    assert {p[1] for p in es.SMA_PLACEMENTS} == set(OUT_OFFSETS)  # v is the output
    assert any(v != s for _, v, s in es.SMA_PLACEMENTS)


def test_mismatches_tolerates_only_nan_payloads():
    for dt in DTS:
        p = es.pool(dt)
        assert es.same(dt, p, p.copy())
        q = p.copy()
        q[-1] = p[-1] if dt != "bf16" else 0xFFC0  # another NaN
        if dt != "bf16":
            es.bits(q)[-1] |= 1
        assert es.same(dt, p, q)
        for i in (0, 1, 16, 17):  # -0 / +0, -inf / +inf: sign matters
            q = p.copy()
            q[i] = p[i ^ 1]
            assert not es.same(dt, p, q) and list(es.mismatches(dt, p, q)) == [i]
        q = p.copy()
        q[-1] = p[5]  # NaN against a number
        assert not es.same(dt, p, q)


# ---- the oracle against numpy ------------------------------------------------

def _np_avg(orc, xs, dt, np_):
    with np.errstate(all="ignore"):
        if dt in ("f32", "f64"):
            s = xs[0].copy()
            for x in xs[1:]:
                s = s + x
            return s / es.NP[dt](np_)
        if dt == "f16":
            s = xs[0].copy()
            for x in xs[1:]:
                s = (s.astype(np.float32) + x.astype(np.float32)).astype(np.float16)
            return (s.astype(np.float32) / np.float32(np_)).astype(np.float16)
        acc = orc.bf16_bits_to_f32(xs[0])
        for x in xs[1:]:
            acc = acc + orc.bf16_bits_to_f32(x)
        return orc.f32_to_bf16_bits(acc / np.float32(np_))


def _np_sma(orc, v, s, dt, np_, alpha):
    with np.errstate(all="ignore"):
        if dt == "f64":
            return (1.0 - alpha) * v + alpha * (s / np.float64(np_))
        c1, c2, d = np.float32(1.0 - alpha), np.float32(alpha), np.float32(np_)
        if dt == "f32":
            return c1 * v + c2 * (s / d)
        if dt == "f16":
            r = c1 * v.astype(np.float32) + c2 * (s.astype(np.float32) / d)
            return r.astype(np.float16)
        r = c1 * orc.bf16_bits_to_f32(v) + c2 * (orc.bf16_bits_to_f32(s) / d)
        return orc.f32_to_bf16_bits(r)


@pytest.mark.parametrize("dt", DTS)
def test_oracle_reduce_avg_vs_numpy(orc, dt):
    for n in es.shapes(dt)[2:]:
        for k in (1, 2, 3):
            xs = [es.fill(dt, n, j) for j in range(k)]
            for np_ in NPS:
                want = _np_avg(orc, xs, dt, np_)
                got = orc.reduce_avg(xs, dt, np_)
                assert es.same(dt, got, want), (n, k, np_, es.describe(dt, got, want))
                # -0 survives every divisor: where all inputs are -0
                nz = _sum_is_neg_zero(dt, n, k)
                assert nz.any() and es.is_neg_zero(dt, got)[nz].all(), (n, k, np_)
    # every ordered pair of the pool, explicitly
    p = es.pool(dt)
    x, y = np.repeat(p, p.size), np.tile(p, p.size)
    for np_ in NPS:
        got = orc.reduce_avg([x, y], dt, np_)
        assert es.same(dt, got, _np_avg(orc, [x, y], dt, np_)), np_


@pytest.mark.parametrize("dt", DTS)
def test_oracle_sma_blend_vs_numpy(orc, dt):
    p = es.pool(dt)
    cases = [(es.fill(dt, n, 0), es.fill(dt, n, 1)) for n in es.shapes(dt)[2:]]
    cases.append((np.repeat(p, p.size), np.tile(p, p.size)))
    for v, s in cases:
        for np_, alpha in ((2, 0.1), (3, 0.25), (8, 0.1)):
            got = orc.sma_blend(v, s, dt, np_, alpha)
            want = _np_sma(orc, v, s, dt, np_, alpha)
            assert es.same(dt, got, want), (np_, alpha, es.describe(dt, got, want))


@pytest.mark.parametrize("op", ["sum", "min", "max", "prod"])
def test_oracle_bf16_two_input_vs_numpy(orc, op):
    p = es.pool("bf16")
    x, y = np.repeat(p, p.size), np.tile(p, p.size)
    a, b = orc.bf16_bits_to_f32(x), orc.bf16_bits_to_f32(y)
    with np.errstate(all="ignore"):
        if op == "sum":
            want = orc.f32_to_bf16_bits(a + b)
        elif op == "prod":
            want = orc.f32_to_bf16_bits(a * b)
        elif op == "min":
            want = np.where(b < a, y, x)  # (b < a) ? b : a, the input's bits
        else:
            want = np.where(a < b, y, x)  # (a < b) ? b : a
    got = orc.transform2(x, y, "bf16", op)
    assert es.same("bf16", got, want), es.describe("bf16", got, want)
    if op in ("min", "max"):
        assert np.array_equal(got, want)  # bits of an input, NaNs too
        assert ((got == x) | (got == y)).all()
