"""IEEE specials through the fused epilogues on the GPU: the /np average
(kf_bucket_reduce_avg, kf_bucket_div, kf_bucket_reduce_peers and
kf_bucket_reduce_batch with np) and the SMA blend (kf_sma_blend,
kf_sma_blend_batch), and every ordered pair of bf16 specials through the
plain bf16 ops. Signed zeros, subnormals and their ties, the largest finite
value, infinities and a NaN reach the scalar head, a full tile, the ragged
tile and the scalar tail of every launch (tests/epilogue_specials.py; the
inputs and the oracle are checked on the CPU in
tests/test_epilogue_specials.py). Bit-exact against the oracle; NaNs by
position.

Every launch writes into a buffer pre-filled with a guard byte, and the bytes
before and after the output must come back unchanged.

Before Elt<f16_t>::div narrowed its product through f32_product_to_f16
(kf_reduce_kernels.hpp), the fp16 average failed here for every power-of-two
np (1, 2, 4, 8), single launch and batch, in head and tail elements only: a
sum of -0 averaged to +0 (0x0000 for 0x8000). Nothing else failed.

Pointers whose 16-byte residues differ ("mixed") stay on the vector path
with unaligned loads, for the reduce and for the SMA blend alike; the
element-at-a-time bodies (reduce_kernel_unaligned, the blend's vec_ok = 0)
are reached only with KUNGFU_AMD_NO_UNALIGNED_VECTOR=1, which no test sets.
"""
import ctypes

import numpy as np
import pytest

import epilogue_specials as es

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

DTS = es.DTS
NPS = (1, 2, 3, 4, 8)
GUARD = 0xA5
PAD = 32  # guard bytes on either side of an array (two 16-byte vectors)


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


@pytest.fixture(scope="module")
def ref(orc):
    """The oracle's results, computed once per argument set and shared
    read-only among the cases."""
    cache = {}

    def get(kind, dt, n, js, *args):
        key = (kind, dt, n, tuple(js)) + args
        if key not in cache:
            xs = [es.fill(dt, n, j) for j in js]
            if kind == "avg":
                r = orc.reduce_avg(xs, dt, *args)
            elif kind == "sma":
                r = orc.sma_blend(xs[0], xs[1], dt, *args)
            else:
                raise KeyError(kind)
            r.setflags(write=False)
            cache[key] = r
        return cache[key]
    return get


class Arena:
    """Arrays laid out in ONE device buffer, each at a chosen element offset
    past a 16-byte boundary with PAD guard bytes on either side: one upload,
    one download, and the guards checked after the launches."""

    def __init__(self, dev):
        self.dev = dev
        self.slots = []  # (byte offset, nbytes)
        self.parts = []
        self.size = 0

    def add(self, arr, off_elems, dt):
        """A copy of arr (or, for an int, that many guard-filled elements)."""
        isz = es.itemsize(dt)
        assert 0 <= off_elems * isz < 16
        if isinstance(arr, int):
            data = np.full(arr * isz, GUARD, np.uint8)
        else:
            data = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
        start = self.size + PAD + off_elems * isz
        end = start + data.size
        total = -(-(end + PAD) // 16) * 16
        blob = np.full(total - self.size, GUARD, np.uint8)
        blob[start - self.size:end - self.size] = data
        self.parts.append(blob)
        self.slots.append((start, data.size))
        self.size = total
        return len(self.slots) - 1

    def upload(self):
        self.host = np.concatenate(self.parts)
        self.t = torch.from_numpy(self.host.copy()).to(self.dev)
        assert self.t.data_ptr() % 16 == 0
        return self

    def ptr(self, i):
        return self.t.data_ptr() + self.slots[i][0]

    def download(self):
        torch.cuda.synchronize()
        self.back = self.t.cpu().numpy()
        return self

    def get(self, i, dt):
        start, nbytes = self.slots[i]
        return self.back[start:start + nbytes].view(es.NP[dt])

    def guards_intact(self):
        """Every byte outside the arrays still holds the guard value."""
        mask = np.ones(self.size, dtype=bool)
        for start, nbytes in self.slots:
            mask[start:start + nbytes] = False
        return bool((self.back[mask] == GUARD).all())

    def inputs_intact(self, idx):
        return all(np.array_equal(self.back[s:s + n], self.host[s:s + n])
                   for s, n in (self.slots[i] for i in idx))


def stream():
    return torch.cuda.current_stream().cuda_stream


def placements(dt):
    """(name, output offset, offset of input j), in elements past a 16-byte
    boundary: all aligned; all one element past alignment (a head of E - 1);
    the output one past and the inputs at other residues (unaligned 16-byte
    loads in the vector body)."""
    E = 16 // es.itemsize(dt)
    return (("aligned", 0, lambda j: 0),
            ("co1", 1, lambda j: 1),
            ("mixed", 1, lambda j: (2 + j) % E))


def check(fails, tag, dt, got, want, reg):
    if not es.same(dt, got, want):
        fails.append((tag, es.describe(dt, got, want, reg)))


# ---- the /np average, one launch per bucket ----------------------------------

@pytest.mark.parametrize("np_", NPS)
@pytest.mark.parametrize("dt", DTS)
def test_avg_single_launch(lib, ref, dev, dt, np_):
    from kungfu_amd import _lib
    from oracle.oracle import DT
    isz = es.itemsize(dt)
    fails = []
    for n in es.shapes(dt):
        for pname, ooff, ioff in placements(dt):
            a = Arena(dev)
            ins = [a.add(es.fill(dt, n, j), ioff(j), dt) for j in range(3)]
            calls = [("avg_k%d" % k, k) for k in (1, 2, 3)] + [("peers_k%d" % k, k) for k in (2, 3)]
            outs = [a.add(n, ooff, dt) for _ in calls]
            inplace = a.add(es.fill(dt, n, 0), ooff, dt) if pname != "mixed" else None
            a.upload()
            for (name, k), o in zip(calls, outs):
                ptrs = _lib.ptr_array([a.ptr(i) for i in ins[:k]])
                if name.startswith("avg"):
                    rc = lib.kf_bucket_reduce_avg(ptrs, k, a.ptr(o), n, DT[dt], np_, stream())
                else:
                    rc = lib.kf_bucket_reduce_peers(ptrs, k, a.ptr(o), n, DT[dt], 0, np_, stream())
                assert rc == 0, (name, lib.kf_last_error())
            if inplace is not None:
                assert lib.kf_bucket_div(a.ptr(inplace), n, DT[dt], np_, stream()) == 0
            a.download()
            reg = es.regions(ooff * isz, n, isz)
            for (name, k), o in zip(calls, outs):
                check(fails, (name, n, pname), dt, a.get(o, dt), ref("avg", dt, n, range(k), np_),
                      reg)
            if inplace is not None:
                check(fails, ("div", n, pname), dt, a.get(inplace, dt),
                      ref("avg", dt, n, range(1), np_), reg)
            assert a.guards_intact() and a.inputs_intact(ins), (n, pname)
    assert not fails, (len(fails), fails[:12])


# ---- the /np average, batched --------------------------------------------------

def _batch_cases(dt):
    """(name, k, bucket sizes, tile in vectors): k = 1 with 2 equal buckets
    (2-D rows), 32 / 40 / 64 (rows handed out XCD by XCD), 33 (plain rows)
    and 5 unequal (the bucket search); k = 2 and 3 with 3 unequal and 16
    equal buckets."""
    s = es.shapes(dt)
    big = s[-1]
    cases = [("k1_eq%d" % nb, 1, [big] * nb, es.TILE_VECS_BATCH_K1) for nb in (2, 32, 33, 40, 64)]
    cases.append(("k1_uneq5", 1, list(s), es.TILE_VECS_BATCH_K1))
    for k in (2, 3):
        cases.append(("k%d_uneq3" % k, k, list(s[2:]), es.TILE_VECS))
        cases.append(("k%d_eq16" % k, k, [big] * 16, es.TILE_VECS))
    return cases


@pytest.mark.parametrize("np_", NPS)
@pytest.mark.parametrize("dt", DTS)
def test_avg_batch(lib, ref, dev, dt, np_):
    from kungfu_amd import _lib
    from oracle.oracle import DT
    isz = es.itemsize(dt)
    fails = []
    for name, k, sizes, tile in _batch_cases(dt):
        a = Arena(dev)
        ins, outs, offs = [], [], []
        for b, n in enumerate(sizes):
            off = b % 2  # every other bucket one element past alignment
            # bucket b folds inputs b, b + 1, ..: no two buckets hold the same data
            ins.append([a.add(es.fill(dt, n, b + j), off, dt) for j in range(k)])
            outs.append(a.add(n, off, dt))
            offs.append(off)
        a.upload()
        rc = lib.kf_bucket_reduce_batch(
            _lib.ptr_array([a.ptr(i) for row in ins for i in row]), k,
            _lib.ptr_array([a.ptr(o) for o in outs]),
            (ctypes.c_size_t * len(sizes))(*sizes), len(sizes), DT[dt], 0, np_, stream())
        assert rc == 0, (name, lib.kf_last_error())
        a.download()
        for b, n in enumerate(sizes):
            check(fails, (name, b, n), dt, a.get(outs[b], dt),
                  ref("avg", dt, n, range(b, b + k), np_), es.regions(offs[b] * isz, n, isz, tile))
        assert a.guards_intact(), name  # the bytes around every output
        assert a.inputs_intact([i for row in ins for i in row]), name
    assert not fails, (len(fails), fails[:12])


# ---- the SMA blend -----------------------------------------------------------

SMA_CASES = ((2, 0.1), (3, 0.25), (8, 0.1))


@pytest.mark.parametrize("np_,alpha", SMA_CASES)
@pytest.mark.parametrize("dt", DTS)
def test_sma_blend_single(lib, ref, dev, dt, np_, alpha):
    from oracle.oracle import DT
    isz = es.itemsize(dt)
    fails = []
    for n in es.shapes(dt):
        a = Arena(dev)
        slots = []
        for pname, voff, soff in es.SMA_PLACEMENTS:
            slots.append((pname, voff, a.add(es.fill(dt, n, 0), voff, dt),
                          a.add(es.fill(dt, n, 1), soff, dt)))
        a.upload()
        for pname, voff, v, s in slots:
            rc = lib.kf_sma_blend(a.ptr(v), a.ptr(s), n, DT[dt], np_, alpha, stream())
            assert rc == 0, lib.kf_last_error()
        a.download()
        for pname, voff, v, s in slots:
            check(fails, (n, pname), dt, a.get(v, dt), ref("sma", dt, n, (0, 1), np_, alpha),
                  es.regions(voff * isz, n, isz))
        assert a.guards_intact() and a.inputs_intact([s for _, _, _, s in slots]), n
    assert not fails, (len(fails), fails[:12])


@pytest.mark.parametrize("np_,alpha", SMA_CASES)
@pytest.mark.parametrize("dt", DTS)
def test_sma_blend_batch(lib, ref, dev, dt, np_, alpha):
    """20 buckets: two launches of the batch kernel (16 + 4), the five shapes
    and the three placements in turn."""
    from kungfu_amd import _lib
    from oracle.oracle import DT
    isz = es.itemsize(dt)
    a = Arena(dev)
    buckets = []
    for b, (n, (pname, voff, soff)) in enumerate(es.sma_batch_layout(dt)):
        buckets.append((n, pname, voff, a.add(es.fill(dt, n, 2 * b), voff, dt),
                        a.add(es.fill(dt, n, 2 * b + 1), soff, dt)))
    a.upload()
    rc = lib.kf_sma_blend_batch(
        _lib.ptr_array([a.ptr(v) for _, _, _, v, _ in buckets]),
        _lib.ptr_array([a.ptr(s) for _, _, _, _, s in buckets]),
        (ctypes.c_size_t * 20)(*[n for n, _, _, _, _ in buckets]), 20, DT[dt], np_, alpha,
        stream())
    assert rc == 0, lib.kf_last_error()
    a.download()
    fails = []
    for b, (n, pname, voff, v, s) in enumerate(buckets):
        check(fails, (b, n, pname), dt, a.get(v, dt),
              ref("sma", dt, n, (2 * b, 2 * b + 1), np_, alpha), es.regions(voff * isz, n, isz))
    assert a.guards_intact() and a.inputs_intact([s for _, _, _, _, s in buckets])
    assert not fails, (len(fails), fails[:12])


# ---- bf16 plain ops: every ordered pair of specials -------------------------------

@pytest.mark.parametrize("op", ["sum", "min", "max", "prod"])
def test_bf16_all_pairs(lib, orc, dev, op):
    """tests/test_gpu_parity.py::test_specials_all_pairs runs the golden set,
    which has no bf16. n = 19 * 19 pairs, continued to 367 elements: 45
    vectors and a scalar tail of 7 (aligned), a head of 7 (one past)."""
    from kungfu_amd import _lib
    from oracle.oracle import DT, OPS
    p = es.pool("bf16")
    n = p.size * p.size + 6
    x = np.resize(np.repeat(p, p.size), n)
    y = np.resize(np.tile(p, p.size), n)
    assert len(set(zip(x.tolist(), y.tolist()))) == p.size ** 2
    want = orc.transform2(x, y, "bf16", op)
    for off in (0, 1):
        reg = es.regions(off * 2, n, 2)
        assert reg["tail" if off == 0 else "head"].size == 7 and reg["ragged"].size
        a = Arena(dev)
        ix, iy, o = a.add(x, off, "bf16"), a.add(y, off, "bf16"), a.add(n, off, "bf16")
        a.upload()
        rc = lib.kf_bucket_reduce(_lib.ptr_array([a.ptr(ix), a.ptr(iy)]), 2, a.ptr(o), n,
                                  DT["bf16"], OPS[op], stream())
        assert rc == 0, lib.kf_last_error()
        a.download()
        got = a.get(o, "bf16")
        assert es.same("bf16", got, want), (off, es.describe("bf16", got, want, reg))
        if op in ("min", "max"):
            # Elt<bf16_t>: MIN / MAX select an input and keep its bits
            assert ((got == x) | (got == y)).all(), off
            assert np.array_equal(got, want), off
        assert a.guards_intact() and a.inputs_intact([ix, iy])
