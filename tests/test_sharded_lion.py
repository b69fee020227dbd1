"""ShardedLionOptimizer without a GPU: tests/lion_ref.py's known answers at the
decision points, apply(signs) == update, the C entries' refusals in their
documented order and the constructor's."""
import ctypes
import types

import numpy as np
import pytest
import torch

import lion_ref
from oracle.oracle import f32_to_bf16_bits

ERR_DTYPE, ERR_ARG = 1, 3
F32, BF16, F16, F64 = 0x20408, 0x20209, 0x20208, 0x20808


def _store(x, dt):
    x = np.asarray(x, np.float32)
    return f32_to_bf16_bits(x) if dt == "bf16" else x


def _bits(a):
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint16).tolist()


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_known_answers(dt):
    h = lion_ref.hyper(0.25, (0.5, 0.5), 0.0)  # every scalar a power of two: exact answers
    g = _store([0.0, -0.0, np.nan, 1.0, -1.0, 0.0], dt)
    m = _store([0.0, -0.0, 0.0, 0.0, 0.0, 2.0], dt)
    p = _store([-0.0, 1.0, 1.0, 1.0, 1.0, -0.0], dt)
    g, m, p = (np.concatenate([a, _store(np.zeros(26), dt)]) for a in (g, m, p))
    m2, words = lion_ref.signs(g, m, dt, h)
    # c = +0, -0, NaN, +, -, + (from m alone)
    assert lion_ref.codes_of(words, 6).tolist() == [0, 0, 2, 1, 3, 1]
    out = lion_ref.apply(p, words, dt, h)
    want = _store([-0.0, 1.0, 0, 0.75, 1.25, -0.25], dt)
    assert _bits(out)[:2] == _bits(want)[:2] and _bits(out)[3:6] == _bits(want)[3:6]
    assert _bits(out)[2] == int(lion_ref.QNAN[dt])
    assert _bits(m2)[3:6] == _bits(_store([0.5, -0.5, 1.0], dt))
    # decay alone: code 0 keeps dk * p, and -0 * dk stays -0
    hd = lion_ref.hyper(0.25, (0.5, 0.5), 2.0)  # dk = 0.5
    outd = lion_ref.apply(p, np.zeros_like(words), dt, hd)
    assert _bits(outd)[:2] == _bits(_store([-0.0, 0.5], dt))


def test_code_positions():
    assert [lion_ref.sign_bytes(q) for q in (32, 64, 96, 128, 4096 + 32)] == [16, 16, 32, 32, 1040]
    for i, (word, shift) in zip((0, 15, 16, 31), ((0, 0), (0, 30), (1, 0), (1, 30))):
        g = np.zeros(32, np.float32)
        g[i] = -1.0
        _, words = lion_ref.signs(g, np.zeros(32, np.float32), "f32", lion_ref.hyper(0.1))
        want = np.zeros(4, np.uint32)
        want[word] = 3 << shift
        assert words.tolist() == want.tolist(), i


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("wd", [0.0, 0.1])
def test_apply_of_signs_is_update(dt, wd):
    rng, n = np.random.default_rng(3), 4096 + 96
    p, g, m = (_store(rng.standard_normal(n), dt) for _ in range(3))
    g[rng.integers(0, n, 200)] = 0
    m[g == 0] = 0
    h = lion_ref.hyper(1e-3, weight_decay=wd)
    m1, words = lion_ref.signs(g, m, dt, h, np_=3)
    a = lion_ref.apply(p, words, dt, h, 4096, 7, 11)
    u, m2 = lion_ref.update(p, g, m, dt, h, 3, 4096, 7, 11)
    assert a.tobytes() == u.tobytes() and m1.tobytes() == m2.tobytes()
    # the data reach all three outcomes (a bf16 step of 1e-3 moves p only with probability)
    k = lion_ref.codes_of(words, n)
    assert (a != p).sum() > n // 8 and all((k == code).sum() >= 100 for code in (0, 1, 3))


def test_c_entries_refusals_in_order():
    """Every check comes before any HIP call, in the header's order: each call
    has one fault more to its right than the refusal it must report."""
    from kungfu_amd import _lib
    lib, pa = _lib.load(), _lib.ptr_array
    assert [lib.kf_lion_sign_bytes(q) for q in (0, 32, 96, 4128)] == \
        [lion_ref.sign_bytes(q) for q in (0, 32, 96, 4128)]
    h = _lib.lion_hyper_array([lion_ref.hyper(0.1)])
    cnt = lambda n: (ctypes.c_size_t * 1)(n)  # noqa: E731
    u64, u32 = (ctypes.c_uint64 * 1), (ctypes.c_uint32 * 1)

    def why():
        return lib.kf_last_error().decode()

    def update(p=16, g=32, m=48, c=cnt(64), base=u64(0), st=u32(0), nb=1, dt=BF16, np_=0, hy=h):
        return lib.kf_lion_update_batch(pa([p]), g and pa([g]), pa([m]), c, base, st, nb, dt, np_,
                                        hy, 0, None)

    def signs(g=16, m=32, codes=48, c=cnt(64), nb=1, dt=F32, np_=0):
        return lib.kf_lion_signs_batch(pa([g]), pa([m]), codes and pa([codes]), c, nb, dt, np_, h, None)

    def apply(p=16, codes=32, c=cnt(64), base=u64(0), st=u32(0), nb=1, dt=BF16):
        return lib.kf_lion_apply_signs_batch(pa([p]), pa([codes]), c, base, st, nb, dt, h, 0, None)

    assert update(nb=-1, g=None) == ERR_ARG and "nb < 0" in why()
    assert update(nb=0, g=None) == 0
    assert update(g=None, dt=F16) == ERR_ARG and "null table" in why()
    for dt in (F16, F64, 0x10408):
        assert update(dt=dt, st=None) == ERR_DTYPE and "stochastic narrowing" in why()
    assert update(st=None, np_=-1) == ERR_ARG and "null table" in why()
    assert update(dt=F32, base=None, st=None, np_=-1) == ERR_ARG and "np < 0" in why()
    assert update(np_=-1, p=0) == ERR_ARG and "np < 0" in why()
    assert update(p=0, g=36) == ERR_ARG and "null pointer" in why()
    assert update(m=50, c=cnt(48)) == ERR_ARG and "16-byte" in why()
    assert update(c=cnt(48), base=u64(4)) == ERR_ARG and "multiples of 32" in why()
    assert update(base=u64(4)) == ERR_ARG and "multiples of 8" in why()
    assert update(base=u64(1 << 33)) == ERR_ARG and "2^33" in why()
    assert signs(codes=None) == ERR_ARG and "null table" in why()
    assert signs(dt=F16) == ERR_DTYPE and signs(np_=-1) == ERR_ARG
    assert signs(codes=52) == ERR_ARG and "16-byte" in why()
    assert signs(c=cnt(16)) == ERR_ARG and "multiples of 32" in why()
    assert apply(dt=F64) == ERR_DTYPE and apply(st=None) == ERR_ARG
    assert apply(codes=0) == ERR_ARG and "null pointer" in why()
    assert apply(c=cnt(80)) == ERR_ARG and apply(base=u64(12)) == ERR_ARG
    # the exchange entry: no handle is refused before anything else
    assert lib.kf_exchange_lion_batch(None, None, None, None, None, 0, F32, None, None, 0, 0, 1,
                                      None) == ERR_ARG


def test_construction_rules_and_refusals():
    from kungfu_amd import optimizers as kopt
    from kungfu_amd.torch import optimizers as topt
    assert "ShardedLionOptimizer" in topt.__all__
    m = torch.nn.Linear(5, 3)

    def adam(cls=torch.optim.AdamW, **options):
        o = cls(m.parameters(), lr=1e-4, betas=(0.9, 0.99), weight_decay=0.1)
        o.param_groups[0].update(options)
        return o

    o = topt.ShardedLionOptimizer(adam(torch.optim.Adam), m.named_parameters(), sr_seed=5)
    assert isinstance(o, torch.optim.Adam) and len(o.state) == 0 and o.momentum_buffers() == {}
    assert (o._kf_sign_wire, o._kf_sr_seed) == (False, 5)
    no_gather = types.SimpleNamespace(world=1, rank=0, reduce_shards_=0, grad_shards_=0)
    for error, word, opt, kw in (
            (TypeError, "Adam or AdamW", torch.optim.SGD(m.parameters(), lr=0.1), {}),
            (ValueError, "amsgrad", adam(amsgrad=True), {}),
            (ValueError, "maximize", adam(maximize=True), {}),
            (ValueError, "sr_seed", adam(), {"sr_seed": -1}),
            (ValueError, "sr_seed", adam(), {"sr_seed": True}),
            (ValueError, "sign_wire", adam(), {"sign_wire": 1}),
            (ValueError, "gather_params_", adam(), {"exchange": no_gather}),
            (ValueError, "NativeExchange", adam(), {"sign_wire": True}),  # collective.Exchange
            (ValueError, "NativeExchange", adam(), {"sign_wire": True, "exchange": no_gather})):
        with pytest.raises(error, match=word):
            kopt.ShardedLionOptimizer(opt, **kw)
    f16 = torch.nn.Parameter(torch.zeros(64, dtype=torch.float16))
    bad = kopt.ShardedLionOptimizer(torch.optim.AdamW([f16], lr=1e-4))
    f16.grad = torch.zeros_like(f16)
    with pytest.raises(TypeError, match="f32 and bf16"):
        bad.step()
