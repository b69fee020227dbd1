"""Muon without a device: the constructor's refusals, the C entries' checks (all
before any HIP call), the names, and tests/muon_ref.py's own properties."""
import ctypes
import types

import numpy as np
import pytest
import torch

import muon_ref

ERR_DTYPE, ERR_ARG = 1, 3
F32, BF16, F16 = 0x20408, 0x20209, 0x20208


def test_names_declared_and_exported():
    from kungfu_amd import _lib, exchange, ops
    from kungfu_amd.torch import optimizers as topt
    assert "ShardedMuonOptimizer" in topt.__all__
    header = open(_lib.__file__.replace("kungfu_amd/_lib.py", "include/kungfu_amd.h")).read()
    lib = _lib.load()
    for name in ("kf_muon_tile", "kf_muon_momentum_batch", "kf_muon_scale_batch",
                 "kf_muon_gemm_grouped", "kf_muon_apply_batch", "kf_exchange_muon_batch"):
        assert name in _lib.EXPORTED and name + "(" in header and getattr(lib, name)
    for name in ("muon_momentum_batch_", "muon_gemm_grouped_", "muon_newton_schulz_",
                 "muon_apply_batch_", "MuonPlan"):
        assert hasattr(ops, name)
    assert hasattr(exchange.NativeExchange, "muon_step_")
    assert ops.muon_tile() == 64


def test_construction_rules_and_refusals():
    from kungfu_amd import optimizers as kopt
    from kungfu_amd.torch import optimizers as topt
    m = torch.nn.Linear(5, 3, bias=False)

    def sgd(params=None, **options):
        o = torch.optim.SGD(params or m.parameters(), lr=0.02, momentum=0.95, nesterov=True)
        o.param_groups[0].update(options)
        return o

    o = topt.ShardedMuonOptimizer(sgd(), m.named_parameters(), ns_steps=3)
    assert isinstance(o, torch.optim.SGD) and len(o.state) == 0 and o.momentum_buffers() == {}
    assert o._kf_ns_steps == 3
    no_gather = types.SimpleNamespace(world=1, rank=0, reduce_shards_=0, grad_shards_=0)
    for error, word, opt, kw in (
            (TypeError, "wraps a torch.optim.SGD", torch.optim.AdamW(m.parameters(), lr=0.1), {}),
            (ValueError, "dampening must be 0", sgd(dampening=0.1, nesterov=False), {}),
            (ValueError, "maximize=True is not supported", sgd(maximize=True), {}),
            (ValueError, r"ns_steps must be an int in \[1, 16\]", sgd(), {"ns_steps": 0}),
            (ValueError, "ns_steps", sgd(), {"ns_steps": 17}),
            (ValueError, "ns_steps", sgd(), {"ns_steps": True}),
            (ValueError, "ns_steps", sgd(), {"ns_steps": 5.0}),
            (ValueError, "fewer than 2 dimensions.*ShardedAdamOptimizer built over their own "
                         "named_parameters", sgd(torch.nn.Linear(5, 3).parameters()), {}),
            (ValueError, "gather_params_", sgd(), {"exchange": no_gather})):
        with pytest.raises(error, match=word):
            kopt.ShardedMuonOptimizer(opt, **kw)
    bf = torch.nn.Parameter(torch.zeros(8, 8, dtype=torch.bfloat16))
    bad = kopt.ShardedMuonOptimizer(sgd([bf]))
    bf.grad = torch.zeros_like(bf)
    with pytest.raises(TypeError, match="updates f32 parameters"):
        bad.step()


def test_c_entries_refusals_in_order():
    """Each call has one fault more to its right than the refusal it must report."""
    from kungfu_amd import _lib
    lib, pa = _lib.load(), _lib.ptr_array
    cnt = lambda n: (ctypes.c_size_t * 1)(n)  # noqa: E731
    why = lambda: lib.kf_last_error().decode()  # noqa: E731
    mh, ah = (_lib.MuonHyper * 1)(), (_lib.MuonApply * 1)()

    def mom(g=16, m=32, d=48, c=cnt(64), nb=1, dt=F32, np_=0, h=mh):
        return lib.kf_muon_momentum_batch(pa([g]), m and pa([m]), pa([d]), c, nb, dt, np_, h, None)

    assert mom(nb=-1, dt=BF16) == ERR_ARG and "nb < 0" in why()
    assert mom(nb=0, dt=BF16) == 0
    assert mom(dt=BF16, m=None) == ERR_DTYPE and "f32" in why()
    assert mom(m=None, g=0) == ERR_ARG and "null table" in why()
    assert mom(h=None) == ERR_ARG and "null table" in why()
    assert mom(g=0, d=50) == ERR_ARG and "null pointer" in why()
    assert mom(d=50, np_=-1) == ERR_ARG and "misaligned" in why()
    assert mom(np_=-1, c=cnt(12)) == ERR_ARG and "np < 0" in why()
    assert mom(c=cnt(12)) == ERR_ARG and "multiples of 8" in why()

    def scale(d=2, x=4, c=cnt(5), sq=8, nb=1):
        return lib.kf_muon_scale_batch(pa([d]), pa([x]), c, sq, nb, None)

    assert scale(nb=-1) == ERR_ARG and scale(nb=0) == 0
    assert scale(sq=None) == ERR_ARG and "null table" in why()
    assert scale(d=0) == ERR_ARG and "null pointer" in why()
    assert scale(x=5) == ERR_ARG and "misaligned" in why()
    assert scale(sq=12) == ERR_ARG and "misaligned" in why()

    def apply(p=4, x=2, c=cnt(5), h=ah, nb=1, dt=F32):
        return lib.kf_muon_apply_batch(pa([p]), pa([x]), c, h, nb, dt, None)

    assert apply(nb=-1, dt=BF16) == ERR_ARG and apply(nb=0) == 0 and apply(dt=BF16, h=None) == ERR_DTYPE
    assert apply(h=None) == ERR_ARG and "null table" in why()
    assert apply(x=0) == ERR_ARG and "null pointer" in why()
    assert apply(p=6) == ERR_ARG and "misaligned" in why()

    def gemm(count=1, dt=BF16, table=True, **fields):
        q = (_lib.MuonGemm * 1)()
        vals = dict(a=2, b=4, c=6, cin=None, m=3, n=7, k=5, lda=5, ldb=7, ldcin=7, ldc=7,
                    trans_a=0, trans_b=0)
        vals.update(fields)
        for k, v in vals.items():
            setattr(q[0], k, v)
        return lib.kf_muon_gemm_grouped(q if table else None, count, dt, 1.0, 1.0, None)

    assert gemm(count=-1, table=False) == ERR_ARG and "count < 0" in why()
    assert gemm(count=0, table=False) == 0
    assert gemm(dt=F16, table=False) == ERR_DTYPE and "bf16" in why()
    assert gemm(table=False, m=0) == ERR_ARG and "null table" in why()
    assert gemm(k=0, a=None) == ERR_ARG and "dimension" in why()
    assert gemm(k=(1 << 31) - 32, a=None) == ERR_ARG and "INT_MAX" in why()
    assert gemm(c=None, b=5) == ERR_ARG and "null matrix" in why()
    assert gemm(cin=9, trans_a=2) == ERR_ARG and "misaligned" in why()
    assert gemm(trans_b=2, lda=4) == ERR_ARG and "0 or 1" in why()
    for ld in ({"lda": 4}, {"ldb": 6}, {"ldc": 6}, {"cin": 8, "ldcin": 6},
               {"trans_a": 1, "lda": 2}, {"trans_b": 1, "ldb": 4}):
        assert gemm(**ld) == ERR_ARG and "leading dimension" in why(), ld
    assert gemm(m=1 << 30, n=1 << 30, lda=5, ldb=1 << 30, ldc=1 << 30) == ERR_ARG and "tiles" in why()
    # the exchange entry: no handle is refused before anything else
    assert lib.kf_exchange_muon_batch(None, None, None, None, None, 0, F32, None, 1, None) == ERR_ARG


def test_reference_newton_schulz_properties():
    rng = np.random.default_rng(0)
    wide = muon_ref.bf16(rng.standard_normal((48, 80)))
    x = muon_ref.newton_schulz(wide, 5, muon_ref.identity)
    sv = np.linalg.svd(x, compute_uv=False)
    assert 0.5 <= sv.min() and sv.max() <= 1.5, sv
    tall = muon_ref.newton_schulz(wide.T.copy(), 5, muon_ref.identity)
    assert np.abs(tall - x.T).max() <= 1e-12
