"""ShardedAdamOptimizer(state_bits=8) without a GPU: the
format's numpy restatement (tests/adam8_ref.py) on its own contract, the host
codebook, the source pins and the C ABI's argument checks (no device touched),
the construction rules, and the whole step over a numpy epilogue and an
in-process loopback at worlds 1, 2 and 4, with and without a gate, with a
checkpoint in the middle."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import adam8_cpu as cpu
import adam8_ref as ref
import adam_ref

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

OK, ERR_DTYPE, ERR_ARG = 0, 1, 3
F32, I32, F16, BF16, F64 = 0x20408, 0x10408, 0x20208, 0x20209, 0x20808

# kf_adam8.hip: segments per launch, elements one workgroup does per round,
# blocks of a codec launch (test_sources_pinned)
ADAM8_SEG = 24
TILE = 256 * 4 * 1
CODEC_BLOCKS = 1024


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- the format -------------------------------------------------------------------

def test_tables_known_answers():
    ts, tu = ref.TABLES
    f = np.float32
    assert ts[0] == f(-0.99296874) and ts[127] == 0 and ts[254] == f(0.99296874) and ts[255] == 1
    assert tu[0] == 0 and tu[1] == f(3.25e-07) and tu[2] == f(7.75e-07)
    assert tu[254] == f(0.9964844) and tu[255] == 1
    assert np.array_equal(ts[:127], -ts[254:127:-1]) and not np.signbit(ts[127])
    for t, mid in zip(ref.TABLES, ref.MIDS):
        assert t.dtype == np.float32 and t.size == 256 and mid.size == 255
        assert (np.diff(t) > 0).all() and (np.diff(mid) > 0).all()
        assert (mid > t[:-1]).all() and (mid < t[1:]).all()
    assert ref.TABLES[0][ref.ZERO_CODE[0]] == 0 and ref.TABLES[1][ref.ZERO_CODE[1]] == 0


def test_host_codebook_is_the_restatement():
    from kungfu_amd import _lib, ops
    for which in (0, 1):
        got = ops.adam8_codebook(which)
        assert got.dtype == np.float32 and got.tobytes() == ref.TABLES[which].tobytes()
    lib = _lib.load()
    out = (ctypes.c_float * 256)()
    assert lib.kf_adam8_codebook(2, out) == ERR_ARG and lib.kf_adam8_codebook(-1, out) == ERR_ARG
    assert lib.kf_adam8_codebook(0, None) == ERR_ARG
    assert b"kf_adam8_codebook:" in lib.kf_last_error()
    assert ops.ADAM8_ZERO_CODE == ref.ZERO_CODE and ops.ADAM8_BLOCK == ref.BLOCK


def _random_blocks(seed, nblocks, lo, hi, signed):
    """Blocks of standard-normal values times 2^k, k uniform in [lo, hi) per
    block."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((nblocks, 64))
    x = x if signed else np.abs(x)
    return np.ldexp(x, rng.integers(lo, hi, (nblocks, 1))).astype(np.float32).reshape(-1)


@pytest.mark.parametrize("which", [ref.SIGNED, ref.UNSIGNED])
def test_round_trip(which):
    """The signed scale comes back bit for bit, every block holds a code 255,
    and no element is further from its value than D * (1 + 2^-16) * |a|: half
    the widest interval of the table's top decade, with a margin for the
    rounding of the division and of the multiply."""
    x = _random_blocks(3 + which, 20000, -38, 86, which == ref.SIGNED)
    codes, a = ref.quantize(x, which)
    back = ref.dequantize(codes, a, which)
    blocks = back.reshape(-1, 64)
    top = codes.reshape(-1, 64) == 255
    assert top.any(axis=1).all()
    assert (_bits(blocks[top]) == _bits(np.repeat(a, top.sum(axis=1)))).all()
    assert np.array_equal(_bits(ref.scales_of(back)), _bits(a))
    err = np.abs(back.astype(np.float64) - x.astype(np.float64)) / \
        np.repeat(np.abs(a).astype(np.float64), 64)
    print("largest round-trip error / |a|: %.7f (D = %.7f)" % (err.max(), ref.D[which]))
    assert err.max() <= ref.D[which] * (1 + 2.0 ** -16)
    assert a.min() < 0 if which == ref.SIGNED else a.min() > 0


@pytest.mark.parametrize("which", [ref.SIGNED, ref.UNSIGNED])
def test_requantization_is_idempotent(which):
    """Quantizing a dequantized block gives the same codes and the same
    scale, for |a| from 2^-40 to 2^80: checkpoints rest on it."""
    x = _random_blocks(7 + which, 20000, -42, 79, which == ref.SIGNED)
    codes, a = ref.quantize(x, which)
    keep = np.repeat((np.abs(a) >= 2.0 ** -40) & (np.abs(a) <= 2.0 ** 80), 64)
    assert keep.mean() > 0.9
    back = ref.dequantize(codes, a, which)
    codes2, a2 = ref.quantize(back, which)
    assert np.array_equal(codes2[keep], codes[keep])
    assert np.array_equal(_bits(a2)[keep[::64]], _bits(a)[keep[::64]])


def test_format_edges():
    z = np.zeros(64, np.float32)
    for which in (0, 1):
        c, a = ref.quantize(z, which)
        zc, za = ref.zero_state(64, which)
        assert np.array_equal(c, zc) and _bits(a)[0] == 0 and za[0] == 0
        assert not ref.dequantize(c, a, which).any()
    x = z.copy()
    x[3], x[9] = -2.0, 2.0
    assert ref.quantize(x, 0)[1][0] == 2.0      # +mag present: a positive scale
    x[9] = 1.0
    c, a = ref.quantize(x, 0)
    assert a[0] == -2.0 and c[3] == 255              # only -mag: a negative scale
    assert abs(ref.TABLES[0][c[9]] + 0.5) <= ref.D[0]  # y = 1 / -2
    x[20] = np.nan
    c, a = ref.quantize(x, 0)
    assert _bits(a)[0] == ref.NAN_BITS and not c.any()
    # a y exactly on a midpoint takes the lower code
    y = z.copy()
    y[0], y[1:4] = 1.0, ref.MIDS[1][[0, 100, 254]]
    assert list(ref.quantize(y, 1)[0][:4]) == [255, 0, 100, 254]


# ---- sources, exports, argument checks -----------------------------------------------

def test_sources_pinned():
    src = open(os.path.join(ROOT, "kungfu_amd", "csrc", "kf_adam8.hip")).read()
    assert "constexpr int kAdam8Seg   = %d;" % ADAM8_SEG in src
    block = int(re.search(r"constexpr int kAdam8Block = (\d+);", src).group(1))
    elts = int(re.search(r"constexpr int kAdam8Elts  = (\d+);", src).group(1))
    unroll = int(re.search(r"#define KF_ADAM8_UNROLL (\d+)", src).group(1))
    assert block * elts * unroll == TILE and block == 256
    assert "constexpr unsigned kAdam8CodecBlocks = %d;" % CODEC_BLOCKS in src
    assert "plan_update_batch<Adam8Args>(" in src and '#include "kf_adam_math.hpp"' in src
    assert "adam_math<float, DIV, DECAY, 2, f32x2>" in src
    assert "v_max_f32" not in src.split("#include")[1] and "fmaxf" not in src
    mk = open(os.path.join(ROOT, "kungfu_amd", "csrc", "Makefile")).read()
    assert re.search(r"NAMES\s*:=.*\bkf_adam8\b", mk)
    from kungfu_amd import _lib
    lib = _lib.load()
    for name in ("kf_adam8_codebook", "kf_adam8_update_batch", "kf_adam8_update_batch_gated",
                 "kf_adam8_master_update_batch", "kf_adam8_master_update_batch_gated",
                 "kf_adam8_quantize", "kf_adam8_dequantize"):
        assert name in _lib.EXPORTED and getattr(lib, name) is not None
    hdr = open(os.path.join(ROOT, "include", "kungfu_amd.h")).read()
    for name in _lib.EXPORTED:
        if name.startswith("kf_adam8"):
            assert re.search(r"\bint %s\(" % name, hdr), name


def test_entries_arg_errors():
    """Every check of the entries comes before any HIP call."""
    from kungfu_amd import _lib
    lib = _lib.load()
    pa = _lib.ptr_array
    cnt = lambda *v: (ctypes.c_size_t * len(v))(*v)  # noqa: E731
    plain = _lib.adam_hyper_array([adam_ref.hyper(1e-3)])
    six = [pa([16 * (i + 1)]) for i in range(6)]
    seven = [pa([16 * (i + 1)]) for i in range(7)]

    def make(fn, tabs, dt0, gated_):
        def call(t=tabs, c=cnt(64), nb=1, dt=dt0, np_=0, h=plain, gate=96, st=128):
            extra = (gate, st) if gated_ else ()
            return fn(*t, c, nb, dt, np_, h, *extra, None)
        return call

    cases = ((lib.kf_adam8_update_batch, six, F32, False, b"kf_adam8_update_batch"),
             (lib.kf_adam8_update_batch_gated, six, F32, True, b"kf_adam8_update_batch_gated"),
             (lib.kf_adam8_master_update_batch, seven, BF16, False,
              b"kf_adam8_master_update_batch"),
             (lib.kf_adam8_master_update_batch_gated, seven, F16, True,
              b"kf_adam8_master_update_batch_gated"))
    for fn, tabs, dt0, gated_, name in cases:
        call = make(fn, tabs, dt0, gated_)
        k = len(tabs)
        assert call(t=[None] * k, c=None, nb=0) == OK
        assert call(c=cnt(0)) == OK
        assert call(nb=-1) == ERR_ARG
        for i in range(k):
            t = list(tabs)
            t[i] = None
            assert call(t=t) == ERR_ARG, i
            t[i] = pa([0])
            assert call(t=t) == ERR_ARG, i
            t[i] = pa([16 * (i + 1) + 2])        # misaligned for every stream
            assert call(t=t) == ERR_ARG, i
            if i < k - 2:                        # 4-byte alignment serves the scales alone
                t[i] = pa([16 * (i + 1) + 4])
                assert call(t=t) == ERR_ARG, i
        assert call(c=None) == ERR_ARG and call(h=None) == ERR_ARG
        assert call(np_=-1) == ERR_ARG
        for n in (1, 63, 65, 96, 4097):
            assert call(c=cnt(n)) == ERR_ARG, n
        assert b"multiples of 64" in lib.kf_last_error() and name + b":" in lib.kf_last_error()
        others = {F32, BF16, F16, F64, I32} - ({F32} if k == 6 else {BF16, F16})
        for dt in others:
            assert call(dt=dt) == ERR_DTYPE, hex(dt)
        zero = _lib.adam_hyper_array([adam_ref.hyper(1e-3, betas=(1.0, 0.999))])
        if not gated_:
            assert call(h=zero) == ERR_ARG
        else:
            assert call(gate=None) == ERR_ARG and call(st=None) == ERR_ARG
    for fn, name in ((lib.kf_adam8_quantize, b"kf_adam8_quantize"),
                     (lib.kf_adam8_dequantize, b"kf_adam8_dequantize")):
        assert fn(None, None, None, 0, 0, None) == OK
        assert fn(16, 32, 48, 64, 2, None) == ERR_ARG
        assert fn(16, 32, 48, 63, 0, None) == ERR_ARG
        assert fn(None, 32, 48, 64, 0, None) == ERR_ARG
        assert fn(16, None, 48, 64, 0, None) == ERR_ARG and fn(16, 32, None, 64, 0, None) == ERR_ARG
        assert fn(24, 32, 48, 64, 0, None) == ERR_ARG and fn(16, 36, 50, 64, 0, None) == ERR_ARG
        assert name + b":" in lib.kf_last_error()


# ---- construction and refusals ------------------------------------------------------------

def _lin(dtype=torch.float32):
    torch.manual_seed(0)
    return torch.nn.Linear(5, 3).to(dtype)


class _NoGatherExchange:
    world, rank = 1, 0

    def adam_step_(self, *a):
        return None

    adam_master_step_ = adam_step_


def test_construction_rules_and_refusals():
    from kungfu_amd import optimizers as kopt
    from kungfu_amd.torch import optimizers as topt
    m = _lin()
    adam = lambda mod=m: torch.optim.Adam(mod.parameters(), lr=1e-3)  # noqa: E731
    assert kopt.ShardedAdamOptimizer(adam())._kf_state_bits == 32
    assert kopt.ShardedAdamOptimizer(adam(), state_bits=32)._kf_state_bits == 32
    o = topt.ShardedAdamOptimizer(adam(), m.named_parameters(), state_bits=8)
    assert o._kf_state_bits == 8 and o.state_buffers() == {}
    o = kopt.ShardedAdamOptimizer(adam(), state_bits=8, max_grad_norm=1.0, loss_scale="dynamic")
    assert o._kf_state_bits == 8 and o._kf_gated
    for bits in (0, 4, 16, 64, "8", 8.5, None, True):
        with pytest.raises(ValueError, match="state_bits"):
            kopt.ShardedAdamOptimizer(adam(), state_bits=bits)
    with pytest.raises(ValueError, match="state_bits=8.*stochastic_rounding"):
        kopt.ShardedAdamOptimizer(adam(_lin(torch.bfloat16)), state_bits=8,
                                  stochastic_rounding=True)
    with pytest.raises(ValueError, match="state_bits=8.*f64"):
        kopt.ShardedAdamOptimizer(adam(_lin(torch.float64)), state_bits=8)
    for dt in (torch.bfloat16, torch.float16):
        with pytest.raises(ValueError, match="state_bits=8.*master_weights=True"):
            kopt.ShardedAdamOptimizer(adam(_lin(dt)), state_bits=8)
        kopt.ShardedAdamOptimizer(adam(_lin(dt)), state_bits=8, master_weights=True)
    with pytest.raises(ValueError, match="state_bits"):
        kopt.ShardedLAMBOptimizer(adam(), state_bits=8)
    kopt.ShardedLAMBOptimizer(adam(), state_bits=32)
    with pytest.raises(ValueError, match=r"state_bits=8.*reduce_shards_"):
        kopt.ShardedAdamOptimizer(adam(), exchange=_NoGatherExchange(), state_bits=8)
    kopt.ShardedAdamOptimizer(adam(), exchange=_NoGatherExchange())  # not needed without it
    doc = kopt.ShardedAdamOptimizer.__doc__
    for words in ("state_bits=8", "2.125", "16.25", "identical bit for bit for any", "subnormal",
                  "divides\n        by eps alone"):
        assert words in doc, words


# ---- the whole step -------------------------------------------------------------------------

def _world1_exchange():
    from kungfu_amd.collective import Exchange
    return Exchange(epilogue=cpu.CpuAdam8Epilogue())


def _run_world(world, body):
    if world == 1:
        body(0, _world1_exchange())
    else:
        cpu.loop_ranks(world, body)


@pytest.mark.parametrize("gate", [False, True])
@pytest.mark.parametrize("kind", ["f32", "bf16"])
def test_worlds_1_2_4_give_the_same_bits(kind, gate):
    """Five steps over the numpy epilogue at worlds 1, 2 and 4 on gradients
    whose average is the same in every world: parameters, master and the
    dequantized state equal adam8_ref's on the unsharded buckets, on every
    rank of every world. Under the gate step BAD carries an inf on the last
    rank and is skipped."""
    want = cpu.reference_run(kind, gate=gate)
    assert want["applied"] == (cpu.STEPS - 1 if gate else cpu.STEPS)
    for world in (1, 2, 4):
        def body(rank, ex):
            ps, opt = cpu.make_optimizer(ex, kind, gate=gate)
            cpu.run_steps(ps, opt, kind, world, rank, gate=gate)
            assert len(opt.state) == 0 and len(opt._kf_groups[0]["pb"].buckets) == 2
            cpu.check_against_reference(ps, opt, want, kind)
            if gate:
                assert opt.skipped_steps() == 1
                assert opt.loss_scale_value() == float(want["gate"]["loss_scale"])
        _run_world(world, body)


@pytest.mark.parametrize("kind", ["f32", "f16"])
def test_a_skipped_step_keeps_every_byte(kind):
    ps, opt = cpu.make_optimizer(_world1_exchange(), kind, gate=True)
    cpu.run_steps(ps, opt, kind, 1, 0, steps=cpu.BAD, gate=True)
    G = opt._kf_groups[0]
    assert G["b8"] and G["m"][0].dtype == torch.uint8 and G["ms"][0].dtype == torch.float32
    assert (G["w"] is not None) == (kind != "f32")

    def raw():
        ts = G["m"] + G["v"] + G["ms"] + G["vs"] + (G["w"] or []) + list(G["pb"].buckets)
        return [cpu.to_numpy(t).tobytes() for t in ts]
    before, scale = raw(), opt.loss_scale_value()
    cpu.run_steps(ps, opt, kind, 1, 0, first=cpu.BAD, steps=1, gate=True)
    assert opt.skipped_steps() == 1 and opt.applied_steps() == cpu.BAD
    assert opt.loss_scale_value() == scale / 2
    assert raw() == before
    cpu.run_steps(ps, opt, kind, 1, 0, first=cpu.BAD + 1, steps=1, gate=True)
    assert raw() != before


def test_state_is_allocated_as_the_zero_state():
    ps, opt = cpu.make_optimizer(_world1_exchange(), "f32")
    opt._kf_build_sharded()
    G = opt._kf_groups[0]
    opt._kf_states(G)
    for codes, scales, which in ((G["m"], G["ms"], 0), (G["v"], G["vs"], 1)):
        for c, s, b in zip(codes, scales, G["pb"].buckets):
            assert c.numel() == b.numel() and s.numel() * 64 == b.numel()
            assert (c == ref.ZERO_CODE[which]).all() and not s.any()
    # bytes per element of the state, from the tensors themselves
    elts = sum(b.numel() for b in G["pb"].buckets)
    nbytes = sum(t.numel() * t.element_size() for k in ("m", "v", "ms", "vs") for t in G[k])
    assert nbytes / elts == 2.125


@pytest.mark.parametrize("kind,worlds", [("f32", (1, 1)), ("bf16", (2, 4)), ("f32", (4, 2))])
def test_checkpoint_round_trip(kind, worlds):
    """state_buffers() after step 3, load_state_buffers() into a new optimizer
    (of another world), three more steps: the uninterrupted run's bits at step
    6, which are adam8_ref's."""
    first, second = worlds
    saved = {}

    def save(rank, ex):
        ps, opt = cpu.make_optimizer(ex, kind)
        cpu.run_steps(ps, opt, kind, first, rank, steps=3)
        snap = cpu.snapshot(ps, opt)
        if rank == 0:
            saved["snap"] = snap
    _run_world(first, save)
    params, state = saved["snap"]
    want = cpu.reference_run(kind, 6)

    def resume(rank, ex):
        ps, opt = cpu.make_optimizer(ex, kind, arrays=params)
        for g in opt.param_groups:
            g["lr"] = cpu.HYPER["lr"] * 0.5 ** 3
        cpu.load_snapshot(ps, opt, state)
        cpu.run_steps(ps, opt, kind, second, rank, first=3, steps=3)
        cpu.check_against_reference(ps, opt, want, kind)
    _run_world(second, resume)


# ---- a sanity cap on quality ------------------------------------------------------------------

def test_quality_cap_on_a_noisy_quadratic():
    """0.5 * sum h_i (p_i - t_i)^2 over 4096 parameters, h = exp(U(-3, 3)),
    gradient noise 0.1 N(0, 1), 300 Adam steps at lr 1e-2 from p = 0, on the
    restatement alone: the loss with 8-bit state is at most 1.1 times the loss
    with f32 state. This guards against exp_avg_sq collapsing to code 0 (the
    update then divides by eps); it is not a quality claim."""
    n, steps = 4096, 300
    rng = np.random.default_rng(0)
    hess = np.exp(rng.uniform(-3, 3, n)).astype(np.float32)
    target = rng.standard_normal(n).astype(np.float32)
    noise = np.random.default_rng(1)
    h64 = hess.astype(np.float64)
    loss = lambda p: float(0.5 * np.sum(h64 * (p - target) ** 2.0))  # noqa: E731
    p32 = np.zeros(n, np.float32)
    m32, v32 = np.zeros(n, np.float32), np.zeros(n, np.float32)
    p8 = np.zeros(n, np.float32)
    s8 = list(ref.zero_state(n, 0) + ref.zero_state(n, 1))
    s8 = [s8[0], s8[2], s8[1], s8[3]]
    start = loss(p32)
    for t in range(1, steps + 1):
        h = adam_ref.hyper(1e-2, step=t)
        e = (0.1 * noise.standard_normal(n)).astype(np.float32)
        p32, m32, v32 = adam_ref.step(p32, hess * (p32 - target) + e, m32, v32, "f32", h)
        new = ref.step(p8, hess * (p8 - target) + e, *s8, h)
        p8, s8 = new[0], list(new[1:])
    f32, f8 = loss(p32), loss(p8)
    print("loss: start %.1f, f32 state %.2f, 8-bit state %.2f, ratio %.3f"
          % (start, f32, f8, f8 / f32))
    assert f32 < 0.1 * start
    assert f8 <= 1.1 * f32
