"""The gated chains that tests/test_capture_replay_gpu.py captures into a graph
and replays, restated from the references alone: six steps of a world-1 gated
Adam step (every gated update entry) and of a gated LAMB step, with a dynamic
loss scale, clipping and one overflow. The builders here are the GPU file's:
both see the same inputs. The tests below show that those inputs are worth the
comparison: the scale grows and backs off, exactly one step is skipped,
clipping is on for some applied steps and off for others, and every buffer
moves.

Gradients are multiples of 1/4 in [-8, 8] times a power of two (the step's
amplitude times the loss scale in force), as tests/test_sharded_adam_gated_gpu.py
draws them: every square and every partial sum of squares is exact in fp64, so
the sum the device's norm pass gives is the exact one, whatever its order."""
import math

import numpy as np
import pytest

import adam8_ref
import adam_master_ref
import adam_ref
import adam_sr_ref
import lamb_gated_ref
import lamb_ref
import monitor_ref
import step_gate_ref
import test_sharded_adam as adam_cpu
import test_sharded_adam8 as adam8_cpu
import test_sharded_adam_master as master_cpu
import test_sharded_adam_sr as sr_cpu
import test_sharded_lamb as lamb_cpu

STEPS, BAD = 6, 3                 # step index BAD carries one +inf
SCALE0, MAX_NORM = 1024.0, 1.0
RULE = dict(growth_factor=2.0, backoff_factor=0.5, growth_interval=2)
# The unscaled gradients are AMPS[s] * (k / 4), |k| <= 32. A chain has at least
# 2000 elements and E[(k / 4)^2] = 22, so at amplitude 1 the norm is above 200
# (clipped at MAX_NORM = 1), and with at most 20000 elements it is below
# 2^-12 * 8 * sqrt(20000) = 0.28 at amplitude 2^-12 (not clipped).
AMPS = (1.0, 2.0 ** -12, 1.0, 1.0, 2.0 ** -12, 1.0)
SCALES_IN_FORCE = [1024.0, 1024.0, 2048.0, 2048.0, 1024.0, 1024.0]
SCALES_AFTER = [1024.0, 2048.0, 2048.0, 1024.0, 1024.0, 2048.0]
GROUPS = [{"lr": 1e-3, "betas": (0.9, 0.999)}, {"lr": 3e-2, "betas": (0.8, 0.95)}]
SR_KEY = 0x9ABCDEF1
TRUST_CLIP = 10.0

_ADAM_TILE = adam_cpu.BLOCK * adam_cpu.UNROLL          # 16-byte vectors per tile
_ONES = lambda seg: (1,) * (seg + 8)                   # noqa: E731

# name -> (kind, the 16-bit or plain dtype, group, sizes). Every layout has an
# empty segment, a ragged last tile and more non-empty segments than one
# launch's table holds (SEG[name]).
ADAM_CHAINS = {
    "adam-f32": ("plain", "f32", 0, (0, 1, 3, 1021, _ADAM_TILE * 4 + 5) + _ONES(adam_cpu.ADAM_SEG)),
    "adam-bf16": ("plain", "bf16", 1, (0, 1, 3, 1021, _ADAM_TILE * 8 + 9) + _ONES(adam_cpu.ADAM_SEG)),
    "master-f16": ("master", "f16", 0, (0, 1, 3, 5, 6, 1021, 4096 + 7) + _ONES(master_cpu.MASTER_SEG)),
    "sr": ("sr", "bf16", 1, (0, 1, 7, 8, 9, 1023, 8192 + 13) + _ONES(sr_cpu.SR_SEG)),
    "adam8": ("adam8", "f32", 0, (0, 64, 64 * 15, adam8_cpu.TILE + 64, 2 * adam8_cpu.TILE + 64 * 3)
              + (64,) * (adam8_cpu.ADAM8_SEG + 8)),
    "adam8-master-f16": ("adam8m", "f16", 1,
                         (0, 64, 64 * 15, adam8_cpu.TILE + 64, 2 * adam8_cpu.TILE + 64 * 3)
                         + (64,) * (adam8_cpu.ADAM8_SEG + 8)),
}
SEG = {"adam-f32": adam_cpu.ADAM_SEG, "adam-bf16": adam_cpu.ADAM_SEG,
       "master-f16": master_cpu.MASTER_SEG, "sr": sr_cpu.SR_SEG, "adam8": adam8_cpu.ADAM8_SEG,
       "adam8-master-f16": adam8_cpu.ADAM8_SEG,
       "lamb-f32": lamb_cpu.LAMB_SEG, "lamb-master-bf16": lamb_cpu.LAMB_MASTER_SEG}
# elements per tile of each chain's update kernel (tests/large_launch.py UPDATE_KERNELS)
TILE = {"adam-f32": 4 * _ADAM_TILE, "adam-bf16": 8 * _ADAM_TILE, "master-f16": 4096, "sr": 8192,
        "adam8": adam8_cpu.TILE, "adam8-master-f16": adam8_cpu.TILE, "lamb-f32": 4096,
        "lamb-master-bf16": 4096}
# The tables of the gated entries in their argument order; "g" is the gradient.
COLS = {"plain": ("p", "g", "m", "v"), "master": ("p16", "g", "w", "m", "v"),
        "sr": ("p", "g", "m", "v"), "adam8": ("p", "g", "mc", "vc", "ms", "vs"),
        "adam8m": ("p16", "g", "w", "mc", "vc", "ms", "vs")}

# name -> (the gradients' dtype, sizes); tensor t belongs to group LAMB_GROUP_OF(t)
LAMB_CHAINS = {
    "lamb-f32": ("f32", (0, 1, 7, 9, 4096, 4097 + 2048) + _ONES(lamb_cpu.LAMB_SEG)),
    "lamb-master-bf16": ("bf16", (0, 1, 7, 9, 4096, 4097 + 2048) + _ONES(lamb_cpu.LAMB_MASTER_SEG)),
}


def lamb_group_of(t):
    """Tensors 1, 3 and 4 are group 1's: group 0 keeps more non-empty tensors
    than one launch's table, and both groups have a tensor of more than a tile."""
    return 1 if t in (1, 3, 4) else 0


def hyper(group):
    """What a gated update entry is given for `group`: no step."""
    return dict(GROUPS[group], eps=1e-8, weight_decay=1e-2, decoupled=group == 0)


def lamb_hyper(group):
    return dict(GROUPS[group], eps=1e-6, weight_decay=1e-2 if group == 0 else 0.0,
                adapt=True)


def _seed(name):
    return sum(ord(c) * (i + 1) for i, c in enumerate(name))


def store16(x, dt):
    """f32 values -> the 16-bit storage of the references: bf16 as uint16 bit
    patterns, f16 as numpy's float16."""
    x = np.asarray(x, np.float32)
    return adam_ref.f32_to_bf16_bits(x) if dt == "bf16" else adam_master_ref.narrow(x, "f16")


def store(x, dt):
    return np.asarray(x, np.float32) if dt == "f32" else store16(x, dt)


def widen(a, dt):
    if dt == "f32":
        return np.asarray(a, np.float32)
    return adam_ref.bf16_bits_to_f32(a) if dt == "bf16" else np.asarray(a).astype(np.float32)


def grads(name, sizes, dt, s, scale):
    """Step s's gradients, already multiplied by the loss scale in force."""
    out = []
    for i, n in enumerate(sizes):
        k = np.random.default_rng(_seed(name) + 1000 * s + i).integers(-32, 33, n)
        out.append((k / 4.0 * (AMPS[s] * scale)).astype(np.float32))
    if s == BAD:
        big = max(range(len(sizes)), key=lambda i: sizes[i])
        out[big][sizes[big] // 2] = np.inf
    got = [store(g, dt) for g in out]
    for a, b in zip(out, got):  # the grid is exact in every storage type
        assert np.array_equal(widen(b, dt), a)
    return got


def exact_sq(gs, dt):
    """The exact sum of squares of a step's gradients (inf on the bad step)."""
    with np.errstate(over="ignore", invalid="ignore"):
        return math.fsum(monitor_ref.exact_sq(g, {"f32": "f32", "bf16": "bf16", "f16": "f16"}[dt])
                         for g in gs if g.size)


def _moments(rng, n):
    m = (0.1 * rng.standard_normal(n)).astype(np.float32)
    v = np.square(0.1 * rng.standard_normal(n)).astype(np.float32)
    return m, v


def adam_initial(name):
    """The chain's buffers before the first step: {column: [array per segment]}."""
    kind, dt, _, sizes = ADAM_CHAINS[name]
    cols = {c: [] for c in COLS[kind] if c != "g"}
    for i, n in enumerate(sizes):
        rng = np.random.default_rng(_seed(name) + 77 * i + 5)
        p = rng.standard_normal(n).astype(np.float32)
        m, v = _moments(rng, n)
        if kind in ("plain", "sr"):
            new = {"p": store(p, dt), "m": store(m, dt), "v": store(v, dt)}
        elif kind == "master":
            new = {"p16": store16(p, dt), "w": p, "m": m, "v": v}
        else:
            mc, ms = adam8_ref.quantize(m, adam8_ref.SIGNED)
            vc, vs = adam8_ref.quantize(v, adam8_ref.UNSIGNED)
            new = {"p": p, "mc": mc, "vc": vc, "ms": ms, "vs": vs}
            if kind == "adam8m":
                new["p16"], new["w"] = store16(new.pop("p"), dt), p
        for c, a in new.items():
            cols[c].append(a)
    return cols


def sr_words(name):
    """(bases, stream words) of the SR chain's segments."""
    n = len(ADAM_CHAINS[name][3])
    return ([8 * (1000 * i + 3) for i in range(n)],
            [(0x01234567 * (i + 1)) & 0xFFFFFFFF for i in range(n)])


def adam_advance(name, cols, gs, gate, state):
    """One gated update of every segment: the new {column: [array]}."""
    kind, dt, group, sizes = ADAM_CHAINS[name]
    h = hyper(group)
    out = {c: [] for c in cols}
    bases, words = sr_words(name)
    for i in range(len(sizes)):
        a = {c: cols[c][i] for c in cols}
        if kind == "plain":
            new = dict(zip("pmv", step_gate_ref.update(a["p"], gs[i], a["m"], a["v"], dt, h, gate,
                                                       state)))
        elif kind == "sr":
            new = dict(zip("pmv", adam_sr_ref.step_gated(a["p"], gs[i], a["m"], a["v"], h, gate,
                                                         state, bases[i], words[i], SR_KEY)))
        elif kind == "master":
            new = dict(zip(("p16", "w", "m", "v"), step_gate_ref.update_master(
                a["w"], gs[i], a["m"], a["v"], dt, h, gate, state)))
        elif kind == "adam8":
            new = dict(zip(("p", "mc", "vc", "ms", "vs"), adam8_ref.step_gated(
                a["p"], gs[i], a["mc"], a["vc"], a["ms"], a["vs"], h, gate, state)))
        else:
            new = dict(zip(("p16", "w", "mc", "vc", "ms", "vs"), adam8_ref.step_master_gated(
                a["w"], gs[i], a["mc"], a["vc"], a["ms"], a["vs"], dt, h, gate, state)))
        for c in cols:
            x = a[c] if new[c] is None else new[c]  # a skipped step writes no 16-bit parameters
            out[c].append(np.ascontiguousarray(x, a[c].dtype))
    return out


class AdamChain:
    """The reference's side of one chain: `scale` is the loss scale in force,
    step(gs, sq) takes a step's gradients and their sum of squares."""

    def __init__(self, name):
        self.name = name
        self.kind, self.dt, self.group, self.sizes = ADAM_CHAINS[name]
        self.cols = adam_initial(name)
        self.gate = step_gate_ref.new_gate(SCALE0)
        self.states = [step_gate_ref.new_state() for _ in GROUPS]
        self.s = 0

    @property
    def scale(self):
        return float(self.gate["loss_scale"])

    def grads(self):
        return grads(self.name, self.sizes, self.dt, self.s, self.scale)

    def step(self, gs, sq):
        step_gate_ref.gate_update([[sq]], [0], GROUPS, self.states, self.gate, max_norm=MAX_NORM,
                                  **RULE)
        self.cols = adam_advance(self.name, self.cols, gs, self.gate, self.states[self.group])
        self.s += 1


class LambChain:
    """The reference's side of a gated LAMB chain over T tensors of one piece
    each. step(gs, sq, sums): sums is None (lamb_ref.sq_sum stands in) or the
    2T sums of squares of the parameters and the updates."""

    def __init__(self, name):
        self.name = name
        self.dt, self.sizes = LAMB_CHAINS[name]
        self.master = self.dt != "f32"
        self.T = len(self.sizes)
        self.group_of = [lamb_group_of(t) for t in range(self.T)]
        self.hs = [lamb_hyper(g) for g in self.group_of]
        cols = {c: [] for c in ("p", "m", "v", "u")}
        for i, n in enumerate(self.sizes):
            rng = np.random.default_rng(_seed(name) + 77 * i + 5)
            cols["p"].append(rng.standard_normal(n).astype(np.float32))
            m, v = _moments(rng, n)
            cols["m"].append(m)
            cols["v"].append(v)
            cols["u"].append(np.full(n, 7.0, np.float32))
        if self.master:
            cols["p16"] = [lamb_ref.narrow16(p, self.dt) for p in cols["p"]]
        self.cols = cols
        self.nlr, self.ratio = np.full(self.T, -3.0), np.full(self.T, 5.0)
        self.gate = lamb_gated_ref.new_gate(SCALE0)
        self.states = [lamb_gated_ref.new_state() for _ in GROUPS]
        self.s = 0

    @property
    def scale(self):
        return float(self.gate["loss_scale"])

    def grads(self):
        return grads(self.name, self.sizes, self.dt, self.s, self.scale)

    def step(self, gs, sq, sums=None):
        lamb_gated_ref.verdict([[sq]], [0], GROUPS, self.states, self.gate, max_norm=MAX_NORM,
                               **RULE)
        c = self.cols
        cuts = [[(0, n)] for n in self.sizes]
        ps, ms, vs, us, self.nlr, self.ratio = lamb_gated_ref.step_tensors(
            c["p"], [widen(g, self.dt) for g in gs], c["m"], c["v"], c["u"], "f32", self.hs,
            [self.states[g] for g in self.group_of], self.gate, cuts, self.nlr, self.ratio,
            trust_clip=TRUST_CLIP, sums=None if sums is None else np.asarray(sums).reshape(1, -1))
        c["p"], c["m"], c["v"], c["u"] = ps, ms, vs, us
        if self.master and not self.gate["skip"]:
            c["p16"] = [lamb_ref.narrow16(p, self.dt) for p in ps]
        self.s += 1


def _snapshot(chain):
    out = {c: [a.copy() for a in col] for c, col in chain.cols.items()}
    if isinstance(chain, LambChain):
        out["nlr"], out["ratio"] = [chain.nlr.copy()], [chain.ratio.copy()]
    return out


def _run(chain):
    """Six steps on the exact sums: per step (scale in force, gate, states,
    buffers)."""
    out = []
    for _ in range(STEPS):
        scale, gs = chain.scale, chain.grads()
        chain.step(gs, exact_sq(gs, chain.dt))
        out.append((scale, dict(chain.gate), [dict(st) for st in chain.states], _snapshot(chain)))
    return out


def _make(name):
    return AdamChain(name) if name in ADAM_CHAINS else LambChain(name)


@pytest.mark.parametrize("name", list(ADAM_CHAINS) + list(LAMB_CHAINS))
def test_layout_reaches_the_branches(name):
    sizes = (ADAM_CHAINS[name][3] if name in ADAM_CHAINS else LAMB_CHAINS[name][1])
    assert 0 in sizes
    assert sum(1 for n in sizes if n) > SEG[name]          # a call is at least two launches
    assert 2000 <= sum(sizes) <= 20000                      # what AMPS was chosen for
    if name in LAMB_CHAINS:
        mine = [n for t, n in enumerate(sizes) if lamb_group_of(t) == 0 and n]
        assert len(mine) > SEG[name]
        assert any(n for t, n in enumerate(sizes) if lamb_group_of(t) == 1)
    assert any(n > TILE[name] and n % TILE[name] for n in sizes)  # a ragged last tile
    assert GROUPS[0]["betas"] != GROUPS[1]["betas"] and GROUPS[0]["lr"] != GROUPS[1]["lr"]
    assert {g for _, _, g, _ in ADAM_CHAINS.values()} == {0, 1}


@pytest.mark.parametrize("name", list(ADAM_CHAINS) + list(LAMB_CHAINS))
def test_schedule_is_worth_the_comparison(name):
    chain = _make(name)
    first = _snapshot(chain)
    steps = _run(chain)
    assert [s[0] for s in steps] == SCALES_IN_FORCE
    assert [float(s[1]["loss_scale"]) for s in steps] == SCALES_AFTER
    assert [s[1]["skip"] for s in steps] == [int(i == BAD) for i in range(STEPS)]
    assert steps[-1][1]["skipped"] == 1 and steps[-1][1]["applied"] == STEPS - 1
    # grad_mul is clip / scale: clipped where it is below 1 / scale
    clipped = [float(s[1]["grad_mul"]) * s[0] < 1.0 for s in steps]
    applied = [i for i in range(STEPS) if i != BAD]
    assert any(clipped[i] for i in applied) and any(not clipped[i] for i in applied)
    assert [clipped[i] for i in applied] == [AMPS[i] == 1.0 for i in applied]
    # the skipped step moved nothing but the gate
    before, after = steps[BAD - 1], steps[BAD]
    assert before[2] == after[2]
    for c in before[3]:
        for a, b in zip(before[3][c], after[3][c]):
            assert a.tobytes() == b.tobytes(), c
    # both groups' pows advanced on the applied steps only
    for j, st in enumerate(steps[-1][2]):
        assert st["step"] == STEPS - 1
        assert st["beta1_pow"] != steps[0][2][j]["beta1_pow"]
    assert steps[-1][2][0] != steps[-1][2][1]
    # every buffer moved: at the first step and between the first and the last
    for c in first:
        was = np.concatenate([a.reshape(-1).view(np.uint8) for a in first[c]])
        one = np.concatenate([a.reshape(-1).view(np.uint8) for a in steps[0][3][c]])
        last = np.concatenate([a.reshape(-1).view(np.uint8) for a in steps[-1][3][c]])
        assert not np.array_equal(was, one), c
        assert not np.array_equal(one, last), c
