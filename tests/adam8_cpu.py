"""Test helpers of ShardedAdamOptimizer(state_bits=8): the
numpy epilogue (tests/adam8_ref.py behind collective.HipEpilogue's adam8_*
names), an in-process loopback exchange whose ranks are threads on CPU
tensors, and the small model, its gradients and its reference run that
tests/test_sharded_adam8.py and tests/test_sharded_adam8_gpu.py share."""
import threading
import traceback

import numpy as np
import torch

import adam8_ref as ref
import adam_master_ref
import cpu_epilogue
import step_gate_ref
import test_sharded_adam_gated as gated


# ---- the numpy epilogue ----------------------------------------------------------

class CpuAdam8Epilogue(gated.CpuGatedEpilogue):
    """The CPU epilogues of the other sharded Adam tests plus the 8-bit
    updates and the quantizer, from adam8_ref."""

    @staticmethod
    def _state(mc, vc, ms, vs):
        return [np.ascontiguousarray(x.numpy()).copy() for x in (mc, vc, ms, vs)]

    @staticmethod
    def _put(dst, new):
        for t, n in zip(dst, new):
            t.numpy()[...] = n

    def adam8_update_(self, params, grads, mcs, vcs, mss, vss, hypers, np_):
        for p, g, mc, vc, ms, vs, h in zip(params, grads, mcs, vcs, mss, vss, hypers):
            assert p.dtype == torch.float32 and p.numel() % 64 == 0
            new = ref.step(p.numpy().copy(), g.numpy().copy(), *self._state(mc, vc, ms, vs), h, np_)
            self._put((p, mc, vc, ms, vs), new)
        return params

    def adam8_update_gated_(self, params, grads, mcs, vcs, mss, vss, hyper, gate, states, group,
                            np_):
        g_, st = gated.read_gate(gate), gated.read_states(states)[group]
        for p, g, mc, vc, ms, vs in zip(params, grads, mcs, vcs, mss, vss):
            new = ref.step_gated(p.numpy().copy(), g.numpy().copy(), *self._state(mc, vc, ms, vs),
                                 hyper, g_, st, np_)
            self._put((p, mc, vc, ms, vs), new)
        return params

    def adam8_master_update_(self, params16, grads16, masters, mcs, vcs, mss, vss, hypers, np_):
        for p, g, w, mc, vc, ms, vs, h in zip(params16, grads16, masters, mcs, vcs, mss, vss,
                                              hypers):
            dt = cpu_epilogue._DT[p.dtype]
            new = ref.step_master(w.numpy().copy(), np.ascontiguousarray(cpu_epilogue._np(g)),
                                  *self._state(mc, vc, ms, vs), dt, h, np_)
            cpu_epilogue._np(p)[...] = new[0]
            self._put((w, mc, vc, ms, vs), new[1:])
        return params16

    def adam8_master_update_gated_(self, params16, grads16, masters, mcs, vcs, mss, vss, hyper,
                                   gate, states, group, np_):
        g_, st = gated.read_gate(gate), gated.read_states(states)[group]
        for p, g, w, mc, vc, ms, vs in zip(params16, grads16, masters, mcs, vcs, mss, vss):
            dt = cpu_epilogue._DT[p.dtype]
            new = ref.step_master_gated(w.numpy().copy(), np.ascontiguousarray(cpu_epilogue._np(g)),
                                        *self._state(mc, vc, ms, vs), dt, hyper, g_, st, np_)
            if new[0] is not None:
                cpu_epilogue._np(p)[...] = new[0]
            self._put((w, mc, vc, ms, vs), new[1:])
        return params16

    def adam8_quantize_(self, x, which, codes, scales):
        c, a = ref.quantize(x.numpy().copy(), which)
        codes.numpy()[...] = c
        scales.numpy()[...] = a
        return codes, scales

    def adam8_dequantize(self, codes, scales, which):
        return torch.from_numpy(ref.dequantize(codes.numpy().copy(), scales.numpy().copy(), which))


# ---- the in-process loopback ------------------------------------------------------

class LoopGroup:
    """`world` ranks as threads of this process; a collective hands every
    rank the ranks' tensors."""

    def __init__(self, world):
        self.world = world
        self.barrier = threading.Barrier(world)
        self.slots = [None] * world

    def all(self, rank, value):
        self.slots[rank] = value
        self.barrier.wait(60)
        out = list(self.slots)
        self.barrier.wait(60)
        return out


class LoopExchange:
    """The methods of collective.Exchange a sharded step with its update
    outside the exchange uses, over a LoopGroup: the gradients' shards are
    folded in rank order with the / world (the epilogue's fold_), as the
    exchange's all-to-all path does."""

    def __init__(self, group, rank, epilogue):
        self.group, self.rank, self.world = group, rank, group.world
        self.epilogue = epilogue
        self._ws = {}

    def _shard(self, key, i, like, q):
        t = self._ws.get((key, i))
        if t is None:
            t = self._ws[(key, i)] = torch.zeros(q, dtype=like.dtype)
        return t

    def grad_shards_(self, grad_buckets, key):
        grads = list(grad_buckets)
        if self.world == 1:
            return grads
        return [self._shard(key, i, g, g.numel() // self.world) for i, g in enumerate(grads)]

    def reduce_shards_(self, grad_buckets, key):
        grads = list(grad_buckets)
        if self.world == 1:
            return 1
        everyone = self.group.all(self.rank, grads)
        shards = self.grad_shards_(grads, key)
        for i, s in enumerate(shards):
            q = s.numel()
            parts = [everyone[r][i][self.rank * q:(self.rank + 1) * q].clone()
                     for r in range(self.world)]
            self.epilogue.fold_(parts, s, 0, self.world)
        self.group.all(self.rank, None)  # nobody overwrites a bucket still being read
        return 0

    def gather_params_(self, param_buckets):
        params = list(param_buckets)
        if self.world == 1:
            return params
        q = [p.numel() // self.world for p in params]
        mine = [p[self.rank * n:(self.rank + 1) * n].clone() for p, n in zip(params, q)]
        everyone = self.group.all(self.rank, mine)
        for i, (p, n) in enumerate(zip(params, q)):
            for r in range(self.world):
                p[r * n:(r + 1) * n].copy_(everyone[r][i])
        return params

    def gather_doubles_(self, send, recv):
        everyone = self.group.all(self.rank, send.clone())
        recv.copy_(torch.cat(everyone))
        return recv

    def all_reduce_(self, buckets, op="sum", average=False):
        assert op == "sum" and not average
        everyone = self.group.all(self.rank, [b.clone() for b in buckets])
        for i, b in enumerate(buckets):
            b.copy_(sum(everyone[r][i] for r in range(self.world)))
        return buckets

    # only looked up when the optimizer is made: every group here is 8-bit
    def adam_step_(self, *a):
        raise NotImplementedError

    adam_master_step_ = adam_gated_step_ = adam_step_


def loop_ranks(world, body, epilogue=CpuAdam8Epilogue):
    """body(rank, exchange) on `world` threads; the first failure is re-raised."""
    group = LoopGroup(world)
    errs = []

    def run(r):
        try:
            body(r, LoopExchange(group, r, epilogue()))
        except BaseException:
            errs.append("rank %d: %s" % (r, traceback.format_exc()))
            group.barrier.abort()

    ts = [threading.Thread(target=run, args=(r,)) for r in range(world)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(120)
    assert not errs, "\n".join(errs)
    assert not any(t.is_alive() for t in ts), "a rank did not finish"


# ---- the model ---------------------------------------------------------------------
#
# Two layers (weight and bias each) and an empty tensor in buckets of 1500
# elements, every bucket ending in padding. The ranks' gradients are a base, the
# same for every world, plus offsets that cancel over the ranks; all are
# multiples of 3/2, so every sum, average and sum of squares is exact in any
# order: every world sees the same averaged gradient, bit for bit. Step BAD of
# a `bad` run carries one inf on the last rank.

NUMELS = [1000, 5, 0, 1031, 7]
HYPER = {"lr": 0.05, "weight_decay": 1e-2, "betas": (0.9, 0.999), "eps": 1e-8}
BUCKET_ELTS = 1500
STEPS, BAD = 5, 1
GATE = {"max_grad_norm": 40.0, "loss_scale": {"init_scale": 8.0, "growth_interval": 2}}
KINDS = ("f32", "bf16", "f16")
_TORCH = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}


def narrow(x, kind):
    return np.asarray(x, np.float32) if kind == "f32" else adam_master_ref.narrow(x, kind)


def widen(a, kind):
    return np.asarray(a, np.float32) if kind == "f32" else adam_master_ref.widen(a, kind)


def model_arrays(kind, seed=3):
    rng = np.random.default_rng(seed)
    return [narrow(rng.standard_normal(n).astype(np.float32), kind) for n in NUMELS]


def grad_arrays(world, step, bad=False, seed=11):
    """[rank][param], float32 values (exact in every kind)."""
    rng = np.random.default_rng(seed + 100 * step)
    base = [(rng.integers(-32, 33, n) * 1.5).astype(np.float32) for n in NUMELS]
    out = [[b.copy() for b in base] for _ in range(world)]
    for r in range(0, world - 1, 2):  # pairs of ranks whose offsets cancel
        for j, n in enumerate(NUMELS):
            d = (rng.integers(-8, 9, n) * 1.5).astype(np.float32)
            out[r][j] += d
            out[r + 1][j] -= d
    if bad and step == BAD:
        out[world - 1][3][17] = np.inf
    return out


def to_torch(a, kind):
    a = np.ascontiguousarray(a)
    if kind == "bf16":
        return torch.from_numpy(a.view(np.int16).copy()).view(torch.bfloat16)
    return torch.from_numpy(a.copy())


def to_numpy(t):
    t = t.detach().cpu().contiguous()
    if t.dtype == torch.bfloat16:
        return t.view(torch.int16).numpy().view(np.uint16).copy()
    return t.numpy().copy()


def make_optimizer(exchange, kind, device="cpu", gate=False, arrays=None):
    from kungfu_amd.optimizers import ShardedAdamOptimizer
    arrays = model_arrays(kind) if arrays is None else arrays
    ps = [torch.nn.Parameter(to_torch(a, kind).to(device)) for a in arrays]
    opt = ShardedAdamOptimizer(torch.optim.AdamW(ps, **HYPER), exchange=exchange,
                               bucket_bytes=BUCKET_ELTS * ps[0].element_size(), state_bits=8,
                               master_weights=kind != "f32", **(GATE if gate else {}))
    return ps, opt


def run_steps(ps, opt, kind, world, rank, device="cpu", first=0, steps=STEPS, gate=False):
    """The lr is halved after every step; under a gate the gradients carry the
    loss scale (a power of two) and step BAD an inf."""
    for s in range(first, first + steps):
        scale = np.float32(opt.loss_scale_value()) if gate else np.float32(1)
        for p, g in zip(ps, grad_arrays(world, s, gate)[rank]):
            p.grad = to_torch(narrow(g * scale, kind), kind).to(device)
        opt.step()
        for g in opt.param_groups:
            g["lr"] = g["lr"] * 0.5


def bucket_layout(kind):
    """[[tensor indices of bucket b]]: GradBuckets' greedy grouping, which does
    not depend on the world."""
    from kungfu_amd.collective import GradBuckets
    return GradBuckets._groups_greedy(NUMELS, BUCKET_ELTS)


_REFERENCE = {}


def reference_run(kind, steps=STEPS, gate=False):
    """The model after `steps` steps by adam8_ref on the unsharded buckets,
    each padded with zeros to a multiple of 64 elements (the padding of any
    world adds only blocks of zeros, which stay zeros). Computed once per case
    and shared; callers leave it unchanged."""
    key = (kind, steps, gate)
    if key in _REFERENCE:
        return _REFERENCE[key]
    layout = bucket_layout(kind)
    arrs = model_arrays(kind)

    def bucket(idx, arrays, dtype=np.float32):
        cat = np.concatenate([np.asarray(arrays[t], dtype) for t in idx])
        return np.concatenate([cat, np.zeros(-cat.size % 64, dtype)])

    w = [bucket(idx, [widen(a, kind) for a in arrs]) for idx in layout]
    state = [ref.zero_state(b.size, ref.SIGNED) + ref.zero_state(b.size, ref.UNSIGNED) for b in w]
    state = [(mc, vc, ms, vs) for mc, ms, vc, vs in state]
    p16 = [narrow(b, kind) for b in w]
    g_ = step_gate_ref.new_gate(GATE["loss_scale"]["init_scale"])
    st = [step_gate_ref.new_state(betas=HYPER["betas"])]
    lr, applied = HYPER["lr"], 0
    for s in range(steps):
        scale = np.float32(g_["loss_scale"]) if gate else np.float32(1)
        gr = grad_arrays(1, s, gate)[0]
        gb = [bucket(idx, [g * scale for g in gr]) for idx in layout]
        h = dict(HYPER, lr=lr, decoupled=True, step=applied + 1)
        if gate:
            sq = step_gate_ref.sum_sq(gb)
            step_gate_ref.gate_update([[sq]], [1], [h], st, g_, max_norm=GATE["max_grad_norm"],
                                      growth_factor=2.0, backoff_factor=0.5,
                                      growth_interval=GATE["loss_scale"]["growth_interval"])
        for b in range(len(layout)):
            g = narrow(gb[b], kind)
            if kind == "f32":
                new = ref.step_gated(w[b], g, *state[b], h, g_, st[0], 1) if gate else \
                    ref.step(w[b], g, *state[b], h, 1)
                w[b], state[b] = new[0], new[1:]
                p16[b] = w[b]
            else:
                new = ref.step_master_gated(w[b], g, *state[b], kind, h, g_, st[0], 1) if gate \
                    else ref.step_master(w[b], g, *state[b], kind, h, 1)
                if new[0] is not None:
                    p16[b] = new[0]
                w[b], state[b] = new[1], new[2:]
        if not (gate and g_["skip"]):
            applied += 1
        lr *= 0.5

    def split(buckets):
        out = [None] * len(NUMELS)
        for idx, b in zip(layout, buckets):
            off = 0
            for t in idx:
                out[t] = b[off:off + NUMELS[t]].copy()
                off += NUMELS[t]
        return out

    _REFERENCE[key] = {
        "p": split(p16), "master": split(w), "applied": applied, "gate": dict(g_),
        "m": split([ref.dequantize(s[0], s[2], ref.SIGNED) for s in state]),
        "v": split([ref.dequantize(s[1], s[3], ref.UNSIGNED) for s in state])}
    return _REFERENCE[key]


def snapshot(ps, opt):
    """(parameter bits, {index: state_buffers entry as numpy}) of this rank."""
    sb = opt.state_buffers()
    state = {}
    for j, p in enumerate(ps):
        if p in sb:
            state[j] = {k: (to_numpy(x) if isinstance(x, torch.Tensor) else x)
                        for k, x in sb[p].items()}
    return [to_numpy(p) for p in ps], state


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def check_against_reference(ps, opt, want, kind):
    got_p, got = snapshot(ps, opt)
    assert set(got) == {j for j, n in enumerate(NUMELS) if n}
    for j, p in enumerate(got_p):
        assert same_bits(p, want["p"][j]), ("param", j)
        if not NUMELS[j]:
            continue
        assert got[j]["step"] == want["applied"]
        assert got[j]["exp_avg"].dtype == np.float32
        assert same_bits(got[j]["exp_avg"].reshape(-1), want["m"][j]), ("exp_avg", j)
        assert same_bits(got[j]["exp_avg_sq"].reshape(-1), want["v"][j]), ("exp_avg_sq", j)
        assert ("master" in got[j]) == (kind != "f32")
        if kind != "f32":
            assert same_bits(got[j]["master"].reshape(-1), want["master"][j]), ("master", j)
    return got_p, got


def load_snapshot(ps, opt, state, device="cpu"):
    opt.load_state_buffers({ps[j]: {k: (torch.from_numpy(x).to(device)
                                        if isinstance(x, np.ndarray) else x)
                                    for k, x in e.items()} for j, e in state.items()})
