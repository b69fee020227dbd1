"""Device bucket-reduce ops on torch tensors (C-ABI B2, include/kungfu_amd.h).

Every op launches a hand-written gfx950 HIP kernel from libkungfu_amd.so on
the caller's current HIP stream (or the stream given). Tensors must be
contiguous and on the GPU; there is no CPU path — a CPU tensor or a missing
library raises.
"""
import ctypes

import torch

from . import _lib
from .base import OP, OP_NAMES, DataType

_TORCH_DTYPES = {
    torch.uint8: DataType.U8,
    torch.int8: DataType.I8,
    torch.int16: DataType.I16,
    torch.int32: DataType.I32,
    torch.int64: DataType.I64,
    torch.float16: DataType.F16,
    torch.bfloat16: DataType.BF16,
    torch.float32: DataType.F32,
    torch.float64: DataType.F64,
}
for _name, _dt in (("uint16", DataType.U16), ("uint32", DataType.U32),
                   ("uint64", DataType.U64)):
    if hasattr(torch, _name):
        _TORCH_DTYPES[getattr(torch, _name)] = _dt


def kungfu_dtype(t):
    try:
        return _TORCH_DTYPES[t.dtype]
    except KeyError:
        raise TypeError("kungfu_amd: unsupported dtype %s" % t.dtype)


# The reference's TF dtype map, as it is (tensorflow/ops.h:14-33): no fp16,
# and DT_BFLOAT16 -> KungFu_FLOAT16, so a bf16 tensor's bit patterns are
# reduced as fp16 numbers. The build's own map (kungfu_dtype) gives bf16 its
# own code and fp32-accumulated semantics; this one exists so that a caller
# that wants the reference's exact bits can ask for them (pass the code as
# `dtype` to the device ops).
TF_DTYPES = {
    "int32": DataType.I32,
    "int64": DataType.I64,
    "bfloat16": DataType.F16,
    "float32": DataType.F32,
    "float64": DataType.F64,
    "bool": DataType.BOOL,
}


def to_kungfu_type(tf_dtype):
    """ops.h:14-33 to_kungfu_type: a TF dtype name ("float32", "bfloat16", ...
    or anything with such a `name`) -> KungFu code; anything else raises, as
    the reference's `throw std::invalid_argument("unsupported dtype")`."""
    name = getattr(tf_dtype, "name", tf_dtype)
    try:
        return TF_DTYPES[name]
    except KeyError:
        raise ValueError("unsupported dtype")


def _dtype_for(t, dtype):
    """The KungFu code a device op runs with: the tensor's own, or an explicit
    one of the same element size (e.g. to_kungfu_type("bfloat16") on a bf16
    tensor, the reference's TF semantics)."""
    if dtype is None:
        return kungfu_dtype(t)
    dt = DataType(int(dtype))
    if dt.size() != t.element_size():
        raise ValueError("dtype %s does not match the tensor's %d-byte elements"
                         % (dt.name, t.element_size()))
    return dt


def _op(op):
    if op is None:
        return OP.SUM
    if isinstance(op, str):
        return OP_NAMES[op]
    return OP(op)


def _check_dev(ts):
    for t in ts:
        if not t.is_cuda:
            raise ValueError("kungfu_amd device ops need GPU tensors (got %s)"
                             % t.device)
        if not t.is_contiguous():
            raise ValueError("kungfu_amd device ops need contiguous tensors")


def _stream(stream, dev):
    s = stream if stream is not None else torch.cuda.current_stream(dev)
    return s.cuda_stream


def bucket_reduce(inputs, out=None, op="sum", stream=None, dtype=None):
    """out = inputs[0] op inputs[1] op ... (left fold, in the given order).
    `dtype`: a KungFu code to reduce with instead of the tensors' own
    (same element size)."""
    inputs = list(inputs)
    if out is None:
        out = torch.empty_like(inputs[0])
    _check_dev(inputs + [out])
    n = out.numel()
    for t in inputs:
        if t.numel() != n or t.dtype != out.dtype:
            raise ValueError("bucket_reduce: shape/dtype mismatch")
    lib = _lib.load()
    rc = lib.kf_bucket_reduce(_lib.ptr_array([t.data_ptr() for t in inputs]),
                              len(inputs), out.data_ptr(), n,
                              int(_dtype_for(out, dtype)), int(_op(op)),
                              _stream(stream, out.device))
    _lib.check(rc, "kf_bucket_reduce")
    return out


def bucket_reduce_avg(inputs, np_, out=None, stream=None):
    """out = sum(inputs) / np_ with a true division (TF's g / np)."""
    inputs = list(inputs)
    if out is None:
        out = torch.empty_like(inputs[0])
    _check_dev(inputs + [out])
    lib = _lib.load()
    rc = lib.kf_bucket_reduce_avg(
        _lib.ptr_array([t.data_ptr() for t in inputs]), len(inputs),
        out.data_ptr(), out.numel(), int(kungfu_dtype(out)), int(np_),
        _stream(stream, out.device))
    _lib.check(rc, "kf_bucket_reduce_avg")
    return out


def bucket_div_(x, np_, stream=None):
    """x /= np_ in place (the step between reduce-scatter and all-gather)."""
    _check_dev([x])
    lib = _lib.load()
    rc = lib.kf_bucket_div(x.data_ptr(), x.numel(), int(kungfu_dtype(x)),
                           int(np_), _stream(stream, x.device))
    _lib.check(rc, "kf_bucket_div")
    return x


def sma_blend_(v, summed, np_, alpha, stream=None):
    """v = (1 - alpha) * v + alpha * (summed / np_) in place (sma_sgd.py:60-65)."""
    _check_dev([v, summed])
    if v.numel() != summed.numel() or v.dtype != summed.dtype:
        raise ValueError("sma_blend_: shape/dtype mismatch")
    lib = _lib.load()
    rc = lib.kf_sma_blend(v.data_ptr(), summed.data_ptr(), v.numel(),
                          int(kungfu_dtype(v)), int(np_), float(alpha),
                          _stream(stream, v.device))
    _lib.check(rc, "kf_sma_blend")
    return v


def sma_blend_batch_(vs, sums, np_, alpha, stream=None):
    """sma_blend_ over many buckets (one dtype) in one launch per 16 of them
    (kf_sma_blend_batch); the same bits as one sma_blend_ per bucket."""
    vs, sums = list(vs), list(sums)
    if len(vs) != len(sums):
        raise ValueError("sma_blend_batch_: one sum per variable bucket")
    if not vs:
        return vs
    _check_dev(vs + sums)
    for v, s in zip(vs, sums):
        if v.numel() != s.numel() or v.dtype != vs[0].dtype or s.dtype != v.dtype:
            raise ValueError("sma_blend_batch_: shape/dtype mismatch")
    lib = _lib.load()
    cnt = (ctypes.c_size_t * len(vs))(*[v.numel() for v in vs])
    rc = lib.kf_sma_blend_batch(_lib.ptr_array([v.data_ptr() for v in vs]),
                                _lib.ptr_array([s.data_ptr() for s in sums]), cnt, len(vs),
                                int(kungfu_dtype(vs[0])), int(np_), float(alpha),
                                _stream(stream, vs[0].device))
    _lib.check(rc, "kf_sma_blend_batch")
    return vs


def sgd_update_batch_(params, grads, moms, hypers, np_=0, stream=None):
    """The SGD update of many flat segments of one float dtype in one launch
    per 32 of them (kf_sgd_update_batch, kungfu_amd/csrc/kf_sgd.hip), in
    place on params and moms:

      g = grads[b] / np_ (np_ > 0) ; g += wd * p ; m = first ? g : mu * m + (1 - dampening) * g
      g = nesterov ? g + mu * m : m ; p -= lr * g

    with torch.optim.SGD's single-tensor rounding. hypers[b] is a dict with
    lr and optionally momentum, dampening, weight_decay, nesterov, first.
    moms[b] may be None where momentum is 0 (moms itself may be None). Every
    tensor starts 16-byte aligned. grads are only read."""
    params, grads, hypers = list(params), list(grads), list(hypers)
    moms = [None] * len(params) if moms is None else list(moms)
    if not (len(params) == len(grads) == len(moms) == len(hypers)):
        raise ValueError("sgd_update_batch_: one grad, momentum and hyper per param segment")
    if not params:
        return params
    live = [m for m in moms if m is not None]
    _check_dev(params + grads + live)
    for p, g, m in zip(params, grads, moms):
        if g.numel() != p.numel() or g.dtype != params[0].dtype or p.dtype != g.dtype or \
                (m is not None and (m.numel() != p.numel() or m.dtype != p.dtype)):
            raise ValueError("sgd_update_batch_: shape/dtype mismatch")
    lib = _lib.load()
    cnt = (ctypes.c_size_t * len(params))(*[p.numel() for p in params])
    rc = lib.kf_sgd_update_batch(_lib.ptr_array([p.data_ptr() for p in params]),
                                 _lib.ptr_array([g.data_ptr() for g in grads]),
                                 _lib.ptr_array([0 if m is None else m.data_ptr() for m in moms]),
                                 cnt, len(params), int(kungfu_dtype(params[0])), int(np_),
                                 _lib.sgd_hyper_array(hypers), _stream(stream, params[0].device))
    _lib.check(rc, "kf_sgd_update_batch", source="")
    return params


# -- the batched Adam-family updates: one implementation -------

ADAM8_BLOCK = 64                 # elements per quantization block
_HALF = (torch.bfloat16, torch.float16)


# What a table's tensor must be beside the lead tensor p of its segment: (its
# dtype, None for p's; how many of p's elements one of its elements stands for).
_same, _f32, _u8 = (None, 1), (torch.float32, 1), (torch.uint8, 1)
_scale = (torch.float32, ADAM8_BLOCK)


class _Update:
    """One wrapper's row: its name, the C entry (`fn` once it has been looked
    up), the rules of the tables after the lead one, and its refusals' words."""

    def __init__(self, name, rules, words, mismatch="shape/dtype mismatch", lead=None,
                 lead_words=None, ret=0, hypers_first=False, gate_last=False):
        self.name, self.entry, self.fn = name, "kf_" + name.rstrip("_"), None
        self.rules, self.words, self.mismatch = rules, words, mismatch
        self.lead, self.lead_words = lead, lead_words  # None: the dtype is the C entry's check
        self.ret = ret                                 # the table the wrapper returns
        self.hypers_first = hypers_first               # the hypers are counted on their own, first
        self.gate_last = gate_last                     # the gate is looked at after the tables


_ADAM8 = (_same, _u8, _u8, _scale, _scale)
_ADAM8_MASTER = (_same, _f32, _u8, _u8, _scale, _scale)
_MISMATCH_SR = "bf16 tensors of one shape per segment"
_MISMATCH_8 = ("shape/dtype mismatch (uint8 codes of the parameters' length, one f32 scale per 64 "
               "elements)")
_WORDS_SR = "one grad, exp_avg, exp_avg_sq, base and stream word per param segment"
_WORDS_8 = "one grad, codes and scales tensor of each state per param segment"
_WORDS_8_MASTER = "one grad, codes and scales tensor of each state and a master per param segment"
# One row per wrapper, bound once: _<wrapper> is the row of <wrapper>_.
_adam_update_batch = _Update("adam_update_batch_", (_same,) * 3,
    "one grad, exp_avg, exp_avg_sq and hyper per param segment")
_adam_update_batch_gated = _Update("adam_update_batch_gated_", (_same,) * 3,
    "one grad, exp_avg and exp_avg_sq per param segment")
_adam_master_update_batch = _Update("adam_master_update_batch_", (_same, _f32, _f32, _f32),
    "one grad, master, exp_avg, exp_avg_sq and hyper per param segment",
    lead=_HALF, lead_words="bf16 or f16 parameters")
_adam_master_update_batch_gated = _Update(
    "adam_master_update_batch_gated_", (_same, _f32, _f32, _f32),
    "one grad, master, exp_avg and exp_avg_sq per param segment",
    lead=_HALF, lead_words="bf16 or f16 parameters")
_adam_sr_update_batch = _Update("adam_sr_update_batch_", (_same,) * 3, _WORDS_SR, _MISMATCH_SR,
    lead=(torch.bfloat16,), lead_words=_MISMATCH_SR, hypers_first=True)
_adam_sr_update_batch_gated = _Update(
    "adam_sr_update_batch_gated_", (_same,) * 3, _WORDS_SR, _MISMATCH_SR,
    lead=(torch.bfloat16,), lead_words=_MISMATCH_SR, gate_last=True)
_adam8_update_batch = _Update("adam8_update_batch_", _ADAM8, _WORDS_8, _MISMATCH_8,
    lead=(torch.float32,), lead_words="torch.float32 parameters", hypers_first=True)
_adam8_update_batch_gated = _Update("adam8_update_batch_gated_", _ADAM8, _WORDS_8, _MISMATCH_8,
    lead=(torch.float32,), lead_words="torch.float32 parameters", gate_last=True)
_adam8_master_update_batch = _Update(
    "adam8_master_update_batch_", _ADAM8_MASTER, _WORDS_8_MASTER, _MISMATCH_8,
    lead=_HALF, lead_words="torch.bfloat16 or torch.float16 parameters", hypers_first=True)
_adam8_master_update_batch_gated = _Update(
    "adam8_master_update_batch_gated_", _ADAM8_MASTER, _WORDS_8_MASTER, _MISMATCH_8,
    lead=_HALF, lead_words="torch.bfloat16 or torch.float16 parameters", gate_last=True)
_lamb_moments_batch = _Update("lamb_moments_batch_", (_same,) * 4,
    "one grad, exp_avg, exp_avg_sq, update and hyper per param segment", ret=4)
_lamb_moments_batch_gated = _Update("lamb_moments_batch_gated_", (_same,) * 4,
    "one grad, exp_avg, exp_avg_sq and update per param segment", ret=4)
_lamb_master_moments_batch = _Update("lamb_master_moments_batch_", (_f32,) * 4,
    "one master, exp_avg, exp_avg_sq, update and hyper per gradient segment",
    lead=_HALF, lead_words="bf16 or f16 gradients", ret=4)
_lamb_master_moments_batch_gated = _Update("lamb_master_moments_batch_gated_", (_f32,) * 4,
    "one master, exp_avg, exp_avg_sq and update per gradient segment",
    lead=_HALF, lead_words="bf16 or f16 gradients", ret=4)


def _update_batch(row, tables, hyper, gated, np_, stream, sr=None):
    """The body of every wrapper that has an _Update row. tables: the tensor tables, the
    lead one first; hyper: one dict per segment, or with gated = (gate, states,
    group) the one dict; sr: (bases, streams, key). Checks, then the C call."""
    name = row.name
    tables = [list(t) for t in tables]
    lead = tables[0]
    nb = len(lead)
    fits = True
    for t in tables:
        fits = fits and len(t) == nb
    if gated is None:
        hyper = list(hyper)
        if len(hyper) != nb:
            if row.hypers_first:
                raise ValueError("%s: one hyper per param segment" % name)
            fits = False
    if sr is not None:
        bases, streams = [int(b) for b in sr[0]], [int(x) for x in sr[1]]
        fits = fits and len(bases) == nb == len(streams)
    if not fits:
        raise ValueError("%s: %s" % (name, row.words))
    if sr is not None:
        key = int(sr[2])
        if not 0 <= key < 1 << 32 or any(not 0 <= x < 1 << 32 for x in streams) or \
                any(not 0 <= b < 1 << 64 for b in bases):
            raise ValueError("%s: key and stream words are 32-bit, bases 64-bit unsigned" % name)
    if not lead:
        return tables[row.ret]
    for ts in tables:
        _check_dev(ts)
    if gated is not None and not row.gate_last:
        _check_gate(gated[0], gated[1], int(gated[2]) + 1)
    if row.lead is not None and lead[0].dtype not in row.lead:
        raise ValueError("%s: %s" % (name, row.lead_words))
    first, counts, bad = lead[0].dtype, [p.numel() for p in lead], False
    for p in lead:
        bad = bad or p.dtype != first
    for (dtype, k), ts in zip(row.rules, tables[1:]):
        dtype = dtype or first
        for t, n in zip(ts, counts):
            bad = bad or t.dtype != dtype or t.numel() * k != n
    if bad:
        raise ValueError("%s: %s" % (name, row.mismatch))
    if gated is not None and row.gate_last:
        _check_gate(gated[0], gated[1], int(gated[2]) + 1)
    args = [_lib.ptr_array([t.data_ptr() for t in ts]) for ts in tables]
    args.append((ctypes.c_size_t * nb)(*counts))
    if sr is not None:
        args += [(ctypes.c_uint64 * nb)(*bases), (ctypes.c_uint32 * nb)(*streams)]
    args += [nb, int(kungfu_dtype(lead[0])), int(np_),
             _lib.adam_hyper_array(hyper if gated is None else [dict(hyper, step=1)])]
    if sr is not None:
        args.append(key)
    if gated is not None:
        args += [gated[0].data_ptr(), _state_ptr(gated[1], gated[2])]
    if row.fn is None:
        row.fn = getattr(_lib.load(), row.entry)
    rc = row.fn(*args, _stream(stream, lead[0].device))
    _lib.check(rc, row.entry, source="")
    return tables[row.ret]


def adam_update_batch_(params, grads, exp_avgs, exp_avg_sqs, hypers, np_=0, stream=None):
    """The Adam / AdamW update of many flat segments of one dtype (f32, bf16
    or f64) in one launch per 24 of them (kf_adam_update_batch,
    kungfu_amd/csrc/kf_adam.hip), in place on params and both states:

      g = grads[b] / np_ (np_ > 0) ; L2: g += wd * p ; decoupled: p *= 1 - lr * wd
      m = b1 * m + (1 - b1) * g ; v = b2 * v + (1 - b2) * g * g
      p -= lr / (1 - b1**step) * m / (sqrt(v) / sqrt(1 - b2**step) + eps)

    rounded as include/kungfu_amd.h states. hypers[b] is a dict with lr,
    step (>= 1) and optionally betas, eps, weight_decay, decoupled. Every
    tensor starts 16-byte aligned. grads are only read."""
    return _update_batch(_adam_update_batch, (params, grads, exp_avgs, exp_avg_sqs), hypers,
                         None, np_, stream)


def adam_master_update_batch_(params16, grads16, masters, exp_avgs, exp_avg_sqs, hypers, np_=0,
                              stream=None):
    """adam_update_batch_ for bf16 or f16 parameters with fp32 master weights
    and fp32 state, one launch per 32 segments (kf_adam_master_update_batch,
    kungfu_amd/csrc/kf_adam_master.hip): the gradient is widened, the f32
    update of adam_update_batch_ runs on (masters, g, exp_avgs, exp_avg_sqs)
    in place, and params16 = masters narrowed, round-to-nearest-even, the only
    rounding to 16 bits. params16 is written, never read; grads16 only read.
    hypers[b] as adam_update_batch_ takes them. Every tensor starts 16-byte
    aligned."""
    return _update_batch(_adam_master_update_batch,
                         (params16, grads16, masters, exp_avgs, exp_avg_sqs),
                         hypers, None, np_, stream)


def new_step_gate(device, loss_scale=1.0):
    """A kf_step_gate on `device` as a uint8 tensor: zero-filled, with the
    initial loss scale (1.0 without loss scaling)."""
    import numpy as np
    a = np.zeros(1, _lib.step_gate_dtype())
    a["loss_scale"] = loss_scale
    return torch.from_numpy(a.view(np.uint8).copy()).to(device)


def new_step_states(device, ngroup, steps=None, betas=None):
    """kf_step_state[ngroup] on `device` as a uint8 tensor: zero-filled with
    both pows 1, or, resuming, step = steps[j] and the pows Python's
    beta ** step for betas[j] = (beta1, beta2)."""
    import numpy as np
    a = np.zeros(max(1, ngroup), _lib.step_state_dtype())
    a["beta1_pow"] = a["beta2_pow"] = 1.0
    for j, t in enumerate(steps or []):
        a["step"][j] = int(t)
        a["beta1_pow"][j] = float(betas[j][0]) ** int(t)
        a["beta2_pow"][j] = float(betas[j][1]) ** int(t)
    return torch.from_numpy(a.view(np.uint8).copy()).to(device)


def read_step_gate(gate):
    """The gate as a numpy record (synchronises with the device)."""
    return gate.cpu().numpy().view(_lib.step_gate_dtype())[0]


def read_step_states(states):
    """The step states as a numpy record array (synchronises)."""
    return states.cpu().numpy().view(_lib.step_state_dtype())


def _check_gate(gate, states=None, ngroup=1):
    ts = [gate] if states is None else [gate, states]
    _check_dev(ts)
    for t, size, what in ((gate, ctypes.sizeof(_lib.StepGate), "gate"),
                          (states, ngroup * ctypes.sizeof(_lib.StepState), "step states")):
        if t is not None and (t.dtype != torch.uint8 or t.numel() < size or t.data_ptr() % 8):
            raise ValueError("the %s must be at least %d uint8 bytes, 8-byte aligned" % (what, size))


def step_gate_update_(sq, world, nps, groups, states, gate, max_norm=0.0, growth_factor=1.0,
                      backoff_factor=1.0, growth_interval=0, stream=None):
    """One verdict of a gated optimizer step on the device (kf_step_gate_update,
    kungfu_amd/csrc/kf_step_gate.hip). sq: fp64 device tensor of world *
    len(nps) sums of squares, sq[r * nplan + k]; nps[k]: what plan k's gradients
    are still to be divided by (0: nothing); groups[j]: dict with lr and betas;
    states: new_step_states' tensor for them; gate: new_step_gate's. Writes
    skip, grad_mul, grad_norm, the loss scale's update and, unless the step is
    skipped, every group's step, pows, s2 and nss. No host sync."""
    nps, groups = [int(n) for n in nps], list(groups)
    _check_dev([sq])
    _check_gate(gate, states if groups else None, len(groups))
    if sq.dtype != torch.float64 or sq.numel() != int(world) * len(nps) or not nps:
        raise ValueError("step_gate_update_: sq is world * len(nps) float64 values")
    garr = (_lib.StepGroup * max(1, len(groups)))()
    for a, h in zip(garr, groups):
        a.lr = float(h["lr"])
        a.beta1, a.beta2 = (float(b) for b in h.get("betas", (0.9, 0.999)))
    rc = _lib.load().kf_step_gate_update(
        sq.data_ptr(), int(world), len(nps), (ctypes.c_int * len(nps))(*nps), garr,
        states.data_ptr() if groups else None, len(groups), float(max_norm or 0.0),
        float(growth_factor), float(backoff_factor), int(growth_interval), gate.data_ptr(),
        _stream(stream, gate.device))
    _lib.check(rc, "kf_step_gate_update", source="")
    return gate


def _state_ptr(states, group):
    return states.data_ptr() + int(group) * ctypes.sizeof(_lib.StepState)


def adam_update_batch_gated_(params, grads, exp_avgs, exp_avg_sqs, hyper, gate, states, group=0,
                             np_=0, stream=None):
    """adam_update_batch_ under a step gate (kf_adam_update_batch_gated): one
    `hyper` dict for every segment (lr, betas, eps, weight_decay, decoupled; no
    step: the bias corrections are the device's), the gate and group `group`
    of `states` as step_gate_update_ left them. A skipped step leaves params
    and both states untouched; otherwise g is multiplied by the gate's
    grad_mul directly after the /np_."""
    return _update_batch(_adam_update_batch_gated, (params, grads, exp_avgs, exp_avg_sqs),
                         hyper, (gate, states, group), np_, stream)


def adam_master_update_batch_gated_(params16, grads16, masters, exp_avgs, exp_avg_sqs, hyper, gate,
                                    states, group=0, np_=0, stream=None):
    """adam_master_update_batch_ under a step gate
    (kf_adam_master_update_batch_gated); hyper, gate, states and group as
    adam_update_batch_gated_ takes them. A skipped step leaves params16,
    masters and both states untouched."""
    return _update_batch(_adam_master_update_batch_gated,
                         (params16, grads16, masters, exp_avgs, exp_avg_sqs),
                         hyper, (gate, states, group), np_, stream)


# -- Adam, stochastic rounding (include/kungfu_amd.h) -----------

def adam_sr_update_batch_(params, grads, exp_avgs, exp_avg_sqs, hypers, bases, streams, key,
                          np_=0, stream=None):
    """The Adam / AdamW update of many flat bf16 segments with bf16 state,
    fp32 arithmetic in registers and stochastic rounding of p and exp_avg_sq,
    one launch per 32 segments (kf_adam_sr_update_batch,
    kungfu_amd/csrc/kf_adam_sr.hip), in place on params and both states. The
    arithmetic is adam_master_update_batch_'s on the widened values; exp_avg is
    narrowed round-to-nearest-even. bases[b] is the element index of segment
    b's first element (a multiple of 8), streams[b] its 32-bit stream word and
    `key` the call's 32-bit key: the random bits are Philox2x32-10 of (key,
    stream word, element index) and of nothing else. hypers[b] as
    adam_update_batch_ takes them. grads are only read."""
    return _update_batch(_adam_sr_update_batch, (params, grads, exp_avgs, exp_avg_sqs), hypers,
                         None, np_, stream, (bases, streams, key))


def adam_sr_update_batch_gated_(params, grads, exp_avgs, exp_avg_sqs, hyper, gate, states, bases,
                                streams, key, group=0, np_=0, stream=None):
    """adam_sr_update_batch_ under a step gate (kf_adam_sr_update_batch_gated);
    hyper, gate, states and group as adam_update_batch_gated_ takes them. A
    skipped step leaves params and both states untouched."""
    return _update_batch(_adam_sr_update_batch_gated, (params, grads, exp_avgs, exp_avg_sqs),
                         hyper, (gate, states, group), np_, stream, (bases, streams, key))


def adam_sr_narrow(x, r):
    """sr(x, r) element-wise on the device (kf_adam_sr_narrow): x holds fp32
    bit patterns as int32, r 16-bit random words as int16; returns the bf16
    results as an int16 tensor. The update kernels' own narrowing, for sweeps."""
    _check_dev([x, r])
    if x.dtype != torch.int32 or r.dtype != torch.int16 or x.numel() != r.numel() or \
            not (x.is_contiguous() and r.is_contiguous()):
        raise ValueError("adam_sr_narrow: int32 bit patterns and as many int16 random words")
    out = torch.empty_like(r)
    rc = _lib.load().kf_adam_sr_narrow(x.data_ptr(), r.data_ptr(), out.data_ptr(), x.numel(),
                                       _stream(None, x.device))
    _lib.check(rc, "kf_adam_sr_narrow", source="")
    return out


# -- Lion (include/kungfu_amd.h "Lion") -------------------------

def lion_sign_bytes(q):
    """The bytes of a piece's sign codes (kf_lion_sign_bytes; no device needed):
    q / 16 dwords, padded to the next 16 bytes."""
    return int(_lib.load().kf_lion_sign_bytes(int(q)))


def _lion_tables(name, tables, hypers, sr):
    """The checks the three Lion wrappers share; tables[0] leads (its dtype,
    f32 or bf16, is every float table's). Returns (nb, counts, hyper array,
    bases, streams, key) for the C call."""
    nb = len(tables[0])
    if any(len(t) != nb for t in tables) or len(hypers) != nb:
        raise ValueError("%s: one tensor of every table and one hyper per segment" % name)
    for t in tables:
        _check_dev(t)
    lead = tables[0][0]
    if any(x.dtype != lead.dtype or x.numel() != y.numel()
           for t in tables for x, y in zip(t, tables[0])):
        raise ValueError("%s: shape/dtype mismatch" % name)
    bases = streams = None
    key = 0
    if lead.dtype == torch.bfloat16 and sr is not False:
        if sr is None:
            raise ValueError("%s: bf16 needs sr=(bases, streams, key)" % name)
        b, s, key = [int(x) for x in sr[0]], [int(x) for x in sr[1]], int(sr[2])
        if len(b) != nb or len(s) != nb or not 0 <= key < 1 << 32 or \
                any(not 0 <= x < 1 << 32 for x in s) or any(not 0 <= x < 1 << 64 for x in b):
            raise ValueError("%s: a base (64-bit) and a stream word (32-bit) per segment and a "
                             "32-bit key" % name)
        bases, streams = (ctypes.c_uint64 * nb)(*b), (ctypes.c_uint32 * nb)(*s)
    counts = (ctypes.c_size_t * nb)(*[p.numel() for p in tables[0]])
    return nb, counts, _lib.lion_hyper_array(hypers), bases, streams, key


def _ptrs(ts):
    return _lib.ptr_array([t.data_ptr() for t in ts])


def lion_update_batch_(params, grads, moms, hypers, np_=0, sr=None, stream=None):
    """The Lion update of many flat segments of one dtype (f32 or bf16) in one
    launch per 32 of them (kf_lion_update_batch, kungfu_amd/csrc/kf_lion.hip),
    in place on params and moms:

      g = grads[b] / np_ (np_ > 0) ; c = b1 * m + (1 - b1) * g ; m = b2 * m + (1 - b2) * g
      p *= 1 - lr * wd ; p -= lr * sign(c)

    rounded as include/kungfu_amd.h ("Lion") states. hypers[b] is a dict with
    lr and optionally betas (0.9, 0.99) and weight_decay. bf16 parameters are
    stored with stochastic rounding and need sr = (bases, streams, key) as
    adam_sr_update_batch_ takes them. Lengths are multiples of 32; every tensor
    starts 16-byte aligned. grads are only read."""
    params, grads, moms, hypers = list(params), list(grads), list(moms), list(hypers)
    if not params and not grads and not moms:
        return params
    nb, cnt, h, bases, streams, key = _lion_tables("lion_update_batch_", (params, grads, moms),
                                                   hypers, sr)
    rc = _lib.load().kf_lion_update_batch(_ptrs(params), _ptrs(grads), _ptrs(moms), cnt, bases,
                                          streams, nb, int(kungfu_dtype(params[0])), int(np_), h,
                                          key, _stream(stream, params[0].device))
    _lib.check(rc, "kf_lion_update_batch", source="")
    return params


def _lion_codes(name, codes, lead):
    """codes[b]: int32, lion_sign_bytes(n) / 4 values for a segment of n elements."""
    _check_dev(codes)
    if len(codes) != len(lead) or any(
            c.dtype != torch.int32 or c.numel() * 4 != lion_sign_bytes(p.numel())
            for c, p in zip(codes, lead)):
        raise ValueError("%s: codes[b] holds lion_sign_bytes(n) / 4 int32 values" % name)


def lion_signs_batch_(grads, moms, codes, hypers, np_=0, stream=None):
    """Lion's momentum update and the 2-bit codes of its sign update
    (kf_lion_signs_batch): reads grads and moms, writes moms and codes, touches
    no parameter. codes[b] is an int32 tensor of lion_sign_bytes(n) / 4 values:
    element i's code (0 keep, 1 p -= lr, 3 p += lr, 2 NaN) in bits 2 * (i % 16)
    of value i // 16, zero padding behind."""
    grads, moms, codes, hypers = list(grads), list(moms), list(codes), list(hypers)
    if not grads and not moms and not codes:
        return codes
    nb, cnt, h, _, _, _ = _lion_tables("lion_signs_batch_", (grads, moms), hypers, False)
    _lion_codes("lion_signs_batch_", codes, grads)
    rc = _lib.load().kf_lion_signs_batch(_ptrs(grads), _ptrs(moms), _ptrs(codes), cnt, nb,
                                         int(kungfu_dtype(grads[0])), int(np_), h,
                                         _stream(stream, grads[0].device))
    _lib.check(rc, "kf_lion_signs_batch", source="")
    return codes


def lion_apply_signs_batch_(params, codes, hypers, sr=None, stream=None):
    """Apply lion_signs_batch_'s codes to params in place
    (kf_lion_apply_signs_batch): the decay, then -lr, 0 or +lr per element (or
    NaN). lion_apply_signs_batch_(p, lion_signs_batch_(g, m)) leaves the bits
    lion_update_batch_(p, g, m) leaves; for bf16 with the same sr = (bases,
    streams, key), however the elements are cut into segments."""
    params, codes, hypers = list(params), list(codes), list(hypers)
    if not params and not codes:
        return params
    nb, cnt, h, bases, streams, key = _lion_tables("lion_apply_signs_batch_", (params,), hypers, sr)
    _lion_codes("lion_apply_signs_batch_", codes, params)
    rc = _lib.load().kf_lion_apply_signs_batch(_ptrs(params), _ptrs(codes), cnt, bases, streams, nb,
                                               int(kungfu_dtype(params[0])), h, key,
                                               _stream(stream, params[0].device))
    _lib.check(rc, "kf_lion_apply_signs_batch", source="")
    return params


# -- Muon (include/kungfu_amd.h "Muon") -------------------------

MUON_COEFFS = (3.4445, -4.7750, 2.0315)  # the quintic's (a, b, c)


def muon_tile():
    """The grouped GEMM kernel's block tile, both ways (kf_muon_tile; no device
    needed)."""
    return int(_lib.load().kf_muon_tile())


def _muon_flat(name, tables, dtypes):
    """The checks of the element-wise Muon wrappers: one tensor per table and
    segment, table i of dtypes[i], equal lengths across a segment."""
    nb = len(tables[0])
    if any(len(t) != nb for t in tables):
        raise ValueError("%s: one tensor of every table per segment" % name)
    for t, dt in zip(tables, dtypes):
        _check_dev(t)
        if any(x.dtype != dt or x.numel() != y.numel() for x, y in zip(t, tables[0])):
            raise ValueError("%s: shape/dtype mismatch" % name)
    return nb, (ctypes.c_size_t * max(1, nb))(*[t.numel() for t in tables[0]])


def muon_momentum_batch_(grads, moms, dirs, hypers, np_=0, stream=None):
    """Muon's momentum on many flat f32 segments in one launch per 32 of them
    (kf_muon_momentum_batch, kungfu_amd/csrc/kf_muon.hip):

      g = grads[b] / np_ (np_ > 0) ; m = mu * m + g ; d = nesterov ? g + mu * m : m

    moms in place (f32), d rounded once into the bf16 dirs[b]. hypers[b] is a
    dict with momentum and optionally nesterov. Lengths are multiples of 8;
    every tensor starts 16-byte aligned. grads are only read."""
    grads, moms, dirs, hypers = list(grads), list(moms), list(dirs), list(hypers)
    if not grads and not moms and not dirs:
        return dirs
    nb, cnt = _muon_flat("muon_momentum_batch_", (grads, moms, dirs),
                         (torch.float32, torch.float32, torch.bfloat16))
    if len(hypers) != nb:
        raise ValueError("muon_momentum_batch_: one hyper per segment")
    rc = _lib.load().kf_muon_momentum_batch(_ptrs(grads), _ptrs(moms), _ptrs(dirs), cnt, nb,
                                            int(DataType.F32), int(np_),
                                            _lib.muon_hyper_array(hypers),
                                            _stream(stream, grads[0].device))
    _lib.check(rc, "kf_muon_momentum_batch", source="")
    return dirs


def muon_scale_batch_(dirs, xs, sq, stream=None):
    """xs[b] = dirs[b] / (sqrt(sq[b]) + 1e-7) (kf_muon_scale_batch): bf16 in and
    out, sq a float64 device tensor of at least len(dirs) squared norms
    (SegNorm.run's out over dirs). Nothing synchronises the host."""
    dirs, xs = list(dirs), list(xs)
    if not dirs and not xs:
        return xs
    nb, cnt = _muon_flat("muon_scale_batch_", (dirs, xs), (torch.bfloat16, torch.bfloat16))
    _check_dev([sq])
    if sq.dtype != torch.float64 or sq.numel() < nb:
        raise ValueError("muon_scale_batch_: sq holds a float64 squared norm per segment")
    rc = _lib.load().kf_muon_scale_batch(_ptrs(dirs), _ptrs(xs), cnt, sq.data_ptr(), nb,
                                         _stream(stream, dirs[0].device))
    _lib.check(rc, "kf_muon_scale_batch", source="")
    return xs


def muon_apply_batch_(params, xs, hypers, stream=None):
    """p = (1 - lr * weight_decay) * p - lr * scale * x on many flat f32
    segments with bf16 xs (kf_muon_apply_batch), in place. hypers[b] is a dict
    with lr and optionally weight_decay and scale (Muon's
    sqrt(max(1, rows / cols)); 1 by default). Tensors may start at any element."""
    params, xs, hypers = list(params), list(xs), list(hypers)
    if not params and not xs:
        return params
    nb, cnt = _muon_flat("muon_apply_batch_", (params, xs), (torch.float32, torch.bfloat16))
    if len(hypers) != nb:
        raise ValueError("muon_apply_batch_: one hyper per segment")
    h = (_lib.MuonApply * max(1, nb))()
    for a, x in zip(h, hypers):
        a.lr, a.weight_decay = float(x["lr"]), float(x.get("weight_decay", 0.0))
        a.scale = float(x.get("scale", 1.0))
    rc = _lib.load().kf_muon_apply_batch(_ptrs(params), _ptrs(xs), cnt, h, nb, int(DataType.F32),
                                         _stream(stream, params[0].device))
    _lib.check(rc, "kf_muon_apply_batch", source="")
    return params


def _muon_table(name, problems):
    """(kf_muon_gemm[], the tensors kept alive) of problems (a, b, c[, cin[,
    trans_a[, trans_b]]]): 2-D bf16 device tensors whose rows are contiguous
    (stride(1) == 1; stride(0) is the leading dimension)."""
    tab, keep = (_lib.MuonGemm * max(1, len(problems)))(), []
    for q, prob in zip(tab, problems):
        a, b, c, cin, ta, tb = (tuple(prob) + (None, False, False))[:6]
        ts = [t for t in (a, b, c, cin) if t is not None]
        for t in ts:
            if not t.is_cuda or t.dtype != torch.bfloat16 or t.dim() != 2 or \
                    (t.shape[1] > 1 and t.stride(1) != 1):
                raise ValueError("%s: 2-D bf16 GPU tensors with contiguous rows" % name)
        (m, k), (k2, n) = (a.shape[::-1] if ta else a.shape), (b.shape[::-1] if tb else b.shape)
        if k != k2 or tuple(c.shape) != (m, n) or (cin is not None and tuple(cin.shape) != (m, n)):
            raise ValueError("%s: op(a) is m x k, op(b) k x n, c and cin m x n" % name)
        ld = lambda t: max(int(t.stride(0)), int(t.shape[1])) if t.shape[0] > 1 else int(t.shape[1])  # noqa: E731
        q.a, q.b, q.c = a.data_ptr(), b.data_ptr(), c.data_ptr()
        q.cin = cin.data_ptr() if cin is not None else None
        q.m, q.n, q.k, q.lda, q.ldb, q.ldc = m, n, k, ld(a), ld(b), ld(c)
        q.ldcin = ld(cin) if cin is not None else 0
        q.trans_a, q.trans_b = int(bool(ta)), int(bool(tb))
        keep.append(ts)
    return tab, keep


def _muon_gemm(tab, count, alpha, beta, stream):
    rc = _lib.load().kf_muon_gemm_grouped(tab, count, int(DataType.BF16), float(alpha), float(beta),
                                          stream)
    _lib.check(rc, "kf_muon_gemm_grouped", source="")


def muon_gemm_grouped_(problems, alpha=1.0, beta=1.0, stream=None):
    """c = alpha * cin + beta * op(a) @ op(b) for every problem, in one launch
    per 32 problems of the MFMA kernel (kf_muon_gemm_grouped): bf16 matrices,
    f32 accumulation, one rounding. A problem is (a, b, c[, cin[, trans_a[,
    trans_b]]]); op(x) is x.T where its flag is set; any m, n, k >= 1; rows may
    be strided. c must not overlap a or b (cin may be c). The same bits on
    every run. Returns the cs."""
    problems = list(problems)
    if not problems:
        return []
    tab, keep = _muon_table("muon_gemm_grouped_", problems)
    _muon_gemm(tab, len(problems), alpha, beta, _stream(stream, problems[0][2].device))
    return [p[2] for p in problems]


def _muon_syrk_table(name, problems):
    """_muon_table for the symmetric product's problems (a, c[, cin[,
    trans_a]]): checked as the general product of op(a) and op(a).T, then b
    is NULL and n is m."""
    general = []
    for prob in problems:
        a, c, cin, ta = (tuple(prob) + (None, False))[:4]
        general.append((a, a, c, cin, ta, not ta))
    tab, keep = _muon_table(name, general)
    for q in tab:
        q.b, q.ldb, q.trans_b = None, 0, 0
    return tab, keep


def _muon_syrk(tab, count, alpha, beta, stream):
    rc = _lib.load().kf_muon_syrk_grouped(tab, count, int(DataType.BF16), float(alpha), float(beta),
                                          stream)
    _lib.check(rc, "kf_muon_syrk_grouped", source="")


def muon_syrk_grouped_(problems, alpha=1.0, beta=1.0, stream=None):
    """c = alpha * cin + beta * op(a) @ op(a).T for every problem, in one launch
    per 32 problems of the symmetric MFMA kernel (kf_muon_syrk_grouped): only
    the lower triangle of c's 64 x 64 tiles is computed, with
    muon_gemm_grouped_'s bits, and mirrored, so c equals c.T bit for bit. A
    problem is (a, c[, cin[, trans_a]]); op(a) is a.T where the flag is set;
    c and cin are m x m, and cin is read at row >= col only; any m, k >= 1;
    rows may be strided. c must not overlap a (cin may be c). Returns the cs."""
    problems = list(problems)
    if not problems:
        return []
    tab, keep = _muon_syrk_table("muon_syrk_grouped_", problems)
    _muon_syrk(tab, len(problems), alpha, beta, _stream(stream, problems[0][1].device))
    return [p[1] for p in problems]


def _muon_symmetric(name, symmetric):
    if not isinstance(symmetric, bool):
        raise ValueError("%s: symmetric must be a bool, not %r" % (name, symmetric))
    return symmetric


class MuonPlan:
    """Newton-Schulz over a fixed list of tensors: dirs[t] is a flat bf16
    device tensor of rows * cols elements (a tensor's view in a direction
    bucket: any element offset) and shapes[t] its (rows, cols). Made once: the
    workspace (two copies of every tensor and two s x s matrices each, s =
    min(rows, cols): 2 * sum(rows * cols) + 2 * sum(s * s) bf16, each piece
    16-byte aligned), the norms' SegNorm plan and the GEMM tables are kept, so
    run() allocates nothing, does not synchronise the host and can be captured
    into a graph.

    run(steps) -> the orthogonalised tensors, as rows x cols views of the
    workspace that the next run overwrites: 2 launches for the norms, the
    scale, and per step 3 grouped GEMM launches per 32 tensors (X X^T; b A + c
    A A; a X + B X; for rows > cols X^T X and a X + X B).

    symmetric=True runs the first two products, whose results are symmetric,
    on the symmetric kernel (muon_syrk_grouped_: the lower triangle of tiles,
    mirrored) and the third on the general one as before; same workspace,
    same launch count."""

    def __init__(self, dirs, shapes, symmetric=False):
        self.symmetric = _muon_symmetric("MuonPlan", symmetric)
        dirs, shapes = list(dirs), [tuple(int(x) for x in s) for s in shapes]
        if not dirs or len(dirs) != len(shapes):
            raise ValueError("MuonPlan: at least one tensor, and a (rows, cols) for each")
        _check_dev(dirs)
        for d, (r, c) in zip(dirs, shapes):
            if d.dtype != torch.bfloat16 or d.dim() != 1 or r < 1 or c < 1 or d.numel() != r * c:
                raise ValueError("MuonPlan: flat bf16 tensors of rows * cols >= 1 elements")
        up = lambda n: (n + 7) // 8 * 8  # noqa: E731
        need = sum(2 * up(r * c) + 2 * up(min(r, c) ** 2) for r, c in shapes)
        self.device, self.dirs, self.shapes = dirs[0].device, dirs, shapes
        self.workspace = torch.zeros(need, dtype=torch.bfloat16, device=self.device)
        self.norms = SegNorm(dirs)
        self.sq = torch.zeros(len(dirs) + 1, dtype=torch.float64, device=self.device)
        off, self.x, gram, quint, xmul = 0, ([], []), ([], []), [], ([], [])
        sgram, squint = ([], []), []

        def take(n):
            nonlocal off
            off += up(n)
            return self.workspace[off - up(n):off - up(n) + n]

        for r, c in shapes:
            s, tall = min(r, c), r > c
            x = [take(r * c).view(r, c) for _ in range(2)]
            a, b = (take(s * s).view(s, s) for _ in range(2))
            quint.append((a, a, b, a))
            squint.append((a, b, a))
            for p in range(2):
                self.x[p].append(x[p])
                # rows > cols: the short side's Gram matrix, with no transposed copy
                gram[p].append((x[p], x[p], a, None, tall, not tall))
                sgram[p].append((x[p], a, None, tall))
                xmul[p].append((x[p], b, x[1 - p], x[p]) if tall else (b, x[p], x[1 - p], x[p]))
        if symmetric:
            self._tables = [[_muon_syrk_table("MuonPlan", sgram[p]),
                             _muon_syrk_table("MuonPlan", squint),
                             _muon_table("MuonPlan", xmul[p])] for p in range(2)]
        else:
            self._tables = [[_muon_table("MuonPlan", t) for t in (gram[p], quint, xmul[p])]
                            for p in range(2)]

    def run(self, steps=5, stream=None):
        if isinstance(steps, bool) or not isinstance(steps, int) or not 1 <= steps <= 16:
            raise ValueError("MuonPlan.run: steps must be an int in [1, 16], not %r" % (steps,))
        n, a, b, c = len(self.dirs), *MUON_COEFFS
        self.norms.run("sq", out=self.sq, stream=stream)
        muon_scale_batch_(self.dirs, [x.view(-1) for x in self.x[0]], self.sq, stream=stream)
        s = _stream(stream, self.device)
        first = _muon_syrk if self.symmetric else _muon_gemm
        for i in range(steps):
            gram, quint, xmul = self._tables[i & 1]
            first(gram[0], n, 0.0, 1.0, s)
            first(quint[0], n, b, c, s)
            _muon_gemm(xmul[0], n, a, 1.0, s)
        return self.x[steps & 1]


def muon_newton_schulz_(tensors2d, steps=5, stream=None, symmetric=False):
    """Every tensor (bf16, contiguous, viewed as shape[0] x the rest) replaced
    by its Newton-Schulz orthogonalisation, `steps` iterations of the quintic
    on t / (|t|_F + 1e-7): the whole chain of a MuonPlan made for this call.
    An optimizer keeps its plan instead (MuonPlan). symmetric: MuonPlan's."""
    _muon_symmetric("muon_newton_schulz_", symmetric)
    ts = list(tensors2d)
    if not ts:
        return ts
    for t in ts:
        if t.dim() < 2 or not t.is_contiguous():
            raise ValueError("muon_newton_schulz_: contiguous tensors of 2 or more dimensions")
    plan = MuonPlan([t.view(-1) for t in ts], [(t.shape[0], t.numel() // t.shape[0]) for t in ts],
                    symmetric)
    for t, x in zip(ts, plan.run(steps, stream)):
        t.view(x.shape).copy_(x)
    return ts


# -- Adam, 8-bit block-wise state (include/kungfu_amd.h) --------

ADAM8_ZERO_CODE = (127, 0)       # the code of 0.0: signed (exp_avg), unsigned (exp_avg_sq)


def adam8_codebook(which):
    """Table `which` (0: signed, exp_avg; 1: unsigned, exp_avg_sq) as a float32
    numpy array of 256 values (kf_adam8_codebook; no device needed)."""
    import numpy as np
    out = (ctypes.c_float * 256)()
    _lib.check(_lib.load().kf_adam8_codebook(int(which), out), "kf_adam8_codebook", source="")
    return np.frombuffer(out, np.float32).copy()


def adam8_zero_state(n, device):
    """(exp_avg codes, exp_avg_sq codes, exp_avg scales, exp_avg_sq scales) of
    n zeros: scale 0, code 127 and code 0. n must be a multiple of 64."""
    if n % ADAM8_BLOCK:
        raise ValueError("adam8_zero_state: n must be a multiple of 64")
    return (torch.full((n,), ADAM8_ZERO_CODE[0], dtype=torch.uint8, device=device),
            torch.full((n,), ADAM8_ZERO_CODE[1], dtype=torch.uint8, device=device),
            torch.zeros(n // ADAM8_BLOCK, dtype=torch.float32, device=device),
            torch.zeros(n // ADAM8_BLOCK, dtype=torch.float32, device=device))


def adam8_update_batch_(params, grads, m_codes, v_codes, m_scales, v_scales, hypers, np_=0,
                        stream=None):
    """The Adam / AdamW update of many flat f32 segments whose exp_avg and
    exp_avg_sq are block-wise 8-bit codes (kf_adam8_update_batch,
    kungfu_amd/csrc/kf_adam8.hip), one launch per 24 segments, in place on
    params, codes and scales: dequantize, adam_update_batch_'s f32 arithmetic,
    quantize. Every segment's length is a multiple of 64; codes are uint8 of
    that length, scales f32 of a 64th of it. hypers[b] as adam_update_batch_
    takes them. grads are only read."""
    return _update_batch(_adam8_update_batch,
                         (params, grads, m_codes, v_codes, m_scales, v_scales),
                         hypers, None, np_, stream)


def adam8_update_batch_gated_(params, grads, m_codes, v_codes, m_scales, v_scales, hyper, gate,
                              states, group=0, np_=0, stream=None):
    """adam8_update_batch_ under a step gate (kf_adam8_update_batch_gated);
    hyper, gate, states and group as adam_update_batch_gated_ takes them. A
    skipped step leaves params, codes and scales untouched."""
    return _update_batch(_adam8_update_batch_gated,
                         (params, grads, m_codes, v_codes, m_scales, v_scales), hyper,
                         (gate, states, group), np_, stream)


def adam8_master_update_batch_(params16, grads16, masters, m_codes, v_codes, m_scales, v_scales,
                               hypers, np_=0, stream=None):
    """adam8_update_batch_ for bf16 or f16 parameters with an fp32 master copy
    (kf_adam8_master_update_batch): the f32 update runs on (masters, widened
    grads16, dequantized state) and params16 = masters narrowed,
    round-to-nearest-even. params16 is written, never read."""
    return _update_batch(_adam8_master_update_batch,
                         (params16, grads16, masters, m_codes, v_codes, m_scales, v_scales),
                         hypers, None, np_, stream)


def adam8_master_update_batch_gated_(params16, grads16, masters, m_codes, v_codes, m_scales,
                                     v_scales, hyper, gate, states, group=0, np_=0, stream=None):
    """adam8_master_update_batch_ under a step gate
    (kf_adam8_master_update_batch_gated). A skipped step leaves params16,
    masters, codes and scales untouched."""
    return _update_batch(_adam8_master_update_batch_gated,
                         (params16, grads16, masters, m_codes, v_codes, m_scales, v_scales),
                         hyper, (gate, states, group), np_, stream)


def adam8_quantize(x, which, codes=None, scales=None, stream=None):
    """(codes, scales) of the flat f32 tensor x in table `which`'s format
    (kf_adam8_quantize): uint8 codes of x's length and one f32 scale per 64
    elements, new tensors unless given."""
    n = x.numel()
    if x.dtype != torch.float32 or n % ADAM8_BLOCK:
        raise ValueError("adam8_quantize: a flat f32 tensor of a multiple of 64 elements")
    codes = torch.empty(n, dtype=torch.uint8, device=x.device) if codes is None else codes
    scales = torch.empty(n // ADAM8_BLOCK, dtype=torch.float32, device=x.device) \
        if scales is None else scales
    _check_dev([x, codes, scales])
    if codes.dtype != torch.uint8 or codes.numel() != n or scales.dtype != torch.float32 or \
            scales.numel() * ADAM8_BLOCK != n:
        raise ValueError("adam8_quantize: uint8 codes of x's length, one f32 scale per 64 elements")
    rc = _lib.load().kf_adam8_quantize(x.data_ptr(), codes.data_ptr(), scales.data_ptr(), n,
                                       int(which), _stream(stream, x.device))
    _lib.check(rc, "kf_adam8_quantize", source="")
    return codes, scales


def adam8_dequantize(codes, scales, which, out=None, stream=None):
    """The f32 values of (codes, scales) in table `which`'s format
    (kf_adam8_dequantize), a new tensor unless `out` is given."""
    n = codes.numel()
    out = torch.empty(n, dtype=torch.float32, device=codes.device) if out is None else out
    _check_dev([codes, scales, out])
    if codes.dtype != torch.uint8 or n % ADAM8_BLOCK or scales.dtype != torch.float32 or \
            scales.numel() * ADAM8_BLOCK != n or out.dtype != torch.float32 or out.numel() != n:
        raise ValueError("adam8_dequantize: uint8 codes of a multiple of 64 elements, one f32 "
                         "scale per 64 and an f32 result of the codes' length")
    rc = _lib.load().kf_adam8_dequantize(codes.data_ptr(), scales.data_ptr(), out.data_ptr(), n,
                                         int(which), _stream(stream, codes.device))
    _lib.check(rc, "kf_adam8_dequantize", source="")
    return out


# -- the MXFP8 gradient wire (include/kungfu_amd.h) -------------

MX8_BLOCK = 32                   # elements per scale byte


def mx8_piece_bytes(q):
    """The bytes of one packed piece of q elements (kf_mx8_piece_bytes): q
    codes, q // 32 scale bytes, rounded up to 16."""
    return int(_lib.load().kf_mx8_piece_bytes(int(q)))


def mx8_pack_batch_(grads, world, packed=None, stream=None):
    """Every flat f32, bf16 or f16 bucket of `grads` as `world` packed MXFP8
    pieces (kf_mx8_pack_batch), all buckets in one launch: packed[b] is a uint8
    tensor of world * mx8_piece_bytes(numel // world) bytes, new unless given;
    piece j is what rank j receives. numel // world must be a multiple of 32;
    the numel % world tail is not packed. grads are only read."""
    grads, world = list(grads), int(world)
    if world < 1:
        raise ValueError("mx8_pack_batch_: world >= 1")
    need = [world * mx8_piece_bytes(g.numel() // world) for g in grads]
    if packed is None:
        packed = [torch.empty(n, dtype=torch.uint8, device=g.device) for n, g in zip(need, grads)]
    packed = list(packed)
    if len(packed) != len(grads):
        raise ValueError("mx8_pack_batch_: one packed tensor per bucket")
    if not grads:
        return packed
    _check_dev(grads + packed)
    for g, p, n in zip(grads, packed, need):
        if g.dtype != grads[0].dtype or p.dtype != torch.uint8 or p.numel() != n:
            raise ValueError("mx8_pack_batch_: one dtype, and uint8 tensors of world pieces")
    cnt = (ctypes.c_size_t * len(grads))(*[g.numel() for g in grads])
    rc = _lib.load().kf_mx8_pack_batch(_lib.ptr_array([g.data_ptr() for g in grads]),
                                       _lib.ptr_array([p.data_ptr() for p in packed]), cnt,
                                       len(grads), world, int(kungfu_dtype(grads[0])),
                                       _stream(stream, grads[0].device))
    _lib.check(rc, "kf_mx8_pack_batch", source="")
    return packed


def _mx8_pack_variant(name, grads, world, packed, stream, call, piece_bytes=mx8_piece_bytes):
    """What the pack variants (and the 1-bit wire's pack, with its own
    piece_bytes) share with mx8_pack_batch_: its checks, then
    call(lib, grad pointers, packed pointers, counts, nb, dtype, stream)."""
    grads, world = list(grads), int(world)
    if world < 1:
        raise ValueError("%s: world >= 1" % name)
    need = [world * piece_bytes(g.numel() // world) for g in grads]
    if packed is None:
        packed = [torch.empty(n, dtype=torch.uint8, device=g.device) for n, g in zip(need, grads)]
    packed = list(packed)
    if len(packed) != len(grads):
        raise ValueError("%s: one packed tensor per bucket" % name)
    if not grads:
        return packed
    _check_dev(grads + packed)
    for g, p, n in zip(grads, packed, need):
        if g.dtype != grads[0].dtype or p.dtype != torch.uint8 or p.numel() != n:
            raise ValueError("%s: one dtype, and uint8 tensors of world pieces" % name)
    cnt = (ctypes.c_size_t * len(grads))(*[g.numel() for g in grads])
    rc = call(_lib.load(), _lib.ptr_array([g.data_ptr() for g in grads]),
              _lib.ptr_array([p.data_ptr() for p in packed]), cnt, len(grads),
              int(kungfu_dtype(grads[0])), _stream(stream, grads[0].device))
    _lib.check(rc, "kf_" + name.rstrip("_"), source="")
    return packed


def _wire_pack_ef(name, piece_bytes, grads, residuals, world, packed, stream, extra=()):
    """An error-feedback pack (kf_<name>): the residuals' checks, then
    _mx8_pack_variant's. `extra`: the entry's own arguments before the stream."""
    grads, residuals = list(grads), list(residuals)
    if len(residuals) != len(grads) or any(
            r.dtype != torch.float32 or r.numel() != g.numel() or not r.is_contiguous()
            for r, g in zip(residuals, grads)):
        raise ValueError("%s: one contiguous f32 residual of its bucket's length per bucket" % name)
    _check_dev(grads + residuals)
    res = _lib.ptr_array([r.data_ptr() for r in residuals])
    entry = "kf_" + name.rstrip("_")
    return _mx8_pack_variant(
        name, grads, world, packed, stream,
        lambda lib, g, p, cnt, nb, dt, s: getattr(lib, entry)(g, res, p, cnt, nb, int(world), dt,
                                                              *extra, s),
        piece_bytes)


def _wire_fold(name, piece_bytes, packed, out_shards, world, np_, stream, extra=()):
    """A wire's fold (kf_<name>): one shard per packed tensor of world pieces.
    `extra`: the entry's own arguments before the stream."""
    packed, outs, world = list(packed), list(out_shards), int(world)
    if len(packed) != len(outs):
        raise ValueError("%s: one shard per packed tensor" % name)
    if not outs:
        return outs
    _check_dev(packed + outs)
    for p, o in zip(packed, outs):
        if o.dtype != outs[0].dtype or p.dtype != torch.uint8 or \
                p.numel() != world * piece_bytes(o.numel()):
            raise ValueError("%s: one dtype, and uint8 tensors of world pieces" % name)
    q = (ctypes.c_size_t * len(outs))(*[o.numel() for o in outs])
    entry = "kf_" + name.rstrip("_")
    rc = getattr(_lib.load(), entry)(_lib.ptr_array([p.data_ptr() for p in packed]),
                                     _lib.ptr_array([o.data_ptr() for o in outs]), q, len(outs),
                                     world, int(kungfu_dtype(outs[0])), int(np_), *extra,
                                     _stream(stream, outs[0].device))
    _lib.check(rc, entry, source="")
    return outs


def mx8_pack_ef_batch_(grads, residuals, world, packed=None, stream=None):
    """mx8_pack_batch_ with error feedback (kf_mx8_pack_ef_batch, DESIGN.md
    §25): residuals[b] is an f32 tensor of grads[b]'s length; every piece packs
    g + r and leaves r = (g + r) - unpack(what was packed) in place, +0.0 over a
    block that was not finite. grads are only read; the numel % world tail's
    residuals are not touched."""
    return _wire_pack_ef("mx8_pack_ef_batch_", mx8_piece_bytes, grads, residuals, world, packed,
                         stream)


def mx8_pack_sr_batch_(grads, world, seed, step, rank, bucket0=0, packed=None, stream=None):
    """mx8_pack_batch_ with stochastic rounding (kf_mx8_pack_sr_batch,
    DESIGN.md §25): every element goes to one of its two E4M3 neighbours at
    the block's scale, up with the probability of its distance from the lower
    one. The draws are a pure function of (seed, step, rank, bucket0 + b,
    element index in the bucket); seed and step are ints in [0, 2**64)."""
    return _mx8_pack_variant(
        "mx8_pack_sr_batch_", grads, world, packed, stream,
        lambda lib, g, p, cnt, nb, dt, s: lib.kf_mx8_pack_sr_batch(
            g, p, cnt, nb, int(world), dt, int(seed), int(step), int(rank), int(bucket0), s))


def mx8_fold_batch_(packed, out_shards, world, np_=0, stream=None):
    """out_shards[b] = (the `world` pieces of packed[b], unpacked and added in
    f32 in rank order) / np_ (np_ > 0), narrowed once to the shard's dtype
    (kf_mx8_fold_batch), all buckets in one launch. packed[b]: uint8, world *
    mx8_piece_bytes(q) bytes for a shard of q elements (a multiple of 32)."""
    return _wire_fold("mx8_fold_batch_", mx8_piece_bytes, packed, out_shards, world, np_, stream)


# -- the 1-bit gradient wire (include/kungfu_amd.h) -------------

SIGN1_BLOCK = 64                 # elements per f32 scale


def sign1_piece_bytes(q):
    """The bytes of one packed piece of q elements (kf_sign1_piece_bytes):
    q // 8 bytes of sign bits, q // 64 f32 scales, rounded up to 16."""
    return int(_lib.load().kf_sign1_piece_bytes(int(q)))


def sign1_pack_ef_batch_(grads, residuals, world, packed=None, stream=None):
    """Every flat f32, bf16 or f16 bucket of `grads` as `world` packed 1-bit
    pieces (kf_sign1_pack_ef_batch), all buckets in one launch: per block of 64
    elements the sign bits of s = g + r and the scale mean(|s|); residuals[b]
    (f32, grads[b]'s length) is left as s - (the scale with s's sign), +0.0
    over a block that was not finite. packed[b] is a uint8 tensor of world *
    sign1_piece_bytes(numel // world) bytes, new unless given. numel // world
    must be a multiple of 64; the numel % world tail is not packed and its
    residuals are not touched. grads are only read."""
    return _wire_pack_ef("sign1_pack_ef_batch_", sign1_piece_bytes, grads, residuals, world, packed,
                         stream)


def sign1_fold_batch_(packed, out_shards, world, np_=0, stream=None):
    """mx8_fold_batch_ over 1-bit pieces (kf_sign1_fold_batch): packed[b] is
    uint8, world * sign1_piece_bytes(q) bytes for a shard of q elements (a
    multiple of 64)."""
    return _wire_fold("sign1_fold_batch_", sign1_piece_bytes, packed, out_shards, world, np_, stream)


# -- the top-k gradient wire (include/kungfu_amd.h) -------------

TOPK_BLOCK = 64                  # elements per selection
TOPK_K = (1, 2, 4, 8)            # entries sent per block


def _topk_k(name, k):
    if isinstance(k, bool) or k not in TOPK_K:
        raise ValueError("%s: k must be 1, 2, 4 or 8 (got %r)" % (name, k))
    return int(k)


def topk_piece_bytes(q, k):
    """The bytes of one packed piece of q elements (kf_topk_piece_bytes):
    q // 64 * k f32 values, as many index bytes, rounded up to 16."""
    return int(_lib.load().kf_topk_piece_bytes(int(q), _topk_k("topk_piece_bytes", k)))


def topk_pack_ef_batch_(grads, residuals, world, k, packed=None, stream=None):
    """Every flat f32, bf16 or f16 bucket of `grads` as `world` packed top-k
    pieces (kf_topk_pack_ef_batch), all buckets in one launch: per block of 64
    elements the k (1, 2, 4 or 8) largest magnitudes of s = g + r, bits
    unchanged, and their places in the block, largest first and the smaller
    index first among equals; residuals[b] (f32, grads[b]'s length) is left as
    +0.0 where an element was sent or is not finite and s elsewhere. packed[b]
    is a uint8 tensor of world * topk_piece_bytes(numel // world, k) bytes, new
    unless given. numel // world must be a multiple of 64; the numel % world
    tail is not packed and its residuals are not touched. grads are only read."""
    k = _topk_k("topk_pack_ef_batch_", k)
    return _wire_pack_ef("topk_pack_ef_batch_", lambda q: topk_piece_bytes(q, k), grads, residuals,
                         world, packed, stream, (k,))


def topk_fold_batch_(packed, out_shards, world, k, np_=0, stream=None):
    """out_shards[b] = (the entries of the `world` pieces of packed[b], added
    in f32 in rank order where their indices say, zeros elsewhere) / np_
    (np_ > 0), narrowed once (kf_topk_fold_batch): packed[b] is uint8, world *
    topk_piece_bytes(q, k) bytes for a shard of q elements (a multiple of 64)."""
    k = _topk_k("topk_fold_batch_", k)
    return _wire_fold("topk_fold_batch_", lambda q: topk_piece_bytes(q, k), packed, out_shards,
                      world, np_, stream, (k,))


# -- LAMB (include/kungfu_amd.h "LAMB") -------------------------

def lamb_moments_batch_(params, grads, exp_avgs, exp_avg_sqs, updates, hypers, np_=0, stream=None):
    """LAMB's moments pass over many flat f32 or f64 segments, one launch per
    24 of them (kf_lamb_moments_batch, kungfu_amd/csrc/kf_lamb.hip):

      g = grads[b] / np_ (np_ > 0)
      m = b1 * m + (1 - b1) * g ; v = b2 * v + (1 - b2) * g * g
      u = (m / (1 - b1**step)) / (sqrt(v) / sqrt(1 - b2**step) + eps) + wd * p

    rounded as include/kungfu_amd.h states. exp_avgs and exp_avg_sqs are
    updated in place, updates[b] is written, params and grads are only read.
    hypers[b] as adam_update_batch_ takes them (lr and decoupled are ignored).
    Every tensor starts 16-byte aligned."""
    return _update_batch(_lamb_moments_batch, (params, grads, exp_avgs, exp_avg_sqs, updates),
                         hypers, None, np_, stream)


def lamb_master_moments_batch_(grads16, masters, exp_avgs, exp_avg_sqs, updates, hypers, np_=0,
                               stream=None):
    """lamb_moments_batch_ for bf16 or f16 gradients with fp32 master weights
    and state, one launch per 32 segments (kf_lamb_master_moments_batch): the
    gradient is widened, the f32 arithmetic runs on (masters, g, exp_avgs,
    exp_avg_sqs) and writes the fp32 updates. masters and grads16 are only
    read; the 16-bit parameters are not touched (LambApplyPlan writes them)."""
    return _update_batch(_lamb_master_moments_batch,
                         (grads16, masters, exp_avgs, exp_avg_sqs, updates), hypers, None, np_,
                         stream)


def lamb_trust_update_(sq, world, group_of, groups, nlr, ratio, trust_clip=0.0, stream=None):
    """The trust ratios of T = group_of.numel() tensors on the device
    (kf_lamb_trust_update): sq is world * 2 * T float64 sums of squares,
    sq[r * 2T + t] of rank r's piece of tensor t's parameters and
    sq[r * 2T + T + t] of its update; group_of an int32 device tensor (tensor
    -> group); groups[j] a dict with lr and adapt. Writes ratio[t] =
    ||p|| / ||u|| (1 where adapt is off or a norm is not > 0), clipped from
    above by trust_clip > 0, and nlr[t] = -(lr * ratio[t]). No host sync."""
    return _trust_update("lamb_trust_update_", sq, world, group_of, groups, nlr, ratio, None,
                         trust_clip, stream)


def _trust_update(name, sq, world, group_of, groups, nlr, ratio, gate, trust_clip, stream):
    """Both trust updates: gate is None for the ungated one."""
    groups = list(groups)
    _check_dev([sq, group_of, nlr, ratio])
    if gate is not None:
        _check_gate(gate)
    T = group_of.numel()
    if group_of.dtype != torch.int32 or T < 1 or not groups:
        raise ValueError("%s: group_of is a non-empty int32 tensor, and at least one group" % name)
    if sq.dtype != torch.float64 or sq.numel() != int(world) * 2 * T or int(world) < 1:
        raise ValueError("%s: sq is world * 2 * T float64 values" % name)
    for t in (nlr, ratio):
        if t.dtype != torch.float64 or t.numel() != T:
            raise ValueError("%s: nlr and ratio are T float64 values" % name)
    garr = (_lib.LambGroup * len(groups))()
    for a, h in zip(garr, groups):
        a.lr, a.adapt = float(h["lr"]), int(bool(h["adapt"]))
    entry = "kf_lamb_trust_update" if gate is None else "kf_lamb_trust_update_gated"
    rc = getattr(_lib.load(), entry)(
        sq.data_ptr(), int(world), T, group_of.data_ptr(), garr, len(groups),
        float(trust_clip or 0.0), nlr.data_ptr(), ratio.data_ptr(),
        *([] if gate is None else [gate.data_ptr()]), _stream(stream, sq.device))
    _lib.check(rc, entry, source="")
    return nlr


# -- LAMB under a gate (include/kungfu_amd.h "LAMB under a gate")

def lamb_moments_batch_gated_(params, grads, exp_avgs, exp_avg_sqs, updates, hyper, gate, states,
                              group=0, np_=0, stream=None):
    """lamb_moments_batch_ under a step gate (kf_lamb_moments_batch_gated): one
    `hyper` dict for every segment (betas, eps, weight_decay; no step: the bias
    corrections are the device's), the gate and group `group` of `states` as a
    step_gate_update_ with every group's lr = 1 left them. A skipped step
    leaves exp_avgs, exp_avg_sqs and updates untouched; otherwise g is
    multiplied by the gate's grad_mul directly after the /np_."""
    return _update_batch(_lamb_moments_batch_gated,
                         (params, grads, exp_avgs, exp_avg_sqs, updates), hyper,
                         (gate, states, group), np_, stream)


def lamb_master_moments_batch_gated_(grads16, masters, exp_avgs, exp_avg_sqs, updates, hyper, gate,
                                     states, group=0, np_=0, stream=None):
    """lamb_master_moments_batch_ under a step gate
    (kf_lamb_master_moments_batch_gated); hyper, gate, states and group as
    lamb_moments_batch_gated_ takes them."""
    return _update_batch(_lamb_master_moments_batch_gated,
                         (grads16, masters, exp_avgs, exp_avg_sqs, updates), hyper,
                         (gate, states, group), np_, stream)


def lamb_trust_update_gated_(sq, world, group_of, groups, nlr, ratio, gate, trust_clip=0.0,
                             stream=None):
    """lamb_trust_update_ under a step gate (kf_lamb_trust_update_gated): a
    skipped step leaves nlr and ratio as they were."""
    return _trust_update("lamb_trust_update_gated_", sq, world, group_of, groups, nlr, ratio, gate,
                         trust_clip, stream)


class LambApplyPlan:
    """LAMB's apply pass over "tensor ∩ own shard" pieces (kf_lamb_apply_*):
    built once over views that never move, run(nlr) is one launch whatever
    the number of pieces:

      params[i] += nlr[tensors[i]] * updates[i]       (in the pieces' f32 / f64)

    With params16 (bf16 or f16 views of the same lengths) params are the fp32
    master pieces and params16[i] = params[i] narrowed, round-to-nearest-even.
    Pieces are aligned to the element only; a piece's tensors must share their
    element offset from a 16-byte boundary. A piece may be empty. The plan
    keeps the tensors alive. nlr: ntensor float64 values on the device.
    run(nlr, gate=gate) is the same launch under a step gate
    (kf_lamb_apply_run_gated): a skipped step touches nothing."""

    def __init__(self, params, updates, tensors, ntensor, params16=None):
        ps, us, ts = list(params), list(updates), [int(t) for t in tensors]
        p16 = None if params16 is None else list(params16)
        if not (len(ps) == len(us) == len(ts)) or (p16 is not None and len(p16) != len(ps)):
            raise ValueError("LambApplyPlan: one update and tensor index per piece")
        _check_dev(ps + us + (p16 or []))
        for i, (p, u) in enumerate(zip(ps, us)):
            if p.dtype != ps[0].dtype or u.dtype != p.dtype or u.numel() != p.numel():
                raise ValueError("LambApplyPlan: shape/dtype mismatch")
            if p16 is not None and (p16[i].numel() != p.numel() or p16[i].dtype != p16[0].dtype):
                raise ValueError("LambApplyPlan: shape/dtype mismatch")
        if ps:
            if p16 is not None:
                if ps[0].dtype != torch.float32 or \
                        p16[0].dtype not in (torch.bfloat16, torch.float16):
                    raise ValueError("LambApplyPlan: fp32 masters and bf16 or f16 parameters")
            elif ps[0].dtype not in (torch.float32, torch.float64):
                raise ValueError("LambApplyPlan: f32 or f64 parameters (bf16 and f16 through "
                                 "their masters)")
        self._keep = (ps, us, p16)
        self.npiece, self.ntensor = len(ps), int(ntensor)
        self.device = ps[0].device if ps else None
        self._plan = None
        if not ps:
            return
        lib = _lib.load()
        dt = int(kungfu_dtype(p16[0] if p16 is not None else ps[0]))
        with torch.cuda.device(self.device):
            self._plan = lib.kf_lamb_apply_create(
                _lib.ptr_array([t.data_ptr() for t in ps]),
                _lib.ptr_array([t.data_ptr() for t in us]),
                None if p16 is None else _lib.ptr_array([t.data_ptr() for t in p16]),
                (ctypes.c_size_t * len(ps))(*[t.numel() for t in ps]),
                (ctypes.c_int * len(ps))(*ts), len(ps), self.ntensor, dt)
        if not self._plan:
            raise _lib.KungFuAMDError("kf_lamb_apply_create failed: %s"
                                      % lib.kf_last_error().decode())

    def run(self, nlr, stream=None, gate=None):
        if not self.npiece:
            return
        if self._plan is None:
            raise ValueError("LambApplyPlan: closed")
        _check_dev([nlr])
        if nlr.dtype != torch.float64 or nlr.numel() != self.ntensor or nlr.device != self.device:
            raise ValueError("LambApplyPlan.run: nlr must be %d float64 values on %s"
                             % (self.ntensor, self.device))
        if gate is not None:
            _check_gate(gate)
            rc = _lib.load().kf_lamb_apply_run_gated(self._plan, nlr.data_ptr(), gate.data_ptr(),
                                                     _stream(stream, self.device))
            _lib.check(rc, "kf_lamb_apply_run_gated", source="")
            return
        rc = _lib.load().kf_lamb_apply_run(self._plan, nlr.data_ptr(),
                                           _stream(stream, self.device))
        _lib.check(rc, "kf_lamb_apply_run", source="")

    def close(self):
        if self._plan is not None:
            _lib.load().kf_lamb_apply_destroy(self._plan)
            self._plan = None
            self._keep = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# -- LARS (include/kungfu_amd.h "LARS") --

LARS_COEF = _lib.LARS_COEF_DOUBLES


def lars_trust_update_(sq, world, group_of, groups, coef, ratio, np_=0, stream=None):
    """The coefficient rows of T = group_of.numel() tensors on the device
    (kf_lars_trust_update): sq is world * 2 * T float64 sums of squares,
    sq[r * 2T + t] of rank r's piece of tensor t's parameters and
    sq[r * 2T + T + t] of its reduced gradient before the / np_; group_of an
    int32 device tensor (tensor -> group); groups[j] a dict with lr, momentum,
    dampening, weight_decay, nesterov, trust_coefficient, eps, first and
    adapt. Writes coef[6t:6t + 6] = (ratio, weight_decay, momentum,
    1 - dampening, -lr, flags) and ratio[t], where ratio =
    tc * ||p|| / (||g|| / np_ + wd * ||p|| + eps), or 1 where adapt is off or
    a norm is not > 0. No host sync."""
    groups = list(groups)
    _check_dev([sq, group_of, coef, ratio])
    T = group_of.numel()
    if group_of.dtype != torch.int32 or T < 1 or not groups:
        raise ValueError("lars_trust_update_: group_of is a non-empty int32 tensor, and at least "
                         "one group")
    if sq.dtype != torch.float64 or sq.numel() != int(world) * 2 * T or int(world) < 1:
        raise ValueError("lars_trust_update_: sq is world * 2 * T float64 values")
    if coef.dtype != torch.float64 or coef.numel() != LARS_COEF * T or \
            ratio.dtype != torch.float64 or ratio.numel() != T:
        raise ValueError("lars_trust_update_: coef is %d * T and ratio T float64 values"
                         % LARS_COEF)
    rc = _lib.load().kf_lars_trust_update(
        sq.data_ptr(), int(world), T, group_of.data_ptr(), _lib.lars_group_array(groups),
        len(groups), int(np_), coef.data_ptr(), ratio.data_ptr(), _stream(stream, sq.device))
    _lib.check(rc, "kf_lars_trust_update", source="")
    return coef


class LarsApplyPlan:
    """LARS's fused momentum update over "tensor ∩ own shard" pieces
    (kf_lars_apply_*): built once over views that never move, run(coef, np_)
    is one launch whatever the number of pieces. Per element of piece i, with
    the scalars of row tensors[i] of coef (lars_trust_update_'s):

      g = grads[i] / np_;  wd != 0: g += wd * p;  g *= ratio
      momentum != 0: m = first ? g : mu * m + (1 - dampening) * g
                     g = nesterov ? g + mu * m : m
      params[i] += -lr * g

    in the pieces' f32 / f64. With params16 (bf16 or f16 views of the same
    lengths) params are the fp32 master pieces, moms fp32, grads of the 16-bit
    type, and params16[i] = params[i] narrowed, round-to-nearest-even. Pieces
    are aligned to the element only; a piece's tensors must share their
    element offset from a 16-byte boundary. A piece may be empty. The
    gradients are only read; a piece whose row has momentum 0 leaves its moms
    alone. The plan keeps the tensors alive."""

    def __init__(self, params, grads, moms, tensors, ntensor, params16=None):
        ps, gs, ms, ts = list(params), list(grads), list(moms), [int(t) for t in tensors]
        p16 = None if params16 is None else list(params16)
        if not (len(ps) == len(gs) == len(ms) == len(ts)) or \
                (p16 is not None and len(p16) != len(ps)):
            raise ValueError("LarsApplyPlan: one gradient, momentum and tensor index per piece")
        _check_dev(ps + gs + ms + (p16 or []))
        for i, (p, g, m) in enumerate(zip(ps, gs, ms)):
            if p.dtype != ps[0].dtype or m.dtype != p.dtype or g.dtype != gs[0].dtype or \
                    g.numel() != p.numel() or m.numel() != p.numel():
                raise ValueError("LarsApplyPlan: shape/dtype mismatch")
            if p16 is not None and (p16[i].numel() != p.numel() or p16[i].dtype != gs[0].dtype):
                raise ValueError("LarsApplyPlan: shape/dtype mismatch")
        if ps:
            if p16 is not None:
                if ps[0].dtype != torch.float32 or \
                        gs[0].dtype not in (torch.bfloat16, torch.float16):
                    raise ValueError("LarsApplyPlan: fp32 masters and momentum, bf16 or f16 "
                                     "gradients and parameters")
            elif ps[0].dtype not in (torch.float32, torch.float64) or gs[0].dtype != ps[0].dtype:
                raise ValueError("LarsApplyPlan: f32 or f64 parameters (bf16 and f16 through "
                                 "their masters)")
        self._keep = (ps, gs, ms, p16)
        self.npiece, self.ntensor = len(ps), int(ntensor)
        self.device = ps[0].device if ps else None
        self._plan = None
        if not ps:
            return
        lib = _lib.load()
        dt = int(kungfu_dtype(gs[0]))
        with torch.cuda.device(self.device):
            self._plan = lib.kf_lars_apply_create(
                _lib.ptr_array([t.data_ptr() for t in ps]),
                _lib.ptr_array([t.data_ptr() for t in gs]),
                _lib.ptr_array([t.data_ptr() for t in ms]),
                None if p16 is None else _lib.ptr_array([t.data_ptr() for t in p16]),
                (ctypes.c_size_t * len(ps))(*[t.numel() for t in ps]),
                (ctypes.c_int * len(ps))(*ts), len(ps), self.ntensor, dt)
        if not self._plan:
            raise _lib.KungFuAMDError("kf_lars_apply_create failed: %s"
                                      % lib.kf_last_error().decode())

    def run(self, coef, np_=0, stream=None):
        if not self.npiece:
            return
        if self._plan is None:
            raise ValueError("LarsApplyPlan: closed")
        _check_dev([coef])
        if coef.dtype != torch.float64 or coef.numel() != LARS_COEF * self.ntensor or \
                coef.device != self.device:
            raise ValueError("LarsApplyPlan.run: coef must be %d float64 values on %s"
                             % (LARS_COEF * self.ntensor, self.device))
        rc = _lib.load().kf_lars_apply_run(self._plan, coef.data_ptr(), int(np_),
                                           _stream(stream, self.device))
        _lib.check(rc, "kf_lars_apply_run", source="")

    def close(self):
        if self._plan is not None:
            _lib.load().kf_lars_apply_destroy(self._plan)
            self._plan = None
            self._keep = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def lars_apply_plan(params, grads, moms, tensors, ntensor, params16=None):
    """A LarsApplyPlan: run(coef, np_) is the one apply launch."""
    return LarsApplyPlan(params, grads, moms, tensors, ntensor, params16)


def lars_apply_tile(dtype):
    """Elements of one block's tile in the apply launch for parameters of
    `dtype` (kf_lars_apply_tile)."""
    return int(_lib.load().kf_lars_apply_tile(int(kungfu_dtype(torch.empty(0, dtype=dtype)))))


_NORM_DTYPES = (torch.float32, torch.float16, torch.bfloat16, torch.float64)


class SegNorm:
    """Squared norms of many tensors in one pass (kf_segnorm_*): a plan over
    a list of tensors, or of (a, b) tensor pairs, of one float dtype on one
    GPU. The plan keeps the tensors alive and reads them where they are on
    every run, so build it once over views that never move (bucket views).

    run(mode) returns a device fp64 tensor of nseg + 1 values:
      "sq"   out[s] = sum a_s[i]^2
      "var"  out[s] = sum d_i^2, d_i = fl(a_s[i] - fl(b_s[i] * b_s[i])) in the
             tensors' dtype (needs pairs)
      out[nseg] = out[0] + ... + out[nseg - 1] left to right, or with
      total_sqrt=True the sum of sqrt(out[s]).
    fp64 accumulation, |out[s] - exact| <= (n_s + 2) * 2^-53 * exact, the same
    bits on every run of the same bytes. Nothing is allocated and the host is
    not synchronised once `out` is given, so a run can be captured into a
    graph. Runs of one plan on two streams at once are the caller's to order
    (one workspace per plan)."""

    MODES = {"sq": _lib.NORM_SQ, "var": _lib.NORM_VAR}

    def __init__(self, tensors):
        tensors = list(tensors)
        if not tensors:
            raise ValueError("SegNorm: at least one segment")
        paired = isinstance(tensors[0], (tuple, list))
        a = [t[0] for t in tensors] if paired else tensors
        b = [t[1] for t in tensors] if paired else None
        _check_dev(a + (b or []))
        first = a[0]
        if first.dtype not in _NORM_DTYPES:
            raise TypeError("SegNorm: unsupported dtype %s" % first.dtype)
        for t in a + (b or []):
            if t.dtype != first.dtype or t.device != first.device:
                raise ValueError("SegNorm: one dtype and one device per plan")
        if b is not None:
            for x, y in zip(a, b):
                if x.numel() != y.numel():
                    raise ValueError("SegNorm: a pair's tensors differ in length")
        self._keep = (a, b)
        self.nseg = len(a)
        self.paired = paired
        self.device = first.device
        self.counts = [t.numel() for t in a]
        lib = _lib.load()
        cnt = (ctypes.c_size_t * self.nseg)(*self.counts)
        with torch.cuda.device(self.device):
            self._plan = lib.kf_segnorm_create(
                _lib.ptr_array([t.data_ptr() for t in a]),
                _lib.ptr_array([t.data_ptr() for t in b]) if paired else None,
                cnt, self.nseg, int(kungfu_dtype(first)))
        if not self._plan:
            raise _lib.KungFuAMDError("kf_segnorm_create failed: %s"
                                      % lib.kf_last_error().decode())

    def run(self, mode="sq", out=None, stream=None, total_sqrt=False):
        if self._plan is None:
            raise ValueError("SegNorm: closed")
        m = self.MODES[mode] if isinstance(mode, str) else int(mode)
        if total_sqrt:
            m |= _lib.NORM_TOTAL_SQRT
        if out is None:
            out = torch.empty(self.nseg + 1, dtype=torch.float64, device=self.device)
        else:
            _check_dev([out])
            if (out.dtype != torch.float64 or out.numel() != self.nseg + 1
                    or out.device != self.device):
                raise ValueError("SegNorm.run: out must be %d float64 values on %s"
                                 % (self.nseg + 1, self.device))
        rc = _lib.load().kf_segnorm_run(self._plan, m, out.data_ptr(),
                                        _stream(stream, self.device))
        _lib.check(rc, "kf_segnorm_run", source="")
        return out

    def close(self):
        if self._plan is not None:
            _lib.load().kf_segnorm_destroy(self._plan)
            self._plan = None
            self._keep = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def noise_scale_update_(sq_small, sq_big, batch_small, batch_big, alpha, state, stream=None):
    """One update of the gradient noise scale's running estimate on the device
    (kf_noise_scale_update: monitor.py:10-17 and the NoiseScale op, in fp32).
    sq_small, sq_big: fp64 device scalars (|g_local|^2, |g_averaged|^2);
    state: 4 fp32 device values {g_ema, s_ema, noise_scale, has_value}, all
    zero before the first update. Returns state."""
    _check_dev([sq_small, sq_big, state])
    if sq_small.dtype != torch.float64 or sq_big.dtype != torch.float64 or \
            sq_small.numel() != 1 or sq_big.numel() != 1:
        raise ValueError("noise_scale_update_: sq_small and sq_big are fp64 scalars")
    if state.dtype != torch.float32 or state.numel() != 4:
        raise ValueError("noise_scale_update_: state is 4 float32 values")
    rc = _lib.load().kf_noise_scale_update(sq_small.data_ptr(), sq_big.data_ptr(),
                                           float(batch_small), float(batch_big), float(alpha),
                                           state.data_ptr(), _stream(stream, state.device))
    _lib.check(rc, "kf_noise_scale_update", source="")
    return state
