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
