"""numpy restatement of the sharded SGD update's rounding definition
(include/kungfu_amd.h kf_sgd_update_batch); what
tests/test_sharded_sgd*.py measure the device code against.

torch.optim.SGD's single-tensor path, one IEEE operation per step:

    g = np > 0 ? sum / np : sum        (np a power of two: sum * 2^-k)
    if wd != 0:  g = g + wd*p
    if mu != 0:  m = first ? g : (mu*m) + (c*g)        c = 1 - dampening
                 g = nesterov ? g + mu*m : m
    p = p + nlr*g                                      nlr = -lr

f32 / f64: every product and every sum rounded in that type. f16 / bf16:
computed in fp32 and rounded to the storage type after the /np, the
weight-decay add, mu*m, the momentum add, the nesterov add and the final add;
the alpha*x product and the add inside each are two fp32 roundings. Scalars
are computed in double and cast once to the compute type.

bf16 arrays travel as uint16 bit patterns (oracle.f32_to_bf16_bits /
bf16_bits_to_f32); f16, f32 and f64 as numpy's own types.
"""
import numpy as np

from oracle.oracle import bf16_bits_to_f32, f32_to_bf16_bits

STORAGE = {"f32": np.float32, "f64": np.float64, "f16": np.float16, "bf16": np.uint16}


def _codec(dt):
    """(widen to the compute type, narrow to storage, compute type)."""
    if dt == "bf16":
        return bf16_bits_to_f32, f32_to_bf16_bits, np.float32
    if dt == "f16":
        return (lambda a: np.asarray(a, np.float16).astype(np.float32),
                lambda x: x.astype(np.float16), np.float32)
    t = STORAGE[dt]
    return (lambda a: np.asarray(a, t)), (lambda x: x.astype(t)), t


def hyper(lr, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False, first=False):
    return {"lr": lr, "momentum": momentum, "dampening": dampening,
            "weight_decay": weight_decay, "nesterov": nesterov, "first": first}


def step(p, g, m, dt, h, np_=0):
    """One update. p, g, m: arrays in dt's representation (m may be None when
    momentum is 0). Returns (p', m') as new arrays; m' is m itself (or None)
    when momentum is 0."""
    widen, narrow, C = _codec(dt)
    R = lambda x: widen(narrow(x))  # noqa: E731  the rounding to storage
    nlr, mu = C(-float(h["lr"])), C(float(h.get("momentum", 0.0)))
    c = C(1.0 - float(h.get("dampening", 0.0)))
    wd = C(float(h.get("weight_decay", 0.0)))
    with np.errstate(over="ignore", invalid="ignore", under="ignore", divide="ignore"):
        pw, gw = widen(p), widen(g)
        if np_ > 0:
            if np_ & (np_ - 1) == 0:
                gw = R(gw * C(1.0 / np_))
            else:
                gw = R(gw / C(np_))
        if wd != 0:
            gw = R(gw + wd * pw)
        mw = None
        if mu != 0:
            if h.get("first", False):
                mw = gw
            else:
                mw = R(R(mu * widen(m)) + c * gw)
            gw = R(gw + mu * mw) if h.get("nesterov", False) else mw
        pw = R(pw + nlr * gw)
        return narrow(pw), (narrow(mw) if mw is not None else m)
