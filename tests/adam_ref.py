"""numpy restatement of the sharded Adam / AdamW update's rounding definition
(include/kungfu_amd.h kf_adam_update_batch); what
tests/test_sharded_adam*.py measure the device code against.

torch.optim.Adam / AdamW's single-tensor path, each parenthesised operation
one IEEE operation:

    g = np > 0 ? sum / np : sum                 (np a power of two: sum * 2^-k)
    wd != 0, decoupled == 0 (Adam, L2):   g = g + (wd*p)
    wd != 0, decoupled != 0 (AdamW):      p = dk*p              dk = 1 - lr*wd
    m = (b1*m) + (c1*g)                         c1 = 1 - beta1
    v = (b2*v) + (c2*(g*g))                     c2 = 1 - beta2
    d = (sqrt(v) / s2) + eps                    s2 = sqrt(bias_correction2)
    p = p + (nss*(m / d))                       nss = -(lr / bias_correction1)

f32 / f64: every operation rounded in that type. bf16: computed in fp32 and
rounded to bf16 after the /np, after the L2 add or the decay multiply, after
m (once), after b2*v, after the v add, after the sqrt, after the / s2, after
the + eps and after the final add. The scalars, the bias corrections
1 - beta**step among them, are computed in Python doubles and cast once to
the compute type.

bf16 arrays travel as uint16 bit patterns (oracle.f32_to_bf16_bits /
bf16_bits_to_f32); f32 and f64 as numpy's own types.
"""
import math

import numpy as np

from oracle.oracle import bf16_bits_to_f32, f32_to_bf16_bits

STORAGE = {"f32": np.float32, "f64": np.float64, "bf16": np.uint16}


def _codec(dt):
    """(widen to the compute type, narrow to storage, compute type)."""
    if dt == "bf16":
        return bf16_bits_to_f32, f32_to_bf16_bits, np.float32
    t = STORAGE[dt]
    return (lambda a: np.asarray(a, t)), (lambda x: x.astype(t)), t


def hyper(lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, decoupled=False, step=1):
    return {"lr": lr, "betas": betas, "eps": eps, "weight_decay": weight_decay,
            "decoupled": decoupled, "step": step}


def step(p, g, m, v, dt, h, np_=0):
    """One update. p, g, m, v: arrays in dt's representation. Returns
    (p', m', v') as new arrays."""
    widen, narrow, C = _codec(dt)
    R = lambda x: widen(narrow(x))  # noqa: E731  the rounding to storage
    lr, (beta1, beta2) = float(h["lr"]), (float(b) for b in h.get("betas", (0.9, 0.999)))
    wd, t = float(h.get("weight_decay", 0.0)), int(h["step"])
    bc1, bc2 = 1.0 - beta1 ** t, 1.0 - beta2 ** t
    b1, c1, b2, c2 = C(beta1), C(1.0 - beta1), C(beta2), C(1.0 - beta2)
    s2, eps, nss = C(math.sqrt(bc2)), C(float(h.get("eps", 1e-8))), C(-(lr / bc1))
    with np.errstate(over="ignore", invalid="ignore", under="ignore", divide="ignore"):
        pw, gw, mw, vw = widen(p), widen(g), widen(m), widen(v)
        if np_ > 0:
            if np_ & (np_ - 1) == 0:
                gw = R(gw * C(1.0 / np_))
            else:
                gw = R(gw / C(np_))
        if wd != 0:
            if h.get("decoupled", False):
                pw = R(C(1.0 - lr * wd) * pw)
            else:
                gw = R(gw + C(wd) * pw)
        mw = R(b1 * mw + c1 * gw)
        vw = R(R(b2 * vw) + c2 * (gw * gw))
        d = R(R(R(np.sqrt(vw)) / s2) + eps)
        pw = R(pw + nss * (mw / d))
        return narrow(pw), narrow(mw), narrow(vw)
