"""numpy restatement of the sharded LARS step's rounding definition
(include/kungfu_amd.h "LARS"); what tests/test_sharded_lars*.py
measure the device code against. tests/sgd_ref.py's conventions: every
parenthesis is one IEEE operation in the compute type C (f32 or f64; f32 on the
master copy of bf16 / f16 parameters), scalars computed in double, cast once:

  trust, fp64, per tensor t of T
    P = 0; for r in rank order: P = P + sq[r][t]      G likewise from sq[r][T + t]
    wn = sqrt(P); gn = np > 0 ? sqrt(G) / np : sqrt(G)
    ratio = (adapt && wn > 0 && gn > 0) ? (tc*wn) / ((gn + (wd*wn)) + eps) : 1
    coef[t] = (ratio, wd, mu, c = 1 - dampening, nlr = -lr, flags)
    flags: 1 momentum != 0, 2 nesterov, 4 first
  apply, per element
    g = np > 0 ? g / np : g                     (np a power of two: g * 2^-k)
    wd != 0:        g = g + (wd*p)
    g = ratio * g
    momentum != 0:  m = first ? g : (mu*m) + (c*g)
                    g = nesterov ? g + (mu*m) : m
    p = p + (nlr*g)
16-bit arrays travel as uint16 bit patterns (lamb_ref.widen16 / narrow16).
"""
import numpy as np

from lamb_ref import COMPUTE, narrow16, sq_sum, widen16  # noqa: F401  (the tests' codecs)

MOMENTUM, NESTEROV, FIRST = 1, 2, 4


def hyper(lr, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False, first=False,
          trust_coefficient=0.001, eps=1e-8, adapt=None):
    return {"lr": lr, "momentum": momentum, "dampening": dampening, "weight_decay": weight_decay,
            "nesterov": nesterov, "first": first, "trust_coefficient": trust_coefficient,
            "eps": eps, "adapt": weight_decay != 0 if adapt is None else adapt}


def trust(sq, hs, np_=0):
    """sq: [world][2T] sums of squares (rank r's piece of tensor t's parameters
    at [r][t], of its reduced gradient at [r][T + t]); hs: a hyper per tensor.
    Returns coef, a float64 array [T][6]."""
    sq = np.asarray(sq, np.float64)
    T = sq.shape[1] // 2
    coef = np.zeros((T, 6))
    with np.errstate(all="ignore"):
        for t, h in enumerate(hs):
            P, G = np.float64(0.0), np.float64(0.0)
            for r in range(sq.shape[0]):
                P = P + sq[r][t]
                G = G + sq[r][T + t]
            wn, gn = np.sqrt(P), np.sqrt(G)
            if np_ > 0:
                gn = gn / np.float64(np_)
            wd, x = np.float64(h["weight_decay"]), np.float64(1.0)
            if h["adapt"] and wn > 0 and gn > 0:
                x = (np.float64(h["trust_coefficient"]) * wn) / ((gn + (wd * wn)) + np.float64(h["eps"]))
            flags = (MOMENTUM if h["momentum"] != 0 else 0) | (NESTEROV if h["nesterov"] else 0) | \
                (FIRST if h["first"] else 0)
            coef[t] = (x, wd, h["momentum"], 1.0 - h["dampening"], -h["lr"], flags)
    return coef


def apply(p, g, m, row, dt, np_=0):
    """One piece: p, g, m arrays of the compute type dt ("f32" / "f64"; a
    16-bit gradient comes widened), row a tensor's 6 coefficients. Returns
    (p', m') as new arrays; m' is m itself where the row's momentum is 0."""
    C = COMPUTE[dt]
    p, g = np.asarray(p, C), np.asarray(g, C)
    ratio, wd, mu, c, nlr = (C(x) for x in row[:5])
    flags = int(row[5])
    with np.errstate(all="ignore"):
        if np_ > 0:
            g = g * C(1.0 / np_) if np_ & (np_ - 1) == 0 else g / C(np_)
        if wd != 0:
            g = g + (wd * p)
        g = ratio * g
        if flags & MOMENTUM:
            m = g if flags & FIRST else (mu * np.asarray(m, C)) + (c * g)
            g = g + (mu * m) if flags & NESTEROV else m
        return p + (nlr * g), m


def step_tensors(ps, gs, ms, dt, hs, np_=0, sums=None):
    """One whole step on unsharded flat tensors of the compute type: ps / gs /
    ms and hs (a hyper per tensor) are lists of T; gs are the reduced gradients
    before the / np_. sums: the [world][2T] gathered sums of squares to use in
    place of the whole tensors' own. Returns (ps', ms', ratios)."""
    if sums is None:
        sums = [[sq_sum(np.asarray(a, COMPUTE[dt])) for a in list(ps) + list(gs)]]
    coef = trust(sums, hs, np_)
    new = [apply(p, g, m, coef[t], dt, np_) for t, (p, g, m) in enumerate(zip(ps, gs, ms))]
    return [a for a, _ in new], [b for _, b in new], coef[:, 0].copy()
