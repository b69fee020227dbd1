"""numpy restatement of the sharded LAMB step's rounding definition
(include/kungfu_amd.h "LAMB"); what tests/test_sharded_lamb*.py
measure the device code against.

Every parenthesis is one IEEE operation in the compute type C (f32 or f64;
bf16 / f16 parameters compute in f32 on their fp32 master copy), the sqrt and
the divisions correctly rounded, the scalars computed in Python doubles and
cast once to C:

  pass 1, moments
    g = np > 0 ? g / np : g                     (np a power of two: g * 2^-k)
    m = (b1*m) + (c1*g)                         c1 = 1 - beta1
    v = (b2*v) + (c2*(g*g))                     c2 = 1 - beta2
    d = (sqrt(v) / s2) + eps                    s2 = sqrt(bias_correction2)
    u = rb1 * (m / d)                           rb1 = (C)(1 / bias_correction1)
    weight_decay != 0:  u = u + (wd*p)
  trust, fp64, per tensor t of T
    P = 0; for r in rank order: P = P + sq[r][t]      U likewise from sq[r][T + t]
    wn = sqrt(P); un = sqrt(U)
    ratio = (adapt && wn > 0 && un > 0) ? wn / un : 1
    trust_clip > 0:  ratio = ratio < trust_clip ? ratio : trust_clip
    nlr = -(lr * ratio)
  pass 2, apply
    p = p + ((C)nlr * u)                        master path: p16 = narrow(master)

16-bit arrays travel as uint16 bit patterns.
"""
import math

import numpy as np

from oracle.oracle import bf16_bits_to_f32, f32_to_bf16_bits

COMPUTE = {"f32": np.float32, "f64": np.float64}
_QUIET = dict(over="ignore", invalid="ignore", under="ignore", divide="ignore")


def hyper(lr, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.0, step=1, adapt=None):
    return {"lr": lr, "betas": betas, "eps": eps, "weight_decay": weight_decay, "step": step,
            "decoupled": False, "adapt": weight_decay != 0 if adapt is None else adapt}


def widen16(bits, dt):
    """bf16 / f16 bit patterns -> f32 (exact)."""
    bits = np.ascontiguousarray(bits, np.uint16)
    return bf16_bits_to_f32(bits) if dt == "bf16" else bits.view(np.float16).astype(np.float32)


def narrow16(x, dt):
    """f32 -> bf16 / f16 bit patterns, round-to-nearest-even."""
    x = np.ascontiguousarray(x, np.float32)
    with np.errstate(**_QUIET):
        return f32_to_bf16_bits(x) if dt == "bf16" else x.astype(np.float16).view(np.uint16)


def moments(p, g, m, v, dt, h, np_=0):
    """Pass 1 on arrays of the compute type dt ("f32" / "f64"; a 16-bit
    gradient comes widened). Returns (m', v', u) as new arrays."""
    C = COMPUTE[dt]
    p, g, m, v = (np.asarray(x, C) for x in (p, g, m, v))
    beta1, beta2 = (float(b) for b in h.get("betas", (0.9, 0.999)))
    wd, t = float(h.get("weight_decay", 0.0)), int(h["step"])
    bc1, bc2 = 1.0 - beta1 ** t, 1.0 - beta2 ** t
    b1, c1, b2, c2 = C(beta1), C(1.0 - beta1), C(beta2), C(1.0 - beta2)
    s2, eps, rb1 = C(math.sqrt(bc2)), C(float(h.get("eps", 1e-8))), C(1.0 / bc1)
    with np.errstate(**_QUIET):
        if np_ > 0:
            g = g * C(1.0 / np_) if np_ & (np_ - 1) == 0 else g / C(np_)
        m = (b1 * m) + (c1 * g)
        v = (b2 * v) + (c2 * (g * g))
        d = (np.sqrt(v) / s2) + eps
        u = rb1 * (m / d)
        if wd != 0:
            u = u + (C(wd) * p)
    return m, v, u


def sq_sum(a):
    """The host's stand-in for one segment's fp64 sum of squares."""
    with np.errstate(**_QUIET):
        return float(np.sum(np.square(np.asarray(a, np.float64))))


def trust(sq, lrs, adapts, trust_clip=0.0):
    """sq: [world][2T] sums of squares (rank r's piece of tensor t's
    parameters at [r][t], of its update at [r][T + t]); lrs / adapts: per
    tensor. Returns (nlr, ratio) as float64 arrays of T."""
    sq = np.asarray(sq, np.float64)
    T = sq.shape[1] // 2
    nlr, ratio = np.zeros(T), np.zeros(T)
    with np.errstate(**_QUIET):
        for t in range(T):
            P, U = np.float64(0.0), np.float64(0.0)
            for r in range(sq.shape[0]):
                P = P + sq[r][t]
                U = U + sq[r][T + t]
            wn, un = np.sqrt(P), np.sqrt(U)
            x = wn / un if (adapts[t] and wn > 0 and un > 0) else np.float64(1.0)
            if trust_clip and trust_clip > 0:
                x = x if x < trust_clip else np.float64(trust_clip)
            ratio[t] = x
            nlr[t] = -(np.float64(lrs[t]) * x)
    return nlr, ratio


def apply(p, u, nlr, dt):
    """Pass 2 on one piece: p + ((C)nlr * u), a new array."""
    C = COMPUTE[dt]
    with np.errstate(**_QUIET):
        return np.asarray(p, C) + (C(nlr) * np.asarray(u, C))


def step_tensors(ps, gs, ms, vs, dt, hs, cuts, trust_clip=0.0, np_=0, sums=None):
    """One whole step on unsharded flat tensors of the compute type:
    ps / gs / ms / vs and hs (a hyper per tensor) are lists of T; cuts[t] is
    the list, in rank order, of (start, stop) of tensor t's piece on every
    rank (start == stop where the rank holds none), over which the norm sums
    are taken per shard and added in rank order. sums: [world][2T] sums to
    use in place of sq_sum's (a device's own). Returns (ps', ms', vs',
    ratios)."""
    T, world = len(ps), len(cuts[0]) if cuts else 1
    new_m, new_v, us = [], [], []
    for p, g, m, v, h in zip(ps, gs, ms, vs, hs):
        m2, v2, u = moments(p, g, m, v, dt, h, np_)
        new_m.append(m2)
        new_v.append(v2)
        us.append(u)
    if sums is None:
        sums = np.zeros((world, 2 * T))
        for t in range(T):
            for r, (a, b) in enumerate(cuts[t]):
                sums[r][t] = sq_sum(np.asarray(ps[t], COMPUTE[dt])[a:b])
                sums[r][T + t] = sq_sum(us[t][a:b])
    nlr, ratio = trust(sums, [h["lr"] for h in hs], [h["adapt"] for h in hs], trust_clip)
    new_p = [apply(p, u, nlr[t], dt) for t, (p, u) in enumerate(zip(ps, us))]
    return new_p, new_m, new_v, ratio
