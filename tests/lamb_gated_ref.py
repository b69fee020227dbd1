"""numpy restatement of the LAMB step under a gate (include/kungfu_amd.h "LAMB
under a gate"), composed from tests/lamb_ref.py and
tests/step_gate_ref.py; what tests/test_sharded_lamb_gated*.py measure the
device code against.

The verdict is step_gate_ref.gate_update, unchanged, called with every group's
lr = 1 (`verdict`): the state's nss is then -(1 / (1 - beta1_pow)), and the
moments pass takes rb1 = -nss and s2 from the state (s2_f64 / nss_f64 for f64).

    moments, not skipped:  lamb_ref.moments' /np, then the one inserted
                           operation g = (g * (C)grad_mul), then lamb_ref's
                           remaining operations with the state's s2 and rb1
    trust, not skipped:    lamb_ref.trust
    apply, not skipped:    lamb_ref.apply (master path: p16 = narrow(master))
    skipped:               every array comes back as it went in

lamb_ref.moments takes its bias corrections from a step count and cannot be
handed scalars, so its operations after the /np are restated in `moments`;
tests/test_sharded_lamb_gated.py pins it with grad_mul = 1 and lamb_ref's own
scalars (`scalars_of`) to lamb_ref.moments' bits.
"""
import numpy as np

import lamb_ref
import step_gate_ref

COMPUTE = lamb_ref.COMPUTE
_QUIET = dict(over="ignore", invalid="ignore", under="ignore", divide="ignore")

new_gate, new_state = step_gate_ref.new_gate, step_gate_ref.new_state


def verdict(sq, nps, groups, states, gate, **rule):
    """step_gate_ref.gate_update with every group's lr = 1 (D of the step)."""
    return step_gate_ref.gate_update(sq, nps, [dict(g, lr=1.0) for g in groups], states, gate,
                                     **rule)


def scalars_of(h):
    """The step state lamb_ref.moments' own scalars correspond to: those of
    step_gate_ref.scalars_of at lr = 1."""
    return step_gate_ref.scalars_of(dict(h, lr=1.0))


def no_gate():
    """skip = 0 and grad_mul = 1: a gate that changes nothing."""
    return dict(new_gate(), grad_mul=np.float32(1))


def state_scalars(state, dt):
    """(s2, rb1) as the gated moments kernel reads them, in the compute type."""
    C = COMPUTE[dt]
    if dt == "f64":
        return C(state["s2_f64"]), -C(state["nss_f64"])
    return C(state["s2"]), -C(state["nss"])


def moments(p, g, m, v, u, dt, h, gate, state, np_=0):
    """Pass 1 under a gate on arrays of the compute type dt ("f32" / "f64"; a
    16-bit gradient comes widened). Returns (m', v', u') as new arrays; on a
    skipped step copies of m, v and of the previous u."""
    C = COMPUTE[dt]
    p, g, m, v, u = (np.asarray(x, C) for x in (p, g, m, v, u))
    if gate["skip"]:
        return m.copy(), v.copy(), u.copy()
    beta1, beta2 = (float(b) for b in h.get("betas", (0.9, 0.999)))
    wd = float(h.get("weight_decay", 0.0))
    b1, c1, b2, c2 = C(beta1), C(1.0 - beta1), C(beta2), C(1.0 - beta2)
    eps = C(float(h.get("eps", 1e-8)))
    s2, rb1 = state_scalars(state, dt)
    with np.errstate(**_QUIET):
        if np_ > 0:
            g = g * C(1.0 / np_) if np_ & (np_ - 1) == 0 else g / C(np_)
        g = g * C(np.float32(gate["grad_mul"]))  # the one inserted operation
        m = (b1 * m) + (c1 * g)
        v = (b2 * v) + (c2 * (g * g))
        d = (np.sqrt(v) / s2) + eps
        u = rb1 * (m / d)
        if wd != 0:
            u = u + (C(wd) * p)
    return m, v, u


def trust(sq, lrs, adapts, nlr, ratio, gate, trust_clip=0.0):
    """lamb_ref.trust, or on a skipped step copies of the previous nlr and ratio."""
    if gate["skip"]:
        return np.array(nlr, np.float64), np.array(ratio, np.float64)
    return lamb_ref.trust(sq, lrs, adapts, trust_clip)


def apply(p, u, nlr, dt, gate):
    """lamb_ref.apply on one piece, or on a skipped step a copy of p."""
    if gate["skip"]:
        return np.array(p, COMPUTE[dt])
    return lamb_ref.apply(p, u, nlr, dt)


def apply_master(master, p16, u, nlr, dt16, gate):
    """(master', p16') of one piece on the master path; both unchanged on a skip."""
    if gate["skip"]:
        return np.array(master, np.float32), np.array(p16, np.uint16)
    w = lamb_ref.apply(master, u, nlr, "f32")
    return w, lamb_ref.narrow16(w, dt16)


def step_tensors(ps, gs, ms, vs, us, dt, hs, states, gate, cuts, nlr, ratio, trust_clip=0.0,
                 np_=0, sums=None):
    """E to G on unsharded flat tensors of the compute type, after `verdict`:
    lamb_ref.step_tensors' arguments plus the previous us, nlr and ratio, the
    gate and a step state per tensor. Returns (ps', ms', vs', us', nlr',
    ratio'). sums: [world][2T] sums to use in place of lamb_ref.sq_sum's."""
    T, world = len(ps), len(cuts[0]) if cuts else 1
    new = [moments(p, g, m, v, u, dt, h, gate, st, np_)
           for p, g, m, v, u, h, st in zip(ps, gs, ms, vs, us, hs, states)]
    new_m, new_v, new_u = ([n[i] for n in new] for i in range(3))
    if sums is None:
        sums = np.zeros((world, 2 * T))
        for t in range(T):
            for r, (a, b) in enumerate(cuts[t]):
                sums[r][t] = lamb_ref.sq_sum(np.asarray(ps[t], COMPUTE[dt])[a:b])
                sums[r][T + t] = lamb_ref.sq_sum(new_u[t][a:b])
    nlr, ratio = trust(sums, [h["lr"] for h in hs], [h["adapt"] for h in hs], nlr, ratio, gate,
                       trust_clip)
    new_p = [apply(p, u, nlr[t], dt, gate) for t, (p, u) in enumerate(zip(ps, new_u))]
    return new_p, new_m, new_v, new_u, nlr, ratio
