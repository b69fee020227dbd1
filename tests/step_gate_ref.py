"""numpy restatement of the gated optimizer step (include/kungfu_amd.h
kf_step_gate_update, kf_adam_update_batch_gated,
kf_adam_master_update_batch_gated); what
tests/test_sharded_adam_gated*.py measure the device code against.

The verdict, fp64, one IEEE operation per parenthesis:

    total = 0; for k in plan order:
        s = 0; for r in rank order: s = s + sq[r][k]
        if np_k > 0: s = s / (np_k * np_k)
        total = total + s
    skip      = !isfinite(total)
    grad_norm = sqrt(total) / loss_scale
    clip      = max_norm > 0 ? (x = max_norm / (grad_norm + 1e-6); x < 1 ? x : 1) : 1
    grad_mul  = (float)(clip / loss_scale)

then torch.amp.GradScaler's update of the fp32 loss scale and, unless the step
is skipped, every group's running products, step, s2 and nss.

The gated update: adam_ref.step's /np, the one multiply g = R(g * grad_mul),
then adam_ref.step's remaining operations with the gate's s2 and nss.
adam_ref.step takes its bias corrections from a step count
(1 - beta ** step) and cannot be handed scalars, while the gated path's are
running products the device keeps; so those remaining operations are restated
in `_rest`, and tests/test_sharded_adam_gated.py pins `update` with
grad_mul = 1 and adam_ref's own scalars (`scalars_of`) to adam_ref.step's and
adam_master_ref.step's bits. bf16 arrays travel as uint16 bit patterns, as in
adam_ref.
"""
import math

import numpy as np

import adam_master_ref
import adam_ref

GATE_FIELDS = ("skip", "grad_mul", "loss_scale", "good_steps", "grad_norm", "total", "applied",
               "skipped")
STATE_FIELDS = ("beta1_pow", "beta2_pow", "step", "s2_f64", "nss_f64", "s2", "nss")


def new_gate(loss_scale=1.0):
    return {"skip": 0, "grad_mul": np.float32(0), "loss_scale": np.float32(loss_scale),
            "good_steps": 0, "grad_norm": 0.0, "total": 0.0, "applied": 0, "skipped": 0}


def new_state(step=0, betas=(0.9, 0.999)):
    """Zero-filled with both pows 1, or resumed at `step` with Python's beta ** step."""
    return {"beta1_pow": float(betas[0]) ** step, "beta2_pow": float(betas[1]) ** step,
            "step": step, "s2_f64": 0.0, "nss_f64": 0.0, "s2": np.float32(0), "nss": np.float32(0)}


def gate_update(sq, nps, groups, states, gate, max_norm=0.0, growth_factor=1.0,
                backoff_factor=1.0, growth_interval=0):
    """One verdict, in place on `gate` and `states`. sq[r][k]: rank r's sum of
    squares of plan k; nps[k]; groups[j]: dict with lr and betas."""
    sq = np.asarray(sq, np.float64)
    assert sq.ndim == 2 and sq.shape[1] == len(nps)
    f64 = np.float64
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        total = f64(0)
        for k, n in enumerate(nps):
            s = f64(0)
            for r in range(sq.shape[0]):
                s = s + sq[r][k]
            if n > 0:
                s = s / (f64(n) * f64(n))
            total = total + s
        skip = not np.isfinite(total)
        scale = np.float32(gate["loss_scale"])
        ls = f64(scale)
        norm = np.sqrt(total) / ls
        clip = f64(1)
        if max_norm and max_norm > 0:
            x = f64(max_norm) / (norm + f64(1e-6))
            if x < 1.0:
                clip = x
        gate["total"], gate["skip"], gate["grad_norm"] = float(total), int(skip), float(norm)
        gate["grad_mul"] = np.float32(clip / ls)
        if skip:
            gate["loss_scale"] = np.float32(scale * np.float32(backoff_factor))
            gate["good_steps"] = 0
            gate["skipped"] += 1
        else:
            good = gate["good_steps"] + 1
            if good == growth_interval:
                grown = np.float32(scale * np.float32(growth_factor))
                if np.isfinite(grown):
                    gate["loss_scale"] = grown
                gate["good_steps"] = 0
            else:
                gate["good_steps"] = good
            gate["applied"] += 1
            for g, st in zip(groups, states):
                b1, b2 = (f64(b) for b in g.get("betas", (0.9, 0.999)))
                st["beta1_pow"] = float(f64(st["beta1_pow"]) * b1)
                st["beta2_pow"] = float(f64(st["beta2_pow"]) * b2)
                st["step"] += 1
                st["s2_f64"] = float(np.sqrt(f64(1) - f64(st["beta2_pow"])))
                st["nss_f64"] = float(-(f64(g["lr"]) / (f64(1) - f64(st["beta1_pow"]))))
                st["s2"], st["nss"] = np.float32(st["s2_f64"]), np.float32(st["nss_f64"])
    return gate


def update(p, g, m, v, dt, h, gate, state, np_=0):
    """The gated update of one segment in adam_ref's representation (f32, f64,
    bf16 as uint16 bits). A skipped step returns copies of p, m, v."""
    if gate["skip"]:
        return p.copy(), m.copy(), v.copy()
    widen, narrow, C = adam_ref._codec(dt)
    R = lambda x: widen(narrow(x))  # noqa: E731
    s2 = C(state["s2_f64"] if dt == "f64" else state["s2"])
    nss = C(state["nss_f64"] if dt == "f64" else state["nss"])
    with np.errstate(over="ignore", invalid="ignore", under="ignore", divide="ignore"):
        gw = widen(g)
        if np_ > 0:
            gw = R(gw * C(1.0 / np_)) if np_ & (np_ - 1) == 0 else R(gw / C(np_))
        gw = R(gw * C(np.float32(gate["grad_mul"])))  # the one inserted operation
        return _rest(widen(p), gw, widen(m), widen(v), h, s2, nss, C, R, narrow)


def _rest(pw, gw, mw, vw, h, s2, nss, C, R, narrow):
    """adam_ref.step after its /np, with s2 and nss given (not from a step
    count); test_rest_is_adam_ref pins it to adam_ref.step."""
    lr, (beta1, beta2) = float(h["lr"]), (float(b) for b in h.get("betas", (0.9, 0.999)))
    wd = float(h.get("weight_decay", 0.0))
    b1, c1, b2, c2 = C(beta1), C(1.0 - beta1), C(beta2), C(1.0 - beta2)
    eps = C(float(h.get("eps", 1e-8)))
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


def update_master(master, g16, m, v, dt, h, gate, state, np_=0):
    """The gated update with fp32 master weights: adam_master_ref.step's shape
    around `update`'s f32 path. Returns (p16', master', m', v'), or None for
    p16' on a skipped step (params16 is not written)."""
    if gate["skip"]:
        return None, master.copy(), m.copy(), v.copy()
    w, m, v = update(np.asarray(master, np.float32), adam_master_ref.widen(g16, dt),
                     np.asarray(m, np.float32), np.asarray(v, np.float32), "f32", h, gate, state,
                     np_)
    return adam_master_ref.narrow(w, dt), w, m, v


def scalars_of(h):
    """The step state adam_ref.step's own scalars correspond to: s2 and nss
    from 1 - beta ** step in Python doubles (adam_scalars on the host)."""
    b1, b2 = (float(b) for b in h.get("betas", (0.9, 0.999)))
    t = int(h["step"])
    s2, nss = math.sqrt(1.0 - b2 ** t), -(float(h["lr"]) / (1.0 - b1 ** t))
    return {"beta1_pow": b1 ** t, "beta2_pow": b2 ** t, "step": t, "s2_f64": s2, "nss_f64": nss,
            "s2": np.float32(s2), "nss": np.float32(nss)}


def sum_sq(arrays, dt=None):
    """The fp64 sum of squares kf_segnorm_run's total gives, up to its
    documented (n + 2) * 2^-53 relative error: for exact tests use inputs
    whose squares sum exactly."""
    tot = 0.0
    for a in arrays:
        x = adam_ref.bf16_bits_to_f32(a) if dt == "bf16" else np.asarray(a)
        with np.errstate(over="ignore", invalid="ignore"):
            tot += float(np.sum(x.astype(np.float64) ** 2))
    return tot
