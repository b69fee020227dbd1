"""Muon restated in numpy (include/kungfu_amd.h "Muon"): the grouped GEMM in
f64, the Newton-Schulz chain in pure f64 or rounding to bf16 wherever the
kernels store, and the optimizer's step on whole buffers."""
import numpy as np

A, B, C = 3.4445, -4.7750, 2.0315


def bf16(x):
    """x (f32 or f64) rounded to the nearest bf16, ties to even, as f64."""
    u = np.asarray(x, np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7fff + ((u >> 16) & 1)) >> 16 << 16
    return u.astype(np.uint32).view(np.float32).astype(np.float64)


def identity(x):
    return np.asarray(x, np.float64)


def gemm_ref(a, b, cin, alpha, beta, trans_a, trans_b):
    """alpha * cin + beta * op(a) @ op(b) in f64, and the magnitude
    |alpha| |cin| + |beta| (|op(a)| @ |op(b)|) the error bound scales with."""
    a, b = (np.asarray(x, np.float64) for x in (a, b))
    a, b = (a.T if trans_a else a), (b.T if trans_b else b)
    c = 0.0 if cin is None else np.asarray(cin, np.float64)
    return alpha * c + beta * (a @ b), abs(alpha) * np.abs(c) + abs(beta) * (np.abs(a) @ np.abs(b))


def newton_schulz(d, steps, store):
    """d (rows x cols, exact in bf16) -> X after `steps` iterations; store is
    applied to X0, A, B and every X (identity, or bf16)."""
    d = np.asarray(d, np.float64)
    # the scale as the kernel takes it: 1 / (sqrt(sum d^2) + 1e-7) in f64, cast to f32
    s = np.float64(np.float32(1.0 / (np.sqrt((d * d).sum()) + 1e-7))) if store is bf16 else \
        1.0 / (np.sqrt((d * d).sum()) + 1e-7)
    x = store(np.float32(d) * np.float32(s)) if store is bf16 else d * s
    tall = d.shape[0] > d.shape[1]
    for _ in range(steps):
        a = store(x.T @ x if tall else x @ x.T)
        b = store(B * a + C * (a @ a))
        x = store(A * x + (x @ b if tall else b @ x))
    return x


def momentum(g, m, mu, nesterov, world):
    """The shard kernel on f32 arrays: -> (m', the direction as bf16 values in f32)."""
    g = np.float32(g) / np.float32(world) if world > 1 else np.float32(g)
    m = np.float32(mu) * np.float32(m) + g
    d = g + np.float32(mu) * m if nesterov else m
    return m.astype(np.float32), bf16(d).astype(np.float32)


def muon_step(params, grads, moms, lr, mu, nesterov, wd, steps, world=1):
    """One step over lists of arrays shaped as the parameters (grads: the
    ranks' f32 sum): -> (params', moms'). The update is the kernel's f32
    arithmetic on the pure-f64 Newton-Schulz result cast to f32 (not narrowed
    to bf16: the kernel's narrowing of X is part of the delta the test allows)."""
    out_p, out_m = [], []
    for p, g, m in zip(params, grads, moms):
        m2, d = momentum(g, m, mu, nesterov, world)
        rows = p.shape[0]
        x = newton_schulz(d.reshape(rows, -1), steps, identity).reshape(p.shape)
        scale = max(1.0, rows / (p.size // rows)) ** 0.5
        dk, nc = np.float32(1.0 - lr * wd), np.float32(-lr * scale)
        out_p.append(dk * np.float32(p) + nc * np.float32(x))
        out_m.append(m2)
    return out_p, out_m
