"""numpy restatement of the gradient monitors' semantics (include/kungfu_amd.h
"gradient monitors"), the yardstick of tests/test_monitor*.py.

  exact_sq      sum of squares, correctly rounded from the exact sum
                (math.fsum over fp64 squares: exact for <= 24-bit significands)
  var_terms     d = fl_T(a - fl_T(b * b)) in the tensors' dtype T
                (square_grad - tf.square(grad), grad_variance.py:51-54)
  noise_scale_step  monitor.py:10-17, ema.hpp:19-27, collective.cpp:298-300
                in fp32

bf16 arrays travel as uint16 bit patterns (oracle.f32_to_bf16_bits /
bf16_bits_to_f32); f16, f32 and f64 as numpy's own types.
"""
import math

import numpy as np

from oracle.oracle import bf16_bits_to_f32, f32_to_bf16_bits

U = 2.0 ** -53


def widen(x, dt):
    """The values of `x` as fp64 (exact for every dtype here)."""
    if dt == "bf16":
        return bf16_bits_to_f32(x).astype(np.float64)
    return np.asarray(x).astype(np.float64)


def exact_sq(x, dt):
    """sum x[i]^2; an inf or NaN element gives inf or NaN as IEEE would."""
    w = widen(x, dt)
    if w.size == 0:
        return 0.0
    if not np.isfinite(w).all():
        return float("nan") if np.isnan(w).any() else float("inf")
    return math.fsum((w * w).tolist())


def var_terms(a, b, dt):
    """d[i] = fl_T(a[i] - fl_T(b[i] * b[i])), returned in T's representation."""
    if dt == "bf16":
        fb = bf16_bits_to_f32(b)
        p = bf16_bits_to_f32(f32_to_bf16_bits(fb * fb))
        return f32_to_bf16_bits(bf16_bits_to_f32(a) - p)
    t = {"f16": np.float16, "f32": np.float32, "f64": np.float64}[dt]
    a, b = np.asarray(a, dtype=t), np.asarray(b, dtype=t)
    with np.errstate(over="ignore", invalid="ignore"):
        return (a - (b * b).astype(t)).astype(t)


def exact_var(a, b, dt):
    return exact_sq(var_terms(a, b, dt), dt)


def bound(n):
    """Relative error allowed for one segment of n elements."""
    return (n + 2) * U


def total_sqrt_bound(counts):
    """Relative error allowed for sum_s sqrt(out[s]): the sqrt halves a
    relative error and adds one rounding, the sum adds at most nseg."""
    return (max(counts) + len(counts) + 2) * U


def left_sum(values):
    tot = np.float64(0.0)
    for v in values:
        tot = np.float64(tot + np.float64(v))
    return tot


def noise_scale_step(state, sq_small, sq_big, bs, bb, alpha):
    """One kf_noise_scale_update: state is 4 fp32 values {g_ema, s_ema,
    noise_scale, has_value}; returns the new state (fp32 array)."""
    f = np.float32
    one = f(1.0)
    with np.errstate(all="ignore"):
        Gs, Gb = f(np.float64(sq_small)), f(np.float64(sq_big))
        bs, bb, alpha = f(bs), f(bb), f(alpha)
        G = f(f(one / f(bb - bs)) * f(f(bb * Gb) - f(bs * Gs)))
        S = f(f(one / f(f(one / bs) - f(one / bb))) * f(Gs - Gb))
        g, s = G, S
        if state[3] != 0:
            c = f(one - alpha)
            g = f(f(alpha * f(state[0])) + f(c * G))
            s = f(f(alpha * f(state[1])) + f(c * S))
        return np.array([g, s, f(s / g), one], dtype=np.float32)
