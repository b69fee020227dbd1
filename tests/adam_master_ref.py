"""numpy restatement of the Adam / AdamW update with fp32 master weights and
fp32 state for 16-bit parameters (include/kungfu_amd.h
kf_adam_master_update_batch); what
tests/test_sharded_adam_master*.py measure the device code against.

    g = widen(g16)                                   exact
    (master, m, v) = adam_ref.step(master, g, m, v, "f32", h, np_)
    p16 = narrow(master)                             round-to-nearest-even

The fp32 arithmetic is adam_ref's f32 path, untouched: the /np is the fp32 one
and nothing else is rounded to 16 bits.

bf16 arrays travel as uint16 bit patterns (oracle.f32_to_bf16_bits /
bf16_bits_to_f32), f16 arrays as numpy's float16; master, m and v as float32.
"""
import numpy as np

import adam_ref
from oracle.oracle import bf16_bits_to_f32, f32_to_bf16_bits

STORAGE = {"bf16": np.uint16, "f16": np.float16}


def widen(a, dt):
    """16-bit storage -> float32, exact."""
    if dt == "bf16":
        return bf16_bits_to_f32(np.asarray(a, np.uint16))
    return np.asarray(a, np.float16).astype(np.float32)


def narrow(x, dt):
    """float32 -> 16-bit storage, round-to-nearest-even."""
    x = np.asarray(x, np.float32)
    if dt == "bf16":
        return f32_to_bf16_bits(x)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        return x.astype(np.float16)


def step(master, g16, m, v, dt, h, np_=0):
    """One update. master, m, v: float32 arrays; g16: the summed gradient in
    dt's representation. Returns (p16', master', m', v') as new arrays."""
    w, m, v = adam_ref.step(np.asarray(master, np.float32), widen(g16, dt),
                            np.asarray(m, np.float32), np.asarray(v, np.float32), "f32", h, np_)
    return narrow(w, dt), w, m, v
