"""Pure-Python model of the pair-averaging model store (include/kungfu_amd.h
"pair averaging") and the numpy yardstick of its blend; what
tests/test_pairavg*.py measure the device code against.

The protocol model: a Store holds `latest`, one seqlock per slot and the slot
contents. A Writer publishes version n (counted from 1) into slot n % S in
phases begin, copy and end, the copy split into two halves so that a reader
can meet a half-written slot. A Reader pulls in phases pick, fetch and check.
Every phase is atomic; a test interleaves them.

  blend(v, o, dt)   fl_T(0.5 * fl_T(v + o)) in the tensors' dtype T
                    (TF's 0.5 * (v + other_v), async_sgd.py:130-133); f16 and
                    bf16 go through fp32 and round to T after the add and
                    after the multiply.

bf16 arrays travel as uint16 bit patterns (oracle.f32_to_bf16_bits /
bf16_bits_to_f32); f16, f32 and f64 as numpy's own types.
"""
import numpy as np

from oracle.oracle import bf16_bits_to_f32, f32_to_bf16_bits

VALID, TORN, EMPTY = "valid", "torn", "empty"


class Store:
    def __init__(self, slots, width=4):
        self.S = slots
        self.width = width
        self.latest = 0
        self.lock = [0] * slots
        self.slot = [[0] * width for _ in range(slots)]
        self.published = 0


class Writer:
    """Version n's content is a vector of all n."""

    def __init__(self, store):
        self.st = store

    def _n(self):
        return self.st.published + 1

    def begin(self):
        self.st.lock[self._n() % self.st.S] += 1

    def copy(self, half=None):
        """half None: the whole slot; 0 / 1: its first / second half."""
        n, w = self._n(), self.st.width
        lo, hi = {None: (0, w), 0: (0, w // 2), 1: (w // 2, w)}[half]
        for i in range(lo, hi):
            self.st.slot[n % self.st.S][i] = n

    def end(self):
        n = self._n()
        self.st.lock[n % self.st.S] += 1
        self.st.latest = n
        self.st.published = n

    def publish(self):
        self.begin()
        self.copy()
        self.end()

    def phases(self):
        """One publish as its four atomic steps (the copy in halves)."""
        return [self.begin, lambda: self.copy(0), lambda: self.copy(1), self.end]


class Reader:
    def __init__(self, store):
        self.st = store
        self.state = None  # after pick: None (picked), EMPTY or TORN
        self.slot = self.lock0 = self.version = None
        self.staging = None
        self.outcome = None
        self.counters = {VALID: 0, TORN: 0, EMPTY: 0}

    def pick(self):
        v0 = self.st.latest
        s = v0 % self.st.S
        l0 = self.st.lock[s]
        self.slot, self.lock0, self.version = s, l0, v0
        self.state = EMPTY if v0 == 0 else (TORN if l0 & 1 else None)
        self.outcome = None

    def fetch(self):
        if self.state is None:
            self.staging = list(self.st.slot[self.slot])

    def check(self):
        if self.state is not None:
            self.outcome = self.state
        else:
            self.outcome = VALID if self.st.lock[self.slot] == self.lock0 else TORN
        self.counters[self.outcome] += 1
        return self.outcome

    def phases(self):
        return [self.pick, self.fetch, self.check]


def blend(v, o, dt):
    """fl_T(0.5 * fl_T(v + o)), returned in T's representation."""
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        if dt == "bf16":
            s = bf16_bits_to_f32(f32_to_bf16_bits(bf16_bits_to_f32(v) + bf16_bits_to_f32(o)))
            return f32_to_bf16_bits(np.float32(0.5) * s)
        if dt == "f16":
            v, o = np.asarray(v, np.float16), np.asarray(o, np.float16)
            s = (v.astype(np.float32) + o.astype(np.float32)).astype(np.float16)
            return (np.float32(0.5) * s.astype(np.float32)).astype(np.float16)
        t = {"f32": np.float32, "f64": np.float64}[dt]
        v, o = np.asarray(v, t), np.asarray(o, t)
        return (t(0.5) * (v + o).astype(t)).astype(t)
