"""Graph capture and replay of device work, as tests/test_gpu_parity.py and
tests/test_monitor_gpu.py do it and tests/test_capture_replay_gpu.py does it
for every update entry: the work runs once eagerly on twin buffers (so that
code objects are loaded before capture), is captured on one side stream,
capture is shown to have run nothing, and the graph is replayed. Capture is
single-stream and linear.

Guarded keeps the buffers of one side: every buffer is followed by sentinel
bytes, and whole buffers, sentinels included, are what two sides are compared
by."""
import numpy as np
import torch

SENTINEL = 0x5A
GUARD = 64  # sentinel bytes after every buffer

_TORCH = {np.dtype(np.float32): torch.float32, np.dtype(np.float64): torch.float64,
          np.dtype(np.float16): torch.float16, np.dtype(np.uint16): torch.bfloat16,
          np.dtype(np.uint8): torch.uint8, np.dtype(np.int32): torch.int32,
          np.dtype(np.int16): torch.int16, np.dtype(np.int64): torch.int64}


class Guarded:
    """Device buffers, each 16-byte aligned with GUARD sentinel bytes after it."""

    def __init__(self, device="cuda"):
        self.device = device
        self.wholes, self.sizes, self.names = [], [], []

    def add(self, a, dtype=None, name=""):
        """The numpy array `a` on the device as a flat tensor of `dtype` (by
        default a's own; uint16 holds bf16 bit patterns)."""
        a = np.ascontiguousarray(a).reshape(-1)
        dtype = dtype or _TORCH[a.dtype]
        raw = a.view(np.uint8)
        whole = torch.full((raw.size + GUARD,), SENTINEL, dtype=torch.uint8, device=self.device)
        whole[:raw.size].copy_(torch.from_numpy(raw.copy()))
        assert whole.data_ptr() % 16 == 0
        self.wholes.append(whole)
        self.sizes.append(raw.size)
        self.names.append(name)
        return whole.view(dtype)[:a.size]

    def add_all(self, arrays, dtype=None, name=""):
        return [self.add(a, dtype, "%s[%d]" % (name, i)) for i, a in enumerate(arrays)]

    def bytes(self):
        """Every buffer's bytes, sentinels included (synchronises)."""
        torch.cuda.synchronize()
        return [w.cpu().numpy() for w in self.wholes]

    def check_sentinels(self, where=()):
        for raw, n, name in zip(self.bytes(), self.sizes, self.names):
            assert (raw[n:] == SENTINEL).all(), ("written beyond count", name) + tuple(where)


def host(t, dtype):
    """A flat device tensor's bytes as a numpy array of `dtype`."""
    return t.detach().contiguous().view(torch.uint8).cpu().numpy().view(dtype).copy()


def put(t, a):
    """The numpy array `a`'s bytes into the flat device tensor `t`."""
    raw = np.ascontiguousarray(a).reshape(-1).view(np.uint8)
    assert raw.size == t.numel() * t.element_size()
    if raw.size:
        t.view(torch.uint8).copy_(torch.from_numpy(raw.copy()))


def same_bytes(a, b):
    return len(a) == len(b) and all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def first_difference(a, b, names):
    for x, y, name in zip(a, b, names):
        if x.tobytes() != y.tobytes():
            at = int(np.nonzero(x != y)[0][0])
            return name, at, x.size
    return None


def capture(work):
    """work(stream) queued into a graph on a side stream, which is the current
    stream meanwhile; nothing of it has run when this returns."""
    graph = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            work(s)
    torch.cuda.synchronize()
    return graph


class Twins:
    """Two sides built by make(): objects with `bufs` (a Guarded) and
    work(stream). One runs eagerly on the current stream, the other is
    captured once and replayed; after replay j the eager side has made j calls
    and both hold the same bytes."""

    def __init__(self, make):
        self.eager, self.cap = make(), make()
        self.graph, self.replays, self.calls = None, 0, 0
        assert same_bytes(self.eager.bufs.bytes(), self.cap.bufs.bytes())

    def feed(self, fn):
        """fn(side) on both sides: the coming call's inputs."""
        fn(self.eager)
        fn(self.cap)

    def _call(self):
        self.eager.work(None)
        torch.cuda.synchronize()
        self.calls += 1

    def capture(self):
        self._call()  # the first eager call: code objects are loaded before capture
        before = self.cap.bufs.bytes()
        self.graph = capture(self.cap.work)
        after = self.cap.bufs.bytes()
        assert same_bytes(before, after), \
            ("capture ran something", first_difference(before, after, self.cap.bufs.names))

    def replay(self, where=()):
        self.replays += 1
        while self.calls < self.replays:
            self._call()
        self.graph.replay()
        torch.cuda.synchronize()
        a, b = self.eager.bufs.bytes(), self.cap.bufs.bytes()
        assert same_bytes(a, b), ("replay %d differs from the eager twin" % self.replays,
                                  first_difference(a, b, self.cap.bufs.names)) + tuple(where)
        self.cap.bufs.check_sentinels(("replay", self.replays) + tuple(where))
