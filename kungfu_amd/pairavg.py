"""Asynchronous pair averaging (AD-PSGD, the reference's PairAveragingOptimizer,
srcs/python/kungfu/tensorflow/optimizers/async_sgd.py) on the device.

The reference keeps a versioned model store on the host: a step fuses the
model, saves it under a lock, requests a random peer's copy over rchannel,
defuses the reply and runs ``0.5 * (v + other)`` in TF. Here the store lives
in HBM (kf_pairavg_*, kungfu_amd/csrc/kf_pairavg.hip): every rank publishes
whole snapshots of its variable buckets into seqlocked slots that its peers
have mapped through HIP IPC; ``pull_average_`` reads the chosen peer's latest
snapshot straight out of its HBM over the pair's xGMI link, validates it and
blends it in. No host copy, no socket and no host synchronisation inside a
step, and no kernel ever waits for another rank: a pull that finds no version
yet (empty) or a slot that was rewritten while it was read (torn) leaves the
variables as they are and is counted.

Ranks sharing one GPU (the tests) work like ranks on the GPUs of one node;
behaviour across two physical GPUs is unmeasured.
"""
import ctypes

import torch
import torch.distributed as dist

from . import _lib
from .ops import kungfu_dtype

FLOAT_DTYPES = (torch.float32, torch.float16, torch.bfloat16, torch.float64)
COUNTERS = ("valid", "torn", "empty", "published")


def random_peer(rng, world, rank):
    """The reference's get_random_peer (async_sgd.py:71-75): draw t uniformly
    from [0, world); if t == rank return (t + 1) % world, else t. Rank
    `rank + 1` is therefore twice as likely as each other peer, as in the
    reference. With one rank the only peer is the rank itself
    ((0 + 1) % 1 == 0): it averages with its own last published model."""
    t = rng.randrange(world)
    return (t + 1) % world if t == rank else t


def _check(rc, what):
    _lib.check(rc, what, source="pairavg")


class PeerModelStore:
    """This rank's published model and its view of every peer's.

    `buckets`: flat contiguous GPU tensors of one float dtype on one device
    (the variable spans; every rank passes the same lengths). Collective over
    `group`: construction exchanges the IPC handles, close() ends with a
    barrier. Without an initialised process group the world is this process.
    """

    def __init__(self, buckets, group=None, slots=2):
        if int(slots) < 2:
            raise ValueError("PeerModelStore needs at least 2 slots")
        self.buckets = list(buckets)
        if not self.buckets:
            raise ValueError("PeerModelStore needs at least one bucket")
        first = self.buckets[0]
        if first.dtype not in FLOAT_DTYPES:
            raise ValueError("PeerModelStore: f32, f16, bf16 and f64 only, not %s" % first.dtype)
        for b in self.buckets:
            if b.dtype != first.dtype or b.device != first.device:
                raise ValueError("PeerModelStore: one dtype and one device per store")
            if not b.is_cuda or b.dim() != 1 or not b.is_contiguous():
                raise ValueError("PeerModelStore buckets must be flat contiguous GPU tensors")
        self.group = group
        self.slots = int(slots)
        self.world = dist.get_world_size(group) if dist.is_initialized() else 1
        self.rank = dist.get_rank(group) if dist.is_initialized() else 0
        self.device = first.device
        self.lib = _lib.load()
        self._bases = {}
        n = len(self.buckets)
        lens = [b.numel() * b.element_size() for b in self.buckets]
        with torch.cuda.device(self.device):
            self._plan = self.lib.kf_pairavg_create(
                _lib.ptr_array([b.data_ptr() for b in self.buckets]),
                (ctypes.c_size_t * n)(*lens), n, int(kungfu_dtype(first)), self.slots,
                self.world, self.rank)
        if not self._plan:
            raise _lib.KungFuAMDError("kf_pairavg_create failed: %s"
                                      % self.lib.kf_pairavg_last_error().decode())
        self._out = torch.zeros(4, dtype=torch.int64, device=self.device)
        if self.world > 1:
            self._connect(lens)

    def _connect(self, lens):
        from .p2p import share_ipc
        slot, ctrl, nbytes = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_size_t()
        _check(self.lib.kf_pairavg_local(self._plan, ctypes.byref(slot), ctypes.byref(ctrl),
                                         ctypes.byref(nbytes)), "kf_pairavg_local")
        shapes = [None] * self.world
        dist.all_gather_object(shapes, (lens, self.slots, str(self.buckets[0].dtype)),
                               group=self.group)
        if any(s != shapes[0] for s in shapes):
            raise ValueError("PeerModelStore: ranks differ in spans, slots or dtype: %r" % (shapes,))
        rows = share_ipc(self.lib, self.group, self.world, self.rank, [slot.value, ctrl.value],
                         self._bases)
        _check(self.lib.kf_pairavg_set_peers(self._plan, _lib.ptr_array(rows[0]),
                                             _lib.ptr_array(rows[1]), self.world),
               "kf_pairavg_set_peers")

    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    def _target(self, target):
        target = int(target)
        if not 0 <= target < self.world:
            raise ValueError("target %d out of range for world %d" % (target, self.world))
        return target

    def publish(self):
        """Queue a snapshot of the buckets as the next version (no sync)."""
        _check(self.lib.kf_pairavg_publish(self._plan, self._stream()), "kf_pairavg_publish")

    def pull_average_(self, target):
        """Queue: fetch rank `target`'s latest version and, if it arrived
        whole, buckets = 0.5 * (buckets + fetched) in place (no sync)."""
        _check(self.lib.kf_pairavg_pull_average(self._plan, self._target(target), self._stream()),
               "kf_pairavg_pull_average")

    # the phases singly: for tests and tools
    def _publish_begin(self):
        _check(self.lib.kf_pairavg_publish_begin(self._plan, self._stream()), "publish_begin")

    def _publish_copy(self):
        _check(self.lib.kf_pairavg_publish_copy(self._plan, self._stream()), "publish_copy")

    def _publish_end(self):
        _check(self.lib.kf_pairavg_publish_end(self._plan, self._stream()), "publish_end")

    def _pick(self, target):
        _check(self.lib.kf_pairavg_pick(self._plan, self._target(target), self._stream()), "pick")

    def _fetch(self, target):
        _check(self.lib.kf_pairavg_fetch(self._plan, self._target(target), self._stream()), "fetch")

    def _check_(self, target):
        _check(self.lib.kf_pairavg_check(self._plan, self._target(target), self._stream()), "check")

    def _blend(self):
        _check(self.lib.kf_pairavg_blend(self._plan, self._stream()), "blend")

    def counters(self):
        """{valid, torn, empty, published} so far; waits for the queued work."""
        _check(self.lib.kf_pairavg_counters(self._plan, self._out.data_ptr(), self._stream()),
               "kf_pairavg_counters")
        return dict(zip(COUNTERS, self._out.cpu().tolist()))

    def close(self):
        """Collective. Nothing is freed or unmapped before every rank's queued
        work is done: a peer may still be reading this rank's slots."""
        if self._plan is None:
            return
        torch.cuda.synchronize(self.device)
        if self.world > 1:
            dist.barrier(group=self.group)
        for base in self._bases.values():
            self.lib.kf_ipc_close(base)
        self._bases = {}
        self.lib.kf_pairavg_destroy(self._plan)
        self._plan = None
