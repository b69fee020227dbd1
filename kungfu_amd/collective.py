"""Bucketed data-parallel all-reduce across the GPUs of a node.

What the reference does (per gradient tensor, on the host):
  AllReduce op -> Session.AllReduce -> 1 MiB chunks -> strategy graphs ->
  std_transform_2 per received chunk (session.go:231-326), then the optimizer
  divides by np in a separate TF op (sync_sgd.py:103-104) or blends
  (sma_sgd.py:60-65).

What this module does instead: gradients live in a few large
flat device buckets; each bucket is split evenly into one shard per rank and
  1. RCCL reduce-scatter (sum)  — each rank receives the sum of its shard
  2. HIP epilogue on the shard  — /np (S-SGD) via kf_bucket_div, bit-exact
                                  against "sum, then g / np"
  3. RCCL all-gather            — every rank gets the full reduced bucket
over xGMI, one process per GPU. Buckets are issued back to back so the
epilogue of bucket i overlaps the reduce-scatter of bucket i+1 (all RS on the
RCCL stream first, each AG queued behind its own epilogue).

For f16/bf16 (and float MIN/MAX) step 1 is instead an all-to-all of the
shards followed by the HIP k-input fold of the `world` received shards in rank
order (algo "a2a"): RCCL's reduce-scatter would add in its own order and, for
bf16, round to bf16 at every hop, while the build defines bf16 as fp32
accumulation with one rounding (the oracle's semantics and the P2P path's).
Same xGMI bytes as the reduce-scatter; the bits no longer depend on the
transport (kungfu_amd/csrc/kf_exchange.hip does the same natively).

The epilogue runs through ``kungfu_amd.ops`` (HIP kernels). It is injectable
only so the orchestration can be exercised over gloo on CPU in tests; the
product default is the HIP path and it raises on CPU tensors.
"""
import torch
import torch.distributed as dist

from . import ops
from .base import OP_NAMES, OP, EvenPartition

# Shards start on 256-byte boundaries so every shard pointer is 16-B aligned
# for the vector path and RCCL's preferred alignment.
ALIGN_BYTES = 256

_RED_OPS = {
    OP.SUM: dist.ReduceOp.SUM,
    OP.MIN: dist.ReduceOp.MIN,
    OP.MAX: dist.ReduceOp.MAX,
    OP.PROD: dist.ReduceOp.PRODUCT,
}


class HipEpilogue:
    """The shard epilogues as HIP kernels (default, product path)."""

    def div_(self, x, np_):
        return ops.bucket_div_(x, np_)

    def fold_(self, inputs, out, op, np_):
        """out = left fold of inputs (rank order); np_ > 0: SUM then / np_."""
        if np_:
            return ops.bucket_reduce_avg(inputs, np_, out=out)
        return ops.bucket_reduce(inputs, out=out, op=op)

    def sma_blend_(self, v, summed, np_, alpha):
        return ops.sma_blend_(v, summed, np_, alpha)

    def sgd_update_(self, params, grads, moms, hypers, np_):
        """The SGD update of the shards (ops.sgd_update_batch_), one launch."""
        return ops.sgd_update_batch_(params, grads, moms, hypers, np_)

    def adam_update_(self, params, grads, exp_avgs, exp_avg_sqs, hypers, np_):
        """The Adam / AdamW update of the shards (ops.adam_update_batch_), one launch."""
        return ops.adam_update_batch_(params, grads, exp_avgs, exp_avg_sqs, hypers, np_)

    def adam_master_update_(self, params16, grads16, masters, exp_avgs, exp_avg_sqs, hypers, np_):
        """The Adam / AdamW update of 16-bit shards through their fp32 master
        and state shards (ops.adam_master_update_batch_), one launch."""
        return ops.adam_master_update_batch_(params16, grads16, masters, exp_avgs, exp_avg_sqs,
                                             hypers, np_)

    # -- the gated step --
    def sq_norm_plan(self, tensors):
        """A plan whose run("sq", out=...) writes the tensors' fp64 sums of
        squares and their total (ops.SegNorm), built once over fixed shards."""
        return ops.SegNorm(tensors)

    def step_gate_update_(self, sq, world, nps, groups, states, gate, **rule):
        """The verdict of a gated step (ops.step_gate_update_), one launch."""
        return ops.step_gate_update_(sq, world, nps, groups, states, gate, **rule)

    def adam_update_gated_(self, params, grads, exp_avgs, exp_avg_sqs, hyper, gate, states, group,
                           np_):
        return ops.adam_update_batch_gated_(params, grads, exp_avgs, exp_avg_sqs, hyper, gate,
                                            states, group, np_)

    def adam_master_update_gated_(self, params16, grads16, masters, exp_avgs, exp_avg_sqs, hyper,
                                  gate, states, group, np_):
        return ops.adam_master_update_batch_gated_(params16, grads16, masters, exp_avgs,
                                                   exp_avg_sqs, hyper, gate, states, group, np_)

    # -- Adam with stochastic rounding --
    def adam_sr_update_(self, params, grads, exp_avgs, exp_avg_sqs, hypers, np_, bases, streams,
                        key):
        """The stochastic-rounding Adam / AdamW update of bf16 shards
        (ops.adam_sr_update_batch_), one launch."""
        return ops.adam_sr_update_batch_(params, grads, exp_avgs, exp_avg_sqs, hypers, bases,
                                         streams, key, np_)

    def adam_sr_update_gated_(self, params, grads, exp_avgs, exp_avg_sqs, hyper, gate, states,
                              group, np_, bases, streams, key):
        return ops.adam_sr_update_batch_gated_(params, grads, exp_avgs, exp_avg_sqs, hyper, gate,
                                               states, bases, streams, key, group, np_)

    # -- Adam with 8-bit block-wise state --
    def adam8_update_(self, params, grads, m_codes, v_codes, m_scales, v_scales, hypers, np_):
        """The Adam / AdamW update of f32 shards with 8-bit state
        (ops.adam8_update_batch_), one launch."""
        return ops.adam8_update_batch_(params, grads, m_codes, v_codes, m_scales, v_scales,
                                       hypers, np_)

    def adam8_master_update_(self, params16, grads16, masters, m_codes, v_codes, m_scales,
                             v_scales, hypers, np_):
        return ops.adam8_master_update_batch_(params16, grads16, masters, m_codes, v_codes,
                                              m_scales, v_scales, hypers, np_)

    def adam8_update_gated_(self, params, grads, m_codes, v_codes, m_scales, v_scales, hyper,
                            gate, states, group, np_):
        return ops.adam8_update_batch_gated_(params, grads, m_codes, v_codes, m_scales, v_scales,
                                             hyper, gate, states, group, np_)

    def adam8_master_update_gated_(self, params16, grads16, masters, m_codes, v_codes, m_scales,
                                   v_scales, hyper, gate, states, group, np_):
        return ops.adam8_master_update_batch_gated_(params16, grads16, masters, m_codes, v_codes,
                                                    m_scales, v_scales, hyper, gate, states,
                                                    group, np_)

    def adam8_quantize_(self, x, which, codes, scales):
        """x in table `which`'s format into (codes, scales) (ops.adam8_quantize)."""
        return ops.adam8_quantize(x, which, codes, scales)

    def adam8_dequantize(self, codes, scales, which):
        """A new f32 tensor of (codes, scales)'s values (ops.adam8_dequantize)."""
        return ops.adam8_dequantize(codes, scales, which)

    # -- LAMB --
    def lamb_moments_(self, params, grads, exp_avgs, exp_avg_sqs, updates, hypers, np_):
        """LAMB's moments pass over the shards (ops.lamb_moments_batch_)."""
        return ops.lamb_moments_batch_(params, grads, exp_avgs, exp_avg_sqs, updates, hypers, np_)

    def lamb_master_moments_(self, grads16, masters, exp_avgs, exp_avg_sqs, updates, hypers, np_):
        """The same through fp32 master and state shards
        (ops.lamb_master_moments_batch_)."""
        return ops.lamb_master_moments_batch_(grads16, masters, exp_avgs, exp_avg_sqs, updates,
                                              hypers, np_)

    def lamb_trust_update_(self, sq, world, group_of, groups, nlr, ratio, trust_clip=0.0):
        """The tensors' trust ratios (ops.lamb_trust_update_), one launch per 16 groups."""
        return ops.lamb_trust_update_(sq, world, group_of, groups, nlr, ratio, trust_clip)

    def lamb_apply_plan(self, params, updates, tensors, ntensor, params16=None):
        """A plan whose run(nlr) applies the updates to the pieces
        (ops.LambApplyPlan), built once over fixed views."""
        return ops.LambApplyPlan(params, updates, tensors, ntensor, params16)

    # -- LAMB under a gate; the apply plan's run takes gate= --
    def lamb_moments_gated_(self, params, grads, exp_avgs, exp_avg_sqs, updates, hyper, gate,
                            states, group, np_):
        return ops.lamb_moments_batch_gated_(params, grads, exp_avgs, exp_avg_sqs, updates, hyper,
                                             gate, states, group, np_)

    def lamb_master_moments_gated_(self, grads16, masters, exp_avgs, exp_avg_sqs, updates, hyper,
                                   gate, states, group, np_):
        return ops.lamb_master_moments_batch_gated_(grads16, masters, exp_avgs, exp_avg_sqs,
                                                    updates, hyper, gate, states, group, np_)

    def lamb_trust_update_gated_(self, sq, world, group_of, groups, nlr, ratio, gate,
                                 trust_clip=0.0):
        return ops.lamb_trust_update_gated_(sq, world, group_of, groups, nlr, ratio, gate,
                                            trust_clip)


def coalesce_runs(buckets):
    """Maximal runs of buckets that are consecutive in one storage, each as
    one flat view."""
    runs, cur = [], []

    def flush():
        if not cur:
            return
        if len(cur) == 1:
            runs.append(cur[0])
        else:
            first = cur[0]
            n = sum(t.numel() for t in cur)
            runs.append(torch.empty(0, dtype=first.dtype, device=first.device).set_(
                first.untyped_storage(), first.storage_offset(), (n,)))
        cur.clear()

    for b in buckets:
        if cur:
            last = cur[-1]
            adjacent = (b.dtype == last.dtype and b.device == last.device and
                        b.untyped_storage().data_ptr() == last.untyped_storage().data_ptr() and
                        b.storage_offset() == last.storage_offset() + last.numel())
            if not adjacent:
                flush()
        cur.append(b)
    flush()
    return runs


def workspace_like(buckets):
    """One workspace tensor per bucket (e.g. SMA's sum of each variable
    bucket). When the buckets are one contiguous run (GradBuckets' flat
    layout), the workspaces are views of ONE flat allocation in the same
    order, so a kernel over (bucket, workspace) pairs sees two contiguous
    ranges and launches once over them (kf_sma_blend_batch merges such
    buckets)."""
    buckets = list(buckets)
    if len(buckets) > 1 and len(coalesce_runs(buckets)) == 1:
        flat = torch.empty(sum(b.numel() for b in buckets), dtype=buckets[0].dtype,
                           device=buckets[0].device)
        out, off = [], 0
        for b in buckets:
            out.append(flat[off:off + b.numel()].view_as(b))
            off += b.numel()
        return out
    return [torch.empty_like(b) for b in buckets]


def resolve_algo(algo, dtype, op, world):
    """"rs" (RCCL reduce-scatter) or "a2a" (all-to-all + HIP rank-order fold)
    for one bucket dtype; "auto" keeps RCCL's reduce-scatter where its order
    cannot change what the result means (integers; f32/f64, the north_star's
    path; for MIN/MAX only NaN inputs could select differently) and folds on
    the GPU where the build defines the arithmetic: f16 (per-hop rounding) and
    bf16 (fp32 accumulation, one rounding) — kf_exchange.hip resolve_algo."""
    if algo in ("rs", "a2a"):
        return algo
    if algo != "auto":
        raise ValueError("algo must be 'auto', 'rs' or 'a2a'")
    own = dtype in (torch.float16, torch.bfloat16)
    return "a2a" if own and world <= 16 else "rs"


def padded_count(count, world, itemsize):
    """Smallest length >= count that splits into `world` aligned shards."""
    unit = world * max(1, ALIGN_BYTES // itemsize)
    return ((count + unit - 1) // unit) * unit


PHASES = ("reduce_scatter", "epilogue", "all_gather", "blend")


class _PhaseClock:
    """Per-phase timing of the calls in a window (Exchange.set_timing): timing
    events on the current stream at every point where it moves from one phase
    to the next, so the segments partition the stream's time from a call's
    first launch to its last wait. A segment counts for the phase that ends
    at its closing mark: waiting on a reduce-scatter (or all-to-all) is
    phase 1, the HIP shard work phase 2, waiting on the all-gathers phase 3."""

    def __init__(self):
        self.calls = []

    def begin(self):
        marks = []
        self.calls.append(marks)
        self.mark(marks, "start")
        return marks

    @staticmethod
    def mark(marks, label):
        ev = torch.cuda.Event(enable_timing=True)
        ev.record()
        marks.append((label, ev))

    def sums(self):
        out = dict.fromkeys(PHASES, 0.0)
        for marks in self.calls:
            marks[-1][1].synchronize()
            for (_, a), (label, b) in zip(marks, marks[1:]):
                out[label] += 1e3 * a.elapsed_time(b)
        out["calls"] = len(self.calls)
        out["untimed_calls"] = 0
        return out


class Exchange:
    """One process group, its shard workspaces and the epilogue."""

    def __init__(self, group=None, epilogue=None, algo="auto"):
        self.group = group
        self.world = dist.get_world_size(group) if dist.is_initialized() else 1
        self.rank = dist.get_rank(group) if dist.is_initialized() else 0
        self.epilogue = epilogue if epilogue is not None else HipEpilogue()
        self.algo = algo
        resolve_algo(algo, torch.float32, OP.SUM, self.world)  # validates
        self._ws = {}
        self._clock = None

    def set_timing(self, on):
        """Start (zeroed) or stop the per-phase timing window (the native
        exchange's kf_exchange_set_timing, for this path)."""
        self._clock = _PhaseClock() if on else None

    def phase_times(self):
        """The window's per-phase sums in us (PHASES) and the timed calls."""
        if self._clock is None:
            return dict(dict.fromkeys(PHASES, 0.0), calls=0, untimed_calls=0)
        return self._clock.sums()

    def _marks(self):
        return self._clock.begin() if self._clock is not None else None

    @staticmethod
    def _mark(marks, label):
        if marks is not None:
            _PhaseClock.mark(marks, label)

    def _workspace(self, key, n, like):
        t = self._ws.get(key)
        if t is None or t.numel() < n or t.dtype != like.dtype or t.device != like.device:
            t = torch.empty(n, dtype=like.dtype, device=like.device)
            self._ws[key] = t
        return t[:n]

    def _check(self, buf):
        if buf.dim() != 1 or not buf.is_contiguous():
            raise ValueError("bucket must be a flat contiguous tensor")
        if buf.numel() % self.world:
            raise ValueError("bucket length %d not divisible by world %d; use "
                             "padded_count()" % (buf.numel(), self.world))

    def all_reduce_(self, buckets, op="sum", average=False, coalesce=True):
        """In-place all-reduce of flat padded buckets. average=True applies the
        S-SGD epilogue (sum, then / np) on each shard.

        coalesce=True merges buckets that lie back to back in one storage
        (GradBuckets(n_buckets=k) lays them out that way) into one
        reduce-scatter -> epilogue -> all-gather run: the same values with
        one RCCL launch pair instead of one per bucket — the fusion the
        reference's S-SGD applies to ready gradients (nccl_fusion,
        sync_sgd.py:87-92). Buckets handed over one call at a time (e.g. as
        backward produces them) are reduced as they come."""
        self.start_(buckets, op=op, average=average, coalesce=coalesce).wait()
        return buckets

    def start_(self, buckets, op="sum", average=False, coalesce=True, key="ar"):
        """Queue the all-reduce of `buckets` and return a handle whose wait()
        completes it. With RCCL nothing here blocks the host: each shard
        epilogue is ordered behind its reduce-scatter on the device, and each
        all-gather behind its epilogue, so this can be called from a backward
        hook while later gradients are still being computed. Concurrent calls
        must use different `key`s (their shard workspaces)."""
        red = OP_NAMES[op] if isinstance(op, str) else OP(op)
        if average and red != OP.SUM:
            raise ValueError("average requires op='sum'")
        for b in buckets:
            self._check(b)
        if self.world == 1:
            # a single peer: the reduce is the identity; g / 1 == g exactly
            return _Handle([])
        if coalesce:
            runs = coalesce_runs(buckets)
            if len(runs) < len(buckets):
                return self.start_(runs, op=op, average=average, coalesce=False, key=key)
        marks = self._marks()
        shards = []
        works = []
        for i, b in enumerate(buckets):
            shard = self._workspace((key, "rs", i), b.numel() // self.world, b)
            works.append(self._scatter(b, shard, red, (key, "a2a", i)))
            shards.append(shard)
        gathers = []
        for b, shard, (w, recv) in zip(buckets, shards, works):
            w.wait()
            self._mark(marks, "reduce_scatter")
            if recv is not None:  # the rank-order fold of the received shards
                self.epilogue.fold_(list(recv.chunk(self.world)), shard, red,
                                    self.world if average else 0)
            elif average:
                self.epilogue.div_(shard, self.world)
            self._mark(marks, "epilogue")
            gathers.append(dist.all_gather_into_tensor(b, shard, group=self.group,
                                                       async_op=True))
        return _Handle(gathers, None if marks is None else
                       (lambda: _PhaseClock.mark(marks, "all_gather")))

    def _scatter(self, b, shard, red, key):
        """Step 1 for one bucket: (work, None) for RCCL's reduce-scatter into
        `shard`, or (work, recv) for the all-to-all whose `recv` holds the
        `world` shards (rank order) still to be folded."""
        if resolve_algo(self.algo, b.dtype, red, self.world) == "rs":
            return (dist.reduce_scatter_tensor(shard, b, op=_RED_OPS[red], group=self.group,
                                               async_op=True), None)
        recv = self._workspace(key, b.numel(), b)
        return dist.all_to_all_single(recv, b, group=self.group, async_op=True), recv

    def sma_(self, buckets, alpha):
        """SMA over flat variable buckets (sma_sgd.py:60-65): each rank's v
        becomes (1-alpha) v + alpha * (sum_ranks v) / np."""
        for b in buckets:
            self._check(b)
        sums = []
        if self.world == 1:
            for i, b in enumerate(buckets):
                s = self._workspace(("sum", i), b.numel(), b)
                s.copy_(b)
                sums.append(s)
            for b, s in zip(buckets, sums):
                self.epilogue.sma_blend_(b, s, self.world, alpha)
            return buckets
        # pipelined: every reduce-scatter is queued first, each all-gather
        # right behind its reduce-scatter, and each bucket's blend waits only
        # for its own all-gather, so blends overlap later buckets' transfers.
        # The reduce-scatter reads v before any blend of that bucket runs.
        marks = self._marks()
        rs = []
        for i, b in enumerate(buckets):
            shard = self._workspace(("rs", i), b.numel() // self.world, b)
            rs.append((shard, self._scatter(b, shard, OP.SUM, ("a2a", i))))
        ags = []
        for i, (b, (shard, (w, recv))) in enumerate(zip(buckets, rs)):
            w.wait()
            self._mark(marks, "reduce_scatter")
            if recv is not None:
                self.epilogue.fold_(list(recv.chunk(self.world)), shard, OP.SUM, 0)
                self._mark(marks, "epilogue")
            s = self._workspace(("sum", i), b.numel(), b)
            ags.append((s, dist.all_gather_into_tensor(s, shard, group=self.group,
                                                       async_op=True)))
        for b, (s, w) in zip(buckets, ags):
            w.wait()
            self._mark(marks, "all_gather")
            self.epilogue.sma_blend_(b, s, self.world, alpha)
            self._mark(marks, "blend")
        return buckets


    def sgd_step_(self, param_buckets, grad_buckets, mom_shards, hypers):
        """The synchronous step with the SGD update on this rank's shards (the
        native exchange's kf_exchange_sgd_batch, for this path): every
        gradient bucket is reduce-scattered (or all-to-all'ed and folded in
        rank order with the / world), epilogue.sgd_update_ runs once over the
        shards — parameters, summed gradients, momentum shards — and every
        parameter bucket is all-gathered in place. After a reduce-scatter
        the update divides by the world itself. mom_shards[b] holds
        numel // world elements (None where hypers[b]'s momentum is 0). The
        gradient buckets are only read here; callers must not rely on that
        (the native exchange uses them as scratch)."""
        params = list(param_buckets)
        moms = [None] * len(params) if mom_shards is None else mom_shards
        return self._shard_schedule("sgd_step_", "sgd", params, grad_buckets, (moms,),
                                    hypers, self.epilogue.sgd_update_)

    def adam_step_(self, param_buckets, grad_buckets, exp_avg_shards, exp_avg_sq_shards, hypers):
        """sgd_step_ with the Adam / AdamW update on this rank's shards (the
        native exchange's kf_exchange_adam_batch, for this path): every
        gradient bucket is reduce-scattered (or all-to-all'ed and folded in
        rank order with the / world), epilogue.adam_update_ runs once over the
        shards — parameters, summed gradients, both state shards — and every
        parameter bucket is all-gathered in place. Both state shards of
        bucket b hold numel // world elements. hypers[b] as
        ops.adam_update_batch_ takes them. The gradient buckets are only read
        here; callers must not rely on that."""
        return self._shard_schedule("adam_step_", "adam", param_buckets, grad_buckets,
                                    (exp_avg_shards, exp_avg_sq_shards), hypers,
                                    self.epilogue.adam_update_)

    def adam_master_step_(self, param_buckets, grad_buckets, master_shards, exp_avg_shards,
                          exp_avg_sq_shards, hypers):
        """adam_step_ for bf16 / f16 buckets with fp32 master weights and state
        (the native exchange's kf_exchange_adam_master_batch, for this path):
        the same schedule on the 16-bit buckets; epilogue.adam_master_update_
        runs once over the shards (16-bit parameters, summed 16-bit gradients,
        and this rank's fp32 master, exp_avg and exp_avg_sq shards of
        numel // world elements each)."""
        return self._shard_schedule("adam_master_step_", "adam", param_buckets, grad_buckets,
                                    (master_shards, exp_avg_shards, exp_avg_sq_shards), hypers,
                                    self.epilogue.adam_master_update_)

    def _shard_schedule(self, name, key, param_buckets, grad_buckets, state_shards, hypers,
                        update):
        """What sgd_step_, adam_step_ and adam_master_step_ share:
        update(params, grads, *states, hypers, np_) on this rank's shards
        between the gradients' reduce-scatter and the parameters' all-gather.
        A state shard may be None (SGD without momentum); `key` names the
        workspaces."""
        params, grads, hypers = list(param_buckets), list(grad_buckets), list(hypers)
        states = [list(s) for s in state_shards]
        if not all(len(x) == len(params) for x in [grads, hypers] + states):
            raise ValueError("%s: one grad bucket, %d state shards and a hyper per bucket"
                             % (name, len(states)))
        for i, (p, g) in enumerate(zip(params, grads)):
            self._check(p)
            self._check(g)
            if g.numel() != p.numel() or g.dtype != p.dtype or \
                    any(s[i] is not None and s[i].numel() * self.world != p.numel()
                        for s in states):
                raise ValueError("%s: bucket / shard sizes do not match" % name)
        if not params:
            return params
        if self.world == 1:
            update(params, grads, *states, hypers, 1)
            return params
        marks = self._marks()
        shards, nps = self._reduce_shards(key, grads, marks)
        # one update launch over all shards: the / world is the fold's where
        # the shards were folded here, the update's own after a reduce-scatter
        width = 3 + len(states)
        sets = {0: tuple([] for _ in range(width)), self.world: tuple([] for _ in range(width))}
        for i, (p, h, shard, np_) in enumerate(zip(params, hypers, shards, nps)):
            q = shard.numel()
            row = (p[self.rank * q:(self.rank + 1) * q], shard) + tuple(s[i] for s in states) + (h,)
            for lst, x in zip(sets[np_], row):
                lst.append(x)
        for np_, lists in sets.items():
            if lists[0]:
                update(*lists, np_)
        self._mark(marks, "epilogue")
        self._gather_params(params, marks)
        return params

    def _reduce_shards(self, key, grads, marks):
        """Phase 1 and the rank-order folds of a sharded step: (this rank's
        reduced shards, what the update must still divide each by: the world
        after a reduce-scatter, 0 after the fold). The shards are the cached
        workspaces (key, "rs", i): the same addresses at every step."""
        works = []
        for i, g in enumerate(grads):
            shard = self._workspace((key, "rs", i), g.numel() // self.world, g)
            works.append((shard, self._scatter(g, shard, OP.SUM, (key, "a2a", i))))
        for _, (w, _) in works:
            w.wait()
        self._mark(marks, "reduce_scatter")
        shards, nps = [], []
        for shard, (w, recv) in works:
            if recv is not None:
                self.epilogue.fold_(list(recv.chunk(self.world)), shard, OP.SUM, self.world)
            shards.append(shard)
            nps.append(0 if recv is not None else self.world)
        return shards, nps

    def _gather_params(self, params, marks):
        """Phase 3 of a sharded step: every parameter bucket's in-place all-gather."""
        gathers = []
        for p in params:
            q = p.numel() // self.world
            gathers.append(dist.all_gather_into_tensor(p, p[self.rank * q:(self.rank + 1) * q],
                                                       group=self.group, async_op=True))
        for w in gathers:
            w.wait()
        self._mark(marks, "all_gather")

    # -- the gated step: adam_step_ / adam_master_step_ in two
    # halves, with the optimizer's verdict over all its bucket groups between
    def grad_shards_(self, grad_buckets, key):
        """Where reduce_shards_(grad_buckets, key) leaves this rank's reduced
        shards: fixed addresses, so a norm plan over them is built once."""
        grads = list(grad_buckets)
        for g in grads:
            self._check(g)
        if self.world == 1:
            return grads
        return [self._workspace((key, "rs", i), g.numel() // self.world, g)
                for i, g in enumerate(grads)]

    def reduce_shards_(self, grad_buckets, key):
        """Half one (the native exchange's kf_exchange_reduce_shards_batch):
        the gradients' reduce-scatter, or all-to-all and rank-order fold with
        the / world. Returns what the update must still divide by: the world
        after a reduce-scatter, 0 after the fold, 1 at world 1."""
        grads = list(grad_buckets)
        for g in grads:
            self._check(g)
        if self.world == 1:
            return 1
        if not grads:
            return 0
        _, nps = self._reduce_shards(key, grads, self._marks())
        if len(set(nps)) != 1:
            raise ValueError("reduce_shards_: one dtype per call")
        return nps[0]

    def gather_doubles_(self, send, recv):
        """recv[r * n + k] = rank r's send[k] (kf_exchange_all_gather_doubles):
        the plans' sums of squares of a gated step."""
        if recv.numel() != send.numel() * self.world or send.dtype != torch.float64 or \
                recv.dtype != torch.float64:
            raise ValueError("gather_doubles_: recv holds world * send.numel() float64 values")
        if self.world == 1:
            if recv.data_ptr() != send.data_ptr():
                recv.copy_(send)
            return recv
        dist.all_gather_into_tensor(recv, send.clone(), group=self.group)
        return recv

    def gather_params_(self, param_buckets):
        """Phase 3 alone (the native exchange's kf_exchange_gather_params_batch):
        every parameter bucket's in-place all-gather of the ranks' shards, for
        a step whose update ran outside the exchange (LAMB). Nothing at world 1."""
        params = list(param_buckets)
        for p in params:
            self._check(p)
            if p.numel() % self.world:
                raise ValueError("gather_params_: bucket sizes must be multiples of the world")
        if self.world == 1 or not params:
            return params
        self._gather_params(params, self._marks())
        return params

    def adam_gated_step_(self, param_buckets, grad_buckets, master_shards, exp_avg_shards,
                         exp_avg_sq_shards, hyper, np_, gate, states, group, key):
        """Half two (the native exchange's kf_exchange_adam_gated_batch):
        epilogue.adam_update_gated_, or with master_shards
        epilogue.adam_master_update_gated_, on the shards reduce_shards_ left
        under the same `key`, with the one `hyper`, `np_` as reduce_shards_
        returned it, the gate and step state `group` of `states`; then every
        parameter bucket is all-gathered in place."""
        params, grads = list(param_buckets), list(grad_buckets)
        with_master = master_shards is not None
        states_ = [list(s) for s in ((master_shards,) if with_master else ()) +
                   (exp_avg_shards, exp_avg_sq_shards)]
        if not all(len(x) == len(params) for x in [grads] + states_):
            raise ValueError("adam_gated_step_: one grad bucket and %d state shards per bucket"
                             % len(states_))
        for i, (p, g) in enumerate(zip(params, grads)):
            self._check(p)
            if g.numel() != p.numel() or g.dtype != p.dtype or \
                    any(s[i].numel() * self.world != p.numel() for s in states_):
                raise ValueError("adam_gated_step_: bucket / shard sizes do not match")
        if not params:
            return params
        shards = self.grad_shards_(grads, key)
        q = [p.numel() // self.world for p in params]
        mine = [p[self.rank * n:(self.rank + 1) * n] for p, n in zip(params, q)]
        update = self.epilogue.adam_master_update_gated_ if with_master else \
            self.epilogue.adam_update_gated_
        marks = self._marks() if self.world > 1 else None
        update(mine, shards, *states_, hyper, gate, states, group, np_)
        if self.world > 1:
            self._mark(marks, "epilogue")
            self._gather_params(params, marks)
        return params


class _Handle:
    """Pending collectives of one start_() call."""

    def __init__(self, works, on_done=None):
        self.works = works
        self.on_done = on_done

    def wait(self):
        for w in self.works:
            w.wait()
        self.works = []
        if self.on_done is not None:
            self.on_done()
            self.on_done = None


class GradBuckets:
    """Flat, padded device storage for a list of same-dtype tensors.

    Two layouts:
      * ``bucket_bytes`` (default): tensors are grouped, in order, into buckets
        of about that size at tensor boundaries (a larger tensor gets a bucket
        of its own); each bucket is its own flat buffer, padded to split into
        ``world`` aligned shards.
      * ``n_buckets=k``: all tensors are laid out back to back in ONE flat
        buffer, which is cut into k contiguous buckets by EvenPartition
        (interval.go:12-27) of its aligned units — tensors may straddle bucket
        boundaries (the reduce is element-wise). This is SURVEY §8(a) C4:
        ResNet-50's 25,583,592 fp32 in 16 buckets of ~1.6 M elements.
    ``views[i]`` is tensor i's view into the flat storage, so gradients can be
    written in place and reduced without fuse/defuse copies (the reference's
    NCCL path concatenates and slices instead, ops/__init__.py:29-46).
    ``spans[j]`` is the number of real (non-padding) elements of bucket j,
    which always precede its padding.
    """

    def __init__(self, numels, dtype, device, world, bucket_bytes=32 << 20,
                 n_buckets=None):
        itemsize = torch.empty((), dtype=dtype).element_size()
        self.buckets, self.views, self.spans, self.flats = [], [None] * len(numels), [], []
        if n_buckets is not None:
            total = sum(numels)
            unit = world * max(1, ALIGN_BYTES // itemsize)
            units = max(1, (total + unit - 1) // unit)
            flat = torch.zeros(units * unit, dtype=dtype, device=device)
            self.flats.append(flat)
            off = 0
            for i, n in enumerate(numels):
                self.views[i] = flat[off:off + n]
                off += n
            for ub, ue in EvenPartition(0, units, min(n_buckets, units)):
                b, e = ub * unit, ue * unit
                self.buckets.append(flat[b:e])
                self.spans.append(max(0, min(e, total) - b))
            return
        for g in self._groups_greedy(numels, max(1, bucket_bytes // itemsize)):
            count = sum(numels[i] for i in g)
            b = torch.zeros(padded_count(max(count, 1), world, itemsize),
                            dtype=dtype, device=device)
            off = 0
            for i in g:
                self.views[i] = b[off:off + numels[i]]
                off += numels[i]
            self.flats.append(b)
            self.buckets.append(b)
            self.spans.append(count)

    @staticmethod
    def _groups_greedy(numels, cap):
        groups, cur, size = [], [], 0
        for i, n in enumerate(numels):
            if cur and size + n > cap:
                groups.append(cur)
                cur, size = [], 0
            cur.append(i)
            size += n
        if cur:
            groups.append(cur)
        return groups


def group_all_reduce(tensors, op="sum", average=False, exchange=None,
                     bucket_bytes=32 << 20):
    """Mirror of the reference's group_all_reduce (ops/collective.py:71-73):
    returns all-reduced copies of `tensors`. Fuses them into flat buckets
    (copy in, reduce, copy out); optimizers that own their gradient storage
    use GradBuckets directly and skip the copies."""
    ex = exchange or Exchange()
    if not tensors:
        return []
    by_dtype = {}
    for i, t in enumerate(tensors):
        by_dtype.setdefault((t.dtype, t.device), []).append(i)
    out = [None] * len(tensors)
    for (dtype, device), idx in by_dtype.items():
        gb = GradBuckets([tensors[i].numel() for i in idx], dtype, device,
                         ex.world, bucket_bytes=bucket_bytes)
        for j, i in enumerate(idx):
            gb.views[j].copy_(tensors[i].reshape(-1))
        ex.all_reduce_(gb.buckets, op=op, average=average)
        for j, i in enumerate(idx):
            out[i] = gb.views[j].view_as(tensors[i]).clone()
    return out


def all_reduce(t, op="sum", exchange=None):
    """Mirror of all_reduce(t, op) (ops/collective.py:22-24)."""
    return group_all_reduce([t], op=op, exchange=exchange)[0]
