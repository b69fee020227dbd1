"""Synchronous data-parallel optimizers whose gradient/variable reduction runs on
the MI355X bucket path (RCCL reduce-scatter + HIP epilogue + RCCL all-gather).

Operator surface kept from the reference:

* ``SynchronousSGDOptimizer(optimizer, named_parameters=None, op=None, ...)``
  — torch signature of srcs/python/kungfu/torch/optimizers/sync_sgd.py:31-34
  (wraps an optimizer instance, reduces every gradient in ``step()``). The
  arithmetic is that of the TF S-SGD (sync_sgd.py:78-109): all-reduce-sum of
  each gradient, then ``g / np`` — here fused into the shard epilogue and
  bit-exact against "sum, then divide". ``average=False`` gives the torch
  reference's sum-only behaviour (torch/optimizers/sync_sgd.py:12-22).
* ``SynchronousAveragingOptimizer(optimizer, named_parameters=None, alpha=0.1)``
  — SMA (sma_sgd.py:9-74): before the local update every variable with a
  gradient becomes ``(1 - alpha) * v + alpha * allreduce_sum(v) / np``.
* ``MonitorGradientNoiseScaleOptimizer`` and ``MonitorGradientVarianceOptimizer``
  (grad_noise_scale.py, grad_variance.py): S-SGD (sum, / np) that on every
  ``monitor_interval``-th step also reduces the gradient buckets to scalars
  on the device (ops.SegNorm: one read-only pass, fp64) — the gradient noise
  scale's running estimate, or the per-parameter gradient variance.
* ``PairAveragingOptimizer(optimizer, named_parameters=None, ...)`` — AD-PSGD
  (async_sgd.py): asynchronous; every step averages the variables with one
  peer's latest published model, read out of that peer's HBM through a
  device-side model store (``pairavg.PeerModelStore``), with no collective.
* ``ShardedSGDOptimizer(optimizer, named_parameters=None, ...)`` — S-SGD with
  the SGD update itself moved onto each rank's shard, between the gradients'
  reduce-scatter and an all-gather of the parameters; the momentum state is
  sharded over the ranks. The package's own (the reference has none).
* ``ShardedAdamOptimizer(optimizer, named_parameters=None, ...)`` — the same
  for torch.optim.Adam / AdamW: exp_avg and exp_avg_sq sharded over the ranks.
* ``ShardedLAMBOptimizer(optimizer, named_parameters=None, ...)`` — LAMB on
  the same shards: per-tensor trust ratios from norms taken across the ranks.

Buckets: parameters are grouped (in registration order, per dtype/device) into
flat padded device buckets (``collective.GradBuckets``); ``p.grad`` (S-SGD) or
``p.data`` (SMA) are made views into them so the reduction needs no fuse /
defuse copies. If a training loop replaces ``p.grad`` (``zero_grad`` with
``set_to_none=True``), the new gradient is copied into the bucket view once.
"""

from .collective import Exchange, GradBuckets


def _wrap(optimizer, mixin):
    # same trick as the reference (torch/optimizers/sync_sgd.py:31-34): a
    # subclass of the user's optimizer class, sharing its param_groups/state
    cls = type(optimizer.__class__.__name__, (mixin, optimizer.__class__), {})
    obj = cls.__new__(cls)
    obj.__dict__.update(optimizer.__dict__)
    return obj


def _finish(exchange):
    """An exchange whose queued work can fail without the host seeing it
    (the P2P device barriers) settles and raises here, before the update
    consumes the reduced values."""
    fin = getattr(exchange, "finish", None)
    if fin is not None:
        fin()


class _Bucketed:
    def _kf_setup(self, named_parameters, exchange, bucket_bytes):
        if named_parameters is None:
            params = [p for g in self.param_groups for p in g["params"]]
        else:
            params = [p for _, p in named_parameters]
        self._kf_params = [p for p in params if p.requires_grad]
        self._kf_ex = exchange if exchange is not None else Exchange()
        self._kf_bucket_bytes = bucket_bytes
        self._kf_groups = None

    def _kf_build(self, tensors_of):
        groups = {}
        for p in self._kf_params:
            groups.setdefault((p.dtype, p.device), []).append(p)
        self._kf_groups = []
        for (dtype, device), ps in groups.items():
            gb = GradBuckets([p.numel() for p in ps], dtype, device,
                             self._kf_ex.world, bucket_bytes=self._kf_bucket_bytes)
            self._kf_groups.append((ps, gb))


class _SyncSGD(_Bucketed):
    def _kf_setup_overlap(self):
        """Buckets in backward order (parameters reversed) with one
        post-accumulate-grad hook per parameter: when the last gradient of a
        bucket is in, that bucket's RS -> /np -> AG is queued at once, while
        backward goes on computing earlier layers. Buckets are launched strictly
        in index order (a ready bucket waits for the ones before it), so every
        rank issues the same collectives in the same order."""
        groups = {}
        for p in reversed(self._kf_params):
            groups.setdefault((p.dtype, p.device), []).append(p)
        self._kf_slots = []  # (bucket, [(param, view)]) in launch order
        self._kf_slot_of = {}
        for (dtype, device), ps in groups.items():
            gb = GradBuckets([p.numel() for p in ps], dtype, device,
                             self._kf_ex.world, bucket_bytes=self._kf_bucket_bytes)
            members = [[] for _ in gb.buckets]
            for p, v in zip(ps, gb.views):
                j = next(j for j, b in enumerate(gb.buckets)
                         if b.data_ptr() <= v.data_ptr() < b.data_ptr() + b.numel() * b.element_size())
                members[j].append((p, v.view_as(p)))
            for b, m in zip(gb.buckets, members):
                for p, v in m:
                    self._kf_slot_of[p] = (len(self._kf_slots), v)
                self._kf_slots.append((b, m))
        self._kf_reset_overlap()
        for p in self._kf_params:
            p.register_post_accumulate_grad_hook(self._kf_grad_ready)

    def _kf_reset_overlap(self):
        self._kf_missing = [len(m) for _, m in self._kf_slots]
        self._kf_next = 0
        self._kf_handles = []

    def _kf_grad_ready(self, p):
        i, v = self._kf_slot_of[p]
        if p.grad.data_ptr() != v.data_ptr():
            v.copy_(p.grad)
        self._kf_missing[i] -= 1
        self._kf_launch_ready()

    def _kf_launch_ready(self):
        # every bucket that is ready in index order goes out in ONE start_
        # call: the native exchange runs a call's buckets as one grouped RCCL
        # launch per phase and one batched HIP epilogue (kf_bucket_reduce_batch)
        first = self._kf_next
        while self._kf_next < len(self._kf_slots) and self._kf_missing[self._kf_next] <= 0:
            self._kf_next += 1
        if self._kf_next > first:
            self._kf_handles.append(self._kf_ex.start_(
                [b for b, _ in self._kf_slots[first:self._kf_next]], op=self._kf_op,
                average=self._kf_average, coalesce=False, key="ovl%d" % first))

    def _kf_finish_overlap(self):
        # parameters that got no gradient this step contribute zeros
        # (sync_gradients' rule); then every remaining bucket goes, in order
        for i, (b, m) in enumerate(self._kf_slots):
            if i >= self._kf_next and self._kf_missing[i] > 0:
                for p, v in m:
                    if p.grad is None:
                        v.zero_()
                self._kf_missing[i] = 0
        self._kf_launch_ready()
        for h in self._kf_handles:
            h.wait()
        for b, m in self._kf_slots:
            for p, v in m:
                p.grad = v
        self._kf_reset_overlap()

    @staticmethod
    def _kf_place(ps, gb):
        """Every gradient of one group into its bucket view (zeros for a
        parameter without one)."""
        for p, view in zip(ps, gb.views):
            g = p.grad
            v = view.view_as(p)
            if g is None:
                v.zero_()
                p.grad = v
            elif g.data_ptr() != v.data_ptr():
                v.copy_(g)
                p.grad = v

    def sync_gradients(self):
        if self._kf_overlap:
            return self._kf_finish_overlap()
        if self._kf_groups is None:
            self._kf_build(None)
        for ps, gb in self._kf_groups:
            self._kf_place(ps, gb)
            self._kf_ex.all_reduce_(gb.buckets, op=self._kf_op,
                                    average=self._kf_average)

    def step(self, closure=None):
        self.sync_gradients()
        _finish(self._kf_ex)
        return super().step(closure)


def SynchronousSGDOptimizer(optimizer, named_parameters=None, op=None,
                            average=True, exchange=None, bucket_bytes=32 << 20,
                            overlap=False):
    """S-SGD: all-reduce gradients (sum, then / np when average) before each
    step. Returns the wrapped optimizer (reference: sync_sgd.py:81-84).

    overlap=True starts each bucket's exchange from a backward hook as soon as
    its gradients are complete (one backward per step), so the RCCL traffic
    of late layers hides behind the backward of early ones; step() waits for
    the rest. Same values as overlap=False up to the bucket grouping."""
    opt = _wrap(optimizer, _SyncSGD)
    opt._kf_setup(named_parameters, exchange, bucket_bytes)
    opt._kf_op = op if op is not None else "sum"
    opt._kf_average = bool(average)
    if opt._kf_average and opt._kf_op != "sum":
        raise ValueError("average=True needs op='sum'")
    opt._kf_overlap = bool(overlap)
    if opt._kf_overlap:
        if not hasattr(opt._kf_ex, "start_"):
            raise ValueError("overlap=True needs an exchange with start_() "
                             "(collective.Exchange)")
        opt._kf_setup_overlap()
    return opt


class _Monitored(_SyncSGD):
    """S-SGD (sum, / np) with a monitor on every `monitor_interval`-th step
    (step counter from 0). The monitor reads each gradient bucket where it is
    with one segmented-norm pass (ops.SegNorm) and leaves its results on the
    device; a step that is not monitored is exactly plain S-SGD, and a
    monitored one changes no gradient either.

    overlap=True is not offered: the local norm has to be read after the last
    gradient is in its bucket and before that bucket is exchanged in place,
    which is the window the overlapped schedule removes."""

    def _kf_setup_monitor(self, named_parameters, exchange, bucket_bytes, monitor_interval,
                          overlap):
        if overlap:
            raise ValueError("the monitoring optimizers have no overlap=True: the local "
                             "norm is read before a bucket is exchanged in place")
        if int(monitor_interval) < 1:
            raise ValueError("monitor_interval must be at least 1")
        self._kf_setup(named_parameters, exchange, bucket_bytes)
        self._kf_op = "sum"
        self._kf_average = True
        self._kf_overlap = False
        self._kf_interval = int(monitor_interval)
        self._kf_step = 0
        self._kf_plans = None

    def _kf_result_device(self):
        return self._kf_params[0].device

    def sync_gradients(self):
        if self._kf_groups is None:
            self._kf_build(None)
        monitored = self._kf_step % self._kf_interval == 0
        self._kf_step += 1
        for ps, gb in self._kf_groups:
            self._kf_place(ps, gb)
        if monitored:
            self._kf_before_exchange()
        for ps, gb in self._kf_groups:
            self._kf_ex.all_reduce_(gb.buckets, op="sum", average=True)
        if monitored:
            self._kf_after_exchange()

    def _kf_total(self, outs, into):
        """The groups' totals (each run's last value) added into `into`."""
        dev = into.device
        tot = outs[0][-1].to(dev)
        for o in outs[1:]:  # several dtype groups: one tiny add each
            tot = tot + o[-1].to(dev)
        into.copy_(tot)


class _NoiseScale(_Monitored):
    def _kf_before_exchange(self):
        from . import ops
        import torch
        if self._kf_plans is None:
            # one segment per bucket: its real span, not the padding
            self._kf_plans = [ops.SegNorm([b[:sp] for b, sp in zip(gb.buckets, gb.spans)])
                              for _, gb in self._kf_groups]
            self._kf_outs = [(torch.zeros(pl.nseg + 1, dtype=torch.float64, device=pl.device),
                              torch.zeros(pl.nseg + 1, dtype=torch.float64, device=pl.device))
                             for pl in self._kf_plans]
        for pl, (small, _) in zip(self._kf_plans, self._kf_outs):
            pl.run("sq", out=small)
        self._kf_total([o[0] for o in self._kf_outs], self._kf_sq[0])

    def _kf_after_exchange(self):
        from . import ops
        for pl, (_, big) in zip(self._kf_plans, self._kf_outs):
            pl.run("sq", out=big)
        self._kf_total([o[1] for o in self._kf_outs], self._kf_sq[1])
        bs = self._kf_device_batch
        ops.noise_scale_update_(self._kf_sq[0], self._kf_sq[1], bs, bs * self._kf_ex.world,
                                self._kf_alpha, self._kf_ns_state)

    @property
    def noise_scale(self):
        """0-dim fp32 device tensor: the running s_ema / g_ema (`.item()` it
        when wanted; nothing here synchronises the host)."""
        return self._kf_ns_state[2]

    @property
    def noise_scale_state(self):
        """{g_ema, s_ema, noise_scale, has_value} as 4 fp32 device values."""
        return self._kf_ns_state

    @property
    def last_sq_small(self):
        """|local gradient|^2 of the last monitored step (0-dim fp64, device)."""
        return self._kf_sq[0]

    @property
    def last_sq_big(self):
        """|averaged gradient|^2 of the last monitored step."""
        return self._kf_sq[1]


def MonitorGradientNoiseScaleOptimizer(optimizer, device_batch_size, monitor_interval=1,
                                       named_parameters=None, alpha=0.9, exchange=None,
                                       bucket_bytes=32 << 20, overlap=False):
    """S-SGD that also estimates the gradient noise scale (grad_noise_scale.py):
    on a monitored step |g|^2 of the local gradients (before the exchange) and
    of the averaged ones (after it) are taken over the buckets' real spans,
    and kf_noise_scale_update runs monitor.py:10-17 and the NoiseScale op's
    two EMAs on the device with batch_small = device_batch_size and
    batch_big = device_batch_size * world. With one peer the formula divides
    by zero and gives inf or NaN, as the reference.

    Results stay on the device: `noise_scale` (0-dim fp32), `last_sq_small`
    and `last_sq_big` (0-dim fp64)."""
    if not device_batch_size > 0:
        raise ValueError("device_batch_size must be greater than zero")
    if not alpha > 0:
        raise ValueError("alpha must be greater than zero")
    import torch
    opt = _wrap(optimizer, _NoiseScale)
    opt._kf_setup_monitor(named_parameters, exchange, bucket_bytes, monitor_interval, overlap)
    opt._kf_device_batch = float(device_batch_size)
    opt._kf_alpha = float(alpha)
    dev = opt._kf_result_device()
    opt._kf_ns_state = torch.zeros(4, dtype=torch.float32, device=dev)
    opt._kf_sq = torch.zeros(2, dtype=torch.float64, device=dev)
    return opt


class _GradVariance(_Monitored):
    def _kf_build_variance(self):
        from . import ops
        from .collective import workspace_like
        import torch
        self._kf_work, self._kf_plans, self._kf_outs, self._kf_index = [], [], [], []
        pos = {id(p): i for i, p in enumerate(self._kf_params)}
        for ps, gb in self._kf_groups:
            if gb.buckets[0].dtype == torch.float16:
                raise TypeError("MonitorGradientVarianceOptimizer: fp16 gradients have no "
                                "element-wise product on the device (the reduce defines "
                                "fp16 SUM only)")
            ws = workspace_like(gb.buckets)
            pairs = []
            for v in gb.views:  # the workspace view under each gradient view
                j = next(j for j, b in enumerate(gb.buckets)
                         if b.data_ptr() <= v.data_ptr() < b.data_ptr() + max(1, b.numel()) * b.element_size())
                off = (v.data_ptr() - gb.buckets[j].data_ptr()) // v.element_size()
                pairs.append((ws[j][off:off + v.numel()], v))
            pl = ops.SegNorm(pairs)
            self._kf_work.append(ws)
            self._kf_plans.append(pl)
            self._kf_outs.append(torch.zeros(pl.nseg + 1, dtype=torch.float64, device=pl.device))
            self._kf_index.append(torch.tensor([pos[id(p)] for p in ps], dtype=torch.int64,
                                               device=self._kf_var.device))

    def _kf_before_exchange(self):
        from . import ops
        if self._kf_plans is None:
            self._kf_build_variance()
        for (_, gb), ws in zip(self._kf_groups, self._kf_work):
            for b, w in zip(gb.buckets, ws):  # w = g * g, the reduce's own PROD
                ops.bucket_reduce([b, b], out=w, op="prod")

    def _kf_after_exchange(self):
        for ws in self._kf_work:  # mean over the peers of g * g
            self._kf_ex.all_reduce_(ws, op="sum", average=True)
        dev = self._kf_var.device
        for pl, out, idx in zip(self._kf_plans, self._kf_outs, self._kf_index):
            pl.run("var", out=out, total_sqrt=True)
            self._kf_var.index_copy_(0, idx, out[:-1].to(dev))
        self._kf_total(self._kf_outs, self._kf_var_total)

    @property
    def variance(self):
        """0-dim fp64 device tensor: sum over the parameters of
        ||mean(g^2) - mean(g)^2|| (grad_variance.py:55-58)."""
        return self._kf_var_total

    @property
    def last_variances(self):
        """Per parameter (registration order) sum d^2, d = mean(g^2) -
        mean(g)^2 element-wise in the gradient's dtype; fp64, device."""
        return self._kf_var


def MonitorGradientVarianceOptimizer(optimizer, monitor_interval=1, named_parameters=None,
                                     exchange=None, bucket_bytes=32 << 20, overlap=False):
    """S-SGD that also monitors the gradient variance (grad_variance.py): on a
    monitored step each bucket's g * g goes into a workspace (the reduce
    kernel's PROD) before the exchange, gradients and workspaces are both
    averaged over the peers, and one segmented pass takes, per parameter,
    sum d^2 with d = mean(g^2) - mean(g)^2 rounded as the tensors' dtype
    (KF_NORM_VAR), and the sum of their square roots.

    Results stay on the device: `variance` (0-dim fp64) and `last_variances`
    (fp64, one per parameter). fp64 accumulation in a fixed order; the
    reference's tf.norm sums in fp32 in an order TF does not define."""
    import torch
    opt = _wrap(optimizer, _GradVariance)
    opt._kf_setup_monitor(named_parameters, exchange, bucket_bytes, monitor_interval, overlap)
    dev = opt._kf_result_device()
    opt._kf_var = torch.zeros(len(opt._kf_params), dtype=torch.float64, device=dev)
    opt._kf_var_total = torch.zeros((), dtype=torch.float64, device=dev)
    return opt


class _SMA(_Bucketed):
    def _kf_build_sma(self):
        self._kf_build(None)
        for ps, gb in self._kf_groups:  # move the variables into buckets
            for p, view in zip(ps, gb.views):
                v = view.view_as(p)
                v.copy_(p.data)
                p.data = v

    def sync_variables(self):
        if self._kf_groups is None:
            self._kf_build_sma()
        if self._kf_overlap:
            return self._kf_sync_overlapped()
        for ps, gb in self._kf_groups:
            # sma_sgd.py:53-57: only variables that have a gradient take part;
            # others are restored after the blend
            saved = [(p, p.data.clone()) for p in ps if p.grad is None]
            self._kf_ex.sma_(gb.buckets, self._kf_alpha)
            for p, d in saved:
                p.data.copy_(d)

    # overlap=True: the sum of the variables is all-reduced while the next
    # step's forward and backward run. SMA reduces v_t, the variables the
    # step's forward used (sma_sgd.py:60-65: group_all_reduce(variables)
    # before the blend and the gradient update), and they do not change
    # between the end of step t-1 and the blend of step t, so the sum can
    # start as soon as step t-1 has updated them — on the exchange's own
    # stream, into a workspace per bucket (out of place on the native
    # exchange; a copy, then in place, on collective.Exchange) — and step t
    # only waits for it and blends. The collectives and the blend kernel are those of sma_(), so the
    # result is the same bit for bit.
    def _kf_start_sums(self):
        if self._kf_sums is None:
            from .collective import workspace_like
            self._kf_sums = [workspace_like(gb.buckets) for _, gb in self._kf_groups]
        self._kf_pending = []
        into = getattr(self._kf_ex, "start_into_", None)
        for gi, ((_, gb), sums) in enumerate(zip(self._kf_groups, self._kf_sums)):
            if into is not None:  # the native exchange: out of place, no copy
                self._kf_pending.append(into(gb.buckets, sums, op="sum"))
                continue
            for s, b in zip(sums, gb.buckets):
                s.copy_(b)
            self._kf_pending.append(self._kf_ex.start_(sums, op="sum", average=False,
                                                       coalesce=False, key=("sma", gi)))

    def _kf_sync_overlapped(self):
        if self._kf_pending is None:  # the first step: nothing started yet
            self._kf_start_sums()
        world = self._kf_ex.world
        epilogue = getattr(self._kf_ex, "epilogue", None)
        for (ps, gb), sums, h in zip(self._kf_groups, self._kf_sums, self._kf_pending):
            saved = [(p, p.data.clone()) for p in ps if p.grad is None]
            h.wait()
            if epilogue is not None:  # collective.Exchange: its own epilogue
                for b, s in zip(gb.buckets, sums):
                    epilogue.sma_blend_(b, s, world, self._kf_alpha)
            else:  # the native exchange's blend: the batched HIP kernel
                from . import ops
                ops.sma_blend_batch_(gb.buckets, sums, world, self._kf_alpha)
            for p, d in saved:
                p.data.copy_(d)
        self._kf_pending = None

    def step(self, closure=None):
        self.sync_variables()
        _finish(self._kf_ex)
        out = super().step(closure)
        if self._kf_overlap:  # v_{t+1} is final: start its sum now
            self._kf_start_sums()
        return out

    def wait_overlap(self):
        """overlap=True leaves the next step's sum in flight when step()
        returns. After the last step, wait for it here (collective: every
        rank) before the process group or the exchange is torn down under
        it. A later step() starts the sum again, so the values are the same
        either way."""
        for h in self._kf_pending or []:
            h.wait()
        self._kf_pending = None


def SynchronousAveragingOptimizer(optimizer, named_parameters=None, alpha=0.1,
                                  exchange=None, bucket_bytes=32 << 20, overlap=False):
    """SMA: v <- (1 - alpha) v + alpha * mean_ranks(v) before each local step
    (sma_sgd.py:50-74).

    overlap=True starts the all-reduce of the next step's variables at the
    end of step() on the exchange's stream, so it runs during that step's
    forward and backward; step() then waits for it and blends. Same values as
    overlap=False, provided the variables change only through step() (the
    first step reduces synchronously). The last step leaves a sum in flight:
    call wait_overlap() before destroying the process group."""
    opt = _wrap(optimizer, _SMA)
    opt._kf_setup(named_parameters, exchange, bucket_bytes)
    opt._kf_alpha = float(alpha)
    opt._kf_overlap = bool(overlap)
    opt._kf_sums = None
    opt._kf_pending = None
    if opt._kf_overlap and not hasattr(opt._kf_ex, "start_"):
        raise ValueError("overlap=True needs an exchange with start_() "
                         "(collective.Exchange or exchange.NativeExchange)")
    return opt


class _PairAveraging:
    """AD-PSGD (async_sgd.py): no exchange and no collective in a step. The
    variables live in buckets like `_SMA`'s; one pairavg.PeerModelStore per
    dtype group publishes them and pulls a peer's. Everything that touches
    the device is built on the first step."""

    def _kf_setup_pair(self, named_parameters, bucket_bytes, slots, seed, peer_selector):
        import torch
        if int(slots) < 2:
            raise ValueError("slots must be at least 2")
        if named_parameters is None:
            params = [p for g in self.param_groups for p in g["params"]]
        else:
            params = [p for _, p in named_parameters]
        for p in params:  # an integer parameter cannot require a gradient: check all
            if p.dtype not in (torch.float32, torch.float16, torch.bfloat16, torch.float64):
                raise ValueError("PairAveragingOptimizer averages f32, f16, bf16 and f64 "
                                 "parameters, not %s" % p.dtype)
        self._kf_params = [p for p in params if p.requires_grad]
        if len({p.device for p in self._kf_params}) > 1:
            raise ValueError("PairAveragingOptimizer: parameters on more than one device")
        self._kf_bucket_bytes = bucket_bytes
        self._kf_slots = int(slots)
        self._kf_seed = seed
        self._kf_selector = peer_selector
        self._kf_rng = None
        self._kf_groups = None
        self._kf_stores = None
        self._kf_step = 0
        self._kf_last_target = None

    @staticmethod
    def _kf_world_rank():
        import torch.distributed as dist
        if dist.is_initialized():
            return dist.get_world_size(), dist.get_rank()
        return 1, 0

    def _kf_select(self):
        world, rank = self._kf_world_rank()
        if self._kf_selector is not None:
            target = int(self._kf_selector(self._kf_step, rank, world))
        else:
            if self._kf_rng is None:
                import random
                # the generator stays on the host; without a seed every rank
                # draws its own sequence
                self._kf_rng = random.Random(self._kf_seed if self._kf_seed is not None
                                             else 0x9E3779B1 * (rank + 1))
            from .pairavg import random_peer
            target = random_peer(self._kf_rng, world, rank)
        if not 0 <= target < world:
            raise ValueError("peer_selector returned %d, outside [0, %d)" % (target, world))
        return target

    def _kf_build_pair(self):
        import torch
        import torch.distributed as dist
        from .pairavg import PeerModelStore
        groups = {}
        for p in self._kf_params:
            groups.setdefault((p.dtype, p.device), []).append(p)
        self._kf_groups, self._kf_stores = [], []
        for (dtype, device), ps in groups.items():
            # the buckets are never exchanged in shards: no padding for a world
            gb = GradBuckets([p.numel() for p in ps], dtype, device, 1,
                             bucket_bytes=self._kf_bucket_bytes)
            for p, view in zip(ps, gb.views):  # move the variables into buckets
                v = view.view_as(p)
                v.copy_(p.data)
                p.data = v
            self._kf_groups.append((ps, gb))
            self._kf_stores.append(PeerModelStore(
                [b[:sp] for b, sp in zip(gb.buckets, gb.spans)], slots=self._kf_slots))
        # init_store + barrier (async_sgd.py:113-121): after it no peer finds
        # version 0
        for st in self._kf_stores:
            st.publish()
        torch.cuda.current_stream().synchronize()
        if dist.is_initialized() and dist.get_world_size() > 1:
            dist.barrier()

    def step(self, closure=None):
        target = self._kf_select()
        if self._kf_stores is None:
            self._kf_build_pair()
        for (ps, gb), st in zip(self._kf_groups, self._kf_stores):
            # only variables that have a gradient take part (async_sgd.py:
            # 110-112 pairs grads_and_vars); others are restored after the blend
            saved = [(p, p.data.clone()) for p in ps if p.grad is None]
            st.pull_average_(target)
            for p, d in saved:
                p.data.copy_(d)
        self._kf_last_target = target
        out = super().step(closure)
        for st in self._kf_stores:
            st.publish()
        self._kf_step += 1
        return out

    @property
    def pair_counters(self):
        """{valid, torn, empty, published} of the pulls and publishes so far,
        summed over the dtype groups (one store each). Waits for the device."""
        tot = dict.fromkeys(("valid", "torn", "empty", "published"), 0)
        for st in self._kf_stores or []:
            for k, v in st.counters().items():
                tot[k] += v
        return tot

    @property
    def last_target(self):
        """The peer the last step pulled from (None before the first)."""
        return self._kf_last_target

    def close(self):
        """Collective: release the stores (PeerModelStore.close)."""
        for st in self._kf_stores or []:
            st.close()
        self._kf_stores = None


def PairAveragingOptimizer(optimizer, named_parameters=None, bucket_bytes=32 << 20, slots=2,
                           seed=None, peer_selector=None):
    """AD-PSGD (async_sgd.py:110-142). Each step: pull a peer's latest
    published model out of its HBM and average it into the variables
    (v = 0.5 * (v + other), pairavg.PeerModelStore), run the wrapped
    optimizer's step on the gradients already computed, publish the result.
    The first step first publishes the initial model and joins a barrier, so
    that no peer finds an empty store afterwards. No rank ever waits for
    another after that: a pull that would mix two versions is skipped and
    counted (`pair_counters`).

    The peer is the reference's random choice (pairavg.random_peer, host-side
    random.Random(seed), or a per-rank sequence without a seed) unless
    `peer_selector(step, rank, world) -> int` gives it; `last_target` is the
    last one. Parameters live on one device and are f32, f16, bf16 or f64.
    RCCL plays no part."""
    opt = _wrap(optimizer, _PairAveraging)
    opt._kf_setup_pair(named_parameters, bucket_bytes, slots, seed, peer_selector)
    return opt


class _Sharded(_Bucketed):
    """What the sharded optimizers share. Parameters and gradients live in
    two GradBuckets of identical layout per (param group, dtype, device); the
    optimizer state is one shard (1 / world of the elements) per bucket and
    state tensor."""

    _kf_name = ""          # the public constructor, for messages
    _kf_dtypes = ()        # torch dtype names the update kernel takes
    _kf_dtype_words = ""

    def _kf_new_group(self):
        """The state entries of a new bucket group."""
        return {}

    def _kf_build_sharded(self):
        import torch
        mine = {id(p) for p in self._kf_params}
        self._kf_groups = []
        for gi, group in enumerate(self.param_groups):
            by = {}
            for p in group["params"]:
                if id(p) in mine:
                    by.setdefault((p.dtype, p.device), []).append(p)
            for (dtype, device), ps in by.items():
                if dtype not in tuple(getattr(torch, n) for n in self._kf_dtypes):
                    raise TypeError("%s updates %s parameters, not %s"
                                    % (self._kf_name, self._kf_dtype_words, dtype))
                numels = [p.numel() for p in ps]
                pb = GradBuckets(numels, dtype, device, self._kf_ex.world,
                                 bucket_bytes=self._kf_bucket_bytes)
                gb = GradBuckets(numels, dtype, device, self._kf_ex.world,
                                 bucket_bytes=self._kf_bucket_bytes)
                for p, view in zip(ps, pb.views):  # move the variables into buckets
                    v = view.view_as(p)
                    v.copy_(p.data)
                    p.data = v
                G = {"gi": gi, "ps": ps, "pb": pb, "gb": gb}
                G.update(self._kf_new_group())
                self._kf_groups.append(G)

    def _kf_zero_shards(self, G, dtype=None):
        """One zeroed state shard per bucket of the group, of the buckets'
        dtype or of `dtype`."""
        import torch
        world = self._kf_ex.world
        return [torch.zeros(b.numel() // world, dtype=dtype or b.dtype, device=b.device)
                for b in G["pb"].buckets]

    def _kf_closure(self, closure):
        if closure is None:
            return None
        import torch
        with torch.enable_grad():
            return closure()

    def _kf_gather(self, shard):
        """All ranks' shards of one bucket, in rank order. The shards travel
        as integers through the exchange's sum, with zeros everywhere else, so
        every bit arrives as it is (16-bit patterns widened to int32, which
        every transport sums)."""
        import torch
        ex = self._kf_ex
        q = shard.numel()
        if ex.world == 1:
            return shard.clone()
        if shard.element_size() == 2:
            full = torch.zeros(q * ex.world, dtype=torch.int32, device=shard.device)
            full[ex.rank * q:(ex.rank + 1) * q].copy_(shard.view(torch.int16))
            ex.all_reduce_([full], op="sum", average=False)
            return full.to(torch.int16).view(shard.dtype)
        ints = torch.int32 if shard.element_size() == 4 else torch.int64
        full = torch.zeros(q * ex.world, dtype=shard.dtype, device=shard.device)
        full[ex.rank * q:(ex.rank + 1) * q].copy_(shard)
        ex.all_reduce_([full.view(ints)], op="sum", average=False)
        return full

    def _kf_unshard(self, G, shards):
        """Collective: {parameter: its full state tensor} of one group, from
        the ranks' shards of one state (a new tensor each)."""
        out = {}
        off = {}
        for p, v in zip(G["ps"], G["pb"].views):
            off[id(p)] = v.data_ptr()
        for b, m in zip(G["pb"].buckets, shards):
            full = self._kf_gather(m)
            lo, hi = b.data_ptr(), b.data_ptr() + b.numel() * b.element_size()
            for p in G["ps"]:
                at = off[id(p)]
                if lo <= at < hi and p.numel():
                    i = (at - lo) // b.element_size()
                    out[p] = full[i:i + p.numel()].view_as(p).clone()
        return out

    def _kf_reshard(self, G, shards, tensor_of):
        """This rank's slice of every bucket of one state into `shards`:
        tensor_of(p) is the parameter's full state tensor, or None (zeros)."""
        import torch
        ex = self._kf_ex
        for b, m in zip(G["pb"].buckets, shards):
            full = torch.zeros(b.numel(), dtype=m.dtype, device=b.device)
            lo, hi = b.data_ptr(), b.data_ptr() + b.numel() * b.element_size()
            for p, v in zip(G["ps"], G["pb"].views):
                t = tensor_of(p) if lo <= v.data_ptr() < hi and p.numel() else None
                if t is not None:
                    i = (v.data_ptr() - lo) // b.element_size()
                    full[i:i + p.numel()].copy_(t.reshape(-1))
            q = m.numel()
            m.copy_(full[ex.rank * q:(ex.rank + 1) * q])


class _ShardedSGD(_Sharded):
    """reduce-scatter(grads) -> SGD update on the own shard -> all-gather(params).
    The momentum is one shard per bucket."""

    _kf_name = "ShardedSGDOptimizer"
    _kf_dtypes = ("float32", "float16", "bfloat16", "float64")
    _kf_dtype_words = "f32, f16, bf16 and f64"

    def _kf_new_group(self):
        return {"moms": None, "first": True}

    def _kf_moms(self, G):
        """The group's zeroed momentum shards, allocated when first needed."""
        if G["moms"] is None:
            G["moms"] = self._kf_zero_shards(G)
            G["first"] = True
        return G["moms"]

    def step(self, closure=None):
        loss = self._kf_closure(closure)
        if self._kf_groups is None:
            self._kf_build_sharded()
        for G in self._kf_groups:
            _SyncSGD._kf_place(G["ps"], G["gb"])
        for G in self._kf_groups:
            pg = self.param_groups[G["gi"]]  # read at every step: schedulers change them
            mu = float(pg["momentum"])
            moms = self._kf_moms(G) if mu != 0 else None
            h = {"lr": float(pg["lr"]), "momentum": mu, "dampening": float(pg["dampening"]),
                 "weight_decay": float(pg["weight_decay"]), "nesterov": bool(pg["nesterov"]),
                 "first": G["first"]}
            nb = len(G["pb"].buckets)
            self._kf_ex.sgd_step_(G["pb"].buckets, G["gb"].buckets, moms, [h] * nb)
            if mu != 0:
                G["first"] = False
        _finish(self._kf_ex)
        return loss

    def momentum_buffers(self):
        """Collective: {parameter: its full momentum buffer}, gathered from
        the ranks' shards (a new tensor each; empty for a group that has not
        yet stepped with momentum). With load_momentum_buffers, the
        checkpoint path: `state` stays empty, so state_dict() carries no
        momentum."""
        out = {}
        for G in self._kf_groups or []:
            if G["moms"] is None or G["first"]:
                continue
            out.update(self._kf_unshard(G, G["moms"]))
        _finish(self._kf_ex)
        return out

    def load_momentum_buffers(self, mapping):
        """{parameter: full momentum buffer} (momentum_buffers' result, on
        every rank): each rank keeps its own slice of every bucket, and the
        next step is no longer a group's first. A group none of whose
        parameters is in `mapping` is left as it is; a parameter missing from
        a loaded group gets zeros."""
        if self._kf_groups is None:
            self._kf_build_sharded()
        for G in self._kf_groups:
            if not any(p in mapping for p in G["ps"]):
                continue
            self._kf_reshard(G, self._kf_moms(G), mapping.get)
            G["first"] = False


class _AdamState:
    """The storage variant of one Adam bucket group: where its
    exp_avg / exp_avg_sq shards live, how they are zeroed, updated with and
    without a gate, and presented to and restored from a checkpoint. Made once,
    with the buckets; what a step needs of the exchange is bound then. This one
    is the plain variant: state in the buckets' dtype, updated by the
    exchange's fused step. o is the optimizer, G the group's dict."""

    def __init__(self, o, G):
        self.o, self.G, self.ex = o, G, o._kf_ex
        self.pb, self.gb = G["pb"].buckets, G["gb"].buckets

    def zero(self, dtype=None):
        G = self.G
        G["m"], G["v"] = (self.o._kf_zero_shards(G, dtype) for _ in range(2))

    def step(self, j, h):
        G = self.G
        self.ex.adam_step_(self.pb, self.gb, G["m"], G["v"], [h] * len(self.pb))

    def step_gated(self, j, h):
        o, G = self.o, self.G
        self.ex.adam_gated_step_(self.pb, self.gb, G["w"], G["m"], G["v"], h, G["np"], o._kf_gate,
                                 o._kf_gstates, j, ("gated", j))

    def present(self):
        """Collective: {entry of state_buffers(): {parameter: full tensor}}."""
        o, G = self.o, self.G
        return {"exp_avg": o._kf_unshard(G, G["m"]), "exp_avg_sq": o._kf_unshard(G, G["v"])}

    def restore(self, mapping, step):
        """load_state_buffers' mapping into this rank's shards."""
        o, G = self.o, self.G
        for key, shards in (("exp_avg", G["m"]), ("exp_avg_sq", G["v"])):
            o._kf_reshard(G, shards, lambda p, key=key: mapping[p][key] if p in mapping else None)


class _WithMaster:
    """Beside a variant: G["w"], the fp32 master shards, as "master"."""

    def present(self):
        out = super().present()
        out["master"] = self.o._kf_unshard(self.G, self.G["w"])
        return out

    def restore(self, mapping, step):
        super().restore(mapping, step)
        self.o._kf_reshard(self.G, self.G["w"],
                           lambda p: mapping.get(p, {}).get("master", p.data))


class _AdamMaster(_WithMaster, _AdamState):
    """16-bit parameters through fp32 masters and fp32 state."""

    def zero(self):
        import torch
        super().zero(torch.float32)

    def step(self, j, h):
        G = self.G
        self.ex.adam_master_step_(self.pb, self.gb, G["w"], G["m"], G["v"], [h] * len(self.pb))


class _AdamOnShards(_AdamState):
    """A variant whose update is not the exchange's own: reduce-scatter, the
    epilogue's update(...) on this rank's shards, all-gather. `key` names the
    exchange's workspace of the ungated step, `probe` the method by which an
    injected epilogue is told from the HIP one, `name` the epilogue's ungated
    update (its gated twin ends in gated_). The slices of the parameter buckets
    that are this rank's never move, so they are made here."""

    def __init__(self, o, G, key, probe, name):
        super().__init__(o, G)
        self.key, self.ep, self.mine = key, o._kf_ops(probe), o._kf_mine(G)
        self.run, self.run_gated = getattr(self.ep, name), getattr(self.ep, name + "gated_")

    def step(self, j, h):
        ex = self.ex
        np_ = ex.reduce_shards_(self.gb, (self.key, j))
        self.update(ex.grad_shards_(self.gb, (self.key, j)), [h] * len(self.pb), np_, ())
        ex.gather_params_(self.pb)

    def step_gated(self, j, h):
        o = self.o
        self.update(self.ex.grad_shards_(self.gb, ("gated", j)), h, self.G["np"],
                    (o._kf_gate, o._kf_gstates, j))
        self.ex.gather_params_(self.pb)


class _AdamSR(_AdamOnShards):
    """bf16 state and stochastic rounding; "sr_draw" is the
    host's count of draws."""

    def __init__(self, o, G):
        super().__init__(o, G, "sr", "adam_sr_update_", "adam_sr_update_")
        self.bases = [self.ex.rank * m.numel() for m in self.mine]  # offsets in the buckets

    def update(self, shards, hyper, np_, gated):
        G = self.G
        G["draw"] += 1  # the host's count: a step the device skips draws too
        (self.run_gated if gated else self.run)(
            self.mine, shards, G["m"], G["v"], hyper, *gated, np_, self.bases, G["streams"],
            G["draw"] & 0xffffffff)

    def present(self):
        out = super().present()
        out["sr_draw"] = {p: self.G["draw"] for p in out["exp_avg"]}
        return out

    def restore(self, mapping, step):
        super().restore(mapping, step)
        draws = {int(mapping[p]["sr_draw"]) for p in self.G["ps"]
                 if p in mapping and "sr_draw" in mapping[p]}
        if len(draws) > 1:
            raise ValueError("load_state_buffers: the parameters of one group differ in "
                             "sr_draw: %s" % sorted(draws))
        self.G["draw"] = draws.pop() if draws else step


class _Adam8(_AdamOnShards):
    """exp_avg / exp_avg_sq as block-wise 8-bit codes G["m"], G["v"] and f32
    scales G["ms"], G["vs"]; a checkpoint holds them
    dequantized, a form that does not depend on world or layout."""

    parts = (("exp_avg", "m", "ms"), ("exp_avg_sq", "v", "vs"))  # of table 0 and of table 1

    def __init__(self, o, G, name="adam8_update_"):
        super().__init__(o, G, "adam8", "adam8_update_", name)

    def zero(self):
        # the zero state: scale 0, exp_avg code 127, exp_avg_sq code 0
        import torch
        from .ops import ADAM8_BLOCK, ADAM8_ZERO_CODE
        o, G = self.o, self.G
        for key, code in zip(("m", "v"), ADAM8_ZERO_CODE):
            G[key] = o._kf_zero_shards(G, torch.uint8)
            for c in G[key]:
                c.fill_(code)
        for key in ("ms", "vs"):
            G[key] = [torch.zeros(c.numel() // ADAM8_BLOCK, dtype=torch.float32, device=c.device)
                      for c in G["m"]]

    def update(self, shards, hyper, np_, gated):
        G = self.G
        (self.run_gated if gated else self.run)(
            self.mine, shards, G["m"], G["v"], G["ms"], G["vs"], hyper, *gated, np_)

    def present(self):
        o, G, ep = self.o, self.G, self.ep
        return {key: o._kf_unshard(G, [ep.adam8_dequantize(c, x, which)
                                       for c, x in zip(G[codes], G[scales])])
                for which, (key, codes, scales) in enumerate(self.parts)}

    def restore(self, mapping, step):
        # requantized; idempotent on what present() gave
        import torch
        o, G, ep = self.o, self.G, self.ep
        for which, (key, codes, scales) in enumerate(self.parts):
            full = [torch.zeros(c.numel(), dtype=torch.float32, device=c.device) for c in G[codes]]
            o._kf_reshard(G, full, lambda p, key=key: mapping[p][key] if p in mapping else None)
            for x, c, sc in zip(full, G[codes], G[scales]):
                ep.adam8_quantize_(x, which, c, sc)


class _Adam8Master(_WithMaster, _Adam8):
    """8-bit state beside fp32 masters of 16-bit parameters."""

    def __init__(self, o, G):
        super().__init__(o, G, "adam8_master_update_")

    def update(self, shards, hyper, np_, gated):
        G = self.G
        (self.run_gated if gated else self.run)(
            self.mine, shards, G["w"], G["m"], G["v"], G["ms"], G["vs"], hyper, *gated, np_)


# (8-bit state, master weights) -> the variant; stochastic rounding comes first
_ADAM_STATES = {(False, False): _AdamState, (False, True): _AdamMaster,
                (True, False): _Adam8, (True, True): _Adam8Master}


class _ShardedAdam(_Sharded):
    """reduce-scatter(grads) -> Adam / AdamW update on the own shard ->
    all-gather(params). exp_avg and exp_avg_sq are one shard each per bucket;
    one step counter per bucket group. With master weights a bf16 / f16 group
    has a third shard per bucket, "w", the fp32 master copy of this rank's
    slice of the parameters, and its exp_avg / exp_avg_sq shards are fp32."""

    _kf_name = "ShardedAdamOptimizer"
    _kf_dtypes = ("float32", "bfloat16", "float64")
    _kf_dtype_words = "f32, bf16 and f64"
    _kf_decoupled = False
    _kf_master = False
    _kf_sr = False      # stochastic rounding of the bf16 groups
    _kf_sr_seed = 0
    _kf_state_bits = 32  # 8: exp_avg / exp_avg_sq as block-wise codes

    def _kf_new_group(self):
        return {"m": None, "v": None, "w": None, "step": 0, "sr": False, "draw": 0, "b8": False,
                "ms": None, "vs": None}

    def _kf_build_sharded(self):
        import torch
        super()._kf_build_sharded()
        ex = self._kf_ex
        for G in self._kf_groups if self._kf_master else []:
            if G["pb"].buckets and G["pb"].buckets[0].element_size() == 2:
                G["w"] = self._kf_zero_shards(G, torch.float32)
                for b, w in zip(G["pb"].buckets, G["w"]):  # the widening is exact
                    q = w.numel()
                    w.copy_(b[ex.rank * q:(ex.rank + 1) * q])
        for j, G in enumerate(self._kf_groups if self._kf_sr else []):
            if G["pb"].buckets and G["pb"].buckets[0].dtype == torch.bfloat16:
                G["sr"] = True
                G["streams"] = [sr_stream_word(self._kf_sr_seed, j, i)
                                for i in range(len(G["pb"].buckets))]
        for G in self._kf_groups:
            # 8-bit state: the dtypes were checked when the optimizer was made
            G["b8"] = self._kf_state_bits == 8
            kind = _AdamSR if G["sr"] else _ADAM_STATES[G["b8"], G["w"] is not None]
            G["var"] = kind(self, G)
        if self._kf_gated:
            self._kf_build_gated()

    def _kf_ops(self, probe):
        """Where a family of device steps runs: the exchange's epilogue if it
        has the method `probe` (collective.Exchange; injectable for CPU
        tests), else the HIP one."""
        from .collective import HipEpilogue
        ep = getattr(self._kf_ex, "epilogue", None)
        return ep if hasattr(ep, probe) else HipEpilogue()

    def _kf_mine(self, G):
        """This rank's slices of the group's parameter buckets."""
        ex = self._kf_ex
        q = [b.numel() // ex.world for b in G["pb"].buckets]
        return [b[ex.rank * n:(ex.rank + 1) * n] for b, n in zip(G["pb"].buckets, q)]

    def _kf_states(self, G):
        """The group's exp_avg / exp_avg_sq shards, zeroed by its variant on
        the first step."""
        if G["m"] is None:
            G["var"].zero()
        return G["m"], G["v"]

    def _kf_hyper(self, G, **more):
        """The group's hyper, read at every step (schedulers change them), with
        what the caller adds: step, adapt."""
        pg = self.param_groups[G["gi"]]
        return dict(lr=float(pg["lr"]), betas=tuple(float(b) for b in pg["betas"]),
                    eps=float(pg["eps"]), weight_decay=float(pg["weight_decay"]),
                    decoupled=self._kf_decoupled, **more)

    # -- the gated step ---------------------------------------
    _kf_gated = False
    _kf_max_norm = 0.0
    _kf_rule = None     # init_scale, growth_factor, backoff_factor, growth_interval
    _kf_gate = None     # kf_step_gate on the device, a uint8 tensor
    _kf_gstates = None  # kf_step_state per bucket group

    def _kf_gate_tensor(self):
        """The gate, created when first needed (scale_loss comes before the
        first step) on the parameters' device."""
        if self._kf_gate is None:
            from . import ops
            devices = {p.device for p in self._kf_params}
            if len(devices) != 1:
                raise ValueError("%s: a gated step needs all parameters on one device"
                                 % self._kf_name)
            self._kf_gate = ops.new_step_gate(devices.pop(), self._kf_rule["init_scale"])
        return self._kf_gate

    def _kf_build_gated(self):
        """Once, with the buckets: the groups' step states, one norm plan per
        dtype over this rank's gradient shards (fixed addresses), and the
        buffers of the plans' sums of squares."""
        import torch
        from . import ops
        gate, ex, ep = self._kf_gate_tensor(), self._kf_ex, self._kf_ops("step_gate_update_")
        self._kf_gstates = ops.new_step_states(gate.device, len(self._kf_groups))
        by = {}
        for j, G in enumerate(self._kf_groups):
            by.setdefault(G["pb"].buckets[0].dtype, []).append(j)
        self._kf_plans = []
        for dtype, js in by.items():
            shards = [t for j in js
                      for t in ex.grad_shards_(self._kf_groups[j]["gb"].buckets, ("gated", j))]
            plan = ep.sq_norm_plan(shards)
            out = torch.zeros(len(shards) + 1, dtype=torch.float64, device=gate.device)
            self._kf_plans.append((js, plan, out))
        n = len(self._kf_plans)
        self._kf_sq = torch.zeros(n, dtype=torch.float64, device=gate.device)
        self._kf_sq_all = torch.zeros(n * ex.world, dtype=torch.float64, device=gate.device)

    def _kf_gate_verdict(self, gate_lr=None):
        """A (every group's reduce), B (the norm pass), C (the all-gather of
        the plans' sums), D (the verdict): queued, nothing waits. Returns
        every group's hyper. gate_lr: the lr the step states are advanced
        with in place of the groups' own (LAMB: 1.0)."""
        ex, ep, groups = self._kf_ex, self._kf_ops("step_gate_update_"), self._kf_groups
        for j, G in enumerate(groups):
            self._kf_states(G)
            G["np"] = ex.reduce_shards_(G["gb"].buckets, ("gated", j))
        nps = []
        for k, (js, plan, out) in enumerate(self._kf_plans):
            if len({groups[j]["np"] for j in js}) != 1:
                raise ValueError("%s: bucket groups of one dtype were reduced differently"
                                 % self._kf_name)
            nps.append(groups[js[0]]["np"])
            plan.run("sq", out=out)
            self._kf_sq[k:k + 1].copy_(out[-1:])
        ex.gather_doubles_(self._kf_sq, self._kf_sq_all)
        hs = [self._kf_hyper(G) for G in groups]
        r = self._kf_rule
        ghs = hs if gate_lr is None else [dict(h, lr=float(gate_lr)) for h in hs]
        ep.step_gate_update_(self._kf_sq_all, ex.world, nps, ghs, self._kf_gstates, self._kf_gate,
                             max_norm=self._kf_max_norm, growth_factor=r["growth_factor"],
                             backoff_factor=r["backoff_factor"],
                             growth_interval=r["growth_interval"])
        return hs

    def _kf_step_gated(self):
        """A to D (_kf_gate_verdict), E (every group's gated update and the
        parameters' all-gather): queued, nothing waits for the verdict."""
        for j, (G, h) in enumerate(zip(self._kf_groups, self._kf_gate_verdict())):
            G["var"].step_gated(j, h)

    _kf_gate_words = "max_grad_norm or loss_scale"  # what turns the gate on

    def _kf_need_gate(self, what):
        if not self._kf_gated:
            raise ValueError("%s.%s needs %s" % (self._kf_name, what, self._kf_gate_words))

    def scale_loss(self, loss):
        """loss * loss_scale, a device multiply by the gate's current scale:
        no host sync. Call backward() on the result."""
        import torch
        self._kf_need_gate("scale_loss")
        # kf_step_gate.loss_scale: the fp32 word at byte 8
        return loss * self._kf_gate_tensor()[8:12].view(torch.float32)[0]

    def _kf_read_gate(self):
        from . import ops
        self._kf_need_gate("gate state")
        return ops.read_step_gate(self._kf_gate_tensor())

    def loss_scale_value(self):
        """The loss scale the next loss is to be multiplied by (synchronises)."""
        return float(self._kf_read_gate()["loss_scale"])

    def last_grad_norm(self):
        """The last step's norm of the unscaled, averaged gradient before
        clipping; inf or NaN on a skipped step (synchronises)."""
        return float(self._kf_read_gate()["grad_norm"])

    def skipped_steps(self):
        """Steps skipped so far for non-finite gradients (synchronises)."""
        return int(self._kf_read_gate()["skipped"])

    def applied_steps(self):
        """Steps applied so far (synchronises)."""
        return int(self._kf_read_gate()["applied"])

    def scaler_state(self):
        """{"loss_scale", "good_steps"}: the loss scale and its growth tracker,
        for a checkpoint beside state_buffers() (synchronises)."""
        g = self._kf_read_gate()
        return {"loss_scale": float(g["loss_scale"]), "good_steps": int(g["good_steps"])}

    def load_scaler_state(self, state):
        """scaler_state()'s result back into the gate; the counters of
        applied and skipped steps start again at zero."""
        import numpy as np
        import torch
        from . import _lib
        self._kf_need_gate("load_scaler_state")
        gate = self._kf_gate_tensor()
        a = np.zeros(1, _lib.step_gate_dtype())
        a["loss_scale"], a["good_steps"] = float(state["loss_scale"]), int(state["good_steps"])
        gate.copy_(torch.from_numpy(a.view(np.uint8).copy()))

    def _kf_steps(self):
        """Every bucket group's step count: the device's on the gated path."""
        if not self._kf_gated or self._kf_gstates is None:
            return [G["step"] for G in self._kf_groups or []]
        from . import ops
        return [int(t) for t in ops.read_step_states(self._kf_gstates)["step"]]

    def step(self, closure=None):
        loss = self._kf_closure(closure)
        if self._kf_groups is None:
            self._kf_build_sharded()
        for G in self._kf_groups:
            _SyncSGD._kf_place(G["ps"], G["gb"])
        if self._kf_gated:
            self._kf_step_gated()
            _finish(self._kf_ex)
            return loss
        for j, G in enumerate(self._kf_groups):
            if G["m"] is None:
                G["var"].zero()
            G["step"] += 1
            G["var"].step(j, self._kf_hyper(G, step=G["step"]))
        _finish(self._kf_ex)
        return loss

    def state_buffers(self):
        """Collective: {parameter: {"step": int, "exp_avg": tensor,
        "exp_avg_sq": tensor}}, the full state tensors gathered from the
        ranks' shards (new tensors; empty for a group that has not stepped).
        With load_state_buffers, the checkpoint path: `state` stays empty, so
        state_dict() carries no Adam state. A bf16 / f16 group with master
        weights gives fp32 exp_avg and exp_avg_sq and a third entry, "master",
        the fp32 master copy of the parameter."""
        out = {}
        # gated: the step counts are the device's (skipped steps do not count)
        for G, step in zip(self._kf_groups or [], self._kf_steps()):
            if G["m"] is None or step == 0:
                continue
            for key, full in G["var"].present().items():
                for p, t in full.items():
                    out.setdefault(p, {"step": step})[key] = t
        _finish(self._kf_ex)
        return out

    def load_state_buffers(self, mapping):
        """{parameter: {"step", "exp_avg", "exp_avg_sq"}} (state_buffers'
        result, on every rank): each rank keeps its own slice of every
        bucket, and the group goes on from `step`. A group none of whose
        parameters is in `mapping` is left as it is; a parameter missing from
        a loaded group gets zeros. The parameters of one group must agree on
        `step` (ValueError otherwise). In a group with master weights a
        parameter's "master" entry becomes its master copy; where the entry
        (or the parameter) is absent, the master is the current 16-bit
        parameter widened again, which drops what the master held below the
        16-bit precision. The parameters themselves are not touched: the
        caller restores them as usual, and the next step rewrites them from
        the master."""
        if self._kf_groups is None:
            self._kf_build_sharded()
        for j, G in enumerate(self._kf_groups):
            steps = {int(mapping[p]["step"]) for p in G["ps"] if p in mapping}
            if not steps:
                continue
            if len(steps) > 1:
                raise ValueError("load_state_buffers: the parameters of one group differ in "
                                 "step: %s" % sorted(steps))
            self._kf_states(G)
            G["step"] = steps.pop()
            G["var"].restore(mapping, G["step"])
            if self._kf_gated:
                self._kf_seed_state(j, G["step"], self.param_groups[G["gi"]]["betas"])

    def _kf_seed_state(self, j, step, betas):
        """Bucket group j's device step state resumed at `step`: the running
        products start from Python's beta ** step."""
        import numpy as np
        import torch
        from . import _lib, ops
        a = ops.read_step_states(self._kf_gstates).copy()
        a[j] = np.zeros(1, _lib.step_state_dtype())[0]
        a["step"][j] = step
        a["beta1_pow"][j], a["beta2_pow"][j] = float(betas[0]) ** step, float(betas[1]) ** step
        self._kf_gstates.copy_(torch.from_numpy(a.view(np.uint8).copy()))


def splitmix64(x):
    """One step of SplitMix64 (Steele, Lea, Flood 2014) on a 64-bit word:
    z = x + 0x9E3779B97F4A7C15; z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9;
    z = (z ^ z >> 27) * 0x94D049BB133111EB; z ^ z >> 31, all modulo 2^64."""
    mask = (1 << 64) - 1
    z = (x + 0x9E3779B97F4A7C15) & mask
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & mask
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & mask
    return z ^ (z >> 31)


def sr_stream_word(sr_seed, group_index, bucket_index):
    """The Philox stream word of one bucket of a stochastic-rounding group:
    low32(splitmix64(splitmix64(sr_seed) ^ (group_index << 32 | bucket_index)))."""
    return splitmix64(splitmix64(sr_seed) ^ (group_index << 32 | bucket_index)) & 0xffffffff


def lamb_pieces(gb, world, rank):
    """The "tensor ∩ shard" pieces of one GradBuckets layout on `rank`:
    [(tensor, bucket, offset, count)] with `offset` counted from the start of
    the rank's shard of that bucket, one entry per tensor that has elements
    there (a tensor is contiguous in one bucket, so it has at most one piece
    per rank). Bucket padding lies in no piece; a tensor of zero elements has
    none."""
    out = []
    for t, v in enumerate(gb.views):
        n = v.numel()
        if n == 0:
            continue
        for j, b in enumerate(gb.buckets):
            lo = b.data_ptr()
            if lo <= v.data_ptr() < lo + b.numel() * b.element_size():
                break
        else:
            raise ValueError("lamb_pieces: a view outside every bucket")
        s = (v.data_ptr() - lo) // b.element_size()
        q = b.numel() // world
        a, e = max(s, rank * q), min(s + n, (rank + 1) * q)
        if a < e:
            out.append((t, j, a - rank * q, e - a))
    return out


class _ShardedLAMB(_ShardedAdam):
    """reduce-scatter(grads) -> moments on the own shard -> segmented norms of
    the (parameter, update) pieces -> all-gather of the sums -> trust ratios
    -> apply on the own pieces -> all-gather(params). The
    state is _ShardedAdam's; "u", the update direction, is one scratch shard
    per bucket in the compute type and is not checkpointed."""

    _kf_name = "ShardedLAMBOptimizer"
    _kf_dtypes = ("float32", "float64")
    _kf_dtype_words = "f32 and f64 (bf16 and f16 with master_weights=True)"
    _kf_trust_clip = 0.0
    _kf_always_adapt = False
    _kf_lamb = None  # the plans, one per (dtype, device)
    _kf_gate_words = "gate="

    def _kf_new_group(self):
        return dict(super()._kf_new_group(), u=None)

    def _kf_build_sharded(self):
        """Once, with the buckets: the state and update shards (fixed
        addresses), the piece list of every bucket group, and per (dtype,
        device) the norm plan over 2T segments, the tensor -> group table,
        the ratios' buffers and the apply plan."""
        import torch
        super()._kf_build_sharded()
        ex, ep = self._kf_ex, self._kf_ops("lamb_moments_")
        by = {}
        for j, G in enumerate(self._kf_groups):
            self._kf_states(G)
            G["u"] = self._kf_zero_shards(G, G["m"][0].dtype if G["m"] else None)
            b = G["pb"].buckets[0]
            by.setdefault((b.dtype, b.device), []).append(j)
        self._kf_lamb = []
        for (dtype, device), js in by.items():
            pp, uu, p16, tensors, group_of, owners = [], [], [], [], [], []
            for k, j in enumerate(js):
                G = self._kf_groups[j]
                pieces = {t: (b, off, n) for t, b, off, n in
                          lamb_pieces(G["pb"], ex.world, ex.rank)}
                for t, p in enumerate(G["ps"]):
                    b, off, n = pieces.get(t, (0, 0, 0))
                    bucket = G["pb"].buckets[b]
                    q = bucket.numel() // ex.world
                    mine = bucket[ex.rank * q:(ex.rank + 1) * q]
                    pp.append((G["w"][b] if G["w"] is not None else mine)[off:off + n])
                    uu.append(G["u"][b][off:off + n])
                    if G["w"] is not None:
                        p16.append(mine[off:off + n])
                    tensors.append(len(owners))
                    group_of.append(k)
                    owners.append(p)
            T = len(owners)
            f64 = dict(dtype=torch.float64, device=device)
            self._kf_lamb.append({
                "js": js, "owners": owners, "T": T,
                "norm": ep.sq_norm_plan(pp + uu),
                "out": torch.zeros(2 * T + 1, **f64),
                "sq": torch.zeros(2 * T * ex.world, **f64),
                "group_of": torch.tensor(group_of, dtype=torch.int32, device=device),
                "nlr": torch.zeros(T, **f64), "ratio": torch.ones(T, **f64),
                "apply": ep.lamb_apply_plan(pp, uu, tensors, T, p16 if p16 else None)})

    def step(self, closure=None):
        loss = self._kf_closure(closure)
        if self._kf_groups is None:
            self._kf_build_sharded()
        ex, ep, groups = self._kf_ex, self._kf_ops("lamb_moments_"), self._kf_groups
        for G in groups:
            _SyncSGD._kf_place(G["ps"], G["gb"])
        if self._kf_gated:
            self._kf_step_gated()
            _finish(ex)
            return loss
        for j, G in enumerate(groups):
            G["np"] = ex.reduce_shards_(G["gb"].buckets, ("lamb", j))
        for j, G in enumerate(groups):
            G["step"] += 1
            h = G["h"] = self._kf_hyper(G, step=G["step"])
            h["decoupled"] = False
            h["adapt"] = h["weight_decay"] != 0 or self._kf_always_adapt
            shards = ex.grad_shards_(G["gb"].buckets, ("lamb", j))
            hs = [G["h"]] * len(shards)
            if G["w"] is not None:
                ep.lamb_master_moments_(shards, G["w"], G["m"], G["v"], G["u"], hs, G["np"])
            else:
                ep.lamb_moments_(self._kf_mine(G), shards, G["m"], G["v"], G["u"], hs, G["np"])
        for L in self._kf_lamb:
            L["norm"].run("sq", out=L["out"])
            ex.gather_doubles_(L["out"][:2 * L["T"]], L["sq"])
            ep.lamb_trust_update_(L["sq"], ex.world, L["group_of"],
                                  [groups[j]["h"] for j in L["js"]], L["nlr"], L["ratio"],
                                  self._kf_trust_clip)
            L["apply"].run(L["nlr"])
        for G in groups:
            ex.gather_params_(G["pb"].buckets)
        _finish(ex)
        return loss

    def _kf_step_gated(self):
        """The step under a gate (include/kungfu_amd.h "LAMB under a gate",
        DESIGN.md §19): A to D are _ShardedAdam's with every group's lr = 1
        for the step states, E the gated moments, F the norms of (p, u), G the
        gated trust ratios and apply pass, H the parameters' all-gather.
        Queued; nothing waits for the verdict."""
        ex, ep, groups = self._kf_ex, self._kf_ops("lamb_moments_"), self._kf_groups
        gate, states = self._kf_gate, self._kf_gstates
        hs = self._kf_gate_verdict(gate_lr=1.0)
        for j, (G, h) in enumerate(zip(groups, hs)):
            wd = h["weight_decay"]
            G["h"] = dict(h, decoupled=False, adapt=wd != 0 or self._kf_always_adapt)
            shards = ex.grad_shards_(G["gb"].buckets, ("gated", j))
            if G["w"] is not None:
                ep.lamb_master_moments_gated_(shards, G["w"], G["m"], G["v"], G["u"], G["h"], gate,
                                              states, j, G["np"])
            else:
                ep.lamb_moments_gated_(self._kf_mine(G), shards, G["m"], G["v"], G["u"], G["h"],
                                       gate, states, j, G["np"])
        for L in self._kf_lamb:
            L["norm"].run("sq", out=L["out"])  # unconditional: read-only
            ex.gather_doubles_(L["out"][:2 * L["T"]], L["sq"])
            ep.lamb_trust_update_gated_(L["sq"], ex.world, L["group_of"],
                                        [groups[j]["h"] for j in L["js"]], L["nlr"], L["ratio"],
                                        gate, self._kf_trust_clip)
            L["apply"].run(L["nlr"], gate=gate)
        for G in groups:
            ex.gather_params_(G["pb"].buckets)

    def last_trust_ratios(self):
        """{parameter: the trust ratio its last step used} (1.0 before the
        first step; under a gate, the last applied step's); synchronises
        with the device."""
        out = {}
        for L in self._kf_lamb or []:
            for p, r in zip(L["owners"], L["ratio"].cpu().tolist()):
                out[p] = float(r)
        return out


def ShardedSGDOptimizer(optimizer, named_parameters=None, exchange=None, bucket_bytes=32 << 20):
    """Synchronous SGD with the optimizer update sharded over the ranks
    (sharded optimizer state): every step is

      reduce-scatter(grads) -> [own shard: g / np, weight decay, momentum,
                                p -= lr * g] -> all-gather(params)

    in one call of the exchange's `sgd_step_` per (param group, dtype): the
    same xGMI bytes as S-SGD's gradient all-reduce, the update over 1 / np
    of the model per rank in one batched HIP launch (ops.sgd_update_batch_),
    and a momentum buffer of 1 / np of the model per rank. The arithmetic is
    torch.optim.SGD's single-tensor path (foreach=False) on the averaged
    gradient, rounded as include/kungfu_amd.h kf_sgd_update_batch states.

    `optimizer` must be a torch.optim.SGD (TypeError otherwise); it only
    lends its class and its param_groups: its own step() is never called and
    `state` stays empty. lr, momentum, dampening, weight_decay and nesterov
    are read from param_groups at every step, so LR schedulers work.

    Two differences from torch.optim.SGD:
      * a parameter without a gradient is updated as with a zero gradient
        (weight decay and momentum still move it); torch skips it;
      * after step(), p.grad does not hold the averaged gradient: the
        gradient buckets are scratch of the exchange.

    momentum_buffers() (collective) and load_momentum_buffers(mapping) are
    the checkpoint path for the sharded momentum.

    Not offered: overlap=True, the hierarchical (multi-host) path, maximize,
    differentiable, and any optimizer other than SGD."""
    import torch
    if not isinstance(optimizer, torch.optim.SGD):
        raise TypeError("ShardedSGDOptimizer wraps a torch.optim.SGD, not %s"
                        % type(optimizer).__name__)
    for g in optimizer.param_groups:
        if g.get("maximize", False):
            raise ValueError("ShardedSGDOptimizer: maximize=True is not supported")
        if g.get("differentiable", False):
            raise ValueError("ShardedSGDOptimizer: differentiable=True is not supported")
    opt = _wrap(optimizer, _ShardedSGD)
    opt._kf_setup(named_parameters, exchange, bucket_bytes)
    if not hasattr(opt._kf_ex, "sgd_step_"):
        raise ValueError("ShardedSGDOptimizer needs an exchange with sgd_step_() "
                         "(collective.Exchange or exchange.NativeExchange)")
    return opt


def ShardedAdamOptimizer(optimizer, named_parameters=None, exchange=None, bucket_bytes=32 << 20,
                         master_weights=False, max_grad_norm=None, loss_scale=None,
                         stochastic_rounding=False, sr_seed=0, state_bits=32):
    """Synchronous Adam / AdamW with the optimizer update and its state
    sharded over the ranks, as ShardedSGDOptimizer does for SGD: every step is

      reduce-scatter(grads) -> [own shard: g / np, weight decay, exp_avg,
                                exp_avg_sq, p -= step_size * m / denom] -> all-gather(params)

    in one call of the exchange's `adam_step_` per (param group, dtype): the
    same xGMI bytes as S-SGD's gradient all-reduce, the update over 1 / np of
    the model per rank in one batched HIP launch (ops.adam_update_batch_),
    and exp_avg / exp_avg_sq of 1 / np of the model each per rank. The
    arithmetic source is torch.optim.Adam / AdamW's single-tensor path
    (foreach=False) on the averaged gradient, rounded as include/kungfu_amd.h
    kf_adam_update_batch states.

    `optimizer` must be a torch.optim.Adam or torch.optim.AdamW (TypeError
    otherwise); an AdamW decays the weights decoupled (p *= 1 - lr * wd), an
    Adam adds wd * p to the gradient. It only lends its class and its
    param_groups: its own step() is never called and `state` stays empty. lr,
    betas, eps and weight_decay are read from param_groups at every step, so
    LR schedulers work. Every (param group, dtype) bucket group counts its
    own steps from 1; the bias corrections 1 - beta ** step are taken in
    Python doubles.

    Differences from torch.optim.Adam / AdamW:
      * a parameter without a gradient is updated as with a zero gradient
        (its state decays, and AdamW's decay still applies); torch skips it;
      * after step(), p.grad does not hold the averaged gradient: the
        gradient buckets are scratch of the exchange;
      * exp_avg is b1*m + (1 - b1)*g, two products and a sum, not torch's
        lerp: the results differ from torch's in the last bits;
      * no f16 parameters (TypeError on the first step): eps = 1e-8 rounds
        to 0 in f16, so every element with exp_avg_sq == 0 would be 0 / 0.
        The state has the parameters' dtype (f32, bf16 or f64). Both hold
        without master_weights; see below.

    master_weights=True: every bf16 or f16 bucket group keeps
    an fp32 master copy of this rank's shard of the parameters and fp32
    exp_avg / exp_avg_sq shards, 12 / world bytes of state per element and
    rank. The master is taken from the parameters when the buckets are built
    (the widening is exact). The 16-bit parameters and gradients travel as
    before; the update (the exchange's `adam_master_step_`,
    ops.adam_master_update_batch_) widens the gradient, runs the f32
    arithmetic on the master and the state, and writes the parameters as the
    master narrowed, round-to-nearest-even: after every step() each 16-bit
    parameter equals the narrowing of its master on every rank, and no other
    rounding to 16 bits happens (kf_adam_master_update_batch). Updates below
    half a 16-bit ulp accumulate in the master instead of being rounded away.
    f16 parameters are accepted. Without the two keywords below there is
    no loss scaling, no inf / NaN step skipping and no gradient clipping: f16
    users must then keep their gradients finite themselves. f32 and f64
    groups take the path above and give the same bits as without the flag.
    state_buffers() carries the master as a third entry, "master".

    max_grad_norm / loss_scale: with either set, every step is
    gated by one verdict computed on the device over all bucket groups; with
    both None nothing changes. The step becomes: every group's reduce-scatter;
    one norm pass over this rank's shards (ops.SegNorm, fp64); an all-gather
    of 8 bytes per dtype and rank; the gate kernel (ops.step_gate_update_);
    every group's gated update (ops.adam_update_batch_gated_ /
    ops.adam_master_update_batch_gated_) and the parameters' all-gather. All
    of it is queued; the host never waits for the verdict.
      * max_grad_norm: a positive number. The gradients are multiplied by
        min(1, max_grad_norm / (norm + 1e-6)), torch's clip_grad_norm_, with
        the global norm of the unscaled, averaged gradient over all groups.
      * loss_scale: a number (static), "dynamic" (torch.amp.GradScaler's
        rule and defaults: 65536, x2 after 2000 good steps, x0.5 on a skip) or
        a dict overriding init_scale, growth_factor, backoff_factor,
        growth_interval. Train on scale_loss(loss).backward(): the update
        divides the gradients by the scale the loss was multiplied by.
      * A step whose gradients hold an inf or a NaN on any rank is skipped on
        every rank: parameters, masters and state keep their bits, the step
        count and the bias corrections do not advance, and a dynamic scale
        backs off. Clipping without a loss scale skips such steps too.
      * The bias corrections are running products in double kept on the
        device (the host does not know which steps were skipped), not
        1 - beta ** step; load_state_buffers seeds them with beta ** step.
      * loss_scale_value(), last_grad_norm(), skipped_steps(),
        applied_steps(), scaler_state() and state_buffers() read the device
        state and are the only calls that synchronise; load_scaler_state()
        restores the scale and its growth tracker.
    Gating takes every dtype the optimizer takes; f16 still needs
    master_weights=True (TypeError on the first step otherwise).

    stochastic_rounding=True, the alternative to
    master_weights for a bf16 model (both together: ValueError): every bf16
    bucket group keeps bf16 parameters and bf16 exp_avg / exp_avg_sq, 4 / world
    bytes of state per element and rank and 14 bytes of kernel traffic per
    element, as without the flag, but the update (ops.adam_sr_update_batch_)
    runs master_weights' f32 arithmetic in registers on the widened values and
    narrows the results itself. Round-to-nearest-even loses every update below
    half a bf16 ulp of the parameter, and at beta2 = 0.999 it leaves every
    normal exp_avg_sq where it is (b2 * v rounds back to v), so the second
    moment never decays; stochastic rounding removes both stalls in
    expectation.
      * What is stochastic: the narrowing of the new parameter and of the new
        exp_avg_sq, sr(x, r) = (bits(x) + r) >> 16 with 16 random bits each:
        up (away from zero) with probability low16(x) / 2^16, truncated
        otherwise, so the expectation is x; a value that is a bf16 already is
        kept for every r. What is not: the f32 arithmetic, exp_avg (narrowed
        round-to-nearest-even; it decays by 10 % a step and cannot stall), the
        gradient's reduce, and every f32 / f64 group, which takes the path
        above with the same bits as without the flag. f16 parameters remain a
        TypeError on the first step.
      * A finite value in bf16's top binade may round up to inf.
      * The random bits are Philox2x32-10 of (key, stream word, element
        index) and of nothing else: key = draw mod 2^32, where draw is the
        group's host-side count of step() calls from 1 (equal to `step`
        without a gate; under max_grad_norm / loss_scale it also advances on
        a step the device skips); the element index is the element's offset
        in its bucket; stream word = low32(splitmix64(splitmix64(sr_seed) ^
        (group_index << 32 | bucket_index))), group_index counting the
        (param group, dtype) bucket groups and bucket_index the group's
        buckets, splitmix64(x) being z = x + 0x9E3779B97F4A7C15; z = (z ^
        z >> 30) * 0xBF58476D1CE4E5B9; z = (z ^ z >> 27) *
        0x94D049BB133111EB; z ^ z >> 31 modulo 2^64. sr_seed is an int in
        [0, 2^64) (ValueError otherwise). Rank, world, shard boundaries and
        launch geometry play no part: given identical averaged gradients and
        the same sr_seed, the results are identical bit for bit for any world.
      * The step follows ShardedLAMBOptimizer's pattern: reduce_shards_,
        grad_shards_, the update on this rank's slice of the parameter
        buckets, gather_params_. Under a gate the group's last phase is
        ops.adam_sr_update_batch_gated_ and gather_params_.
      * state_buffers() adds "sr_draw" to every parameter's entry of such a
        group and load_state_buffers() restores it (absent: draw = step), so
        a resumed run draws the bits the uninterrupted run would have drawn.

    state_bits=8 (32, the default, is everything above): exp_avg
    and exp_avg_sq are kept as block-wise 8-bit codes (Dettmers et al., "8-bit
    Optimizers via Block-wise Quantization"): one uint8 code per element and
    state and one f32 scale per block of 64 consecutive bucket elements and
    state, 2.125 / world bytes per element and rank where f32 state takes 8,
    and 16.25 bytes of kernel traffic per element where the f32 update moves
    28. With master_weights=True a bf16 / f16 group keeps its fp32 master
    beside them: 6.125 / world bytes where it kept 12.
      * The update (ops.adam8_update_batch_ / ops.adam8_master_update_batch_,
        under max_grad_norm / loss_scale their _gated twins) dequantizes a
        block, runs the f32 arithmetic above on it bit for bit, takes the
        parameter from the unquantized new moments and quantizes them again;
        include/kungfu_amd.h states the format. The step follows
        stochastic_rounding's pattern: reduce_shards_, grad_shards_, the
        update on this rank's slices, gather_params_.
      * Shards are 256-byte aligned, so every shard boundary is a block
        boundary: parameters and state are identical bit for bit for any
        world, given identical averaged gradients.
      * Quality: a value is held to within 0.9/128 (exp_avg) or 0.9/256
        (exp_avg_sq) of its block's largest magnitude, and an exp_avg_sq below
        about 3e-7 of its block's largest becomes 0, where the update divides
        by eps alone. That is the format's known weakness; it is not
        bitsandbytes' table and makes no claim to match its results.
      * f32 groups take the f32 kernel; bf16 and f16 groups need
        master_weights=True; f64 groups, stochastic_rounding=True and any
        state_bits other than 8 and 32 are refused (ValueError).
      * state_buffers() returns the dequantized f32 exp_avg / exp_avg_sq per
        parameter (and "master", "step"), a form that depends on neither world
        nor layout; load_state_buffers() quantizes them again. Quantizing a
        dequantized block gives the same codes and scale, so save -> load ->
        continue is bit-identical to the uninterrupted run, also when the
        world changes, as long as the buckets' layout (bucket_bytes, the
        parameters' order) stays. A block whose scale is so small that
        table value * scale is subnormal is outside that guarantee.

    state_buffers() (collective) and load_state_buffers(mapping) are the
    checkpoint path for the sharded state.

    Not offered: overlap=True, the hierarchical (multi-host) path, amsgrad,
    maximize, differentiable, and any optimizer other than Adam / AdamW."""
    import torch
    if isinstance(optimizer, torch.optim.AdamW):  # first: newer torch derives it from Adam
        decoupled = True
    elif isinstance(optimizer, torch.optim.Adam):
        decoupled = False
    else:
        raise TypeError("ShardedAdamOptimizer wraps a torch.optim.Adam or AdamW, not %s"
                        % type(optimizer).__name__)
    for g in optimizer.param_groups:
        for option in ("amsgrad", "maximize", "differentiable"):
            if g.get(option, False):
                raise ValueError("ShardedAdamOptimizer: %s=True is not supported" % option)
    opt = _wrap(optimizer, _ShardedAdam)
    opt._kf_decoupled = decoupled
    opt._kf_setup(named_parameters, exchange, bucket_bytes)
    if not hasattr(opt._kf_ex, "adam_step_"):
        raise ValueError("ShardedAdamOptimizer needs an exchange with adam_step_() "
                         "(collective.Exchange or exchange.NativeExchange)")
    if master_weights:
        if not hasattr(opt._kf_ex, "adam_master_step_"):
            raise ValueError("ShardedAdamOptimizer(master_weights=True) needs an exchange with "
                             "adam_master_step_() (collective.Exchange or exchange.NativeExchange)")
        opt._kf_master = True
        opt._kf_dtypes = ("float32", "float16", "bfloat16", "float64")
        opt._kf_dtype_words = "f32, f16, bf16 and f64"
    if max_grad_norm is not None or loss_scale is not None:
        opt._kf_max_norm, opt._kf_rule = _gate_rule(max_grad_norm, loss_scale)
        for method in ("reduce_shards_", "gather_doubles_", "adam_gated_step_"):
            if not hasattr(opt._kf_ex, method):
                raise ValueError("ShardedAdamOptimizer(max_grad_norm / loss_scale) needs an "
                                 "exchange with %s() (collective.Exchange or "
                                 "exchange.NativeExchange)" % method)
        opt._kf_gated = True
    if isinstance(sr_seed, bool) or not isinstance(sr_seed, int) or not 0 <= sr_seed < 1 << 64:
        raise ValueError("ShardedAdamOptimizer: sr_seed must be an int in [0, 2**64), not %r"
                         % (sr_seed,))
    if stochastic_rounding:
        if master_weights:
            raise ValueError("ShardedAdamOptimizer: stochastic_rounding and master_weights are "
                             "alternatives, not both")
        for method in ("reduce_shards_", "grad_shards_", "gather_params_"):
            if not hasattr(opt._kf_ex, method):
                raise ValueError("ShardedAdamOptimizer(stochastic_rounding=True) needs an "
                                 "exchange with %s() (collective.Exchange or "
                                 "exchange.NativeExchange)" % method)
        opt._kf_sr, opt._kf_sr_seed = True, sr_seed
    if isinstance(state_bits, bool) or state_bits not in (8, 32):
        raise ValueError("ShardedAdamOptimizer: state_bits must be 8 or 32, not %r"
                         % (state_bits,))
    if state_bits == 8:
        if stochastic_rounding:
            raise ValueError("ShardedAdamOptimizer: state_bits=8 and stochastic_rounding=True "
                             "do not combine")
        for p in opt._kf_params:
            if p.dtype == torch.float64:
                raise ValueError("ShardedAdamOptimizer: state_bits=8 takes no f64 parameters")
            if p.dtype in (torch.bfloat16, torch.float16) and not master_weights:
                raise ValueError("ShardedAdamOptimizer: state_bits=8 needs master_weights=True "
                                 "for %s parameters" % str(p.dtype).replace("torch.", ""))
        for method in ("reduce_shards_", "grad_shards_", "gather_params_"):
            if not hasattr(opt._kf_ex, method):
                raise ValueError("ShardedAdamOptimizer(state_bits=8) needs an exchange with "
                                 "%s() (collective.Exchange or exchange.NativeExchange)" % method)
        opt._kf_state_bits = 8
    return opt


# torch.amp.GradScaler's defaults
_DYNAMIC_SCALE = {"init_scale": 65536.0, "growth_factor": 2.0, "backoff_factor": 0.5,
                  "growth_interval": 2000}


def _gate_rule(max_grad_norm, loss_scale, name="ShardedAdamOptimizer"):
    """(max_norm, rule) of a gated optimizer `name` from the two settings
    (ShardedAdamOptimizer's keywords, ShardedLAMBOptimizer's gate= entries),
    ValueError for anything else."""
    import math
    max_norm = 0.0
    if max_grad_norm is not None:
        if isinstance(max_grad_norm, bool) or not isinstance(max_grad_norm, (int, float)) or \
                not (0 < max_grad_norm < math.inf):
            raise ValueError(name + ": max_grad_norm must be a positive finite "
                             "number or None, not %r" % (max_grad_norm,))
        max_norm = float(max_grad_norm)
    static = {"init_scale": 1.0, "growth_factor": 1.0, "backoff_factor": 1.0, "growth_interval": 0}
    if loss_scale is None:
        return max_norm, static
    if isinstance(loss_scale, str):
        if loss_scale != "dynamic":
            raise ValueError(name + ": loss_scale must be None, a positive number, "
                             "'dynamic' or a dict, not %r" % (loss_scale,))
        return max_norm, dict(_DYNAMIC_SCALE)
    if isinstance(loss_scale, dict):
        unknown = set(loss_scale) - set(_DYNAMIC_SCALE)
        if unknown:
            raise ValueError(name + ": loss_scale has unknown keys %s (known: %s)"
                             % (sorted(unknown), sorted(_DYNAMIC_SCALE)))
        rule = dict(_DYNAMIC_SCALE, **loss_scale)
        for k in ("init_scale", "growth_factor", "backoff_factor"):
            v = rule[k]
            if isinstance(v, bool) or not isinstance(v, (int, float)) or not (0 < v < math.inf):
                raise ValueError(name + ": loss_scale[%r] must be a positive finite "
                                 "number, not %r" % (k, v))
            rule[k] = float(v)
        n = rule["growth_interval"]
        if isinstance(n, bool) or not isinstance(n, int) or n < 0:
            raise ValueError(name + ": loss_scale['growth_interval'] must be an "
                             "integer >= 0, not %r" % (n,))
        return max_norm, rule
    if isinstance(loss_scale, bool) or not isinstance(loss_scale, (int, float)) or \
            not (0 < loss_scale < math.inf):
        raise ValueError(name + ": loss_scale must be None, a positive number, "
                         "'dynamic' or a dict, not %r" % (loss_scale,))
    return max_norm, dict(static, init_scale=float(loss_scale))


def ShardedLAMBOptimizer(optimizer, named_parameters=None, exchange=None, bucket_bytes=32 << 20,
                         master_weights=False, trust_clip=None, always_adapt=False, gate=None,
                         **unsupported):
    """LAMB (layer-wise adaptive moments for large batches) with the update
    and its state sharded over the ranks as ShardedAdamOptimizer's are
    (DESIGN.md §17). Every step is

      reduce-scatter(grads) -> [own shard: g / np, exp_avg, exp_avg_sq,
                                u = m^ / (sqrt(v^) + eps) + weight_decay * p]
        -> norms of every tensor's piece of p and of u on this rank (one
           ops.SegNorm pass, fp64) -> all-gather of 16 bytes per tensor and rank
        -> trust ratio per tensor, ||p|| / ||u|| (ops.lamb_trust_update_)
        -> [own pieces: p -= lr * ratio * u] -> all-gather(params)

    all queued on the current stream: the host never waits for a norm. A
    tensor's norms are taken over the whole tensor although its elements are
    spread over the ranks' shards at element offsets; the sums are added in
    rank order, so every rank computes the same ratios bit for bit. The
    arithmetic is include/kungfu_amd.h's ("LAMB"): apex FusedLAMB's
    formulation with bias correction, without its global gradient clipping
    unless gate= asks for it.

    `optimizer` must be a torch.optim.Adam or torch.optim.AdamW (TypeError
    otherwise); it only lends its class and its param_groups (lr, betas, eps,
    weight_decay, read at every step, so LR schedulers work). weight_decay is
    LAMB's lambda for both classes: wd * p joins the update before the norm.
    A parameter group adapts (uses the trust ratio) when its weight_decay != 0
    or always_adapt=True, apex's rule; otherwise its ratio is 1. A tensor
    whose parameter norm or update norm is not > 0 (a zero-element tensor
    among them) has ratio 1.

      * trust_clip: None, or a positive number the ratio is clipped to from
        above (1.0 gives "LAMBC"-style clipping).
      * master_weights=True: bf16 and f16 groups keep fp32 master weights
        and fp32 state, as ShardedAdamOptimizer(master_weights=True) does;
        both passes run in fp32 on the master and the 16-bit parameters are
        the master narrowed. Without it bf16 and f16 parameters are refused
        (TypeError on the first step): f32 and f64 only.
      * Non-finite gradients are not skipped: they reach the parameters as
        they do in torch.optim.Adam. That is the behaviour without a gate.
      * gate: None, or a dict with the keys "max_grad_norm" and / or
        "loss_scale", whose values are what ShardedAdamOptimizer's keywords
        of those names take (FusedLAMB's default is {"max_grad_norm": 1.0}; an
        f16 model wants "loss_scale": "dynamic" too). The step then runs under
        ShardedAdamOptimizer's device-side gate: one verdict
        per step from the global norm of the averaged gradient, which the
        moments pass multiplies the gradient by (clipping and unscaling), and
        a step whose gradients are not finite is skipped: parameters, master,
        exp_avg, exp_avg_sq, the trust ratios and the step count stay as they
        were, and a dynamic loss scale backs off. The host never waits for the
        verdict. scale_loss(), loss_scale_value(), last_grad_norm(),
        skipped_steps(), applied_steps(), scaler_state() and
        load_scaler_state() are ShardedAdamOptimizer's; without a gate they
        raise ValueError. The bias corrections are then the device's running
        products, and state_buffers() reports the device's step count. An
        empty dict, an unknown key or anything that is not a dict is a
        ValueError. All parameters must be on one device.
      * A parameter without a gradient is updated as with a zero gradient,
        and p.grad does not hold the averaged gradient after step().

    state_buffers() / load_state_buffers() are ShardedAdamOptimizer's
    checkpoint path (step, exp_avg, exp_avg_sq, master); the update direction
    is scratch and is not part of it. last_trust_ratios() returns {parameter:
    float} of the last step and synchronises.

    Not offered: max_grad_norm= / loss_scale= as keywords (they are gate='s
    entries), overlap=True, the hierarchical (multi-host) path, amsgrad,
    maximize, capturable, differentiable, and any optimizer other than Adam /
    AdamW."""
    import math
    import torch
    for k in unsupported:
        if k == "state_bits":
            if unsupported[k] == 32 and not isinstance(unsupported[k], bool):
                continue
            raise ValueError("ShardedLAMBOptimizer: state_bits=%r is not supported (8-bit state "
                             "is ShardedAdamOptimizer's)" % (unsupported[k],))
        if k in ("max_grad_norm", "loss_scale"):
            raise ValueError("ShardedLAMBOptimizer: %s is not a keyword here; the gated step "
                             "is gate={%r: ...}" % (k, k))
        raise TypeError("ShardedLAMBOptimizer got an unexpected keyword argument %r" % k)
    if not isinstance(optimizer, (torch.optim.Adam, torch.optim.AdamW)):
        raise TypeError("ShardedLAMBOptimizer wraps a torch.optim.Adam or AdamW, not %s"
                        % type(optimizer).__name__)
    for g in optimizer.param_groups:
        for option in ("amsgrad", "maximize", "capturable", "differentiable"):
            if g.get(option, False):
                raise ValueError("ShardedLAMBOptimizer: %s=True is not supported" % option)
    if trust_clip is not None and (isinstance(trust_clip, bool) or
                                   not isinstance(trust_clip, (int, float)) or
                                   not (0 < trust_clip < math.inf)):
        raise ValueError("ShardedLAMBOptimizer: trust_clip must be a positive finite number or "
                         "None, not %r" % (trust_clip,))
    opt = _wrap(optimizer, _ShardedLAMB)
    opt._kf_setup(named_parameters, exchange, bucket_bytes)
    for method in ("reduce_shards_", "grad_shards_", "gather_doubles_", "gather_params_"):
        if not hasattr(opt._kf_ex, method):
            raise ValueError("ShardedLAMBOptimizer needs an exchange with %s() "
                             "(collective.Exchange or exchange.NativeExchange)" % method)
    opt._kf_trust_clip = float(trust_clip) if trust_clip is not None else 0.0
    opt._kf_always_adapt = bool(always_adapt)
    if master_weights:
        opt._kf_master = True
        opt._kf_dtypes = ("float32", "float16", "bfloat16", "float64")
        opt._kf_dtype_words = "f32, f16, bf16 and f64"
    if gate is not None:
        known = ("max_grad_norm", "loss_scale")
        if not isinstance(gate, dict) or not gate or set(gate) - set(known) or \
                all(v is None for v in gate.values()):
            raise ValueError("ShardedLAMBOptimizer: gate must be None or a dict with the keys "
                             "'max_grad_norm' and / or 'loss_scale', not %r" % (gate,))
        opt._kf_max_norm, opt._kf_rule = _gate_rule(gate.get("max_grad_norm"),
                                                    gate.get("loss_scale"), opt._kf_name)
        opt._kf_gated = True
    return opt
