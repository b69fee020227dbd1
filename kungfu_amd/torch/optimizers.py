"""``kungfu.torch.optimizers`` mirror.

``SynchronousSGDOptimizer(optimizer, named_parameters, op=None)`` keeps the
reference torch wrapper's signature AND arithmetic
(srcs/python/kungfu/torch/optimizers/sync_sgd.py:12-34): ``named_parameters``
is required, and every gradient is all-reduced with ``op`` (default 'sum')
and NOT divided by np — unlike the TF S-SGD (tensorflow/optimizers/
sync_sgd.py:103-104), whose averaging variant is
``kungfu_amd.optimizers.SynchronousSGDOptimizer`` (average=True). Extra
keyword arguments (``overlap``, ``exchange``, ``bucket_bytes``, ``average``)
pass through to it.

``SynchronousAveragingOptimizer`` is the SMA wrapper (sma_sgd.py:9-74); the
reference has no torch version, so it is the package's own.

``MonitorGradientNoiseScaleOptimizer`` and ``MonitorGradientVarianceOptimizer``
(grad_noise_scale.py, grad_variance.py; TF only in the reference) take
``named_parameters`` positionally like the S-SGD wrapper; they average
(sum, / np) as their TF originals do.

``PairAveragingOptimizer`` (async_sgd.py; TF only in the reference) likewise
takes ``named_parameters`` positionally.

``ShardedSGDOptimizer`` (the package's own: S-SGD with the SGD update and its
momentum sharded over the ranks) likewise takes ``named_parameters``
positionally, and so does ``ShardedAdamOptimizer`` (the same for
torch.optim.Adam / AdamW and their two state tensors) and
``ShardedLAMBOptimizer`` (LAMB's layer-wise trust ratios on the same shards).
"""
from .. import optimizers as _opt
from ..optimizers import SynchronousAveragingOptimizer

__all__ = ["SynchronousSGDOptimizer", "SynchronousAveragingOptimizer",
           "MonitorGradientNoiseScaleOptimizer", "MonitorGradientVarianceOptimizer",
           "PairAveragingOptimizer", "ShardedSGDOptimizer", "ShardedAdamOptimizer",
           "ShardedLAMBOptimizer"]


def SynchronousSGDOptimizer(optimizer, named_parameters, op=None, **kwargs):
    """Reference torch S-SGD (sync_sgd.py:31-34): sum (or `op`) of every
    gradient across peers before the wrapped optimizer's step; no /np."""
    kwargs.setdefault("average", False)
    return _opt.SynchronousSGDOptimizer(optimizer, named_parameters=named_parameters, op=op,
                                        **kwargs)


def MonitorGradientNoiseScaleOptimizer(optimizer, named_parameters, device_batch_size,
                                       monitor_interval=1, alpha=0.9, **kwargs):
    """kungfu_amd.optimizers.MonitorGradientNoiseScaleOptimizer with
    `named_parameters` positional."""
    return _opt.MonitorGradientNoiseScaleOptimizer(
        optimizer, device_batch_size, monitor_interval=monitor_interval,
        named_parameters=named_parameters, alpha=alpha, **kwargs)


def MonitorGradientVarianceOptimizer(optimizer, named_parameters, monitor_interval=1, **kwargs):
    """kungfu_amd.optimizers.MonitorGradientVarianceOptimizer with
    `named_parameters` positional."""
    return _opt.MonitorGradientVarianceOptimizer(
        optimizer, monitor_interval=monitor_interval, named_parameters=named_parameters,
        **kwargs)


def PairAveragingOptimizer(optimizer, named_parameters, **kwargs):
    """kungfu_amd.optimizers.PairAveragingOptimizer with `named_parameters`
    positional."""
    return _opt.PairAveragingOptimizer(optimizer, named_parameters=named_parameters, **kwargs)


def ShardedSGDOptimizer(optimizer, named_parameters, **kwargs):
    """kungfu_amd.optimizers.ShardedSGDOptimizer with `named_parameters`
    positional."""
    return _opt.ShardedSGDOptimizer(optimizer, named_parameters=named_parameters, **kwargs)


def ShardedAdamOptimizer(optimizer, named_parameters, **kwargs):
    """kungfu_amd.optimizers.ShardedAdamOptimizer with `named_parameters`
    positional. Keywords pass through: `exchange`, `bucket_bytes`, and
    `master_weights=True` for fp32 master weights and fp32 state on the shard
    of bf16 / f16 parameters, and `max_grad_norm` / `loss_scale` for the gated
    step (gradient-norm clipping, loss scaling, inf / NaN step skipping)."""
    return _opt.ShardedAdamOptimizer(optimizer, named_parameters=named_parameters, **kwargs)


def ShardedLAMBOptimizer(optimizer, named_parameters, **kwargs):
    """kungfu_amd.optimizers.ShardedLAMBOptimizer with `named_parameters`
    positional. Keywords pass through: `exchange`, `bucket_bytes`,
    `master_weights`, `trust_clip`, `always_adapt` and `gate` (a dict with
    `max_grad_norm` and / or `loss_scale`: the step under the device-side gate)."""
    return _opt.ShardedLAMBOptimizer(optimizer, named_parameters=named_parameters, **kwargs)
