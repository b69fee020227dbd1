"""The monitoring optimizers' host side (no GPU): constructor validation, the
argument errors of kf_segnorm_create that touch no device, and the numpy
yardstick (monitor_ref) pinned against hand-computed steps."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import monitor_ref

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
LIB = os.path.join(ROOT, "kungfu_amd", "libkungfu_amd.so")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "kungfu_amd", "csrc")],
                       check=True)
    from kungfu_amd import _lib
    return _lib.load()


def _sgd():
    p = torch.nn.Parameter(torch.zeros(4))
    return torch.optim.SGD([p], lr=0.1)


@pytest.mark.parametrize("bad", [0, -1, -0.5])
def test_noise_scale_rejects_device_batch_size(bad):
    from kungfu_amd.optimizers import MonitorGradientNoiseScaleOptimizer
    with pytest.raises(ValueError, match="device_batch_size"):
        MonitorGradientNoiseScaleOptimizer(_sgd(), bad)


@pytest.mark.parametrize("bad", [0, -0.1])
def test_noise_scale_rejects_alpha(bad):
    from kungfu_amd.optimizers import MonitorGradientNoiseScaleOptimizer
    with pytest.raises(ValueError, match="alpha"):
        MonitorGradientNoiseScaleOptimizer(_sgd(), 32, alpha=bad)


def test_monitors_reject_overlap_and_interval():
    from kungfu_amd.optimizers import (MonitorGradientNoiseScaleOptimizer,
                                       MonitorGradientVarianceOptimizer)
    with pytest.raises(ValueError, match="overlap"):
        MonitorGradientNoiseScaleOptimizer(_sgd(), 32, overlap=True)
    with pytest.raises(ValueError, match="overlap"):
        MonitorGradientVarianceOptimizer(_sgd(), overlap=True)
    with pytest.raises(ValueError, match="monitor_interval"):
        MonitorGradientVarianceOptimizer(_sgd(), monitor_interval=0)


def test_monitors_construct_and_export():
    """Both wrap the user's optimizer class like the S-SGD wrapper, start
    their step counter at 0, and are exported with named_parameters
    positional from kungfu_amd.torch.optimizers."""
    from kungfu_amd.torch import optimizers as topt
    assert {"MonitorGradientNoiseScaleOptimizer",
            "MonitorGradientVarianceOptimizer"} <= set(topt.__all__)
    p = torch.nn.Parameter(torch.zeros(4))
    ns = topt.MonitorGradientNoiseScaleOptimizer(torch.optim.SGD([p], lr=0.1), [("p", p)], 32,
                                                 monitor_interval=2)
    gv = topt.MonitorGradientVarianceOptimizer(torch.optim.SGD([p], lr=0.1), [("p", p)])
    for o in (ns, gv):
        assert isinstance(o, torch.optim.SGD)
        assert o._kf_step == 0 and o._kf_op == "sum" and o._kf_average
    assert ns._kf_interval == 2 and gv._kf_interval == 1
    assert ns.noise_scale.dtype == torch.float32 and ns.noise_scale.dim() == 0
    assert ns.last_sq_small.dtype == torch.float64 and ns.last_sq_big.dim() == 0
    assert gv.variance.dtype == torch.float64 and gv.variance.dim() == 0
    assert gv.last_variances.shape == (1,)


def _err(lib):
    return lib.kf_last_error().decode()


def test_segnorm_create_arg_errors(lib):
    """Argument checks come before any HIP call (no device here)."""
    from kungfu_amd import _lib
    cnt = (ctypes.c_size_t * 2)(16, 16)
    arr = _lib.ptr_array([8, 8])
    # null tables with nseg > 0
    assert lib.kf_segnorm_create(None, None, cnt, 2, 0x20408) is None
    assert _err(lib).startswith("KF_ERR_ARG")
    assert lib.kf_segnorm_create(arr, None, None, 2, 0x20408) is None
    assert _err(lib).startswith("KF_ERR_ARG")
    # nseg <= 0
    for nseg in (0, -3):
        assert lib.kf_segnorm_create(arr, None, cnt, nseg, 0x20408) is None
        assert _err(lib).startswith("KF_ERR_ARG")
    # integers, BOOL and unknown codes have no norm
    for code in (0x10408, 0x00108, 0x30108, 0x12345):
        assert lib.kf_segnorm_create(arr, None, cnt, 2, code) is None
        assert _err(lib).startswith("KF_ERR_DTYPE"), code
    # a null pointer in a non-empty segment; a pointer off the element size
    assert lib.kf_segnorm_create(_lib.ptr_array([8, 0]), None, cnt, 2, 0x20408) is None
    assert _err(lib).startswith("KF_ERR_ARG")
    assert lib.kf_segnorm_create(arr, _lib.ptr_array([8, 0]), cnt, 2, 0x20408) is None
    assert _err(lib).startswith("KF_ERR_ARG")
    assert lib.kf_segnorm_create(_lib.ptr_array([8, 10]), None, cnt, 2, 0x20408) is None
    assert _err(lib).startswith("KF_ERR_ARG")
    # run / update / destroy on nothing
    assert lib.kf_segnorm_run(None, 0, 8, None) == 3
    lib.kf_segnorm_destroy(None)
    assert lib.kf_noise_scale_update(None, 8, 32.0, 64.0, 0.9, 8, None) == 3
    assert lib.kf_noise_scale_update(8, 8, 32.0, 64.0, 0.0, 8, None) == 3  # collective.cpp:283
    assert lib.kf_noise_scale_update(8, 8, 32.0, 64.0, -1.0, 8, None) == 3
    assert "alpha" in _err(lib)


def test_ref_noise_scale_chain_by_hand():
    """Three updates whose every fp32 operation is exact, worked by hand:
    bs = 32, bb = 64, alpha = 0.5.
      (3, 2):   G = (1/32)(128 - 96) = 1, S = 64 (3 - 2) = 64     -> 1, 64, 64
      (5, 3):   G = (1/32)(192 - 160) = 1, S = 64 * 2 = 128        -> 1, 96, 96
      (4, 3.5): G = (1/32)(224 - 128) = 3, S = 64 * 0.5 = 32       -> 2, 64, 32"""
    st = np.zeros(4, np.float32)
    want = [(1.0, 64.0, 64.0), (1.0, 96.0, 96.0), (2.0, 64.0, 32.0)]
    for (small, big), w in zip([(3.0, 2.0), (5.0, 3.0), (4.0, 3.5)], want):
        st = monitor_ref.noise_scale_step(st, small, big, 32, 64, 0.5)
        assert st.dtype == np.float32
        assert tuple(st) == w + (1.0,)
    # world 1: bb == bs divides by zero, as the reference (not an error)
    with np.errstate(all="ignore"):
        st = monitor_ref.noise_scale_step(np.zeros(4, np.float32), 3.0, 2.0, 32, 32, 0.5)
    assert not np.isfinite(st[:3]).all() and st[3] == 1.0


def test_ref_sums_and_var_terms():
    assert monitor_ref.exact_sq(np.array([3e38] * 4, np.float32), "f32") == \
        4 * float(np.float32(3e38)) ** 2
    assert monitor_ref.exact_sq(np.zeros(0, np.float32), "f32") == 0.0
    assert np.isnan(monitor_ref.exact_sq(np.array([1, np.nan], np.float32), "f32"))
    assert monitor_ref.exact_sq(np.array([1, np.inf], np.float32), "f32") == float("inf")
    # fp32: 1 + 2^-23 squared rounds to 1 + 2^-22; a - that is exact
    b = np.array([1 + 2.0 ** -23], np.float32)
    a = np.array([2.0], np.float32)
    d = monitor_ref.var_terms(a, b, "f32")
    assert d.dtype == np.float32 and float(d[0]) == 2.0 - (1 + 2.0 ** -22)
    # bf16: 1.0078125 (1 + 2^-7) squared = 1.0156860..., rounds to 1.015625
    from oracle.oracle import bf16_bits_to_f32, f32_to_bf16_bits
    bb = f32_to_bf16_bits(np.array([1.0078125], np.float32))
    ab = f32_to_bf16_bits(np.array([3.0], np.float32))
    db = monitor_ref.var_terms(ab, bb, "bf16")
    assert db.dtype == np.uint16 and float(bf16_bits_to_f32(db)[0]) == 1.984375
    # f16: 1 + 2^-10 squared rounds to 1 + 2^-9
    d16 = monitor_ref.var_terms(np.array([2.0], np.float16), np.array([1 + 2.0 ** -10], np.float16),
                                "f16")
    assert d16.dtype == np.float16 and float(d16[0]) == 2.0 - (1 + 2.0 ** -9)
    assert monitor_ref.left_sum([1.0, 2.0 ** -53, 2.0 ** -53]) == 1.0
