"""The stochastic-rounding Adam kernels in the built library (no GPU needed),
read from the code objects' metadata notes as tests/test_sharded_lamb_isa.py
does: both kernels of kf_adam_sr.hip exist for bf16 alone and touch no
scratch."""
import re

import pytest

from test_sharded_lamb_isa import kernel_meta  # noqa: F401  (the fixture)

BF16_ONLY = {"NS_6bf16_tE"}
TEMPLATES = ("adam_sr_kernel", "adam_sr_gated_kernel")
NARROW = re.compile(r"^_ZN2kf\d+adam_sr_narrow_kernelE")


def _template(name):
    return re.compile(r"^_ZN2kf\d+%sI(\w+?)EEv" % name)


def _sr_kernels(meta):
    out = {k: v for k, v in meta.items() if NARROW.match(k)}
    for name in TEMPLATES:
        out.update({k: v for k, v in meta.items() if _template(name).match(k)})
    return out


@pytest.mark.parametrize("name", TEMPLATES)
def test_sr_kernels_exist_for_bf16_only(kernel_meta, name):  # noqa: F811
    rx = _template(name)
    found = {rx.match(k).group(1) for k in kernel_meta if rx.match(k)}
    assert found == BF16_ONLY, (name, found)


def test_sr_kernels_use_no_scratch(kernel_meta):  # noqa: F811
    ks = _sr_kernels(kernel_meta)
    assert len(ks) == 3, sorted(ks)
    for k, v in ks.items():
        assert "private_segment_fixed_size" in v and "vgpr_spill_count" in v, (k, v)
    bad = [(k, v) for k, v in ks.items()
           if v["private_segment_fixed_size"] != 0 or v["vgpr_spill_count"] != 0]
    assert not bad, bad
    print({k: v.get("vgpr_count") for k, v in ks.items()})
