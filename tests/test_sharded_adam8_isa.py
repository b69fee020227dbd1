"""The 8-bit Adam kernels in the built library (no GPU needed), read from the
code objects' metadata notes as tests/test_sharded_adam_sr_isa.py does: the
kernels of kf_adam8.hip exist for exactly their types and touch no scratch."""
import re

import pytest

from test_sharded_lamb_isa import kernel_meta  # noqa: F401  (the fixture)

TYPES = {"f", "NS_6bf16_tE", "NS_5f16_tE"}
TEMPLATES = ("adam8_kernel", "adam8_gated_kernel")
CODEC = re.compile(r"^_ZN2kf\d+adam8_(de)?quantize_kernelE")


def _template(name):
    return re.compile(r"^_ZN2kf\d+%sI(\w+?)EEv" % name)


def _adam8_kernels(meta):
    out = {k: v for k, v in meta.items() if CODEC.match(k)}
    for name in TEMPLATES:
        out.update({k: v for k, v in meta.items() if _template(name).match(k)})
    return out


@pytest.mark.parametrize("name", TEMPLATES)
def test_adam8_kernels_exist_for_exactly_their_types(kernel_meta, name):  # noqa: F811
    rx = _template(name)
    found = {rx.match(k).group(1) for k in kernel_meta if rx.match(k)}
    assert found == TYPES, (name, found)


def test_adam8_kernels_use_no_scratch(kernel_meta):  # noqa: F811
    ks = _adam8_kernels(kernel_meta)
    assert len(ks) == 8, sorted(ks)
    for k, v in ks.items():
        assert "private_segment_fixed_size" in v and "vgpr_spill_count" in v, (k, v)
    bad = [(k, v) for k, v in ks.items()
           if v["private_segment_fixed_size"] != 0 or v["vgpr_spill_count"] != 0]
    assert not bad, bad
    print({k: v.get("vgpr_count") for k, v in ks.items()})
