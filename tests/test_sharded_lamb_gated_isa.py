"""The gated LAMB kernels in the built library (no GPU needed),
read from the code objects' metadata notes with tests/test_sharded_lamb_isa.py's
reader: the five new kernel families of kf_lamb.hip exist for exactly their
dtypes, beside the nine parents, and touch no scratch. No instruction text is
looked at."""
import re

import pytest

import test_sharded_lamb_isa as base
from test_sharded_lamb_isa import kernel_meta  # noqa: F401  (the module-scoped fixture)

TEMPLATES = {"lamb_moments_gated_kernel": base.F32_F64,
             "lamb_master_moments_gated_kernel": base.SIXTEEN,
             "lamb_apply_gated_kernel": base.F32_F64,
             "lamb_master_apply_gated_kernel": base.SIXTEEN}
TRUST = re.compile(r"^_ZN2kf\d+lamb_trust_gated_kernelE")


def _gated_kernels(meta):
    out = {k: v for k, v in meta.items() if TRUST.match(k)}
    for name in TEMPLATES:
        out.update({k: v for k, v in meta.items() if base._template(name).match(k)})
    return out


@pytest.mark.parametrize("name", sorted(TEMPLATES))
def test_gated_kernels_exist_for_exactly_their_dtypes(kernel_meta, name):  # noqa: F811
    rx = base._template(name)
    found = {rx.match(k).group(1) for k in kernel_meta if rx.match(k)}
    assert found == TEMPLATES[name], (name, found)


def test_gated_trust_kernel_exists_once(kernel_meta):  # noqa: F811
    assert len([k for k in kernel_meta if TRUST.match(k)]) == 1


def test_gated_kernels_use_no_scratch_and_parents_are_all_there(kernel_meta):  # noqa: F811
    ks = _gated_kernels(kernel_meta)
    assert len(ks) == 9, sorted(ks)
    assert len(base._lamb_kernels(kernel_meta)) == 9  # the parents, under their own names
    assert not set(ks) & set(base._lamb_kernels(kernel_meta))
    for k, v in ks.items():
        assert "private_segment_fixed_size" in v and "vgpr_spill_count" in v, (k, v)
    bad = [(k, v) for k, v in ks.items()
           if v["private_segment_fixed_size"] != 0 or v["vgpr_spill_count"] != 0]
    assert not bad, bad
    print({k: v.get("vgpr_count") for k, v in ks.items()})
    print({k: v.get("vgpr_count") for k, v in base._lamb_kernels(kernel_meta).items()})
