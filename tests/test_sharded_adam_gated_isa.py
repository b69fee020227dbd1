"""The gated Adam update kernels in the built library (no GPU needed), read
from the code objects' metadata notes as tests/test_sharded_adam_master_isa.py
reads them: kf::adam_update_gated_kernel exists for exactly f32, f64 and bf16,
kf::adam_master_gated_kernel for exactly bf16 and f16, and none touches
scratch."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
LIB = os.path.join(ROOT, "kungfu_amd", "libkungfu_amd.so")
OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"
READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"

# <kernel><T>: any T, so that another dtype would be seen
PLAIN = re.compile(r"^_ZN2kf24adam_update_gated_kernelI(\w+?)EEv")
MASTER = re.compile(r"^_ZN2kf24adam_master_gated_kernelI(\w+?)EEv")


@pytest.fixture(scope="module")
def kernel_meta(tmp_path_factory):
    if not (os.path.exists(OBJDUMP) and os.path.exists(READELF)):
        pytest.skip("llvm tools not found")
    if not os.path.exists(LIB):
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "kungfu_amd", "csrc")],
                       check=True)
    d = tmp_path_factory.mktemp("adam_gated_isa")
    lib = d / "lib.so"
    shutil.copy(LIB, lib)
    subprocess.run([OBJDUMP, "--offloading", str(lib)], check=True, capture_output=True)
    objs = sorted(p for p in d.iterdir() if p.name.endswith("gfx950"))
    assert objs, "no gfx950 code object in the library"
    meta = {}
    for o in objs:
        notes = subprocess.run([READELF, "--notes", str(o)], check=True, capture_output=True,
                               text=True).stdout
        cur = {}
        for line in notes.splitlines():
            m = re.match(r"^\s+-?\s*\.(\w+):\s+(\S+)\s*$", line)
            if not m:
                continue
            k, v = m.groups()
            if k == "agpr_count" and line.lstrip().startswith("-"):
                cur = {}
            if k == "name":
                meta[v] = cur
            elif k in ("vgpr_count", "private_segment_fixed_size", "vgpr_spill_count"):
                cur[k] = int(v)
    return meta


def test_gated_kernels_exist_for_exactly_the_expected_dtypes(kernel_meta):
    plain = {PLAIN.match(k).group(1) for k in kernel_meta if PLAIN.match(k)}
    assert plain == {"f", "d", "NS_6bf16_tE"}, plain
    master = {MASTER.match(k).group(1) for k in kernel_meta if MASTER.match(k)}
    assert master == {"NS_6bf16_tE", "NS_5f16_tE"}, master


def test_gated_kernels_use_no_scratch(kernel_meta):
    ks = {k: v for k, v in kernel_meta.items() if PLAIN.match(k) or MASTER.match(k)}
    assert len(ks) == 5, sorted(ks)
    for k, v in ks.items():
        assert "private_segment_fixed_size" in v and "vgpr_spill_count" in v, (k, v)
    bad = [(k, v) for k, v in ks.items()
           if v["private_segment_fixed_size"] != 0 or v["vgpr_spill_count"] != 0]
    assert not bad, bad
    print({k: v.get("vgpr_count") for k, v in ks.items()})
