"""The LAMB kernels in the built library (no GPU needed), read from the code
objects' metadata notes as tests/test_sharded_adam_isa.py does: every kernel
of kf_lamb.hip exists for exactly its dtypes and touches no scratch."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
LIB = os.path.join(ROOT, "kungfu_amd", "libkungfu_amd.so")
OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"
READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"

# kernel<T>: any T, so that a dtype too many would be seen
F32_F64 = {"f", "d"}
SIXTEEN = {"NS_6bf16_tE", "NS_5f16_tE"}
TEMPLATES = {"lamb_moments_kernel": F32_F64, "lamb_master_moments_kernel": SIXTEEN,
             "lamb_apply_kernel": F32_F64, "lamb_master_apply_kernel": SIXTEEN}
TRUST = re.compile(r"^_ZN2kf\d+lamb_trust_kernelE")


def _template(name):
    return re.compile(r"^_ZN2kf\d+%sI(\w+?)EEv" % name)


@pytest.fixture(scope="module")
def kernel_meta(tmp_path_factory):
    if not (os.path.exists(OBJDUMP) and os.path.exists(READELF)):
        pytest.skip("llvm tools not found")
    if not os.path.exists(LIB):
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "kungfu_amd", "csrc")],
                       check=True)
    d = tmp_path_factory.mktemp("lamb_isa")
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


def _lamb_kernels(meta):
    out = {k: v for k, v in meta.items() if TRUST.match(k)}
    for name in TEMPLATES:
        out.update({k: v for k, v in meta.items() if _template(name).match(k)})
    return out


@pytest.mark.parametrize("name", sorted(TEMPLATES))
def test_lamb_kernels_exist_for_exactly_their_dtypes(kernel_meta, name):
    rx = _template(name)
    found = {rx.match(k).group(1) for k in kernel_meta if rx.match(k)}
    assert found == TEMPLATES[name], (name, found)


def test_trust_kernel_exists_once(kernel_meta):
    assert len([k for k in kernel_meta if TRUST.match(k)]) == 1


def test_lamb_kernels_use_no_scratch(kernel_meta):
    ks = _lamb_kernels(kernel_meta)
    assert len(ks) == 9, sorted(ks)
    for k, v in ks.items():
        assert "private_segment_fixed_size" in v and "vgpr_spill_count" in v, (k, v)
    bad = [(k, v) for k, v in ks.items()
           if v["private_segment_fixed_size"] != 0 or v["vgpr_spill_count"] != 0]
    assert not bad, bad
    print({k: v.get("vgpr_count") for k, v in ks.items()})
