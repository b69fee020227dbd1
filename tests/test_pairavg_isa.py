"""gfx950 ISA of the pair-averaging kernels, read from the built library (no
GPU needed), by the method of tests/test_monitor_isa.py: the copy / fetch
kernels and the blend kernels for the four float dtypes exist, their streaming
loads and stores are 16-B and non-temporal, none of the family touches
scratch, and they stay within 64 VGPRs."""
import os
import re
import shutil
import subprocess
from collections import defaultdict

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
LIB = os.path.join(ROOT, "kungfu_amd", "libkungfu_amd.so")
OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"
READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"

# pairavg_blend_kernel<T>: f32, f64, f16_t, bf16_t
BLEND = re.compile(r"^_ZN2kf20pairavg_blend_kernelI(f|d|NS_5f16_tE|NS_6bf16_tE)EEv")
COPIES = ("_ZN2kf19pairavg_copy_kernelE", "_ZN2kf20pairavg_fetch_kernelE")
MARKERS = ("_ZN2kf20pairavg_begin_kernelE", "_ZN2kf18pairavg_end_kernelE",
           "_ZN2kf19pairavg_pick_kernelE", "_ZN2kf20pairavg_check_kernelE")


def _family(name):
    return bool(BLEND.match(name)) or name.startswith(COPIES + MARKERS)


@pytest.fixture(scope="module")
def objects(tmp_path_factory):
    if not (os.path.exists(OBJDUMP) and os.path.exists(READELF)):
        pytest.skip("llvm tools not found")
    if not os.path.exists(LIB):
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "kungfu_amd", "csrc")],
                       check=True)
    d = tmp_path_factory.mktemp("pairavg_isa")
    lib = d / "lib.so"
    shutil.copy(LIB, lib)
    subprocess.run([OBJDUMP, "--offloading", str(lib)], check=True, capture_output=True)
    objs = sorted(p for p in d.iterdir() if p.name.endswith("gfx950"))
    assert objs, "no gfx950 code object in the library"
    return objs


@pytest.fixture(scope="module")
def kernels(objects):
    body = defaultdict(list)
    for o in objects:
        asm = subprocess.run([OBJDUMP, "-d", str(o)], check=True, capture_output=True,
                             text=True).stdout
        name = None
        for line in asm.splitlines():
            m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
            if m:
                name = m.group(1)
            elif name and line.strip():
                body[name].append(line.split("//")[0].strip())
            else:
                name = None
    return body


@pytest.fixture(scope="module")
def kernel_meta(objects):
    meta = {}
    for o in objects:
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


def test_pairavg_kernels_exist(kernels):
    found = {BLEND.match(k).group(1) for k in kernels if BLEND.match(k)}
    assert found == {"f", "d", "NS_5f16_tE", "NS_6bf16_tE"}, found
    for h in COPIES + MARKERS:
        assert sum(1 for k in kernels if k.startswith(h)) == 1, h


def test_pairavg_kernels_are_not_other_isa_tests_subjects(kernels):
    """tests/test_isa.py and tests/test_monitor_isa.py pick their subjects by
    these prefixes; the new family must not change what they select."""
    taken = ("_ZN2kf13reduce_kernel", "_ZN2kf19reduce_batch_kernel",
             "_ZN2kf20reduce_spread_kernel", "_ZN2kf10sma_kernel", "_ZN2kf16sma_batch_kernel",
             "_ZN2kf14segnorm_kernel", "_ZN2kf19segnorm_fold_kernel",
             "_ZN2kf20segnorm_total_kernel", "_ZN2kf18noise_scale_kernel")
    ours = [k for k in kernels if _family(k)]
    assert len(ours) == 10, sorted(ours)
    for k in ours:
        assert not k.startswith(taken), k


def test_pairavg_streaming_accesses_are_16_byte_nontemporal(kernels):
    subjects = [k for k in kernels if BLEND.match(k) or k.startswith(COPIES)]
    assert len(subjects) == 6, sorted(subjects)
    for name in subjects:
        lines = kernels[name]
        loads = [i for i in lines if re.match(r"(global|flat|buffer)_load_dwordx4", i)]
        stores = [i for i in lines if re.match(r"(global|flat|buffer)_store_dwordx4", i)]
        # a tile is 4 vectors per lane: 4 loads per stream, 4 stores
        want_loads = 8 if BLEND.match(name) else 4
        assert len(loads) >= want_loads and len(stores) >= 4, (name, len(loads), len(stores))
        bad = [i for i in loads + stores
               if not i.startswith("global_") or not re.search(r"\bnt\b", i)]
        assert not bad, (name, bad[:3])


def test_pairavg_kernels_use_no_scratch(kernel_meta):
    ks = {k: v for k, v in kernel_meta.items() if _family(k)}
    assert len(ks) == 10, sorted(ks)
    bad = [(k, v) for k, v in ks.items()
           if v.get("private_segment_fixed_size", 0) or v.get("vgpr_spill_count", 0)]
    assert not bad, bad
    # eight waves per SIMD: the family stays within 64 VGPRs
    over = [(k, v["vgpr_count"]) for k, v in ks.items() if v["vgpr_count"] > 64]
    assert not over, over
