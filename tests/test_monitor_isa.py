"""gfx950 ISA of the segmented-norm kernels, read from the built library (no
GPU needed), as tests/test_isa.py does for the reduce kernels: they exist for
the four float dtypes in both modes, their streaming loads are 16-B and
non-temporal, they accumulate in fp64 and they never touch scratch."""
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

# segnorm_kernel<T, MODE>: f32, f64, f16_t, bf16_t x {SQ, VAR}
NORM = re.compile(r"^_ZN2kf14segnorm_kernelI(f|d|NS_5f16_tE|NS_6bf16_tE)Li([01])EEEv")
HELPERS = ("_ZN2kf19segnorm_fold_kernelE", "_ZN2kf20segnorm_total_kernelE",
           "_ZN2kf18noise_scale_kernelE")


@pytest.fixture(scope="module")
def objects(tmp_path_factory):
    if not (os.path.exists(OBJDUMP) and os.path.exists(READELF)):
        pytest.skip("llvm tools not found")
    if not os.path.exists(LIB):
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "kungfu_amd", "csrc")],
                       check=True)
    d = tmp_path_factory.mktemp("monitor_isa")
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


def test_norm_kernels_exist_for_the_four_dtypes(kernels):
    found = {NORM.match(k).groups() for k in kernels if NORM.match(k)}
    assert found == {(t, m) for t in ("f", "d", "NS_5f16_tE", "NS_6bf16_tE") for m in "01"}, found
    for h in HELPERS:
        assert any(k.startswith(h) for k in kernels), h


def test_norm_kernels_are_not_test_isa_subjects(kernels):
    """tests/test_isa.py picks its subjects by these prefixes; the new family
    must not change what it selects."""
    taken = ("_ZN2kf13reduce_kernel", "_ZN2kf19reduce_batch_kernel",
             "_ZN2kf20reduce_spread_kernel", "_ZN2kf10sma_kernel", "_ZN2kf16sma_batch_kernel")
    for k in kernels:
        if NORM.match(k) or k.startswith(HELPERS):
            assert not k.startswith(taken), k


def test_norm_streaming_loads_are_16_byte_nontemporal(kernels):
    for name, lines in kernels.items():
        m = NORM.match(name)
        if not m:
            continue
        loads = [i for i in lines if i.startswith("global_load_dwordx4")]
        # the full tile's eight loads and the ragged tile's (two streams in VAR)
        assert len(loads) >= 9, (name, len(loads))
        bad = [i for i in loads if not re.search(r"\bnt\b", i)]
        assert not bad, (name, bad[:3])
        # the full tile issues its eight loads before the first wait on them
        run = best = 0
        for ins in lines:
            if ins.startswith("global_load_dwordx4"):
                run += 1
                best = max(best, run)
            elif ins.startswith("s_waitcnt") and "vmcnt" in ins:
                run = 0
        assert best >= 8, (name, best)
        # fp64 from the first add, and no float atomics anywhere
        assert any(re.match(r"v_fmac?_f64", i) for i in lines), name
        assert not [i for i in lines if "atomic" in i], name


def test_norm_kernels_use_no_scratch(kernel_meta):
    ks = {k: v for k, v in kernel_meta.items() if NORM.match(k) or k.startswith(HELPERS)}
    assert len(ks) == 8 + len(HELPERS), sorted(ks)
    bad = [(k, v) for k, v in ks.items()
           if v.get("private_segment_fixed_size", 0) or v.get("vgpr_spill_count", 0)]
    assert not bad, bad
    # eight waves per SIMD: the streaming kernels stay within 64 VGPRs
    over = [(k, v["vgpr_count"]) for k, v in ks.items() if v["vgpr_count"] > 64]
    assert not over, over
