"""The refusals of the batched update wrappers that sit behind the device
check, with their full texts: the lead table's dtype, a state of the wrong
dtype or length, 8-bit codes and scales of the wrong length, and a gate that
is too small or misaligned. No call here gets as far as a launch."""
import pytest
import torch

from kungfu_amd import _lib, ops

pytestmark = pytest.mark.gpu

N = (64, 192)  # the smallest legal adam8 segments: one shape list for every wrapper
H = {"lr": 1e-3, "step": 1}
f32, f16, bf16, f64, i32 = (torch.float32, torch.float16, torch.bfloat16, torch.float64,
                            torch.int32)

# wrapper -> (a lead dtype it takes, the tables after the lead, a lead dtype it refuses, the
#             refusal of that lead: its type and text, the text of a mismatching table)
MISMATCH = "%s: shape/dtype mismatch"
MISMATCH_SR = "%s: bf16 tensors of one shape per segment"
MISMATCH_8 = ("%s: shape/dtype mismatch (uint8 codes of the parameters' length, one f32 scale "
              "per 64 elements)")
C_DTYPE = "%s failed: KF_ERR_DTYPE (KF_ERR_DTYPE: %s: %s)"
ADAM8_TABLES = ["same", "u8", "u8", "scale", "scale"]
WRAPPERS = {
    "sgd_update_batch_": (f32, ["same"] * 2, i32, _lib.KungFuAMDError, C_DTYPE % (
        "kf_sgd_update_batch", "kf_sgd_update_batch", "f32, f16, bf16 and f64 only"), MISMATCH),
    "adam_update_batch_": (f32, ["same"] * 3, f16, _lib.KungFuAMDError, C_DTYPE % (
        "kf_adam_update_batch", "kf_adam_update_batch",
        "f32, bf16 and f64 only (eps = 1e-8 is 0 in f16: 0 / 0 where v == 0)"), MISMATCH),
    "adam_update_batch_gated_": (f32, ["same"] * 3, f16, _lib.KungFuAMDError, C_DTYPE % (
        "kf_adam_update_batch_gated", "kf_adam_update_batch_gated",
        "f32, bf16 and f64 only (eps = 1e-8 is 0 in f16: 0 / 0 where v == 0)"), MISMATCH),
    "adam_master_update_batch_": (
        bf16, ["same", "f32", "f32", "f32"], f32, ValueError,
        "adam_master_update_batch_: bf16 or f16 parameters", MISMATCH),
    "adam_master_update_batch_gated_": (
        f16, ["same", "f32", "f32", "f32"], f32, ValueError,
        "adam_master_update_batch_gated_: bf16 or f16 parameters", MISMATCH),
    "adam_sr_update_batch_": (
        bf16, ["same"] * 3, f32, ValueError, MISMATCH_SR % "adam_sr_update_batch_", MISMATCH_SR),
    "adam_sr_update_batch_gated_": (
        bf16, ["same"] * 3, f16, ValueError, MISMATCH_SR % "adam_sr_update_batch_gated_",
        MISMATCH_SR),
    "adam8_update_batch_": (
        f32, ADAM8_TABLES, bf16, ValueError, "adam8_update_batch_: torch.float32 parameters",
        MISMATCH_8),
    "adam8_update_batch_gated_": (
        f32, ADAM8_TABLES, f64, ValueError,
        "adam8_update_batch_gated_: torch.float32 parameters", MISMATCH_8),
    "adam8_master_update_batch_": (
        bf16, ["same", "f32"] + ADAM8_TABLES[1:], f32, ValueError,
        "adam8_master_update_batch_: torch.bfloat16 or torch.float16 parameters", MISMATCH_8),
    "adam8_master_update_batch_gated_": (
        f16, ["same", "f32"] + ADAM8_TABLES[1:], f32, ValueError,
        "adam8_master_update_batch_gated_: torch.bfloat16 or torch.float16 parameters",
        MISMATCH_8),
    "lamb_moments_batch_": (f32, ["same"] * 4, bf16, _lib.KungFuAMDError, C_DTYPE % (
        "kf_lamb_moments_batch", "kf_lamb_moments_batch",
        "f32 and f64 only (bf16 and f16 take kf_lamb_master_moments_batch)"), MISMATCH),
    "lamb_moments_batch_gated_": (f32, ["same"] * 4, f16, _lib.KungFuAMDError, C_DTYPE % (
        "kf_lamb_moments_batch_gated", "kf_lamb_moments_batch_gated",
        "f32 and f64 only (bf16 and f16 take kf_lamb_master_moments_batch_gated)"), MISMATCH),
    "lamb_master_moments_batch_": (
        bf16, ["f32"] * 4, f32, ValueError, "lamb_master_moments_batch_: bf16 or f16 gradients",
        MISMATCH),
    "lamb_master_moments_batch_gated_": (
        f16, ["f32"] * 4, f64, ValueError,
        "lamb_master_moments_batch_gated_: bf16 or f16 gradients", MISMATCH),
}
GATED = sorted(n for n in WRAPPERS if n.endswith("gated_"))
# the gated wrappers that look at the gate only after the tables
TABLES_BEFORE_GATE = {n for n in GATED if "_sr_" in n or "adam8" in n}
GATE_TEXT = "the gate must be at least 48 uint8 bytes, 8-byte aligned"


def dev():
    return torch.device("cuda", torch.cuda.current_device())


def one(kind, lead, n):
    dtype = {"same": lead, "f32": f32, "u8": torch.uint8, "scale": f32}[kind]
    return torch.zeros(n // 64 if kind == "scale" else n, dtype=dtype, device=dev())


def tables(name, lead=None):
    spec = WRAPPERS[name]
    lead = spec[0] if lead is None else lead
    return [[one(kind, lead, n) for n in N] for kind in ["same"] + spec[1]]


def call(name, tabs, gate=None, states=None, group=0):
    fn, gated, sr = getattr(ops, name), name.endswith("gated_"), "_sr_" in name
    if gated:
        gate = ops.new_step_gate(dev()) if gate is None else gate
        states = ops.new_step_states(dev(), group + 1) if states is None else states
    args = list(tabs) + ([H, gate, states] if gated else [[H] * len(tabs[0])])
    if sr:
        args += [[0, 64], [1, 2], 7]
    return fn(*args, **(dict(group=group) if gated else {}))


def refused(kind, text, name, *a, **kw):
    with pytest.raises(kind) as err:
        call(name, *a, **kw)
    assert type(err.value) is kind and str(err.value) == text


@pytest.mark.parametrize("name", sorted(WRAPPERS))
def test_lead_table_of_the_wrong_dtype(name):
    _, _, bad, kind, text, mismatch = WRAPPERS[name]
    refused(kind, text, name, tables(name, bad))
    t = tables(name)
    t[0][1] = torch.zeros(N[1], dtype=f64, device=dev())  # segment 1 differs from segment 0
    refused(ValueError, mismatch % name, name, t)


@pytest.mark.parametrize("name", sorted(WRAPPERS))
def test_table_of_the_wrong_dtype_or_length(name):
    """Every table after the lead, in either segment: states, masters, 8-bit
    codes and scales."""
    mismatch = WRAPPERS[name][5] % name
    for i in range(1, len(WRAPPERS[name][1]) + 1):
        for seg in (0, 1):
            good = tables(name)[i][seg]
            for wrong in (torch.zeros(good.numel(), dtype=f64, device=dev()),
                          torch.zeros(128, dtype=good.dtype, device=dev()),
                          torch.zeros(good.numel() + 1, dtype=good.dtype, device=dev())):
                t = tables(name)
                t[i][seg] = wrong
                refused(ValueError, mismatch, name, t)


@pytest.mark.parametrize("name", GATED)
def test_gate_too_small_or_misaligned(name):
    t = tables(name)
    d = dev()
    refused(ValueError, GATE_TEXT, name, t, gate=torch.zeros(47, dtype=torch.uint8, device=d))
    refused(ValueError, GATE_TEXT, name, t, gate=torch.zeros(64, dtype=torch.uint8, device=d)[4:])
    refused(ValueError, GATE_TEXT, name, t, gate=torch.zeros(12, dtype=f32, device=d))
    states = "the step states must be at least %d uint8 bytes, 8-byte aligned"
    refused(ValueError, states % 48, name, t, states=torch.zeros(40, dtype=torch.uint8, device=d))
    refused(ValueError, states % 96, name, t, group=1,
            states=torch.zeros(95, dtype=torch.uint8, device=d))
    refused(ValueError, states % 48, name, t,
            states=torch.zeros(64, dtype=torch.uint8, device=d)[4:])
    refused(ValueError, "kungfu_amd device ops need GPU tensors (got cpu)", name, t,
            gate=torch.zeros(48, dtype=torch.uint8))


@pytest.mark.parametrize("name", GATED)
def test_gate_and_tables_keep_their_order(name):
    """A gate that is too small and a table that does not fit, in one call."""
    _, _, bad, kind, text, mismatch = WRAPPERS[name]
    small = torch.zeros(8, dtype=torch.uint8, device=dev())
    t = tables(name)
    t[1][1] = torch.zeros(128, dtype=t[1][1].dtype, device=dev())
    refused(ValueError, mismatch % name if name in TABLES_BEFORE_GATE else GATE_TEXT, name, t,
            gate=small)
    if kind is ValueError:  # the lead's dtype is the wrapper's own check
        refused(ValueError, text if name in TABLES_BEFORE_GATE else GATE_TEXT, name,
                tables(name, bad), gate=small)


@pytest.mark.parametrize("name", ["lamb_trust_update_", "lamb_trust_update_gated_"])
def test_trust_update_refusals(name):
    d, gated = dev(), name.endswith("gated_")
    groups = [{"lr": 1.0, "adapt": True}]

    def refuse(text, sq=4, group_of=2, group_dtype=torch.int32, groups=groups, nlr=2, ratio=2,
               out_dtype=f64, sq_dtype=f64, world=1, gate=None):
        args = [torch.zeros(sq, dtype=sq_dtype, device=d), world,
                torch.zeros(group_of, dtype=group_dtype, device=d), groups,
                torch.zeros(nlr, dtype=out_dtype, device=d),
                torch.zeros(ratio, dtype=out_dtype, device=d)]
        if gated:
            args.append(ops.new_step_gate(d) if gate is None else gate)
        with pytest.raises(ValueError) as err:
            getattr(ops, name)(*args)
        assert str(err.value) == text

    first = name + ": group_of is a non-empty int32 tensor, and at least one group"
    refuse(first, group_dtype=torch.int64)
    refuse(first, group_of=0, sq=0, nlr=0, ratio=0)
    refuse(first, groups=[])
    second = name + ": sq is world * 2 * T float64 values"
    refuse(second, sq=5)
    refuse(second, sq_dtype=f32)
    refuse(second, world=0, sq=0)
    third = name + ": nlr and ratio are T float64 values"
    refuse(third, nlr=3)
    refuse(third, ratio=1)
    refuse(third, out_dtype=f32)
    refuse(first, group_dtype=torch.int64, sq=5, nlr=3)   # in this order
    refuse(second, sq=5, nlr=3)
    if gated:
        refuse(GATE_TEXT, gate=torch.zeros(8, dtype=torch.uint8, device=d), groups=[])
