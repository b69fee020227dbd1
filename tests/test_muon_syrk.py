"""The symmetric product without a device: names, refusals, the keyword."""
import pytest
import torch

ERR_DTYPE, ERR_ARG = 1, 3
BF16, F16 = 0x20209, 0x20208


def test_names_declared_and_exported():
    from kungfu_amd import _lib, ops
    header = open(_lib.__file__.replace("kungfu_amd/_lib.py", "include/kungfu_amd.h")).read()
    assert "kf_muon_syrk_grouped" in _lib.EXPORTED and "kf_muon_syrk_grouped(" in header
    assert _lib.load().kf_muon_syrk_grouped and hasattr(ops, "muon_syrk_grouped_")
    assert ops.muon_syrk_grouped_([]) == [] and ops.muon_tile() == 64


def test_c_entry_refusals_in_order():
    """Each call has one fault more to its right than the refusal it must report."""
    from kungfu_amd import _lib
    lib = _lib.load()
    why = lambda: lib.kf_last_error().decode()  # noqa: E731

    def syrk(count=1, dt=BF16, table=True, **fields):
        q = (_lib.MuonGemm * 1)()
        vals = dict(a=2, b=None, c=6, cin=None, m=3, n=3, k=5, lda=5, ldb=0, ldcin=3, ldc=3,
                    trans_a=0, trans_b=0)
        vals.update(fields)
        for k, v in vals.items():
            setattr(q[0], k, v)
        return lib.kf_muon_syrk_grouped(q if table else None, count, dt, 1.0, 1.0, None)

    assert syrk(count=-1, table=False) == ERR_ARG and "count < 0" in why()
    assert syrk(count=0, table=False) == 0
    assert syrk(dt=F16, table=False) == ERR_DTYPE and "bf16" in why()
    assert syrk(table=False, m=0) == ERR_ARG and "null table" in why()
    assert syrk(k=0, n=4) == ERR_ARG and "dimension" in why()
    assert syrk(k=(1 << 31) - 32, n=4) == ERR_ARG and "INT_MAX" in why()
    assert syrk(n=4, a=None) == ERR_ARG and "symmetric" in why()
    assert syrk(b=4, c=None) == ERR_ARG and "symmetric" in why()
    assert syrk(c=None, cin=9) == ERR_ARG and "null matrix" in why()
    for off in ({"a": 3}, {"c": 7}, {"cin": 9}):
        assert syrk(trans_a=2, **off) == ERR_ARG and "misaligned" in why(), off
    assert syrk(trans_a=2, lda=4) == ERR_ARG and "0 or 1" in why()
    big = dict(m=1 << 30, n=1 << 30, ldc=1 << 30)
    for ld in ({"lda": 4}, {"ldc": 2}, {"cin": 8, "ldcin": 2}, {"trans_a": 1, "lda": 2},
               dict(big, cin=8, ldcin=3)):
        assert syrk(**ld) == ERR_ARG and "leading dimension" in why(), ld
    assert syrk(**big) == ERR_ARG and "tiles" in why()
    # 2896 tiles a side are 4,194,856 launched tiles: one row of tiles too many
    assert syrk(m=2896 * 64, n=2896 * 64, ldc=2896 * 64) == ERR_ARG and "tiles" in why()


@pytest.mark.parametrize("bad", [1, 0, None, "yes"])
def test_symmetric_must_be_a_bool(bad):
    from kungfu_amd import ops
    from kungfu_amd.optimizers import ShardedMuonOptimizer
    sgd = torch.optim.SGD(torch.nn.Linear(5, 3, bias=False).parameters(), lr=0.02)
    for name, call in (("MuonPlan", lambda: ops.MuonPlan([], [], symmetric=bad)),
                       ("muon_newton_schulz_", lambda: ops.muon_newton_schulz_([], symmetric=bad)),
                       ("ShardedMuonOptimizer", lambda: ShardedMuonOptimizer(sgd, symmetric=bad))):
        with pytest.raises(ValueError) as e:
            call()
        assert str(e.value) == "%s: symmetric must be a bool, not %r" % (name, bad)
    assert ShardedMuonOptimizer(sgd, symmetric=True)._kf_symmetric
