"""vitmi.wgrad.plan / table with accumulating specs at split 1: the spec becomes a direct table member that adds into
its destination inside the launch (its eighth element is wgrad.DIRECT_ACCUMULATE), with no slab and no reduce job.
Pure layout: CPU tensors, the prepared table replaced by a recorder."""
import pytest
import torch

from vitmi import ops, wgrad
from vitmi.wgrad import Spec

K = 128


def spec(M=256, N=320, batch=1, **kw):
    A, B = torch.zeros(K, M, dtype=torch.bfloat16), torch.zeros(K, batch * N, dtype=torch.bfloat16)
    out = torch.zeros(batch * (M * N + 64))
    return Spec(A, M, B, batch * N, M, N, out, N, batch=batch, b_bs=N if batch > 1 else 0,
                out_bs=M * N + 64 if batch > 1 else 0, **kw)


def test_accumulating_split_1_spec_is_a_direct_accumulating_member():
    sp = spec(batch=3, accumulate=True)
    views, members, jobs = wgrad.plan([sp], K, [1], None, table=True)
    assert views == [None] and jobs == []
    (m,) = members
    assert len(m) == 8 and m[7] == wgrad.DIRECT_ACCUMULATE == 2 and m[7] is not True
    assert m[2] is sp.out and (m[3], m[4], m[5]) == (sp.M, sp.N, K)
    assert (m[6]["ldc"], m[6]["c_bs"], m[6]["split_k"], m[6]["batch"]) == (sp.ldo, sp.out_bs, 1, 3)


def test_plain_direct_member_still_carries_true():
    plain, acc = spec(), spec(accumulate=True)
    _, members, jobs = wgrad.plan([plain, acc], K, [1, 1], None, table=True)
    assert members[0][7] is True and members[1][7] == wgrad.DIRECT_ACCUMULATE and jobs == []


def test_split_2_accumulating_spec_keeps_its_slab_and_accumulating_job():
    sp = spec(accumulate=True)
    ws = torch.zeros(2 * sp.M * sp.N)
    views, members, jobs = wgrad.plan([sp], K, [2], ws, table=True)
    assert views[0] is not None and members[0][7] is False
    assert len(jobs) == 1 and jobs[0][8] is True


@pytest.mark.parametrize("acc", [False, True, (True, False, True)])
def test_per_z_destination_list_still_raises(acc):
    sp = spec(batch=3)
    sp = sp._replace(out=[torch.zeros(sp.M, sp.N) for _ in range(3)], accumulate=acc)
    with pytest.raises(ValueError):
        wgrad.plan([sp], K, [1], None, table=True)


def test_table_prepares_one_entry_per_flag_under_one_slot(monkeypatch):
    built = []

    class Recorder:
        def __init__(self, members):
            built.append([m[7] for m in members])

        def launch(self):
            pass

    monkeypatch.setattr(ops, "GemmGroupTable", Recorder)
    monkeypatch.setattr(ops, "splitk_factor_group", lambda *a, **k: 1)
    a, b = spec(), spec(M=512, N=256)
    plain, acc = [a, b], [a._replace(accumulate=True), b._replace(accumulate=True)]
    tables = {}
    wgrad.table(plain, K, tables, "slot")
    assert built == [[True, True]]
    wgrad.table(plain, K, tables, "slot")
    assert len(built) == 1                                    # the same key: not prepared again
    wgrad.table(acc, K, tables, "slot")
    assert built[1:] == [[wgrad.DIRECT_ACCUMULATE] * 2]       # the flag is part of the key: a new entry
    wgrad.table(acc, K, tables, "slot")
    assert len(built) == 2
    # distinct slots keep both prepared, as the engine's (batch, launch) / (batch, True, launch) slots do
    wgrad.table(plain, K, tables, "other")
    wgrad.table(acc, K, tables, ("other", True))
    wgrad.table(plain, K, tables, "other")
    wgrad.table(acc, K, tables, ("other", True))
    assert len(built) == 4
