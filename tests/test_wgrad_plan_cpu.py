"""The weight-gradient scheduler's planning step (vitmi.wgrad.plan): slab placement, the member tuples of the grouped
and table launches and the reduce jobs, on meta tensors (only shapes and storage offsets are read; no library)."""
import itertools

import torch

from vitmi import ops, wgrad
from vitmi._lib import EPI_SPLITK, MN_CONTIG
from vitmi.wgrad import Spec

K = 4096
D = 768
SZ = D * D


def t(*shape, dtype=torch.bfloat16):
    return torch.empty(*shape, device="meta", dtype=dtype)


def specs(out_bs=4 * SZ):
    A1, B1, A2, B2 = t(K, D), t(K, D), t(K, D), t(K, 3 * D)
    o1, o2 = t(D, D, dtype=torch.float32), t(3 * out_bs, dtype=torch.float32)
    return [Spec(A1, D, B1, D, D, D, o1, D), Spec(A2, D, B2, 3 * D, D, D, o2, D, batch=3, b_bs=D, out_bs=out_bs)]


def own_and_common(sps):
    own = [ops.splitk_factor(sp.M, sp.N, K, sp.batch) for sp in sps]
    return own, ops.splitk_factor_group([(sp.M, sp.N, sp.batch) for sp in sps], K)


def test_spec_defaults():
    sp = Spec(None, 1, None, 2, 3, 4, None, 5)
    assert (sp.batch, sp.a_bs, sp.b_bs, sp.out_bs, sp.accumulate) == (1, 0, 0, 0, False)


def test_splits_of_the_two_specs():
    own, common = own_and_common(specs())
    assert own == [8, 7] and common == 6


def test_own_split_plan_packs_slabs_in_spec_order():
    sps = specs()
    ws = t(64 * SZ, dtype=torch.float32)
    views, members, jobs = wgrad.plan(sps, K, [8, 7], ws)
    assert [v.numel() for v in views] == [8 * SZ, 3 * 7 * SZ]
    assert [v.storage_offset() for v in views] == [0, 8 * SZ]
    assert all(v.storage_offset() % 4 == 0 for v in views)
    assert len(members) == 2 and all(len(m) == 7 for m in members)  # ops.gemm_splitk_group's form
    for sp, s, v, (A, B, C, M, N, k, kw) in zip(sps, [8, 7], views, members):
        assert A is sp.A and B is sp.B and C is v and (M, N, k) == (D, D, K)
        assert kw == dict(a_layout=MN_CONTIG, b_layout=MN_CONTIG, lda=sp.lda, ldb=sp.ldb, ldc=N, epilogue=EPI_SPLITK,
                          batch=sp.batch, a_bs=0, b_bs=sp.b_bs, c_bs=0, split_k=s)
    # ops.splitk_reduce_group's order: (ws, batch, split, M, N, out, ldo, out_bs, accumulate)
    assert len(jobs) == 2
    for sp, s, v, job in zip(sps, [8, 7], views, jobs):
        assert job[0] is v and job[5] is sp.out
        assert job[1:5] + job[6:] == (sp.batch, s, D, D, D, sp.out_bs, False)


def test_common_split_plan():
    sps = specs()
    views, members, jobs = wgrad.plan(sps, K, [6, 6], t(64 * SZ, dtype=torch.float32))
    assert [v.numel() for v in views] == [6 * SZ, 3 * 6 * SZ]
    assert [v.storage_offset() for v in views] == [0, 6 * SZ]
    assert all(m[6]["ldc"] == m[4] and m[6]["split_k"] == 6 for m in members)
    assert [j[2] for j in jobs] == [6, 6]


def test_table_plan_with_slabs_marks_no_member_direct():
    sps = specs()
    views, members, jobs = wgrad.plan(sps, K, [6, 6], t(64 * SZ, dtype=torch.float32), table=True)
    assert all(len(m) == 8 and m[7] is False and m[2] is v and m[6]["ldc"] == D for m, v in zip(members, views))
    assert len(jobs) == 2


def test_direct_table_plan_has_no_slab_and_no_reduce_job():
    sps = specs()
    views, members, jobs = wgrad.plan(sps, K, [1, 1], None, table=True)
    assert views == [None, None] and jobs == []
    for sp, (A, B, C, M, N, k, kw, direct) in zip(sps, members):
        assert direct is True and C is sp.out and A is sp.A and B is sp.B
        assert kw["ldc"] == sp.ldo and kw["c_bs"] == sp.out_bs and kw["split_k"] == 1 and kw["batch"] == sp.batch
    assert members[1][6]["c_bs"] == 4 * SZ


def test_accumulate_reaches_the_reduce_job():
    sp = specs()[0]._replace(accumulate=True)
    _, _, jobs = wgrad.plan([sp], K, [8], t(8 * SZ, dtype=torch.float32))
    assert jobs[0][8] is True


def test_per_batch_destinations_give_one_job_per_element():
    sp = specs()[1]
    outs = [t(D, D, dtype=torch.float32) for _ in range(3)]
    sp = sp._replace(out=outs, accumulate=(True, False, True))
    first = specs()[0]
    views, members, jobs = wgrad.plan([first, sp], K, [8, 7], t(64 * SZ, dtype=torch.float32))
    assert len(members) == 2 and members[1][6]["batch"] == 3 and members[1][2] is views[1]
    assert len(jobs) == 4
    for z, job in enumerate(jobs[1:]):
        w, batch, s, M, N, out, ldo, out_bs, acc = job
        assert (batch, s, M, N, ldo, out_bs) == (1, 7, D, D, D, 0) and out is outs[z]
        assert w.numel() == 7 * SZ and w.storage_offset() == 8 * SZ + z * 7 * SZ
        assert acc is (True, False, True)[z]


def test_single_and_group_cost_models_agree_on_256_tiles():
    """the property the one model function rests on: a lone member with M, N >= 256 gets the same split from either
    public function"""
    for M, N, k, b in itertools.product((256, 512, 768, 1024, 3072), (256, 768, 2304), (192, 4096, 50432), (1, 3)):
        assert ops.splitk_factor(M, N, k, b) == ops.splitk_factor_group([(M, N, b)], k), (M, N, k, b)
