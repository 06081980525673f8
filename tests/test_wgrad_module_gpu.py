"""The weight-gradient scheduler's launch forms (vitmi.wgrad.group / table) against the single form (ops.wgrad) at the
same split: bit for bit, since the same slabs are summed in the same order (and a direct table member accumulates
its one chain over all K rows exactly as a split-1 slab does).

K = 1024 (16 k-tiles: every split the cost model can pick is 1 or 2, and it picks 2 for all of these); members
(M, N, batch) = (256, 256, 1), (256, 320, 3) with a B batch stride and padded destination strides, and for the group
form one sub-256 member (64, 320, 1). Operands are random bf16 with the last 64 K rows zero (the token padding)."""
import functools

import pytest
import torch

from vitmi import ops, wgrad
from vitmi.wgrad import Spec

pytestmark = pytest.mark.gpu

K = 1024
OUT_BS = 256 * 320 + 64  # destination stride of the batch-3 member


def operand(g, cols):
    x = torch.randn(K, cols, generator=g).to(torch.bfloat16)
    x[K - 64:] = 0
    return x.cuda()


@functools.lru_cache(maxsize=None)
def problem():
    """operand-only specs (out = None) and each member's ops.wgrad result at its natural split (2): computed once,
    never written"""
    g = torch.Generator().manual_seed(5)
    sps = [Spec(operand(g, 256), 256, operand(g, 256), 256, 256, 256, None, 256),
           Spec(operand(g, 256), 256, operand(g, 960), 960, 256, 320, None, 320, batch=3, b_bs=320, out_bs=OUT_BS),
           Spec(operand(g, 64), 64, operand(g, 320), 320, 64, 320, None, 320)]
    for sp in sps:
        assert ops.splitk_factor(sp.M, sp.N, K, sp.batch) == 2
    for n in (2, 3):
        assert ops.splitk_factor_group([(sp.M, sp.N, sp.batch) for sp in sps[:n]], K) == 2
    return sps, [reference(sp) for sp in sps]


def dest(sp, init=None):
    n = sp.batch * (sp.out_bs or sp.M * sp.N)
    return torch.zeros(n, device="cuda") if init is None else init.clone()


def reference(sp, init=None):
    out = dest(sp, init)
    ops.wgrad(sp.A, sp.lda, sp.B, sp.ldb, sp.M, sp.N, K, out, sp.ldo, accumulate=init is not None, batch=sp.batch,
              a_bs=sp.a_bs, b_bs=sp.b_bs, out_bs=sp.out_bs)
    return out


@pytest.mark.parametrize("common", [False, True], ids=["own", "common"])
def test_group_equals_single(common):
    sps, refs = problem()
    outs = [dest(sp) for sp in sps]
    wgrad.group([sp._replace(out=o) for sp, o in zip(sps, outs)], K, common=common)
    for o, r in zip(outs, refs):
        assert r.abs().max() > 0 and torch.equal(o, r)


@pytest.mark.parametrize("common", [False, True], ids=["own", "common"])
def test_group_accumulates_into_a_nonzero_destination(common):
    sps, _ = problem()
    g = torch.Generator().manual_seed(6)
    inits = [torch.randn(dest(sp).numel(), generator=g).cuda() for sp in sps]
    refs = [reference(sp, i) for sp, i in zip(sps, inits)]
    outs = [i.clone() for i in inits]
    wgrad.group([sp._replace(out=o, accumulate=True) for sp, o in zip(sps, outs)], K, common=common)
    for o, r, i in zip(outs, refs, inits):
        assert not torch.equal(r, i) and torch.equal(o, r)


def test_group_per_batch_destinations():
    """the batch-3 member's elements each into a tensor of their own, one of them accumulating"""
    sps, refs = problem()
    g = torch.Generator().manual_seed(7)
    init = torch.randn(256, 320, generator=g).cuda()
    zs = [torch.zeros(256, 320, device="cuda"), init.clone(), torch.zeros(256, 320, device="cuda")]
    o0 = dest(sps[0])
    wgrad.group([sps[0]._replace(out=o0), sps[1]._replace(out=zs, accumulate=(False, True, False))], K, common=False)
    assert torch.equal(o0, refs[0])
    ref1 = reference(sps[1], torch.cat([torch.zeros(OUT_BS), init.cpu().flatten(), torch.zeros(64),
                                        torch.zeros(OUT_BS)]).cuda())
    for z in range(3):
        assert torch.equal(zs[z].flatten(), ref1[z * OUT_BS:z * OUT_BS + 256 * 320]), z


@pytest.mark.parametrize("split", [1, 2], ids=["direct", "slabs"])
def test_table_equals_single(monkeypatch, split):
    """the members the table takes (M, N >= 256); the prepared table is launched twice and built once"""
    sps, refs = problem()
    sps, refs = sps[:2], refs[:2]
    if split == 1:
        monkeypatch.setattr(ops, "splitk_factor", lambda *a, **k: 1)
        monkeypatch.setattr(ops, "splitk_factor_group", lambda *a, **k: 1)
        refs = [reference(sp) for sp in sps]
    outs = [dest(sp) for sp in sps]
    ws = torch.empty(4 * 2 * 256 * 320, device="cuda")
    tables = {}
    run = [sp._replace(out=o) for sp, o in zip(sps, outs)]
    wgrad.table(run, K, tables, "t", alloc=lambda n: ws)
    assert len(tables) == 1
    (ent,) = tables.values()
    for o, r in zip(outs, refs):
        assert torch.equal(o, r)
        o.zero_()
    wgrad.table(run, K, tables, "t", alloc=lambda n: ws)
    assert len(tables) == 1 and next(iter(tables.values())) is ent  # not prepared again
    for o, r in zip(outs, refs):
        assert torch.equal(o, r)
