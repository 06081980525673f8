"""vitmi.wgrad.table with accumulating specs at split 1 (direct members that add into their destination inside the
launch) against the single form, ops.wgrad(..., accumulate=True) at split 1, on a copy of the same random non-zero
destination: bit for bit, since both add the same one-chain f32 accumulator to the old value once.

test_wgrad_module_gpu's operands and its two table members, (256, 256, 1) and (256, 320, 3) with a B batch stride and
a padded destination stride, K = 1024 with the last 64 rows zero; the splits forced to 1."""
import torch
import pytest

from test_wgrad_module_gpu import K, dest, problem, reference
from vitmi import ops, wgrad

pytestmark = pytest.mark.gpu


def test_accumulating_table_equals_single_accumulate(monkeypatch):
    sps = problem()[0][:2]  # (before the splits are forced: it checks the cost model's own)
    monkeypatch.setattr(ops, "splitk_factor", lambda *a, **k: 1)
    monkeypatch.setattr(ops, "splitk_factor_group", lambda *a, **k: 1)
    g = torch.Generator().manual_seed(8)
    inits = [torch.randn(dest(sp).numel(), generator=g).cuda() for sp in sps]
    refs = [reference(sp, i) for sp, i in zip(sps, inits)]           # ops.wgrad(accumulate=True), split 1
    twice = [reference(sp, r) for sp, r in zip(sps, refs)]
    outs = [i.clone() for i in inits]
    run = [sp._replace(out=o, accumulate=True) for sp, o in zip(sps, outs)]
    tables = {}
    wgrad.table(run, K, tables, "t")
    (ent,) = tables.values()
    assert ent[2] == []                                               # direct members: no reduce job
    for o, r, i in zip(outs, refs, inits):
        assert not torch.equal(r, i) and torch.equal(o, r), float((o - r).abs().max())
    wgrad.table(run, K, tables, "t")                                  # the same prepared table adds again
    assert len(tables) == 1 and next(iter(tables.values())) is ent
    for o, r in zip(outs, twice):
        assert torch.equal(o, r)
    # the gap of the padded destination stride is untouched
    pad = outs[1].view(3, -1)[:, 256 * 320:]
    assert torch.equal(pad, inits[1].view(3, -1)[:, 256 * 320:])


def test_overwriting_and_accumulating_members_share_a_launch(monkeypatch):
    sps = problem()[0][:2]  # (before the splits are forced: it checks the cost model's own)
    monkeypatch.setattr(ops, "splitk_factor", lambda *a, **k: 1)
    monkeypatch.setattr(ops, "splitk_factor_group", lambda *a, **k: 1)
    g = torch.Generator().manual_seed(9)
    init = torch.randn(dest(sps[1]).numel(), generator=g).cuda()
    refs = [reference(sps[0]), reference(sps[1], init)]
    outs = [torch.full_like(dest(sps[0]), float("nan")), init.clone()]
    wgrad.table([sps[0]._replace(out=outs[0]), sps[1]._replace(out=outs[1], accumulate=True)], K, {}, "t")
    assert torch.equal(outs[0], refs[0]) and torch.equal(outs[1], refs[1])
