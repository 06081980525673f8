"""Deferred weight gradients (ViTEngine.wgrad_defer, VITMI_WGRAD_DEFER): the full-token layers' weight-gradient
GEMMs recorded during the backward and run as one batched launch (ops.GemmGroupTable) per N layers.

Config: D = 256, 4 heads, MLP 512, 3 layers, 32-px images in 8-px patches (17 tokens), batch 8, so T = 136 is no
multiple of 64 and the token rows are zero-padded to 192 (3 k-tiles). Every layer's four weight gradients have
M, N >= 256 and join the batch; the 192-column patch-embedding gradient and the pruned last layer's cls-row
gradients stay on their own launches in both modes.
"""
import functools

import pytest
import torch

from oracle.vit_oracle import ViTConfig, init_params, loss_and_grads, tame_params
from test_parity_gpu import check_grads, make_model

pytestmark = pytest.mark.gpu

CFG = ViTConfig(image_size=32, patch_size=8, emb_dim=256, mlp_dim=512, num_heads=4, num_layers=3, num_classes=10)
BS = 8
DEFER = ["0", "1", "2", "all"]


@functools.lru_cache(maxsize=None)
def problem():
    """params, x, y and the oracle's gradients: computed once, shared by every case, never written"""
    params = tame_params(init_params(CFG, seed=42))
    g = torch.Generator().manual_seed(21)
    x = torch.randn(BS, 3, CFG.image_size, CFG.image_size, generator=g)
    y = torch.randint(0, CFG.num_classes, (BS,), generator=g)
    _, _, ref_grads = loss_and_grads(params, x, y, CFG)
    return params, x.cuda(), y.cuda(), ref_grads


def run(monkeypatch, prune, defer, hook=None):
    """one forward + backward with VITMI_WGRAD_DEFER = defer; returns (model, a copy of the flat gradient buffer)"""
    from vitmi.model import CrossEntropyLoss
    params, x, y, _ = problem()
    monkeypatch.setenv("VITMI_WGRAD_DEFER", defer)
    m = make_model(CFG, params)
    m(x[:1])  # builds the engine (which reads the knob)
    eng = m._engine
    assert eng.wgrad_defer == (CFG.num_layers if defer == "all" else int(defer))
    eng.prune_last = prune
    eng.grad_ready_hook = hook
    m.zero_grad()
    CrossEntropyLoss()(m(x), y).backward()
    torch.cuda.synchronize()
    return m, eng.grad.detach().clone()


def force_split_1(monkeypatch):
    from vitmi import ops
    monkeypatch.setattr(ops, "splitk_factor", lambda *a, **k: 1)
    monkeypatch.setattr(ops, "splitk_factor_group", lambda *a, **k: 1)


@pytest.mark.parametrize("prune", [False, True], ids=["full", "pruned"])
def test_deferred_equals_per_layer_at_split_1(monkeypatch, prune):
    """With every split forced to 1 both paths accumulate each tile over all tokens in one chain, in the same
    order: the whole gradient buffer must agree bit for bit, for every layers-per-launch setting."""
    force_split_1(monkeypatch)
    _, ref = run(monkeypatch, prune, "0")
    for defer in DEFER[1:]:
        m, got = run(monkeypatch, prune, defer)
        assert len(m._engine._wgrad_tables) == -(-CFG.num_layers // m._engine.wgrad_defer), defer
        assert torch.equal(got, ref), (defer, float((got - ref).abs().max()))


@pytest.mark.parametrize("defer", DEFER)
@pytest.mark.parametrize("prune", [False, True], ids=["full", "pruned"])
def test_gradients_pass_the_oracle_gate(monkeypatch, prune, defer):
    """the split factors as the cost model picks them; the gate is test_parity_gpu's"""
    m, _ = run(monkeypatch, prune, defer)
    check_grads(m, problem()[3])


@pytest.mark.parametrize("prune", [False, True], ids=["full", "pruned"])
def test_deferred_runs_are_bit_identical(monkeypatch, prune):
    _, g0 = run(monkeypatch, prune, "all")
    _, g1 = run(monkeypatch, prune, "all")
    assert torch.equal(g0, g1)


def test_grad_ready_hook_keeps_the_per_layer_path(monkeypatch):
    """A reducer's hook needs each bucket's gradients when the hook fires, so the per-layer path must run: one
    call per bucket in backward order, each bucket already complete at its call (compared on the hook's stream
    order with the per-layer run), and no batched launch prepared."""
    _, ref = run(monkeypatch, True, "0")
    calls, snaps = [], []

    def hook(g, name, start, end, events):
        calls.append(name)
        snaps.append((start, end, g[start:end].clone()))

    m, got = run(monkeypatch, True, "all", hook=hook)
    L = CFG.num_layers
    assert calls == ["head"] + [f"layer{i}" for i in reversed(range(L))] + ["embed"]
    assert m._engine._wgrad_tables == {}
    for start, end, snap in snaps:
        assert torch.equal(snap, ref[start:end]), (start, end)
    assert torch.equal(got, ref)
