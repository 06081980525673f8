"""Gradient accumulation over micro-batches, from the engine up to the training loop, and norm clipping in vitmi.optim.SGD.

Config (test_wgrad_deferred_gpu's): D = 256, 4 heads, MLP 512, 3 layers, 32-px images in 8-px patches (17 tokens),
batch 8, tamed seed-42 parameters. Every layer's four weight gradients are table members, at split 1 (K = the padded
token rows: 3 k-tiles at most, so the cost model has no other split; the bitwise tests also force it), and the padded
rows are no multiple of 64 (micro-batches of 4, 3 and 2 images: 68, 51 and 34 token rows).
"""
import functools
from collections import OrderedDict

import pytest
import torch

from oracle.vit_oracle import OneCycle, ViTConfig, init_params, loss_and_grads, sgd_step, tame_params
from test_parity_gpu import check_grads, make_model, rel

pytestmark = pytest.mark.gpu

CFG = ViTConfig(image_size=32, patch_size=8, emb_dim=256, mlp_dim=512, num_heads=4, num_layers=3, num_classes=10)
BS = 8
L = CFG.num_layers


@functools.lru_cache(maxsize=None)
def problem():
    """params, two batches (x, y) and the oracle's full-batch gradients of the first: computed once, never written"""
    params = tame_params(init_params(CFG, seed=42))
    g = torch.Generator().manual_seed(21)
    x = torch.randn(2 * BS, 3, CFG.image_size, CFG.image_size, generator=g)
    y = torch.randint(0, CFG.num_classes, (2 * BS,), generator=g)
    _, _, ref_grads = loss_and_grads(params, x[:BS], y[:BS], CFG)
    return params, x.cuda(), y.cuda(), ref_grads


def force_split_1(monkeypatch):
    from vitmi import ops
    monkeypatch.setattr(ops, "splitk_factor", lambda *a, **k: 1)
    monkeypatch.setattr(ops, "splitk_factor_group", lambda *a, **k: 1)


def model(monkeypatch, defer="all", prune=True):
    params, x, _, _ = problem()
    monkeypatch.setenv("VITMI_WGRAD_DEFER", defer)
    m = make_model(CFG, params)
    m(x[:1])  # builds the engine (which reads the knob) and its bf16 mirror
    m._engine.prune_last = prune
    return m


def cuts(sizes):
    o, out = 0, []
    for b in sizes:
        out.append(slice(o, o + b))
        o += b
    return out


def engine_backward(eng, sl, accumulate):
    """forward + fused cross-entropy + backward of the images `sl` of batch 0, each sample weighted 1 / BS"""
    _, x, y, _ = problem()
    eng.forward(x[sl])
    dl, _ = eng.cross_entropy(y[sl], grad_scale=1.0 / BS)
    if accumulate:
        eng.backward(dl, eng.grad, accumulate=True)
    else:
        eng.backward(dl)
    torch.cuda.synchronize()
    return eng.grad.detach().clone()


# ---- 1. bitwise: accumulate adds exactly the overwriting backward's gradient -------------------------------------
@pytest.mark.parametrize("sizes", [(4, 4), (3, 3, 2)], ids=["4+4", "3+3+2"])
@pytest.mark.parametrize("hook", [False, True], ids=["deferred", "hooked"])
@pytest.mark.parametrize("prune", [False, True], ids=["full", "pruned"])
@pytest.mark.parametrize("defer", ["0", "all"])
def test_accumulated_gradient_is_the_sum_bit_for_bit(monkeypatch, defer, prune, hook, sizes):
    """G = backward(A), then backward(B, accumulate) ... against G0 + g (+ g2): every producer adds its finished f32
    value once, so the whole flat buffer, alignment padding included, is equal. `hooked`: a grad_ready_hook is set,
    so the per-layer path runs and accumulates through the reductions' flag."""
    force_split_1(monkeypatch)
    eng = model(monkeypatch, defer, prune)._engine
    calls = []
    if hook:
        eng.grad_ready_hook = lambda g, name, s, e, evs: calls.append(name)
    parts = [engine_backward(eng, sl, False) for sl in cuts(sizes)]
    assert all(float(p.abs().max()) > 0 for p in parts)
    want = parts[0]
    for p in parts[1:]:
        want = want + p
    got = None
    for i, sl in enumerate(cuts(sizes)):
        got = engine_backward(eng, sl, i > 0)
    assert torch.equal(got, want), (int((got != want).sum()), float((got - want).abs().max()))
    deferred = defer == "all" and not hook
    assert bool(eng._wgrad_tables) == deferred
    if deferred:  # the accumulating backwards ran the table launch with accumulating members
        assert any(len(slot) == 3 and slot[1] is True for slot, _ in eng._wgrad_tables)
    assert len(calls) == (2 * len(sizes) * (L + 2) if hook else 0)


def test_overlap_stream_accumulates_too(monkeypatch):
    force_split_1(monkeypatch)
    monkeypatch.setenv("VITMI_OVERLAP", "1")
    eng = model(monkeypatch)._engine
    assert eng.overlap_wgrad
    a, b = cuts((4, 4))
    want = engine_backward(eng, a, False) + engine_backward(eng, b, False)
    engine_backward(eng, a, False)
    assert torch.equal(engine_backward(eng, b, True), want)


# ---- 2. / 3. the model's two accumulation paths against the oracle -----------------------------------------------
def micro_backwards(m, sizes):
    from vitmi.model import CrossEntropyLoss
    _, x, y, _ = problem()
    crit = CrossEntropyLoss()
    m.zero_grad()
    for sl in cuts(sizes):
        (crit(m(x[sl]), y[sl]) * ((sl.stop - sl.start) / BS)).backward()
    torch.cuda.synchronize()


def is_engine_view(m):
    eng = m._engine
    return all(p.grad is not None and p.grad.data_ptr() == eng.layout.view(eng.grad, n).data_ptr()
               for n, p in zip(m._flat_names, m._flat_params))


@pytest.mark.parametrize("sizes", [(4, 4), (3, 3, 2)], ids=["4+4", "3+3+2"])
def test_in_place_accumulation_passes_the_oracle_gate(monkeypatch, sizes):
    m = model(monkeypatch)
    m.accumulate_in_place = True
    micro_backwards(m, sizes)
    check_grads(m, problem()[3])
    assert is_engine_view(m) and m._scratch is None


def test_default_path_is_unchanged(monkeypatch):
    """accumulate_in_place off: the second backward goes through the scratch buffer and autograd's adds"""
    m = model(monkeypatch)
    assert m.accumulate_in_place is False
    micro_backwards(m, (4, 4))
    assert m._scratch is not None
    check_grads(m, problem()[3])


def test_in_place_falls_back_when_a_grad_is_not_the_engine_view(monkeypatch):
    m = model(monkeypatch)
    m.accumulate_in_place = True
    m.zero_grad()
    for p in m.parameters():
        p.grad = torch.zeros_like(p)
    from vitmi.model import CrossEntropyLoss
    _, x, y, _ = problem()
    for sl in cuts((4, 4)):
        (CrossEntropyLoss()(m(x[sl]), y[sl]) * 0.5).backward()
    assert m._scratch is not None and not is_engine_view(m)
    check_grads(m, problem()[3])


# ---- 4. prepared tables: one overwrite set and one accumulate set ------------------------------------------------
@pytest.mark.parametrize("defer,launches", [("all", 1), ("1", L)])
def test_tables_are_prepared_once_per_flag(monkeypatch, defer, launches):
    from vitmi import ops
    from vitmi.optim import SGD
    built = []

    class Counting(ops.GemmGroupTable):
        def __init__(self, members):
            built.append(len(members))
            super().__init__(members)

    monkeypatch.setattr(ops, "GemmGroupTable", Counting)
    m = model(monkeypatch, defer)
    m.accumulate_in_place = True
    opt = SGD(m.parameters(), lr=0.01, momentum=0.9, model=m)
    for step in range(3):
        micro_backwards(m, (2, 2, 2))  # K = 3 micro-batches of 2 images
        opt.step()
        assert len(built) == (2 * launches), (step, built)
    assert is_engine_view(m)


# ---- 5. no_sync ------------------------------------------------------------------------------------------------------
def test_no_sync_defers_the_hook_to_the_last_micro_step(monkeypatch):
    from vitmi.model import CrossEntropyLoss
    force_split_1(monkeypatch)
    _, x, y, _ = problem()
    ref = model(monkeypatch)
    ref.accumulate_in_place = True
    micro_backwards(ref, (3, 3, 2))
    want = ref._engine.grad.detach().clone()

    m = model(monkeypatch)
    m.accumulate_in_place = True
    eng = m._engine
    calls, snaps, finished = [], [], []

    def hook(g, name, start, end, events):
        calls.append(name)
        snaps.append((start, end, g[start:end].clone()))

    finish = lambda: finished.append(len(calls))
    eng.grad_ready_hook, eng.grad_ready_finish = hook, finish
    crit = CrossEntropyLoss()
    m.zero_grad()
    sls = cuts((3, 3, 2))
    for sl in sls[:-1]:
        with m.no_sync():
            assert eng.grad_ready_hook is None and eng.grad_ready_finish is None
            (crit(m(x[sl]), y[sl]) * ((sl.stop - sl.start) / BS)).backward()
        assert eng.grad_ready_hook is hook and eng.grad_ready_finish is finish
    assert calls == [] and finished == []
    sl = sls[-1]
    (crit(m(x[sl]), y[sl]) * ((sl.stop - sl.start) / BS)).backward()
    torch.cuda.synchronize()
    assert calls == ["head"] + [f"layer{i}" for i in reversed(range(L))] + ["embed"]
    assert finished == [L + 2]
    for start, end, snap in snaps:  # every bucket complete, and accumulated, when its hook ran
        assert torch.equal(snap, want[start:end]), (start, end)
    assert torch.equal(eng.grad, want)
    with pytest.raises(KeyError):
        with m.no_sync():
            raise KeyError("body")
    assert eng.grad_ready_hook is hook and eng.grad_ready_finish is finish


# ---- 6. the training loop ------------------------------------------------------------------------------------------
def test_train_epoch_accumulating_follows_the_oracle_trajectory(monkeypatch):
    """two optimizer steps of SGD + OneCycle through train_epoch(accum_steps=2) over four micro-batches of 4 images,
    against the oracle's sgd_step / OneCycle on the two full batches of 8: test_engine_fused_step_matches_oracle_sgd's
    gate on the updates (relative 3e-2 per tensor, its skips)"""
    from vitmi import train
    from vitmi.model import CrossEntropyLoss
    from vitmi.optim import SGD
    params, x, y, _ = problem()
    m = model(monkeypatch)
    m.accumulate_in_place = True
    m.train()
    opt = SGD(m.parameters(), lr=0.05, momentum=0.9, weight_decay=1e-4, model=m)
    sched = torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=0.05, pct_start=0.2, total_steps=10)
    loader = [(x[s:s + 4], y[s:s + 4]) for s in range(0, 2 * BS, 4)]
    metrics = train.MetricTracker("loss", "acc1", "acc5")
    out = train.train_epoch(1, m, loader, CrossEntropyLoss(), opt, sched, metrics, torch.device("cuda"),
                            accum_steps=2)
    torch.cuda.synchronize()
    assert sched.last_epoch == 2 and metrics._count["loss"] == 2
    assert is_engine_view(m) and m._scratch is None

    ref = OrderedDict((k, v.clone()) for k, v in params.items())
    bufs, oc, losses = {}, OneCycle(0.05, 10, 0.2), []
    for step in range(2):
        lr, mom = oc.at(step)
        sl = slice(step * BS, (step + 1) * BS)
        _, rloss, rgrads = loss_and_grads(ref, x[sl].cpu(), y[sl].cpu(), CFG)
        losses.append(float(rloss))
        ref, bufs = sgd_step(ref, rgrads, bufs, lr, mom, 1e-4, first=(step == 0))
    assert abs(out["loss"] - sum(losses) / 2) <= 1e-3 * sum(losses) / 2
    st = m._engine.state()
    for k in ref:
        upd_ref = ref[k].double() - params[k].double()
        upd = st[k].double().cpu().reshape(upd_ref.shape) - params[k].double()
        if k.endswith("attn.key.bias") or float(upd_ref.norm()) < 1e-6:
            continue
        assert rel(upd, upd_ref) < 3e-2, (k, rel(upd, upd_ref))


# ---- 7. norm clipping ----------------------------------------------------------------------------------------------
def stepped(monkeypatch, max_norm_of):
    """one full-batch backward, then SGD.step() with max_grad_norm = max_norm_of(float64 norm); returns what the
    checks need"""
    from vitmi.optim import SGD
    m = model(monkeypatch)
    micro_backwards(m, (BS,))
    eng = m._engine
    g0, p0 = eng.grad.detach().clone(), eng.flat.detach().clone()
    n64 = float(g0.double().cpu().norm())
    mx = max_norm_of(n64)
    opt = SGD(m.parameters(), lr=0.1, momentum=0.9, weight_decay=1e-4, model=m, max_grad_norm=mx)
    opt.step()
    torch.cuda.synchronize()
    return m, opt, g0, p0, n64


def test_clip_scales_the_gradient_and_the_update(monkeypatch):
    m, opt, g0, p0, n64 = stepped(monkeypatch, lambda n: 0.5 * n)
    eng = m._engine
    norm, coef = (float(v) for v in opt.last_norm.double().cpu())
    assert abs(norm - n64) <= 1e-6 * n64, (norm, n64)
    assert abs(coef - 0.5 * n64 / (n64 + 1e-6)) <= 1e-6, coef
    g64 = g0.double() * coef
    # .grad is left clipped: the old gradient times the f32 coefficient, one f32 rounding
    assert bool(((eng.grad.double() - g64).abs() <= 2.0 ** -24 * g64.abs() + 1e-45).all())
    assert is_engine_view(m)
    # first step: buf = d = coef g + wd p, p <- p - lr d; four f32 roundings (coef g, wd p, their sum, the update)
    d = g64 + 1e-4 * p0.double()
    want = p0.double() - 0.1 * d
    bound = 2.0 ** -22 * (p0.double().abs() + 0.1 * d.abs())
    err = (eng.flat.double() - want).abs()
    assert bool((err <= bound).all()), float((err - bound).max())
    assert float((eng.flat - p0).abs().max()) > 0


def test_clip_above_the_norm_changes_nothing(monkeypatch):
    m1, opt1, _, _, n64 = stepped(monkeypatch, lambda n: 2.0 * n)
    m0, _, _, _, _ = stepped(monkeypatch, lambda n: None)
    assert float(opt1.last_norm[1]) == 1.0
    assert torch.equal(m1._engine.flat, m0._engine.flat) and torch.equal(m1._engine.grad, m0._engine.grad)


def test_clip_off_the_fast_path_is_refused(monkeypatch):
    from vitmi.optim import SGD
    m = model(monkeypatch)
    micro_backwards(m, (BS,))
    opt = SGD(list(m.parameters())[:3], lr=0.1, model=m, max_grad_norm=1.0)
    with pytest.raises(NotImplementedError, match="fast path"):
        opt.step()
