"""The stage audit of one real training step (tests/step_ref.py): every stage of ViTEngine.forward / backward recomputed
in float64 from the engine's own inputs to that stage and the fp32 master weights by name, every output element held to
that stage's derived gate; the worst ratio per stage kind is printed (RATIO <stage> <value>).

The step is driven through VisionTransformer, so the mirror handling is the real one; engine switches are set as
attributes. Shapes are the smallest that still take the production paths (deferral and grouping need D, M >= 256):
  A  image 32, patch 8 (N 17, patch_k 192), D 256, 4 heads (hd 64), M 512, 3 layers, batch 8: T 136 -> Tp 192 (partial
     128- and 256-row tiles), table members 256 x 256 and 256 x 512, the embedding gradient (N 192) on the single form
  B  image 24 x 40, patch 4 (N 61, patch_k 48: the padded wconv), D 320, 4 heads (hd 80), M 640, 2 layers, batch 5
     (T 305, bp 64)
  C  image 72, patch 4 (N 325 > 320: the K/V-tiled attention and its per-block bias partials), D 256, 8 heads (hd 32),
     M 256, 2 layers, batch 2
Every mode runs on A, the first two on B and C, the step after an optimizer update on B as well (the padded wconv
exists only there). The planted wiring errors (A) each produce wrong values only, never an address out of range, go
through the recorder's hooks, and must be named at exactly their stage."""
import functools
from types import SimpleNamespace

import pytest
import torch

import step_ref as S
from oracle.vit_oracle import init_params, tame_params

pytestmark = pytest.mark.gpu
NAN = float("nan")


def _shape(image, patch, D, H, M, L, b):
    gh, gw = image[0] // patch, image[1] // patch
    return SimpleNamespace(image=image, patch=(patch, patch), image_size=image, patch_size=patch, emb_dim=D, num_heads=H,
                           mlp_dim=M, num_layers=L, num_classes=10, num_tokens=gh * gw + 1, b=b)


SHAPES = {"A": _shape((32, 32), 8, 256, 4, 512, 3, 8), "B": _shape((24, 40), 4, 320, 4, 640, 2, 5),
          "C": _shape((72, 72), 4, 256, 8, 256, 2, 2)}


@functools.lru_cache(maxsize=None)
def problem(shape):
    """params, two micro-batches and their labels: made once, shared by every case, never written"""
    s = SHAPES[shape]
    params = tame_params(init_params(s, seed=42))
    g = torch.Generator().manual_seed(21)
    x = torch.randn(2, s.b, 3, *s.image, generator=g)
    y = torch.randint(0, s.num_classes, (2, s.b), generator=g)
    return params, x.cuda(), y.cuda()


def build(shape, dropout=0.0, drop_path=0.0):
    from vitmi.model import VisionTransformer
    s = SHAPES[shape]
    params, x, _ = problem(shape)
    torch.manual_seed(42)
    m = VisionTransformer(image_size=s.image, patch_size=s.patch, emb_dim=s.emb_dim, mlp_dim=s.mlp_dim,
                          num_heads=s.num_heads, num_layers=s.num_layers, num_classes=s.num_classes,
                          attn_dropout_rate=0.0, dropout_rate=dropout, drop_path_rate=drop_path)
    m.load_state_dict(params)
    m = m.cuda()
    m(x[0, :1])  # builds the engine
    return m


def step(m, x, y, rec=None, nan_fill=False):
    from vitmi.model import CrossEntropyLoss
    if rec is not None:
        rec.active = True
    loss = CrossEntropyLoss()(m(x), y)
    if nan_fill:
        assert all(p.grad is None for p in m.parameters())   # an overwriting backward into the engine's buffer
        m._engine.grad.fill_(NAN)
    loss.backward()
    torch.cuda.synchronize()
    if rec is not None:
        rec.active = False


def expected_stages(L, path, pruned):
    """forward 2 (+ the drop-path table) + 7 per layer (+ the cls copy) + 2, the loss, backward 3 (+ the dhb fill) + 7
    per layer (+ the dO fill), one per parameter (8 + 16 L)"""
    return 17 + 30 * L + int(path) + int(pruned)


def recorder(monkeypatch, m, shape):
    from vitmi import ops
    rec = S.Recorder(m._engine, SHAPES[shape].b)
    rec.install(monkeypatch, ops)
    return rec


def check(tr, path=False, pruned=True, expect=()):
    w = S.audit(tr)
    print(w.report())
    assert w.problems == [], w.problems
    assert w.failed == list(expect), w.report()
    assert len(w.stages) == expected_stages(tr.dims.L, path, pruned)
    assert tr.pruned == pruned
    return w


# ---- modes -------------------------------------------------------------------------------------------------------------
SWITCHES = {
    "default": {},
    "full": dict(prune_last=False),
    "defer0_group": dict(wgrad_defer=0, group_wgrad=True),
    "defer0_nogroup": dict(wgrad_defer=0, group_wgrad=False),
    "defer1": dict(wgrad_defer=1),
    "overlap": dict(overlap_wgrad=True),
}


@pytest.mark.parametrize("shape,mode", [("A", k) for k in SWITCHES] + [(s, k) for s in "BC" for k in ("default", "full")])
def test_step_audit(monkeypatch, shape, mode):
    m = build(shape)
    eng = m._engine
    assert eng.wgrad_defer == SHAPES[shape].num_layers and not eng.overlap_wgrad and eng.prune_last and eng.group_wgrad
    for k, v in SWITCHES[mode].items():
        setattr(eng, k, v)
    _, x, y = problem(shape)
    rec = recorder(monkeypatch, m, shape)
    step(m, x[0], y[0], rec, nan_fill=True)
    check(rec.trace(x[0], y[0], nan_filled=True), pruned=mode != "full")
    if shape == "B":
        assert eng.wconv is not None
    if shape == "C":
        assert eng.acts(SHAPES[shape].b).attn_bias_rows == -(-SHAPES[shape].num_tokens // 64)


def test_step_audit_dropout_and_drop_path(monkeypatch):
    m = build("A", dropout=0.1, drop_path=0.5)
    m.train()
    _, x, y = problem("A")
    rec = recorder(monkeypatch, m, "A")
    step(m, x[0], y[0], rec, nan_fill=True)
    tr = rec.trace(x[0], y[0], nan_filled=True)
    tab = m._engine.acts(8).path_scale
    for s, p in enumerate(tr.path):
        if p > 0:
            assert bool((tab[s] == 0).any()) and bool((tab[s] > 0).any()), (s, tab[s])
    assert tr.p_drop > 0 and tr.path[2] > 0
    check(tr, path=True, pruned=False)


def test_step_audit_accumulating_micro_step(monkeypatch):
    """the second micro-step adds into the first one's gradient inside the kernels: gradient = first + audited"""
    m = build("A")
    m.accumulate_in_place = True
    _, x, y = problem("A")
    step(m, x[0], y[0])
    first = m._engine.grad.detach().clone()
    rec = recorder(monkeypatch, m, "A")
    step(m, x[1], y[1], rec)
    check(rec.trace(x[1], y[1], accumulate=True, grad_before=first))


@pytest.mark.parametrize("shape", ["A", "B"])
@pytest.mark.parametrize("which", ["sgd", "adamw"])
def test_step_audit_after_a_fused_optimizer_update(monkeypatch, which, shape):
    """the weights the second forward reads must be bf16(master): a stale mirror, wqkv or wconv (which exists on B
    only) shows per element"""
    from vitmi.optim import SGD, EngineAdamW
    m = build(shape)
    if which == "sgd":
        opt = SGD(m.parameters(), lr=1.0, momentum=0.9, weight_decay=1e-4, model=m)
    else:
        opt = EngineAdamW(m.parameters(), lr=1e-2, model=m)
    params, x, y = problem(shape)
    step(m, x[0], y[0])
    opt.step()
    opt.zero_grad(set_to_none=True)
    torch.cuda.synchronize()
    moved = m._engine.pv("transformer.encoder_layers.0.attn.query.weight").cpu().bfloat16()
    assert not torch.equal(moved, params["transformer.encoder_layers.0.attn.query.weight"].bfloat16())
    rec = recorder(monkeypatch, m, shape)
    step(m, x[1], y[1], rec, nan_fill=True)
    check(rec.trace(x[1], y[1], nan_filled=True))


# ---- planted wiring errors ---------------------------------------------------------------------------------------------
def _lp(i, s):
    return f"transformer.encoder_layers.{i}.{s}"


def test_planted_stale_master_element(monkeypatch):
    m = build("A")
    _, x, y = problem("A")
    rec = recorder(monkeypatch, m, "A")

    def after_refresh(rec, arg):     # the first launch of the forward: the mirror has been made from the old value
        rec.eng.flat[rec.eng.off("embedding.weight") + 1234] += 0.5
    rec.pre_hooks["im2col_hw"] = after_refresh
    step(m, x[0], y[0], rec, nan_fill=True)
    check(rec.trace(x[0], y[0], nan_filled=True), expect=["fwd.h[0]"])


def test_planted_qkv_row_zeroed(monkeypatch):
    m = build("A")
    _, x, y = problem("A")
    rec = recorder(monkeypatch, m, "A")

    def zero_row(rec, arg):
        if arg["C"].data_ptr() == rec.buffer("qkv[1]").data_ptr():
            arg["C"][5].zero_()
    rec.post_hooks["gemm"] = zero_row
    step(m, x[0], y[0], rec, nan_fill=True)
    check(rec.trace(x[0], y[0], nan_filled=True), expect=["fwd.qkv[1]"])


def test_planted_ln2_backward_dropout_site(monkeypatch):
    from vitmi import ops
    m = build("A", dropout=0.1, drop_path=0.5)
    m.train()
    _, x, y = problem("A")
    rec = recorder(monkeypatch, m, "A")

    def shift_site(rec, arg):
        if arg["x"].data_ptr() == rec.buffer("hm[1]").data_ptr():
            d = arg["dx_dropout"]
            arg["dx_dropout"] = ops.dropout_desc(d.p, d.site + 1, d.seed, d.offset, d.row_stride)
    rec.pre_hooks["layernorm_bwd"] = shift_site
    step(m, x[0], y[0], rec, nan_fill=True)
    check(rec.trace(x[0], y[0], nan_filled=True), path=True, pruned=False, expect=["bwd.ln2[1]"])


def test_planted_path_scale_rows_swapped(monkeypatch):
    """between forward and backward; row 1 (layer 0's MLP branch, rate 0: all ones, never read) and row 2 (layer 1's
    attention branch), so the one launch that reads row 2 sees other multipliers"""
    m = build("A", dropout=0.1, drop_path=0.5)
    m.train()
    _, x, y = problem("A")
    rec = recorder(monkeypatch, m, "A")

    def swap(rec, arg):
        if arg["_call"] == 2:      # the first launch of the backward (call 1 made the logits)
            t = rec.buffer("path_scale")
            t[[1, 2]] = t[[2, 1]]
    rec.pre_hooks["gemm_f32"] = swap
    step(m, x[0], y[0], rec, nan_fill=True)
    check(rec.trace(x[0], y[0], nan_filled=True), path=True, pruned=False, expect=["bwd.ln2[1]"])


def test_planted_weight_gradient_k(monkeypatch):
    """K = Tp - 64 = 128 on the embedding weight gradient (the single form): token rows 128..135 are lost"""
    from vitmi._lib import EPI_SPLITK
    m = build("A")
    _, x, y = problem("A")
    rec = recorder(monkeypatch, m, "A")
    hit = []

    def short_k(rec, arg):
        if arg.get("epilogue") == EPI_SPLITK and arg["N"] == 192:
            assert arg["K"] == 192 and arg["split_k"] == 1
            arg["K"] -= 64
            hit.append(1)
    rec.pre_hooks["gemm"] = short_k
    step(m, x[0], y[0], rec, nan_fill=True)
    assert hit == [1]
    check(rec.trace(x[0], y[0], nan_filled=True), expect=["grad.embedding.weight"])


def test_planted_bias_reduction_overwrites(monkeypatch):
    m = build("A")
    m.accumulate_in_place = True
    _, x, y = problem("A")
    step(m, x[0], y[0])
    first = m._engine.grad.detach().clone()
    rec = recorder(monkeypatch, m, "A")
    eng = m._engine
    target = eng.layout.view(eng.grad, _lp(1, "mlp.fc1.bias")).data_ptr()
    hit = []

    def overwrite(rec, arg):
        jobs = list(arg["jobs"])
        for k, (inp, rows, cols, ld, seg, outs, acc) in enumerate(jobs):
            if outs[0].data_ptr() == target:
                assert acc
                jobs[k] = (inp, rows, cols, ld, seg, outs, False)
                hit.append(1)
        arg["jobs"] = jobs
    rec.pre_hooks["colsum_batch"] = overwrite
    step(m, x[1], y[1], rec)
    assert hit == [1]
    check(rec.trace(x[1], y[1], accumulate=True, grad_before=first), expect=["grad.mlp.fc1.bias[1]"])
