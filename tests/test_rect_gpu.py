"""Rectangular images and patches on the GPU: vit_im2col_hw / _f32 bit-exact against torch's unfold, the training
step of rectangular models against the CPU oracle (oracle.vit_oracle reads only emb_dim / num_layers / patch_size
from its config, the latter as the conv stride, so a duck-typed config with patch_size=(fh, fw) runs the
reference arithmetic on any [b, 3, H, W]), HF.patch_embed against F.conv2d, the Res-ViT fused token embedding
against its per-op path, and a square checkpoint loaded through resize_pos_embedding.

Tolerances are tests/test_parity_gpu.py's (bf16 operands, fp32 accumulation): logits relative Frobenius error
< 1e-2, loss within 1e-3 relative, gradients 3e-2 per parameter (near-zero gradients: 1e-3 x the global norm);
the fp32 forward within 1e-3."""
import math
from types import SimpleNamespace

import pytest
import torch

from oracle.vit_oracle import loss_and_grads, tame_params

pytestmark = pytest.mark.gpu
DEV = "cuda"


def rel(a, b):
    a = torch.as_tensor(a).detach().double().cpu()
    b = torch.as_tensor(b).detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def check_grads(model, ref_grads):
    tot = math.sqrt(sum(float(g.double().norm()) ** 2 for g in ref_grads.values()))
    named = dict(model.named_parameters())
    for k, g in ref_grads.items():
        mine = named[k].grad
        assert mine is not None, k
        gn = float(g.double().norm())
        if k.endswith("attn.key.bias") or gn < 1e-4 * tot:
            assert float((mine.double().cpu() - g.double()).norm()) <= 1e-3 * tot, k
        else:
            assert rel(mine, g) < 3e-2, (k, rel(mine, g))


# ---- im2col ---------------------------------------------------------------------------------------------
def _im2col_ref(x, Ph, Pw, Kpad):
    B, _, H, W = x.shape
    gh, gw = H // Ph, W // Pw
    K = 3 * Ph * Pw
    cols = x.unfold(2, Ph, Ph).unfold(3, Pw, Pw)  # B,3,gh,gw,Ph,Pw
    cols = cols.permute(0, 2, 3, 1, 4, 5).reshape(B, gh * gw, K)
    ref = torch.zeros(B, gh * gw + 1, Kpad, device=x.device)
    ref[:, 1:, :K] = cols
    return ref.reshape(B * (gh * gw + 1), Kpad)


IM2COL_CASES = [
    (16, 40, 8, 8, 192, False),   # vector form, wide grid 2x5
    (40, 16, 8, 8, 192, False),   # vector form, tall grid
    (32, 16, 4, 8, 128, False),   # pad columns, Ph != Pw
    (16, 40, 8, 4, 128, False),   # Pw % 8 != 0: scalar form
    (18, 43, 4, 8, 128, False),   # W % 4 != 0 and a floor in both directions (grid 4x5): scalar form
    (28, 42, 14, 14, 640, False),  # the H/14 patch
    (16, 40, 8, 8, 192, True),    # x one float into its storage (not 16-B aligned): scalar form
]


@pytest.mark.parametrize("bf16", [True, False], ids=["bf16", "f32"])
@pytest.mark.parametrize("H,W,Ph,Pw,Kpad,offset", IM2COL_CASES)
def test_im2col_hw_bit_exact(H, W, Ph, Pw, Kpad, offset, bf16):
    from vitmi import ops
    B = 2
    torch.manual_seed(H * 100 + W)
    if offset:
        x = torch.randn(B * 3 * H * W + 1, device=DEV)[1:].view(B, 3, H, W)
        assert x.data_ptr() % 16 == 4 and x.is_contiguous()
    else:
        x = torch.randn(B, 3, H, W, device=DEV)
    N = (H // Ph) * (W // Pw) + 1
    out = torch.full((B * N, Kpad), float("nan"), device=DEV, dtype=torch.bfloat16 if bf16 else torch.float32)
    (ops.im2col_hw if bf16 else ops.im2col_hw_f32)(x, out, B, H, W, Ph, Pw, Kpad)
    ref = _im2col_ref(x, Ph, Pw, Kpad)
    if bf16:
        ref = ref.bfloat16()
    assert torch.equal(out, ref)  # (NaN anywhere — an unwritten cls row or pad column — compares unequal)


@pytest.mark.parametrize("img,P,Kpad", [(32, 8, 192), (28, 14, 640), (30, 4, 64)])
def test_im2col_hw_equals_square_entry_points(img, P, Kpad):
    from vitmi import ops
    B = 2
    x = torch.randn(B, 3, img, img, device=DEV)
    N = (img // P) ** 2 + 1
    for dt, old, new in ((torch.bfloat16, ops.im2col, ops.im2col_hw), (torch.float32, ops.im2col_f32, ops.im2col_hw_f32)):
        a = torch.full((B * N, Kpad), float("nan"), device=DEV, dtype=dt)
        b = torch.full((B * N, Kpad), float("nan"), device=DEV, dtype=dt)
        old(x, a, B, img, P, Kpad)
        new(x, b, B, img, img, P, P, Kpad)
        assert torch.equal(a, b)


def test_im2col_hw_bad_arguments_launch_nothing():
    from vitmi import ops
    from vitmi._lib import VitHipError
    x = torch.randn(2, 3, 16, 40, device=DEV)
    for fn, dt in ((ops.im2col_hw, torch.bfloat16), (ops.im2col_hw_f32, torch.float32)):
        out = torch.full((2 * 11, 192), float("nan"), device=DEV, dtype=dt)
        with pytest.raises(VitHipError):
            fn(x, out, 2, 4, 40, 8, 8, 192)    # H < Ph
        with pytest.raises(VitHipError):
            fn(x, out, 2, 16, 4, 8, 8, 192)    # W < Pw
        with pytest.raises(VitHipError):
            fn(x, out, 2, 16, 40, 8, 8, 128)   # Kpad < 3 Ph Pw
        with pytest.raises(VitHipError):
            fn(None, out, 2, 16, 40, 8, 8, 192)
        torch.cuda.synchronize()
        assert torch.isnan(out).all()


# ---- the training step against the oracle ---------------------------------------------------------------
def _cfg(image, patch, D, M, heads=2, layers=2):
    return SimpleNamespace(image_size=image, patch_size=patch, emb_dim=D, mlp_dim=M, num_heads=heads, num_layers=layers,
                           num_classes=10)


CASES = {
    "A": (_cfg((16, 32), (8, 8), 64, 128), 4, 9),      # basic rectangular grid
    "B": (_cfg((32, 16), (4, 8), 128, 256), 3, 17),    # rectangular patch; embedding weight gradient with K = 96
    "C": (_cfg((18, 43), (4, 8), 64, 128), 3, 21),     # floors; scalar im2col inside the engine
    "D": (_cfg((56, 96), (4, 4), 128, 256), 2, 337),   # > 320 tokens: the K/V-tiled attention path
}
_STEP = {}


def _model(cfg, seed=42):
    from vitmi.model import VisionTransformer
    torch.manual_seed(seed)
    return VisionTransformer(image_size=cfg.image_size, patch_size=cfg.patch_size, emb_dim=cfg.emb_dim,
                             mlp_dim=cfg.mlp_dim, num_heads=cfg.num_heads, num_layers=cfg.num_layers,
                             num_classes=cfg.num_classes, attn_dropout_rate=0.0, dropout_rate=0.0)


def _oracle_step(case):
    """(cfg, params, x, y, oracle logits / loss / grads) of a case, computed once"""
    if case not in _STEP:
        cfg, bs, tokens = CASES[case]
        params = tame_params(_model(cfg).state_dict())  # the model's own seeded construction, tamed
        g = torch.Generator().manual_seed(5)
        x = torch.randn(bs, 3, *cfg.image_size, generator=g)
        y = torch.randint(0, cfg.num_classes, (bs,), generator=g)
        assert params["transformer.pos_embedding.pos_embedding"].shape[1] == tokens
        _STEP[case] = (cfg, params, x, y, loss_and_grads(params, x, y, cfg))
    return _STEP[case]


@pytest.mark.parametrize("case", sorted(CASES))
def test_rect_step_matches_oracle(case):
    from vitmi.model import CrossEntropyLoss
    cfg, params, x, y, (ref_logits, ref_loss, ref_grads) = _oracle_step(case)
    m = _model(cfg)
    m.load_state_dict(params)
    m = m.cuda()
    logits = m(x.cuda())
    loss = CrossEntropyLoss()(logits, y.cuda())
    loss.backward()
    print(f"case {case}: logits rel {rel(logits, ref_logits):.3e}, loss {float(loss.detach()):.6f} vs {float(ref_loss):.6f}")
    assert rel(logits, ref_logits) < 1e-2
    assert abs(float(loss.detach()) - float(ref_loss)) <= 1e-3 * abs(float(ref_loss))
    check_grads(m, ref_grads)


def test_rect_exact_forward_logits_within_1e3():
    cfg, params, x, y, (ref_logits, _, _) = _oracle_step("B")
    m = _model(cfg)
    m.load_state_dict(params)
    m = m.cuda()
    m.precision = "fp32"
    with torch.no_grad():
        logits = m(x.cuda())
    assert rel(logits, ref_logits) < 1e-3, rel(logits, ref_logits)


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_transposed_batch_is_refused(precision):
    """[b, 3, 32, 16] has the token count of a (16, 32) model: it must raise, not run"""
    m = _model(CASES["A"][0]).cuda()
    m.precision = precision
    with torch.no_grad():
        with pytest.raises(ValueError):
            m(torch.randn(2, 3, 32, 16, device=DEV))
        assert m(torch.randn(2, 3, 16, 32, device=DEV)).shape == (2, 10)


# ---- HF.patch_embed -------------------------------------------------------------------------------------
def test_patch_embed_rectangular_matches_conv2d():
    """16x40 images, patches (8, 4), against F.conv2d in f32: output 1e-2, weight / bias gradients 3e-2 (the bf16
    GEMM tolerances of tests/test_submodules_gpu.py)"""
    from vitmi import functional as HF
    torch.manual_seed(2)
    B, D, H, W, fh, fw = 3, 64, 16, 40, 8, 4
    x = torch.randn(B, 3, H, W, device=DEV)
    w = (torch.randn(D, 3, fh, fw, device=DEV) / math.sqrt(3 * fh * fw)).requires_grad_(True)
    b = (0.1 * torch.randn(D, device=DEV)).requires_grad_(True)
    gy = torch.randn(B, (H // fh) * (W // fw), D, device=DEV)
    y = HF.patch_embed(x, w, b, (fh, fw))
    (y * gy).sum().backward()
    wr, br = w.detach().clone().requires_grad_(True), b.detach().clone().requires_grad_(True)
    yr = torch.nn.functional.conv2d(x, wr, br, stride=(fh, fw)).flatten(2).transpose(1, 2)  # b (h w) c
    (yr * gy).sum().backward()
    assert y.shape == yr.shape == (B, 20, D)
    assert rel(y, yr) < 1e-2, rel(y, yr)
    assert rel(w.grad, wr.grad) < 3e-2, rel(w.grad, wr.grad)
    assert rel(b.grad, br.grad) < 3e-2, rel(b.grad, br.grad)
    # an int patch is the square pair
    with torch.no_grad():
        w8 = torch.randn(D, 3, 8, 8, device=DEV)
        assert torch.equal(HF.patch_embed(x, w8, b, 8), HF.patch_embed(x, w8, b, (8, 8)))


# ---- Res-ViT --------------------------------------------------------------------------------------------
def test_resvit_embed_tokens_matches_per_op_rectangular():
    """tests/test_resvit_gpu.py::test_embed_tokens_matches_per_op at a 16x32 image with patch (8, 8)"""
    from vitmi import resvit
    from vitmi import resvit_fused as rf
    torch.manual_seed(11)
    args = resvit.ModelArgs(dim=128, mlp_dim=256, n_layers=1, n_heads=2, n_kv_heads=2, lora_rank=4, use_lora=True,
                            use_reslr=False, image_size=(16, 32), patch_size=(8, 8), num_classes=10)
    m = resvit.Transformer(args).cuda()
    assert not m.embedding.weight.requires_grad and m.cls_token.requires_grad
    x = torch.randn(3, 3, 16, 32, device=DEV)
    assert rf.embed_supported(m, x)
    assert not rf.embed_supported(m, torch.randn(3, 3, 20, 32, device=DEV))  # 20 rows: no whole number of patches
    w = torch.randn(3, 2 * 4 + 1, 128, device=DEV)
    outs = []
    for fused in (False, True):
        m.cls_token.grad = None
        if fused:
            t = rf.embed_tokens(m, x)
        else:
            t = m.embed(x)
            t = torch.cat([m.cls_token.expand(t.shape[0], 1, -1), t], dim=1)
            t = m.pos_embedding(t)
        (t * w).sum().backward()
        outs.append((t.detach(), m.cls_token.grad.clone()))
    (t0, g0), (t1, g1) = outs
    assert t1.shape == t0.shape == (3, 9, 128)
    assert torch.equal(t1[:, 0], t0[:, 0])
    assert rel(t1, t0) < 1e-5
    assert rel(g1, g0) < 1e-6


# ---- checkpoint round trip ------------------------------------------------------------------------------
def test_square_checkpoint_into_rectangular_model():
    from vitmi.checkpoint import resize_pos_embedding
    sq = _model(_cfg((32, 32), (8, 8), 64, 128), seed=3)
    sd = tame_params(sq.state_dict())
    rect = _model(CASES["A"][0])
    rect.load_state_dict(resize_pos_embedding(sd, (2, 4)), strict=True)
    rect = rect.cuda()
    with torch.no_grad():
        logits = rect(torch.randn(2, 3, 16, 32, device=DEV))
    assert logits.shape == (2, 10) and torch.isfinite(logits).all()
