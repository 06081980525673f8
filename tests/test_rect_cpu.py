"""Rectangular images and patches, host side (no GPU): constructors and their RNG order (reference
src/model.py:173-181, res-vit/model.py ModelArgs), ArchConfig geometry, the position-table resampling of
vitmi.checkpoint.resize_pos_embedding against a float64 evaluation of its closed form, and --image-size HxW."""
import math

import numpy as np
import pytest
import torch

RECTS = [((16, 32), (8, 8)), ((32, 16), (4, 8))]
ARCH = dict(emb_dim=64, mlp_dim=128, num_heads=2, num_layers=1, num_classes=10)
RESVIT = dict(dim=64, mlp_dim=128, n_layers=2, n_heads=2, n_kv_heads=2, norm_eps=1e-5, lora_rank=4,
              dynamic_active_target=0.4, dynamic_start_layer=1, dynamic_router_hdim=32, dynamic_reserve_initials=1,
              low_rank_dim=16, block_size=2, use_lora=True, use_reslr=True, num_classes=10, device="cpu")
KEY = "transformer.pos_embedding.pos_embedding"


# ---- construction ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("image,patch", RECTS)
def test_vit_constructs_rectangular(image, patch):
    from vitmi.model import VisionTransformer
    (h, w), (fh, fw) = image, patch
    m = VisionTransformer(image_size=image, patch_size=patch, **ARCH)
    n = (h // fh) * (w // fw) + 1
    assert m.embedding.weight.shape == (64, 3, fh, fw)
    assert m.transformer.pos_embedding.pos_embedding.shape == (1, n, 64)
    assert m.arch.image_hw == image and m.arch.patch_hw == patch and m.arch.tokens == n
    assert m.arch.patch_k == 3 * fh * fw


def test_vit_square_builds_int_config():
    """square models keep the ArchConfig values they always built"""
    from vitmi.engine import ArchConfig
    from vitmi.model import VisionTransformer
    m = VisionTransformer(image_size=(32, 32), patch_size=(8, 8), **ARCH)
    assert m.arch == ArchConfig(image_size=32, patch_size=8, **ARCH)
    assert m.arch.image_size == 32 and m.arch.patch_size == 8


@pytest.mark.parametrize("image,patch", RECTS)
def test_resvit_constructs_rectangular(image, patch):
    from vitmi import resvit
    (h, w), (fh, fw) = image, patch
    m = resvit.Transformer(resvit.ModelArgs(image_size=image, patch_size=patch, **RESVIT))
    assert m.embedding.weight.shape == (64, 3, fh, fw)
    assert m.pos_embedding.pos_embedding.shape == (1, (h // fh) * (w // fw) + 1, 64)
    assert m.patch == (fh if fh == fw else (fh, fw))


@pytest.mark.parametrize("image,patch", RECTS)
def test_vit_seeded_parity_with_reference_order(image, patch):
    """the reference draws nn.Conv2d(3, D, (fh, fw), (fh, fw)), then randn(1, N, D) (src/model.py:179-183, :10)"""
    from vitmi.model import VisionTransformer
    (h, w), (fh, fw) = image, patch
    n = (h // fh) * (w // fw) + 1
    torch.manual_seed(7)
    conv = torch.nn.Conv2d(3, 64, kernel_size=(fh, fw), stride=(fh, fw))
    pos = torch.randn(1, n, 64)
    torch.manual_seed(7)
    m = VisionTransformer(image_size=image, patch_size=patch, **ARCH)
    assert torch.equal(m.embedding.weight, conv.weight)
    assert torch.equal(m.embedding.bias, conv.bias)
    assert torch.equal(m.transformer.pos_embedding.pos_embedding, pos)


# ---- ArchConfig -----------------------------------------------------------------------------------------
def test_arch_config_geometry():
    from vitmi.engine import ArchConfig, flat_param_specs
    sq = ArchConfig(image_size=32, patch_size=8, **ARCH)
    pair = ArchConfig(image_size=(32, 32), patch_size=(8, 8), **ARCH)
    assert sq == sq and hash(sq) == hash(ArchConfig(image_size=32, patch_size=8, **ARCH))
    assert (sq.tokens, sq.patch_k) == (pair.tokens, pair.patch_k) == (17, 192)
    assert sq.grid == 4 and pair.grid == 4
    assert sq.image_hw == (32, 32) and sq.patch_hw == (8, 8) and sq.grid_hw == (4, 4)
    rect = ArchConfig(image_size=(16, 32), patch_size=(8, 8), **ARCH)
    assert rect.grid_hw == (2, 4) and rect.tokens == 9 and rect.patch_k == 192
    with pytest.raises(ValueError):
        rect.grid
    assert hash(ArchConfig(image_size=[16, 32], patch_size=[8, 8], **ARCH)) == hash(rect)
    floor = ArchConfig(image_size=(18, 43), patch_size=(4, 8), **ARCH)
    assert floor.grid_hw == (4, 5) and floor.tokens == 21 and floor.patch_k == 96
    specs = dict(flat_param_specs(floor))
    assert specs["embedding.weight"] == (64, 3, 4, 8)
    assert specs["transformer.pos_embedding.pos_embedding"] == (1, 21, 64)
    assert dict(flat_param_specs(sq))["embedding.weight"] == (64, 3, 8, 8)


# ---- resize_pos_embedding -------------------------------------------------------------------------------
def _closed_form(table, old, new):
    """float64 numpy evaluation of the separable half-pixel bilinear resampling"""
    (gh, gw), (nh, nw) = old, new
    t = table.astype(np.float64)
    grid = t[0, 1:].reshape(gh, gw, -1)

    def axis(a, g, gn, ax):
        s = np.clip((np.arange(gn) + 0.5) * g / gn - 0.5, 0, g - 1)
        i0 = np.floor(s).astype(np.int64)
        i1 = np.minimum(i0 + 1, g - 1)
        wgt = (s - i0).reshape([-1 if d == ax else 1 for d in range(a.ndim)])
        return np.take(a, i0, axis=ax) * (1 - wgt) + np.take(a, i1, axis=ax) * wgt

    out = axis(axis(grid, gh, nh, 0), gw, nw, 1)
    return np.concatenate([t[:, :1], out.reshape(1, nh * nw, -1)], axis=1)


def _table(gh, gw, d=16, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(1, gh * gw + 1, d, generator=g)


def test_resize_same_grid_is_bit_identical():
    from vitmi.checkpoint import resize_pos_embedding
    sd = {KEY: _table(4, 4), "cls_token": torch.zeros(1, 1, 16)}
    out = resize_pos_embedding(sd, (4, 4))
    assert out is not sd and torch.equal(out[KEY], sd[KEY]) and out["cls_token"] is sd["cls_token"]
    rect = {KEY: _table(2, 8)}
    assert torch.equal(resize_pos_embedding(rect, (2, 8), old_grid=(2, 8))[KEY], rect[KEY])


@pytest.mark.parametrize("old,new", [((14, 14), (14, 24)), ((4, 4), (6, 3))])
def test_resize_matches_closed_form(old, new):
    from vitmi.checkpoint import resize_pos_embedding
    sd = {KEY: _table(*old, seed=3)}
    out = resize_pos_embedding(sd, new)[KEY]
    assert out.shape == (1, new[0] * new[1] + 1, 16) and out.dtype == torch.float32
    ref = _closed_form(sd[KEY].numpy(), old, new)
    err = float(np.abs(out.numpy().astype(np.float64) - ref).max())
    bound = 1e-5 * float(sd[KEY].abs().max())  # f32 rounding over a handful of operations
    print(f"resize {old}->{new}: max abs err {err:.3e}, bound {bound:.3e}")
    assert err <= bound
    assert torch.equal(out[:, 0], sd[KEY][:, 0])  # the cls row is copied
    assert sd[KEY].shape[1] == old[0] * old[1] + 1  # the input dict is left alone


def test_resize_constant_table_stays_constant_and_custom_key():
    from vitmi.checkpoint import resize_pos_embedding
    t = torch.full((1, 17, 8), 0.37)
    t[:, 0] = -2.0
    out = resize_pos_embedding({"pos_embedding.pos_embedding": t}, (3, 7), key="pos_embedding.pos_embedding")
    out = out["pos_embedding.pos_embedding"]
    assert out.shape == (1, 22, 8)
    assert torch.equal(out[:, 1:], torch.full((1, 21, 8), 0.37)) and torch.equal(out[:, 0], t[:, 0])


def test_resize_rejects_bad_grids():
    from vitmi.checkpoint import resize_pos_embedding
    with pytest.raises(ValueError):
        resize_pos_embedding({KEY: _table(2, 4)}, (4, 4))  # 8 rows: no square grid
    with pytest.raises(ValueError):
        resize_pos_embedding({KEY: _table(2, 4)}, (4, 4), old_grid=(3, 3))
    assert resize_pos_embedding({KEY: _table(2, 4)}, (4, 4), old_grid=(2, 4))[KEY].shape == (1, 17, 16)


def test_resized_square_checkpoint_loads_into_rectangular_model():
    from vitmi.checkpoint import resize_pos_embedding
    from vitmi.model import VisionTransformer
    torch.manual_seed(1)
    sq = VisionTransformer(image_size=(32, 32), patch_size=(8, 8), **ARCH)
    rect = VisionTransformer(image_size=(16, 32), patch_size=(8, 8), **ARCH)
    with pytest.raises(RuntimeError):
        rect.load_state_dict(sq.state_dict())  # opt-in: load_state_dict alone still refuses the table
    rect.load_state_dict(resize_pos_embedding(sq.state_dict(), (2, 4)), strict=True)
    assert torch.equal(rect.embedding.weight, sq.embedding.weight)
    assert rect.transformer.pos_embedding.pos_embedding.shape == (1, 9, 64)


# ---- command line ---------------------------------------------------------------------------------------
def test_image_size_flag(capsys):
    from vitmi.config import get_eval_config, get_train_config, image_hw
    c = get_train_config(["--image-size", "224", "--no-save"])
    assert c.image_size == 224 and isinstance(c.image_size, int) and not c.resize_pos_embedding
    c = get_train_config(["--image-size", "224x384", "--any-image-size", "--no-save", "--resize-pos-embedding"])
    assert c.image_size == (224, 384) and c.resize_pos_embedding
    assert get_eval_config(["--image-size", "224x384", "--any-image-size"]).image_size == (224, 384)
    with pytest.raises(SystemExit):
        get_train_config(["--image-size", "224x384", "--no-save"])
    with pytest.raises(SystemExit):
        get_train_config(["--image-size", "100", "--no-save"])  # the 224 / 384 check is unchanged
    with pytest.raises(SystemExit):
        get_train_config(["--image-size", "224xx384", "--any-image-size", "--no-save"])
    assert image_hw(224) == (224, 224) and image_hw((224, 384)) == (224, 384)
    capsys.readouterr()


def test_build_model_and_resvit_args_take_pairs():
    from vitmi import resvit_train
    from vitmi.config import get_train_config
    from vitmi.train import build_model
    c = get_train_config(["--image-size", "32x64", "--any-image-size", "--no-save", "--num-classes", "10"])
    c.emb_dim, c.mlp_dim, c.num_heads, c.num_layers = 64, 128, 2, 1
    m = build_model(c, "cpu")
    assert m.arch.image_hw == (32, 64) and m.arch.grid_hw == (2, 4)
    rc = resvit_train.get_train_config(["--image-size", "32x64", "--any-image-size"])
    assert resvit_train.config_to_model_args(rc).image_size == (32, 64)
    assert resvit_train.get_train_config(["--image-size", "384"]).image_size == 384
    with pytest.raises(SystemExit):
        resvit_train.get_train_config(["--image-size", "32x64"])
