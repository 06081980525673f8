"""Checkpoint import: the reference's JAX `.npz` -> PyTorch state_dict conversion.

Follows reference src/checkpoint.py:
  load_checkpoint      :7-17   (.npz -> convert, .pth -> ['state_dict'])
  load_jax             :20-25  (np.load, allow_pickle=False; the reference opens the file through
                                tensorflow.io.gfile, absent here — a plain local open is used)
  save_jax_to_pytorch  :28-33
  replace_names        :36-77  (Flax module path -> reference module names)
  convert_jax_pytorch  :80-115 (per-tensor layout changes)

Layout rules, restated (reference :95-111): rank-1 tensors are squeezed; rank-2 `weight`s (Dense
kernels, stored [in][out] by Flax) are transposed to nn.Linear's [out][in]; the multi-head q/k/v
kernels [D][H][hd] / biases [H][hd] and the out kernel [H][hd][D] already match LinearGeneral and
are kept; the rank-4 conv kernel HWIO is permuted to OIHW. Everything else (cls token [1,1,D],
position embedding [1,N,D]) is kept as is.

Only safe loaders are used: numpy with allow_pickle=False, torch.load with weights_only=True.
The result feeds `VisionTransformer.load_state_dict`, whose parameters are views of the engine's
flat buffer; the bf16 GEMM mirror is rebuilt on the next forward (parameter versions change).
"""
import math
import os

import numpy as np
import torch


def load_jax(path):
    """reference src/checkpoint.py:20-25 — (keys, values) of a Flax `.npz` parameter dump."""
    with open(path, "rb") as f:
        with np.load(f, allow_pickle=False) as ckpt:
            items = [(k, np.asarray(ckpt[k])) for k in ckpt.files]
    if not items:
        return (), ()
    keys, values = zip(*items)
    return keys, values


def replace_names(names):
    """reference src/checkpoint.py:36-77 — one Flax path component -> reference module name(s)."""
    out = []
    for name in names:
        if name == "Transformer":
            out.append("transformer")
        elif name == "encoder_norm":
            out.append("norm")
        elif "encoderblock" in name:
            out += ["encoder_layers", name.split("_")[-1]]
        elif "LayerNorm" in name:
            # LayerNorm_0 is the pre-attention norm, LayerNorm_2 the pre-MLP norm; the reference
            # drops any other index (none occurs inside an encoder block)
            idx = name.split("_")[-1]
            if idx == "0":
                out.append("norm1")
            elif idx == "2":
                out.append("norm2")
        elif "MlpBlock" in name:
            out.append("mlp")
        elif "Dense" in name:
            out.append("fc{}".format(int(name.split("_")[-1]) + 1))
        elif "MultiHeadDotProductAttention" in name:
            out.append("attn")
        elif name in ("kernel", "scale"):
            out.append("weight")
        elif name == "posembed_input":
            out.append("pos_embedding")
        elif name == "head":
            out.append("classifier")
        elif name == "cls":
            out.append("cls_token")
        else:  # bias, pos_embedding, embedding, query/key/value/out, ...
            out.append(name)
    return out


def convert_jax_pytorch(keys, values):
    """reference src/checkpoint.py:80-115 — Flax arrays -> fp32 tensors in the reference's layouts."""
    state_dict = {}
    for key, value in zip(keys, values):
        names = replace_names(key.split("/"))
        t = torch.tensor(np.asarray(value), dtype=torch.float)
        nd = t.dim()
        if nd == 1:
            t = t.squeeze()
        elif nd == 2 and names[-1] == "weight":
            t = t.T
        elif nd == 4 and names[-1] == "weight":
            t = t.permute(3, 2, 0, 1)
        # rank-3 q/k/v/out kernels and rank-2 q/k/v biases: LinearGeneral already uses Flax's layout
        state_dict[".".join(names)] = t.contiguous()
    return state_dict


def load_checkpoint(path):
    """reference src/checkpoint.py:7-17 — weights from a `.npz` (Flax) or `.pth` (reference) file."""
    if path.endswith("npz"):
        return convert_jax_pytorch(*load_jax(path))
    if path.endswith("pth"):
        return torch.load(path, map_location="cpu", weights_only=True)["state_dict"]
    raise ValueError("checkpoint format {} not supported yet!".format(path.split(".")[-1]))


EMA_KEY = "state_dict_ema"  # timm's key for the weight EMA inside a training checkpoint


def load_checkpoint_ema(path):
    """the EMA weights of a vitmi.train `.pth` written by an --ema-decay run; ValueError naming the file when it holds
    none (a Flax `.npz` never does)"""
    ckpt = torch.load(path, map_location="cpu", weights_only=True) if path.endswith("pth") else {}
    if EMA_KEY not in ckpt:
        raise ValueError(f"{path}: no '{EMA_KEY}' in this checkpoint (vitmi.train writes it with --ema-decay)")
    return ckpt[EMA_KEY]


def save_jax_to_pytorch(jax_path, save_path):
    """reference src/checkpoint.py:28-33 — write `<name>.pth` = {'state_dict': converted weights}."""
    model_name = os.path.basename(jax_path).split(".")[0]
    state_dict = convert_jax_pytorch(*load_jax(jax_path))
    out = os.path.join(save_path, model_name + ".pth")
    torch.save({"state_dict": state_dict}, out)
    return out


POS_EMBEDDING_KEY = "transformer.pos_embedding.pos_embedding"


def _lerp_axis(t, g_new, dim):
    """bilinear resample of t along dim to g_new samples, half-pixel centres, edges clamped"""
    g = t.shape[dim]
    s = ((torch.arange(g_new, dtype=torch.float32) + 0.5) * (g / g_new) - 0.5).clamp_(0, g - 1)
    i0 = s.floor().long()
    i1 = (i0 + 1).clamp_(max=g - 1)
    shape = [1] * t.dim()
    shape[dim] = g_new
    w = (s - i0.float()).view(shape)
    return t.index_select(dim, i0) * (1 - w) + t.index_select(dim, i1) * w


def resize_pos_embedding(state_dict, new_grid, old_grid=None, key=POS_EMBEDDING_KEY):
    """A copy of state_dict whose position table [1, 1 + gh*gw, D] is resampled to new_grid = (gh', gw'): the way
    to load a checkpoint into a model of another patch grid (224 -> 384, square -> rectangular), where
    load_state_dict alone refuses the table's shape. The cls row is copied; the gh x gw patch rows are
    resampled separably and bilinearly in f32 with half-pixel centres (output index i samples
    s = (i + 0.5) g / g' - 0.5 clamped to [0, g - 1]: rows i0 = floor(s) and min(i0 + 1, g - 1), weight s - i0),
    rows first, then columns. old_grid None: the square grid sqrt(rows - 1). The same grid returns the table
    unchanged. Host arithmetic at load time; nothing calls it unless asked to."""
    pos = state_dict[key]
    if pos.dim() != 3 or pos.shape[0] != 1:
        raise ValueError(f"{key}: expected [1, tokens, D], got {tuple(pos.shape)}")
    rows, d = pos.shape[1] - 1, pos.shape[2]
    if old_grid is None:
        g = math.isqrt(max(rows, 0))
        if g * g != rows:
            raise ValueError(f"{key}: {rows} patch rows are no square grid; pass old_grid=(gh, gw)")
        old_grid = (g, g)
    (gh, gw), (nh, nw) = (int(v) for v in old_grid), (int(v) for v in new_grid)
    if gh * gw != rows or min(gh, gw, nh, nw) < 1:
        raise ValueError(f"{key}: {rows} patch rows are not a {gh}x{gw} grid, or an empty grid was asked for")
    out = type(state_dict)(state_dict)
    if (gh, gw) == (nh, nw):
        return out
    p = pos.detach().to("cpu", torch.float32)
    grid = _lerp_axis(_lerp_axis(p[0, 1:].view(gh, gw, d), nh, 0), nw, 1)
    out[key] = torch.cat([p[:, :1], grid.reshape(1, nh * nw, d)], dim=1).to(pos.dtype)
    return out
