"""Float64 references and per-element gates for the from-scratch augmentation kernels: the soft-target cross entropy
(vit_cross_entropy_soft), the batch mix (vit_mix_batch), and scalar restatements of the host rules they are fed by
(torchvision's RandomResizedCrop.get_params, timm's rand_bbox). A helper module, not a test file; it builds on
glue_ref (the hard cross entropy's reference, the hit rule, worst()).
"""
import math

import numpy as np
import torch

import glue_ref as G
from glue_ref import NAN, UF, f32


# ---- soft-target cross entropy -----------------------------------------------------------------------------------
def sum_depth(C):
    """additions on the longest path of the kernel's f32 sum over a row of C logits: a thread adds ceil(C / 256)
    values in turn, the wave tree has six levels, three more additions join the four waves"""
    return -(-C // 256) + 6 + 3


def cross_entropy_soft(logits, labels, labels2, lam, smoothing, grad_scale):
    """float64 reference and gates of vit_cross_entropy_soft, extending glue_ref.cross_entropy's derivation. With
    eps = smoothing and lam as the f32 values the kernel receives, wy = (1-eps) lam, wy2 = (1-eps)(1-lam):
        t_c     = wy [c = y] + wy2 [c = y2] + eps / C
        loss    = lse - wy x_y - wy2 x_y2 - eps mean_c x_c
        dlogits = (p - t) grad_scale
    and, with E = 2^-21 (4 + R + |lse|) of the hard case and S = |lse| + wy |x_y| + wy2 |x_y2| + eps |mean x|:
        |loss - ref|    <= E max(1, S) + 2 UF D eps mean|x|
        |dlogits - ref| <= grad_scale (E p + 2^-23 + 2^-23)      per element
    lse and p are the hard kernel's, with its E. The hard loss lse - x_y is one rounding at the size |lse| + |x_y|,
    which E max(1, |lse| + |x_y|) carries; here the loss gains one rounding at the size of each of the three terms,
    so the size becomes S (the weights themselves add at most three roundings relative to their term, inside the
    factor 2 that E already has over its count). The sum of the logits is accumulated in f32 along a path of
    D = sum_depth(C) additions, each within UF of a partial sum of magnitude at most sum|x|; times eps / C that is
    D UF eps mean|x|, with the factor 2 on top. The gradient gains 2^-23 = 2 UF for forming t, a value of at most 1:
    its rounding and the factor 2.
    labels2 None = labels, lam None = 1. Hits are counted against `labels`. Either label outside [0, C): loss and the
    dlogits row are NaN and the row is a miss; a NaN logit makes its row NaN."""
    r = G.CE()
    grad_scale, eps = f32(grad_scale), f32(smoothing)
    x = logits.double()
    B, C = x.shape
    labels2 = labels if labels2 is None else labels2
    lam = torch.ones(B) if lam is None else lam
    l = lam.float().double().to(x.device)
    ok = (labels >= 0) & (labels < C) & (labels2 >= 0) & (labels2 < C)
    y, y2 = labels.clamp(0, C - 1), labels2.clamp(0, C - 1)
    wy, wy2 = (1 - eps) * l, (1 - eps) * (1 - l)
    r.lse = torch.logsumexp(x, 1)
    xy, xy2 = x.gather(1, y[:, None])[:, 0], x.gather(1, y2[:, None])[:, 0]
    nan = torch.full_like(r.lse, NAN)
    mean = x.mean(1)
    r.loss = torch.where(ok, r.lse - wy * xy - wy2 * xy2 - eps * mean, nan)
    r.p = torch.exp(x - r.lse[:, None])
    cls = torch.arange(C, device=x.device)[None, :]
    r.t = wy[:, None] * (cls == y[:, None]) + wy2[:, None] * (cls == y2[:, None]) + eps / C
    r.dlogits = torch.where(ok[:, None], (r.p - r.t) * grad_scale, nan[:, None])
    R = x.max(1).values - x.min(1).values
    r.E = 2.0 ** -21 * (4 + R + r.lse.abs())
    S = r.lse.abs() + wy * xy.abs() + wy2 * xy2.abs() + eps * mean.abs()
    r.bound_loss = r.E * S.clamp_min(1.0) + 2 * UF * sum_depth(C) * eps * x.abs().mean(1)
    r.bound_d = grad_scale * (r.E[:, None] * r.p + 2.0 ** -23 + 2.0 ** -23)
    hit1, hit5 = G.ce_hits(logits, labels)
    r.top1, r.top5 = hit1 * ok, hit5 * ok
    return r


def ce_soft_emulate(logits, labels, labels2, lam, smoothing, grad_scale, drop_uniform=False):
    """the kernel's formula in torch: lse and p in f32 as glue_ref.ce_emulate, the sum of the logits in f32, the
    weights in float64, t and the loss rounded to f32 once: (loss, dlogits) a correct kernel writes up to the order
    of its sums. drop_uniform: the eps / C share left out of t and of the loss (a one-term error the gates must
    catch). Only the CPU test of the gate uses it."""
    x = logits.float()
    C = x.shape[1]
    l2e = torch.tensor(1.4426950408889634, dtype=torch.float32)
    mx = x.max(1, keepdim=True).values
    s = torch.exp2((x - mx) * l2e).sum(1, keepdim=True)
    lse = mx + torch.log(s)
    p = torch.exp2((x - lse) * l2e)
    eps, l = f32(smoothing), lam.float().double()
    wy, wy2, wu = (1 - eps) * l, (1 - eps) * (1 - l), 0.0 if drop_uniform else eps / C
    cls = torch.arange(C)[None, :]
    t = (wy[:, None] * (cls == labels[:, None]) + wy2[:, None] * (cls == labels2[:, None]) + wu).float()
    sx = x.sum(1)
    loss = (lse[:, 0].double() - wy * x.gather(1, labels[:, None])[:, 0].double()
            - wy2 * x.gather(1, labels2[:, None])[:, 0].double() - wu * sx.double()).float()
    return loss, (p - t) * torch.tensor(grad_scale, dtype=torch.float32)


# ---- batch mix -----------------------------------------------------------------------------------------------------
def mix_batch(x, pair, lam, box):
    """float64 reference of vit_mix_batch: (ref [B, 3, H, W], bound, inside mask [B, 1, H, W]). Inside sample b's box
    the output is the partner's value exactly (bound 0); elsewhere lam a + (1 - lam) b with
    |out - ref| <= 2^-23 (|lam a| + |(1 - lam) b|). A pair entry outside [0, B) makes the sample NaN."""
    B, _, H, W = x.shape
    ok = (pair >= 0) & (pair < B)
    xb = x[pair.clamp(0, B - 1)].double()
    xa = x.double()
    l = lam.float().double()[:, None, None, None]
    yy = torch.arange(H)[None, :, None]
    xx = torch.arange(W)[None, None, :]
    inside = ((yy >= box[:, 0, None, None]) & (yy < box[:, 1, None, None]) &
              (xx >= box[:, 2, None, None]) & (xx < box[:, 3, None, None]))[:, None]
    ref = torch.where(inside, xb, l * xa + (1 - l) * xb)
    bound = torch.where(inside, torch.zeros_like(ref), 2.0 ** -23 * ((l * xa).abs() + ((1 - l) * xb).abs()))
    ref = torch.where(ok[:, None, None, None], ref, torch.full_like(ref, NAN))
    return ref, bound, inside


# ---- host rules, restated one sample at a time -------------------------------------------------------------------
def crop_box_scalar(H, W, draws, scale, ratio):
    """torchvision RandomResizedCrop.get_params for one image, its loop as written there, fed the uniforms `draws`
    [10, 4] in place of its generator: (top, left, h, w). The fallback's sides are clamped to the image (and to at
    least one pixel), as vitmi.augment.random_resized_crop_box documents."""
    area = H * W
    log_ratio = (math.log(ratio[0]), math.log(ratio[1]))
    for u_area, u_ratio, u_top, u_left in draws:
        target_area = area * (scale[0] + u_area * (scale[1] - scale[0]))
        aspect_ratio = math.exp(log_ratio[0] + u_ratio * (log_ratio[1] - log_ratio[0]))
        w = int(round(math.sqrt(target_area * aspect_ratio)))
        h = int(round(math.sqrt(target_area / aspect_ratio)))
        if 0 < w <= W and 0 < h <= H:
            top = min(int(math.floor(u_top * (H - h + 1))), H - h)
            left = min(int(math.floor(u_left * (W - w + 1))), W - w)
            return top, left, h, w
    in_ratio = float(W) / float(H)
    if in_ratio < min(ratio):
        w = W
        h = int(round(w / min(ratio)))
    elif in_ratio > max(ratio):
        h = H
        w = int(round(h * max(ratio)))
    else:
        w, h = W, H
    w, h = min(max(w, 1), W), min(max(h, 1), H)
    return (H - h) // 2, (W - w) // 2, h, w


def rand_bbox_scalar(H, W, lam, cy, cx):
    """timm rand_bbox (margin 0) with the centre given, then cutmix_bbox_and_lam's corrected lambda"""
    ratio = np.sqrt(1 - lam)
    cut_h, cut_w = int(H * ratio), int(W * ratio)
    yl, yh = np.clip(cy - cut_h // 2, 0, H), np.clip(cy + cut_h // 2, 0, H)
    xl, xh = np.clip(cx - cut_w // 2, 0, W), np.clip(cx + cut_w // 2, 0, W)
    return (int(yl), int(yh), int(xl), int(xh)), 1.0 - (yh - yl) * (xh - xl) / float(H * W)
