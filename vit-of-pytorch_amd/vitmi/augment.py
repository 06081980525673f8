"""Host policy of the from-scratch augmentations: which crop box, which partner, which lambda. The pixels move on the
device (vit_preprocess_u8_ragged_crop, vit_mix_batch) and the soft target is the loss kernel's
(vit_cross_entropy_soft); nothing here touches an image.

  random_resized_crop_box   torchvision's RandomResizedCrop.get_params (the ViT paper's Inception crop), vectorised
                            over a batch and fed explicit uniform draws, so the rule is testable without its RNG
  CropPlan                  the draws of epoch position k, a function of (seed, epoch, k) alone: the box of a sample
                            does not depend on the batch size, the rank count, --accum-steps or thread timing
  BatchMixer                timm's Mixup in batch mode: one lambda ~ Beta(alpha, alpha) per batch, the partner the
                            reversed batch, Mixup or CutMix (rand_bbox, lambda corrected to the clipped box's area)

torchvision and timm are not part of this stack and their random streams are not reproduced, as with the flips
(vitmi.data): the rules are.
"""
from __future__ import annotations

import math

import numpy as np
import torch

CROP_TRIES = 10      # torchvision's attempts before the central fallback
CROP_CHUNK = 4096    # epoch positions per seeded generator (CropPlan)


def random_resized_crop_box(H, W, draws, scale=(0.08, 1.0), ratio=(3.0 / 4.0, 4.0 / 3.0)):
    """torchvision `RandomResizedCrop.get_params`, restated for n images at once: int64 [n, 4] = (top, left, h, w).

    H, W: the images' sizes (ints or int arrays [n]). draws: float64 [n, 10, 4] in [0, 1): for try t the uniforms
    behind (area, log-ratio, top, left). Try t: area = HW (s0 + u0 (s1 - s0)), r = exp(log r0 + u1 (log r1 - log r0)),
    w = round(sqrt(area r)), h = round(sqrt(area / r)) (round half to even, Python's round); the first try with
    0 < w <= W and 0 < h <= H is taken, top = floor(u2 (H - h + 1)), left = floor(u3 (W - w + 1)): uniform over the
    valid positions. No try fits: the central fallback, the whole image clamped to the ratio bounds (W/H below r0:
    w = W, h = round(W / r0); above r1: h = H, w = round(H r1)), centred. The fallback's sides are clamped to
    [1, H] x [1, W], which differs from torchvision only where its box would be empty or leave the image."""
    draws = np.asarray(draws, np.float64)
    n = draws.shape[0]
    if draws.shape != (n, CROP_TRIES, 4):
        raise ValueError(f"random_resized_crop_box: draws [n, {CROP_TRIES}, 4], got {draws.shape}")
    H = np.broadcast_to(np.asarray(H, np.int64), (n,))
    W = np.broadcast_to(np.asarray(W, np.int64), (n,))
    area = (H * W).astype(np.float64)[:, None] * (scale[0] + draws[:, :, 0] * (scale[1] - scale[0]))
    l0, l1 = math.log(ratio[0]), math.log(ratio[1])
    r = np.exp(l0 + draws[:, :, 1] * (l1 - l0))
    w = np.rint(np.sqrt(area * r)).astype(np.int64)
    h = np.rint(np.sqrt(area / r)).astype(np.int64)
    fits = (w > 0) & (w <= W[:, None]) & (h > 0) & (h <= H[:, None])
    any_fit = fits.any(1)
    t = fits.argmax(1)                      # the first try that fits
    rows = np.arange(n)
    hh, ww = h[rows, t], w[rows, t]
    top = np.floor(draws[rows, t, 2] * (H - hh + 1)).astype(np.int64)
    left = np.floor(draws[rows, t, 3] * (W - ww + 1)).astype(np.int64)
    # central fallback
    in_ratio = W / H
    fw = np.where(in_ratio > max(ratio), np.rint(H * max(ratio)).astype(np.int64), W)
    fh = np.where(in_ratio < min(ratio), np.rint(W / min(ratio)).astype(np.int64), H)
    fw, fh = np.clip(fw, 1, W), np.clip(fh, 1, H)
    hh, ww = np.where(any_fit, hh, fh), np.where(any_fit, ww, fw)
    top = np.where(any_fit, np.minimum(top, H - hh), (H - fh) // 2)
    left = np.where(any_fit, np.minimum(left, W - ww), (W - fw) // 2)
    return np.stack([top, left, hh, ww], 1).astype(np.int64)


class CropPlan:
    """The crop boxes of an epoch by position: position k of epoch e draws from chunk k // CROP_CHUNK's generator,
    seeded with (seed, e, chunk), at row k % CROP_CHUNK. Whoever asks for position k, alone or in any batch, on any
    rank, gets the same ten tries. One chunk of draws (1.3 MB) is alive at a time, whatever the set's size."""

    SEED_OFFSET = 0xC209_B0C5

    def __init__(self, seed, scale=(0.08, 1.0), ratio=(3.0 / 4.0, 4.0 / 3.0)):
        self.seed = int(seed)
        self.scale = (float(scale[0]), float(scale[1]))
        self.ratio = (float(ratio[0]), float(ratio[1]))
        check_crop_ranges(self.scale, self.ratio)
        self._cached = (None, None)

    def _chunk(self, epoch, c):
        if self._cached[0] != (epoch, c):
            g = np.random.default_rng([self.seed + self.SEED_OFFSET, int(epoch), int(c)])
            self._cached = ((epoch, c), g.random((CROP_CHUNK, CROP_TRIES, 4)))
        return self._cached[1]

    def boxes(self, epoch, start, H, W):
        """int64 [m, 4] for epoch positions start .. start + m - 1, whose images are H[i] x W[i]"""
        H, W = np.asarray(H, np.int64).reshape(-1), np.asarray(W, np.int64).reshape(-1)
        out = np.empty((H.size, 4), np.int64)
        k = int(start)
        stop = k + H.size
        while k < stop:
            c = k // CROP_CHUNK
            e = min(stop, (c + 1) * CROP_CHUNK)
            d = self._chunk(epoch, c)[k - c * CROP_CHUNK:e - c * CROP_CHUNK]
            out[k - start:e - start] = random_resized_crop_box(H[k - start:e - start], W[k - start:e - start], d,
                                                               self.scale, self.ratio)
            k = e
        return out


def check_crop_ranges(scale, ratio):
    if not (0.0 < scale[0] <= scale[1] <= 1.0):
        raise ValueError(f"crop scale {tuple(scale)}: expected 0 < min <= max <= 1")
    if not (0.0 < ratio[0] <= ratio[1]) or not math.isfinite(ratio[1]):
        raise ValueError(f"crop ratio {tuple(ratio)}: expected 0 < min <= max")


# ---- Mixup / CutMix --------------------------------------------------------------------------------------------------
def cutmix_box(H, W, lam, cy, cx):
    """timm's `rand_bbox` + `cutmix_bbox_and_lam(correct_lam=True)` for a centre (cy, cx): r = sqrt(1 - lam),
    cut_h = int(H r), cut_w = int(W r), the box [cy - cut_h // 2, cy + cut_h // 2) x [cx - cut_w // 2, cx + cut_w // 2)
    clipped to the image; returns ((y0, y1, x0, x1), 1 - box_area / (H W))."""
    r = math.sqrt(1.0 - lam)
    cut_h, cut_w = int(H * r), int(W * r)
    y0, y1 = min(max(cy - cut_h // 2, 0), H), min(max(cy + cut_h // 2, 0), H)
    x0, x1 = min(max(cx - cut_w // 2, 0), W), min(max(cx + cut_w // 2, 0), W)
    return (y0, y1, x0, x1), 1.0 - (y1 - y0) * (x1 - x0) / float(H * W)


class MixedTarget:
    """the target of a mixed batch: lam[b] of labels y[b] and 1 - lam[b] of y2[b] (device tensors [b]); what
    vitmi.model.CrossEntropyLoss takes in place of an int64 target"""

    def __init__(self, y, y2, lam):
        self.y, self.y2, self.lam = y, y2, lam

    @property
    def shape(self):
        return self.y.shape

    def to(self, *args, **kwargs):
        return MixedTarget(self.y.to(*args, **kwargs), self.y2.to(*args, **kwargs),
                           self.lam.to(*args, **{k: v for k, v in kwargs.items() if k != "dtype"}))


class BatchMixer:
    """timm `Mixup(mixup_alpha, cutmix_alpha, prob, switch_prob, mode='batch')` without its label smoothing (that is
    the loss's): per batch one lambda ~ Beta(alpha, alpha); the partner of sample i is sample b - 1 - i (the reversed
    batch); with probability 1 - prob the batch is left alone (lambda = 1); with both alphas > 0 CutMix is chosen with
    probability switch_prob. CutMix pastes the partner's box (cutmix_box, centre uniform over the image) and corrects
    lambda to the pasted area; Mixup blends whole images. Draws come from numpy's generator seeded with `seed`.

    mixer(x, y) -> (mixed x, MixedTarget): one vit_mix_batch launch into a second buffer that is reused from step to
    step (the mixed batch of step k is dead once step k + 1 is mixed). `last` keeps the latest (lam, use_cutmix, box)
    on the host for inspection."""

    def __init__(self, mixup_alpha=0.0, cutmix_alpha=0.0, prob=1.0, switch_prob=0.5, seed=42):
        if mixup_alpha < 0 or cutmix_alpha < 0 or not (mixup_alpha > 0 or cutmix_alpha > 0):
            raise ValueError(f"BatchMixer: mixup_alpha {mixup_alpha}, cutmix_alpha {cutmix_alpha}: both >= 0 and one > 0")
        if not 0.0 <= prob <= 1.0 or not 0.0 <= switch_prob <= 1.0:
            raise ValueError(f"BatchMixer: prob {prob} and switch_prob {switch_prob} must lie in [0, 1]")
        self.mixup_alpha, self.cutmix_alpha = float(mixup_alpha), float(cutmix_alpha)
        self.prob, self.switch_prob = float(prob), float(switch_prob)
        self.rng = np.random.default_rng([int(seed), 0x313C5])
        self.last = None
        self._out = None
        self._pair = None

    def draw(self, H, W):
        """(lam, use_cutmix, (y0, y1, x0, x1)) of the next batch: host only"""
        lam, use_cutmix, box = 1.0, False, (0, 0, 0, 0)
        if self.rng.random() < self.prob:
            if self.mixup_alpha > 0 and self.cutmix_alpha > 0:
                use_cutmix = bool(self.rng.random() < self.switch_prob)
            else:
                use_cutmix = self.cutmix_alpha > 0
            a = self.cutmix_alpha if use_cutmix else self.mixup_alpha
            lam = float(self.rng.beta(a, a))
            if use_cutmix:
                cy, cx = int(self.rng.integers(0, H)), int(self.rng.integers(0, W))
                box, lam = cutmix_box(H, W, lam, cy, cx)
        self.last = (lam, use_cutmix, box)
        return self.last

    def __call__(self, x, y):
        from . import ops
        b, _, H, W = x.shape
        lam, use_cutmix, box = self.draw(H, W)
        dev = x.device
        if self._pair is None or self._pair.numel() != b or self._pair.device != dev:
            self._pair = torch.arange(b - 1, -1, -1, device=dev, dtype=torch.int64)
        if self._out is None or self._out.shape != x.shape or self._out.device != dev:
            self._out = torch.empty_like(x, memory_format=torch.contiguous_format)
        # CutMix: the box is the partner's, the rest the sample's own (weight 1); Mixup: no box, weight lam
        lam_dev = torch.full((b,), 1.0 if use_cutmix else lam, device=dev, dtype=torch.float32)
        box_dev = torch.tensor(box, dtype=torch.int64).repeat(b, 1).to(dev, non_blocking=True)
        ops.mix_batch(x.contiguous(), self._out, self._pair, lam_dev, box_dev)
        target = MixedTarget(y, y.flip(0), torch.full((b,), lam, device=dev, dtype=torch.float32))
        return self._out, target
