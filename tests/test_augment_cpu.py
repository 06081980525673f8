"""The host side of the from-scratch augmentations (vitmi.augment, the new flags) and the soft cross entropy's gates
(augment_ref), without a GPU: the crop rule against a scalar restatement of torchvision's loop, the crop draws'
independence of batching, timm's CutMix box and corrected lambda, the Beta moments, the gates checked before the
kernel is, flag validation."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

import augment_ref as A
import glue_ref as G

DEFAULT_SCALE, DEFAULT_RATIO = (0.08, 1.0), (3.0 / 4.0, 4.0 / 3.0)


# ---- the crop rule -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(375, 500), (64, 64), (10, 500), (1, 1)])
@pytest.mark.parametrize("scale,ratio", [(DEFAULT_SCALE, DEFAULT_RATIO), ((0.5, 1.0), (0.25, 4.0)),
                                         ((0.9, 1.0), (3.0, 4.0))])
def test_crop_boxes_equal_the_scalar_restatement_and_lie_inside(H, W, scale, ratio):
    from vitmi.augment import random_resized_crop_box
    n = 300
    draws = np.random.default_rng(H * 1000 + W).random((n, 10, 4))
    draws[0, :, 2:] = 1.0 - 2.0 ** -53          # the last valid position, not one past it
    draws[1, :, 2:] = 0.0
    got = random_resized_crop_box(H, W, draws, scale, ratio)
    assert got.shape == (n, 4) and got.dtype == np.int64
    want = np.array([A.crop_box_scalar(H, W, d, scale, ratio) for d in draws])
    assert np.array_equal(got, want)
    top, left, h, w = got.T
    assert (h >= 1).all() and (w >= 1).all() and (top >= 0).all() and (left >= 0).all()
    assert (top + h <= H).all() and (left + w <= W).all()
    if (H, W) == (375, 500) and scale == DEFAULT_SCALE:
        assert len({tuple(b) for b in got}) > n // 2         # they do vary


def test_crop_boxes_take_per_image_sizes():
    from vitmi.augment import random_resized_crop_box
    sizes = np.array([(375, 500), (64, 64), (10, 500), (1, 1), (500, 10)])
    draws = np.random.default_rng(5).random((len(sizes), 10, 4))
    got = random_resized_crop_box(sizes[:, 0], sizes[:, 1], draws)
    want = np.array([A.crop_box_scalar(h, w, d, DEFAULT_SCALE, DEFAULT_RATIO) for (h, w), d in zip(sizes, draws)])
    assert np.array_equal(got, want)


@pytest.mark.parametrize("W", [64, 65, 7])
def test_forced_fallback_is_deterministic_and_centred(W):
    """a square image, scale (1, 1), ratio (2, 2): every try asks for w = round(W sqrt 2) > W, so the fallback
    applies whatever the draws: w = W, h = round(W / 2), centred"""
    from vitmi.augment import random_resized_crop_box
    for seed in (0, 1):
        draws = np.random.default_rng(seed).random((4, 10, 4))
        got = random_resized_crop_box(W, W, draws, (1.0, 1.0), (2.0, 2.0))
        h = int(round(W / 2))
        assert (got == np.array([(W - h) // 2, 0, h, W])).all()


def test_crop_draws_depend_on_seed_epoch_and_position_only():
    from vitmi.augment import CROP_CHUNK, CropPlan
    n = CROP_CHUNK + 50                                    # positions on both sides of a chunk boundary
    rng = np.random.default_rng(3)
    H, W = rng.integers(20, 400, n), rng.integers(20, 400, n)
    whole = CropPlan(7).boxes(1, 0, H, W)
    assert np.array_equal(CropPlan(7).boxes(1, 0, H, W), whole)               # the same seed, the same boxes
    assert not np.array_equal(CropPlan(8).boxes(1, 0, H, W), whole)
    assert not np.array_equal(CropPlan(7).boxes(2, 0, H, W), whole)
    for start, m in ((CROP_CHUNK - 3, 6), (0, 1), (n - 1, 1), (17, 4)):         # any window, asked alone
        assert np.array_equal(CropPlan(7).boxes(1, start, H[start:start + m], W[start:start + m]),
                              whole[start:start + m])


def test_crop_boxes_of_a_position_are_the_same_for_any_batch_size_and_world():
    """what FolderLoader does with the plan: every rank asks for its slices of the epoch's order. Position k gets
    the same box at batch 4 and 6, world 1 and 2"""
    from vitmi.augment import CropPlan
    from vitmi.data import EpochPlan
    n = 24
    rng = np.random.default_rng(4)
    H, W = rng.integers(5, 90, n), rng.integers(5, 90, n)     # sizes by epoch position
    by_position = {}
    for batch, world in ((4, 1), (6, 1), (2, 2), (3, 2)):
        seen = {}
        for rank in range(world):
            plan, crops = EpochPlan(n, batch, True, seed=9, world=world, rank=rank), CropPlan(9)
            for s, e in plan.slices():
                for k, box in zip(range(s, e), crops.boxes(1, s, H[s:e], W[s:e])):
                    seen[k] = tuple(box)
        assert sorted(seen) == list(range(n))
        by_position[(batch, world)] = seen
    first = by_position[(4, 1)]
    assert all(v == first for v in by_position.values())


def test_crop_plan_refuses_bad_ranges():
    from vitmi.augment import CropPlan
    for scale, ratio in (((0.0, 1.0), DEFAULT_RATIO), ((0.5, 0.2), DEFAULT_RATIO), ((0.1, 1.5), DEFAULT_RATIO),
                         (DEFAULT_SCALE, (0.0, 1.0)), (DEFAULT_SCALE, (2.0, 1.0))):
        with pytest.raises(ValueError):
            CropPlan(1, scale, ratio)


# ---- CutMix boxes, lambda --------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,lam,cy,cx", [(32, 48, 0.5, 16, 24), (32, 48, 0.5, 0, 0), (32, 48, 0.5, 31, 47),
                                           (32, 48, 0.3, 0, 47), (32, 48, 0.3, 31, 0), (9, 13, 0.9, 4, 6),
                                           (9, 13, 0.0, 4, 6), (9, 13, 1.0, 4, 6), (224, 224, 0.75, 3, 220)])
def test_cutmix_box_follows_rand_bbox_and_corrects_lambda(H, W, lam, cy, cx):
    from vitmi.augment import cutmix_box
    box, lam2 = cutmix_box(H, W, lam, cy, cx)
    wbox, wlam = A.rand_bbox_scalar(H, W, lam, cy, cx)
    assert box == wbox and lam2 == wlam
    y0, y1, x0, x1 = box
    assert 0 <= y0 <= y1 <= H and 0 <= x0 <= x1 <= W
    assert lam2 == 1.0 - (y1 - y0) * (x1 - x0) / (H * W)


def test_cutmix_boxes_of_the_mixer_clip_at_all_four_edges():
    from vitmi.augment import BatchMixer, cutmix_box
    m = BatchMixer(cutmix_alpha=1.0, seed=3)
    H, W = 16, 20
    edges = set()
    for _ in range(400):
        lam, use_cutmix, (y0, y1, x0, x1) = m.draw(H, W)
        assert use_cutmix and 0 <= y0 <= y1 <= H and 0 <= x0 <= x1 <= W
        assert lam == 1.0 - (y1 - y0) * (x1 - x0) / (H * W)
        edges |= {k for k, hit in (("top", y0 == 0), ("bottom", y1 == H), ("left", x0 == 0), ("right", x1 == W))
                  if hit and (y1 - y0) * (x1 - x0) > 0}
    assert edges == {"top", "bottom", "left", "right"}
    # the same stream gives the same batches; a centre on each edge clips there
    a, b = BatchMixer(0.8, 1.0, seed=5), BatchMixer(0.8, 1.0, seed=5)
    assert [a.draw(H, W) for _ in range(20)] == [b.draw(H, W) for _ in range(20)]
    assert cutmix_box(H, W, 0.75, 0, 10)[0][0] == 0 and cutmix_box(H, W, 0.75, 15, 10)[0][1] == H
    assert cutmix_box(H, W, 0.75, 8, 0)[0][2] == 0 and cutmix_box(H, W, 0.75, 8, 19)[0][3] == W


def test_mixer_policy_prob_and_switch():
    from vitmi.augment import BatchMixer
    off = BatchMixer(0.8, 1.0, prob=0.0, seed=1)
    assert all(off.draw(8, 8) == (1.0, False, (0, 0, 0, 0)) for _ in range(50))     # left alone: lambda = 1
    only_mixup = BatchMixer(mixup_alpha=0.8, seed=1)
    assert all(not only_mixup.draw(8, 8)[1] for _ in range(50))
    both = BatchMixer(0.8, 1.0, switch_prob=0.5, seed=2)
    k = sum(both.draw(8, 8)[1] for _ in range(1000))
    assert abs(k - 500) <= 5 * math.sqrt(250)                                       # five standard deviations
    half = BatchMixer(0.8, 0.0, prob=0.5, seed=2)
    k = sum(half.draw(8, 8)[0] == 1.0 for _ in range(1000))
    assert abs(k - 500) <= 5 * math.sqrt(250)
    for bad in (dict(mixup_alpha=0.0, cutmix_alpha=0.0), dict(mixup_alpha=-1.0, cutmix_alpha=1.0),
                dict(mixup_alpha=1.0, prob=1.5), dict(mixup_alpha=1.0, switch_prob=-0.1)):
        with pytest.raises(ValueError):
            BatchMixer(**bad)


@pytest.mark.parametrize("alpha", [0.2, 0.8, 1.0])
def test_beta_moments_of_the_mixer(alpha):
    """lambda ~ Beta(a, a): mean 1/2, variance 1 / (4 (2a + 1)); 4000 draws, five standard errors. The standard
    error of the sample mean is sqrt(var / n), that of the sample variance sqrt((m4 - var^2) / n), m4 the fourth
    central moment of Beta(a, a), computed below from the raw moments E[x^k] = prod_{r<k} (a + r) / (2a + r)."""
    from vitmi.augment import BatchMixer
    n = 4000
    m = BatchMixer(mixup_alpha=alpha, seed=11)
    lam = np.array([m.draw(8, 8)[0] for _ in range(n)])
    assert ((lam >= 0) & (lam <= 1)).all()
    raw = [1.0]
    for r in range(4):
        raw.append(raw[-1] * (alpha + r) / (2 * alpha + r))
    mean, var = 0.5, 1.0 / (4 * (2 * alpha + 1))
    assert raw[1] == mean and abs(raw[2] - mean ** 2 - var) < 1e-15
    m4 = raw[4] - 4 * mean * raw[3] + 6 * mean ** 2 * raw[2] - 3 * mean ** 4
    assert abs(lam.mean() - mean) <= 5 * math.sqrt(var / n)
    assert abs(lam.var() - var) <= 5 * math.sqrt((m4 - var ** 2) / n)


# ---- the soft cross entropy's reference and gates ----------------------------------------------------------------
def _soft_case(B, C, seed):
    g = torch.Generator().manual_seed(seed)
    x = G.ce_logits(B, C, g)
    y = torch.randint(0, C, (B,), generator=g)
    y2 = torch.randint(0, C, (B,), generator=g)
    y2[0] = y[0]
    lam = torch.tensor(([0.0, 1.0, 0.37] * B)[:B])
    return x, y, y2, lam


@pytest.mark.parametrize("B,C", [(7, 10), (7, 257), (7, 1000), (65, 1023)])
@pytest.mark.parametrize("eps", [0.0, 0.1])
def test_soft_cross_entropy_reference_and_gates(B, C, eps):
    x, y, y2, lam = _soft_case(B, C, C + int(eps * 10))
    for gs in (1.0, 1.0 / B):
        r = A.cross_entropy_soft(x, y, y2, lam, eps, gs)
        # the reference is torch's: soft-target cross entropy on timm's mixup_target with smoothing
        e32, l = G.f32(eps), lam.float().double()[:, None]
        t = (1 - e32) * (l * Fn.one_hot(y, C) + (1 - l) * Fn.one_hot(y2, C)) + e32 / C
        xr = x.double().requires_grad_(True)
        loss = Fn.cross_entropy(xr, t, reduction="none")
        (loss.sum() * G.f32(gs)).backward()
        assert float((r.loss - loss.detach()).abs().max()) < 1e-12
        # (torch's gradient is p sum_c t_c - t: its sum over C targets carries up to C roundings of float64)
        assert float((r.dlogits - xr.grad).abs().max()) < C * 2.0 ** -52
        # ... and torch's label_smoothing for an unmixed row
        ls = Fn.cross_entropy(x.double(), y, reduction="none", label_smoothing=e32)
        assert float((r.loss - ls)[lam == 1.0].abs().max()) < 1e-12
        # the kernel's formula in f32 passes with room
        el, ed = A.ce_soft_emulate(x, y, y2, lam, eps, gs)
        assert G.worst(el, r.loss, r.bound_loss)[0] <= 0.5
        assert G.worst(ed, r.dlogits, r.bound_d)[0] <= 0.5
        # a planted error of twice the bound is found where it is
        badd = ed.double().clone()
        badd[B - 1, C - 1] = r.dlogits[B - 1, C - 1] + 2 * r.bound_d[B - 1, C - 1]
        ratio, at = G.worst(badd, r.dlogits, r.bound_d)
        assert at == (B - 1, C - 1) and ratio == pytest.approx(2, rel=1e-6)
    if eps > 0:
        # a one-term error: eps / C dropped from the target and the loss
        r = A.cross_entropy_soft(x, y, y2, lam, eps, 1.0)
        el, ed = A.ce_soft_emulate(x, y, y2, lam, eps, 1.0, drop_uniform=True)
        assert not G.worst(ed, r.dlogits, r.bound_d)[0] <= 1.0
        assert not G.worst(el, r.loss, r.bound_loss)[0] <= 1.0
        # the partner's label ignored
        el, ed = A.ce_soft_emulate(x, y, y, lam, eps, 1.0)
        assert not G.worst(ed, r.dlogits, r.bound_d)[0] <= 1.0 and not G.worst(el, r.loss, r.bound_loss)[0] <= 1.0


def test_soft_reference_degenerates_to_the_hard_one_and_marks_bad_rows():
    x, y, y2, lam = _soft_case(7, 10, 1)
    hard, soft = G.cross_entropy(x, y, 0.25), A.cross_entropy_soft(x, y, None, None, 0.0, 0.25)
    assert torch.equal(hard.loss, soft.loss) and torch.equal(hard.dlogits, soft.dlogits)
    assert torch.equal(hard.top1, soft.top1) and torch.equal(hard.top5, soft.top5)
    y2 = y2.clone()
    y2[2], y2[4] = 10, -1
    x = x.clone()
    x[5, 3] = float("nan")
    r = A.cross_entropy_soft(x, y, y2, lam, 0.1, 1.0)
    for b in (2, 4, 5):
        assert r.loss[b].isnan() and r.dlogits[b].isnan().all()
    assert r.top1[2] == 0 and r.top5[4] == 0                     # a bad partner label: a miss
    good = [0, 1, 3, 6]
    assert not r.loss[good].isnan().any() and not r.dlogits[good].isnan().any()
    h1, h5 = G.ce_hits(x, y)
    assert torch.equal(r.top1[good], h1[good]) and torch.equal(r.top5[good], h5[good])


def test_mix_reference():
    g = torch.Generator().manual_seed(2)
    x = torch.randn(3, 3, 4, 5, generator=g)
    pair = torch.tensor([2, 1, 7])
    lam = torch.tensor([0.25, 1.0, 0.5])
    box = torch.tensor([[1, 3, 2, 4], [0, 0, 0, 0], [0, 4, 0, 5]])
    ref, bound, inside = A.mix_batch(x, pair, lam, box)
    assert inside[0, 0].sum() == 4 and inside[1].sum() == 0 and inside[2].all()
    assert torch.equal(ref[0, :, 1:3, 2:4], x[2, :, 1:3, 2:4].double()) and (bound[0, :, 1:3, 2:4] == 0).all()
    assert torch.equal(ref[0, :, 0], 0.25 * x[0, :, 0].double() + 0.75 * x[2, :, 0].double())
    assert torch.equal(ref[1], x[1].double()) and ref[2].isnan().all()


# ---- flags -----------------------------------------------------------------------------------------------------
BASE = ["--synthetic", "--no-save", "--checkpoint-path", ""]


def test_new_flags_default_off_and_parse(capsys):
    from vitmi.config import get_train_config
    c = get_train_config(BASE)
    assert (c.random_resized_crop, c.label_smoothing, c.mixup_alpha, c.cutmix_alpha) == (False, 0.0, 0.0, 0.0)
    assert (c.mix_prob, c.mix_switch_prob, c.crop_scale) == (1.0, 0.5, [0.08, 1.0])
    assert c.crop_ratio == [3.0 / 4.0, 4.0 / 3.0]
    c = get_train_config(["--no-save", "--dataset", "ImageNet", "--random-resized-crop", "--crop-scale", "0.2", "1",
                          "--crop-ratio", "0.5", "2", "--label-smoothing", "0.1", "--mixup-alpha", "0.8",
                          "--cutmix-alpha", "1.0", "--mix-prob", "0.9", "--mix-switch-prob", "0.3"])
    assert c.random_resized_crop and c.crop_scale == [0.2, 1.0] and c.crop_ratio == [0.5, 2.0]
    assert (c.label_smoothing, c.mixup_alpha, c.cutmix_alpha, c.mix_prob, c.mix_switch_prob) == (0.1, 0.8, 1.0, 0.9,
                                                                                                 0.3)
    capsys.readouterr()


@pytest.mark.parametrize("args,needle", [
    (["--label-smoothing", "1.0"], "--label-smoothing"), (["--label-smoothing", "-0.1"], "--label-smoothing"),
    (["--mixup-alpha", "-1"], "--mixup-alpha"), (["--cutmix-alpha", "nan"], "--cutmix-alpha"),
    (["--mix-prob", "1.5"], "--mix-prob"), (["--mix-switch-prob", "-0.5"], "--mix-switch-prob"),
    (["--crop-scale", "0", "1"], "--crop-scale"), (["--crop-scale", "0.5", "0.2"], "--crop-scale"),
    (["--crop-scale", "0.5", "1.5"], "--crop-scale"), (["--crop-ratio", "2", "1"], "--crop-ratio"),
    (["--crop-ratio", "0", "1"], "--crop-ratio")])
def test_out_of_range_flags_exit_with_a_message(args, needle, capsys):
    from vitmi.config import get_train_config
    with pytest.raises(SystemExit) as e:
        get_train_config(BASE + args)
    assert needle in str(e.value)
    capsys.readouterr()


@pytest.mark.parametrize("dataset", ["CIFAR10", "CIFAR100"])
def test_random_resized_crop_refuses_cifar_in_one_line(dataset, capsys):
    from vitmi import resvit_train
    from vitmi.config import get_train_config
    with pytest.raises(SystemExit) as e:
        get_train_config(["--no-save", "--checkpoint-path", "", "--dataset", dataset, "--random-resized-crop"])
    assert "--random-resized-crop" in str(e.value) and dataset in str(e.value) and "\n" not in str(e.value)
    with pytest.raises(SystemExit) as e:
        resvit_train.get_train_config(["--no-save", "--dataset", dataset, "--random-resized-crop"])
    assert "--random-resized-crop" in str(e.value) and "\n" not in str(e.value)
    capsys.readouterr()


def test_resvit_train_accepts_the_crop_for_image_folders(capsys):
    from vitmi import resvit_train
    from vitmi.data import crop_of
    c = resvit_train.get_train_config(["--no-save", "--dataset", "TinyImageNet", "--random-resized-crop",
                                       "--crop-scale", "0.3", "1"])
    assert crop_of(c) == ((0.3, 1.0), (3.0 / 4.0, 4.0 / 3.0))
    assert crop_of(resvit_train.get_train_config(["--no-save", "--dataset", "TinyImageNet"])) is None
    assert not hasattr(c, "label_smoothing")                       # its distillation loss is not changed
    capsys.readouterr()


def test_loss_module_and_loader_surface():
    from vitmi.augment import MixedTarget
    from vitmi.model import CrossEntropyLoss
    assert CrossEntropyLoss().label_smoothing == 0.0 and CrossEntropyLoss(label_smoothing=0.1).label_smoothing == 0.1
    with pytest.raises(ValueError):
        CrossEntropyLoss(label_smoothing=1.0)
    t = MixedTarget(torch.arange(4), torch.arange(4).flip(0), torch.full((4,), 0.3))
    assert t.shape[0] == 4 and t.to("cpu").y2.tolist() == [3, 2, 1, 0]
    from vitmi import _lib
    assert _lib.ABI_VERSION == 24
