"""The from-scratch augmentations on the GPU: crop boxes inside the ragged transform (bit-exact against the
Pillow-pinned oracle on numpy slices), the soft-target cross entropy and the batch mix (per-element gates of
augment_ref), FolderLoader(crop=...), and the training step with label smoothing, Mixup and CutMix end to end."""
import math

import numpy as np
import pytest
import torch

import augment_ref as A
import glue_ref as G
from folder_trees import fake_decode
from oracle.preprocess import resize_bilinear_u8, to_tensor_normalize

pytestmark = pytest.mark.gpu
DEV = "cuda"
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
NAN = float("nan")


# ---- vit_preprocess_u8_ragged_crop ---------------------------------------------------------------------------------
SIZES = [(132, 260), (133, 261), (40, 300), (99, 64), (33, 65), (5, 7)]


@pytest.fixture(scope="module")
def packed():
    """the six sources, packed in a shuffled order as tests/test_preprocess_ragged_gpu.py packs them; read-only"""
    rng = np.random.default_rng(21)
    images = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in SIZES]
    order = np.random.default_rng(22).permutation(len(images))
    geom = np.zeros((len(images), 3), np.int64)
    chunks, pos = [], 0
    for i in order:
        geom[i] = (pos, images[i].shape[0], images[i].shape[1])
        chunks.append(images[i].reshape(-1))
        pos += images[i].size
    return images, np.concatenate(chunks), geom


def _want(img, crop, oh, ow, flip):
    t, l, h, w = crop
    r = resize_bilinear_u8(np.ascontiguousarray(img[t:t + h, l:l + w]), oh, ow)
    return to_tensor_normalize(r[:, ::-1, :] if flip else r, MEAN, STD)


def _run_crop(raw, geom, oh, ow, index, flips, crops, labels=None, n_bytes=None, plain=False):
    from vitmi import ops
    B = len(index)
    out = torch.full((B, 3, oh, ow), 7.0, device=DEV)
    lab_in = None if labels is None else torch.as_tensor(np.asarray(labels, np.int64)).to(DEV)
    lab_out = None if labels is None else torch.full((B,), -7, dtype=torch.int64, device=DEV)
    b = raw if torch.is_tensor(raw) else torch.from_numpy(raw).to(DEV)
    kw = dict(index=torch.as_tensor(np.asarray(index, np.int64)).to(DEV),
              flips=torch.as_tensor(np.asarray(flips, np.uint8)).to(DEV), mean=MEAN, std=STD, labels_in=lab_in,
              labels_out=lab_out, n_bytes=n_bytes)
    if plain:
        ops.preprocess_u8_ragged(b, torch.from_numpy(geom).to(DEV), out, **kw)
    else:
        ops.preprocess_u8_ragged_crop(b, torch.from_numpy(geom).to(DEV), out,
                                      None if crops is None else torch.as_tensor(np.asarray(crops, np.int64)).to(DEV),
                                      **kw)
    return out.cpu().numpy(), None if lab_out is None else lab_out.cpu().numpy()


# (source, (top, left, h, w), flip, what it is there for), for outputs of 33 x 65
CASES_33x65 = [
    (0, (50, 100, 20, 40), 0, "3 taps: an upscaled crop, interior"),
    (0, (0, 0, 30, 65), 1, "3 taps, flush with the top and left borders"),
    (0, (66, 130, 66, 130), 0, "5 taps (2x on both axes), flush with the bottom and right borders: the last pixel"),
    (0, (0, 130, 60, 130), 1, "5 taps, top and right borders"),
    (0, (0, 0, 132, 260), 0, "9 taps (4x): the whole image"),
    (1, (1, 1, 132, 260), 1, "9 taps, bottom and right borders of an odd-sized source"),
    (1, (33, 0, 100, 200), 0, "9 taps, left border"),
    (2, (0, 0, 40, 300), 0, "per pixel on the horizontal axis alone (4.6x), 5 taps vertically"),
    (2, (5, 7, 33, 293), 1, "per pixel horizontally, the identity vertically, right border"),
    (3, (0, 10, 99, 7), 1, "9 taps vertically (3x), upscaled horizontally"),
    (1, (0, 0, 133, 261), 0, "per pixel on both axes (4.03x each)"),
    (1, (0, 100, 133, 20), 1, "per pixel vertically alone, upscaled horizontally"),
    (0, (131, 259, 1, 1), 0, "a 1 x 1 crop: the image's last pixel"),
    (5, (4, 6, 1, 1), 1, "a 1 x 1 crop of the smallest source"),
    (0, (17, 29, 33, 65), 0, "a crop of exactly the output size: the identity"),
    (4, (0, 0, 33, 65), 1, "the identity on a whole image"),
    (0, (17, 29, 33, 65), 1, "the same source and crop, flipped"),
    (5, (0, 0, 5, 7), 0, "a tiny source, whole"),
    (5, (2, 0, 3, 7), 1, "bottom border of the tiny source"),
    (3, (98, 0, 1, 64), 0, "one row: the last"),
    (3, (0, 63, 99, 1), 1, "one column: the last"),
]
CASES_7x9 = [
    (5, (0, 0, 5, 7), 0, "3 taps"),
    (5, (1, 2, 4, 5), 1, "3 taps, bottom and right borders"),
    (4, (10, 20, 14, 18), 0, "5 taps"),
    (4, (5, 29, 28, 36), 1, "9 taps, bottom and right borders"),
    (3, (0, 0, 99, 64), 0, "per pixel on both axes"),
    (3, (0, 0, 20, 64), 1, "per pixel on the horizontal axis alone"),
    (3, (0, 60, 99, 4), 0, "per pixel on the vertical axis alone, right border"),
    (0, (125, 251, 7, 9), 1, "the identity, flush with the last pixel"),
    (0, (0, 0, 1, 1), 0, "1 x 1: the first pixel"),
    (2, (39, 0, 1, 300), 1, "the last row"),
]


@pytest.mark.parametrize("oh,ow,cases", [(33, 65, CASES_33x65), (7, 9, CASES_7x9)], ids=["33x65", "7x9"])
def test_cropped_outputs_equal_the_oracle_on_slices(packed, oh, ow, cases):
    images, raw, geom = packed
    index, crops, flips = [c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases]
    for s, (t, l, h, w) in zip(index, crops):                       # the cases are what they say: inside the image
        assert 0 <= t and 0 <= l and h >= 1 and w >= 1 and t + h <= SIZES[s][0] and l + w <= SIZES[s][1]
    labels = np.arange(len(images)) + 100
    got, lab = _run_crop(raw, geom, oh, ow, index, flips, crops, labels=labels)
    for b, (s, crop, flip, what) in enumerate(cases):
        want = _want(images[s], crop, oh, ow, flip)
        assert np.array_equal(got[b], want), (b, what, np.abs(got[b] - want).max())
    assert np.array_equal(lab, labels[index])


def test_paths_taken_are_the_ones_the_cases_name():
    """Pillow's kernel size per axis, ceil(max(in / out, 1)) * 2 + 1, of every 33 x 65 case: the list holds the three
    tiled specialisations and the per-pixel path by one axis alone and by both"""
    def ks(i, o):
        return math.ceil(max(i / o, 1.0)) * 2 + 1
    kinds = set()
    for _, (_, _, h, w), _, _ in CASES_33x65:
        ky, kx = ks(h, 33), ks(w, 65)
        kinds.add("tiled%d" % max(ky, kx) if max(ky, kx) <= 9 else
                  "pixel-both" if min(ky, kx) > 9 else "pixel-x" if kx > 9 else "pixel-y")
    assert {"tiled3", "tiled5", "tiled9", "pixel-x", "pixel-y", "pixel-both"} <= kinds


def test_no_crops_and_full_image_crops_equal_the_uncropped_entry(packed):
    _, raw, geom = packed
    index = [0, 1, 2, 3, 4, 5, 2, 0]
    flips = [0, 1, 0, 1, 0, 1, 1, 1]
    labels = np.arange(6) + 40
    want, wlab = _run_crop(raw, geom, 33, 65, index, flips, None, labels=labels, plain=True)
    assert not np.isnan(want).any()
    none, nlab = _run_crop(raw, geom, 33, 65, index, flips, None, labels=labels)
    full, flab = _run_crop(raw, geom, 33, 65, index, flips, [(0, 0) + SIZES[s] for s in index], labels=labels)
    assert np.array_equal(none, want) and np.array_equal(full, want)
    assert np.array_equal(nlab, wlab) and np.array_equal(flab, wlab)


def test_bad_crops_give_nan_and_label_minus_one_for_those_outputs_only(packed):
    """a negative top, left + w = W + 1, h = 0 (and their kin). `bytes` is a view into the middle of an allocation
    twice as long, so a kernel that read through a bad box would still read allocated memory and fail by value"""
    images, raw, geom = packed
    nb = raw.size
    big = torch.from_numpy(np.random.default_rng(23).integers(0, 256, 2 * nb, dtype=np.uint8)).to(DEV)
    start = nb // 2
    big[start:start + nb] = torch.from_numpy(raw).to(DEV)
    view = big[start:start + nb]
    H, W = SIZES[3]
    cases = [(3, (-1, 0, 10, 10), "negative top"), (3, (0, W - 9, 10, 10), "left + w = W + 1"),
             (3, (5, 5, 0, 10), "h = 0"), (3, (5, 5, 10, 10), None), (3, (0, -1, 10, 10), "negative left"),
             (3, (H - 9, 0, 10, 10), "top + h = H + 1"), (3, (5, 5, 10, 0), "w = 0"), (3, (5, 5, -3, 10), "h < 0"),
             (3, (0, 0, 1 << 40, 1), "h = 2^40"), (3, (1 << 62, 0, 1, 1), "top = 2^62"),
             (0, (0, 0, 132, 260), None), (3, (H - 10, W - 10, 10, 10), None)]
    index, crops = [c[0] for c in cases], [c[1] for c in cases]
    flips = [b % 2 for b in range(len(cases))]
    labels = np.arange(6) + 40
    got, lab = _run_crop(view, geom, 33, 65, index, flips, crops, labels=labels, n_bytes=nb)
    for b, (s, crop, bad) in enumerate(cases):
        if bad:
            assert np.isnan(got[b]).all() and lab[b] == -1, (b, bad)
        else:
            assert np.array_equal(got[b], _want(images[s], crop, 33, 65, flips[b])), b
            assert lab[b] == labels[s]


def test_crop_wrapper_refuses_bad_tables():
    from vitmi import ops
    b = torch.zeros(300, dtype=torch.uint8, device=DEV)
    geom = torch.tensor([[0, 10, 10]], dtype=torch.int64, device=DEV)
    out = torch.full((1, 3, 4, 4), 7.0, device=DEV)
    crops = torch.tensor([[0, 0, 5, 5]], dtype=torch.int64, device=DEV)
    with pytest.raises(TypeError):
        ops.preprocess_u8_ragged_crop(b, geom, out, crops.int())
    with pytest.raises(ValueError):
        ops.preprocess_u8_ragged_crop(b, geom, out, crops.cpu())
    with pytest.raises(ValueError):
        ops.preprocess_u8_ragged_crop(b, geom, out, crops.repeat(2, 1))
    with pytest.raises(ValueError):
        ops.preprocess_u8_ragged_crop(b, geom, out, crops[:, :3])
    torch.cuda.synchronize()
    assert (out == 7.0).all()


# ---- vit_cross_entropy_soft ------------------------------------------------------------------------------------------
def _soft(x, y, y2, lam, eps, gs):
    from vitmi import ops
    B, C = x.shape
    d = torch.full((B, C), 7.0, device=DEV)
    st = torch.full((B, 3), 7.0, device=DEV)
    ops.cross_entropy_soft(x.to(DEV), y.to(DEV), d, gs, st, labels2=None if y2 is None else y2.to(DEV),
                           lam=None if lam is None else lam.to(DEV), smoothing=eps)
    return d.cpu(), st.cpu()


@pytest.mark.parametrize("C", [10, 257, 1000])
@pytest.mark.parametrize("eps", [0.0, 0.1])
def test_soft_cross_entropy_meets_its_gates(C, eps):
    B = 7
    g = torch.Generator().manual_seed(100 + C)
    x = G.ce_logits(B, C, g)
    y = torch.randint(0, C, (B,), generator=g)
    y2 = torch.randint(0, C, (B,), generator=g)
    lam = torch.tensor([0.0, 1.0, 0.37, 0.37, 0.0, 1.0, 0.37])
    y2[3] = y[3]                      # the partner shares the label
    y2[4] = C                         # out of range (with lam = 0)
    x[5, (int(y[5]) + 1) % C] = NAN   # a NaN logit, not the label's own: a miss
    y[6] = int(x[6].argmax())         # a hit by its own label, whatever the partner's
    for gs in (1.0, 1.0 / B):
        d, st = _soft(x, y, y2, lam, eps, gs)
        r = A.cross_entropy_soft(x, y, y2, lam, eps, gs)
        rl, al = G.worst(st[:, 0], r.loss, r.bound_loss)
        rd, ad = G.worst(d, r.dlogits, r.bound_d)
        print(f"soft ce C={C} eps={eps} gs={gs:.3g}: loss ratio {rl:.3f} at {al}, dlogits ratio {rd:.3f} at {ad}")
        assert rl <= 1.0 and rd <= 1.0
        assert st[4, 0].isnan() and d[4].isnan().all() and st[5, 0].isnan() and d[5].isnan().all()
        assert not d[[0, 1, 2, 3, 6]].isnan().any()
        h1, h5 = G.ce_hits(x, y)
        h1[4] = h5[4] = 0.0           # a bad partner label is a miss
        assert torch.equal(st[:, 1].double(), h1) and torch.equal(st[:, 2].double(), h5)
        assert torch.equal(st[:, 1].double(), r.top1) and st[6, 1] == 1.0 and st[5, 1] == 0.0


@pytest.mark.parametrize("C", [10, 257, 1000])
def test_degenerate_soft_call_is_the_hard_kernel_bit_for_bit(C):
    from vitmi import ops
    B = 7
    g = torch.Generator().manual_seed(200 + C)
    x = G.ce_logits(B, C, g)
    y = torch.randint(0, C, (B,), generator=g)
    y[2] = -1
    x[3, 1] = NAN
    x[4, int(y[4])] = -math.inf       # a weight of zero must not meet this logit
    x[5, (int(y[5]) + 1) % C] = -math.inf
    for gs in (1.0, 1.0 / 64):
        d0 = torch.full((B, C), 7.0, device=DEV)
        s0 = torch.full((B, 3), 7.0, device=DEV)
        ops.cross_entropy(x.to(DEV), y.to(DEV), d0, gs, s0)
        d1, s1 = _soft(x, y, None, None, 0.0, gs)
        assert torch.equal(d0.cpu().view(torch.int32), d1.view(torch.int32))
        assert torch.equal(s0.cpu().view(torch.int32), s1.view(torch.int32))
        # lam = 1 with a partner label given is the same again: the partner has no weight
        d2, s2 = _soft(x, y, y.clamp(0, C - 1).flip(0), torch.ones(B), 0.0, gs)
        ok = y >= 0
        assert torch.equal(d0.cpu()[ok].view(torch.int32), d2[ok].view(torch.int32))
        assert torch.equal(s0.cpu()[ok].view(torch.int32), s2[ok].view(torch.int32))


def test_soft_cross_entropy_null_outputs_and_refusals():
    from vitmi import _lib, ops
    x = G.ce_logits(3, 10, torch.Generator().manual_seed(1)).to(DEV)
    y = torch.tensor([1, 2, 3], device=DEV)
    st = torch.full((3, 3), 7.0, device=DEV)
    ops.cross_entropy_soft(x, y, None, 1.0, st, smoothing=0.1)             # no gradient wanted
    d = torch.full((3, 10), 7.0, device=DEV)
    ops.cross_entropy_soft(x, y, d, 1.0, None, smoothing=0.1)              # no statistics wanted
    r = A.cross_entropy_soft(x.cpu(), y.cpu(), None, None, 0.1, 1.0)
    assert G.worst(st[:, 0].cpu(), r.loss, r.bound_loss)[0] <= 1.0
    assert G.worst(d.cpu(), r.dlogits, r.bound_d)[0] <= 1.0
    with pytest.raises(ValueError):
        ops.cross_entropy_soft(x, y, d, 1.0, st, smoothing=1.0)
    with pytest.raises(ValueError):
        ops.cross_entropy_soft(x, y, d, 1.0, st, lam=torch.ones(2, device=DEV))
    with pytest.raises(TypeError):
        ops.cross_entropy_soft(x, y, d, 1.0, st, labels2=y.int())
    lib = _lib.load()
    before = d.clone()
    assert lib.vit_cross_entropy_soft(x.data_ptr(), y.data_ptr(), None, None, 1.0, 3, 10, d.data_ptr(), 1.0, None,
                                      None) == 1                             # VIT_ERR_INVALID_ARG
    assert lib.vit_cross_entropy_soft(x.data_ptr(), y.data_ptr(), None, None, NAN, 3, 10, d.data_ptr(), 1.0, None,
                                      None) == 1
    torch.cuda.synchronize()
    assert torch.equal(d, before)


# ---- vit_mix_batch -------------------------------------------------------------------------------------------------
def _mix_case(B, H, W, seed, misalign=0):
    """x and a NaN-filled output inside flat buffers with guard elements; misalign: elements the two are shifted by
    (the scalar path also for W % 4 == 0)"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, 3, H, W, generator=g)
    x[0, 0, 0, 0], x[B - 1, 2, H - 1, W - 1] = -0.0, 1e-30
    n = x.numel()
    xf = torch.full((n + 16,), NAN, device=DEV)
    of = torch.full((n + 16,), NAN, device=DEV)
    xv, ov = xf[misalign:misalign + n].view(B, 3, H, W), of[misalign:misalign + n].view(B, 3, H, W)
    xv.copy_(x)
    return x, xv, ov, of


def _check_mix(B, H, W, pair, lam, box, seed, misalign=0):
    from vitmi import ops
    x, xv, ov, of = _mix_case(B, H, W, seed, misalign)
    pair, lam, box = torch.tensor(pair), torch.tensor(lam, dtype=torch.float32), torch.tensor(box)
    ops.mix_batch(xv, ov, pair.to(DEV), lam.to(DEV), box.to(DEV))
    got = ov.cpu()
    ref, bound, inside = A.mix_batch(x, pair, lam, box)
    ratio, at = G.worst(got, ref, bound)
    print(f"mix [{B},3,{H},{W}] misalign {misalign}: worst ratio {ratio:.3f} at {at}")
    assert ratio <= 1.0
    ok = (pair >= 0) & (pair < B)
    partner = x[pair.clamp(0, B - 1)]
    full = inside.expand_as(x)
    for b in range(B):
        if not ok[b]:
            assert got[b].isnan().all(), b
            continue
        m = full[b]
        assert torch.equal(got[b][m].view(torch.int32), partner[b][m].view(torch.int32)), b     # an exact copy
        if lam[b] == 1.0:
            assert torch.equal(got[b][~m].view(torch.int32), x[b][~m].view(torch.int32)), b
        if lam[b] == 0.0:
            assert torch.equal(got[b][~m].view(torch.int32), partner[b][~m].view(torch.int32)), b
    assert torch.equal(xv.cpu(), x)                                         # the input is left alone
    assert G.first_touched(of, ov) is None                                  # nothing outside the output is written
    return got


def test_mix_scalar_path_odd_batch():
    """[5, 3, 9, 13]: W is no multiple of 4; the middle sample of the reversed batch pairs with itself"""
    B, H, W = 5, 9, 13
    pair = [4, 3, 2, 1, 0]
    lam = [0.3, 1.0, 0.3, 0.0, 1.0]
    box = [[0, 0, 0, 0],            # empty: Mixup
           [2, 7, 3, 10],           # CutMix, interior
           [0, H, 0, W],            # full: the partner (itself)
           [0, 4, 0, 5],            # top-left corner, blended elsewhere with lam = 0
           [5, H, 6, W]]            # bottom-right corner, lam = 1
    _check_mix(B, H, W, pair, lam, box, seed=1)


def test_mix_vector_path_boxes_start_and_end_mid_vector():
    """[4, 3, 8, 16]: float4 accesses; box edges inside a vector, on vector boundaries and on the image's edges"""
    B, H, W = 4, 8, 16
    pair = [3, 2, 1, 0]
    for lam, box in (([0.3, 1.0, 0.0, 1.0], [[0, 0, 0, 0], [1, 7, 5, 11], [0, H, 0, W], [0, 3, 0, 6]]),
                     ([1.0, 1.0, 0.3, 0.3], [[2, 8, 13, 16], [0, 8, 4, 8], [3, 4, 1, 2], [0, 8, 15, 16]]),
                     ([0.3, 0.3, 0.3, 0.3], [[-5, 3, -2, 3], [6, 99, 14, 99], [4, 4, 0, 16], [0, 8, 7, 7]])):
        _check_mix(B, H, W, pair, lam, box, seed=2)


def test_mix_scalar_path_for_unaligned_pointers():
    _check_mix(4, 8, 16, [3, 2, 1, 0], [0.3, 1.0, 0.0, 0.3], [[0, 0, 0, 0], [1, 7, 5, 11], [0, 8, 0, 16], [2, 3, 3, 9]],
               seed=3, misalign=1)


@pytest.mark.parametrize("B,H,W", [(5, 9, 13), (4, 8, 16)])
def test_mix_bad_pair_gives_a_nan_sample_for_that_row_only(B, H, W):
    pair = list(range(B - 1, -1, -1))
    pair[1], pair[B - 1] = B, -1
    lam = [0.3] * B
    box = [[1, 5, 2, 9]] * B
    got = _check_mix(B, H, W, pair, lam, box, seed=4)
    assert got[1].isnan().all() and got[B - 1].isnan().all() and not got[0].isnan().any()


def test_mix_more_than_one_block_and_refusals():
    from vitmi import _lib, ops
    B, H, W = 6, 32, 48                      # 27648 elements: 27 blocks of float4 threads
    _check_mix(B, H, W, [5, 4, 3, 2, 1, 0], [0.3, 0.7, 1.0, 0.0, 0.5, 0.9],
               [[0, 0, 0, 0], [3, 30, 5, 41], [0, 32, 0, 48], [10, 11, 0, 48], [0, 32, 47, 48], [31, 32, 0, 1]], seed=5)
    x = torch.zeros(2, 3, 4, 4, device=DEV)
    out = torch.full((2, 3, 4, 4), 7.0, device=DEV)
    pair = torch.tensor([1, 0], device=DEV)
    lam = torch.ones(2, device=DEV)
    box = torch.zeros(2, 4, dtype=torch.int64, device=DEV)
    with pytest.raises(_lib.VitHipError):
        ops.mix_batch(x, x, pair, lam, box)                                    # in place
    with pytest.raises(ValueError):
        ops.mix_batch(x, out[:1], pair, lam, box)
    with pytest.raises(ValueError):
        ops.mix_batch(x, out, pair, lam, box[:, :3])
    with pytest.raises(TypeError):
        ops.mix_batch(x, out, pair.int(), lam, box)
    with pytest.raises(TypeError):
        ops.mix_batch(x, out, pair, lam.double(), box)
    torch.cuda.synchronize()
    assert (out == 7.0).all()


def test_batch_mixer_on_the_device():
    """BatchMixer end to end: the reversed batch as partner, the box pasted exactly (CutMix) or the blend (Mixup),
    the target carrying (y, reversed y, lambda); its second buffer is reused"""
    from vitmi.augment import BatchMixer
    g = torch.Generator().manual_seed(6)
    x = torch.randn(6, 3, 16, 20, generator=g).to(DEV)
    y = torch.arange(6, device=DEV)
    m = BatchMixer(0.8, 1.0, seed=4)
    seen, ptrs = set(), set()
    for _ in range(12):
        out, t = m(x, y)
        lam, use_cutmix, (y0, y1, x0, x1) = m.last
        seen.add(use_cutmix)
        ptrs.add(out.data_ptr())
        assert torch.equal(t.y, y) and torch.equal(t.y2, y.flip(0))
        assert torch.equal(t.lam.cpu(), torch.full((6,), lam, dtype=torch.float32))
        if use_cutmix:
            want = x.clone()
            want[:, :, y0:y1, x0:x1] = x.flip(0)[:, :, y0:y1, x0:x1]
            assert torch.equal(out, want)
            assert lam == 1.0 - (y1 - y0) * (x1 - x0) / (16 * 20)
        else:
            l32 = float(torch.tensor(lam, dtype=torch.float32))
            ref = l32 * x.double() + (1 - l32) * x.flip(0).double()
            bound = 2.0 ** -23 * ((l32 * x.double()).abs() + ((1 - l32) * x.flip(0).double()).abs())
            assert G.worst(out.cpu(), ref.cpu(), bound.cpu())[0] <= 1.0
    assert seen == {True, False} and len(ptrs) == 1
    alone = BatchMixer(0.8, 1.0, prob=0.0)
    out, t = alone(x, y)
    assert torch.equal(out, x) and bool((t.lam == 1.0).all())


# ---- FolderLoader(crop=...) ----------------------------------------------------------------------------------------
N, BATCH, OUT = 23, 4, (16, 24)
PATHS = [f"/nowhere/class_{i % 5}/img_{i:03d}.JPEG" for i in range(N)]
LABELS = np.arange(N) % 5
CROP = ((0.08, 1.0), (3.0 / 4.0, 4.0 / 3.0))


def _loader(**kw):
    from vitmi.data import FolderLoader
    args = dict(batch_size=BATCH, image_size=OUT, device=DEV, train=True, seed=7, num_classes=5, workers=3,
                decode=fake_decode, crop=CROP)
    args.update(kw)
    return FolderLoader(PATHS, LABELS, **args)


def test_folder_loader_crops_equal_the_oracle_streaming_and_resident():
    from vitmi.data import EpochPlan
    stream, resident = _loader(), _loader(resident=True)
    plan = EpochPlan(N, BATCH, True, seed=7)
    sources = [fake_decode(p) for p in PATHS]
    epochs = []
    for _ in range(2):
        order, flips = plan.next_epoch()
        boxes = []
        for (xa, ya), (xb, yb), (s, e) in zip(stream, resident, plan.slices() + [None]):
            crops = stream.last_crops.numpy()
            assert crops.shape == (e - s, 4)
            assert np.array_equal(resident.last_crops.numpy()[s:e], crops)
            idx = order[s:e].tolist()
            for k, i in enumerate(idx):
                t, l, h, w = crops[k]
                H, W, _ = sources[i].shape
                assert 0 <= t and 0 <= l and h >= 1 and w >= 1 and t + h <= H and l + w <= W
                r = resize_bilinear_u8(np.ascontiguousarray(sources[i][t:t + h, l:l + w]), *OUT)
                want = to_tensor_normalize(r[:, ::-1] if flips[s + k] else r)
                assert np.array_equal(xa[k].cpu().numpy(), want), (s, k)
            assert torch.equal(xa, xb) and torch.equal(ya, yb)
            assert np.array_equal(ya.cpu().numpy(), LABELS[idx])
            boxes.append(crops)
        assert resident.last_crops.shape == (N, 4)
        epochs.append(np.concatenate(boxes))
    assert not np.array_equal(epochs[0], epochs[1])                  # a new epoch, new boxes


def test_folder_loader_crops_do_not_depend_on_batch_size_or_world():
    whole = _loader(batch_size=4, resident=True)
    list(whole)
    for kw in (dict(batch_size=6), dict(batch_size=2, world=2, rank=1)):
        other = _loader(resident=True, **kw)
        list(other)
        assert torch.equal(other.last_crops, whole.last_crops)
    halves = [[(x.cpu(), y.cpu()) for x, y in _loader(batch_size=2, world=2, rank=r)] for r in range(2)]
    full = [(x.cpu(), y.cpu()) for x, y in _loader(batch_size=4)]
    for k in range(5):
        assert torch.equal(torch.cat([halves[0][k][0], halves[1][k][0]]), full[k][0])
        assert torch.equal(torch.cat([halves[0][k][1], halves[1][k][1]]), full[k][1])


@pytest.mark.parametrize("resident", [False, True])
def test_eval_split_ignores_crop(resident):
    cropped, plain = _loader(train=False, resident=resident), _loader(train=False, resident=resident, crop=None)
    for (xa, ya), (xb, yb) in zip(cropped, plain):
        assert torch.equal(xa, xb) and torch.equal(ya, yb)
    assert cropped.last_crops is None and cropped.crop_plan is None


# ---- the step, end to end ------------------------------------------------------------------------------------------
FLAGS = ["--label-smoothing", "0.1", "--mixup-alpha", "0.8", "--cutmix-alpha", "1.0"]


@pytest.mark.parametrize("accum", [1, 2])
def test_three_steps_with_smoothing_mixup_and_cutmix_report_the_reference_loss(accum, capsys):
    """A tiny ViT on synthetic batches, train_epoch with the mixer and the smoothed criterion built from the parsed
    flags: every step's reported loss equals the float64 soft cross entropy of that step's logits and mixed target.
    Gate: each micro-batch's loss is the f32 mean of b row losses, each within augment_ref's bound_loss, the mean adding
    at most b roundings of a partial sum (b UF mean|loss|); the step's loss is the weighted sum over its micro-batches,
    two more roundings each (4 UF)."""
    from vitmi.augment import BatchMixer, MixedTarget
    from vitmi.config import get_train_config
    from vitmi.model import CrossEntropyLoss, VisionTransformer
    from vitmi.optim import SGD
    from vitmi.train import MetricTracker, accum_weights, train_epoch
    c = get_train_config(["--synthetic", "--no-save", "--checkpoint-path", "", "--accum-steps", str(accum),
                          "--batch-size", str(8 * accum)] + FLAGS)
    capsys.readouterr()
    b, C, steps = 8, 10, 3
    torch.manual_seed(42)
    m = VisionTransformer(image_size=(32, 32), patch_size=(4, 4), emb_dim=128, mlp_dim=256, num_heads=2, num_layers=2,
                          num_classes=C, dropout_rate=0.0).cuda()
    g = torch.Generator().manual_seed(8)
    loader = [(torch.randn(b, 3, 32, 32, generator=g).cuda(), torch.randint(0, C, (b,), generator=g).cuda())
              for _ in range(steps * accum)]
    m(loader[0][0][:1])                         # bind the engine before the optimizer holds the parameters
    m.accumulate_in_place = accum > 1
    opt = SGD(m.parameters(), lr=0.01, weight_decay=0.0, momentum=0.9, model=m)
    sched = torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=0.01, pct_start=0.3, total_steps=100)

    class Recording(CrossEntropyLoss):
        def __init__(self, **kw):
            super().__init__(**kw)
            self.seen = []

        def forward(self, logits, target):
            self.seen.append((logits.detach().clone(), target))
            return super().forward(logits, target)

    crit = Recording(label_smoothing=c.label_smoothing)
    mixer = BatchMixer(c.mixup_alpha, c.cutmix_alpha, c.mix_prob, c.mix_switch_prob, seed=c.seed)
    metrics = MetricTracker("loss", "acc1", "acc5")
    m.train()
    res = train_epoch(1, m, loader, crit, opt, sched, metrics, torch.device("cuda"), accum_steps=accum, mixer=mixer)
    capsys.readouterr()
    reported = [v for _, tag, v in metrics.writer.scalars_host() if tag.startswith("loss")]
    assert len(reported) == steps and len(crit.seen) == steps * accum
    mixed = 0
    for k in range(steps):
        group = crit.seen[k * accum:(k + 1) * accum]
        ref = bound = 0.0
        for (logits, t), w in zip(group, accum_weights([b] * accum)):
            assert isinstance(t, MixedTarget)
            mixed += int(float(t.lam[0]) < 1.0)
            r = A.cross_entropy_soft(logits.cpu(), t.y.cpu(), t.y2.cpu(), t.lam.cpu(), c.label_smoothing, 1.0 / b)
            ref += w * float(r.loss.mean())
            bound += w * (float(r.bound_loss.mean()) + (b + 4) * G.UF * float(r.loss.abs().mean()))
        print(f"accum {accum} step {k}: reported {reported[k]!r}, reference {ref!r}, bound {bound:.3g}")
        assert abs(reported[k] - ref) <= bound
    assert mixed > 0 and math.isfinite(res["loss"])
    for name, p in m.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name


@pytest.mark.parametrize("extra", [[], ["--accum-steps", "2"]], ids=["plain", "accum2"])
def test_train_main_runs_with_the_flags(extra, capsys):
    from vitmi import train
    train.main(["--model-arch", "b32", "--image-size", "32", "--any-image-size", "--batch-size", "16", "--num-classes",
                "10", "--synthetic", "--checkpoint-path", "", "--steps-per-epoch", "3" if not extra else "6",
                "--train-steps", "6", "--warmup-steps", "2", "--no-save"] + FLAGS + extra)
    out = capsys.readouterr().out
    losses = [float(l.split("Loss: ")[1].split()[0]) for l in out.splitlines() if l.startswith("Train Epoch")]
    assert losses and all(math.isfinite(v) for v in losses)
    assert "val_loss" in out


# ---- the drivers on an image-folder tree, with Pillow ------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny_imagenet_dir(tmp_path_factory):
    pytest.importorskip("PIL.Image")
    from folder_trees import write_tiny_imagenet
    root = tmp_path_factory.mktemp("augment_folders")
    write_tiny_imagenet(str(root / "TinyImageNet"), per_class=4, n_val=6, seed=3, val_form="annotations")
    return root


def test_train_main_crops_tiny_imagenet(tiny_imagenet_dir, capsys, monkeypatch):
    """the whole recipe through the CLI on a folder tree; the crop changes what the first step sees"""
    import re
    from vitmi import train
    monkeypatch.setenv("VITMI_EXP_STAMP", "test")
    args = ["--model-arch", "b32", "--image-size", "32", "--any-image-size", "--batch-size", "4", "--dataset",
            "TinyImageNet", "--num-classes", "3", "--checkpoint-path", "", "--train-steps", "6", "--warmup-steps", "2",
            "--no-save", "--num-workers", "4", "--data-dir", str(tiny_imagenet_dir)]
    first = re.compile(r"Train Epoch: 001 Batch: 00000/00003 Loss: (\S+) ")
    train.main(args)
    plain = first.search(capsys.readouterr().out).group(1)
    train.main(args + ["--random-resized-crop"])
    cropped = first.search(capsys.readouterr().out).group(1)
    train.main(args + ["--random-resized-crop"] + FLAGS)
    text = capsys.readouterr().out
    full = first.search(text).group(1)
    assert all(math.isfinite(float(v)) for v in (plain, cropped, full))
    assert cropped != plain and full != cropped
    assert "val_loss" in text


def test_resvit_train_main_crops_tiny_imagenet(tiny_imagenet_dir, capsys, monkeypatch):
    """vitmi.resvit_train takes --random-resized-crop through the same loader (the smallest model of its own tests)"""
    from test_resvit_cpu import TINY
    from vitmi import data, resvit, resvit_train
    monkeypatch.setenv("VITMI_EXP_STAMP", "test")
    monkeypatch.setattr(resvit_train, "build_model",
                        lambda config, device: resvit.Transformer(resvit.ModelArgs(**dict(TINY, device="cuda"))).to(device))
    made = []
    real = data.FolderLoader

    def spy(*a, **kw):
        made.append(real(*a, **kw))
        return made[-1]

    monkeypatch.setattr(data, "FolderLoader", spy)
    best = resvit_train.main(["--image-size", "32", "--any-image-size", "--batch-size", "4", "--dataset", "TinyImageNet",
                              "--data-dir", str(tiny_imagenet_dir), "--checkpoint-path", "", "--train-steps", "6",
                              "--warmup-steps", "2", "--no-save", "--random-resized-crop", "--crop-scale", "0.3", "1"])
    capsys.readouterr()
    assert math.isfinite(best)
    train_loader, valid_loader = made
    assert train_loader.crop_plan is not None and train_loader.crop_plan.scale == (0.3, 1.0)
    assert train_loader.last_crops is not None and train_loader.last_crops.shape[1] == 4
    assert valid_loader.crop_plan is None and valid_loader.last_crops is None
