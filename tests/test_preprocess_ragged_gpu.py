"""vit_preprocess_u8_ragged (ops.preprocess_u8_ragged): one launch over a batch whose source images differ in
size (ImageNet / TinyImageNet folders: Resize((s, s)) of every decoded file, src/data_loaders.py:100-112,
res-vit/data_loaders.py:110-122) against the Pillow-pinned oracle applied per image. Bit-exact: np.array_equal,
no tolerance. The sizes take both paths of the kernel (<= 9 taps on both axes: tiled through LDS; above: per
pixel), partial blocks on both output axes, and metadata that must never be read through."""
import numpy as np
import pytest
import torch

from oracle.preprocess import resize_bilinear_u8, to_tensor_normalize

pytestmark = pytest.mark.gpu
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def _images(sizes, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in sizes]


def _pack(images, seed=0, shuffle=True):
    """(bytes uint8 [n_bytes], geom int64 [n, 3]) with the images laid end to end in a shuffled order, so that
    the offsets are not monotone in the image index"""
    order = np.random.default_rng(seed).permutation(len(images)) if shuffle else np.arange(len(images))
    geom = np.zeros((len(images), 3), np.int64)
    chunks, pos = [], 0
    for i in order:
        h, w, _ = images[i].shape
        geom[i] = (pos, h, w)
        chunks.append(images[i].reshape(-1))
        pos += images[i].size
    return np.concatenate(chunks), geom


def _want(img, oh, ow, flip, mean, std):
    r = resize_bilinear_u8(img, oh, ow)
    return to_tensor_normalize(r[:, ::-1, :] if flip else r, mean, std)


def _run(bytes_np, geom_np, B, oh, ow, index=None, flips=None, mean=MEAN, std=STD, labels=None, **kw):
    from vitmi import ops
    dev = "cuda"
    out = torch.full((B, 3, oh, ow), 7.0, device=dev)
    lab_in = None if labels is None else torch.as_tensor(np.asarray(labels, np.int64)).to(dev)
    lab_out = None if labels is None else torch.full((B,), -7, dtype=torch.int64, device=dev)
    b = bytes_np if torch.is_tensor(bytes_np) else torch.from_numpy(bytes_np).to(dev)
    ops.preprocess_u8_ragged(b, torch.from_numpy(geom_np).to(dev), out,
                             index=None if index is None else torch.as_tensor(np.asarray(index, np.int64)).to(dev),
                             flips=None if flips is None else torch.as_tensor(np.asarray(flips, np.uint8)).to(dev),
                             mean=mean, std=std, labels_in=lab_in, labels_out=lab_out, **kw)
    return out.cpu().numpy(), None if lab_out is None else lab_out.cpu().numpy()


def _check_launch(sizes, oh, ow, seed, flips=None):
    images = _images(sizes, seed)
    raw, geom = _pack(images, seed)
    n = len(images)
    flips = [0] * n if flips is None else flips
    labels = np.arange(100, 100 + n)
    got, lab = _run(raw, geom, n, oh, ow, flips=flips, labels=labels)
    for i, img in enumerate(images):
        want = _want(img, oh, ow, flips[i], MEAN, STD)
        assert np.array_equal(got[i], want), (sizes[i], (oh, ow), np.abs(got[i] - want).max())
    assert np.array_equal(lab, labels)


def test_mixed_sizes_to_33x65_take_both_paths_and_partial_blocks():
    """two row blocks and two column blocks, each with a partial one; 9-tap sources (the longest band the LDS
    path meets), 11-tap sources on both axes and on one axis alone (per-pixel path), up- and downscaling mixed
    within one image, the identity, and tiny sources"""
    sizes = [(132, 260), (131, 259), (133, 261), (40, 300), (66, 130), (99, 64), (33, 65), (5, 7), (1, 1)]
    _check_launch(sizes, 33, 65, seed=11, flips=[0, 1, 1, 0, 1, 0, 1, 1, 0])


def test_mixed_sizes_to_7x9():
    _check_launch([(64, 64), (7, 9), (2, 90)], 7, 9, seed=12, flips=[1, 0, 1])


def test_workload_ratios_to_224():
    _check_launch([(375, 500), (32, 32)], 224, 224, seed=13, flips=[0, 1])


def test_index_with_repeats_and_bad_entries_carries_the_labels():
    sizes = [(20, 31), (9, 50), (45, 12), (33, 33)]
    images = _images(sizes, 14)
    raw, geom = _pack(images, 14)
    n = len(images)
    index = [2, 2, -1, 0, n, 3, 1, 2]
    flips = [0, 1, 1, 0, 1, 1, 0, 0]
    labels = np.array([5, 6, 7, 8])
    got, lab = _run(raw, geom, len(index), 16, 24, index=index, flips=flips, labels=labels)
    for b, s in enumerate(index):
        if 0 <= s < n:
            assert np.array_equal(got[b], _want(images[s], 16, 24, flips[b], MEAN, STD)), (b, s)
            assert lab[b] == labels[s]
        else:
            assert np.isnan(got[b]).all() and lab[b] == -1, (b, s)


def test_bad_table_rows_give_nan_for_those_outputs_only():
    """H = 0, W = 2^15, a negative offset and an extent past n_bytes. `bytes` is a view into the middle of an
    allocation twice as long, so a kernel that ignored a check would still read allocated memory and fail here
    by value."""
    sizes = [(12, 17), (30, 8), (21, 21), (64, 40), (10, 10), (7, 33), (100, 400)]
    images = _images(sizes, 15)
    raw, geom = _pack(images, 15, shuffle=False)
    nb = raw.size
    rng = np.random.default_rng(16)
    big = torch.from_numpy(rng.integers(0, 256, 2 * nb, dtype=np.uint8)).cuda()
    start = nb // 2
    big[start:start + nb] = torch.from_numpy(raw).cuda()
    view = big[start:start + nb]
    bad = {1: "H0", 2: "W32768", 3: "negative", 5: "past"}
    geom[1, 1] = 0
    geom[2] = (0, 1, 1 << 15)  # 3 * 2^15 bytes from offset 0 lie inside n_bytes: only the W limit refuses it
    assert 3 * (1 << 15) <= nb
    geom[3, 0] = -(start // 2)  # before the view, inside the allocation
    geom[5, 0] = nb - int(geom[5, 1] * geom[5, 2] * 3) + 1  # one byte past n_bytes, inside the allocation
    labels = np.arange(7) + 40
    got, lab = _run(view, geom, 7, 20, 70, labels=labels, n_bytes=nb)
    for i, img in enumerate(images):
        if i in bad:
            assert np.isnan(got[i]).all() and lab[i] == -1, (i, bad[i])
        else:
            assert np.array_equal(got[i], _want(img, 20, 70, 0, MEAN, STD)), i
            assert lab[i] == labels[i]


def test_uniform_batch_equals_preprocess_u8():
    from vitmi import ops
    rng = np.random.default_rng(17)
    imgs = rng.integers(0, 256, (3, 50, 37, 3), dtype=np.uint8)
    flips = np.array([1, 0, 1], np.uint8)
    dev_imgs = torch.from_numpy(imgs).cuda()
    want = torch.empty(3, 3, 32, 32, device="cuda")
    ops.preprocess_u8(dev_imgs, want, torch.from_numpy(flips).cuda())
    geom = np.array([[i * 50 * 37 * 3, 50, 37] for i in range(3)], np.int64)
    got, _ = _run(dev_imgs.reshape(-1), geom, 3, 32, 32, flips=flips, mean=(0.5,) * 3, std=(0.5,) * 3)
    assert np.array_equal(got, want.cpu().numpy())


def test_host_side_refusals_raise_and_launch_nothing():
    from vitmi import _lib, ops
    b = torch.zeros(300, dtype=torch.uint8, device="cuda")
    geom = torch.tensor([[0, 10, 10]], dtype=torch.int64, device="cuda")
    out = torch.full((1, 3, 4, 4), 7.0, device="cuda")
    with pytest.raises(TypeError):
        ops.preprocess_u8_ragged(b.float(), geom, out)
    with pytest.raises(TypeError):
        ops.preprocess_u8_ragged(b, geom.int(), out)
    with pytest.raises(ValueError):
        ops.preprocess_u8_ragged(b.cpu(), geom, out)
    with pytest.raises(ValueError):
        ops.preprocess_u8_ragged(b[::2], geom, out)
    with pytest.raises(ValueError):
        ops.preprocess_u8_ragged(b, geom, out, index=torch.zeros(2, dtype=torch.int64, device="cuda"))
    with pytest.raises(ValueError):
        ops.preprocess_u8_ragged(b, geom, out, n_bytes=301)
    with pytest.raises(_lib.VitHipError):
        ops.preprocess_u8_ragged(b, geom, out, n_bytes=0)
    with pytest.raises(_lib.VitHipError):
        ops.preprocess_u8_ragged(b, geom, torch.empty(0, 3, 4, 4, device="cuda"),
                                 index=torch.zeros(0, dtype=torch.int64, device="cuda"))
    lib = _lib.load()
    assert lib.vit_preprocess_u8_ragged(None, 300, geom.data_ptr(), 1, None, 1, None, 4, 4, None, out.data_ptr(),
                                        None, None, None) == 1  # VIT_ERR_INVALID_ARG
    torch.cuda.synchronize()
    assert (out == 7.0).all()
