"""vit_preprocess_u8_gather (gather + layout + the reference loader's transform in one launch),
vitmi.data.ResidentLoader and the CIFAR entry points of vitmi.train / vitmi.eval / vitmi.resvit_train.

Every image comparison is bit-exact (np.array_equal) against the Pillow-pinned oracle,
oracle.preprocess.transform_batch(images_hwc[index], size, flips), and against vit_preprocess_u8 on an
index_select-ed HWC copy; every case runs both source layouts (HWC and planar CHW)."""
import re

import numpy as np
import pytest
import torch

from cifar_trees import write_tree
from oracle.preprocess import transform_batch

pytestmark = pytest.mark.gpu
LAYOUTS = ["hwc", "chw"]


def _device_set(imgs_hwc, layout, stride=None):
    """the set on the device in `layout`; stride: bytes between images, the padding filled with 255"""
    src = imgs_hwc if layout == "hwc" else np.ascontiguousarray(imgs_hwc.transpose(0, 3, 1, 2))
    n, per = src.shape[0], int(np.prod(src.shape[1:]))
    if stride is None:
        return torch.from_numpy(np.ascontiguousarray(src)).cuda()
    buf = torch.full((n, stride), 255, dtype=torch.uint8, device="cuda")
    buf[:, :per] = torch.from_numpy(src.reshape(n, per)).cuda()
    return buf[:, :per].view(src.shape)


def _gather(images, index, size, flips, layout, labels=None):
    from vitmi import ops
    index = torch.as_tensor(index, dtype=torch.int64).cuda()
    out = torch.full((index.numel(), 3, *size), 7.0, device="cuda")
    f = None if flips is None else torch.as_tensor(np.asarray(flips, np.uint8)).cuda()
    lab_out = None if labels is None else torch.full((index.numel(),), -7, dtype=torch.int64, device="cuda")
    ops.preprocess_u8_gather(images, index, out, f, layout=ops.IMAGES_CHW if layout == "chw" else ops.IMAGES_HWC,
                             labels_in=labels, labels_out=lab_out)
    return out.cpu().numpy(), None if lab_out is None else lab_out.cpu().numpy()


def _two_launches(imgs_hwc, index, size, flips):
    """the path this launch replaces: index_select, then vit_preprocess_u8"""
    from vitmi import ops
    sel = torch.from_numpy(imgs_hwc).cuda().index_select(0, torch.as_tensor(index).cuda())
    out = torch.empty(len(index), 3, *size, device="cuda")
    f = None if flips is None else torch.as_tensor(np.asarray(flips, np.uint8)).cuda()
    ops.preprocess_u8(sel, out, f)
    return out.cpu().numpy()


# (id, n, H, W, (out_h, out_w), index, flips)
CASES = [
    ("cifar_3tap_tiled", 10, 32, 32, (224, 224), [9, 0, 0, 3, 9, 5], [1, 0, 1, 0, 0, 1]),
    ("tile_edges", 5, 40, 56, (70, 100), [4, 1, 1, 0], [0, 1, 1, 0]),
    ("tile_edges_odd_width", 5, 40, 57, (70, 100), [3, 4, 0], [1, 0, 1]),
    ("5tap", 4, 64, 48, (32, 24), [2, 2, 0, 3], [1, 0, 0, 1]),
    ("9tap", 4, 70, 105, (20, 30), [3, 0, 1], [0, 1, 1]),
    ("generic", 3, 64, 64, (7, 9), [1, 2, 0, 1], [1, 1, 0, 0]),
    ("single", 1, 32, 32, (48, 48), [0], [1]),
]


@pytest.fixture(scope="module")
def case_data():
    """per case: the HWC set and the oracle's output, computed once and shared by both layouts"""
    out = {}
    for k, (cid, n, H, W, size, index, flips) in enumerate(CASES):
        imgs = np.random.default_rng(100 + k).integers(0, 256, (n, H, W, 3), dtype=np.uint8)
        want = transform_batch(imgs[index], size, flips)
        want.setflags(write=False)
        out[cid] = (imgs, want)
    return out


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_gather_matches_oracle_and_two_launch_path(case_data, case, layout):
    cid, n, H, W, size, index, flips = case
    imgs, want = case_data[cid]
    got, _ = _gather(_device_set(imgs, layout), index, size, flips, layout)
    assert got.shape == want.shape and np.array_equal(got, want), cid
    assert np.array_equal(got, _two_launches(imgs, index, size, flips)), cid


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("cid", ["cifar_3tap_tiled", "tile_edges_odd_width", "generic"])
def test_padded_image_stride(case_data, cid, layout):
    """image_stride > 3*H*W: the set carved out of a larger allocation whose padding bytes are 255"""
    _, n, H, W, size, index, flips = next(c for c in CASES if c[0] == cid)
    imgs, want = case_data[cid]
    dev = _device_set(imgs, layout, stride=3 * H * W + 37)
    assert dev.stride(0) == 3 * H * W + 37
    got, _ = _gather(dev, index, size, flips, layout)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_labels_travel_with_the_index(case_data, layout):
    _, n, H, W, size, index, flips = CASES[0]
    imgs, want = case_data[CASES[0][0]]
    labels = torch.arange(100, 100 + n, dtype=torch.int64).cuda()
    got, lab = _gather(_device_set(imgs, layout), index, size, flips, layout, labels)
    assert np.array_equal(lab, 100 + np.asarray(index)) and np.array_equal(got, want)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("H,W,size", [(32, 32, (48, 48)), (64, 64, (7, 9))], ids=["tiled", "generic"])
def test_bad_indices_give_nan_and_label_minus_one(layout, H, W, size):
    """index outside [0, n): NaN image, label -1, never read through. The set fills its allocation from the first
    byte to the last, so the neighbours (the first and the last image) matching the oracle is the check that nothing
    outside it was used."""
    n = 3
    imgs = np.random.default_rng(H).integers(0, 256, (n, H, W, 3), dtype=np.uint8)
    index, flips = [2, -1, n, 0], [1, 1, 0, 0]
    labels = torch.tensor([5, 6, 7], dtype=torch.int64).cuda()
    got, lab = _gather(_device_set(imgs, layout), index, size, flips, layout, labels)
    assert np.isnan(got[1]).all() and np.isnan(got[2]).all()
    assert lab.tolist() == [7, -1, -1, 5]
    want = transform_batch(imgs[[2, 0]], size, [1, 0])
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[3], want[1])


def test_bad_arguments_are_refused_and_launch_nothing():
    from vitmi import _lib, ops
    imgs = torch.zeros(4, 8, 8, 3, dtype=torch.uint8, device="cuda")
    index = torch.zeros(2, dtype=torch.int64, device="cuda")
    out = torch.full((2, 3, 4, 4), 7.0, device="cuda")
    for kw in (dict(image_stride=3 * 8 * 8 - 1), dict(layout=2), dict(layout=-1)):
        with pytest.raises(_lib.VitHipError, match="status 1"):
            ops.preprocess_u8_gather(imgs, index, out, **kw)
    with pytest.raises(_lib.VitHipError, match="status 1"):  # n_images == 0
        ops.preprocess_u8_gather(imgs[:0], index, out)
    with pytest.raises(_lib.VitHipError, match="status 1"):  # B == 0
        ops.preprocess_u8_gather(imgs, index[:0], out[:0])
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    # the wrapper's own checks, as ops.preprocess_u8's
    with pytest.raises(ValueError):
        ops.preprocess_u8_gather(imgs, index, out, layout=ops.IMAGES_CHW)  # [n,8,8,3] is not [n,3,H,W]
    with pytest.raises(TypeError):
        ops.preprocess_u8_gather(imgs, index.int(), out)
    with pytest.raises(ValueError):
        ops.preprocess_u8_gather(imgs, index, out, torch.zeros(3, dtype=torch.uint8, device="cuda"))


def test_preprocess_u8_keeps_its_results(case_data):
    """the original entry runs the same kernels with no index"""
    cid, n, H, W, size, index, flips = CASES[1]
    imgs, want = case_data[cid]
    assert np.array_equal(_two_launches(imgs, index, size, flips), want)


# ---- ResidentLoader ---------------------------------------------------------------------------------------
def test_resident_loader_two_epochs_match_oracle():
    from vitmi.data import ResidentLoader, epoch_order
    rng = np.random.default_rng(8)
    n, bs, size = 37, 8, 40
    chw = rng.integers(0, 256, (n, 3, 32, 32), dtype=np.uint8)
    hwc = np.ascontiguousarray(chw.transpose(0, 2, 3, 1))
    labels = rng.integers(0, 10, n)
    loader = ResidentLoader(chw, labels, bs, size, "cuda", train=True, seed=5, num_classes=10)
    assert len(loader) == 5
    g = torch.Generator().manual_seed(5)
    orders = []
    for _ in range(2):
        order = epoch_order(n, g).numpy()
        orders.append(order)
        batches = [(x.cpu().numpy(), y.cpu().numpy()) for x, y in loader]
        flips = loader.last_flips.numpy()
        assert flips.shape == (n,) and 0 < flips.sum() < n
        assert [len(y) for _, y in batches] == [8, 8, 8, 8, 5]  # the ragged batch is present
        want = transform_batch(hwc[order], size, flips)
        assert np.array_equal(np.concatenate([x for x, _ in batches]), want)
        assert np.array_equal(np.concatenate([y for _, y in batches]), labels[order])
    assert not np.array_equal(orders[0], orders[1])


def test_resident_loader_eval_is_file_order_without_flips():
    from vitmi.data import ResidentLoader
    rng = np.random.default_rng(9)
    chw = rng.integers(0, 256, (11, 3, 32, 32), dtype=np.uint8)
    labels = rng.integers(0, 10, 11)
    loader = ResidentLoader(chw, labels, 4, 40, "cuda", train=False, seed=5)
    want = transform_batch(np.ascontiguousarray(chw.transpose(0, 2, 3, 1)), 40, None)
    for _ in range(2):
        batches = list(loader)
        assert [len(y) for _, y in batches] == [4, 4, 3] and loader.last_flips is None
        assert np.array_equal(torch.cat([x for x, _ in batches]).cpu().numpy(), want)
        assert np.array_equal(torch.cat([y for _, y in batches]).cpu().numpy(), labels)


def test_resident_loader_rank_slices_make_the_global_batch():
    """two ranks' batches of a step concatenate to the one-rank batch of that step, bit for bit"""
    from vitmi.data import ResidentLoader
    rng = np.random.default_rng(10)
    chw = rng.integers(0, 256, (20, 3, 32, 32), dtype=np.uint8)
    labels = rng.integers(0, 10, 20)
    one = list(ResidentLoader(chw, labels, 8, 40, "cuda", train=True, seed=3))
    two = [list(ResidentLoader(chw, labels, 4, 40, "cuda", train=True, seed=3, world=2, rank=r)) for r in range(2)]
    assert [len(y) for _, y in one] == [8, 8, 4] and [len(y) for _, y in two[0]] == [4, 4, 2]
    for k, (x, y) in enumerate(one):
        assert torch.equal(torch.cat([two[0][k][0], two[1][k][0]]), x)
        assert torch.equal(torch.cat([two[0][k][1], two[1][k][1]]), y)


# ---- entry points -----------------------------------------------------------------------------------------
TRAIN_ARGS = ["--model-arch", "b32", "--image-size", "32", "--any-image-size", "--batch-size", "16", "--dataset",
              "CIFAR10", "--num-classes", "10", "--checkpoint-path", "", "--train-steps", "6", "--warmup-steps", "2",
              "--no-save"]
FIRST_LOSS = re.compile(r"Train Epoch: 001 Batch: 00000/00003 Loss: (\S+) ")


@pytest.fixture(scope="module")
def trees(tmp_path_factory):
    """the same 40 train / 16 test CIFAR-10 images in the python form and in the binary form"""
    root = tmp_path_factory.mktemp("cifar")
    for form in ("python", "binary"):
        write_tree(str(root / form / "CIFAR10"), "CIFAR10", form, per_train_file=8, n_test=16, seed=21)
    return root


def _train_main(data_dir):
    """(best accuracy, everything printed) of one vitmi.train run"""
    import contextlib
    import io
    from vitmi import train
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        best = train.main(TRAIN_ARGS + ["--data-dir", str(data_dir)])
    return best, buf.getvalue()


@pytest.fixture(scope="module")
def python_form_run(trees):
    return _train_main(trees / "python")


def test_train_main_runs_cifar10_from_disk(python_form_run):
    best, text = python_form_run
    assert "6 3 2" in text  # train steps, batches per epoch (16, 16, 8), epochs
    assert FIRST_LOSS.search(text) and "Train Epoch: 002 Batch: 00000/00003" in text
    assert re.search(r"epoch\s+: 2", text) and "val_acc1" in text
    assert np.isfinite(best) and 0.0 <= best <= 100.0


def test_binary_form_gives_the_same_first_step(trees, python_form_run):
    """same seed, same order, same bytes: the binary tree prints the python tree's first-step loss"""
    _, text = _train_main(trees / "binary")
    first = FIRST_LOSS.search(text).group(1)
    assert first == FIRST_LOSS.search(python_form_run[1]).group(1) and np.isfinite(float(first))


def test_eval_main_runs_cifar10_from_disk(trees, capsys):
    from vitmi import eval as vit_eval
    acc1, acc5 = vit_eval.main(["--model-arch", "b32", "--image-size", "32", "--any-image-size", "--batch-size", "16",
                                "--dataset", "CIFAR10", "--num-classes", "10", "--data-dir", str(trees / "python")])
    assert "Evaluation of model b32 on dataset CIFAR10" in capsys.readouterr().out
    assert 0.0 <= acc1 <= acc5 <= 100.0


def test_unsupported_dataset_and_missing_directory_exit_with_a_reason(trees):
    from vitmi import train
    with pytest.raises(SystemExit, match="CIFAR10 and CIFAR100"):
        train.main([a if a != "CIFAR10" else "ImageNet" for a in TRAIN_ARGS] + ["--data-dir", str(trees / "python")])
    with pytest.raises(SystemExit, match="cifar-100-python"):
        train.main([a if a != "CIFAR10" else "CIFAR100" for a in TRAIN_ARGS] + ["--data-dir", str(trees / "python")])
    with pytest.raises(SystemExit, match="--num-classes"):
        train.main([a if a != "10" else "5" for a in TRAIN_ARGS] + ["--data-dir", str(trees / "python")])


def test_resvit_train_main_runs_cifar10_from_disk(trees, capsys, monkeypatch):
    """the Res-ViT driver on the same tree, with the smallest model of its own tests (test_resvit_cpu.TINY)"""
    from test_resvit_cpu import TINY
    from vitmi import resvit, resvit_train
    monkeypatch.setenv("VITMI_EXP_STAMP", "test")

    def tiny_model(config, device):
        return resvit.Transformer(resvit.ModelArgs(**dict(TINY, device="cuda"))).to(device)

    monkeypatch.setattr(resvit_train, "build_model", tiny_model)
    best = resvit_train.main(["--image-size", "32", "--any-image-size", "--batch-size", "16", "--dataset", "CIFAR10",
                              "--data-dir", str(trees / "python"), "--checkpoint-path", "", "--train-steps", "6",
                              "--warmup-steps", "2", "--no-save"])
    text = capsys.readouterr().out
    assert "Training for 2 epochs based on 6 steps" in text and "Train Epoch: 001 Batch: 00000/00003 Acc@1" in text
    assert np.isfinite(best) and 0.0 <= best <= 100.0
