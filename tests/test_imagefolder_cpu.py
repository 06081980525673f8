"""Image folders on the host (vitmi.datasets.find_image_folder / find_tiny_imagenet / decode_rgb and
vitmi.data.loaders): the file lists follow torchvision's ImageFolder rules and res-vit/data_loaders.py:124-152,
decoding equals Pillow's convert('RGB'), and what is missing or broken is named. No GPU."""
import argparse
import os

import numpy as np
import pytest

from folder_trees import pixels, save_image, touch, write_tiny_imagenet
from vitmi import datasets
from vitmi.datasets import DatasetError


def _png(path, h=4, w=5, seed=0):
    save_image(path, pixels(h, w, seed))


def test_image_folder_rules_exact_paths_and_labels(tmp_path):
    pytest.importorskip("PIL.Image")
    root = str(tmp_path / "train")
    j = os.path.join
    # class directories created in non-sorted order; a nested directory; upper-case .JPEG; a text file to skip
    _png(j(root, "zebra", "b.png"))
    _png(j(root, "ant", "2.png"))
    save_image(j(root, "ant", "10.JPEG"), pixels(6, 6, 1))
    _png(j(root, "ant", "sub", "deep", "x.png"))
    _png(j(root, "ant", "sub", "a.bmp"))
    touch(j(root, "ant", "notes.txt"), b"skip me")
    _png(j(root, "mole", "m.png"))
    touch(j(root, "stray.png"), b"a file directly under root is no class")
    paths, labels, classes = datasets.find_image_folder(root)
    assert classes == ["ant", "mole", "zebra"]
    assert paths == [j(root, "ant", "10.JPEG"), j(root, "ant", "2.png"), j(root, "ant", "sub", "a.bmp"),
                     j(root, "ant", "sub", "deep", "x.png"), j(root, "mole", "m.png"), j(root, "zebra", "b.png")]
    assert labels.dtype == np.int64 and labels.tolist() == [0, 0, 0, 0, 1, 2]


def test_image_folder_empty_class_and_missing_root_are_errors(tmp_path):
    root = tmp_path / "train"
    touch(str(root / "ant" / "a.png"), b"x")  # listing does not decode
    touch(str(root / "bee" / "notes.txt"), b"x")
    with pytest.raises(DatasetError, match="bee"):
        datasets.find_image_folder(str(root))
    missing = tmp_path / "nowhere" / "val"
    with pytest.raises(DatasetError, match=str(missing)):
        datasets.find_image_folder(str(missing))
    assert not (tmp_path / "nowhere").exists()
    os.makedirs(tmp_path / "hollow")
    with pytest.raises(DatasetError, match="no class directories"):
        datasets.find_image_folder(str(tmp_path / "hollow"))


@pytest.mark.parametrize("val_form", ["folders", "annotations"])
def test_tiny_imagenet_both_forms(tmp_path, val_form):
    pytest.importorskip("PIL.Image")
    root = str(tmp_path / "TinyImageNet")
    train, val = write_tiny_imagenet(root, classes=("n30", "n10", "n20"), per_class=3, n_val=5, val_form=val_form)
    order = {"n10": 0, "n20": 1, "n30": 2}
    paths, labels, classes = datasets.find_tiny_imagenet(root, "train")
    assert classes == ["n10", "n20", "n30"]
    want = sorted(train, key=lambda pc: (order[pc[1]], os.path.basename(pc[0])))
    assert paths == [p for p, _ in want] and labels.tolist() == [order[c] for _, c in want]
    assert not any(p.endswith(".txt") for p in paths)
    paths, labels, _ = datasets.find_tiny_imagenet(root, "val")
    if val_form == "folders":
        want = sorted(val, key=lambda pc: (order[pc[1]], os.path.basename(pc[0])))
    else:
        want = sorted(val, key=lambda pc: os.path.basename(pc[0]))
    assert paths == [p for p, _ in want]
    assert labels.dtype == np.int64 and labels.tolist() == [order[c] for _, c in want]


def test_tiny_imagenet_missing_split_names_the_path(tmp_path):
    with pytest.raises(DatasetError, match=str(tmp_path / "TinyImageNet" / "val")):
        datasets.find_tiny_imagenet(str(tmp_path / "TinyImageNet"), "val")
    assert not (tmp_path / "TinyImageNet").exists()


def test_decode_rgb_equals_pillow_convert(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    known = pixels(7, 11, 3)
    p = str(tmp_path / "known.png")
    save_image(p, known)
    got = datasets.decode_rgb(p)
    assert got.dtype == np.uint8 and got.flags["C_CONTIGUOUS"] and np.array_equal(got, known)  # lossless
    files = {"rgb.jpg": Image.fromarray(pixels(20, 33, 4)),
             "gray.png": Image.fromarray(pixels(9, 14, 5)[:, :, 0]),
             "gray.jpg": Image.fromarray(pixels(16, 16, 6)[:, :, 1]),
             "palette.png": Image.fromarray(pixels(12, 10, 7)).convert("P", palette=Image.ADAPTIVE, colors=17),
             "rgba.png": Image.fromarray(np.dstack([pixels(8, 9, 8), pixels(8, 9, 9)[:, :, :1]]), "RGBA"),
             "cmyk.jpg": Image.fromarray(pixels(10, 10, 10)).convert("CMYK")}
    for name, im in files.items():
        path = str(tmp_path / name)
        im.save(path)
        with Image.open(path) as ref:
            want = np.asarray(ref.convert("RGB"))
        got = datasets.decode_rgb(path)
        assert got.shape == want.shape and got.shape[2] == 3 and np.array_equal(got, want), name


def test_truncated_and_foreign_files_raise_naming_the_file(tmp_path):
    pytest.importorskip("PIL.Image")
    whole = str(tmp_path / "whole.jpg")
    save_image(whole, pixels(64, 64, 11), quality=95)
    data = open(whole, "rb").read()
    cut = str(tmp_path / "cut.jpg")
    touch(cut, data[:len(data) // 3])
    with pytest.raises(DatasetError, match="cut.jpg"):
        datasets.decode_rgb(cut)
    text = str(tmp_path / "text.png")
    touch(text, b"this is not a PNG")
    with pytest.raises(DatasetError, match="text.png"):
        datasets.decode_rgb(text)
    with pytest.raises(DatasetError, match="gone.png"):
        datasets.decode_rgb(str(tmp_path / "gone.png"))


def test_decode_rgb_without_pillow_says_so(tmp_path, monkeypatch):
    import sys
    monkeypatch.setitem(sys.modules, "PIL", None)  # `from PIL import Image` now raises ImportError
    with pytest.raises(DatasetError, match="Pillow"):
        datasets.decode_rgb(str(tmp_path / "any.png"))


def _config(tmp_path, dataset):
    return argparse.Namespace(dataset=dataset, data_dir=str(tmp_path / "data"), image_size=32, seed=42,
                              num_classes=10, num_workers=2, resident_data=False, resident_gb=32.0)


@pytest.mark.parametrize("dataset", ["ImageNet", "TinyImageNet"])
def test_loaders_missing_folder_names_the_path_lists_the_forms_and_creates_nothing(tmp_path, dataset):
    from vitmi import data
    with pytest.raises(SystemExit) as e:
        data.loaders(_config(tmp_path, dataset), 4, "cpu")
    text = str(e.value)
    assert os.path.join(str(tmp_path / "data"), dataset, "train") in text
    assert "CIFAR10 and CIFAR100" in text and "ImageNet" in text and "TinyImageNet" in text
    assert "val_annotations.txt" in text
    assert not (tmp_path / "data").exists()


def test_loaders_unknown_name_lists_the_forms(tmp_path):
    from vitmi import data
    with pytest.raises(SystemExit, match="CIFAR10 and CIFAR100"):
        data.loaders(_config(tmp_path, "MNIST"), 4, "cpu")


def test_loaders_on_a_cifar_name_still_returns_resident_loaders(tmp_path, monkeypatch):
    """with a stub load_cifar and a stub upload: the CIFAR path is cifar_loaders', unchanged"""
    import torch
    from vitmi import data
    calls = []

    def load_cifar(root, name, train=True):
        calls.append((root, name, train))
        n = 12 if train else 5
        return np.zeros((n, 3, 32, 32), np.uint8), np.arange(n) % 10, None

    monkeypatch.setattr(datasets, "load_cifar", load_cifar)
    monkeypatch.setattr(torch.Tensor, "to", lambda self, *a, **k: self)  # no device here
    train, test = data.loaders(_config(tmp_path, "CIFAR10"), 4, "cpu")
    assert type(train) is data.ResidentLoader and type(test) is data.ResidentLoader
    root = os.path.join(str(tmp_path / "data"), "CIFAR10")
    assert calls == [(root, "CIFAR10", True), (root, "CIFAR10", False)]
    assert len(train) == 3 and len(test) == 2 and train.plan.train and not test.plan.train
