"""vitmi.datasets (CIFAR-10/100 parsed from disk, both published forms, restricted unpickling) and the host
side of vitmi.data.ResidentLoader: the sample order against torch.utils.data.DataLoader itself, the
data-parallel slicing plan, the label check. No GPU, no library."""
import os
import pickle

import numpy as np
import pytest
import torch

from cifar_trees import BIN_DIR, PY_DIR, write_tree


@pytest.mark.parametrize("name", ["CIFAR10", "CIFAR100"])
@pytest.mark.parametrize("form", ["python", "binary"])
def test_readers_round_trip(tmp_path, name, form):
    from vitmi.datasets import load_cifar
    root = str(tmp_path / name)
    want = write_tree(root, name, form, per_train_file=4, n_test=6, seed=3)
    for split, n in (("train", 20 if name == "CIFAR10" else 4), ("test", 6)):
        images, labels, names = load_cifar(root, name, train=split == "train")
        data, lab = want[split]
        assert images.dtype == np.uint8 and images.shape == (n, 3, 32, 32)
        assert labels.dtype == np.int64 and labels.shape == (n,)
        assert np.array_equal(images.reshape(n, 3072), data)  # planar bytes as stored, file order
        assert np.array_equal(labels, lab)  # CIFAR-100: the fine label (the coarse ones all differ)
        assert names == [f"class{i}" for i in range(10 if name == "CIFAR10" else 100)]


def test_class_names_optional(tmp_path):
    from vitmi.datasets import load_cifar
    write_tree(str(tmp_path), "CIFAR10", "binary", meta=False)
    assert load_cifar(str(tmp_path), "CIFAR10", train=False)[2] is None


def test_python_form_preferred_and_binary_found(tmp_path):
    """whichever form is present under root is read"""
    from vitmi.datasets import load_cifar
    a = write_tree(str(tmp_path / "a"), "CIFAR100", "binary", seed=1)
    b = write_tree(str(tmp_path / "b"), "CIFAR100", "python", seed=2)
    assert np.array_equal(load_cifar(str(tmp_path / "a"), "CIFAR100", True)[1], a["train"][1])
    assert np.array_equal(load_cifar(str(tmp_path / "b"), "CIFAR100", True)[1], b["train"][1])


class _Evil:
    def __init__(self, path):
        self.path = path

    def __reduce__(self):
        return (os.system, (f"touch {self.path}",))


def test_pickle_naming_another_global_is_refused_without_side_effect(tmp_path):
    from vitmi.datasets import load_cifar
    root = str(tmp_path)
    write_tree(root, "CIFAR10", "python")
    marker = tmp_path / "ran"
    with open(os.path.join(root, PY_DIR["CIFAR10"], "data_batch_3"), "wb") as f:
        pickle.dump({"data": _Evil(str(marker)), "labels": [0]}, f, protocol=2)
    with pytest.raises(pickle.UnpicklingError, match="system"):
        load_cifar(root, "CIFAR10", train=True)
    assert not marker.exists()
    load_cifar(root, "CIFAR10", train=False)  # the untouched test file still loads


def test_truncated_binary_is_refused(tmp_path):
    from vitmi.datasets import DatasetError, load_cifar
    root = str(tmp_path)
    write_tree(root, "CIFAR100", "binary")
    path = os.path.join(root, BIN_DIR["CIFAR100"], "train.bin")
    with open(path, "r+b") as f:
        f.truncate(os.path.getsize(path) - 5)
    with pytest.raises(DatasetError, match="train.bin"):
        load_cifar(root, "CIFAR100", train=True)


def test_wrong_record_width_is_refused(tmp_path):
    from vitmi.datasets import DatasetError, load_cifar
    root = str(tmp_path)
    write_tree(root, "CIFAR10", "python")
    with open(os.path.join(root, PY_DIR["CIFAR10"], "test_batch"), "wb") as f:
        pickle.dump({"data": np.zeros((2, 3071), np.uint8), "labels": [0, 1]}, f, protocol=2)
    with pytest.raises(DatasetError, match="3072"):
        load_cifar(root, "CIFAR10", train=False)


def test_missing_directory_names_the_paths_tried(tmp_path):
    from vitmi.datasets import DatasetError, load_cifar
    with pytest.raises(DatasetError) as e:
        load_cifar(str(tmp_path / "nowhere"), "CIFAR10", train=True)
    assert "cifar-10-batches-py" in str(e.value) and "cifar-10-batches-bin" in str(e.value)
    assert not (tmp_path / "nowhere").exists()  # nothing created, nothing downloaded


@pytest.mark.parametrize("name", ["ImageNet", "TinyImageNet"])
def test_other_datasets_say_what_is_supported(tmp_path, name):
    from vitmi.datasets import DatasetError, load_cifar
    with pytest.raises(DatasetError, match="CIFAR10 and CIFAR100"):
        load_cifar(str(tmp_path), name, train=True)


@pytest.mark.parametrize("seed", [0, 42])
@pytest.mark.parametrize("n,batch", [(1, 1), (23, 4), (64, 16)])
def test_epoch_order_is_the_seeded_dataloader_order(n, batch, seed):
    from torch.utils.data import DataLoader, TensorDataset
    from vitmi.data import epoch_order
    loader = DataLoader(TensorDataset(torch.arange(n)), batch_size=batch, shuffle=True,
                        generator=torch.Generator().manual_seed(seed))
    g = torch.Generator().manual_seed(seed)
    for _ in range(3):
        want = torch.cat([b for b, in loader])
        got = epoch_order(n, g)
        assert got.dtype == torch.int64 and torch.equal(got, want)


def test_data_parallel_slices_concatenate_to_the_global_batch():
    from vitmi.data import EpochPlan
    n, g = 70, 16
    one = EpochPlan(n, g, train=True, seed=7, world=1, rank=0)
    assert len(one) == 5 and one.slices()[-1] == (64, 70) and one.skipped == 0  # the ragged 6 is kept
    epochs = [one.next_epoch() for _ in range(2)]
    assert all(0 < int(f.sum()) < n for _, f in epochs)
    assert sorted(epochs[0][0].tolist()) == list(range(n)) and not torch.equal(epochs[0][0], epochs[1][0])
    for world in (2, 4):
        plans = [EpochPlan(n, g // world, train=True, seed=7, world=world, rank=r) for r in range(world)]
        assert all(len(p) == (5 if world == 2 else 4) for p in plans)  # 6 = 2 * 3 is kept, 6 % 4 is skipped
        assert all(p.skipped == (0 if world == 2 else 6) for p in plans)
        for order1, flips1 in epochs:
            per_rank = [p.next_epoch() for p in plans]
            for o, f in per_rank:  # every rank computes the same global order and flips
                assert torch.equal(o, order1) and torch.equal(f, flips1)
            for k in range(len(plans[0])):
                s, e = one.slices()[k]
                idx = torch.cat([o[slice(*p.slices()[k])] for p, (o, _) in zip(plans, per_rank)])
                flp = torch.cat([f[slice(*p.slices()[k])] for p, (_, f) in zip(plans, per_rank)])
                assert torch.equal(idx, order1[s:e]) and torch.equal(flp, flips1[s:e]), (world, k)


def test_eval_plan_is_file_order_without_flips():
    from vitmi.data import EpochPlan
    p = EpochPlan(10, 4, train=False, seed=1)
    for _ in range(2):
        order, flips = p.next_epoch()
        assert torch.equal(order, torch.arange(10)) and flips is None
    assert p.slices() == [(0, 4), (4, 8), (8, 10)]


def test_flip_stream_is_separate_from_the_order_stream():
    """flips come from their own generator: the order is the reference's whatever is drawn for the flips"""
    from vitmi.data import EpochPlan, epoch_order
    p = EpochPlan(33, 8, train=True, seed=11)
    g = torch.Generator().manual_seed(11)
    for _ in range(2):
        assert torch.equal(p.next_epoch()[0], epoch_order(33, g))


@pytest.mark.parametrize("bad", [10, -1])
def test_label_out_of_range_names_num_classes(bad):
    from vitmi.data import check_labels
    labels = np.array([0, 9, bad, 3])
    with pytest.raises(ValueError, match="--num-classes"):
        check_labels(labels, 10)
    assert check_labels(np.array([0, 9]), 10).dtype == torch.int64


def test_resident_loader_checks_labels_before_touching_the_device():
    from vitmi.data import ResidentLoader
    with pytest.raises(ValueError, match="--num-classes"):
        ResidentLoader(np.zeros((3, 3, 32, 32), np.uint8), [0, 1, 100], 2, 32, "cuda", train=True, seed=0,
                       num_classes=100)
