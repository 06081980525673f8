"""vitmi.data.FolderLoader (image files of mixed sizes -> one vit_preprocess_u8_ragged launch per batch) and the
entry points on image-folder trees. The mechanics are checked with a decoder that needs no Pillow, bit-exactly
against the Pillow-pinned oracle in EpochPlan's order and flips; the drivers run on small trees written with
Pillow at test time."""
import re
import threading

import numpy as np
import pytest
import torch

from folder_trees import fake_decode, write_image_folder, write_tiny_imagenet
from oracle.preprocess import resize_bilinear_u8, to_tensor_normalize

pytestmark = pytest.mark.gpu

N, BATCH, OUT = 23, 4, (16, 24)
PATHS = [f"/nowhere/class_{i % 5}/img_{i:03d}.JPEG" for i in range(N)]
LABELS = np.arange(N) % 5


@pytest.fixture(scope="module")
def resized():
    """the oracle's resize of every fake image, computed once and left unchanged"""
    return [resize_bilinear_u8(fake_decode(p), *OUT) for p in PATHS]


def _loader(**kw):
    from vitmi.data import FolderLoader
    args = dict(batch_size=BATCH, image_size=OUT, device="cuda", train=True, seed=7, num_classes=5, workers=3,
                decode=fake_decode)
    args.update(kw)
    return FolderLoader(PATHS, LABELS, **args)


def _epoch(loader):
    return [(x.cpu().numpy(), y.cpu().numpy()) for x, y in loader]


def _threads():
    return {t.name for t in threading.enumerate() if t.name.startswith("vitmi-")}


def test_fake_decode_sizes_span_the_range():
    shapes = [fake_decode(p).shape for p in PATHS]
    assert all(3 <= h <= 40 and 5 <= w <= 70 for h, w, _ in shapes) and len(set(shapes)) > 10


@pytest.mark.parametrize("train", [True, False])
def test_streaming_and_resident_yield_the_oracle_batches_for_two_epochs(resized, train):
    from vitmi.data import EpochPlan
    stream, resident = _loader(train=train), _loader(train=train, resident=True)
    plan = EpochPlan(N, BATCH, train, seed=7)
    assert len(stream) == len(resident) == len(plan) == 6
    for _ in range(2):
        order, flips = plan.next_epoch()
        a, b = _epoch(stream), _epoch(resident)
        assert len(a) == len(b) == 6 and a[-1][0].shape == (3, 3) + OUT  # the ragged last batch of 3
        for (s, e), (xa, ya), (xb, yb) in zip(plan.slices(), a, b):
            idx = order[s:e].tolist()
            want = np.stack([to_tensor_normalize(resized[i][:, ::-1] if flips is not None and flips[s + k] else
                                                 resized[i]) for k, i in enumerate(idx)])
            assert np.array_equal(xa, want) and np.array_equal(xb, want), (s, e)
            assert np.array_equal(ya, LABELS[idx]) and np.array_equal(yb, LABELS[idx])
        assert stream.data_wait_s >= 0.0 and resident.data_wait_s == 0.0
    assert not _threads()


@pytest.mark.parametrize("resident", [False, True])
def test_world_2_slices_concatenate_to_the_world_1_batch(resident):
    whole = _epoch(_loader(batch_size=4, resident=resident))
    halves = [_epoch(_loader(batch_size=2, world=2, rank=r, resident=resident)) for r in range(2)]
    # 23 = 5 * 4 + 3: the ragged 3 do not divide over 2 ranks and are skipped there
    assert len(whole) == 6 and len(halves[0]) == len(halves[1]) == 5
    for k in range(5):
        assert np.array_equal(np.concatenate([halves[0][k][0], halves[1][k][0]]), whole[k][0])
        assert np.array_equal(np.concatenate([halves[0][k][1], halves[1][k][1]]), whole[k][1])


def test_a_decode_failure_surfaces_as_the_same_error_and_leaves_no_thread():
    from vitmi.datasets import DatasetError
    bad = PATHS[9]
    error = DatasetError(f"{bad}: cannot be decoded")

    def decode(path):
        if path == bad:
            raise error
        return fake_decode(path)

    seen = 0
    with pytest.raises(DatasetError) as e:
        for _ in _loader(train=False, decode=decode):
            seen += 1
    assert e.value is error and seen <= 2  # file order: the third batch holds sample 9
    assert not _threads()
    with pytest.raises(DatasetError) as e:
        _loader(train=False, decode=decode, resident=True)
    assert e.value is error and not _threads()


def test_leaving_the_loop_early_leaves_no_thread():
    it = iter(_loader())
    next(it)
    it.close()
    assert not _threads()


def test_bad_decoder_output_and_resident_limit_are_refused():
    from vitmi.datasets import DatasetError
    with pytest.raises(DatasetError, match="uint8"):
        _epoch(_loader(decode=lambda p: np.zeros((4, 4, 3), np.float32)))
    with pytest.raises(DatasetError, match="--resident-data"):
        _loader(resident=True, resident_gb=1e-6)
    assert not _threads()


# ---------------------------------------------------------------------------------------------------------
# the drivers, with Pillow


@pytest.fixture(scope="module")
def data_dir(tmp_path_factory):
    pytest.importorskip("PIL.Image")
    root = tmp_path_factory.mktemp("folders")
    write_image_folder(str(root / "ImageNet" / "val"), per_class=4, seed=1)
    write_image_folder(str(root / "ImageNet" / "train"), per_class=4, seed=2)
    write_tiny_imagenet(str(root / "TinyImageNet"), per_class=4, n_val=6, seed=3, val_form="annotations")
    return root


def test_eval_main_runs_an_imagenet_folder(data_dir, capsys):
    from vitmi import eval as vit_eval
    acc1, acc5 = vit_eval.main(["--model-arch", "b32", "--image-size", "32", "--any-image-size", "--batch-size", "8",
                                "--dataset", "ImageNet", "--num-classes", "3", "--num-workers", "4", "--data-dir",
                                str(data_dir)])
    assert "Evaluation of model b32 on dataset ImageNet" in capsys.readouterr().out
    assert 0.0 <= acc1 <= acc5 <= 100.0
    assert not _threads()


TINY_ARGS = ["--model-arch", "b32", "--image-size", "32", "--any-image-size", "--batch-size", "4", "--dataset",
             "TinyImageNet", "--num-classes", "3", "--checkpoint-path", "", "--train-steps", "6", "--warmup-steps", "2",
             "--no-save", "--num-workers", "4"]
FIRST_LOSS = re.compile(r"Train Epoch: 001 Batch: 00000/00003 Loss: (\S+) ")


def test_train_main_runs_tiny_imagenet_and_reports_the_wait(data_dir, capsys, monkeypatch):
    from vitmi import train
    monkeypatch.setenv("VITMI_EXP_STAMP", "test")
    best = train.main(TINY_ARGS + ["--data-dir", str(data_dir)])
    text = capsys.readouterr().out
    loss = float(FIRST_LOSS.search(text).group(1))
    assert np.isfinite(loss) and np.isfinite(best)
    assert re.search(r"Train Epoch: 001 data_wait_s: \d+\.\d+", text)


def test_first_step_loss_is_the_same_streaming_and_resident(data_dir, capsys, monkeypatch):
    from vitmi import train
    monkeypatch.setenv("VITMI_EXP_STAMP", "test")
    args = [a if a != "TinyImageNet" else "ImageNet" for a in TINY_ARGS] + ["--data-dir", str(data_dir)]
    train.main(args)
    streaming = FIRST_LOSS.search(capsys.readouterr().out).group(1)
    train.main(args + ["--resident-data"])
    resident = FIRST_LOSS.search(capsys.readouterr().out).group(1)
    assert streaming == resident and np.isfinite(float(streaming))
    assert not _threads()
