"""Gradient accumulation in the training driver, host side only: the micro-batches of an optimizer step are the samples
of the full batch (vitmi.data.EpochPlan cuts contiguous slices), the step's loss weights, and the two new flags."""
import math

import pytest
import torch

from vitmi import train
from vitmi.config import get_train_config
from vitmi.data import EpochPlan


def test_micro_slices_concatenate_to_the_full_batch():
    """n = 48, batch 8 against micro-batch 4 (K = 2), the same seed, two epochs: slices 2s and 2s + 1 of the micro plan
    together are slice s of the full plan, and the order and the flips are the same arrays"""
    full, micro = EpochPlan(n=48, batch_size=8, seed=7), EpochPlan(n=48, batch_size=4, seed=7)
    assert len(full) == 6 and len(micro) == 12
    for _ in range(2):
        (fo, ff), (mo, mf) = full.next_epoch(), micro.next_epoch()
        assert torch.equal(fo, mo) and torch.equal(ff, mf)
        fs, ms = full.slices(), micro.slices()
        for s, (a, b) in enumerate(fs):
            (a0, b0), (a1, b1) = ms[2 * s], ms[2 * s + 1]
            assert (a0, b1) == (a, b) and b0 == a1
            assert torch.equal(torch.cat([mo[a0:b0], mo[a1:b1]]), fo[a:b])
            assert torch.equal(torch.cat([mf[a0:b0], mf[a1:b1]]), ff[a:b])
    assert sorted(fo.tolist()) == list(range(48))


def test_step_weights():
    assert train.accum_weights([4, 4]) == [0.5, 0.5]
    w = train.accum_weights([4, 2])
    assert w == [4 / 6, 2 / 6] and math.isclose(sum(w), 1.0)


def test_steps_in_epoch_is_the_ceiling():
    assert [train.steps_in_epoch(range(n), 4) for n in (1, 4, 5, 8)] == [1, 1, 2, 2]
    assert train.steps_in_epoch(range(7), 1) == 7


BASE = ["--synthetic", "--no-save", "--checkpoint-path", ""]


def test_batch_must_divide_into_the_micro_batches(capsys):
    with pytest.raises(SystemExit) as e:
        get_train_config(BASE + ["--batch-size", "10", "--accum-steps", "4"])
    msg = str(e.value)
    assert "--batch-size 10" in msg and "--accum-steps 4" in msg and "divide" in msg
    with pytest.raises(SystemExit):
        train.micro_batch(10, 4, 1)
    with pytest.raises(SystemExit):
        train.micro_batch(16, 4, 8)
    assert train.micro_batch(512, 8, 1) == 64 and train.micro_batch(512, 8, 2) == 32


def test_accum_steps_1_leaves_the_config_as_it_was(capsys, monkeypatch):
    monkeypatch.setenv("VITMI_EXP_STAMP", "stamp")
    plain = vars(get_train_config(BASE + ["--batch-size", "32"]))
    one = vars(get_train_config(BASE + ["--batch-size", "32", "--accum-steps", "1", "--clip-grad-norm", "0"]))
    assert plain == one
    assert plain["accum_steps"] == 1 and plain["clip_grad_norm"] == 0.0
    k8 = vars(get_train_config(BASE + ["--batch-size", "512", "--accum-steps", "8", "--clip-grad-norm", "1"]))
    assert (k8["batch_size"], k8["accum_steps"], k8["clip_grad_norm"]) == (512, 8, 1.0)
    assert {k: v for k, v in k8.items() if k not in ("batch_size", "accum_steps", "clip_grad_norm") and
            not k.endswith("_dir")} == \
           {k: v for k, v in plain.items() if k not in ("batch_size", "accum_steps", "clip_grad_norm") and
            not k.endswith("_dir")}
