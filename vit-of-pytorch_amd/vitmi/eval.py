"""Evaluation entry point, mirroring reference src/eval.py:12-77 on the MI355X HIP engine.

    python -m vitmi.eval --model-arch b16 --image-size 384 --checkpoint-path w.pth --synthetic

Same flow as the reference: get_eval_config (src/config.py:5-25, default 384 px, 1000 classes) ->
set_seed -> VisionTransformer -> load_checkpoint (.pth / JAX .npz) -> forward over the val split
under torch.no_grad() -> mean top-1 / top-5 over batches, printed in the reference's format.
Top-1 / top-5 come from the fused cross-entropy kernel's per-row hit counts (vit_cross_entropy,
src/utils.py:28-41 semantics) instead of a topk pass. Sequences above 320 tokens (384 px: 577 for
B/16 and L/16, 730 for H/14) run the K/V-tiled attention kernels. `--precision fp32` evaluates with
the reference's own f32 arithmetic (vit_gemm_f32 projections, f32 attention). `--use-ema` evaluates the weight EMA
of a vitmi.train checkpoint written with --ema-decay (its "state_dict_ema"); a file without one stops the run with one
line naming it.
Data: `--dataset CIFAR10|CIFAR100 --data-dir D` evaluates the test split read from disk and kept in HBM
(vitmi.datasets, vitmi.data.ResidentLoader), in file order; `--synthetic` a synthetic split, as in
vitmi.train. `--dataset ImageNet` (the default) evaluates the image folder D/ImageNet/val/<class>/..., and
`--dataset TinyImageNet` D/TinyImageNet/val in either of its forms (vitmi.datasets), in file order: the files are
decoded on the host with Pillow, --num-workers threads at a time, while the device works on the batch before, and
every image, whatever its size, is resized to --image-size on the device (vitmi.data.FolderLoader).

    python -m vitmi.eval --model-arch b16 --image-size 224 --dataset CIFAR100 --num-classes 100 \\
        --data-dir ../data --checkpoint-path ft.pth
    python -m vitmi.eval --model-arch b16 --image-size 384 --dataset ImageNet --data-dir ../data \\
        --checkpoint-path ../weights/pytorch/imagenet21k+imagenet2012_ViT-B_16-384.pth
"""
from __future__ import annotations

import sys

import numpy as np
import torch

from . import ops
from .checkpoint import load_checkpoint_ema
from .config import get_eval_config
from .train import SyntheticDataLoader, build_model, fit_pos_embedding, load_checkpoint, set_seed


def evaluate(model, data_loader, device):
    """Mean top-1 / top-5 (%) over batches (src/eval.py:56-75)."""
    acc1s, acc5s = [], []
    model.eval()
    with torch.no_grad():
        for data, target in data_loader:
            data = data.to(device)
            target = target.to(device, torch.int64)
            logits = model(data).float().contiguous()
            st = torch.empty(logits.shape[0], 3, device=device)
            ops.cross_entropy(logits, target.contiguous(), None, 1.0, st)
            acc1s.append(st[:, 1].mean() * 100.0)
            acc5s.append(st[:, 2].mean() * 100.0)
    return float(torch.stack(acc1s).mean()), float(torch.stack(acc5s).mean())


def main(argv=None):
    config = get_eval_config(argv)
    set_seed(config.seed)
    ema_state = None
    if config.use_ema:
        # read first: a checkpoint without EMA weights stops the run with one line, before anything else is set up
        if not config.checkpoint_path:
            raise SystemExit("--use-ema needs --checkpoint-path")
        try:
            ema_state = load_checkpoint_ema(config.checkpoint_path)
        except ValueError as e:
            raise SystemExit(str(e)) from None
    if not torch.cuda.is_available():
        raise SystemExit("vitmi.eval needs a ROCm GPU (MI355X)")
    device = torch.device("cuda", 0)
    data_loader = None
    if not config.synthetic:
        # the reference's {dataset}DataLoader(split='val') (src/eval.py:44-50): the test split, in file order; read
        # before the model is built, so that a missing dataset stops the run at once
        from .data import loaders
        data_loader, = loaders(config, config.batch_size, device, splits=("test",))
    model = build_model(config, device)
    if config.checkpoint_path:
        state_dict = load_checkpoint(config.checkpoint_path) if ema_state is None else ema_state
        model.load_state_dict(fit_pos_embedding(state_dict, model, config))
        print("Load {} weights from {}".format("pretrained" if ema_state is None else "EMA", config.checkpoint_path))
    model = model.to(device)
    model.precision = config.precision
    if data_loader is None:
        data_loader = SyntheticDataLoader(config.batch_size, config.image_size, config.num_classes,
                                          config.steps_per_epoch, device, seed=config.seed)
    print("Starting evaluation")
    acc1, acc5 = evaluate(model, data_loader, device)
    print("Evaluation of model {:s} on dataset {:s}, Acc@1: {:.4f}, Acc@5: {:.4f}".format(
        config.model_arch, config.dataset, acc1, acc5))
    return acc1, acc5


if __name__ == "__main__":
    main(sys.argv[1:])
