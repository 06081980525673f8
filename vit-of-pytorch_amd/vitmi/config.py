"""Command-line configuration, mirroring reference src/config.py.

Same flags, defaults and architecture presets (get_b16_config ... get_h14_config,
src/config.py:57-104). Additions for the MI355X path, all optional:
  --synthetic            synthetic N(0,1) images / uniform labels instead of torchvision datasets
  --steps-per-epoch      batches per synthetic epoch
  --synthetic-source-size  >0: synthetic uint8 HWC images of this size, resized / flipped /
                         normalised on the device like the reference's CIFAR transform (vitmi.data)
  --any-image-size       lift the reference's choices=[224, 384] on --image-size (src/config.py:37)
  --image-size HxW       a rectangular input such as 224x384 (needs --any-image-size); config.image_size is then the
                         pair (224, 384); a plain int stays an int
  --resize-pos-embedding resample a checkpoint's position table to the model's patch grid when they differ
                         (vitmi.checkpoint.resize_pos_embedding)
  --no-save              do not create experiments/ directories or checkpoints
  --precision            (eval) bf16 MFMA forward (default) or the reference's f32 arithmetic
  --accum-steps K        (train) every optimizer step as K micro-batches of batch / (K * n_gpu) images, gradients
                         accumulated in the kernels; --batch-size stays the batch of one optimizer step
  --clip-grad-norm X     (train) clip the step's gradient to global 2-norm X (0: off)
  --random-resized-crop  (train, ImageNet / TinyImageNet) torchvision's RandomResizedCrop in place of Resize, inside the
                         ragged transform launch; --crop-scale LO HI (0.08 1.0) and --crop-ratio LO HI (0.75 1.3333)
  --label-smoothing E    (train) cross entropy against (1-E) target + E/C; validation stays plain
  --mixup-alpha A, --cutmix-alpha A   (train) Mixup / CutMix per batch, lambda ~ Beta(A, A) (vitmi.augment.BatchMixer);
                         --mix-prob P (1.0) mixes a batch with probability P, --mix-switch-prob S (0.5) picks CutMix
                         with probability S when both alphas are set
  --optimizer sgd|adamw  (train) sgd (default): momentum 0.9, the reference's fine-tune. adamw: vitmi.optim.EngineAdamW,
                         one launch over the engine's flat buffer; --beta1 0.9 --beta2 0.999 --adam-eps 1e-8; --wd is
                         its decoupled weight decay, applied to the weight matrices only (timm's rule: not to biases,
                         LayerNorms, the position table, cls_token) unless --decay-all
  --lr-schedule onecycle|cosine|auto   (train) cosine: linear warm-up over --warmup-steps, then cosine decay to 0 at
                         --train-steps (vitmi.optim.get_cosine_schedule_with_warmup), stepped per optimizer step.
                         auto (default): onecycle for sgd, cosine for adamw; onecycle with adamw is refused
  --ema-decay D          (train) exponential moving average of the weights, ema = D ema + (1-D) w once per optimizer
                         step (0: off); each epoch also validates the EMA weights (val_ema_*) and the checkpoint gains
                         "state_dict_ema"
  --use-ema              (eval) evaluate the checkpoint's "state_dict_ema"
  --drop-path-rate R     (train) stochastic depth with timm's semantics (drop_path, scale_by_keep, linear depth rule):
                         layer i of L drops each residual branch per sample with probability R i / (L - 1), fused into
                         the residual GEMM epilogues; the cls-only last layer is off with it (0: off)

Without --synthetic, the reference's own commands run on CIFAR read from disk (vitmi.datasets, vitmi.data):
    python -m vitmi.train --dataset CIFAR100 --num-classes 100 --data-dir ../data --checkpoint-path w.pth ...
    python -m vitmi.eval  --dataset CIFAR100 --num-classes 100 --data-dir ../data --checkpoint-path ft.pth ...
  --dataset CIFAR10 | CIFAR100 | ImageNet | TinyImageNet
  --data-dir D           the files live under D/<dataset>/ as src/train.py:135 joins it, in either published form:
                           cifar-10-batches-py/{data_batch_1..5,test_batch}   cifar-100-python/{train,test}
                           cifar-10-batches-bin/{data_batch_1..5,test_batch}.bin   cifar-100-binary/{train,test}.bin
                         nothing is downloaded; a missing directory is an error naming the paths tried
  --num-workers          CIFAR: accepted and unused (the set is resident in HBM and transformed there, one launch per
                         batch). Image folders: the threads that decode files, at most 16 (no worker processes)
  --seed                 seeds the sample order, which is the reference's DataLoader(shuffle=True,
                         generator=manual_seed(seed)) order epoch after epoch, and, through a second generator, the
                         flips. The flips follow the reference's rule (rand < 0.5 per sample) but not its draws: it
                         makes them inside its worker processes, whose streams depend on --num-workers
ImageNet and TinyImageNet are image folders (vitmi.datasets.find_image_folder / find_tiny_imagenet): the files are
decoded on the host with Pillow, as the reference's loader does, and resized on the device, whatever their sizes, by
one launch per batch (vit_preprocess_u8_ragged), to the pair (h, w) of --image-size (the reference's Resize((s, s))):
                           D/ImageNet/{train,val}/<class>/**/<image files>          (torchvision ImageFolder's rules)
                           D/TinyImageNet/{train,val}/<class>/images/<files>, or the published val/images/ +
                           val/val_annotations.txt
  --resident-data        decode the whole split once and keep it in HBM (TinyImageNet's default); without it ImageNet
                         streams: a thread decodes the next batches while the step runs
  --resident-gb G        refuse a resident split larger than G GB (default 32)
  --n-gpu k              every rank takes its contiguous slice of each global batch (DataParallel's scatter); a ragged
                         last global batch is kept for k = 1, split when k divides it, otherwise skipped (one line
                         says how many images per epoch that leaves out)
"""
from __future__ import annotations

import argparse
import json
import os
from datetime import datetime


def _add_common(parser, train: bool):
    parser.add_argument("--n-gpu", type=int, default=1,
                        help="number of gpus to use (one rank per GPU; --batch-size is the global batch)")
    parser.add_argument("--model-arch", type=str, default="b16", help="model setting to use",
                        choices=["b16", "b32", "l16", "l32", "h14"])
    parser.add_argument("--batch-size", type=int, default=32, help="batch size")
    parser.add_argument("--data-dir", type=str, default="../data", help="data folder")
    parser.add_argument("--num-classes", type=int, default=100 if train else 1000, help="number of classes in dataset")
    parser.add_argument("--seed", type=int, default=42, help="random seed for reproducibility")
    parser.add_argument("--synthetic", default=False, action="store_true", help="synthetic data (MI355X benchmark)")
    parser.add_argument("--steps-per-epoch", type=int, default=100, help="batches per synthetic epoch")
    parser.add_argument("--synthetic-source-size", type=int, default=0,
                        help="synthetic uint8 images of this size through the device transform (0: f32 N(0,1))")
    parser.add_argument("--any-image-size", default=False, action="store_true", help="allow any --image-size")
    parser.add_argument("--resident-data", default=False, action="store_true",
                        help="image folders: decode the split once and keep it in HBM instead of streaming it")
    parser.add_argument("--resident-gb", type=float, default=32.0,
                        help="image folders: the largest decoded split --resident-data may hold, in GB")


def _image_size(text):
    """'224' -> 224, '224x384' -> (224, 384)"""
    try:
        if "x" in text.lower():
            h, w = text.lower().split("x")
            return int(h), int(w)
        return int(text)
    except ValueError:
        raise argparse.ArgumentTypeError(f"{text!r}: expected an int or HxW, such as 224 or 224x384") from None


def image_hw(image_size):
    """(h, w) of config.image_size: an int (square) or an (h, w) pair"""
    return (image_size, image_size) if isinstance(image_size, int) else tuple(image_size)


def _image_size_arg(parser, default):
    parser.add_argument("--image-size", type=_image_size, default=default,
                        help="input image size: an int, or HxW with --any-image-size")
    parser.add_argument("--resize-pos-embedding", default=False, action="store_true",
                        help="resample the checkpoint's position embeddings to this model's patch grid")


def get_eval_config(argv=None):
    """reference src/config.py:5-25"""
    parser = argparse.ArgumentParser("Visual Transformer Evaluation")
    _add_common(parser, train=False)
    parser.add_argument("--checkpoint-path", type=str, default=None, help="model checkpoint to load weights")
    _image_size_arg(parser, 384)
    parser.add_argument("--num-workers", type=int, default=8,
                        help="image folders: decode threads, at most 16; unused for CIFAR (resident in HBM)")
    parser.add_argument("--dataset", type=str, default="ImageNet", help="dataset for fine-tunning/evaluation")
    parser.add_argument("--precision", type=str, default="bf16", choices=["bf16", "fp32"],
                        help="bf16 MFMA forward or the reference's f32 arithmetic")
    parser.add_argument("--use-ema", default=False, action="store_true",
                        help="evaluate the checkpoint's EMA weights (state_dict_ema, saved by --ema-decay runs)")
    config = parser.parse_args(argv)
    _check_image_size(config)
    config = globals()["get_{}_config".format(config.model_arch)](config)
    print_config(config)
    return config


def get_train_config(argv=None):
    """reference src/config.py:28-54"""
    parser = argparse.ArgumentParser("Visual Transformer Train/Fine-tune")
    _add_common(parser, train=True)
    parser.add_argument("--exp-name", type=str, default="ft", help="experiment name")
    parser.add_argument("--swanlab", default=False, action="store_true", help="flag of turning on swanlab")
    parser.add_argument("--checkpoint-path", type=str,
                        default="../weights/pytorch/imagenet21k+imagenet2012_ViT-B_16-224.pth",
                        help="model checkpoint to load weights")
    _image_size_arg(parser, 224)
    parser.add_argument("--num-workers", type=int, default=1,
                        help="image folders: decode threads, at most 16; unused for CIFAR (resident in HBM)")
    parser.add_argument("--train-steps", type=int, default=15000, help="number of training/fine-tunning steps")
    parser.add_argument("--lr", type=float, default=0.03, help="learning rate")
    parser.add_argument("--wd", type=float, default=0.0, help="weight decay")
    parser.add_argument("--warmup-steps", type=int, default=500, help="learning rate warm up steps")
    parser.add_argument("--dataset", type=str, default="CIFAR100", help="dataset for fine-tunning/evaluation")
    parser.add_argument("--no-save", default=False, action="store_true", help="no experiment dirs / checkpoints")
    parser.add_argument("--accum-steps", type=int, default=1,
                        help="micro-batches per optimizer step (gradient accumulation); --batch-size stays the "
                             "batch of one optimizer step")
    parser.add_argument("--clip-grad-norm", type=float, default=0.0,
                        help="clip the gradient to this global 2-norm before each update (0: off)")
    add_augment_args(parser, mixing=True)
    parser.add_argument("--optimizer", type=str, default="sgd", choices=["sgd", "adamw"],
                        help="sgd: momentum 0.9 (the reference's fine-tune); adamw: vitmi.optim.EngineAdamW")
    parser.add_argument("--beta1", type=float, default=0.9, help="adamw: beta1")
    parser.add_argument("--beta2", type=float, default=0.999, help="adamw: beta2")
    parser.add_argument("--adam-eps", type=float, default=1e-8, help="adamw: eps")
    parser.add_argument("--decay-all", default=False, action="store_true",
                        help="adamw: decay every parameter (default: not the biases, LayerNorms, position table, cls)")
    parser.add_argument("--lr-schedule", type=str, default="auto", choices=["onecycle", "cosine", "auto"],
                        help="auto: onecycle for sgd, cosine (linear warm-up, cosine decay to 0) for adamw")
    parser.add_argument("--ema-decay", type=float, default=0.0,
                        help="keep an exponential moving average of the weights with this decay (0: off)")
    parser.add_argument("--drop-path-rate", type=float, default=0.0,
                        help="stochastic depth: the last layer's drop-path rate, linear from 0 over the layers (0: off)")
    config = parser.parse_args(argv)
    _check_image_size(config)
    check_augment_args(config)
    check_optimizer_args(config)
    if not 0.0 <= config.drop_path_rate < 1.0:
        raise SystemExit(f"--drop-path-rate {config.drop_path_rate:g}: expected a value in [0, 1) (0: off)")
    if config.accum_steps < 1 or config.batch_size % (config.accum_steps * max(1, config.n_gpu)):
        raise SystemExit(f"--batch-size {config.batch_size} is the batch of one optimizer step and must divide evenly "
                         f"into --accum-steps {config.accum_steps} micro-batches on each of {config.n_gpu} GPUs")
    config = globals()["get_{}_config".format(config.model_arch)](config)
    process_config(config)
    print_config(config)
    return config


def add_augment_args(parser, mixing):
    """the from-scratch augmentation flags, all off by default; mixing: also label smoothing and Mixup / CutMix"""
    parser.add_argument("--random-resized-crop", default=False, action="store_true",
                        help="ImageNet / TinyImageNet training: RandomResizedCrop in place of Resize")
    parser.add_argument("--crop-scale", type=float, nargs=2, default=[0.08, 1.0], metavar=("LO", "HI"),
                        help="--random-resized-crop: the crop's share of the image's area")
    parser.add_argument("--crop-ratio", type=float, nargs=2, default=[3.0 / 4.0, 4.0 / 3.0], metavar=("LO", "HI"),
                        help="--random-resized-crop: the crop's aspect ratio w / h")
    if not mixing:
        return
    parser.add_argument("--label-smoothing", type=float, default=0.0, help="label smoothing of the training loss")
    parser.add_argument("--mixup-alpha", type=float, default=0.0, help="Mixup: lambda ~ Beta(a, a) per batch (0: off)")
    parser.add_argument("--cutmix-alpha", type=float, default=0.0,
                        help="CutMix: lambda ~ Beta(a, a) per batch (0: off)")
    parser.add_argument("--mix-prob", type=float, default=1.0, help="probability that a batch is mixed")
    parser.add_argument("--mix-switch-prob", type=float, default=0.5,
                        help="probability of CutMix over Mixup when both alphas are set")


def check_augment_args(config):
    """out-of-range augmentation flags, and the crop on a dataset whose transform has none, exit with one line"""
    import math
    lo, hi = config.crop_scale
    if not (0.0 < lo <= hi <= 1.0):
        raise SystemExit(f"--crop-scale {lo:g} {hi:g}: expected 0 < LO <= HI <= 1")
    lo, hi = config.crop_ratio
    if not (0.0 < lo <= hi and math.isfinite(hi)):
        raise SystemExit(f"--crop-ratio {lo:g} {hi:g}: expected 0 < LO <= HI")
    if config.random_resized_crop:
        from .data import CROP_NEEDS_FOLDERS, FOLDER_DATASETS
        if config.synthetic:
            raise SystemExit("--random-resized-crop crops decoded image files: it does not go with --synthetic")
        if config.dataset not in FOLDER_DATASETS:
            raise SystemExit(CROP_NEEDS_FOLDERS.format(config.dataset))
    if not hasattr(config, "label_smoothing"):
        return
    if not 0.0 <= config.label_smoothing < 1.0:
        raise SystemExit(f"--label-smoothing {config.label_smoothing:g}: expected a value in [0, 1)")
    for flag, v in (("--mixup-alpha", config.mixup_alpha), ("--cutmix-alpha", config.cutmix_alpha)):
        if not (0.0 <= v and math.isfinite(v)):
            raise SystemExit(f"{flag} {v:g}: expected a value >= 0")
    for flag, v in (("--mix-prob", config.mix_prob), ("--mix-switch-prob", config.mix_switch_prob)):
        if not 0.0 <= v <= 1.0:
            raise SystemExit(f"{flag} {v:g}: expected a value in [0, 1]")


def check_optimizer_args(config):
    """resolves --lr-schedule auto; a schedule that does not go with the optimizer and an out-of-range --ema-decay exit
    with one line"""
    if config.lr_schedule == "auto":
        config.lr_schedule = "cosine" if config.optimizer == "adamw" else "onecycle"
    if config.optimizer == "adamw" and config.lr_schedule == "onecycle":
        raise SystemExit("--lr-schedule onecycle does not go with --optimizer adamw (OneCycleLR would cycle beta1); "
                         "use cosine")
    if not 0.0 <= config.ema_decay < 1.0:
        raise SystemExit(f"--ema-decay {config.ema_decay:g}: expected a value in [0, 1) (0: off)")
    for flag, v in (("--beta1", config.beta1), ("--beta2", config.beta2)):
        if not 0.0 <= v < 1.0:
            raise SystemExit(f"{flag} {v:g}: expected a value in [0, 1)")


def _check_image_size(config):
    if not config.any_image_size and config.image_size not in (224, 384):
        raise SystemExit(f"--image-size {config.image_size}: choose 224 or 384 (reference src/config.py:37), "
                         "or pass --any-image-size")


def get_b16_config(config):
    """ViT-B/16 configuration (reference src/config.py:57-66)"""
    config.patch_size = 16
    config.emb_dim = 768
    config.mlp_dim = 3072
    config.num_heads = 12
    config.num_layers = 12
    config.attn_dropout_rate = 0.0
    config.dropout_rate = 0.0
    return config


def get_b32_config(config):
    """ViT-B/32 configuration (reference src/config.py:69-73)"""
    config = get_b16_config(config)
    config.patch_size = 32
    return config


def get_l16_config(config):
    """ViT-L/16 configuration (reference src/config.py:76-85)"""
    config.patch_size = 16
    config.emb_dim = 1024
    config.mlp_dim = 4096
    config.num_heads = 16
    config.num_layers = 24
    config.attn_dropout_rate = 0.0
    config.dropout_rate = 0.0
    return config


def get_l32_config(config):
    """ViT-L/32 configuration (reference src/config.py:88-92)"""
    config = get_l16_config(config)
    config.patch_size = 32
    return config


def get_h14_config(config):
    """ViT-H/14 configuration (reference src/config.py:95-104)"""
    config.patch_size = 14
    config.emb_dim = 1280
    config.mlp_dim = 5120
    config.num_heads = 16
    config.num_layers = 32
    config.attn_dropout_rate = 0.0
    config.dropout_rate = 0.0
    return config


def process_config(config):
    """Experiment directories + config.json (reference src/utils.py:56-76)."""
    # (ranks started by `--n-gpu k` inherit their launcher's stamp, so all share one experiment dir)
    timestamp = os.environ.get("VITMI_EXP_STAMP") or datetime.now().strftime("%y%m%d_%H%M%S")
    config.exp_stamp = timestamp
    exp_name = config.exp_name + "_{}_bs{}_lr{}_wd{}".format(config.dataset, config.batch_size, config.lr, config.wd)
    exp_name += "_" + timestamp
    config.summary_dir = os.path.join("experiments", "tb", exp_name)
    config.checkpoint_dir = os.path.join("experiments", "save", exp_name, "checkpoints/")
    config.result_dir = os.path.join("experiments", "save", exp_name, "results/")
    if getattr(config, "no_save", False):
        return config
    for d in (config.summary_dir, config.checkpoint_dir, config.result_dir):
        os.makedirs(d, exist_ok=True)
    with open(os.path.join("experiments", "save", exp_name, "config.json"), "w") as f:
        json.dump(vars(config), f, indent=4)
    return config


def print_config(config):
    message = "----------------- Config ---------------\n"
    for k, v in sorted(vars(config).items()):
        message += "{:>35}: {:<30}\n".format(str(k), str(v))
    message += "----------------- End -------------------"
    print(message)
