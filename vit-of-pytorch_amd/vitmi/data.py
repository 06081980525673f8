"""Device-side input pipeline: the reference's loader transforms run as one HIP kernel.

Reference `src/data_loaders.py:66-80` (CIFAR-10/100 train: `transforms.Compose([Resize(size),
RandomHorizontalFlip(), ToTensor(), Normalize([0.5]*3, [0.5]*3)])`, eval without the flip) and
`:100-112` (ImageNet: `Resize((size, size))`). torchvision is not part of this stack: uint8 HWC
batches (as decoded / as CIFAR stores them) go to the GPU once and `vit_preprocess_u8` produces
the f32 NCHW model input, with the resize bit-exact to Pillow's BILINEAR (the arithmetic under
torchvision's PIL path; oracle/preprocess.py, tests/test_preprocess_cpu.py and
tests/test_preprocess_gpu.py). Flip draws come from a torch.Generator: the per-worker RNG streams
of the reference's DataLoader are not reproducible, the decision rule (rand < p) is the same.

Real datasets (vitmi.datasets: CIFAR-10/100 parsed from disk) go through ResidentLoader: the set stays
in HBM as stored (planar uint8), the sample order is the reference's seeded DataLoader order
(epoch_order), and each step's batch is one vit_preprocess_u8_gather launch.
"""
from __future__ import annotations

import os

import torch

from . import ops


def resized_size(h: int, w: int, size):
    """torchvision `Resize(size)` output (h, w): an int maps the shorter side to `size` keeping the
    aspect ratio (longer side truncated); a pair is (h, w)."""
    if isinstance(size, (tuple, list)):
        return int(size[0]), int(size[1])
    if w <= h:
        return int(size * h / w), int(size)
    return int(size), int(size * w / h)


def epoch_order(n: int, generator: torch.Generator) -> torch.Tensor:
    """Sample indices (int64 [n]) of the next epoch of the reference's seeded loader,
    `DataLoader(dataset, shuffle=True, generator=generator)` (src/data_loaders.py:53-61, 85-93), advancing
    `generator` exactly as one full pass over that loader does: the iterator draws its base seed (one int64
    `random_()`), the RandomSampler draws `randperm(n)`, which is the order, and, once exhausted, one more
    `randperm(n)` for its (empty) remainder. Pure host code; pinned against torch.utils.data.DataLoader itself
    by tests/test_datasets_cpu.py."""
    torch.empty((), dtype=torch.int64).random_(generator=generator)
    order = torch.randperm(n, generator=generator)
    torch.randperm(n, generator=generator)
    return order


def check_labels(labels, num_classes: int):
    """labels as int64 [n] on the host; a label outside [0, num_classes) is an error here, before anything
    reaches the device (there it would only surface as a NaN loss, vit_cross_entropy's rule)"""
    labels = torch.as_tensor(labels).to(torch.int64).reshape(-1).cpu()
    if labels.numel() and (int(labels.min()) < 0 or int(labels.max()) >= num_classes):
        bad = labels[(labels < 0) | (labels >= num_classes)]
        raise ValueError(f"{bad.numel()} labels lie outside [0, {num_classes}) (first: {int(bad[0])}, labels span "
                         f"[{int(labels.min())}, {int(labels.max())}]): --num-classes {num_classes} does not fit "
                         "this dataset")
    return labels


class EpochPlan:
    """Which samples, flipped or not, make up each batch of each epoch, for one rank: host only.

    Every rank computes the same global order and flips from `seed` and takes the contiguous slice
    [rank*b, (rank+1)*b) of each global batch of world*b samples - DataParallel's scatter
    (src/train.py:128-129) - so the global batch of step k is the same set of samples at any world size.
      order  train: epoch_order() of a generator seeded with `seed`, epoch after epoch (the reference's
             sample order); eval: file order.
      flips  train: `rand < 0.5`, one draw per sample of the epoch in global-batch order, from a second
             generator seeded from `seed` (the reference draws them in its worker processes: its decision
             rule, not its stream, is reproduced); eval: none.
      ragged the last global batch of r < world*b samples is kept when world == 1 (drop_last=False); with
             more ranks it is split evenly when world divides r and skipped otherwise (ranks with unequal
             batches would weigh unequally in the averaged gradient).
    """

    FLIP_SEED_OFFSET = 0x5EED_F11B

    def __init__(self, n, batch_size, train=True, seed=42, world=1, rank=0):
        if n <= 0 or batch_size <= 0 or world <= 0 or not 0 <= rank < world:
            raise ValueError(f"EpochPlan: n={n}, batch_size={batch_size}, world={world}, rank={rank}")
        self.n, self.batch_size, self.train, self.world, self.rank = n, batch_size, train, world, rank
        self.order_generator = torch.Generator().manual_seed(seed)
        self.flip_generator = torch.Generator().manual_seed(seed + self.FLIP_SEED_OFFSET)
        g = batch_size * world
        self._slices = [(s + rank * batch_size, s + (rank + 1) * batch_size) for s in range(0, n - g + 1, g)]
        r = n % g
        self.skipped = 0
        if r and r % world == 0:
            self._slices.append((n - r + rank * (r // world), n - r + (rank + 1) * (r // world)))
        elif r:
            self.skipped = r

    def __len__(self):
        return len(self._slices)

    def slices(self):
        """[(start, stop)] into the epoch's order / flips, one per batch this rank yields"""
        return list(self._slices)

    def next_epoch(self):
        """(order int64 [n], flips uint8 [n] or None) of the next epoch"""
        if not self.train:
            return torch.arange(self.n, dtype=torch.int64), None
        order = epoch_order(self.n, self.order_generator)
        flips = (torch.rand(self.n, generator=self.flip_generator) < 0.5).to(torch.uint8)
        return order, flips


class ResidentLoader:
    """A whole uint8 dataset resident in HBM, batches produced by one launch each.

    The reference feeds its step from `DataLoader(CIFAR10/100(transform=Resize -> RandomHorizontalFlip ->
    ToTensor -> Normalize), shuffle=train, generator=manual_seed(seed))` (src/data_loaders.py:32-93). Here the
    set (planar uint8 [n, 3, H, W], as the CIFAR files store it; CIFAR-100 train is 150 MB) and its labels are
    uploaded once; each epoch uploads that epoch's order and flips (EpochPlan) once; each step is one
    vit_preprocess_u8_gather launch on views of those two arrays, which gathers, transforms and picks the
    labels: no index_select, no per-step host-to-device copy, no host synchronisation.
    `batch_size` is this rank's batch. Yields (float32 [b, 3, h, w], int64 [b]) on the device."""

    def __init__(self, images_u8_chw, labels, batch_size, image_size, device, train=True, seed=42, world=1, rank=0,
                 num_classes=None, mean=(0.5, 0.5, 0.5), std=(0.5, 0.5, 0.5)):
        images = torch.as_tensor(images_u8_chw)
        if images.dtype != torch.uint8 or images.dim() != 4 or images.shape[1] != 3:
            raise ValueError(f"ResidentLoader: images uint8 [n, 3, H, W], got {images.dtype} {tuple(images.shape)}")
        labels = torch.as_tensor(labels).reshape(-1)
        if labels.numel() != images.shape[0]:
            raise ValueError(f"ResidentLoader: {images.shape[0]} images but {labels.numel()} labels")
        if num_classes is not None:
            labels = check_labels(labels, num_classes)
        self.plan = EpochPlan(images.shape[0], batch_size, train, seed, world, rank)
        if self.plan.skipped and rank == 0:
            print(f"{'train' if train else 'eval'} loader: the last {self.plan.skipped} images of each epoch's order "
                  f"do not divide over {world} ranks and are left out (every epoch)", flush=True)
        self.out_hw = resized_size(images.shape[2], images.shape[3], image_size)
        self.mean, self.std = tuple(mean), tuple(std)
        self.device = torch.device(device)
        self.images = images.contiguous().to(self.device)
        self.labels = labels.to(torch.int64).contiguous().to(self.device)
        self.order = self.flips = None  # this epoch's, on the device
        self.last_flips = None  # the epoch's flips on the host (uint8 [n]; None for eval), for inspection

    def __len__(self):
        return len(self.plan)

    def __iter__(self):
        if self.order is None or self.plan.train:
            order, flips = self.plan.next_epoch()
            self.last_flips = flips
            self.order = order.to(self.device)
            self.flips = None if flips is None else flips.to(self.device)
        h, w = self.out_hw
        for s, e in self.plan.slices():
            out = torch.empty(e - s, 3, h, w, device=self.device, dtype=torch.float32)
            target = torch.empty(e - s, device=self.device, dtype=torch.int64)
            ops.preprocess_u8_gather(self.images, self.order[s:e], out, None if self.flips is None else self.flips[s:e],
                                     self.mean, self.std, layout=ops.IMAGES_CHW, labels_in=self.labels,
                                     labels_out=target)
            yield out, target


def cifar_loaders(config, batch_size, device, world=1, rank=0, splits=("train", "test")):
    """The reference's `{dataset}DataLoader(data_dir=os.path.join(config.data_dir, config.dataset), split=...)`
    pair (src/train.py:134-147) as ResidentLoaders: the train split shuffled and flipped, the test split
    (the reference's split='val') in file order. `batch_size` is the per-rank batch."""
    from . import datasets
    if config.dataset not in datasets.SUPPORTED:
        raise SystemExit(f"--dataset {config.dataset} is not supported without --synthetic: this path reads "
                         f"{' and '.join(datasets.SUPPORTED)} from --data-dir (ImageNet / TinyImageNet need JPEG "
                         "decoding, which is outside it)")
    root = os.path.join(config.data_dir, config.dataset)
    loaders = []
    for split in splits:
        try:
            images, labels, _ = datasets.load_cifar(root, config.dataset, train=split == "train")
            loaders.append(ResidentLoader(images, labels, batch_size, config.image_size, device,
                                          train=split == "train", seed=config.seed, world=world, rank=rank,
                                          num_classes=config.num_classes))
        except (datasets.DatasetError, ValueError) as e:
            raise SystemExit(f"{config.dataset} {split} split: {e}") from e
    return loaders


class GPUTransform:
    """Compose([Resize(size), RandomHorizontalFlip(p)?, ToTensor(), Normalize(mean, std)]) over a
    uint8 [B, H, W, 3] batch on the device -> float32 [B, 3, h, w]."""

    def __init__(self, size, train: bool = True, flip_p: float = 0.5, mean=(0.5, 0.5, 0.5), std=(0.5, 0.5, 0.5),
                 generator: torch.Generator | None = None):
        self.size = size
        self.train = train
        self.flip_p = flip_p
        self.mean = tuple(mean)
        self.std = tuple(std)
        self.generator = generator

    def __call__(self, images: torch.Tensor, flips: torch.Tensor | None = None, out: torch.Tensor | None = None):
        if images.dtype != torch.uint8 or images.dim() != 4 or images.shape[3] != 3:
            raise ValueError(f"expected uint8 images [B, H, W, 3], got {images.dtype} {tuple(images.shape)}")
        if not images.is_cuda:
            raise ValueError("GPUTransform runs on the device: move the uint8 batch to the GPU first")
        images = images.contiguous()
        B, H, W, _ = images.shape
        h, w = resized_size(H, W, self.size)
        if flips is None and self.train and self.flip_p > 0:
            flips = torch.rand(B, generator=self.generator) < self.flip_p
        if flips is not None:
            flips = flips.to(device=images.device, dtype=torch.uint8)
        if out is None:
            out = torch.empty(B, 3, h, w, device=images.device, dtype=torch.float32)
        ops.preprocess_u8(images, out, flips, self.mean, self.std)
        return out
