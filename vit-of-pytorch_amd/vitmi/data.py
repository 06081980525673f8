"""Device-side input pipeline: the reference's loader transforms run as one HIP kernel.

Reference `src/data_loaders.py:66-80` (CIFAR-10/100 train: `transforms.Compose([Resize(size),
RandomHorizontalFlip(), ToTensor(), Normalize([0.5]*3, [0.5]*3)])`, eval without the flip) and
`:100-112` (ImageNet: `Resize((size, size))`). torchvision is not part of this stack: uint8 HWC
batches (as decoded / as CIFAR stores them) go to the GPU once and `vit_preprocess_u8` produces
the f32 NCHW model input, with the resize bit-exact to Pillow's BILINEAR (the arithmetic under
torchvision's PIL path; oracle/preprocess.py, tests/test_preprocess_cpu.py and
tests/test_preprocess_gpu.py). Flip draws come from a torch.Generator: the per-worker RNG streams
of the reference's DataLoader are not reproducible, the decision rule (rand < p) is the same.

Real datasets (vitmi.datasets): CIFAR-10/100 parsed from disk go through ResidentLoader: the set stays
in HBM as stored (planar uint8), the sample order is the reference's seeded DataLoader order
(epoch_order), and each step's batch is one vit_preprocess_u8_gather launch. ImageNet / TinyImageNet image
folders go through FolderLoader: files decoded on the host by Pillow, of whatever sizes, packed end to end, and
each step's batch is one vit_preprocess_u8_ragged launch, streamed or resident; with crop=(scale, ratio) the training
split takes torchvision's RandomResizedCrop in the same launch (vit_preprocess_u8_ragged_crop, boxes from
vitmi.augment.CropPlan). `loaders` picks by --dataset.
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
        raise SystemExit(f"--dataset {config.dataset} is not supported without --synthetic: this project reads "
                         f"{ON_DISK_FORMS}")
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


class _Slot:
    """one batch in flight from the producer to the launch that reads it: a pinned host buffer and its device
    copy for the packed bytes and for the table (geometry rows, then labels)"""

    def __init__(self, batch_size, device):
        self.device = device
        self.host_meta = torch.empty(batch_size * 8, dtype=torch.int64).pin_memory()  # + the crop boxes
        self.dev_meta = torch.empty(batch_size * 8, dtype=torch.int64, device=device)
        self.host_bytes = self.dev_bytes = None
        self.copied = torch.cuda.Event()  # the upload of this slot's batch, on the side stream
        self.consumed = None  # recorded by the consumer behind the launch that read the slot

    def reserve(self, n_bytes):
        if self.host_bytes is None or self.host_bytes.numel() < n_bytes:
            cap = n_bytes + n_bytes // 4
            self.host_bytes = torch.empty(cap, dtype=torch.uint8).pin_memory()
            self.dev_bytes = torch.empty(cap, dtype=torch.uint8, device=self.device)


def _checked_image(a, path):
    """a decoded image as the device transform takes it: uint8 [H, W, 3], 0 < H, W < 2^15, contiguous"""
    import numpy as np
    from .datasets import DatasetError
    a = np.asarray(a)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
        raise DatasetError(f"{path}: decoded to {a.dtype} {a.shape}, expected uint8 [H, W, 3]")
    if not (0 < a.shape[0] < 1 << 15 and 0 < a.shape[1] < 1 << 15):
        raise DatasetError(f"{path}: {a.shape[0]} x {a.shape[1]} pixels; the device transform takes sides in "
                           "[1, 32767]")
    return np.ascontiguousarray(a)


class FolderLoader:
    """Image files of any sizes (ImageNet / TinyImageNet folders), decoded on the host and transformed on the
    device by one launch per batch.

    The reference feeds its step from `DataLoader(ImageFolder(transform=Resize((s, s)) -> RandomHorizontalFlip ->
    ToTensor -> Normalize), shuffle=train, generator=manual_seed(seed), num_workers=k)` (src/data_loaders.py:96-124,
    res-vit/data_loaders.py:96-216). Here EpochPlan gives the same sample order, the flip rule, the ranks' slices
    and the ragged last batch, `decode` (datasets.decode_rgb: Pillow, as the reference) turns a path into uint8
    [H, W, 3], and vit_preprocess_u8_ragged resizes every image of a batch from its own size to `image_size`
    (always the pair (h, w)), flips, normalises and picks the labels in one launch, bit-exact to Pillow's resize.

    streaming (resident=False)  a producer thread decodes the coming batches on a pool of min(workers, 16) threads
        (Pillow releases the GIL while it decodes; no worker processes), packs each batch end to end into a pinned
        buffer with its (offset, H, W) table and labels and uploads both on a side stream. `depth` slots go round;
        events order the upload before the launch that reads a slot, and that launch before the slot's next
        overwrite. The consuming loop only waits for the producer's queue: it never synchronises the device.
    resident=True  one decode pass packs the whole split into HBM with its table and labels (refused above
        `resident_gb`); then a batch is one launch with index = order[s:e], with no host work per step.

    crop=(scale, ratio)  (training split only; ignored for eval) torchvision's RandomResizedCrop(size, scale, ratio) in
        place of Resize: every sample of the epoch gets a box from vitmi.augment.CropPlan, a function of (seed, epoch,
        position in the epoch's order) alone, and the launch is vit_preprocess_u8_ragged_crop. Whole images are still
        packed: one path. Resident: the epoch's boxes are computed from the kept sizes and uploaded once with the
        order and the flips. Streaming: the producer computes each batch's boxes after the decode and ships them in
        the slot's table. `last_crops` holds the epoch's boxes by position (resident) or the last yielded batch's
        (streaming): int64 [., 4] = (top, left, h, w) on the host, None without crop.

    `data_wait_s` is the time the last (or running) epoch's consumer spent waiting for the producer.
    `batch_size` is this rank's batch. Yields (float32 [b, 3, h, w], int64 [b]) on the device."""

    def __init__(self, paths, labels, batch_size, image_size, device, train=True, seed=42, world=1, rank=0,
                 num_classes=None, workers=8, resident=False, resident_gb=32.0, decode=None, depth=2,
                 mean=(0.5, 0.5, 0.5), std=(0.5, 0.5, 0.5), crop=None):
        from . import datasets
        self.paths = list(paths)
        self.crop_plan = None
        if crop is not None and train:
            from .augment import CropPlan
            self.crop_plan = CropPlan(seed, crop[0], crop[1])
        self.epoch = 0  # epochs started: the crop draws' second key
        self.last_crops = self.crops = None
        labels = torch.as_tensor(labels).reshape(-1)
        if labels.numel() != len(self.paths):
            raise ValueError(f"FolderLoader: {len(self.paths)} paths but {labels.numel()} labels")
        labels = check_labels(labels, num_classes) if num_classes is not None else labels.to(torch.int64).cpu()
        self.host_labels = labels.contiguous()
        self.plan = EpochPlan(len(self.paths), batch_size, train, seed, world, rank)
        if self.plan.skipped and rank == 0:
            print(f"{'train' if train else 'eval'} loader: the last {self.plan.skipped} images of each epoch's order "
                  f"do not divide over {world} ranks and are left out (every epoch)", flush=True)
        self.out_hw = (int(image_size), int(image_size)) if isinstance(image_size, int) else \
            (int(image_size[0]), int(image_size[1]))
        self.mean, self.std = tuple(mean), tuple(std)
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:  # the producer thread names it by index
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.decode = datasets.decode_rgb if decode is None else decode
        self.workers = max(1, min(int(workers), 16))  # never the machine's CPU count
        self.depth = max(2, int(depth))
        self.resident = bool(resident)
        self.data_wait_s = 0.0
        self.last_flips = None
        self.order = self.flips = None
        if self.resident:
            self._load_resident(resident_gb)

    def __len__(self):
        return len(self.plan)

    # -- resident ------------------------------------------------------------------------------------------
    def _load_resident(self, resident_gb):
        import numpy as np
        from concurrent.futures import ThreadPoolExecutor
        from .datasets import DatasetError
        limit = int(float(resident_gb) * (1 << 30))
        n = len(self.paths)
        geom = np.zeros((n, 3), np.int64)
        chunks, total = [], 0
        with ThreadPoolExecutor(self.workers, thread_name_prefix="vitmi-decode") as pool:
            for s in range(0, n, 256):
                part = [_checked_image(a, p) for a, p in
                        zip(pool.map(self.decode, self.paths[s:s + 256]), self.paths[s:s + 256])]
                for i, a in enumerate(part):
                    geom[s + i] = (total, a.shape[0], a.shape[1])
                    total += a.size
                if total > limit:
                    raise DatasetError(f"the decoded split passes --resident-gb {resident_gb:g} after {s + len(part)} "
                                       f"of {n} images ({total / (1 << 30):.1f} GB): drop --resident-data to stream "
                                       "it, or raise --resident-gb")
                chunks.append(np.concatenate([a.reshape(-1) for a in part]))
        self.bytes = torch.empty(total, dtype=torch.uint8, device=self.device)
        pos = 0
        for c in chunks:
            self.bytes[pos:pos + c.size].copy_(torch.from_numpy(c))
            pos += c.size
        self.geom = torch.from_numpy(geom).to(self.device)
        self.host_geom = geom
        self.labels = self.host_labels.to(self.device)

    def _iter_resident(self):
        h, w = self.out_hw
        for s, e in self.plan.slices():
            out = torch.empty(e - s, 3, h, w, device=self.device, dtype=torch.float32)
            target = torch.empty(e - s, device=self.device, dtype=torch.int64)
            flips = None if self.flips is None else self.flips[s:e]
            if self.crops is None:
                ops.preprocess_u8_ragged(self.bytes, self.geom, out, index=self.order[s:e], flips=flips,
                                         mean=self.mean, std=self.std, labels_in=self.labels, labels_out=target)
            else:
                ops.preprocess_u8_ragged_crop(self.bytes, self.geom, out, self.crops[s:e], index=self.order[s:e],
                                              flips=flips, mean=self.mean, std=self.std, labels_in=self.labels,
                                              labels_out=target)
            yield out, target

    # -- streaming -----------------------------------------------------------------------------------------
    def _produce(self, order, slices, pool, free, ready, stop, stream, epoch):
        """the producer thread: decode ahead, pack, upload; hands (slot, count, bytes) or an exception to `ready`"""
        from collections import deque
        try:
            torch.cuda.set_device(self.device)
            pending, nxt = deque(), 0
            for start, _ in slices:
                while nxt < len(slices) and len(pending) <= self.depth:  # decode up to depth batches ahead
                    s, e = slices[nxt]
                    idx = order[s:e].tolist()
                    pending.append((idx, [pool.submit(self.decode, self.paths[i]) for i in idx]))
                    nxt += 1
                idx, futures = pending.popleft()
                images = [_checked_image(f.result(), self.paths[i]) for f, i in zip(futures, idx)]
                slot = free.get()
                if slot is None or stop.is_set():
                    return
                if slot.consumed is not None:
                    slot.consumed.synchronize()  # the launch that read this slot last has run
                b, n_bytes = len(images), sum(a.size for a in images)
                slot.reserve(n_bytes)
                host, meta, pos = slot.host_bytes.numpy(), slot.host_meta.numpy(), 0
                for k, a in enumerate(images):
                    host[pos:pos + a.size] = a.reshape(-1)
                    meta[3 * k:3 * k + 3] = (pos, a.shape[0], a.shape[1])
                    pos += a.size
                meta[3 * b:4 * b] = self.host_labels[idx].numpy()
                if self.crop_plan is not None:
                    meta[4 * b:8 * b] = self.crop_plan.boxes(epoch, start, [a.shape[0] for a in images],
                                                             [a.shape[1] for a in images]).reshape(-1)
                with torch.cuda.stream(stream):
                    slot.dev_bytes[:n_bytes].copy_(slot.host_bytes[:n_bytes], non_blocking=True)
                    slot.dev_meta[:8 * b].copy_(slot.host_meta[:8 * b], non_blocking=True)
                    slot.copied.record(stream)
                ready.put((slot, b, n_bytes))
        except BaseException as e:  # surfaces in the consuming loop
            ready.put(e)

    def _iter_streaming(self, order):
        import queue
        import threading
        import time
        from concurrent.futures import ThreadPoolExecutor
        h, w = self.out_hw
        slices = self.plan.slices()
        bmax = max(e - s for s, e in slices)
        free, ready, stop = queue.Queue(), queue.Queue(), threading.Event()
        for _ in range(self.depth):
            free.put(_Slot(bmax, self.device))
        pool = ThreadPoolExecutor(self.workers, thread_name_prefix="vitmi-decode")
        stream = torch.cuda.Stream(self.device)
        producer = threading.Thread(target=self._produce,
                                    args=(order, slices, pool, free, ready, stop, stream, self.epoch),
                                    name="vitmi-producer", daemon=True)
        producer.start()
        try:
            for s, e in slices:
                t0 = time.perf_counter()
                item = ready.get()
                self.data_wait_s += time.perf_counter() - t0
                if isinstance(item, BaseException):
                    raise item
                slot, b, n_bytes = item
                out = torch.empty(b, 3, h, w, device=self.device, dtype=torch.float32)
                target = torch.empty(b, device=self.device, dtype=torch.int64)
                cur = torch.cuda.current_stream(self.device)
                cur.wait_event(slot.copied)
                flips = None if self.flips is None else self.flips[s:e]
                if self.crop_plan is None:
                    ops.preprocess_u8_ragged(slot.dev_bytes, slot.dev_meta[:3 * b].view(b, 3), out, flips=flips,
                                             mean=self.mean, std=self.std, labels_in=slot.dev_meta[3 * b:4 * b],
                                             labels_out=target, n_bytes=n_bytes)
                else:
                    ops.preprocess_u8_ragged_crop(slot.dev_bytes, slot.dev_meta[:3 * b].view(b, 3), out,
                                                  slot.dev_meta[4 * b:8 * b].view(b, 4), flips=flips, mean=self.mean,
                                                  std=self.std, labels_in=slot.dev_meta[3 * b:4 * b],
                                                  labels_out=target, n_bytes=n_bytes)
                    self.last_crops = slot.host_meta[4 * b:8 * b].view(b, 4).clone()
                slot.dev_bytes.record_stream(cur)
                slot.dev_meta.record_stream(cur)
                slot.consumed = torch.cuda.Event()
                slot.consumed.record(cur)
                free.put(slot)
                yield out, target
        finally:
            stop.set()
            free.put(None)
            pool.shutdown(wait=True, cancel_futures=True)
            producer.join()

    def __iter__(self):
        if self.order is None or self.plan.train:
            order, flips = self.plan.next_epoch()
            self.last_flips = flips
            self.host_order = order
            self.order = order.to(self.device)
            self.flips = None if flips is None else flips.to(self.device)
            self.epoch += 1
            if self.crop_plan is not None and self.resident:
                sizes = self.host_geom[order.numpy()]
                self.last_crops = torch.from_numpy(self.crop_plan.boxes(self.epoch, 0, sizes[:, 1], sizes[:, 2]))
                self.crops = self.last_crops.to(self.device)
        self.data_wait_s = 0.0
        return self._iter_resident() if self.resident else self._iter_streaming(self.host_order)


FOLDER_DATASETS = ("ImageNet", "TinyImageNet")
CROP_NEEDS_FOLDERS = ("--random-resized-crop runs inside the ragged image-folder transform (ImageNet, TinyImageNet); "
                      "--dataset {} goes through the fixed-size gather transform, which has no crop")
ON_DISK_FORMS = (
    "CIFAR10 and CIFAR100 in their published python or binary form (<data-dir>/CIFAR10/cifar-10-batches-py or "
    "cifar-10-batches-bin, <data-dir>/CIFAR100/cifar-100-python or cifar-100-binary); ImageNet as image folders "
    "(<data-dir>/ImageNet/train/<class>/<image files> and <data-dir>/ImageNet/val/<class>/<image files>); "
    "TinyImageNet as <data-dir>/TinyImageNet/train/<class>/images/<image files> with val/ in the same form or as "
    "the published val/images/ + val/val_annotations.txt")


def crop_of(config):
    """(scale, ratio) of --random-resized-crop, or None"""
    if not getattr(config, "random_resized_crop", False):
        return None
    return tuple(config.crop_scale), tuple(config.crop_ratio)


def folder_loaders(config, batch_size, device, world=1, rank=0, splits=("train", "test")):
    """The reference's ImageNetDataLoader / TinyImageNetDataLoader pair (src/train.py:134-147 with
    src/data_loaders.py:96-124, res-vit/data_loaders.py:96-216) as FolderLoaders over
    <data-dir>/<dataset>/{train,val}: 'train' shuffled and flipped, 'test' (the reference's split='val') in file
    order. ImageNet streams unless --resident-data; TinyImageNet is resident. --num-workers sizes the decode pool."""
    from . import datasets
    root = os.path.join(config.data_dir, config.dataset)
    resident = bool(getattr(config, "resident_data", False)) or config.dataset == "TinyImageNet"
    loaders_ = []
    for split in splits:
        sub = "train" if split == "train" else "val"
        try:
            if not os.path.isdir(os.path.join(root, sub)):
                raise datasets.DatasetError(f"looked for the directory {os.path.join(root, sub)} and did not find it "
                                            f"(nothing is downloaded or created here). This project reads: "
                                            f"{ON_DISK_FORMS}")
            if config.dataset == "ImageNet":
                paths, labels, _ = datasets.find_image_folder(os.path.join(root, sub))
            else:
                paths, labels, _ = datasets.find_tiny_imagenet(root, sub)
            from .config import image_hw
            loaders_.append(FolderLoader(paths, labels, batch_size, image_hw(config.image_size), device,
                                         train=split == "train", seed=config.seed, world=world, rank=rank,
                                         num_classes=config.num_classes, workers=getattr(config, "num_workers", 8),
                                         resident=resident, resident_gb=getattr(config, "resident_gb", 32.0),
                                         crop=crop_of(config)))
        except (datasets.DatasetError, ValueError) as e:
            raise SystemExit(f"{config.dataset} {sub} split: {e}") from e
    return loaders_


def loaders(config, batch_size, device, world=1, rank=0, splits=("train", "test")):
    """The loaders of `--dataset`, one per split ('train', 'test' = the evaluation split): CIFAR10 / CIFAR100 as
    ResidentLoaders (cifar_loaders), ImageNet / TinyImageNet as FolderLoaders (folder_loaders). Any other name
    exits with the list of what is read."""
    if config.dataset in FOLDER_DATASETS:
        return folder_loaders(config, batch_size, device, world, rank, splits)
    if getattr(config, "random_resized_crop", False):
        raise SystemExit(CROP_NEEDS_FOLDERS.format(config.dataset))
    return cifar_loaders(config, batch_size, device, world, rank, splits)


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
