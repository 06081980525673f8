"""What the from-scratch augmentations cost on the GPU: the batch mix against its byte floor, the cropped ragged
transform beside the uncropped one, the soft cross entropy beside the hard one.

    python tools/augment_bench.py [--out profiles/r10/augment_cost.txt] [--parent-lib PATH/libvit_hip.so]
                                  [--bench-lines FILE ...]

One GPU run writes the file. Kernel times are HIP events around `--launches` back-to-back launches, after a warm-up
of each shape, repeated `--repeats` times; the entries of one comparison alternate within each repeat, so that all see
the same machine, and the median and the spread of the repeats are reported.
  (a) vit_mix_batch on [256, 3, 224, 224] (Mixup: every element blended; CutMix: a quarter-area box) against the
      bytes it must move, two reads and one write, at the HBM peak of 8 TB/s;
  (b) vit_preprocess_u8_ragged_crop with full-image crops, and with RandomResizedCrop boxes, beside
      vit_preprocess_u8_ragged on the same packed batch of 256 x 375x500 -> 224x224; with --parent-lib also the
      library of the commit before the crop existed, called through ctypes on the same buffers;
  (c) vit_cross_entropy_soft beside vit_cross_entropy on [256, 1000].
--bench-lines: files whose last JSON line is a bench.py result; their ms_per_step are copied into the report under
the files' names (the step itself is timed by bench.py, not here).
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "vit-of-pytorch_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

from vitmi import ops  # noqa: E402
from vitmi.augment import CropPlan  # noqa: E402

HBM_PEAK = 8.0e12  # bytes / s


def timed(fn, launches):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(launches):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / launches  # us per launch


def alternate(fns, launches, repeats, warmup):
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            times[k].append(timed(fn, launches))
    return times


def describe(ts):
    return f"median {statistics.median(ts):8.1f} us  (min {min(ts):.1f}, max {max(ts):.1f}, {len(ts)} repeats)"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r10", "augment_cost.txt"))
    ap.add_argument("--parent-lib", default=None, help="libvit_hip.so of the commit before vit_preprocess_u8_ragged_crop")
    ap.add_argument("--bench-lines", nargs="*", default=[], help="files whose last JSON line is a bench.py result")
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("this measurement needs the GPU: nothing is timed without one")
    dev = "cuda"
    B, oh, ow = 256, 224, 224
    lines = [f"device: {torch.cuda.get_device_name(0)}; HIP events around {args.launches} launches, "
             f"{args.warmup} warm-up launches per shape, {args.repeats} repeats, entries alternating"]

    # (a) the mix
    x = torch.randn(B, 3, oh, ow, device=dev)
    out = torch.empty_like(x)
    pair = torch.arange(B - 1, -1, -1, device=dev)
    mixup = (torch.full((B,), 0.3, device=dev), torch.zeros(B, 4, dtype=torch.int64, device=dev))
    cutmix = (torch.ones(B, device=dev), torch.tensor([[56, 168, 56, 168]] * B, dtype=torch.int64, device=dev))
    t = alternate({"mixup": lambda: ops.mix_batch(x, out, pair, *mixup),
                   "cutmix": lambda: ops.mix_batch(x, out, pair, *cutmix)}, args.launches, args.repeats, args.warmup)
    moved = 3 * x.numel() * 4
    floor = moved / HBM_PEAK * 1e6
    lines.append(f"(a) vit_mix_batch [{B}, 3, {oh}, {ow}]: {moved / 1e6:.0f} MB (two reads, one write); floor at 8 TB/s "
                 f"{floor:.1f} us")
    for k in ("mixup", "cutmix"):
        m = statistics.median(t[k])
        lines.append(f"    {k:7s} {describe(t[k])}  {moved / m / 1e3:7.0f} GB/s  {floor / m:.2f} of the floor's rate")
    del x, out

    # (b) the cropped transform
    H, W = 375, 500
    rng = np.random.default_rng(0)
    flat = torch.from_numpy(rng.integers(0, 256, B * H * W * 3, dtype=np.uint8)).to(dev)
    flips = torch.from_numpy(rng.integers(0, 2, B).astype(np.uint8)).to(dev)
    geom = torch.tensor([[i * H * W * 3, H, W] for i in range(B)], dtype=torch.int64, device=dev)
    full = torch.tensor([[0, 0, H, W]] * B, dtype=torch.int64, device=dev)
    boxes = torch.from_numpy(CropPlan(0).boxes(1, 0, [H] * B, [W] * B)).to(dev)
    o_plain, o_full, o_box, o_parent = (torch.empty(B, 3, oh, ow, device=dev) for _ in range(4))
    fns = {"ragged": lambda: ops.preprocess_u8_ragged(flat, geom, o_plain, flips=flips),
           "crop_full": lambda: ops.preprocess_u8_ragged_crop(flat, geom, o_full, full, flips=flips),
           "crop_rrc": lambda: ops.preprocess_u8_ragged_crop(flat, geom, o_box, boxes, flips=flips)}
    if args.parent_lib:
        parent = ctypes.CDLL(os.path.abspath(args.parent_lib))
        vp, i64 = ctypes.c_void_p, ctypes.c_int64
        parent.vit_preprocess_u8_ragged.restype = ctypes.c_int32
        parent.vit_preprocess_u8_ragged.argtypes = [vp, i64, vp, i64, vp, i64, vp, i64, i64, vp, vp, vp, vp, vp]
        ms = (ctypes.c_float * 6)(0.5, 0.5, 0.5, 0.5, 0.5, 0.5)
        stream = torch.cuda.current_stream().cuda_stream

        def call_parent():
            rc = parent.vit_preprocess_u8_ragged(flat.data_ptr(), flat.numel(), geom.data_ptr(), B, None, B,
                                                 flips.data_ptr(), oh, ow, ms, o_parent.data_ptr(), None, None, stream)
            assert rc == 0
        fns["parent"] = call_parent
    t = alternate(fns, args.launches, args.repeats, args.warmup)
    moved = B * H * W * 3 + B * 3 * oh * ow * 4
    lines.append(f"(b) {B} x {H}x{W} -> {oh}x{ow}, {moved / 1e6:.0f} MB read + written per uncropped launch; full-image "
                 f"crops bit-identical to the uncropped entry: {bool(torch.equal(o_plain, o_full))}"
                 + (f"; to the parent's library: {bool(torch.equal(o_plain, o_parent))}" if args.parent_lib else ""))
    names = {"ragged": "vit_preprocess_u8_ragged", "crop_full": "..._ragged_crop, full-image boxes",
             "crop_rrc": "..._ragged_crop, RandomResizedCrop", "parent": "vit_preprocess_u8_ragged, parent commit"}
    base = statistics.median(t["parent" if args.parent_lib else "ragged"])
    for k in fns:
        lines.append(f"    {names[k]:40s} {describe(t[k])}  x{statistics.median(t[k]) / base:.3f}")
    del flat

    # (c) the loss
    C = 1000
    logits = torch.randn(B, C, device=dev) * 3
    y = torch.randint(0, C, (B,), device=dev)
    lam = torch.full((B,), 0.3, device=dev)
    y2 = y.flip(0).contiguous()
    d, st = torch.empty(B, C, device=dev), torch.empty(B, 3, device=dev)
    t = alternate({"hard": lambda: ops.cross_entropy(logits, y, d, 1.0 / B, st),
                   "soft": lambda: ops.cross_entropy_soft(logits, y, d, 1.0 / B, st, labels2=y2, lam=lam,
                                                          smoothing=0.1)}, args.launches, args.repeats, args.warmup)
    lines.append(f"(c) cross entropy [{B}, {C}]")
    lines.append(f"    vit_cross_entropy       {describe(t['hard'])}")
    lines.append(f"    vit_cross_entropy_soft  {describe(t['soft'])}")

    for path in args.bench_lines:
        last = None
        if os.path.isfile(path):
            for text in open(path):
                if text.lstrip().startswith("{"):
                    last = json.loads(text)
        lines.append(f"bench.py {os.path.basename(path)}: " +
                     (f"ms_per_step {last['ms_per_step']}, {last['value']} {last['unit']}" if last else "not measured"))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
