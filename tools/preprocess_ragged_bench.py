"""vit_preprocess_u8_ragged beside vit_preprocess_u8, and the host decode rate beside the step rate.

    python tools/preprocess_ragged_bench.py [--out profiles/r08/preprocess_ragged_v1.txt] [--bench-line FILE]

One GPU run writes the file. Kernel times are HIP events around `--launches` back-to-back launches, after a
warm-up of each shape, repeated `--repeats` times: the median and the spread of the repeats are reported, and
the two entries of (a) alternate within each repeat, so that both see the same machine. A launch is ~100 us, so
a timed window holds enough launches to last tens of milliseconds.
  (a) 256 uniform 375 x 500 -> 224 x 224 through the ragged entry against vit_preprocess_u8 on the same batch
      (the yardstick: both read the same 144 MB and write the same 154 MB), outputs compared bit for bit;
  (b) a mixed-size batch of 256 drawn from a fixed seed (sides 120..640, a few far larger: the per-pixel path);
  (c) datasets.decode_rgb images per second at 1, 8 and 16 threads on 375 x 500 JPEGs this tool writes into a
      temporary directory (host only), beside the training step's rate read from a bench.py result line
      (--bench-line: a file whose last JSON line is one; without it the step rate is "not measured").
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "vit-of-pytorch_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

from vitmi import datasets, ops  # noqa: E402

OUT_HW = (224, 224)


def timed(fn, launches):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(launches):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / launches  # us per launch


def alternate(fns, launches, repeats, warmup):
    """{name: [us per launch, one per repeat]}, the entries taking turns within each repeat"""
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


def pack(images):
    geom, pos = np.zeros((len(images), 3), np.int64), 0
    for i, a in enumerate(images):
        geom[i] = (pos, a.shape[0], a.shape[1])
        pos += a.size
    return np.concatenate([a.reshape(-1) for a in images]), geom


def write_jpegs(directory, n, seed):
    from PIL import Image
    rng = np.random.default_rng(seed)
    paths = []
    for i in range(n):
        # low-frequency content plus noise, so that the files have a photograph's size (~100 KB), not a flat one's
        low = rng.integers(0, 256, (12, 16, 3), dtype=np.uint8)
        im = Image.fromarray(low).resize((500, 375), Image.BICUBIC)
        a = np.clip(np.asarray(im).astype(np.int16) + rng.integers(-20, 21, (375, 500, 3)), 0, 255).astype(np.uint8)
        path = os.path.join(directory, f"img_{i:04d}.JPEG")
        Image.fromarray(a).save(path, format="JPEG", quality=90)
        paths.append(path)
    return paths


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r08", "preprocess_ragged_v1.txt"))
    ap.add_argument("--bench-line", default=None, help="file whose last JSON line is a bench.py result")
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--jpegs", type=int, default=256)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("this measurement needs the GPU: nothing is timed without one")
    dev = "cuda"
    B, (oh, ow) = 256, OUT_HW
    lines = [f"device: {torch.cuda.get_device_name(0)}; HIP events around {args.launches} launches, "
             f"{args.warmup} warm-up launches per shape, {args.repeats} repeats, entries alternating"]
    rng = np.random.default_rng(0)

    # (a) uniform 375 x 500 through both entries
    H, W = 375, 500
    imgs = torch.from_numpy(rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)).to(dev)
    flips = torch.from_numpy(rng.integers(0, 2, B).astype(np.uint8)).to(dev)
    geom = torch.tensor([[i * H * W * 3, H, W] for i in range(B)], dtype=torch.int64, device=dev)
    flat = imgs.reshape(-1)
    out_u, out_r = (torch.empty(B, 3, oh, ow, device=dev) for _ in range(2))
    t = alternate({"uniform": lambda: ops.preprocess_u8(imgs, out_u, flips),
                   "ragged": lambda: ops.preprocess_u8_ragged(flat, geom, out_r, flips=flips)},
                  args.launches, args.repeats, args.warmup)
    same = bool(torch.equal(out_u, out_r))
    moved = (B * H * W * 3 + B * 3 * oh * ow * 4) / 1e9
    mu, mr = statistics.median(t["uniform"]), statistics.median(t["ragged"])
    lines += [f"(a) {B} x {H}x{W} -> {oh}x{ow}, {moved * 1e3:.0f} MB read + written per launch; outputs bit-identical: {same}",
              f"    vit_preprocess_u8         {describe(t['uniform'])}  {moved / mu * 1e6:7.0f} GB/s  {B / mu * 1e6:9.0f} img/s",
              f"    vit_preprocess_u8_ragged  {describe(t['ragged'])}  {moved / mr * 1e6:7.0f} GB/s  {B / mr * 1e6:9.0f} img/s",
              f"    ragged / uniform = {mr / mu:.3f}"]
    del imgs, flat

    # (b) mixed sizes from a fixed seed
    rng = np.random.default_rng(1)
    sizes = [(int(h), int(w)) for h, w in rng.integers(120, 641, (B, 2))]
    for i in range(0, B, 32):  # one in 32 far above 4x: the per-pixel path
        sizes[i] = (int(rng.integers(1000, 2500)), int(rng.integers(1000, 3000)))
    raw, g = pack([rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in sizes])
    raw_d, g_d = torch.from_numpy(raw).to(dev), torch.from_numpy(g).to(dev)
    small = [i for i, (h, w) in enumerate(sizes) if h <= 4 * oh and w <= 4 * ow]
    idx_small = torch.tensor((small * (B // len(small) + 1))[:B], dtype=torch.int64, device=dev)
    t = alternate({"all": lambda: ops.preprocess_u8_ragged(raw_d, g_d, out_r, flips=flips),
                   "tiled": lambda: ops.preprocess_u8_ragged(raw_d, g_d, out_r, index=idx_small, flips=flips)},
                  max(10, args.launches // 4), args.repeats, args.warmup)
    m_all, m_t = statistics.median(t["all"]), statistics.median(t["tiled"])
    lines += [f"(b) {B} mixed sizes (seed 1: sides 120..640, {B - len(small)} images of 1000..3000 on the per-pixel "
              f"path), {raw.size / 1e6:.0f} MB packed -> {oh}x{ow}",
              f"    whole batch               {describe(t['all'])}  {B / m_all * 1e6:9.0f} img/s",
              f"    its <= 4x images only     {describe(t['tiled'])}  {B / m_t * 1e6:9.0f} img/s  (index = those, repeated to {B})"]

    # (c) host decode rate
    with tempfile.TemporaryDirectory() as d:
        paths = write_jpegs(d, args.jpegs, seed=2)
        kb = sum(os.path.getsize(p) for p in paths) / len(paths) / 1e3
        lines.append(f"(c) datasets.decode_rgb on {len(paths)} JPEGs of 375x500 (quality 90, {kb:.0f} KB each), "
                     f"each decoded twice per timing, host has {os.cpu_count()} CPUs visible")
        rates = {}
        for threads in (1, 8, 16):
            with ThreadPoolExecutor(threads) as pool:
                list(pool.map(datasets.decode_rgb, paths[:32]))  # warm the file cache and the pool
                t0 = time.perf_counter()
                n = sum(1 for _ in pool.map(datasets.decode_rgb, paths * 2))
                rates[threads] = n / (time.perf_counter() - t0)
            lines.append(f"    {threads:2d} threads: {rates[threads]:8.0f} img/s")
    step = None
    if args.bench_line and os.path.isfile(args.bench_line):
        for text in open(args.bench_line):
            if text.lstrip().startswith("{"):
                step = json.loads(text)
    if step:
        lines.append(f"    training step ({step['config']['workload']}, batch {step['config']['per_gpu_batch']}): "
                     f"{step['value']:.0f} img/s -> a 16-thread decode feeds {rates[16] / step['value']:.2f} of it; "
                     f"the device transform alone runs at {B / m_all * 1e6 / step['value']:.0f}x the step")
    else:
        lines.append("    training step rate: not measured in this run")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
