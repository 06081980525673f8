"""Times vit_adamw_ema_update (EMA and bf16 mirror on) at the ViT-B/16 and ViT-H/14 flat-buffer sizes against the pieces
it replaces on the same buffers (vit_adamw_update with the mirror, then vit_axpby for the EMA) and against its byte
floor. HIP events around `iters` launches, three alternating rounds. Wrote profiles/r11/adamw_ema_step.txt:

    python tools/adamw_ema_bench.py > profiles/r11/adamw_ema_step.txt
"""
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "vit-of-pytorch_amd")]
from vitmi import ops  # noqa: E402
from vitmi.engine import ArchConfig, FlatLayout  # noqa: E402
from vitmi.optim import adamw_chunk_table  # noqa: E402

HBM = 6.3e12  # achievable HBM bandwidth of one MI355X, bytes per second
FUSED_B, PIECES_B = 38, 42  # bytes per element: 20 read + 18 written; (16 + 14) + (8 + 4)


def say(*a):
    print(" ".join(str(x) for x in a), flush=True)


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters * 1e3  # us


def run(name, cfg, iters):
    lay = FlatLayout(cfg)
    n = lay.numel
    dev = "cuda"
    g_ = torch.Generator(device=dev).manual_seed(0)
    p = torch.randn(n, device=dev, generator=g_) * 0.02
    g = torch.randn(n, device=dev, generator=g_) * 1e-3
    m = torch.zeros(n, device=dev)
    v = torch.rand(n, device=dev, generator=g_) * 1e-6 + 1e-8
    ema = p.clone()
    mirror = torch.zeros(n, device=dev, dtype=torch.bfloat16)
    chunks = adamw_chunk_table(lay).pin_memory()
    steps, used, table = torch.zeros(1, device=dev), torch.ones(1, device=dev), torch.zeros(4, device=dev)
    ops.adamw_prep(None, used, steps, 1e-3, 0.9, 0.999, 0.0, table, None)
    rows = [[0, at, min(8192, n - at)] for at in range(0, n, 8192)]
    chunks_dev = torch.tensor(rows, dtype=torch.int64).to(dev)
    hp = (1e-3, 0.9, 0.999, 1e-8, 0.05)
    fused = lambda wg=False: ops.adamw_ema_update(p, g, m, v, mirror, ema, chunks, table, *hp, 0.9999, wg)
    fused_noema = lambda: ops.adamw_ema_update(p, g, m, v, mirror, None, chunks, table, *hp, None, False)
    upd_only = lambda: ops.adamw_update(p, g, m, v, mirror, chunks_dev, table.view(1, 4), *hp, False)

    def pieces():
        upd_only()
        ops.axpby(p, ema, n, 1.0 - 0.9999, 0.9999)

    say(f"## {name}: {n} flat elements ({n * 4 / 1e9:.3f} GB per f32 buffer), {chunks.shape[0]} chunks, "
        f"{iters} launches per timing")
    for fn in (fused, pieces, fused_noema, upd_only):
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    floor = FUSED_B * n / HBM * 1e6
    for r in range(3):
        tf, tp = timed(fused, iters), timed(pieces, iters)
        say(f"round {r}: fused {tf:9.1f} us   parent pieces (adamw_update+mirror, axpby) {tp:9.1f} us   "
            f"fused/pieces {tf / tp:.3f}   fused: {FUSED_B * n / tf / 1e6:.2f} TB/s, {floor / tf:.3f} of the "
            f"{FUSED_B} B/elem floor at 6.3 TB/s ({floor:.1f} us)   pieces: {PIECES_B * n / tp / 1e6:.2f} TB/s of "
            f"their {PIECES_B} B/elem")
    tw = timed(lambda: fused(True), iters)
    say(f"fused, write_grad=1 (42 B/elem): {tw:9.1f} us, {42 * n / tw / 1e6:.2f} TB/s")
    tn, tu = timed(fused_noema, iters), timed(upd_only, iters)
    say(f"no EMA (30 B/elem): fused kernel {tn:9.1f} us ({30 * n / tn / 1e6:.2f} TB/s)   vit_adamw_update {tu:9.1f} us "
        f"({30 * n / tu / 1e6:.2f} TB/s)")
    assert bool(torch.isfinite(p).all())


if __name__ == "__main__":
    if not torch.cuda.is_available():
        raise SystemExit("tools/adamw_ema_bench.py times kernels: it needs the GPU")
    say("# vit_adamw_ema_update (EMA and bf16 mirror on) vs vit_adamw_update(mirror) + vit_axpby, same buffers, "
        "HIP events")
    say("# bytes per element: fused 20 read + 18 written = 38; pieces (16 read + 14 written) + (8 read + 4 written) "
        "= 42")
    run("ViT-B/16 @224, 1000 classes", ArchConfig(), 100)
    run("ViT-H/14 @224, 1000 classes",
        ArchConfig(patch_size=14, emb_dim=1280, mlp_dim=5120, num_heads=16, num_layers=32), 20)
