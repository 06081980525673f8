"""What stochastic depth costs on the GPU: ViT-B/16 training steps at batch 256 with --drop-path-rate 0 and 0.1.

    python tools/drop_path_bench.py [--out profiles/r12/drop_path_cost.txt] [--steps 20] [--repeats 5]
                                    [--bench-lines FILE ...]

One model, one synthetic HBM-resident batch; a step is forward, vitmi.model.CrossEntropyLoss, backward and the
vitmi.optim.SGD step, as bench.py's user path. After a warm-up of both rates (the first step with drop-path allocates
nothing new, but loads its kernels), `--repeats` blocks of `--steps` steps are timed per rate with a host clock around
a device synchronise, the two rates alternating within each repeat so that both see the same machine. Rate 0 launches
exactly the kernels of a model without the keyword; rate 0.1 adds the one table launch per forward, runs 22 of the 24
residual GEMMs on the drop-path epilogues and 22 LayerNorm backwards on their drop-path form, and turns the cls-only
last layer off. Both ms/step series, their medians and the spread go to --out.
--bench-lines: files whose last JSON line is a bench.py result; their ms_per_step are copied into the report under
the files' names (the default step itself is timed by bench.py, not here).
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "vit-of-pytorch_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

from vitmi.model import CrossEntropyLoss, VisionTransformer  # noqa: E402
from vitmi.optim import SGD  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batch-size", type=int, default=256)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rate", type=float, default=0.1)
    ap.add_argument("--bench-lines", nargs="*", default=[])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("drop_path_bench: needs the GPU (no fallback)")
    dev = "cuda:0"
    torch.manual_seed(0)
    model = VisionTransformer(image_size=(224, 224), patch_size=(16, 16), emb_dim=768, mlp_dim=3072, num_heads=12,
                              num_layers=12, num_classes=1000, dropout_rate=0.0).to(dev).train()
    crit = CrossEntropyLoss()
    opt = SGD(model.parameters(), lr=0.01, momentum=0.9, weight_decay=0.0, model=model)
    g = torch.Generator().manual_seed(7)
    x = torch.randn(args.batch_size, 3, 224, 224, generator=g).to(dev)
    y = torch.randint(0, 1000, (args.batch_size,), generator=g).to(dev)

    def block(rate, n):
        model.drop_path_rate = rate
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            opt.zero_grad(set_to_none=True)
            crit(model(x), y).backward()
            opt.step()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / n

    rates = (0.0, args.rate)
    for r in rates:
        block(r, args.warmup)
    series = {r: [] for r in rates}
    for _ in range(args.repeats):
        for r in rates:
            series[r].append(block(r, args.steps))
    lines = [f"ViT-B/16 224 px, batch {args.batch_size}, forward + loss + backward + SGD step; {args.repeats} repeats of "
             f"{args.steps} steps per rate, alternating; ms/step"]
    med = {}
    for r in rates:
        s = series[r]
        med[r] = statistics.median(s)
        lines.append(f"drop_path_rate {r:g}: " + " ".join(f"{v:.2f}" for v in s) +
                     f" | median {med[r]:.2f} spread {max(s) - min(s):.2f}")
    lines.append(f"cost of rate {args.rate:g}: {med[args.rate] - med[0.0]:+.2f} ms/step "
                 f"({100.0 * (med[args.rate] / med[0.0] - 1.0):+.2f}%)")
    for f in args.bench_lines:
        try:
            last = [ln for ln in open(f).read().splitlines() if ln.startswith("{")][-1]
            lines.append(f"bench.py {os.path.basename(f)}: ms_per_step {json.loads(last).get('ms_per_step')}")
        except (OSError, IndexError, ValueError) as e:
            lines.append(f"bench.py {os.path.basename(f)}: unreadable ({e})")
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
