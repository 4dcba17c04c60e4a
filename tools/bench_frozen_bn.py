#!/usr/bin/env python3
"""What frozen BatchNorm statistics cost or save in the image encoder's training step (forward + backward of the per-frame ResNet-18
encoder, the 57 of 63 ms of an image-conditioned step), measured in ONE process in alternating blocks:

    train   every BatchNorm2d on batch statistics (the parent's only route on the hand-written kernels)
    stats   freeze_batchnorm(affine=False): running statistics, the affine pair trained (conv_raw + sd_bn_frozen_fwd / _bwd)
    all     freeze_batchnorm(affine=True): the inference launch forward, one element-wise launch backward per unit
    all_torch   the same modules under SD_CONV=torch (torch.nn / MIOpen, MIOPEN_FIND_MODE=FAST): the only correct route before

Shapes: the configs[4] per-GPU share, 16 windows x 10 frames of 480 x 640, and sim_scratch.yaml's 16 x 10 frames of 224 x 224.
Writes one JSON line per shape and arm to profiles/frozen_bn_bench.jsonl: the median over the blocks of a block's mean milliseconds per
iteration, and the blocks' spread (min, max)."""
import argparse
import copy
import json
import os
import statistics
import sys
import time

os.environ.setdefault("MIOPEN_FIND_MODE", "FAST")
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from soccerdiffusion_amd.ml.model.encoder.image import ImageEncoderType, ResNetImageEncoder, freeze_batchnorm

ARMS = ("train", "stats", "all", "all_torch")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=16)
    ap.add_argument("--frames", type=int, default=10)
    ap.add_argument("--sizes", type=str, default="480x640,224x224")
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--iters", type=int, default=3, help="iterations per block and arm")
    ap.add_argument("--arms", type=str, default=",".join(ARMS))
    ap.add_argument("--output", type=str, default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "frozen_bn_bench.jsonl"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    arms = [a for a in args.arms.split(",") if a]
    lines = []
    for size in args.sizes.split(","):
        H, W = (int(v) for v in size.split("x"))
        torch.manual_seed(0)
        base = ResNetImageEncoder(ImageEncoderType.RESNET18, 256, True, H).to(dev)
        x = torch.rand(args.windows, args.frames, 3, H, W, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
        encs = {}
        for arm in arms:
            enc = copy.deepcopy(base)
            if arm != "train":
                freeze_batchnorm(enc, affine=arm != "stats")
            encs[arm] = enc.train()

        def run(arm, n):
            enc = encs[arm]
            if arm == "all_torch":
                os.environ["SD_CONV"] = "torch"
            try:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(n):
                    for p in enc.parameters():
                        p.grad = None
                    enc(x).sum().backward()
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) / n * 1e3
            finally:
                os.environ.pop("SD_CONV", None)

        for arm in arms:   # warm-up: lazy initialisations, the allocator's pools, MIOpen's kernel selection
            print(f"[bench_frozen_bn] {size} warm-up {arm}: {run(arm, 1):.1f} ms", file=sys.stderr, flush=True)
        per_block = {arm: [] for arm in arms}
        for b in range(args.blocks):
            for arm in arms:
                per_block[arm].append(run(arm, args.iters))
            print(f"[bench_frozen_bn] {size} block {b}: " + ", ".join(f"{a} {per_block[a][-1]:.2f}" for a in arms), file=sys.stderr, flush=True)
        for arm in arms:
            v = per_block[arm]
            lines.append({"what": "image encoder forward + backward, ms per iteration", "arm": arm, "size": size, "windows": args.windows,
                          "frames": args.frames, "blocks": args.blocks, "iters_per_block": args.iters, "median_ms": round(statistics.median(v), 3),
                          "min_ms": round(min(v), 3), "max_ms": round(max(v), 3), "device": torch.cuda.get_device_name(0)})
        del encs, x, base
        torch.cuda.empty_cache()
    with open(args.output, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")
            print(json.dumps(line))


if __name__ == "__main__":
    main()
