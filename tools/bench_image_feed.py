"""Times the image feed's batch assembly at default.yaml's B = 64 x 10 frames: the area-resampling kernel (ops.frames_area, one launch:
gather + INTER_AREA + normalisation + layout) at R = 224 and R = 240, against the torch route the feed took before it (gather -> float ->
block mean -> normalise -> movedim -> scatter, dataset._preprocess) at R = 240 on the same frames.  Effective bandwidth = distinct frame
bytes read + output bytes, over the median of device-event times around one call.  Then the ResNet-18 encoder heads, forward + backward
(conv_training.ResNetHead on csrc/sd_head.hip against nn.Conv2d / nn.Linear on the permuted map): the no-avgpool head at 640 frames of 224
(7 x 7 x 512 maps, d = 128) and the avgpool head at 160 frames of 480 x 640 (15 x 20 x 512 maps, d = 256).  One JSON line per case.

    python tools/bench_image_feed.py [--iters 50] [--out profiles/image_feed.jsonl]
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import types

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

import torch  # noqa: E402

from soccerdiffusion_amd import ops  # noqa: E402
from soccerdiffusion_amd.dataset import SoccerDiffusionDataset  # noqa: E402


def _time(fn, iters: int) -> tuple:
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = []
    for _ in range(iters):
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts), min(ts)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_image_feed.py needs the MI355X (cuda:0)")
    dev = torch.device("cuda", 0)
    B, F, n_store = 64, 10, 1024
    g = torch.Generator().manual_seed(0)
    store = torch.randint(0, 256, (n_store, 480, 480, 3), dtype=torch.uint8, generator=g).to(dev)
    index = torch.randperm(n_store, generator=g)[: B * F].view(B, F).to(dev)     # 640 distinct frames
    lines = []

    def line(route, R, med, mn, extra=None):
        moved = B * F * 480 * 480 * 3 + B * F * 3 * R * R * 4
        d = {"what": "image_feed", "route": route, "R": R, "batch": B, "frames_per_sample": F, "ms_median": round(med, 4),
             "ms_min": round(mn, 4), "bytes_moved": moved, "tb_per_s": round(moved / (med * 1e-3) / 1e12, 3)}
        d.update(extra or {})
        lines.append(d)
        print(json.dumps(d), flush=True)

    outs = {}
    for R in (224, 240):
        out = torch.empty(B, F, 3, R, R, device=dev)
        med, mn = _time(lambda: ops.frames_area(store, index, R, out=out), args.iters)
        outs[R] = out.clone()
        line("kernel", R, med, mn)

    host = types.SimpleNamespace(image_resolution=240)

    def torch_route():
        out = torch.zeros(B, F, 3, 240, 240, device=dev)
        live = index >= 0
        out[live] = SoccerDiffusionDataset._preprocess(host, store[index[live]])
        return out

    med, mn = _time(torch_route, args.iters)
    diff = float((torch_route() - outs[240]).abs().max())
    line("torch", 240, med, mn, {"max_abs_diff_vs_kernel": diff})
    from torch import nn

    from soccerdiffusion_amd import conv_training as ct

    for name, n, H, W, d, conv in (("conv1x1", 640, 7, 7, 128, True), ("avgpool", 160, 15, 20, 256, False)):
        torch.manual_seed(0)
        pool = nn.Conv2d(512, 32, 1).to(dev) if conv else nn.AdaptiveAvgPool2d((1, 1))
        fc = nn.Linear(32 * H * W if conv else 512, d).to(dev)
        x = torch.relu(torch.randn(n, H, W, 512, device=dev)).requires_grad_()
        dy = torch.randn(n, d, device=dev)

        def hip():
            ct.resnet_head(x, pool if conv else None, fc).backward(dy)

        def torch_head():
            fc(torch.flatten(pool(x.permute(0, 3, 1, 2)), 1)).backward(dy)

        t_hip, t_torch = _time(hip, args.iters), _time(torch_head, args.iters)
        d_ = {"what": "resnet_head_fwd_bwd", "head": name, "frames": n, "map": [H, W, 512], "d": d, "hip_ms_median": round(t_hip[0], 4),
              "hip_ms_min": round(t_hip[1], 4), "torch_ms_median": round(t_torch[0], 4), "torch_ms_min": round(t_torch[1], 4)}
        lines.append(d_)
        print(json.dumps(d_), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.writelines(json.dumps(d) + "\n" for d in lines)
    return 0


if __name__ == "__main__":
    sys.exit(main())
