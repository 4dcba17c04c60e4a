#!/usr/bin/env python3
"""Device time of the session's camera intake (sd_camera_intake: 480 x 640 -> 224 x 224, cv2.resize's INTER_LINEAR + normalisation) next to
the dataset's image feed (sd_frames_area: 480 x 480 -> 224 x 224, INTER_AREA's generic path) at 2, 32 and 128 frames.  Both kernels are
timed in the same process with HIP events around a run of --launches launches, in alternating blocks; a figure is the median over the blocks,
with the extremes.  Achieved bytes per second counts what the algorithm has to move: H W 3 source bytes + 12 R^2 output bytes per frame.
usage: python tools/bench_intake.py [--blocks 9] [--launches 50] [--out profiles/session_raw_intake.jsonl]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from soccerdiffusion_amd import ops  # noqa: E402

R = 224
CAMERA = (480, 640)


def block_us(fn, launches):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(launches):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / launches * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=9)
    ap.add_argument("--launches", type=int, default=50, help="launches per block")
    ap.add_argument("--out", type=str, default=None, help="also write the JSON lines to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_intake.py measures on the GPU: no device found")
    g = torch.Generator().manual_seed(3)
    lines = []
    for n in (2, 32, 128):
        cam = torch.randint(0, 256, (n, *CAMERA, 3), dtype=torch.uint8, generator=g).cuda()
        store = torch.randint(0, 256, (n, ops.FRAME_SIZE, ops.FRAME_SIZE, 3), dtype=torch.uint8, generator=g).cuda()
        index = torch.arange(n, device="cuda")
        out = torch.empty(n, 3, R, R, device="cuda")
        kernels = {"camera_intake_linear": (lambda: ops.camera_intake(cam, R, out=out), CAMERA),
                   "frames_area": (lambda: ops.frames_area(store, index, R, out=out), (ops.FRAME_SIZE, ops.FRAME_SIZE))}
        for fn, _ in kernels.values():                       # warm-up: code objects, the tap tables
            block_us(fn, args.launches)
        times = {k: [] for k in kernels}
        for _ in range(args.blocks):                         # alternating blocks: drift of the box hits both
            for k, (fn, _) in kernels.items():
                times[k].append(block_us(fn, args.launches))
        rec = {"frames": n, "R": R, "blocks": args.blocks, "launches_per_block": args.launches}
        for k, (_, (H, W)) in kernels.items():
            med, nbytes = statistics.median(times[k]), n * (H * W * 3 + 12 * R * R)
            rec[k] = {"source": [H, W], "us": {"median": round(med, 2), "min": round(min(times[k]), 2), "max": round(max(times[k]), 2)},
                      "bytes": nbytes, "GB_per_s": round(nbytes / med * 1e-3, 1)}
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
