#!/usr/bin/env python3
"""Swin-T / Swin-S image-encoder forward (inference: eval mode, no tape) at 224 x 224 on the hand-written kernels (csrc/sd_swin.hip) versus
the torch-op route (SD_SWIN=torch: hipBLASLt GEMMs + ATen element-wise kernels), in one process, the two routes alternating.  Frame counts:
10 (one robot control step, ros.py), 160 and 640 (default.yaml: batch 64 x 10 frames).  Device events around each forward after warm-up;
median of the repeats.  Prints one JSON line: per (model, frames) both routes' ms, the speedup, the algorithmic GFLOP of one forward (from
the shapes: every GEMM, the attention products over whole 7 x 7 windows, the patch embedding) and the max relative difference of the two
routes' output tokens (max-abs / max-abs)."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from soccerdiffusion_amd.ml.model.encoder.image import ImageEncoderType, image_encoder_factory  # noqa: E402


def swin_flops(depths, hidden, H=224, W=224, window=7) -> float:
    """Algorithmic FLOPs (2 per multiply-add) of one frame's forward."""
    h, w, C = H // 4, W // 4, 96
    f = 2.0 * h * w * 96 * 48   # patch embedding
    for stage, depth in enumerate(depths):
        T, heads = h * w, C // 32
        nW = -(-h // window) * -(-w // window)
        per_block = 2.0 * T * C * 3 * C + 2.0 * T * C * C + 2 * 2.0 * T * C * 4 * C   # qkv, proj, fc1, fc2
        per_block += nW * heads * 2 * (2.0 * window ** 4 * 32)                         # q k^T and p v per window and head
        f += depth * per_block
        if stage < len(depths) - 1:
            h, w = (h + 1) // 2, (w + 1) // 2
            f += 2.0 * h * w * 4 * C * 2 * C                                           # patch merging reduction
            C *= 2
    return f + 2.0 * C * hidden


def timed(fn, reps):
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=str, default="10,160,640")
    ap.add_argument("--models", type=str, default="tiny,small")
    ap.add_argument("--hidden", type=int, default=256)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    kinds = {"tiny": (ImageEncoderType.SWIN_TRANSFORMER_TINY, (2, 2, 6, 2)), "small": (ImageEncoderType.SWIN_TRANSFORMER_SMALL, (2, 2, 18, 2))}
    rows = []
    for name in args.models.split(","):
        kind, depths = kinds[name]
        torch.manual_seed(0)
        enc = image_encoder_factory(kind, args.hidden, True, 224).encoder.to(dev).eval()
        for frames in (int(v) for v in args.frames.split(",")):
            x = torch.rand(frames, 3, 224, 224, device=dev) * 2.0 - 0.7
            out = {}

            def hip():
                out["hip"] = enc(x)

            def torch_route():
                os.environ["SD_SWIN"] = "torch"
                try:
                    out["torch"] = enc(x)
                finally:
                    del os.environ["SD_SWIN"]

            reps = max(3, args.reps if frames <= 160 else args.reps // 2)
            with torch.no_grad():
                for _ in range(args.warmup):
                    hip()
                    torch_route()
                torch.cuda.synchronize()
                th, tt = [], []
                for _ in range(reps):   # alternate: both routes see the same clocks and heat
                    th += timed(hip, 1)
                    tt += timed(torch_route, 1)
            diff = float((out["hip"] - out["torch"]).abs().max() / out["torch"].abs().max())
            mh, mt = sorted(th)[len(th) // 2], sorted(tt)[len(tt) // 2]
            gflop = swin_flops(depths, args.hidden) * frames / 1e9
            rows.append({"model": f"swin_{name}", "frames": frames, "hip_ms": round(mh, 3), "torch_ms": round(mt, 3),
                         "speedup": round(mt / mh, 3), "gflop": round(gflop, 1), "hip_tflops": round(gflop / mh, 2),
                         "torch_tflops": round(gflop / mt, 2), "max_rel_diff": diff, "reps": reps})
            print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
            del x, out
            torch.cuda.empty_cache()
    print(json.dumps({"metric": "swin_encoder_forward_224", "device": torch.cuda.get_device_name(0), "hidden_dim": args.hidden,
                      "results": rows}))


if __name__ == "__main__":
    main()
