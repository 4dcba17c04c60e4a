#!/usr/bin/env python3
"""What several noise draws per window cost in a training step (training.train_step(draws=K)), measured in ONE process in alternating
blocks.  Per config and K, four arms on the same model and data:

    a   today's step on C windows (draws = 1): the floor - one encoder pass, C trajectories
    b   train_step(draws=K): encoders once, the context's K | V projected once per window, the shared cross-attention kernels
    c   train_step(draws=K) under SD_TRAIN_SHARED=0: encoders once, the context expanded to one copy per draw, the existing kernels
    d   today's step on C K repeated windows: what the same number of noise samples costs now

Configs: default.yaml's and sim_scratch.yaml's full models with images (10 frames of 224 x 224, ResNet-18) at their batch sizes (64 / 16
windows) and decoder_only.yaml (256 windows, 10 random context rows).  Arm d is skipped where C K exceeds --max-windows image windows
(activation memory of the backbone) and the line says so.  Writes one JSON line per (config, K, arm) to profiles/noise_draws_bench.jsonl:
the median over the blocks of a block's mean milliseconds per step and the blocks' spread (min, max).  No figure is a pass bar."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from soccerdiffusion_amd import cli, training  # noqa: E402
from soccerdiffusion_amd.scheduler import DDIMScheduler  # noqa: E402

BASE = dict(action_context_length=100, trajectory_prediction_length=10, epochs=1, lr=1e-4, train_denoising_timesteps=1000, image_context_length=10,
            imu_context_length=100, joint_state_context_length=100, num_normalization_samples=10, num_joints=20, image_sequence_encoder_type="transformer",
            image_encoder_type="resnet18", num_image_sequence_encoder_layers=1, image_resolution=224, image_use_final_avgpool=False,
            distill_teacher_inference_steps=30)
CONFIGS = {
    "default": dict(hidden_dim=128, batch_size=64, use_images=True, use_action_history=True, num_action_history_encoder_layers=2, use_imu=True,
                    imu_orientation_embedding_method="quaternion", num_imu_encoder_layers=2, use_joint_states=True, joint_state_encoder_layers=2,
                    num_decoder_layers=4, use_gamestate=True, encoder_patch_size=1),
    "sim_scratch": dict(hidden_dim=256, batch_size=16, use_images=True, use_action_history=True, num_action_history_encoder_layers=4, use_imu=True,
                        imu_orientation_embedding_method="five_dim", num_imu_encoder_layers=2, use_joint_states=False, joint_state_encoder_layers=4,
                        num_decoder_layers=6, use_gamestate=False, encoder_patch_size=5),
    "decoder_only": dict(hidden_dim=256, batch_size=256, use_images=False, use_action_history=False, num_action_history_encoder_layers=2, use_imu=False,
                         imu_orientation_embedding_method="quaternion", num_imu_encoder_layers=2, use_joint_states=False, joint_state_encoder_layers=2,
                         num_decoder_layers=4, use_gamestate=False, encoder_patch_size=10),
}
ARMS = ("a", "b", "c", "d")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", type=str, default="default,sim_scratch,decoder_only")
    ap.add_argument("--draws", type=str, default="4,8")
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--iters", type=int, default=3, help="steps per block and arm")
    ap.add_argument("--max-windows", type=int, default=256, help="arm d is skipped above this many image windows")
    ap.add_argument("--output", type=str, default=os.path.join(REPO, "profiles", "noise_draws_bench.jsonl"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    lines = []
    for name in args.configs.split(","):
        params = {**BASE, **CONFIGS[name]}
        C = params["batch_size"]
        torch.manual_seed(0)
        model = cli.build_model(params).to(dev).train()
        model.set_dropout(0.1, seed=1)
        opt = training.FusedAdamW(model.parameters(), lr=1e-4)
        ns = DDIMScheduler(beta_schedule="squaredcos_cap_v2", clip_sample=False)
        gen = torch.Generator(device=dev).manual_seed(2)
        data = {k: v.to(dev) for k, v in cli.synthetic_dataset(C, params, seed=3, image_size=(224, 224)).items()}
        targets = (data["joint_command"] - 3.14159).contiguous()
        inp = {k: data[k].contiguous() for k in cli.CONTEXT_KEYS if k in data}
        full = bool(inp) and any(params[k] for k in ("use_images", "use_action_history", "use_imu", "use_joint_states", "use_gamestate"))
        ctx = None if full else [torch.randn(C, 10, params["hidden_dim"], device=dev, generator=gen)]

        def step(arm, K):
            kw = dict(world_size=1, generator=gen)
            if arm == "d":
                rep = lambda t: t.repeat_interleave(K, 0)   # noqa: E731
                src = dict(input_data={k: rep(v) for k, v in inp.items()}) if full else dict(context=[rep(c) for c in ctx])
                return training.train_step(model, opt, None, ns, rep(targets), **src, **kw)
            src = dict(input_data=inp) if full else dict(context=ctx)
            if arm == "a":
                return training.train_step(model, opt, None, ns, targets, **src, **kw)
            if arm == "c":
                os.environ["SD_TRAIN_SHARED"] = "0"
            try:
                return training.train_step(model, opt, None, ns, targets, draws=K, **src, **kw)
            finally:
                os.environ.pop("SD_TRAIN_SHARED", None)

        def run(arm, K, n):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n):
                step(arm, K)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / n * 1e3

        for K in (int(v) for v in args.draws.split(",")):
            arms = [a for a in ARMS if not (a == "d" and params["use_images"] and C * K > args.max_windows)]
            shared, expanded = training.SHARED_STACKS[0], training.EXPANDED_CONTEXTS[0]
            for arm in arms:   # warm-up: lazy initialisations, the allocator's pools
                print(f"[bench_noise_draws] {name} K={K} warm-up {arm}: {run(arm, K, 1):.1f} ms", file=sys.stderr, flush=True)
            routes = {"b": "shared" if training.SHARED_STACKS[0] > shared else "expanded", "c": "expanded" if training.EXPANDED_CONTEXTS[0] > expanded else "?"}
            per_block = {arm: [] for arm in arms}
            for b in range(args.blocks):
                for arm in arms:
                    per_block[arm].append(run(arm, K, args.iters))
                print(f"[bench_noise_draws] {name} K={K} block {b}: " + ", ".join(f"{a} {per_block[a][-1]:.2f}" for a in arms), file=sys.stderr, flush=True)
            for arm in ARMS:
                rec = {"what": "training step, ms", "config": name, "windows": C, "draws": K, "arm": arm, "trajectories": C * (1 if arm == "a" else K),
                       "hidden_dim": params["hidden_dim"], "images": bool(params["use_images"]), "dropout": 0.1}
                if arm in per_block:
                    v = per_block[arm]
                    rec.update({"route": routes.get(arm, "draws = 1"), "blocks": args.blocks, "iters_per_block": args.iters,
                                "median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3)})
                else:
                    rec["skipped"] = f"{C * K} image windows exceed --max-windows {args.max_windows}"
                rec["device"] = torch.cuda.get_device_name(0)
                lines.append(rec)
            torch.cuda.empty_cache()
        del model, opt, data, inp
        torch.cuda.empty_cache()
    with open(args.output, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")
            print(json.dumps(line))


if __name__ == "__main__":
    main()
