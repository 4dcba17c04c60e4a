#!/usr/bin/env python3
"""Secondary metric: training trajectories/s (one fwd + bwd + AdamW per trajectory) at BASELINE
config 2: decoder d=256, L=4, B=256, T=100, J=20, M=11 (decoder-pretraining path), fp32.
N>1 under torchrun: data parallel, one flat-gradient all-reduce per step.
--ema-decay D: the same step with the weight EMA riding in the AdamW launch (FusedAdamW(ema_decay=D)).
--clip X: what gradient clipping costs (FusedAdamW(max_grad_norm=...)), on the replayed graph (training.GraphedTrainStep) and in ONE
process: three legs - clipping off, the guard alone (inf) and X - from the same seed, timed in alternating blocks of --steps replays,
--blocks times round; one JSON line per leg with the median block, the blocks' spread and the clipping coefficient after every block
(< 1 throughout: X bound), then one line with the differences of the medians."""
import argparse, json, os, sys, time
import torch
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--ema-decay", type=float, default=None)
    ap.add_argument("--clip", type=float, default=None, metavar="X")
    ap.add_argument("--blocks", type=int, default=7)
    args = ap.parse_args()
    rank, world, local = int(os.environ.get("RANK", 0)), int(os.environ.get("WORLD_SIZE", 1)), int(os.environ.get("LOCAL_RANK", 0))
    dev = torch.device("cuda", local)
    torch.cuda.set_device(dev)
    if world > 1:
        import torch.distributed as dist
        dist.init_process_group("nccl", device_id=dev)
    from soccerdiffusion_amd import cli, training
    from soccerdiffusion_amd.scheduler import DDIMScheduler
    params = dict(hidden_dim=256, action_context_length=100, trajectory_prediction_length=100, epochs=1, batch_size=args.batch,
                  lr=1e-4, train_denoising_timesteps=1000, image_context_length=10, imu_context_length=100,
                  num_imu_encoder_layers=2, joint_state_context_length=100, num_normalization_samples=1000, num_joints=20,
                  use_action_history=False, num_action_history_encoder_layers=2, use_imu=False,
                  imu_orientation_embedding_method="quaternion", use_joint_states=False, joint_state_encoder_layers=2,
                  use_images=False, image_sequence_encoder_type="transformer", image_encoder_type="resnet18",
                  num_image_sequence_encoder_layers=1, num_decoder_layers=4, distill_teacher_inference_steps=30,
                  use_gamestate=False, encoder_patch_size=10)
    if args.clip is not None:
        if world > 1:
            sys.exit("--clip measures the replayed single-GPU step")
        return clip_blocks(args, params, dev)
    torch.manual_seed(0)
    model = cli.build_model(params).to(dev).train()
    opt = training.FusedAdamW(model.parameters(), lr=1e-4, ema_decay=args.ema_decay)
    sched = torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=1e-4, total_steps=args.steps + args.warmup + 1)
    ns = DDIMScheduler(beta_schedule="squaredcos_cap_v2", clip_sample=False)
    B = args.batch
    g = torch.Generator(device=dev).manual_seed(1 + rank)
    x0 = torch.randn(B, 100, 20, device=dev, generator=g)
    ctx = [torch.randn(B, 10, 256, device=dev, generator=g)]

    def step():
        return training.train_step(model, opt, sched, ns, x0, context=ctx, world_size=world, generator=g)

    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        loss = step()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    dt = time.perf_counter() - t0
    if rank == 0:
        flops = 3 * 478_478_336 * B * world * args.steps
        print(json.dumps({"metric": "training trajectories/s (fwd+bwd+AdamW, d=256 L=4 T=100 J=20 M=11, fp32)",
                          "value": round(world * B * args.steps / dt, 1), "n_gpus": world, "ms_per_step": round(dt / args.steps * 1e3, 3),
                          "batch_per_gpu": B, "algorithmic_tflops": round(flops / dt / 1e12, 2), "loss": float(loss),
                          **({} if args.ema_decay is None else {"ema_decay": args.ema_decay, "ema_floats": opt.flat_ema.numel()})}))
    if world > 1:
        dist.destroy_process_group()


def clip_blocks(args, params, dev):
    import statistics
    from soccerdiffusion_amd import cli, training
    from soccerdiffusion_amd.scheduler import DDIMScheduler
    B = args.batch
    ns = DDIMScheduler(beta_schedule="squaredcos_cap_v2", clip_sample=False)
    total = args.steps * args.blocks + args.warmup + 8

    def leg(max_grad_norm):
        torch.manual_seed(0)
        model = cli.build_model(params).to(dev).train()
        model.set_dropout(0.1, seed=1234)   # as bench.py --mode train
        opt = training.FusedAdamW(model.parameters(), lr=1e-4, ema_decay=args.ema_decay, max_grad_norm=max_grad_norm)
        sched = torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=1e-4, total_steps=total)
        g = torch.Generator(device=dev).manual_seed(1)
        x0 = torch.randn(B, 100, 20, device=dev, generator=g)
        ctx = [torch.randn(B, 10, 256, device=dev, generator=g)]
        gs = training.GraphedTrainStep(model, opt, sched, ns, generator=g)
        return {"opt": opt, "gs": gs, "x0": x0, "ctx": ctx, "ms": [], "coef": []}

    def run(l, n):
        for _ in range(n):
            l["gs"](l["x0"], context=l["ctx"])

    legs = {"off": leg(None), "inf": leg(float("inf")), "clip": leg(args.clip)}
    for l in legs.values():   # the eager steps, the capture, the first replays
        run(l, args.warmup + 3)
    torch.cuda.synchronize()
    for _ in range(args.blocks):
        for l in legs.values():
            t0 = time.perf_counter()
            run(l, args.steps)
            torch.cuda.synchronize()
            l["ms"].append((time.perf_counter() - t0) / args.steps * 1e3)
            l["coef"].append(None if l["opt"].max_grad_norm is None else l["opt"].grad_stats()["coef"])   # (outside the timed window)
    med = {}
    for name, l in legs.items():
        med[name] = statistics.median(l["ms"])
        print(json.dumps({"leg": name, "max_grad_norm": "inf" if l["opt"].max_grad_norm == float("inf") else l["opt"].max_grad_norm, "median_ms_per_step": round(med[name], 4),
                          "min_ms": round(min(l["ms"]), 4), "max_ms": round(max(l["ms"]), 4), "blocks_ms": [round(t, 4) for t in l["ms"]],
                          "steps_per_block": args.steps, "batch": B, "graph_replay": l["gs"].graph is not None,
                          "coef_after_block": l["coef"], "grad_stats": None if name == "off" else l["opt"].grad_stats(), "flat_grad_floats": l["opt"].flat_grad.numel(),
                          **({} if args.ema_decay is None else {"ema_decay": args.ema_decay})}), flush=True)
    spread = max(max(l["ms"]) - min(l["ms"]) for l in legs.values())
    print(json.dumps({"metric": "ms per replayed training step, clipping on minus off (medians of alternating blocks)",
                      "inf_minus_off_ms": round(med["inf"] - med["off"], 4),
                      "clip_minus_off_ms": round(med["clip"] - med["off"], 4), "largest_block_spread_ms": round(spread, 4)}), flush=True)
    for l in legs.values():
        l["gs"].close()


if __name__ == "__main__":
    main()
