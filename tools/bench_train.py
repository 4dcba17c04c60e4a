#!/usr/bin/env python3
"""Secondary metric: training trajectories/s (one fwd + bwd + AdamW per trajectory) at BASELINE
config 2: decoder d=256, L=4, B=256, T=100, J=20, M=11 (decoder-pretraining path), fp32.
N>1 under torchrun: data parallel, one flat-gradient all-reduce per step.
--ema-decay D: the same step with the weight EMA riding in the AdamW launch (FusedAdamW(ema_decay=D))."""
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


if __name__ == "__main__":
    main()
