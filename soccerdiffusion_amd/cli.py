"""`train` and `sample` entry points with the flags, YAML schema and checkpoint dictionary of
the reference's scripts (soccer_diffusion/ml/training/train.py:26-253,
soccer_diffusion/ml/inference/plot.py:21-135).

    python -m soccerdiffusion_amd.cli train -c cfg.yaml [-p ckpt] [-o out] [--decoder-pretraining] [--pretrained-decoder p] [--ema-decay D [--no-ema-warmup]] [--clip-grad-norm X] [--freeze-bn stats|all] [--pretrained-backbone FILE]
    python -m soccerdiffusion_amd.cli sample ckpt [--steps 30] [--solver ddim|multistep] [--num_samples 10] [--ema] [--draws G] [--hold J=V[,J=V...]] [--limits J=LO:HI[,J=LO:HI...] | --clip R] [--reproject] [--slew V | J=V[,J=V...]] [--accel A | J=A[,J=A...]]
    python -m soccerdiffusion_amd.cli distill cfg.yaml teacher_ckpt [-o out] [--ema-teacher] [--ema-decay D [--no-ema-warmup]] [--clip-grad-norm X] [--freeze-bn stats|all]     (ml/training/distill.py:25-224)
    python -m soccerdiffusion_amd.cli evaluate ckpt --synthetic N [--val-fraction F | --all] [--steps 30] [--solver ddim|multistep] [--draws G] [--grid K | --timesteps a,b,..] [--ema] [--limits J=LO:HI[,J=LO:HI...] | --clip R] [--reproject] [--slew V | J=V[,J=V...]] [--accel A | J=A[,J=A...]] [-o report.json]   (evaluation.py)
    python -m soccerdiffusion_amd.cli rollout ckpt --synthetic N --ticks K [-o out.pt] [--steps 30] [--solver ddim|multistep] [--seed S] [--raw [--camera HxW]] [--ema] [--carry K [--advance S]] [--hold J=V[,J=V...]] [--limits J=LO:HI[,J=LO:HI...] | --clip R] [--reproject] [--slew V | J=V[,J=V...]] [--accel A | J=A[,J=A...]] [--draws G [--select medoid|coherent [--coherence-decay R] [--contrast L]]]   (ml/inference/ros.py:165-335)

Differences, all additive: data comes from the reference's SQLite database (`--db file`,
read once into HBM by soccerdiffusion_amd/dataset.py, image frames included), from a tensor
file (`--data file.pt`: dict with `joint_command` (N,T,J) and the optional context keys of
the reference's `Result` dataclass) or from a synthetic sine-wave generator (`--synthetic N`); wandb and matplotlib are not used; under torchrun
(WORLD_SIZE > 1) training is data parallel with one RCCL all-reduce of the flat gradient
per step and `sample` shards the rollouts over the ranks; `--ema-decay` keeps an exponential
moving average of the weights inside the optimizer step (optim.FusedAdamW) and the checkpoint
gains `ema_model_state_dict` and `ema`, which `--ema` / `--ema-teacher` load instead of the
last iterate (the reference's ml/preliminary scripts kept and sampled such an average);
`train` / `distill --clip-grad-norm X` clip the global gradient norm to X and skip a step whose gradient is not finite, inside the
optimizer step (`inf`: the guard alone); the printed line gains `GradNorm` / `Skipped` and the checkpoint `grad_clip`;
`train` / `distill --val-fraction F` hold the last (or a random) fraction of the windows out of training and of the normaliser fit,
evaluate them every `--val-every` epochs (evaluation.evaluate) and record the reports in the checkpoint's `validation` entry, and
`evaluate` prints that report for any checkpoint as one JSON line.
A distilled checkpoint (`distill`'s student: one forward at t = 0 whose output is the clean trajectory) takes `--limits`, `--clip`, `--slew`,
`--hold`, `--draws`, `--select`, `--coherence-decay` and `--contrast` on `sample`, `rollout` and `evaluate` (model.sample_direct projects
its output inside the launch); `--solver multistep`, `--carry` and `--reproject` exit with a message.
"""

from __future__ import annotations

import argparse
import logging
import math
import os
import sys
from typing import Optional

import torch
import yaml

logger = logging.getLogger("soccerdiffusion_amd")

CONTEXT_KEYS = ("joint_command_history", "rotation", "joint_state", "image_data", "game_state")


def build_model(params: dict):
    """End2EndDiffusionTransformer(**hyperparams) exactly as train.py:113-139 / plot.py:38-64 do."""
    from .ml.model import End2EndDiffusionTransformer
    from .ml.model.encoder.image import ImageEncoderType, SequenceEncoderType
    from .ml.model.encoder.imu import IMUEncoder

    return End2EndDiffusionTransformer(
        num_joints=params["num_joints"],
        hidden_dim=params["hidden_dim"],
        use_action_history=params["use_action_history"],
        num_action_history_encoder_layers=params["num_action_history_encoder_layers"],
        max_action_context_length=params["action_context_length"],
        use_imu=params["use_imu"],
        imu_orientation_embedding_method=IMUEncoder.OrientationEmbeddingMethod(params["imu_orientation_embedding_method"]),
        num_imu_encoder_layers=params["num_imu_encoder_layers"],
        imu_context_length=params["imu_context_length"],
        use_joint_states=params["use_joint_states"],
        joint_state_encoder_layers=params["joint_state_encoder_layers"],
        joint_state_context_length=params["joint_state_context_length"],
        use_images=params["use_images"],
        image_sequence_encoder_type=SequenceEncoderType(params["image_sequence_encoder_type"]),
        image_encoder_type=ImageEncoderType(params["image_encoder_type"]),
        num_image_sequence_encoder_layers=params["num_image_sequence_encoder_layers"],
        image_context_length=params["image_context_length"],
        image_use_final_avgpool=params.get("image_use_final_avgpool", True),
        image_resolution=params.get("image_resolution", 480),
        num_decoder_layers=params["num_decoder_layers"],
        trajectory_prediction_length=params["trajectory_prediction_length"],
        use_gamestate=params["use_gamestate"],
        encoder_patch_size=params["encoder_patch_size"],
    )


def synthetic_dataset(n: int, params: dict, seed: int = 0, image_size: Optional[tuple] = None) -> dict:
    """Sine-wave joints around pi (the reference stores angles in [0, 2pi)), random unit
    quaternions, random game states — shaped like the reference's `Result` fields."""
    g = torch.Generator().manual_seed(seed)
    J, T = params["num_joints"], params["trajectory_prediction_length"]
    Ha, Hi, Hj = params["action_context_length"], params["imu_context_length"], params["joint_state_context_length"]
    total = Ha + T
    phase = torch.rand(n, 1, J, generator=g) * 2 * math.pi
    freq = 0.5 + torch.rand(n, 1, J, generator=g)
    t = torch.arange(total).view(1, total, 1) / 50.0
    wave = math.pi + torch.sin(2 * math.pi * freq * t + phase)
    quat = torch.randn(n, Hi, 4, generator=g)
    quat = quat / quat.norm(dim=-1, keepdim=True)
    feat = 5 if params["imu_orientation_embedding_method"] == "five_dim" else 4
    rot = quat if feat == 4 else torch.cat([quat[..., :3], torch.sin(quat[..., 3:]), torch.cos(quat[..., 3:])], -1)
    extra = {}
    if params.get("use_images"):  # (n, F, 3, H, W) noise frames; the reference's dataset delivers square R x R ones
        R = params.get("image_resolution", 480)
        H, W = image_size if image_size is not None else (R, R)
        extra["image_data"] = torch.rand(n, params["image_context_length"], 3, H, W, generator=g)
    return {
        **extra,
        "joint_command": wave[:, Ha:].contiguous(),
        "joint_command_history": wave[:, :Ha].contiguous(),
        "joint_state": (wave[:, Ha - Hj : Ha] + 0.01 * torch.randn(n, Hj, J, generator=g)).contiguous(),
        "rotation": rot.contiguous(),
        "game_state": torch.randint(0, 4, (n,), generator=g),
    }


class DataSource:
    """Uniform access for the loops: number of samples, device batches by index, and the
    joint commands of a few samples for the normaliser fit."""

    def __init__(self, tensors: Optional[dict] = None, dataset=None, device=None):
        self.dataset = dataset.to(device) if dataset is not None else None
        self.tensors = {k: v.to(device) for k, v in tensors.items()} if tensors is not None else None
        self.n = len(dataset) if dataset is not None else tensors["joint_command"].shape[0]

    def batch(self, idx: torch.Tensor) -> dict:
        if self.dataset is not None:
            return self.dataset.batch(idx)
        dev = self.tensors["joint_command"].device
        return {k: v[idx.to(dev)] for k, v in self.tensors.items()}


def open_database(path: str, params: dict, device=None):
    """The reference's SQLite database (dataset/models.py schema) through the pre-extracting feed; ``device``: the run's GPU (the frames
    go there at construction and every image_resolution in 1 .. 480 is resampled by the feed's kernel)."""
    from .dataset import SoccerDiffusionDataset

    return SoccerDiffusionDataset(
        db_path=path, num_joints=params["num_joints"], num_frames_video=params["image_context_length"],
        num_samples_joint_trajectory_future=params["trajectory_prediction_length"],
        num_samples_joint_trajectory=params["action_context_length"], num_samples_imu=params["imu_context_length"],
        num_samples_joint_states=params["joint_state_context_length"],
        imu_representation=params["imu_orientation_embedding_method"], use_action_history=params["use_action_history"],
        use_imu=params["use_imu"], use_joint_states=params["use_joint_states"], use_images=params["use_images"],
        use_game_state=params["use_gamestate"], image_resolution=params.get("image_resolution", 480), device=device)


def data_source(args, params: dict, device) -> DataSource:
    chosen = [n for n in ("db", "data", "synthetic") if getattr(args, n, None) is not None]
    if len(chosen) != 1:
        raise SystemExit("give exactly one data source: --db FILE (the reference's SQLite database), --data FILE.pt "
                         f"or --synthetic N (got: {', '.join('--' + c for c in chosen) or 'none'})")
    if getattr(args, "db", None):
        return DataSource(dataset=open_database(args.db, params, device), device=device)
    return DataSource(tensors=load_data(args, params), device=device)


def load_data(args, params: dict) -> dict:
    if args.data:
        data = torch.load(args.data, map_location="cpu", weights_only=True)
        if "joint_command" not in data:
            raise SystemExit("--data file must hold a dict with a 'joint_command' (N, T, J) tensor")
        return data
    size = None
    if getattr(args, "image_size", None):
        try:
            h, w = (int(v) for v in args.image_size.lower().split("x"))
        except ValueError:
            raise SystemExit("--image-size expects HxW, e.g. 480x640") from None
        if h != w and not params.get("image_use_final_avgpool", True):
            raise SystemExit("non-square frames need image_use_final_avgpool: True (the no-avgpool head assumes a square map, "
                             "reference encoder/image.py:69-83)")
        size = (h, w)
    return synthetic_dataset(args.synthetic, params, seed=args.seed, image_size=size)


EMA_KEY = "ema_model_state_dict"


def ema_model_state(checkpoint: dict, flag: str, path: str) -> dict:
    """The EMA weights of a checkpoint for ``flag``; a checkpoint trained without --ema-decay ends the command."""
    if EMA_KEY not in checkpoint:
        raise SystemExit(f"{flag}: checkpoint {path} has no '{EMA_KEY}' (it was trained without --ema-decay)")
    return checkpoint[EMA_KEY]


def _ema_decay(text: str) -> float:
    try:
        value = float(text)
    except ValueError:
        value = float("nan")
    if not 0.0 < value < 1.0:
        raise argparse.ArgumentTypeError(f"--ema-decay takes a decay in the open interval (0, 1), got {text!r}")
    return value


def _restore_ema(optimizer, model, checkpoint: Optional[dict]) -> None:
    """The optimizer's EMA from the checkpoint's keys; a checkpoint without them leaves it at the loaded parameters."""
    if optimizer.flat_ema is None or checkpoint is None:
        return
    if EMA_KEY in checkpoint and "ema" in checkpoint:
        optimizer.load_ema_state_dict(model, checkpoint[EMA_KEY], checkpoint["ema"]["num_updates"])
    else:
        logger.warning("the checkpoint holds no EMA: the average starts from the loaded parameters")


def _ema_checkpoint_keys(optimizer, model) -> dict:
    if optimizer.flat_ema is None:
        return {}
    return {EMA_KEY: optimizer.ema_state_dict(model), "ema": optimizer.ema_state()}


def _clip_grad_norm(text: str) -> float:
    try:
        value = float(text)
    except ValueError:
        value = float("nan")
    if not value >= 0.0:   # (NaN fails the comparison)
        raise argparse.ArgumentTypeError(f"--clip-grad-norm takes a norm >= 0, or inf for the non-finite guard alone, got {text!r}")
    return value


def _grad_clip_suffix(optimizer) -> str:
    """What the printed iteration line gains with --clip-grad-norm (one device read, beside the loss's)."""
    if optimizer.max_grad_norm is None:
        return ""
    st = optimizer.grad_stats()
    return f", GradNorm: {st['norm']:.05f}, Skipped: {st['skipped_steps']}"


def _grad_clip_checkpoint_keys(optimizer) -> dict:
    if optimizer.max_grad_norm is None:
        return {}
    return {"grad_clip": {"max_norm": optimizer.max_grad_norm, "skipped_steps": optimizer.grad_stats()["skipped_steps"]}}


FREEZE_BN_MODES = ("stats", "all")


def validate_freeze_bn(mode: Optional[str], params: dict) -> Optional[str]:
    """``--freeze-bn`` against the run's hyperparameters: the mode, or the end of the command where there is no ResNet image encoder to freeze."""
    if mode is None:
        return None
    if mode not in FREEZE_BN_MODES:
        raise SystemExit(f"--freeze-bn takes one of {', '.join(FREEZE_BN_MODES)}, got {mode!r}")
    if not params.get("use_images"):
        raise SystemExit("--freeze-bn: this configuration has no image encoder (use_images is false)")
    if params.get("image_encoder_type") not in ("resnet18", "resnet50"):
        raise SystemExit(f"--freeze-bn: image_encoder_type {params.get('image_encoder_type')!r} has no BatchNorm layers (resnet18 / resnet50 only)")
    return mode


def apply_freeze_bn(model, mode: Optional[str]) -> None:
    """stats: every BatchNorm2d of the image encoder normalises with its running statistics and stops updating them; all: its weight and bias
    are frozen too (the optimizer is built afterwards and owns only what requires a gradient)."""
    if mode is not None:
        from .ml.model.encoder.image import freeze_batchnorm

        freeze_batchnorm(model.image_sequence_encoder, affine=mode == "all")


def _freeze_bn_checkpoint_keys(mode: Optional[str]) -> dict:
    return {} if mode is None else {"freeze_bn": mode}


def load_pretrained_backbone(model, path: str) -> tuple:
    """Loads a state dict with torchvision's ResNet keys (a torchvision checkpoint, or ``backbone.state_dict()`` of this package) into the
    image encoder's backbone: every tensor whose name and shape match, except the classifier ``fc.*`` (the encoder has its own head).
    -> (loaded names, skipped names); the skipped ones are logged."""
    from .ml.model.encoder.image import _ResNet

    enc = getattr(model, "image_sequence_encoder", None)
    backbone = None if enc is None else next((m for m in enc.modules() if isinstance(m, _ResNet)), None)
    if backbone is None:
        raise SystemExit("--pretrained-backbone: this configuration has no ResNet image encoder")
    state = torch.load(path, map_location="cpu", weights_only=True)
    own = backbone.state_dict()
    loaded, skipped = [], []
    for name, value in state.items():
        if not name.startswith("fc.") and name in own and tuple(own[name].shape) == tuple(value.shape):
            loaded.append(name)
        else:
            skipped.append(name)
    backbone.load_state_dict({k: state[k] for k in loaded}, strict=False)
    missing = [k for k in own if k not in loaded and not k.startswith("fc.")]
    logger.info("--pretrained-backbone: loaded %d tensors from %s", len(loaded), path)
    if skipped:
        logger.warning("--pretrained-backbone: not loaded from the file (fc.*, unknown name or other shape): %s", ", ".join(skipped))
    if missing:
        logger.warning("--pretrained-backbone: not in the file, left as initialised: %s", ", ".join(missing))
    return loaded, skipped


def shard_plan(n_total: int, batch_size: int, rank: int, world: int):
    """Sample indices of this rank and the number of optimizer steps per epoch, the SAME on every rank.

    world == 1: all samples, ceil(n / bs) steps, the last batch may be short (the reference's DataLoader default,
    train.py:199-201).  world > 1: every rank owns exactly n_total // world samples (every world-th one; the
    n_total % world trailing samples are dropped) and runs floor(per_rank / bs) full batches - at least one, possibly
    short, when per_rank < bs - so that every rank issues the same number of all-reduces and OneCycleLR gets the same
    total_steps everywhere."""
    if world <= 1:
        return torch.arange(n_total), max(1, math.ceil(n_total / batch_size))
    per_rank = n_total // world
    if per_rank == 0:
        raise SystemExit(f"{n_total} samples cannot be sharded over {world} ranks")
    shard = torch.arange(rank, per_rank * world, world)
    return shard, max(1, per_rank // batch_size)


def _dist_env():
    rank, world, local = int(os.environ.get("RANK", 0)), int(os.environ.get("WORLD_SIZE", 1)), int(os.environ.get("LOCAL_RANK", 0))
    if os.environ.get("SD_BENCH_SHARE_GPU") == "1":   # rehearsal of the multi-rank path on a 1-GPU box (tests): all ranks on cuda:0
        local = 0
    return rank, world, local


def _init_dist(device) -> None:
    import torch.distributed as dist

    if os.environ.get("SD_BENCH_SHARE_GPU") == "1":
        dist.init_process_group("gloo")
    else:
        dist.init_process_group("nccl", device_id=device)   # RCCL over xGMI


def cmd_train(args) -> int:
    assert args.config is not None or args.checkpoint is not None, "Either a config file or a checkpoint must be provided"
    from . import ops, training
    from .scheduler import DDIMScheduler

    rank, world, local = _dist_env()
    device = torch.device("cuda", local)
    torch.cuda.set_device(device)
    if world > 1:
        _init_dist(device)

    checkpoint = None
    params: dict = {}
    if args.checkpoint is not None:
        checkpoint = torch.load(args.checkpoint, map_location="cpu", weights_only=True)
        params = dict(checkpoint["hyperparams"])
    if args.config is not None:
        with open(args.config) as f:
            config_params = yaml.safe_load(f)
        if checkpoint is not None:  # train.py:57-70: differences are warned, then the YAML REPLACES the checkpoint's dict
            logger.warning("Both a configuration file and a checkpoint are provided. "
                           "The configuration file will be used for the hyperparameters.")
            for key, value in config_params.items():
                if key not in params:
                    logger.warning("Key '%s' is not present in the checkpoint", key)
                elif value != params[key]:
                    logger.warning("Key '%s' has a different value in the checkpoint: %r != %r", key, params[key], value)
        params = dict(config_params)
    if params["train_denoising_timesteps"] != 1000:
        raise SystemExit("train_denoising_timesteps must be 1000 (the scheduler table length; see scheduler.py)")
    # a resumed run goes on with its BatchNorm layers as they were
    freeze_bn = validate_freeze_bn(args.freeze_bn if args.freeze_bn is not None or checkpoint is None else checkpoint.get("freeze_bn"), params)
    noise_draws = noise_draws_of(args.noise_draws, checkpoint)   # a resumed run goes on with its draws per window
    if noise_draws > 1 and params.get("use_images") and str(params.get("image_encoder_type", "")).startswith("swin_transformer"):
        raise SystemExit("--noise-draws: not with a Swin image encoder (its training runs on torch's own modules; see README)")
    draws_kw = {} if noise_draws == 1 else {"draws": noise_draws}

    gen = torch.Generator().manual_seed(args.seed + rank)
    source = data_source(args, params, device)
    n_total = source.n
    val = _holdout(args, n_total)
    if val is None:
        norm_idx = torch.randint(0, n_total, (params["num_normalization_samples"],), generator=torch.Generator().manual_seed(args.seed))
    else:   # held-out windows are neither trained on nor seen by the normaliser
        norm_idx = val.train_idx[torch.randint(0, len(val.train_idx), (params["num_normalization_samples"],),
                                               generator=torch.Generator().manual_seed(args.seed))]
    from .dataset import fit_normalizer as fit_rows

    mean, std = fit_rows(source.batch(norm_idx)["joint_command"].cpu())  # train.py:108-110

    torch.manual_seed(args.seed)  # the same initial replica on every rank ...
    model = build_model(params).to(device)
    model.mean.copy_(mean)
    model.std.copy_(std)
    if checkpoint is not None:
        model.load_state_dict(checkpoint["model_state_dict"])
    if args.pretrained_decoder is not None:
        pre = torch.load(args.pretrained_decoder, map_location="cpu", weights_only=True)
        model.load_state_dict(pre["model_state_dict"], strict=False)
    if args.pretrained_backbone is not None:
        load_pretrained_backbone(model, args.pretrained_backbone)
    apply_freeze_bn(model, freeze_bn)   # (before the optimizer: it owns the parameters that require a gradient)
    model.train()
    model.set_dropout(args.dropout, seed=args.seed + 7919 * rank)   # every rank its own mask stream

    ema_decay, ema_warmup = args.ema_decay, not args.no_ema_warmup
    if ema_decay is None and checkpoint is not None and "ema" in checkpoint:   # a resumed run goes on averaging as it did
        ema_decay, ema_warmup = checkpoint["ema"]["decay"], checkpoint["ema"]["warmup"]
    max_grad_norm = args.clip_grad_norm
    if max_grad_norm is None and checkpoint is not None and "grad_clip" in checkpoint:   # ... and clipping as it did
        max_grad_norm = checkpoint["grad_clip"]["max_norm"]
    optimizer = training.FusedAdamW(model.parameters(), lr=params["lr"], ema_decay=ema_decay, ema_warmup=ema_warmup, max_grad_norm=max_grad_norm)
    if checkpoint is not None and "optimizer_state_dict" in checkpoint:
        optimizer.load_state_dict(checkpoint["optimizer_state_dict"])
    _restore_ema(optimizer, model, checkpoint)
    if max_grad_norm is not None and checkpoint is not None and "grad_clip" in checkpoint:
        optimizer.set_skipped_steps(checkpoint["grad_clip"]["skipped_steps"])
    if world > 1:  # ... and rank 0's parameters, moments and buffers are what every rank starts from, whatever happened above
        training.broadcast_parameters(optimizer, model)
    bs = params["batch_size"]
    if val is None:
        shard, steps_per_epoch = shard_plan(n_total, bs, rank, world)
    else:
        shard, steps_per_epoch = shard_plan(len(val.train_idx), bs, rank, world)
        shard = val.train_idx[shard]
    lr_scheduler = torch.optim.lr_scheduler.OneCycleLR(optimizer, max_lr=params["lr"], total_steps=params["epochs"] * steps_per_epoch)
    scheduler = DDIMScheduler(beta_schedule="squaredcos_cap_v2", clip_sample=False)
    scheduler.config["num_train_timesteps"] = params["train_denoising_timesteps"]

    dev_gen = torch.Generator(device=device).manual_seed(args.seed + 1000 * rank)
    for epoch in range(params["epochs"]):
        order = shard[torch.randperm(len(shard), generator=gen)]
        for i in range(steps_per_epoch):
            idx = order[i * bs : (i + 1) * bs]
            batch = source.batch(idx)
            targets = ops.normalize(batch["joint_command"].contiguous(), model.mean, model.std)
            if args.decoder_pretraining:
                ctx = [torch.randn((len(idx), 10, params["hidden_dim"]), device=device, generator=dev_gen)]
                loss = training.train_step(model, optimizer, lr_scheduler, scheduler, targets, context=ctx,
                                           world_size=world, generator=dev_gen, **draws_kw)
            else:
                inp = {k: batch[k].contiguous() for k in CONTEXT_KEYS if k in batch}
                loss = training.train_step(model, optimizer, lr_scheduler, scheduler, targets, input_data=inp,
                                           world_size=world, generator=dev_gen, **draws_kw)
            if i % 20 == 0 and rank == 0:
                print(f"Epoch {epoch}, it {i}, Loss: {float(loss):.05f}, LR: {lr_scheduler.get_last_lr()[0]:0.7f}{_grad_clip_suffix(optimizer)}", flush=True)
        if val is not None and rank == 0:   # (the other ranks wait at the collective below)
            val.run(model, optimizer, source, epoch, params["epochs"])
        training.assert_replicas_equal(optimizer)   # one pair of tiny all-reduces per epoch
        if rank == 0:
            torch.save({"model_state_dict": model.state_dict(), "optimizer_state_dict": optimizer.state_dict(),
                        "lr_scheduler_state_dict": lr_scheduler.state_dict(), "hyperparams": params,
                        "current_epoch": epoch, **_ema_checkpoint_keys(optimizer, model), **_grad_clip_checkpoint_keys(optimizer),
                        **_freeze_bn_checkpoint_keys(freeze_bn), **({} if noise_draws == 1 else {"noise_draws": noise_draws}),
                        **({} if val is None else {"validation": val.entry()})},
                       args.output)
    if world > 1:
        import torch.distributed as dist

        dist.barrier()
        dist.destroy_process_group()
    return 0


def cmd_distill(args) -> int:
    """Single-step distillation (reference ml/training/distill.py:155-221): per batch the teacher
    runs its `distill_teacher_inference_steps`-step DDIM rollout from pure noise under no_grad
    (one native call), the student predicts the sample in ONE forward at t = 0 re-using the
    teacher's context tokens, and is trained with MSE to the teacher's sample."""
    from . import training

    rank, world, local = _dist_env()
    device = torch.device("cuda", local)
    torch.cuda.set_device(device)
    if world > 1:
        _init_dist(device)
    checkpoint = torch.load(args.checkpoint, map_location="cpu", weights_only=True)
    teacher_params = checkpoint["hyperparams"]
    with open(args.config) as f:
        params = yaml.safe_load(f)
    for key, value in params.items():
        if key not in teacher_params:
            logger.warning("parameter %s in the config is not in the checkpoint's hyperparameters", key)
        elif value != teacher_params[key]:
            logger.warning("parameter %s differs from the teacher checkpoint: %r != %r", key, teacher_params[key], value)
    params["distilled_decoder"] = True  # flags the student (distill.py:62)
    freeze_bn = validate_freeze_bn(args.freeze_bn if args.freeze_bn is not None else checkpoint.get("freeze_bn"), params)

    teacher = build_model(params).to(device)
    teacher.load_state_dict(ema_model_state(checkpoint, "--ema-teacher", args.checkpoint) if args.ema_teacher else checkpoint["model_state_dict"])
    # distill.py:127-131 never calls teacher_model.eval(): the reference's teacher rollout (and its context encoders) run
    # with dropout 0.1 live.  --teacher-dropout reproduces that (a Python loop over the training kernels); the default
    # is the clean teacher on the native sampler.
    apply_freeze_bn(teacher, freeze_bn)   # (with --teacher-dropout the teacher's backbone is in train mode: its statistics stay as trained)
    teacher.train(args.teacher_dropout)
    teacher.set_dropout(args.dropout if args.teacher_dropout else 0.0, seed=args.seed + 104729 + 7919 * rank)
    student = build_model(params).to(device)
    student.load_state_dict(checkpoint["model_state_dict"])
    apply_freeze_bn(student, freeze_bn)
    student.train()
    student.set_dropout(args.dropout, seed=args.seed + 7919 * rank)
    # the student's context encoders never see a gradient (the context comes from the teacher under
    # no_grad), so torch's AdamW leaves them untouched; the flat optimizer therefore only owns the rest
    trainable = [p for n, p in student.named_parameters() if n.startswith(("diffusion_action_generator.", "step_encoding."))]
    optimizer = training.FusedAdamW(trainable, lr=params["lr"], ema_decay=args.ema_decay, ema_warmup=not args.no_ema_warmup,
                                    max_grad_norm=args.clip_grad_norm)
    if world > 1:
        training.broadcast_parameters(optimizer, student)

    gen = torch.Generator().manual_seed(args.seed + rank)
    source = data_source(args, params, device)
    n_total = source.n
    bs = params["batch_size"]
    val = _holdout(args, n_total, distilled=True)
    if val is None:
        shard, steps_per_epoch = shard_plan(n_total, bs, rank, world)
    else:
        shard, steps_per_epoch = shard_plan(len(val.train_idx), bs, rank, world)
        shard = val.train_idx[shard]
    lr_scheduler = torch.optim.lr_scheduler.OneCycleLR(optimizer, max_lr=params["lr"], total_steps=params["epochs"] * steps_per_epoch)
    dev_gen = torch.Generator(device=device).manual_seed(args.seed + 1000 * rank)
    n_teacher = params["distill_teacher_inference_steps"]
    for epoch in range(params["epochs"]):
        order = shard[torch.randperm(len(shard), generator=gen)]
        mean_loss = 0.0
        for i in range(steps_per_epoch):
            idx = order[i * bs : (i + 1) * bs]
            batch = source.batch(idx)
            noisy = torch.randn(batch["joint_command"].shape, device=device, generator=dev_gen)
            optimizer.zero_grad()
            with torch.no_grad():
                if params_need_context(params):
                    embedded = teacher.encode_input_data({k: batch[k].contiguous() for k in CONTEXT_KEYS if k in batch})
                else:
                    embedded = [torch.randn(len(idx), 10, params["hidden_dim"], device=device, generator=dev_gen)]
                target = teacher.sample(embedded, noisy, n_teacher, with_dropout=args.teacher_dropout)
            pred = student.forward_with_context(embedded, noisy, torch.zeros(len(idx), device=device))
            loss = training.mse_loss(pred, target)
            loss.backward()
            training.allreduce_gradients(optimizer, world)
            optimizer.step()
            lr_scheduler.step()
            mean_loss += float(loss)
            if i % 20 == 0 and rank == 0:
                print(f"Epoch {epoch}, it {i}, Loss: {mean_loss / (i + 1):.05f}, LR: {lr_scheduler.get_last_lr()[0]:0.7f}{_grad_clip_suffix(optimizer)}",
                      flush=True)
        if val is not None and rank == 0:
            val.run(student, optimizer, source, epoch, params["epochs"])
        training.assert_replicas_equal(optimizer)
        if rank == 0:
            torch.save({"model_state_dict": student.state_dict(), "optimizer_state_dict": optimizer.state_dict(),
                        "lr_scheduler_state_dict": lr_scheduler.state_dict(), "hyperparams": params,
                        "current_epoch": epoch, **_ema_checkpoint_keys(optimizer, student), **_grad_clip_checkpoint_keys(optimizer),
                        **_freeze_bn_checkpoint_keys(freeze_bn),
                        **({} if val is None else {"validation": val.entry()})},
                       args.output)
    if world > 1:
        import torch.distributed as dist

        dist.barrier()
        dist.destroy_process_group()
    return 0


class _Holdout:
    """The held-out windows of a `train` / `distill --val-fraction` run and the reports on them (the checkpoint's `validation` entry)."""

    def __init__(self, args, n_total: int, distilled: bool):
        from .evaluation import holdout_split

        self.fraction, self.split, self.seed = args.val_fraction, args.val_split, args.seed
        self.every, self.draws, self.steps, self.distilled = args.val_every, args.val_draws, args.val_steps, distilled
        self.train_idx, self.val_idx = holdout_split(n_total, self.fraction, self.seed, self.split)
        self.history: list = []

    def run(self, model, optimizer, source, epoch: int, epochs: int) -> None:
        """Every `--val-every` epochs and after the last one: the last iterate and, where the optimizer keeps one, the average.  The model
        returns to the mode it was in; nothing it trains with (parameters, moments, dropout seeds, generators) is written."""
        from .evaluation import evaluate

        if (epoch + 1) % self.every and epoch + 1 != epochs:
            return
        was_training = model.training
        model.eval()
        try:
            kw = dict(steps=self.steps, draws=self.draws, seed=self.seed, distilled=self.distilled)
            entry = {"epoch": epoch, "last": evaluate(model, source, self.val_idx, **kw)}
            if optimizer.flat_ema is not None:
                with optimizer.ema_weights():
                    entry["ema"] = evaluate(model, source, self.val_idx, **kw)
        finally:
            model.train(was_training)
        self.history.append(entry)
        line = ", ".join(f"{name}: " + " ".join(f"{k} {r[k]:.5f}" for k in ("val_loss", "rmse_first_draw", "rmse_medoid") if r[k] is not None)
                         for name, r in entry.items() if name != "epoch")
        print(f"Epoch {epoch}, validation on {len(self.val_idx)} windows - {line}", flush=True)

    def entry(self) -> dict:
        return {"fraction": self.fraction, "split": self.split, "seed": self.seed, "n_val": len(self.val_idx), "history": self.history}


def _holdout(args, n_total: int, distilled: bool = False) -> Optional[_Holdout]:
    return None if args.val_fraction is None else _Holdout(args, n_total, distilled)


def _timesteps(text: str) -> list:
    try:
        return [int(v) for v in text.split(",")]
    except ValueError:
        raise SystemExit(f"--timesteps takes integers a,b,..., got {text!r}") from None


def validate_evaluation_args(args) -> None:
    """The arguments of `evaluate` and of the --val-* flags, checked before anything touches the GPU."""
    from . import evaluation

    try:
        if getattr(args, "val_fraction", None) is not None:
            evaluation.check_fraction(args.val_fraction)
        for name in ("val_draws", "draws") if args.command == "evaluate" else ("val_draws",):   # (sample / rollout --draws: checked by the parser)
            if getattr(args, name, None) is not None:
                evaluation.check_draws(getattr(args, name))
        for name in ("val_every", "val_steps", "steps"):
            if getattr(args, name, None) is not None and getattr(args, name) < 1:
                raise ValueError(f"--{name.replace('_', '-')} must be positive, got {getattr(args, name)}")
        if getattr(args, "timesteps", None) is not None:
            evaluation.check_timesteps(_timesteps(args.timesteps))
        if args.command == "evaluate":
            evaluation.default_timesteps(args.grid)
            if args.all and args.val_fraction is not None:
                raise ValueError("--all evaluates every window: not with --val-fraction")
    except ValueError as e:
        raise SystemExit(str(e)) from None


def cmd_evaluate(args) -> int:
    """The report of evaluation.evaluate on the held-out windows of a data source, as one JSON line.  A checkpoint written by
    `train --val-fraction` carries the fraction, split and seed of its split: they are the defaults, so the same windows are used."""
    import json

    from .evaluation import evaluate, holdout_split

    device = torch.device("cuda", _dist_env()[2])
    torch.cuda.set_device(device)
    checkpoint = torch.load(args.checkpoint, map_location="cpu", weights_only=True)
    params = checkpoint["hyperparams"]
    recorded = checkpoint.get("validation", {})
    if args.seed is None:
        args.seed = recorded.get("seed", 0)
    fraction = args.val_fraction if args.val_fraction is not None else recorded.get("fraction")
    split = args.val_split or recorded.get("split", "tail")
    if not args.all and fraction is None:
        raise SystemExit("evaluate: give --val-fraction F, or --all for every window (the checkpoint records no split)")
    _distilled_arg(args, params)
    limits = _limits_arg(args, params)   # in the space of the target trajectories (x * std + mean), as sample --hold
    slew = _slew_arg(args, params)       # radians per row in the same space
    accel = _accel_arg(args, params)     # radians per row^2 in the same space
    model = build_model(params).to(device)
    model.load_state_dict(ema_model_state(checkpoint, "--ema", args.checkpoint) if args.ema else checkpoint["model_state_dict"])
    model.eval()
    source = data_source(args, params, device)
    idx = torch.arange(source.n) if args.all else holdout_split(source.n, fraction, args.seed, split)[1]
    report = evaluate(model, source, idx, steps=args.steps, draws=args.draws, grid=args.grid, seed=args.seed,
                      max_mode=3 if args.max_mode is None else args.max_mode, timesteps=_timesteps(args.timesteps) if args.timesteps else None,
                      distilled=bool(params.get("distilled_decoder", False)), solver=args.solver, limits=limits,
                      reproject=args.reproject, slew=slew, accel=accel)
    line = json.dumps(report)
    print(line)
    if args.output:
        with open(args.output, "w") as f:
            f.write(line + "\n")
    return 0


def cmd_sample(args) -> int:
    from . import ops

    rank, world, local = _dist_env()
    device = torch.device("cuda", local)
    torch.cuda.set_device(device)
    checkpoint = torch.load(args.checkpoint, map_location="cpu", weights_only=True)
    params = checkpoint["hyperparams"]
    model = build_model(params).to(device)
    model.load_state_dict(ema_model_state(checkpoint, "--ema", args.checkpoint) if args.ema else checkpoint["model_state_dict"])
    model.eval()
    n = args.num_samples
    mine = torch.arange(rank, n, world)  # embarrassingly parallel over ranks, no collective
    source = data_source(args, params, device) if (args.data or getattr(args, "db", None) or params_need_context(params)) else None
    gen = torch.Generator(device=device).manual_seed(args.seed + rank)
    B = len(mine)
    if B == 0:
        return 0
    G = args.draws
    x_T = torch.randn(B * G, params["trajectory_prediction_length"], params["num_joints"], device=device, generator=gen)
    _distilled_arg(args, params)
    hold = None
    if args.hold:   # the joints held at every row of every trajectory, in the space of the file's trajectories (x * std + mean)
        joints, values = _hold_joints(args.hold, params["num_joints"])
        known, mask = torch.zeros_like(x_T), torch.zeros(params["num_joints"], dtype=torch.bool, device=device)
        mean, std = model.mean.reshape(-1), model.std.reshape(-1)
        known[:, :, joints] = (torch.tensor(values, device=device) - mean[joints]) / std[joints]
        mask[joints] = True
        hold = (known, mask)
    limits = _limits_arg(args, params)   # in the space of the file's trajectories (x * std + mean), as --hold
    if limits is not None:
        from .evaluation import normalised_limits

        limits = normalised_limits(limits, model.mean, model.std)
    slew = _slew_arg(args, params)       # radians per row in the same space
    if slew is not None:
        from .evaluation import normalised_slew

        slew = normalised_slew(slew, model.mean, model.std, _limits_arg(args, params))
    accel = _accel_arg(args, params)     # radians per row^2 in the same space
    if accel is not None:
        from .evaluation import normalised_accel

        accel = normalised_accel(accel, model.mean, model.std, _limits_arg(args, params))
    with torch.no_grad():
        if params_need_context(params):
            batch = source.batch(mine % source.n)
            inp = {k: batch[k].contiguous() for k in CONTEXT_KEYS if k in batch}
            context = model.encode_input_data(inp)
        else:
            context = [torch.randn(B, 10, params["hidden_dim"], device=device, generator=gen)]
        distilled = params.get("distilled_decoder", False)
        if distilled and G == 1 and hold is None and limits is None and slew is None and accel is None:  # single forward at t = 0 (plot.py:118-121)
            traj = model.forward_with_context(context, x_T, torch.zeros(B, device=device))
        elif distilled:   # the same forward on G start noises per context; its output is x0: hold, slew and limits project it in the launch
            traj = model.sample_direct(context, x_T, hold=hold, limits=limits, slew=slew, draws=G, accel=accel)
        else:
            traj = model.sample(context, x_T, args.steps, draws=G, hold=hold, solver=args.solver, limits=limits, reproject=args.reproject, slew=slew,
                                accel=accel)   # G draws for each of the B contexts, which are encoded once
        if G > 1:
            medoid = ops.select_medoid(traj.contiguous(), G, gather=False)[0]
        traj = ops.normalize(traj.contiguous(), model.mean, model.std, inverse=True)
    out = args.output if world == 1 else f"{args.output}.rank{rank}"
    saved = {"trajectories": traj.cpu(), "noise": x_T.cpu(), "steps": args.steps, "indices": mine}
    if args.solver != "ddim":
        saved["solver"] = args.solver
    if hold is not None:
        saved["hold"] = dict(args.hold)   # {joint: the value it was held at}
    if limits is not None:
        saved["limits"] = _limits_saved(args)   # {joint: (lo, hi)} or the one range of --clip, as given
    if slew is not None:
        saved["slew"] = args.slew   # one number, or {joint: v}, as given
    if accel is not None:
        saved["accel"] = args.accel   # one number, or {joint: a}, as given
    if G > 1:   # (n, G, T, J): the draws of a context side by side; medoid (n,): the representative draw of each (ops.select_medoid)
        saved.update(trajectories=saved["trajectories"].view(B, G, *traj.shape[1:]), draws=G, medoid=medoid.cpu())
    torch.save(saved, out)
    if rank == 0:
        print(f"sampled {n}{f' x {G}' if G > 1 else ''} trajectories of shape {tuple(traj.shape[1:])} with {args.steps} DDIM steps -> {args.output}")
    return 0


def synthetic_sensor_stream(n: int, params: dict, ticks: int, seed: int = 0) -> dict:
    """A sensor stream for ``ticks`` control ticks of n robots, shaped like what ros.py's timers deliver (ros.py:155-163): per tick
    ``trajectory_prediction_length`` joint-state and rotation samples (the resample rate) and two frames (10 Hz against the 0.2 s tick).
    Sine-wave joints as raw angles around 0 (the node wraps them itself), unit quaternions, noise frames."""
    g = torch.Generator().manual_seed(seed)
    J, T = params["num_joints"], params["trajectory_prediction_length"]
    total = ticks * T
    phase = torch.rand(n, 1, J, generator=g) * 2 * math.pi
    freq = 0.5 + torch.rand(n, 1, J, generator=g)
    wave = torch.sin(2 * math.pi * freq * torch.arange(total).view(1, total, 1) / 50.0 + phase)
    quat = torch.randn(n, total, 4, generator=g)
    quat = quat / quat.norm(dim=-1, keepdim=True)
    rot = quat if params["imu_orientation_embedding_method"] != "five_dim" else torch.cat([quat[..., :3], torch.sin(quat[..., 3:]), torch.cos(quat[..., 3:])], -1)
    out = {"joint_state": wave.contiguous(), "rotation": rot.contiguous()}
    if params.get("use_images"):
        R = params.get("image_resolution", 480)
        out["image_data"] = torch.rand(n, 2 * ticks, 3, R, R, generator=g)
    return out


def raw_sensor_stream(n: int, params: dict, ticks: int, camera: tuple = (480, 640), seed: int = 0) -> dict:
    """``synthetic_sensor_stream`` as the sensors deliver it, before the node's preprocessing (ros.py:186-253): the same joint states,
    ``orientation`` as unit xyzw quaternions (n, total, 4) and ``camera`` as uint8 rgb frames (n, 2 ticks, H, W, 3) of the camera's size."""
    g = torch.Generator().manual_seed(seed)
    J, T = params["num_joints"], params["trajectory_prediction_length"]
    total = ticks * T
    phase = torch.rand(n, 1, J, generator=g) * 2 * math.pi
    freq = 0.5 + torch.rand(n, 1, J, generator=g)
    wave = torch.sin(2 * math.pi * freq * torch.arange(total).view(1, total, 1) / 50.0 + phase)
    quat = torch.randn(n, total, 4, generator=g)
    quat = quat / quat.norm(dim=-1, keepdim=True)
    out = {"joint_state": wave.contiguous(), "orientation": quat.contiguous()}
    if params.get("use_images"):
        out["camera"] = torch.randint(0, 256, (n, 2 * ticks, camera[0], camera[1], 3), dtype=torch.uint8, generator=g)
    return out


def _camera_size(text: str) -> tuple:
    from . import ops

    try:
        h, w = (int(v) for v in text.lower().split("x"))
    except ValueError:
        h = w = 0
    if not (1 <= h <= ops.CAMERA_MAX and 1 <= w <= ops.CAMERA_MAX):
        raise SystemExit(f"--camera takes HxW with 1 <= H, W <= {ops.CAMERA_MAX}, got {text!r}")
    return h, w


def plan_change_rms(published: torch.Tensor, shift: int, resets: Optional[torch.Tensor] = None) -> float:
    """How far successive ticks' plans disagree about the instants both describe: the root mean square, in radians, over ticks k >= 1,
    robots, joints and the T - shift overlapping rows of ``published[k][:, :T - shift] - published[k - 1][:, shift:]`` (``published``
    (K, N, T, J) as ``cli rollout`` saves it; ``shift``: the rows between two ticks).  ``resets`` (K, N) bool: a robot reset after tick
    k - 1 starts a new episode at tick k and that pair is left out.  NaN where nothing overlaps (K < 2, shift >= T, every pair reset).
    This is the number that says whether a selector dithers between modes."""
    K, N, T, _ = published.shape
    if K < 2 or not 0 <= shift < T:
        return float("nan")
    diff = (published[1:, :, :T - shift] - published[:-1, :, shift:]).double()
    if resets is not None:
        diff = diff[~resets[:-1].bool()]
    return float(diff.pow(2).mean().sqrt()) if diff.numel() else float("nan")


def _distilled_arg(args, params: dict) -> None:
    """What a distilled checkpoint still refuses, as argument errors: --solver multistep (one step has no history), --carry (it cannot
    adapt its free rows to pinned ones) and --reproject (it predicts x0: there is no eps to recompute).  --limits, --clip, --slew,
    --hold, --draws and --select are accepted: its output is the x0 they are defined on (model.sample_direct)."""
    if not params.get("distilled_decoder", False):
        return
    if getattr(args, "solver", "ddim") != "ddim":
        raise SystemExit("--solver: a distilled decoder is one forward at t = 0 - there is no rollout for a multistep solver")
    if getattr(args, "carry", 0):
        raise SystemExit("--carry: a distilled decoder is one forward at t = 0 - its free rows cannot adapt to pinned ones "
                         "(--select coherent and --slew give it continuity)")
    if getattr(args, "reproject", False):
        raise SystemExit("--reproject: a distilled decoder predicts x0 itself - there is no eps to recompute from the clamped x0")


def _select_arg(args, T: int) -> None:
    """--select / --coherence-decay / --contrast against the checkpoint's horizon: PolicySession.check_select's errors as argument errors."""
    from .session import PolicySession

    try:
        carry, advance = PolicySession.check_carry(T, args.carry, args.advance)
        PolicySession.check_select(args.select, T, advance, args.draws, args.coherence_decay, args.contrast)
    except ValueError as e:
        raise SystemExit(f"rollout: {e}") from None


def cmd_rollout(args) -> int:
    """The closed control loop (ros.py:165-335) on a synthetic sensor stream: K ticks of a PolicySession over N robots in lockstep.
    --episode-ticks: robot b's episodes last E[b % len(E)] ticks; after the last tick of one, that robot alone starts again.
    --carry K [--advance S]: overlapping ticks - S trajectory points (default T - K) pass between two ticks, the sensor rows of S points
    arrive per tick, and the first K rows of a tick's trajectory are pinned to rows [S, S + K) of the previous one.
    --hold J=V[,J=V...]: joint J of every robot is held at V radians (as published) inside every tick's rollout, from the first tick on.
    --limits J=LO:HI[,J=LO:HI...] | --clip R [--reproject]: every published joint J stays inside [LO, HI] radians (as published), or every
    joint inside [-R, R]: the limits act on the predicted clean trajectory inside every tick's rollout (PolicySession(limits=...)).
    --slew V | J=V[,J=V...]: consecutive published rows differ by at most V radians (every joint, or joint J), also across two ticks
    (PolicySession(slew=...): V = max velocity / row rate).
    --accel A | J=A[,J=A...]: the second difference of three consecutive published rows is at most A radians (every joint, or joint J), also
    across two ticks, wherever neither the box nor the slew limit wins (PolicySession(accel=...): A = max acceleration / row rate^2); it
    needs --limits or --clip finite on both sides for every such joint.
    --select medoid|coherent [--coherence-decay R] [--contrast L]: which of the --draws G draws a tick commits; "coherent" (overlapping ticks
    only) is the draw closest to the previous tick's plan over the rows both describe (PolicySession(select="coherent")).  Whenever ticks
    overlap the line and the file gain ``select`` and ``plan_change_rms`` (``plan_change_rms``), for either selector."""
    from .session import PolicySession

    if args.synthetic is None or args.synthetic < 1 or args.ticks < 1:
        raise SystemExit("rollout needs --synthetic N (robots, N >= 1) and --ticks K (K >= 1)")
    if args.camera is not None and not args.raw:
        raise SystemExit("--camera is the frame size of the --raw stream")
    if args.advance is not None and not args.carry and args.advance < 1:
        raise SystemExit("--advance takes a positive number of trajectory points")
    camera = _camera_size(args.camera or "480x640")
    episode = None
    if args.episode_ticks is not None:
        try:
            lengths = [int(v) for v in args.episode_ticks.split(",")]
        except ValueError:
            lengths = []
        if not lengths or min(lengths) < 1:
            raise SystemExit("--episode-ticks takes positive tick counts E[,E...]")
        episode = torch.tensor([lengths[b % len(lengths)] for b in range(args.synthetic)])
    if (args.select, args.coherence_decay, args.contrast) != ("medoid", 0.5, 0.0):   # say so before anything touches the GPU
        _select_arg(args, torch.load(args.checkpoint, map_location="cpu", weights_only=True)["hyperparams"]["trajectory_prediction_length"])
    if args.carry or args.solver != "ddim" or args.reproject:   # (likewise)
        _distilled_arg(args, torch.load(args.checkpoint, map_location="cpu", weights_only=True)["hyperparams"])
    device = torch.device("cuda", _dist_env()[2])
    torch.cuda.set_device(device)
    session = PolicySession.from_checkpoint(args.checkpoint, device, ema=args.ema, num_inference_steps=args.steps, batch=args.synthetic,
                                            seed=args.seed, carry=args.carry, advance=args.advance, draws=args.draws, holds=bool(args.hold), solver=args.solver,
                                            limits=_limits_arg(args), reproject=args.reproject, slew=_slew_arg(args), select=args.select,
                                            coherence_decay=args.coherence_decay, contrast=args.contrast, direct=None, accel=_accel_arg(args))
    params = session.hyperparams
    if args.hold:
        session.hold(*_hold_joints(args.hold, params["num_joints"]))
    if args.raw:
        stream = raw_sensor_stream(args.synthetic, params, args.ticks, camera, seed=args.seed)
    else:
        stream = synthetic_sensor_stream(args.synthetic, params, args.ticks, seed=args.seed)
    stream = {k: v.to(device) for k, v in stream.items()}
    T = session.advance   # trajectory points - sensor rows - between two ticks: the whole horizon without --carry / --advance
    published, resets = [], []
    for k in range(args.ticks):
        if params["use_joint_states"]:
            session.push_joint_state(stream["joint_state"][:, k * T:(k + 1) * T])
        if params["use_imu"] and args.raw:
            session.push_orientation(stream["orientation"][:, k * T:(k + 1) * T])
        elif params["use_imu"]:
            session.push_rotation(stream["rotation"][:, k * T:(k + 1) * T])
        if params.get("use_images") and args.raw:
            session.push_camera(stream["camera"][:, 2 * k:2 * k + 2])
        elif params.get("use_images"):
            session.push_image(stream["image_data"][:, 2 * k:2 * k + 2])
        published.append(session.step())
        if episode is not None:
            resets.append((k + 1) % episode == 0)
            if resets[-1].any():
                session.reset(robots=resets[-1])
    traj = torch.stack(published).cpu()   # (K, N, T, J)
    saved = {"trajectories": traj, "ticks": args.ticks, "steps": args.steps, "seed": args.seed}
    if args.carry or args.advance is not None:
        saved.update(carry=session.carry, advance=session.advance)
    if args.hold:
        saved["hold"] = dict(args.hold)   # {joint: the radians it was held at}
    if session._limits_rad is not None:
        saved["limits"] = _limits_saved(args)   # {joint: (lo, hi)} radians, or the one range of --clip
    if args.slew is not None:
        saved["slew"] = args.slew   # radians per row: one number, or {joint: v}
    if args.accel is not None:
        saved["accel"] = args.accel   # radians per row^2: one number, or {joint: a}
    if args.draws > 1:
        saved["draws"] = session.draws   # every published trajectory is the selected one of that many draws
    if episode is not None:
        saved["resets"] = torch.stack(resets)   # (K, N): robot n was reset after tick k
    overlap = ""
    if session.advance < session.T:   # overlapping ticks: how far successive plans disagree about the instants both describe
        saved.update(select=session.select, plan_change_rms=plan_change_rms(traj, session.advance, saved.get("resets")))
        overlap = f", select {session.select}, plan_change_rms {saved['plan_change_rms']:.5f} rad"
    torch.save(saved, args.output)
    print(f"rolled out {args.ticks} ticks of {args.synthetic} robots, trajectories of shape {tuple(traj.shape[2:])}{overlap} -> {args.output}")
    return 0


def params_need_context(params: dict) -> bool:
    return any(params.get(k, False) for k in ("use_action_history", "use_imu", "use_joint_states", "use_images", "use_gamestate"))


def _draws(text: str) -> int:
    try:
        g = int(text)
    except ValueError:
        g = 0
    if not 1 <= g <= 64:
        raise argparse.ArgumentTypeError(f"--draws takes a number of draws per context in [1, 64], got {text!r}")
    return g


def _noise_draws(text: str) -> int:
    try:
        k = int(text)
    except ValueError:
        k = 0
    if not 1 <= k <= 64:
        raise argparse.ArgumentTypeError(f"--noise-draws takes a number of (timestep, noise) pairs per window in [1, 64], got {text!r}")
    return k


def noise_draws_of(arg: Optional[int], checkpoint: Optional[dict]) -> int:
    """--noise-draws, else what the resumed checkpoint trained with (``noise_draws``), else 1."""
    if arg is not None:
        return arg
    return int(checkpoint.get("noise_draws", 1)) if checkpoint is not None else 1


def _hold(text: str) -> list:
    """--hold J=V[,J=V...] -> [(joint, value)]; the joints are checked against the model's joint count where it is known."""
    try:
        pairs = [(int(j), float(v)) for j, v in (item.split("=") for item in text.split(","))]
    except ValueError:
        pairs = []
    if not pairs or min(j for j, _ in pairs) < 0 or len({j for j, _ in pairs}) != len(pairs):
        raise argparse.ArgumentTypeError(f"--hold takes JOINT=RADIANS[,JOINT=RADIANS...] with distinct joint indices >= 0, got {text!r}")
    return pairs


def _limits(text: str) -> list:
    """--limits J=LO:HI[,J=LO:HI...] -> [(joint, lo, hi)]; an empty LO or HI (or -inf / inf) leaves that side open."""
    try:
        out = []
        for item in text.split(","):
            j, pair = item.split("=")
            lo, hi = pair.split(":")
            out.append((int(j), float(lo) if lo.strip() else -math.inf, float(hi) if hi.strip() else math.inf))
    except ValueError:
        out = []
    if not out or min(j for j, _, _ in out) < 0 or len({j for j, _, _ in out}) != len(out) or any(not lo <= hi for _, lo, hi in out):
        raise argparse.ArgumentTypeError(f"--limits takes JOINT=LO:HI[,JOINT=LO:HI...] with distinct joint indices >= 0 and LO <= HI, got {text!r}")
    return out


def _limits_arg(args, params: Optional[dict] = None):
    """``limits`` of model.sample / evaluate / PolicySession from --limits / --clip: {joint: (lo, hi)}, one range, or None."""
    if args.limits and args.clip is not None:
        raise SystemExit("--limits and --clip exclude each other")
    if args.reproject and not args.limits and args.clip is None:
        raise SystemExit("--reproject is an option of --limits / --clip")
    if args.clip is not None:
        if not args.clip >= 0:
            raise SystemExit("--clip takes a range R >= 0")
        limits = float(args.clip)
    elif args.limits:
        limits = {j: (lo, hi) for j, lo, hi in args.limits}
    else:
        return None
    if params is not None:
        J = params["num_joints"]
        if args.reproject and params.get("distilled_decoder", False):
            raise SystemExit("--reproject: a distilled decoder predicts x0 itself - there is no eps to recompute from the clamped x0")
        if J > 32 or (isinstance(limits, dict) and max(limits) >= J):
            raise SystemExit(f"--limits: joint indices lie in [0, {J}) and the model has at most 32 joints")
    return limits


def _slew(text: str):
    """--slew V | J=V[,J=V...] -> one float, or {joint: v}; radians per row, v >= 0."""
    try:
        out = float(text) if "=" not in text else {int(j): float(v) for j, v in (item.split("=") for item in text.split(","))}
        ok = out >= 0 if isinstance(out, float) else (len(out) == text.count(",") + 1 and all(j >= 0 and v >= 0 for j, v in out.items()))
    except ValueError:
        ok = False
    if not ok:
        raise argparse.ArgumentTypeError(f"--slew takes V or JOINT=V[,JOINT=V...] with distinct joint indices >= 0 and V >= 0, got {text!r}")
    return out


def _slew_arg(args, params: Optional[dict] = None):
    """``slew`` of model.sample / evaluate / PolicySession from --slew: one number, {joint: v}, or None."""
    if args.slew is None:
        return None
    if params is not None:
        J = params["num_joints"]
        if J > 32 or (isinstance(args.slew, dict) and max(args.slew) >= J):
            raise SystemExit(f"--slew: joint indices lie in [0, {J}) and the model has at most 32 joints")
    return args.slew


def _accel(text: str):
    """--accel A | J=A[,J=A...] -> one float, or {joint: a}; radians per row^2, a >= 0."""
    try:
        out = float(text) if "=" not in text else {int(j): float(v) for j, v in (item.split("=") for item in text.split(","))}
        ok = out >= 0 if isinstance(out, float) else (len(out) == text.count(",") + 1 and all(j >= 0 and v >= 0 for j, v in out.items()))
    except ValueError:
        ok = False
    if not ok:
        raise argparse.ArgumentTypeError(f"--accel takes A or JOINT=A[,JOINT=A...] with distinct joint indices >= 0 and A >= 0, got {text!r}")
    return out


def _accel_arg(args, params: Optional[dict] = None):
    """``accel`` of model.sample / evaluate / PolicySession from --accel: one number, {joint: a}, or None."""
    if args.accel is None:
        return None
    if params is not None:
        J = params["num_joints"]
        if J > 32 or (isinstance(args.accel, dict) and max(args.accel) >= J):
            raise SystemExit(f"--accel: joint indices lie in [0, {J}) and the model has at most 32 joints")
    return args.accel


def _limits_saved(args):
    return float(args.clip) if args.clip is not None else {j: (lo, hi) for j, lo, hi in args.limits}


def _hold_joints(pairs: list, J: int) -> tuple:
    if J > 32 or max(j for j, _ in pairs) >= J:
        raise SystemExit(f"--hold: joint indices lie in [0, {J}) and the model has at most 32 joints")
    return [j for j, _ in pairs], [v for _, v in pairs]


def _add_limit_flags(p) -> None:
    p.add_argument("--limits", type=_limits, default=None, metavar="J=LO:HI[,J=LO:HI...]", help="joint J stays inside [LO, HI] (an empty side is open): "
                   "the predicted clean trajectory is clamped at every denoising step (model.sample(limits=...)); units as --hold's in this "
                   "subcommand (rollout: radians as published; sample / evaluate: the space of the trajectories)")
    p.add_argument("--clip", type=float, default=None, metavar="R", help="--limits with the one range [-R, R] on every joint")
    p.add_argument("--slew", type=_slew, default=None, metavar="V | J=V[,J=V...]", help="consecutive rows of a trajectory differ by at most V "
                   "(every joint, or joint J): the predicted clean trajectory is slew-limited at every denoising step "
                   "(model.sample(slew=...)); radians per row, units as --limits' in this subcommand")
    p.add_argument("--accel", type=_accel, default=None, metavar="A | J=A[,J=A...]", help="the second difference of three consecutive rows of a "
                   "trajectory is at most A (every joint, or joint J): the predicted clean trajectory is acceleration-limited at every denoising "
                   "step, ahead of --slew and --limits, which win (model.sample(accel=...)); radians per row^2, units as --limits' in this "
                   "subcommand; rollout needs --limits / --clip finite on both sides for every such joint")
    p.add_argument("--reproject", action="store_true", help="with --limits / --clip: a clamped element's noise prediction is recomputed from the "
                   "clamped value (diffusers' use_clipped_model_output)")


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="cli", description="SoccerDiffusion denoiser on MI355X: train / sample")
    sub = ap.add_subparsers(dest="command", required=True)
    tr = sub.add_parser("train", help="train the model (flags of the reference's train.py)")
    tr.add_argument("--config", "-c", type=str, default=None, help="Path to the configuration file")
    tr.add_argument("--checkpoint", "-p", type=str, default=None, help="Path to the checkpoint to load")
    tr.add_argument("--output", "-o", type=str, default="trajectory_transformer_model.pth", help="Path to save the model")
    tr.add_argument("--decoder-pretraining", action="store_true", help="Train the decoder only, on random context")
    tr.add_argument("--pretrained-decoder", type=str, default=None, help="Checkpoint whose decoder weights are loaded (strict=False)")
    tr.add_argument("--dropout", type=float, default=0.1, help="dropout probability of the transformer layers in training "
                    "(the reference never sets it: torch's default 0.1, decoder.py:26-33); 0 = the parity path")
    tr.add_argument("--noise-draws", type=_noise_draws, default=None, metavar="K", help="K (timestep, noise) pairs per window on ONE encoded "
                    "observation (train_step(draws=K)): K x the denoising supervision per encoder pass; steps per epoch and the learning-rate "
                    "schedule still count windows; the checkpoint gains noise_draws and a resumed run (-p) continues with it")
    sa = sub.add_parser("sample", help="sample trajectories from a checkpoint (flags of the reference's plot.py)")
    sa.add_argument("checkpoint", type=str, help="Path to the checkpoint to load")
    sa.add_argument("--steps", type=int, default=30, help="Number of denoising steps")
    sa.add_argument("--solver", choices=("ddim", "multistep"), default="ddim", help="the sampler of the rollout: first-order DDIM, or the "
                    "second-order multistep solver on the same timesteps (model.sample(solver=...)): meant for fewer --steps")
    _add_limit_flags(sa)
    sa.add_argument("--num_samples", type=int, default=10, help="Number of samples to generate")
    sa.add_argument("--output", "-o", type=str, default="samples.pt", help="Where to save the sampled trajectories")
    sa.add_argument("--ema", action="store_true", help="sample from the checkpoint's EMA weights (train --ema-decay) instead of the last iterate")
    sa.add_argument("--draws", type=_draws, default=1, metavar="G", help="G draws for each of the --num_samples contexts, sampled on the shared "
                    "folded context: the file gains draws and medoid (n,), trajectories becomes (n, G, T, J)")
    sa.add_argument("--hold", type=_hold, default=None, metavar="J=V[,J=V...]", help="joint J is held at V in every row of every trajectory and "
                    "the other joints are sampled to fit (model.sample(hold=...)); V in the space of the file's trajectories")
    di = sub.add_parser("distill", help="distil the multi-step model into a single-step model (flags of the reference's distill.py)")
    di.add_argument("config", type=str, help="Path to the training configuration file")
    di.add_argument("checkpoint", type=str, help="Path to the checkpoint to load for the teacher model")
    di.add_argument("--output", "-o", type=str, default="distilled_trajectory_transformer_model.pth", help="Path to save the distilled model")
    di.add_argument("--dropout", type=float, default=0.1, help="dropout probability of the student (and of the teacher with --teacher-dropout)")
    di.add_argument("--teacher-dropout", action="store_true", help="leave the teacher in train mode during its rollout, as the "
                    "reference's distill.py does (it never calls teacher_model.eval())")
    di.add_argument("--ema-teacher", action="store_true", help="build the teacher from the checkpoint's EMA weights (train --ema-decay)")
    tr.add_argument("--pretrained-backbone", type=str, default=None, metavar="FILE", help="state dict with torchvision's ResNet keys: every tensor "
                    "whose name and shape match is loaded into the image encoder's backbone, except fc.* (what --freeze-bn is for)")
    for p in (tr, di):
        p.add_argument("--freeze-bn", choices=FREEZE_BN_MODES, default=None, help="fine-tune on frozen BatchNorm statistics: every BatchNorm2d of "
                       "the ResNet image encoder normalises with its running statistics and leaves them alone (stats); all: its weight and bias "
                       "are frozen too; the checkpoint gains freeze_bn and a resumed run continues as it did")
        p.add_argument("--ema-decay", type=_ema_decay, default=None, metavar="D", help="keep an exponential moving average of the trained "
                       "weights with decay D in (0, 1), updated inside the optimizer step; the checkpoint gains ema_model_state_dict and ema")
        p.add_argument("--clip-grad-norm", type=_clip_grad_norm, default=None, metavar="X", help="clip the global 2-norm of the gradient to X "
                       "(>= 0; inf = the guard alone) and skip a step whose gradient holds an inf or NaN, inside the optimizer step; the "
                       "checkpoint gains grad_clip")
        p.add_argument("--no-ema-warmup", action="store_true", help="weight 1 - D from the first update on, instead of "
                       "1 - min(D, (1 + t) / (10 + t)) after t updates")
    for p in (tr, di):
        p.add_argument("--val-fraction", type=float, default=None, metavar="F", help="hold this fraction of the windows out of training and of the "
                       "normaliser fit and evaluate them (evaluation.evaluate); the checkpoint gains a validation entry")
        p.add_argument("--val-split", type=str, default="tail", choices=("tail", "random"), help="which windows: the last block (default) or a seeded "
                       "random subset")
        p.add_argument("--val-every", type=int, default=1, metavar="E", help="evaluate every E epochs (and after the last one)")
        p.add_argument("--val-draws", type=int, default=1, metavar="G", help="draws per held-out window (1 .. 64)")
        p.add_argument("--val-steps", type=int, default=30, metavar="N", help="DDIM steps of the held-out samples")
    ev = sub.add_parser("evaluate", help="held-out validation loss and sampled-trajectory errors of a checkpoint, as one JSON line")
    ev.add_argument("checkpoint", type=str, help="Path to the checkpoint to load")
    ev.add_argument("--steps", type=int, default=30, help="Number of denoising steps")
    ev.add_argument("--solver", choices=("ddim", "multistep"), default="ddim", help="the sampler of the rollout: first-order DDIM, or the "
                    "second-order multistep solver on the same timesteps (model.sample(solver=...)): meant for fewer --steps")
    _add_limit_flags(ev)
    ev.add_argument("--draws", type=int, default=1, metavar="G", help="draws per window (1 .. 64): rmse of the first, the medoid and the best")
    ev.add_argument("--grid", type=int, default=8, metavar="K", help="timesteps of the loss grid, t_k = (2k + 1) 1000 // (2K)")
    ev.add_argument("--timesteps", type=str, default=None, metavar="a,b,...", help="the loss grid's timesteps (0 .. 999) instead of --grid")
    ev.add_argument("--val-fraction", type=float, default=None, metavar="F", help="evaluate the held-out fraction F of the data source "
                    "(default: the checkpoint's validation entry)")
    ev.add_argument("--val-split", type=str, default=None, choices=("tail", "random"), help="default: the checkpoint's, else tail")
    ev.add_argument("--all", action="store_true", help="evaluate every window of the data source")
    ev.add_argument("--ema", action="store_true", help="evaluate the checkpoint's EMA weights (train --ema-decay) instead of the last iterate")
    ev.add_argument("--max-mode", type=int, default=None, choices=(0, 1, 2, 3, 4), help="highest sampler mode of the sampled trajectories (default 3)")
    ev.add_argument("--output", "-o", type=str, default=None, help="also write the report to this file")
    for p in (tr, sa, di, ev):
        p.add_argument("--data", type=str, default=None, help="tensor file with joint_command (+ context keys)")
        p.add_argument("--db", type=str, default=None, help="SQLite database in the reference's schema (SOCCER_DIFFUSION_DB_PATH of the reference)")
        p.add_argument("--synthetic", type=int, default=None, metavar="N", help="train / sample on N synthetic sine-wave samples")
        p.add_argument("--image-size", type=str, default=None, metavar="HxW", help="--synthetic only: frame size when it is not the "
                       "square image_resolution of the config (BASELINE's image-conditioned case uses 480x640)")
        p.add_argument("--seed", type=int, default=None if p is ev else 0)
    ro = sub.add_parser("rollout", help="drive a closed-loop policy session (the tick of the reference's ros.py) from a synthetic sensor stream")
    ro.add_argument("checkpoint", type=str, help="Path to the checkpoint to load")
    ro.add_argument("--synthetic", type=int, default=None, metavar="N", help="number of robots stepping in lockstep on a synthetic sensor stream")
    ro.add_argument("--ticks", type=int, default=10, metavar="K", help="number of control ticks")
    ro.add_argument("--output", "-o", type=str, default="rollout.pt", help="Where to save the K published trajectories")
    ro.add_argument("--steps", type=int, default=30, help="Number of denoising steps per tick")
    ro.add_argument("--solver", choices=("ddim", "multistep"), default="ddim", help="the sampler of the rollout: first-order DDIM, or the "
                    "second-order multistep solver on the same timesteps (model.sample(solver=...)): meant for fewer --steps")
    _add_limit_flags(ro)
    ro.add_argument("--episode-ticks", type=str, default=None, metavar="E[,E...]", help="episode length in ticks, robot b's is E[b %% len(E)]: "
                    "after its last tick that robot alone is reset and goes on; the output gains 'resets' (K, N)")
    ro.add_argument("--raw", action="store_true", help="the stream carries what the sensors deliver - xyzw quaternions and uint8 camera frames - "
                    "and the session preprocesses it on the device (push_orientation, push_camera)")
    ro.add_argument("--camera", type=str, default=None, metavar="HxW", help="--raw only: the camera's frame size (default 480x640)")
    ro.add_argument("--ema", action="store_true", help="run the session on the checkpoint's EMA weights (train --ema-decay)")
    ro.add_argument("--carry", type=int, default=0, metavar="K", help="overlapping ticks: the first K rows of every tick's trajectory are pinned to "
                    "the rows of the previous one that fall in the overlap (PolicySession(carry=K))")
    ro.add_argument("--advance", type=int, default=None, metavar="S", help="trajectory points between two ticks (default: horizon - K); a tick "
                    "commits that many rows to the action history")
    ro.add_argument("--hold", type=_hold, default=None, metavar="J=V[,J=V...]", help="joint J of every robot is held at V radians (as published) "
                    "inside every tick's rollout (PolicySession(holds=True).hold)")
    ro.add_argument("--draws", type=_draws, default=1, metavar="G", help="G draws per robot and tick from the once-encoded context; their medoid is "
                    "committed and published (PolicySession(draws=G))")
    ro.add_argument("--select", choices=("medoid", "coherent"), default="medoid", help="which of the G draws a tick commits: their medoid, or - "
                    "overlapping ticks only - the draw that continues the previous plan (PolicySession(select='coherent'))")
    ro.add_argument("--coherence-decay", type=float, default=0.5, metavar="R", help="--select coherent: overlap row tau weighs R ** tau, R in (0, 1] "
                    "(0.5 is the Bidirectional Decoding paper's value, not measured on this policy)")
    ro.add_argument("--contrast", type=float, default=0.0, metavar="L", help="--select coherent: weight >= 0, per element, of the medoid score "
                    "beside the coherence (0: coherence alone)")
    ro.add_argument("--seed", type=int, default=0)
    return ap


def main(argv: Optional[list] = None) -> int:
    logging.basicConfig(level=os.environ.get("LOGLEVEL", "INFO"))
    args = build_parser().parse_args(argv)
    validate_evaluation_args(args)
    for flag in ("ema", "ema_teacher"):   # asked for EMA weights the checkpoint does not hold: say so before anything touches the GPU
        if getattr(args, flag, False):
            ema_model_state(torch.load(args.checkpoint, map_location="cpu", weights_only=True), "--" + flag.replace("_", "-"), args.checkpoint)
    if not torch.cuda.is_available():
        raise SystemExit("soccerdiffusion_amd needs an MI355X (no CPU fallback)")
    return {"train": cmd_train, "sample": cmd_sample, "distill": cmd_distill, "rollout": cmd_rollout, "evaluate": cmd_evaluate}[args.command](args)


if __name__ == "__main__":
    sys.exit(main())
