"""Held-out evaluation: what a checkpoint, a step count, a sampler mode or a number of draws costs or buys on windows the model has not
seen.  The reference offers a picture per sample (soccer_diffusion/ml/inference/plot.py); this is the number.

    train_idx, val_idx = holdout_split(source.n, 0.1, seed)
    report = evaluate(model.eval(), source, val_idx, steps=30, draws=8, grid=8)

Two measurements per held-out window, both on the context encoded once:
  the training loss on a grid of K timesteps (``ops.noise_loss_grid``: one denoiser evaluation of C K trajectories that share C folded
  contexts and read K distinct step tokens), and
  the error of G sampled trajectories against the recorded one, in radians and modulo 2 pi (``ops.trajectory_errors``), for the first draw,
  for the medoid of the draws - what ``PolicySession`` commits - and for the best draw, which needs the answer and is a diagnostic only.
All randomness comes from one device generator seeded from ``seed`` alone, so two checkpoints are judged on the same draws and neither the
global generator nor a session's or a training run's is touched.  The split is by window; splitting by recording is out of scope."""

from __future__ import annotations

import math
from typing import Optional, Sequence

import numpy as np
import torch

NUM_TRAIN_TIMESTEPS = 1000
SPLITS = ("tail", "random")
MAX_DRAWS = 64
CONTEXT_KEYS = ("joint_command_history", "rotation", "joint_state", "image_data", "game_state")


def holdout_split(n: int, fraction: float, seed: int, split: str = "tail"):
    """``(train_idx, val_idx)``: sorted, disjoint int64 index tensors whose union is ``range(n)``; n_val = min(n - 1, max(1, round(n f))).
    ``tail`` holds out the last n_val indices - neighbouring windows of a recording overlap in time, so a contiguous block leaks only at
    its edge; ``random`` holds out the first n_val entries of ``torch.randperm(n)`` under a generator seeded with ``seed``."""
    check_fraction(fraction)
    if split not in SPLITS:
        raise ValueError(f"split must be one of {SPLITS}, got {split!r}")
    if isinstance(n, bool) or not isinstance(n, int) or n < 2:
        raise ValueError(f"holdout_split needs at least 2 windows, got {n!r}")
    n_val = min(n - 1, max(1, int(round(n * fraction))))
    if split == "tail":
        return torch.arange(n - n_val), torch.arange(n - n_val, n)
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(int(seed)))
    return perm[n_val:].sort().values, perm[:n_val].sort().values


def check_fraction(fraction) -> float:
    if isinstance(fraction, bool) or not isinstance(fraction, (int, float)) or not 0.0 < float(fraction) < 1.0:
        raise ValueError(f"the held-out fraction must lie in the open interval (0, 1), got {fraction!r}")
    return float(fraction)


def check_draws(draws) -> int:
    if isinstance(draws, bool) or not isinstance(draws, int) or not 1 <= draws <= MAX_DRAWS:
        raise ValueError(f"draws must be an int in [1, {MAX_DRAWS}], got {draws!r}")
    return draws


def default_timesteps(K: int) -> list:
    """The midpoints of K equal parts of the training range: t_k = (2 k + 1) 1000 // (2 K)."""
    if isinstance(K, bool) or not isinstance(K, int) or not 1 <= K <= NUM_TRAIN_TIMESTEPS:
        raise ValueError(f"the loss grid takes 1 .. {NUM_TRAIN_TIMESTEPS} timesteps, got {K!r}")
    return [(2 * k + 1) * NUM_TRAIN_TIMESTEPS // (2 * K) for k in range(K)]


def check_timesteps(timesteps: Sequence[int]) -> list:
    ts = list(timesteps)
    if not ts or any(isinstance(t, bool) or not isinstance(t, int) or not 0 <= t < NUM_TRAIN_TIMESTEPS for t in ts):
        raise ValueError(f"grid timesteps must be ints in 0 .. {NUM_TRAIN_TIMESTEPS - 1}, got {ts!r}")
    return ts


def _f64(t) -> torch.Tensor:
    return torch.as_tensor(t).detach().to("cpu", torch.float64)


def normalised_limits(limits, mean: torch.Tensor, std: torch.Tensor) -> tuple:
    """``limits`` in the space of the trajectories (x * std + mean; ``(lo, hi)``, one range or ``{joint: (lo, hi)}`` as ``ops.joint_limits``
    takes them) as ``(lo, hi)`` (J,) fp32 host tensors in the sampler's normalised space, (v - mean) / std per joint; an infinite bound
    stays infinite.  The normaliser's std is positive."""
    from . import ops

    mean, std = mean.detach().reshape(-1).cpu().float(), std.detach().reshape(-1).cpu().float()
    J = mean.numel()
    lo, hi = ops._limits_host(limits, J)
    lo, hi = torch.from_numpy(lo[:J].copy()), torch.from_numpy(hi[:J].copy())
    if not (std > 0).all():
        raise ValueError("limits: the normaliser's std must be positive")
    return (lo - mean) / std, (hi - mean) / std


def normalised_slew(slew, mean: torch.Tensor, std: torch.Tensor, limits=None) -> torch.Tensor:
    """``slew`` in the space of the trajectories (x * std + mean; (J,) floats, one number or ``{joint: v}`` as ``ops.joint_slew`` takes
    them: the largest step between consecutive rows) as a (J,) fp32 host tensor in the sampler's normalised space: (v - margin) / std per
    joint in fp64, rounded toward zero, with ``ops.denormalised_slew_margin`` - what the scan's rounding and the denormalisation's can
    add to the difference of two denormalised values - so that consecutive rows of the DENORMALISED trajectories differ
    by at most v, evaluated exactly.  The margin needs a bound on |x std + mean|: max(|lo|, |hi|) of ``limits`` (the same space, as
    ``normalised_limits`` takes them) where a joint has both, else 2 pi - joint commands lie in [0, 2 pi).  +inf stays +inf; a v not
    above its margin raises ValueError."""
    from . import ops

    mean, std = mean.detach().reshape(-1).cpu().float().numpy(), std.detach().reshape(-1).cpu().float().numpy()
    J = std.size
    if not (std > 0).all():
        raise ValueError("slew: the normaliser's std must be positive")
    v = ops._slew_host(slew, J)[:J].astype(np.float64)
    bound = np.full(J, 2 * math.pi)
    if limits is not None:
        lo, hi = (np.abs(a[:J].astype(np.float64)) for a in ops._limits_host(limits, J))
        both = np.isfinite(lo) & np.isfinite(hi)
        bound = np.where(both, np.maximum(lo, hi), bound)
    margin = ops.denormalised_slew_margin(bound, mean, std)
    finite = np.isfinite(v)
    if (finite & ~(v > margin)).any():
        j = int(np.argmax(finite & ~(v > margin)))
        raise ValueError(f"slew: v[{j}] = {v[j]} is not above the margin {margin[j]:.3e} of the fp32 arithmetic")
    exact = np.where(finite, (np.where(finite, v, 0.0) - margin) / std.astype(np.float64), np.inf)
    out = exact.astype(np.float32)
    over = out.astype(np.float64) > exact
    out[over] = np.nextafter(out[over], np.float32(0))
    return torch.from_numpy(out)


def normalised_accel(accel, mean: torch.Tensor, std: torch.Tensor, limits=None) -> torch.Tensor:
    """``accel`` in the space of the trajectories (x * std + mean; (J,) floats, one number or ``{joint: a}`` as ``ops.joint_accel`` takes
    them: the largest second difference over three consecutive rows) as a (J,) fp32 host tensor in the sampler's normalised space:
    (a - margin) / std per joint in fp64, rounded toward zero, with ``ops.denormalised_accel_margin``, so that the second
    difference of the DENORMALISED trajectories is at most a, evaluated exactly, wherever the acceleration limit is the one that binds.
    The margin needs a bound on |x std + mean|, as ``normalised_slew``'s does, and takes it the same way.  +inf stays +inf; an a not
    above its margin raises ValueError."""
    from . import ops

    mean, std = mean.detach().reshape(-1).cpu().float().numpy(), std.detach().reshape(-1).cpu().float().numpy()
    J = std.size
    if not (std > 0).all():
        raise ValueError("accel: the normaliser's std must be positive")
    a = ops._accel_host(accel, J)[:J].astype(np.float64)
    bound = np.full(J, 2 * math.pi)
    if limits is not None:
        lo, hi = (np.abs(b[:J].astype(np.float64)) for b in ops._limits_host(limits, J))
        both = np.isfinite(lo) & np.isfinite(hi)
        bound = np.where(both, np.maximum(lo, hi), bound)
    margin = ops.denormalised_accel_margin(bound, mean, std)
    finite = np.isfinite(a)
    if (finite & ~(a > margin)).any():
        j = int(np.argmax(finite & ~(a > margin)))
        raise ValueError(f"accel: a[{j}] = {a[j]} is not above the margin {margin[j]:.3e} of the fp32 arithmetic")
    exact = np.where(finite, (np.where(finite, a, 0.0) - margin) / std.astype(np.float64), np.inf)
    out = exact.astype(np.float32)
    over = out.astype(np.float64) > exact
    out[over] = np.nextafter(out[over], np.float32(0))
    return torch.from_numpy(out)


def assemble_report(parts: Sequence[dict], *, timesteps: Optional[Sequence[int]], steps: int, draws: int, max_mode: int, angular: bool,
                    solver: str = "ddim") -> dict:
    """The report from the per-batch marginals, in fp64 on the host.  A part holds, for its C windows: ``err`` (C, G), ``row_err`` (C, G, T),
    ``joint_err`` (C, G, J) (mean squared errors in radians^2: ``ops.trajectory_errors``), ``best`` (C,) and ``medoid`` (C,) draw indices,
    ``spread`` (C, G) the mean squared distance of every draw to the medoid, and ``loss`` (C, K) or None (a distilled decoder predicts no
    noise).  Every window weighs the same, whichever batch it came in."""
    err = torch.cat([_f64(p["err"]) for p in parts])
    row = torch.cat([_f64(p["row_err"]) for p in parts])
    joint = torch.cat([_f64(p["joint_err"]) for p in parts])
    best = torch.cat([torch.as_tensor(p["best"]).to("cpu", torch.int64) for p in parts])
    med = torch.cat([torch.as_tensor(p["medoid"]).to("cpu", torch.int64) for p in parts])
    spread = torch.cat([_f64(p["spread"]) for p in parts])
    n = err.shape[0]
    at = torch.arange(n)
    report = {"n_windows": int(n), "val_loss": None, "val_loss_by_t": None}
    if all(p.get("loss") is not None for p in parts):
        loss = torch.cat([_f64(p["loss"]) for p in parts])
        by_t = loss.mean(0)
        report["val_loss"] = float(by_t.mean())
        report["val_loss_by_t"] = [[int(t), float(v)] for t, v in zip(timesteps, by_t)]
    report.update(
        rmse_first_draw=math.sqrt(float(err[:, 0].mean())),
        rmse_medoid=math.sqrt(float(err[at, med].mean())),
        rmse_best_of_G=math.sqrt(float(err[at, best].mean())),
        rmse_by_row=[math.sqrt(float(v)) for v in row[at, med].mean(0)],
        rmse_by_joint=[math.sqrt(float(v)) for v in joint[at, med].mean(0)],
        spread=math.sqrt(float(spread.mean())),
        steps=int(steps), draws=int(draws), max_mode=int(max_mode), angular=bool(angular), solver=str(solver))
    return report


def _has_context(model) -> bool:
    return any(e is not None for e in (model.action_history_encoder, model.imu_encoder, model.joint_states_encoder, model.image_sequence_encoder,
                                       model.game_state_encoder))


@torch.no_grad()
def evaluate(model, source, idx, *, steps: int = 30, draws: int = 1, grid: int = 8, batch: int = 64, seed: int = 0, max_mode: int = 3,
             angular: bool = True, timesteps: Optional[Sequence[int]] = None, distilled: bool = False, keep: Optional[list] = None, solver: str = "ddim",
             limits=None, reproject: bool = False, slew=None, accel=None) -> dict:
    """The report (a plain dict of Python floats, ints and lists) of ``model`` on the windows ``idx`` of ``source`` (``cli.DataSource``), in
    batches of ``batch`` windows from ``source.batch``.  The model must be in ``eval()``.  Per batch: the context is encoded once; the loss
    grid runs at ``timesteps`` (default ``default_timesteps(grid)``); ``draws`` = G trajectories per window are sampled with ``steps`` DDIM
    steps (``model.sample(draws=G)``; ``solver="multistep"``: with the second-order multistep solver on the same ``steps`` timesteps - the
    instrument for "10 steps against 30" then also says what the solver buys; the report names it in its ``solver`` entry);
    ``limits`` / ``reproject``: the draws are sampled under joint limits given in the space of the target trajectories
    (``normalised_limits``, ``model.sample(limits=...)``) - what a set of limits costs in rmse; the report then gains a ``limits`` entry,
    ``[lo, hi]`` per joint with None for an open side, and ``reproject``;
    ``slew``: the draws are sampled under slew limits given in the same space (``normalised_slew``, ``model.sample(slew=...)``); the report
    then gains a ``slew`` entry, v per joint with None for none.  With or without it the report carries ``max_step_by_joint``: the
    largest |step| between consecutive rows of the sampled trajectories, all draws, in the space of the targets (``ops.max_step``) - the
    number from which a slew limit is chosen, and the one that shows it held: with ``--slew`` it is <= v, as long as the denormalised
    values stay inside the bound the margin was derived for (``normalised_slew``);
    ``accel``: the draws are sampled under acceleration limits given in the same space (``normalised_accel``, ``model.sample(accel=...)``);
    the report then gains an ``accel`` entry.  With or without it the report carries ``max_accel_by_joint``: the largest second
    difference over three consecutive rows of the sampled trajectories, all draws, in the space of the targets (``ops.max_accel``) - the
    number from which an acceleration limit is chosen (where the box or the slew limit wins at a row it can exceed ``accel``: there is
    no braking ahead of the box);
    ``ops.select_medoid`` and ``ops.trajectory_errors`` follow.  ``distilled``: the model is a one-step
    student - one forward at t = 0 on G start noises through the shared loop form; it predicts no noise, so its ``val_loss*`` are None;
    under ``limits`` / ``slew`` its output, which is x0, is projected inside the launch (``model.sample_direct``) and ``max_step_by_joint``
    is reported as for the rollout; ``reproject`` and ``solver="multistep"`` raise for it.
    A model without context encoders (decoder pretraining) gets ten random context rows per window from the same generator.
    ``keep``: a list that receives, per batch, the tensors the marginals were computed from (tests).
    rmse_* are in radians; ``rmse_by_row`` / ``rmse_by_joint`` refer to the medoid draw; ``spread`` is the root mean squared distance, in
    radians, of the G draws to their medoid."""
    from . import ops

    if model.training:
        raise RuntimeError("evaluate: the model must be in eval() (dropout would be live)")
    G = check_draws(draws)
    ts = check_timesteps(timesteps) if timesteps is not None else default_timesteps(grid)
    if steps < 1 or batch < 1:
        raise ValueError("evaluate: steps and batch must be positive")
    if solver not in ("ddim", "multistep") or (distilled and solver != "ddim"):
        raise ValueError(f"evaluate: solver must be 'ddim' or 'multistep' (a distilled decoder has no rollout: 'ddim'), got {solver!r}")
    limits_given = limits
    if reproject and distilled:
        raise ValueError("evaluate: a distilled decoder predicts x0 itself - there is no eps to recompute (reproject)")
    if limits is not None:
        J = model.mean.numel()
        given = [[None if math.isinf(a) else a for a in pair]      # as given, per joint: [lo, hi], None for an open side
                 for pair in zip(*(v[:J].tolist() for v in ops._limits_host(limits, J)))]
        limits = normalised_limits(limits, model.mean, model.std)
    if slew is not None:
        slew_given = [None if math.isinf(a) else a for a in ops._slew_host(slew, model.mean.numel())[: model.mean.numel()].tolist()]
        slew = normalised_slew(slew, model.mean, model.std, limits_given)
    if accel is not None:
        accel_given = [None if math.isinf(a) else a for a in ops._accel_host(accel, model.mean.numel())[: model.mean.numel()].tolist()]
        accel = normalised_accel(accel, model.mean, model.std, limits_given)
    idx = torch.as_tensor(idx, dtype=torch.int64).reshape(-1)
    if idx.numel() == 0:
        raise ValueError("evaluate: no windows to evaluate")
    device = model.mean.device
    gen = torch.Generator(device=device).manual_seed(int(seed))
    t_dev = torch.tensor(ts, dtype=torch.int64, device=device)
    acp = ops.alphas_cumprod().to(device)
    K, d = len(ts), model.hidden_dim
    parts, steps_seen, accels_seen = [], [], []
    for at in range(0, idx.numel(), batch):
        data = source.batch(idx[at : at + batch])
        target = data["joint_command"].to(torch.float32).contiguous()
        Cn, T, J = target.shape
        if _has_context(model):
            ctx = model.encode_input_data({k: data[k].contiguous() for k in CONTEXT_KEYS if k in data})
        else:
            ctx = [torch.randn(Cn, 10, d, device=device, generator=gen)]
        part = {"loss": None}
        if not distilled:
            noise = torch.randn(Cn * K, T, J, device=device, generator=gen)
            x0n = ops.normalize(target, model.mean, model.std)
            part["loss"], eps = ops.noise_loss_grid(model, ctx, x0n, noise, t_dev, acp=acp, return_eps=True)
        x_T = torch.randn(Cn * G, T, J, device=device, generator=gen)
        if distilled and limits is None and slew is None and accel is None:
            x = model.forward_with_context(ctx, x_T, torch.zeros(Cn * G, device=device), draws=G)
        elif distilled:   # the student's output is x0: limits and slew project it inside the same launch (model.sample_direct)
            x = model.sample_direct(ctx, x_T, limits=limits, slew=slew, draws=G, max_mode=max_mode, accel=accel)
        else:
            x = model.sample(ctx, x_T, steps, max_mode=max_mode, draws=G, solver=solver, limits=limits, reproject=reproject, slew=slew, accel=accel)
        x = x.contiguous()
        steps_seen.append(ops.max_step(x, model.mean, model.std).amax(0).cpu())
        accels_seen.append(ops.max_accel(x, model.mean, model.std).amax(0).cpu())
        part["medoid"], chosen = ops.select_medoid(x, G)
        part["err"], part["row_err"], part["joint_err"], part["best"] = ops.trajectory_errors(x, target, model.mean, model.std, draws=G, angular=angular)
        # the distance of every draw to the medoid, in radians: the same kernel against the denormalised medoid, nothing to wrap
        part["spread"] = ops.trajectory_errors(x, ops.normalize(chosen, model.mean, model.std, inverse=True), model.mean, model.std, draws=G,
                                               angular=False)[0]
        if keep is not None:
            keep.append({"x": x, "target": target, "medoid_x": chosen, **({} if distilled else {"eps": eps, "noise": noise}), **part})
        parts.append({k: (None if v is None else v.cpu()) for k, v in part.items()})
    report = assemble_report(parts, timesteps=ts, steps=steps, draws=G, max_mode=max_mode, angular=angular, solver=solver)
    report["max_step_by_joint"] = [float(v) for v in torch.stack(steps_seen).amax(0)]
    report["max_accel_by_joint"] = [float(v) for v in torch.stack(accels_seen).amax(0)]
    if limits is not None:
        report.update(limits=given, reproject=bool(reproject))
    if slew is not None:
        report["slew"] = slew_given
    if accel is not None:
        report["accel"] = accel_given
    return report
