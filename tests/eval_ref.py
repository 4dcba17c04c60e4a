"""fp64 CPU references of the held-out evaluation (csrc/sd_eval.hip, soccerdiffusion_amd/evaluation.py) and the error bounds an fp32 kernel
is held to against them.  The bounds are derived, not measured:

  a sum of n non-negative fp32 terms in any order, divided once, is within (n + 2) 2^-24 of its exact value, relatively (n - 1 additions, the
  squaring, the division, first order); and a term d^2 whose d carries an absolute error of at most delta is off by at most
  2 |d| delta + delta^2.  So for a mean over n terms:   bound = (n + 2) 2^-24 ref + mean(2 |d| delta + delta^2).

  sd_eval_sqerr_rows: d = a - b, delta = 2^-23 (|a| + |b|).
  sd_eval_trajectory_errors: d = x std + mean - target (wrapped), delta = 8 2^-24 (|x std| + |mean| + |target| + 2 pi): the roundings of
  x std, + mean, - target and of the wrap (the quotient's rounding cannot move rintf by more than one turn, which leaves d^2 within
  2 |d| delta of itself only at |d| = pi, where both choices have the same square; the fp32 value of 2 pi is 0.47 2^-24 off, relatively)."""

import math

import numpy as np

import draws_ref

U = 2.0 ** -24
TWO_PI = 2.0 * math.pi


def _np64(t):
    return np.asarray(t.detach().cpu().numpy() if hasattr(t, "detach") else t, dtype=np.float64)


def sqerr_rows(a, b):
    """(ref (rows,), bound (rows,)) of sd_eval_sqerr_rows on the same fp32 inputs."""
    a, b = _np64(a), _np64(b)
    a, b = a.reshape(a.shape[0], -1), b.reshape(b.shape[0], -1)
    d = a - b
    per = d.shape[1]
    ref = (d * d).mean(axis=1)
    delta = 2.0 * U * (np.abs(a) + np.abs(b))
    return ref, (per + 2) * U * ref + (2 * np.abs(d) * delta + delta * delta).mean(axis=1)


def wrap(d):
    return d - TWO_PI * np.rint(d / TWO_PI)


def trajectory_errors(x, target, mean, std, G, angular=True):
    """{name: (ref, bound)} for err (C, G), row_err (C, G, T), joint_err (C, G, J), and "best": (C,) the fp64 argmin of err (lowest index)."""
    target, mean, std = _np64(target), _np64(mean), _np64(std)
    Cn, T, J = target.shape
    x = _np64(x).reshape(Cn, G, T, J)
    xs = x * std
    d = xs + mean - target[:, None]
    if angular:
        d = wrap(d)
    delta = 8 * U * (np.abs(xs) + np.abs(mean) + np.abs(target[:, None]) + TWO_PI)
    sq, slack = d * d, 2 * np.abs(d) * delta + delta * delta
    out = {}
    for name, axes, n in (("err", (2, 3), T * J), ("row_err", (3,), J), ("joint_err", (2,), T)):
        ref = sq.mean(axis=axes)
        out[name] = (ref, (n + 2) * U * ref + slack.mean(axis=axes))
    out["best"] = np.argmin(out["err"][0], axis=1)
    return out


def report(parts, *, timesteps, steps, draws, max_mode, angular, mean, std):
    """evaluation.evaluate's report in fp64 from the tensors the device produced (``keep``): per batch x (C G, T, J) the samples, target
    (C, T, J), and eps / noise (C K, T, J) or neither for a distilled decoder.  Medoid (draws_ref) and best draw are chosen here in fp64."""
    G = draws
    mean, std = _np64(mean), _np64(std)
    err, row, joint, spread, loss = [], [], [], [], []
    for p in parts:
        e = trajectory_errors(p["x"], p["target"], mean, std, G, angular)
        Cn, T, J = _np64(p["target"]).shape
        x = _np64(p["x"]).reshape(Cn, G, T, J)
        med, at = draws_ref.medoid(x, G), np.arange(Cn)
        best = e["best"]
        err.append(np.stack([e["err"][0][:, 0], e["err"][0][at, med], e["err"][0][at, best]], axis=1))
        row.append(e["row_err"][0][at, med])
        joint.append(e["joint_err"][0][at, med])
        dm = (x - x[at, med][:, None]) * std
        spread.append((dm * dm).mean(axis=(2, 3)))
        if "eps" in p:
            K = len(timesteps)
            loss.append(sqerr_rows(p["eps"], p["noise"])[0].reshape(Cn, K))
    err, row, joint, spread = (np.concatenate(v) for v in (err, row, joint, spread))
    out = {"n_windows": int(err.shape[0]), "val_loss": None, "val_loss_by_t": None}
    if loss:
        by_t = np.concatenate(loss).mean(axis=0)
        out["val_loss"] = float(by_t.mean())
        out["val_loss_by_t"] = [[int(t), float(v)] for t, v in zip(timesteps, by_t)]
    out.update(rmse_first_draw=math.sqrt(err[:, 0].mean()), rmse_medoid=math.sqrt(err[:, 1].mean()), rmse_best_of_G=math.sqrt(err[:, 2].mean()),
               rmse_by_row=[math.sqrt(v) for v in row.mean(axis=0)], rmse_by_joint=[math.sqrt(v) for v in joint.mean(axis=0)],
               spread=math.sqrt(spread.mean()), steps=int(steps), draws=int(draws), max_mode=int(max_mode), angular=bool(angular))
    return out
