"""CPU reference of the projection of a distilled one-step decoder's output (sd_direct_sample / sd_direct_project; a plain helper module,
not a conftest): a numpy fp32 restatement from the definition - hold, then slew_row row by row, then the box - one rounding per operation.

With raw (B, T, J) the network's output (it IS x0), v (J,) >= 0 (+inf or None: no slew limit), start (B, J) (NaN or None: row 0 is free),
lo / hi the box (-inf / +inf or None: none), known / mask the hold, per trajectory and joint:
  y = start
  for t = 0 .. T-1:
    a = fl(y - v);  c = fl(y + v)
    z = raw[t] < a ? a : (raw[t] > c ? c : raw[t])             compares: a NaN stays NaN, a NaN y limits nothing
    z = z < lo ? lo : (z > hi ? hi : z)                         the box last: it always wins
    if held: z = known[t]                                       a held element is the scan's state as it stands
    out[t] = y = z
Given raw this is compares, selects and one fp32 add and one fp32 subtract per row: two correct implementations agree bit for bit."""

from __future__ import annotations

import numpy as np

F = np.float32


def _row(a, J, fill):
    return np.full(J, fill, dtype=F) if a is None else np.asarray(a, dtype=F).reshape(-1)[:J].copy()


def project(raw, known=None, mask=None, lo=None, hi=None, v=None, start=None) -> np.ndarray:
    """out (B, T, J) fp32.  raw, known: (B, T, J); mask: (B, T, J) bool; lo, hi, v: (J,) (or longer: the padded 32-float arrays);
    start: (B, J) or (B, 32)."""
    raw = np.ascontiguousarray(np.asarray(raw, dtype=F))
    B, T, J = raw.shape
    lo, hi, v = _row(lo, J, -np.inf), _row(hi, J, np.inf), _row(v, J, np.inf)
    y = np.full((B, J), np.nan, dtype=F) if start is None else np.asarray(start, dtype=F)[:, :J].copy()
    if mask is not None:
        mask = np.asarray(mask, dtype=bool)
        known = np.asarray(known, dtype=F)
    out = np.empty_like(raw)
    with np.errstate(invalid="ignore"):   # inf - inf: a NaN bound, which limits nothing
        for t in range(T):
            x0 = raw[:, t]
            a, c = (y - v).astype(F), (y + v).astype(F)
            z = np.where(x0 < a, a, np.where(x0 > c, c, x0))
            z = np.where(z < lo, lo, np.where(z > hi, hi, z))
            if mask is not None:
                z = np.where(mask[:, t], known[:, t], z)
            out[:, t] = z
            y = z
    return out


def constraints_from(raw, seed: int = 0) -> dict:
    """Constraints that bind whatever the scale of ``raw`` (B, T, J): lo / hi the per-joint 25 % and 75 % quantiles, v the per-joint median
    of |row difference|, start given for the odd trajectories (a row of another trajectory) and NaN for the even ones, the mask 20 % random
    bits plus joint 1 held in full, known drawn at raw's scale.  Keyword arguments of ``project``."""
    raw = np.asarray(raw, dtype=F)
    B, T, J = raw.shape
    rng = np.random.default_rng(1000 + seed)
    flat = raw.reshape(B * T, J).astype(np.float64)
    lo, hi = np.quantile(flat, 0.25, axis=0).astype(F), np.quantile(flat, 0.75, axis=0).astype(F)
    v = np.median(np.abs(np.diff(raw.astype(np.float64), axis=1)).reshape(-1, J), axis=0).astype(F) if T > 1 else np.ones(J, dtype=F)
    start = np.full((B, J), np.nan, dtype=F)
    for b in range(1, B, 2):
        start[b] = raw[(b + 1) % B, T // 2]
    mask = rng.random((B, T, J)) < 0.2
    mask[:, :, 1] = True
    known = (rng.standard_normal((B, T, J)) * raw.std()).astype(F)
    return dict(known=known, mask=mask, lo=lo, hi=hi, v=v, start=start)


def moved_share(raw, out, mask=None) -> float:
    """The share of free elements whose bits the projection changed."""
    raw, out = np.asarray(raw, dtype=F), np.asarray(out, dtype=F)
    free = np.ones(raw.shape, dtype=bool) if mask is None else ~np.asarray(mask, dtype=bool)
    return float((raw.view(np.int32) != out.view(np.int32))[free].mean())
