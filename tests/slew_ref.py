"""CPU reference of the sampler's per-joint slew limits (sd_ddim_sample_slew; a plain helper module, not a conftest): tests/limits_ref.py's
loop with the scan over the rows of the predicted clean trajectory, in plain torch and generic over the dtype.

With x0 of step i as in limits_ref, v (J,) >= 0 (+inf: none), start (B, J) (NaN: none) or None, lo / hi the box, per trajectory and joint:
  y = start
  for t = 0 .. T-1:
    a = y - v;  c = y + v                                       one rounding each
    z = x0[t] < a ? a : (x0[t] > c ? c : x0[t])                 compares: a NaN x0 stays NaN, a NaN y limits nothing
    z = z < lo ? lo : (z > hi ? hi : z)                         the box last: it always wins
    if held: z = known[t]                                       a held element is the scan's state as it stands
    x0c[t] = z;  y = z
  e' = reproject && x0c != x0 ? (x - c0 x0c) / c1 : e;   x = c2 x0c + c3 e' + w (hist - x0c);   hist = x0c
Held elements take the hold's value after every step.  Infinite v without start is limits_ref.sample exactly."""

from __future__ import annotations

import torch

import limits_ref
import pin_ref
from oracle import ddim_ref

Tensor = torch.Tensor


def scan(x0: Tensor, v: Tensor, start: Tensor | None, lo: Tensor, hi: Tensor, known: Tensor | None = None, mask: Tensor | None = None):
    """The scan over dimension 1 of x0 (B, T, J): (x0c, side) with side int8 = -1 where the row was raised to y - v, +1 where it was lowered
    to y + v, 0 where the slew limit left it alone (before the box and the hold)."""
    B, T, J = x0.shape
    v, lo, hi = (t.to(x0.dtype) for t in (v, lo, hi))
    y = torch.full((B, J), float("nan"), dtype=x0.dtype) if start is None else start.to(x0.dtype)
    rows, sides = [], []
    for t in range(T):
        a, c = y - v, y + v
        below, above = x0[:, t] < a, x0[:, t] > c
        z = torch.where(below, a, torch.where(above, c, x0[:, t]))
        z = limits_ref.clamp(z, lo, hi)
        if mask is not None:
            z = torch.where(mask[:, t], known[:, t].to(x0.dtype), z)
        rows.append(z)
        sides.append(above.to(torch.int8) - below.to(torch.int8))
        y = z
    return torch.stack(rows, 1), torch.stack(sides, 1)


def sample(denoise, x_T: Tensor, known: Tensor | None, mask: Tensor | None, num_inference_steps: int, w, v: Tensor, start: Tensor | None,
           lo: Tensor, hi: Tensor, reproject: bool = False, acp: Tensor | None = None):
    """(x after every step, the held value after every step, the noise prediction of every step, the side every step's x0 was slewed on,
    every step's x0c) - five lists of (B, T, J).  Arguments as limits_ref.sample's, plus v and start."""
    acp = ddim_ref.alphas_cumprod() if acp is None else acp
    ts = ddim_ref.timesteps(num_inference_steps).tolist()
    w = [0.0] * len(ts) if w is None else w
    assert len(w) == len(ts)
    if mask is None:
        mask, known = torch.zeros(x_T.shape, dtype=torch.bool), torch.zeros_like(x_T)
    assert mask.dtype == torch.bool and tuple(mask.shape) == tuple(x_T.shape)
    x = torch.where(mask, pin_ref.pinned_value(known, x_T, ddim_ref.step_coefficients(ts[0], num_inference_steps, acp)[0]), x_T)
    out, held, eps, hit, clean = [], [], [], [], []
    x0_before = None
    for i, t in enumerate(ts):
        e = denoise(x, t)
        a_t, a_p = (a.to(x.dtype) for a in ddim_ref.step_coefficients(t, num_inference_steps, acp))
        x0 = (x - (1 - a_t).sqrt() * e) / a_t.sqrt()
        x0c, side = scan(x0, v, start, lo, hi, known, mask)
        e_used = torch.where(x0c == x0, e, (x - a_t.sqrt() * x0c) / (1 - a_t).sqrt()) if reproject else e
        nxt = a_p.sqrt() * x0c + (1 - a_p).sqrt() * e_used
        if float(w[i]) != 0.0:
            nxt = nxt + float(w[i]) * (x0_before - x0c)
        p = pin_ref.pinned_value(known, x_T, a_p)
        x = torch.where(mask, p, nxt)
        x0_before = x0c
        out.append(x)
        held.append(p)
        eps.append(e)
        hit.append(side)
        clean.append(x0c)
    return out, held, eps, hit, clean


def check_properties(x: Tensor, v: Tensor, start: Tensor | None, lo: Tensor, hi: Tensor, free: Tensor):
    """P1 and P2 of a final sample x (B, T, J), bitwise: (every free element inside the box, every free element within fl(p +- v) of its
    predecessor p - row t - 1, or start for row 0 - unless p is NaN or lies outside the box).  Two bools."""
    lo, hi, v = (t.to(x.dtype) for t in (lo, hi, v))
    inside = ((x >= lo) & (x <= hi)) | ~free
    first = torch.full_like(x[:, :1], float("nan")) if start is None else start.to(x.dtype).unsqueeze(1)
    p = torch.cat([first, x[:, :-1]], 1)
    exempt = torch.isnan(p) | (p < lo) | (p > hi) | ~free
    ok = ((x <= p + v) & (x >= p - v)) | exempt
    return bool(inside.all()), bool(ok.all())
