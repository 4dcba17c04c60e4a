"""CPU reference of the sampler's per-joint acceleration limits (sd_ddim_sample_accel; a plain helper module, not a conftest):
tests/slew_ref.py's loop with a scan whose state is two rows, in plain torch and generic over the dtype.

With x0 of step i as in limits_ref, a (J,) >= 0 (+inf: none), v (J,) >= 0 (+inf: none), start (B, J) - row -1 - and start2 (B, J) - row -2 -
(NaN: none) or None, lo / hi the box, per trajectory and joint:
  y1 = start;  y2 = start2
  for t = 0 .. T-1:
    d  = y1 - y2                                                one rounding
    p  = y1 + d                                                 one rounding: the constant-velocity continuation
    al = p - a;  ah = p + a                                     one rounding each
    z  = x0[t] < al ? al : (x0[t] > ah ? ah : x0[t])            compares: a NaN x0 stays NaN, a NaN p limits nothing
    z  = slew_ref's row on (z, y1, v, lo, hi, held, known)      then the slew interval, then the box, then the hold - as they stand
    x0c[t] = z;  y2 = y1;  y1 = z
  e' = reproject && x0c != x0 ? (x - c0 x0c) / c1 : e;   x = c2 x0c + c3 e' + w (hist - x0c);   hist = x0c
The priority order is box, then slew, then acceleration; the row order is part of the definition; a held element enters the state as the
hold's value.  Held elements take the hold's value after every step.  Infinite a without start2 is slew_ref.sample exactly.

Properties of the last step, which returns x0c itself (check_properties, bitwise):
  P1, P2  slew_ref.check_properties as it is.
  P3      with A = [fl(p - a), fl(p + a)], S = [fl(y1 - v), fl(y1 + v)] and box = [lo, hi]: every free element with two predecessors that
          are not NaN lies in A, unless A, S and the box have no common point.  (Sequential clamping in one dimension lands in the
          intersection whenever there is one: clamping a point z of I1 to I2 moves it to the end of I2 nearest to it, and that end lies
          between z and any common point of I1 and I2, hence in I1; I1 and I2 meet in an interval, so the same step takes it into I3.)
  P4      all-infinite a without start2 is the slew call bit for bit, at every step.
  P5      a NaN prediction stays NaN and lifts the acceleration limit for the two rows after it."""

from __future__ import annotations

import torch

import limits_ref
import pin_ref
import slew_ref
from oracle import ddim_ref

Tensor = torch.Tensor


def scan(x0: Tensor, a: Tensor, start2: Tensor | None, v: Tensor, start: Tensor | None, lo: Tensor, hi: Tensor, known: Tensor | None = None,
         mask: Tensor | None = None):
    """The scan over dimension 1 of x0 (B, T, J): (x0c, side) with side int8 = -1 where the row was raised to p - a, +1 where it was lowered
    to p + a, 0 where the acceleration limit left it alone (before the slew interval, the box and the hold)."""
    B, T, J = x0.shape
    a, v, lo, hi = (t.to(x0.dtype) for t in (a, v, lo, hi))
    nan = torch.full((B, J), float("nan"), dtype=x0.dtype)
    y1 = nan if start is None else start.to(x0.dtype)
    y2 = nan if start2 is None else start2.to(x0.dtype)
    rows, sides = [], []
    for t in range(T):
        d = y1 - y2
        p = y1 + d
        al, ah = p - a, p + a
        below, above = x0[:, t] < al, x0[:, t] > ah
        z = torch.where(below, al, torch.where(above, ah, x0[:, t]))
        sl, sh = y1 - v, y1 + v
        z = torch.where(z < sl, sl, torch.where(z > sh, sh, z))
        z = limits_ref.clamp(z, lo, hi)
        if mask is not None:
            z = torch.where(mask[:, t], known[:, t].to(x0.dtype), z)
        rows.append(z)
        sides.append(above.to(torch.int8) - below.to(torch.int8))
        y2, y1 = y1, z
    return torch.stack(rows, 1), torch.stack(sides, 1)


def sample(denoise, x_T: Tensor, known: Tensor | None, mask: Tensor | None, num_inference_steps: int, w, a: Tensor, start2: Tensor | None,
           v: Tensor, start: Tensor | None, lo: Tensor, hi: Tensor, reproject: bool = False, acp: Tensor | None = None):
    """(x after every step, the held value after every step, the noise prediction of every step, the side every step's x0 was limited on by
    the acceleration clamp, every step's x0c) - five lists of (B, T, J).  Arguments as slew_ref.sample's, plus a and start2."""
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
        a_t, a_p = (c.to(x.dtype) for c in ddim_ref.step_coefficients(t, num_inference_steps, acp))
        x0 = (x - (1 - a_t).sqrt() * e) / a_t.sqrt()
        x0c, side = scan(x0, a, start2, v, start, lo, hi, known, mask)
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


def intervals(x: Tensor, a: Tensor, start2: Tensor | None, v: Tensor, start: Tensor | None):
    """Of a final sample x (B, T, J): (al, ah, sl, sh, both) - the acceleration interval A and the slew interval S of every element from its
    two predecessors in x (rows -1 and -2: start and start2), each bound rounded as the scan rounds it, and where both predecessors exist
    (neither is NaN)."""
    a, v = a.to(x.dtype), v.to(x.dtype)
    nan = torch.full_like(x[:, :1], float("nan"))
    s1 = nan if start is None else start.to(x.dtype).unsqueeze(1)
    s2 = nan if start2 is None else start2.to(x.dtype).unsqueeze(1)
    y1 = torch.cat([s1, x[:, :-1]], 1)
    y2 = torch.cat([s2, s1, x[:, :-2]], 1)[:, :x.shape[1]]
    p = y1 + (y1 - y2)
    return p - a, p + a, y1 - v, y1 + v, ~(torch.isnan(y1) | torch.isnan(y2))


def check_properties(x: Tensor, a: Tensor, start2: Tensor | None, v: Tensor, start: Tensor | None, lo: Tensor, hi: Tensor, free: Tensor):
    """P1, P2 and P3 of a final sample x (B, T, J), bitwise.  Three bools."""
    p1, p2 = slew_ref.check_properties(x, v, start, lo, hi, free)
    lo, hi = lo.to(x.dtype), hi.to(x.dtype)
    al, ah, sl, sh, both = intervals(x, a, start2, v, start)
    low = torch.maximum(torch.maximum(al, sl), lo.expand_as(x))
    high = torch.minimum(torch.minimum(ah, sh), hi.expand_as(x))
    exempt = ~free | ~both | torch.isnan(al) | torch.isnan(ah) | ~(low <= high)
    p3 = ((x >= al) & (x <= ah)) | exempt
    return p1, p2, bool(p3.all())
