"""CPU reference of the sampler's per-joint limits (sd_ddim_sample_limits; a plain helper module, not a conftest): tests/multistep_ref.py's
loop with the clamp of the predicted clean trajectory, in plain torch and generic over the dtype.

With (c0, c1, c2, c3) = (sqrt a_t, sqrt(1 - a_t), sqrt a_prev, sqrt(1 - a_prev)) of step i, e the denoiser's prediction, w the multistep
weight (0: DDIM) and lo / hi (J,) limits in normalised space (-inf / +inf: none):
  x0  = (x - c1 e) / c0
  x0c = x0 < lo[j] ? lo[j] : (x0 > hi[j] ? hi[j] : x0)          two compares and selects: a NaN x0 stays NaN
  e'  = e                                                       reproject off
      = (x0c == x0) ? e : (x - c0 x0c) / c1                     reproject on
  x   = c2 x0c + c3 e' + w (hist - x0c);   hist = x0c
Held elements (bool mask (B, T, J)) take the hold's value after every step whatever the limits say; their history entry is x0c as
everything else's.  The noise prediction returned is the denoiser's for all elements.  Infinite limits are multistep_ref.sample exactly."""

from __future__ import annotations

import torch

import pin_ref
from oracle import ddim_ref

Tensor = torch.Tensor


def clamp(x0: Tensor, lo: Tensor, hi: Tensor) -> Tensor:
    """x0 < lo ? lo : (x0 > hi ? hi : x0), elementwise over the last dimension; NaN passes through (torch.clamp would, too - the selects
    are spelled out because they are the definition)."""
    lo, hi = lo.to(x0.dtype).expand_as(x0), hi.to(x0.dtype).expand_as(x0)
    return torch.where(x0 < lo, lo, torch.where(x0 > hi, hi, x0))


def sample(denoise, x_T: Tensor, known: Tensor | None, mask: Tensor | None, num_inference_steps: int, w, lo: Tensor, hi: Tensor,
           reproject: bool = False, acp: Tensor | None = None):
    """(x after every step, the held value after every step, the noise prediction of every step, the side every step's x0 was clamped on:
    int8, -1 at the lower bound, +1 at the upper, 0 not clamped) - four lists of (B, T, J).  ``w``: num_inference_steps weights (floats) or
    None (DDIM); ``mask`` None: nothing held."""
    acp = ddim_ref.alphas_cumprod() if acp is None else acp
    ts = ddim_ref.timesteps(num_inference_steps).tolist()
    w = [0.0] * len(ts) if w is None else w
    assert len(w) == len(ts)
    if mask is None:
        mask, known = torch.zeros(x_T.shape, dtype=torch.bool), torch.zeros_like(x_T)
    assert mask.dtype == torch.bool and tuple(mask.shape) == tuple(x_T.shape)
    x = torch.where(mask, pin_ref.pinned_value(known, x_T, ddim_ref.step_coefficients(ts[0], num_inference_steps, acp)[0]), x_T)
    out, held, eps, hit = [], [], [], []
    x0_before = None
    for i, t in enumerate(ts):
        e = denoise(x, t)
        a_t, a_p = (a.to(x.dtype) for a in ddim_ref.step_coefficients(t, num_inference_steps, acp))
        x0 = (x - (1 - a_t).sqrt() * e) / a_t.sqrt()
        x0c = clamp(x0, lo, hi)
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
        hit.append((x0 > hi.to(x0.dtype)).to(torch.int8) - (x0 < lo.to(x0.dtype)).to(torch.int8))
    return out, held, eps, hit
