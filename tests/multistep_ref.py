"""CPU reference of the sampler's second-order multistep solver (sd_ddim_sample_multistep; a plain helper module, not a conftest):
tests/hold_ref.py's loop with the history term of DPM-Solver++ 2M in its x0 form, in plain torch and generic over the dtype.

With (a_t, a_prev) = ddim_ref.step_coefficients of step i, lambda(a) = 0.5 log(a / (1 - a)) and h_i = lambda(a_prev) - lambda(a_t):
  x0_i    = (x_i - sqrt(1 - a_t) e_i) / sqrt(a_t)
  x_{i+1} = sqrt(a_prev) x0_i + sqrt(1 - a_prev) e_i + w_i (x0_{i-1} - x0_i)
  w_i     = sqrt(a_prev) expm1(-h_i) h_i / (2 h_{i-1});   w_0 = 0 (no history yet);   w_i = 0 where a_prev = 1 (lambda is infinite)
Every w_i = 0 is ddim_ref.sample.  Held elements (hold_ref.sample's semantics: bool mask (B, T, J)) take the hold's value after every
step; the x0 that enters the next step's history is the model's for all elements.  The noise prediction is the denoiser's for all elements.

`weights` is this module's own float64 computation of w (from log and log1p, and exp(-h) - 1 instead of expm1: another route to the same
numbers than ops.multistep_weights takes)."""

from __future__ import annotations

import math

import torch

import pin_ref
from oracle import ddim_ref

Tensor = torch.Tensor


def weights(num_inference_steps: int, acp: Tensor | None = None, num_train_timesteps: int = 1000) -> list:
    """w_0 .. w_{n-1} as Python floats (float64) on the leading grid of ddim_ref.timesteps, from the fp32 table ``acp``."""
    acp = ddim_ref.alphas_cumprod() if acp is None else acp
    ratio = num_train_timesteps // num_inference_steps
    ts = ddim_ref.timesteps(num_inference_steps).tolist()

    def lam(t: int) -> float:
        a = float(acp[t].to(torch.float32))
        return 0.5 * (math.log(a) - math.log1p(-a))

    out = []
    for i, t in enumerate(ts):
        prev = t - ratio
        if i == 0 or prev < 0:
            out.append(0.0)
            continue
        h = lam(prev) - lam(t)
        h_before = lam(t) - lam(ts[i - 1])
        out.append(math.sqrt(float(acp[prev].to(torch.float32))) * (math.exp(-h) - 1.0) * h / (2.0 * h_before))
    return out


def sample(denoise, x_T: Tensor, known: Tensor | None, mask: Tensor | None, num_inference_steps: int, w, acp: Tensor | None = None):
    """(x after every step, the held value after every step, the noise prediction of every step) - three lists of (B, T, J).
    ``w``: num_inference_steps weights (floats); ``mask`` None: nothing held (``known`` is then not read)."""
    acp = ddim_ref.alphas_cumprod() if acp is None else acp
    ts = ddim_ref.timesteps(num_inference_steps).tolist()
    assert len(w) == len(ts)
    if mask is None:
        mask, known = torch.zeros(x_T.shape, dtype=torch.bool), torch.zeros_like(x_T)
    assert mask.dtype == torch.bool and tuple(mask.shape) == tuple(x_T.shape)
    x = torch.where(mask, pin_ref.pinned_value(known, x_T, ddim_ref.step_coefficients(ts[0], num_inference_steps, acp)[0]), x_T)
    out, held, eps = [], [], []
    x0_before = None
    for i, t in enumerate(ts):
        e = denoise(x, t)
        a_t, a_p = (a.to(x.dtype) for a in ddim_ref.step_coefficients(t, num_inference_steps, acp))
        x0 = (x - (1 - a_t).sqrt() * e) / a_t.sqrt()
        nxt = a_p.sqrt() * x0 + (1 - a_p).sqrt() * e          # ddim_ref.step, expression for expression
        if float(w[i]) != 0.0:
            nxt = nxt + float(w[i]) * (x0_before - x0)
        p = pin_ref.pinned_value(known, x_T, a_p)
        x = torch.where(mask, p, nxt)
        x0_before = x0
        out.append(x)
        held.append(p)
        eps.append(e)
    return out, held, eps
