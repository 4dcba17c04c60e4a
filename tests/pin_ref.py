"""CPU reference of the sampler's pinned leading rows (sd_ddim_sample_pin; a plain helper module, not a conftest): oracle/ddim_ref.py's
loop with the pinned rows written over x before the first step and after every step.

Row t of trajectory b is pinned iff t < rows[b].  With (a_t, a_prev) = ddim_ref.step_coefficients of a step:
  entry          x = sqrt(a_t of step 0) known + sqrt(1 - a_t of step 0) x_T   on the pinned rows
  after a step   x = sqrt(a_prev) known + sqrt(1 - a_prev) x_T                  on the pinned rows, ddim_ref.step everywhere else
so at the entry of every step the pinned rows are ddim_ref.add_noise(known, x_T, t) of that step's t, and the last step (a_prev = 1)
leaves known itself.  The noise prediction is the denoiser's for all rows."""

from __future__ import annotations

import torch

from oracle import ddim_ref

Tensor = torch.Tensor


def pin_mask(rows, B: int, T: int) -> Tensor:
    """(B, T, 1) bool: row t of trajectory b is pinned."""
    rows = torch.full((B,), int(rows)) if isinstance(rows, int) else torch.as_tensor(rows).reshape(B)
    return (torch.arange(T)[None, :] < rows[:, None])[:, :, None]


def pinned_value(known: Tensor, noise: Tensor, a: Tensor) -> Tensor:
    a = a.to(known.dtype)
    return a.sqrt() * known + (1 - a).sqrt() * noise


def sample(denoise, x_T: Tensor, known: Tensor, rows, num_inference_steps: int, acp: Tensor | None = None):
    """(x after every step, the pinned value after every step, the noise prediction of every step) - three lists of (B, T, J)."""
    acp = ddim_ref.alphas_cumprod() if acp is None else acp
    B, T, _ = x_T.shape
    mask = pin_mask(rows, B, T)
    ts = ddim_ref.timesteps(num_inference_steps).tolist()
    x = torch.where(mask, pinned_value(known, x_T, ddim_ref.step_coefficients(ts[0], num_inference_steps, acp)[0]), x_T)
    out, pinned, eps = [], [], []
    for t in ts:
        e = denoise(x, t)
        p = pinned_value(known, x_T, ddim_ref.step_coefficients(t, num_inference_steps, acp)[1])
        x = torch.where(mask, p, ddim_ref.step(e, t, x, num_inference_steps, acp))
        out.append(x)
        pinned.append(p)
        eps.append(e)
    return out, pinned, eps
