"""CPU reference of the sampler's held elements (sd_ddim_sample_hold; a plain helper module, not a conftest): tests/pin_ref.py's loop with
an arbitrary bool mask (B, T, J) in place of the leading rows.

Element (b, t, j) is held iff mask[b, t, j].  With (a_t, a_prev) = ddim_ref.step_coefficients of a step:
  entry          x = sqrt(a_t of step 0) known + sqrt(1 - a_t of step 0) x_T   on the held elements
  after a step   x = sqrt(a_prev) known + sqrt(1 - a_prev) x_T                  on the held elements, ddim_ref.step everywhere else
The noise prediction is the denoiser's for all elements.  A mask whose set rows are the leading rows[b] full rows is pin_ref.sample."""

from __future__ import annotations

import torch

import pin_ref
from oracle import ddim_ref

Tensor = torch.Tensor


def rows_mask(rows, B: int, T: int, J: int) -> Tensor:
    """(B, T, J) bool: the leading rows[b] rows of trajectory b, all joints."""
    return pin_ref.pin_mask(rows, B, T).expand(B, T, J).clone()


def pack(mask: Tensor) -> Tensor:
    """The (B, T) int32 words of a (B, T, J) bool mask, bit j = joint j, computed bit by bit in Python integers (independent of
    ops.hold_mask's tensor arithmetic)."""
    B, T, J = mask.shape
    words = torch.zeros(B, T, dtype=torch.int32)
    for b in range(B):
        for t in range(T):
            w = sum(1 << j for j in range(J) if bool(mask[b, t, j]))
            words[b, t] = w - (1 << 32) if w >= (1 << 31) else w
    return words


def sample(denoise, x_T: Tensor, known: Tensor, mask: Tensor, num_inference_steps: int, acp: Tensor | None = None):
    """(x after every step, the held value after every step, the noise prediction of every step) - three lists of (B, T, J)."""
    acp = ddim_ref.alphas_cumprod() if acp is None else acp
    assert mask.dtype == torch.bool and tuple(mask.shape) == tuple(x_T.shape)
    ts = ddim_ref.timesteps(num_inference_steps).tolist()
    x = torch.where(mask, pin_ref.pinned_value(known, x_T, ddim_ref.step_coefficients(ts[0], num_inference_steps, acp)[0]), x_T)
    out, held, eps = [], [], []
    for t in ts:
        e = denoise(x, t)
        p = pin_ref.pinned_value(known, x_T, ddim_ref.step_coefficients(t, num_inference_steps, acp)[1])
        x = torch.where(mask, p, ddim_ref.step(e, t, x, num_inference_steps, acp))
        out.append(x)
        held.append(p)
        eps.append(e)
    return out, held, eps
