"""The definition the clipped optimizer step is held to, on CPU torch: ``torch.nn.utils.clip_grad_norm_`` with norm type 2
over one flat gradient, the sum of squares taken in fp64, and the fp32 ``torch.optim.AdamW`` single-tensor update on the clipped gradient.

    s    = sum_i (double) g[i] * (double) g[i]         (the product of two fp32 values is exact in fp64)
    norm = (float) sqrt(s)
    ok   = isfinite(norm)
    coef = min(1.0f, max_norm / (norm + 1e-6f))         fp32, one rounding per operation
"""

import math

import torch

F32 = torch.float32


def coef_from_norm(norm: torch.Tensor, max_norm: float) -> torch.Tensor:
    """The fp32 coefficient from an fp32 norm (a 0-dim CPU tensor): torch's ``clip_coef_clamped``."""
    assert norm.dtype == F32 and norm.device.type == "cpu"
    return torch.clamp(torch.tensor(max_norm, dtype=F32) / (norm + torch.tensor(1e-6, dtype=F32)), max=1.0)


def norm_coef(g: torch.Tensor, max_norm: float):
    """(norm, coef, ok): 0-dim fp32 CPU tensors and a bool; coef is None where the norm is not finite."""
    g = g.detach().cpu()
    assert g.dtype == F32
    g64 = g.double().reshape(-1)
    norm = torch.sqrt((g64 * g64).sum()).to(F32)
    ok = bool(torch.isfinite(norm))
    return norm, (coef_from_norm(norm, max_norm) if ok else None), ok


def clipped_adamw(p, g, m, v, max_norm, lr, beta1, beta2, eps, weight_decay, step):
    """One step on CPU fp32 tensors, in place: torch.optim.AdamW's single-tensor update (decoupled decay, lerp, addcmul, bias
    corrections, addcdiv) on ``g * coef``; nothing is touched where the norm is not finite.  Returns (norm, coef, ok)."""
    norm, coef, ok = norm_coef(g, max_norm)
    if not ok:
        return norm, coef, ok
    gc = g.detach().cpu() * coef
    p.mul_(1.0 - lr * weight_decay)
    m.lerp_(gc, 1.0 - beta1)
    v.mul_(beta2).addcmul_(gc, gc, value=1.0 - beta2)
    bc1, bc2 = 1.0 - beta1 ** step, 1.0 - beta2 ** step
    denom = (v.sqrt() / math.sqrt(bc2)).add_(eps)
    p.addcdiv_(m, denom, value=-(lr / bc1))
    return norm, coef, ok
