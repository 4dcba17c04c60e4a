"""Reference of the two-segment cross-attention of training with several noise draws per window (a plain helper module, not a conftest).

C * K trajectories attend to C shared contexts: trajectory b's keys are the Mc projected rows of context b // K followed by its own
projected step token at key index Mc - the order of ``cat(context, token)``.  ``forward`` / ``backward`` restate the attention and its
gradient segment by segment in plain torch, in the dtype of their inputs (float64: the yardstick; float32 on the CPU: the error fp32
itself makes).  ``expanded`` is the same attention written the ordinary way on the expanded memory, for torch autograd to differentiate:
tests/test_cpu_noise_draws.py pins the restatement against it.

Dropout: ``mask`` holds the multipliers (0 or 1 / (1 - p)) of the probabilities, shape (C * K, heads, T, Mc + 1); the normaliser is that
of the un-dropped probabilities (nn.MultiheadAttention)."""

from __future__ import annotations

import math

import torch


def _heads(x, heads):
    """(N, R, d) -> (N, heads, R, d / heads)"""
    N, R, d = x.shape
    return x.reshape(N, R, heads, d // heads).transpose(1, 2)


def _probs(q, kv_ctx, kv_tok, heads, draws):
    B, T, d = q.shape
    C, Mc, _ = kv_ctx.shape
    hd = d // heads
    qh = _heads(q, heads)                                   # (B, h, T, hd)
    kc, vc = _heads(kv_ctx[..., :d], heads), _heads(kv_ctx[..., d:], heads)   # (C, h, Mc, hd)
    kt, vt = _heads(kv_tok[..., :d], heads), _heads(kv_tok[..., d:], heads)   # (B, h, 1, hd)
    qg = qh.reshape(C, draws, heads, T, hd)
    s_ctx = torch.einsum("ckhtf,chmf->ckhtm", qg, kc).reshape(B, heads, T, Mc)
    s_tok = (qh * kt).sum(-1, keepdim=True)
    s = torch.cat([s_ctx, s_tok], -1) / math.sqrt(hd)
    lse = torch.logsumexp(s, -1)
    return qh, kc, vc, kt, vt, torch.exp(s - lse[..., None]), lse


def forward(q, kv_ctx, kv_tok, heads: int, draws: int, mask=None):
    """(out (B, T, d), lse2 (B, heads, T): the log2-domain log-sum-exp of the scaled scores)."""
    B, T, d = q.shape
    C, Mc, _ = kv_ctx.shape
    qh, kc, vc, kt, vt, p, lse = _probs(q, kv_ctx, kv_tok, heads, draws)
    pd = p if mask is None else p * mask
    o = torch.einsum("ckhtm,chmf->ckhtf", pd[..., :Mc].reshape(C, draws, heads, T, Mc), vc).reshape(B, heads, T, -1) + pd[..., Mc:] * vt
    return o.transpose(1, 2).reshape(B, T, d), lse / math.log(2.0)


def backward(q, kv_ctx, kv_tok, dO, heads: int, draws: int, mask=None):
    """(dq (B, T, d), dkv_ctx (C, Mc, 2d): summed over the draws of a context and their rows, dkv_tok (B, 1, 2d))."""
    B, T, d = q.shape
    C, Mc, _ = kv_ctx.shape
    hd = d // heads
    qh, kc, vc, kt, vt, p, _ = _probs(q, kv_ctx, kv_tok, heads, draws)
    m = torch.ones_like(p) if mask is None else mask
    pd = p * m
    dOh = _heads(dO, heads)                                  # (B, h, T, hd)
    dOg = dOh.reshape(C, draws, heads, T, hd)
    # dV = P_d^T dO
    dv_ctx = torch.einsum("ckhtm,ckhtf->chmf", pd[..., :Mc].reshape(C, draws, heads, T, Mc), dOg)
    dv_tok = (pd[..., Mc:] * dOh).sum(2, keepdim=True)       # (B, h, 1, hd)
    # dP = (dO V^T) o m, dS = P o (dP - sum_k dP P) / sqrt(hd)
    dp_ctx = torch.einsum("ckhtf,chmf->ckhtm", dOg, vc).reshape(B, heads, T, Mc)
    dp_tok = (dOh * vt).sum(-1, keepdim=True)
    dp = torch.cat([dp_ctx, dp_tok], -1) * m
    ds = p * (dp - (dp * p).sum(-1, keepdim=True)) / math.sqrt(hd)
    dsg = ds[..., :Mc].reshape(C, draws, heads, T, Mc)
    dqh = torch.einsum("ckhtm,chmf->ckhtf", dsg, kc).reshape(B, heads, T, hd) + ds[..., Mc:] * kt
    dk_ctx = torch.einsum("ckhtm,ckhtf->chmf", dsg, qh.reshape(C, draws, heads, T, hd))
    dk_tok = (ds[..., Mc:] * qh).sum(2, keepdim=True)

    def rows(x):   # (N, h, R, hd) -> (N, R, d)
        return x.transpose(1, 2).reshape(x.shape[0], x.shape[2], d)

    return rows(dqh), torch.cat([rows(dk_ctx), rows(dv_ctx)], -1), torch.cat([rows(dk_tok), rows(dv_tok)], -1)


def expand_kv(kv_ctx, kv_tok, draws: int):
    """The memory the existing path attends to: (B, Mc + 1, 2d)."""
    return torch.cat([kv_ctx.repeat_interleave(draws, 0), kv_tok], 1)


def expanded(q, kv, heads: int, mask=None):
    """Ordinary multi-head attention of q (B, T, d) over packed K | V (B, S, 2d), differentiable by torch autograd."""
    B, T, d = q.shape
    hd = d // heads
    qh, kh, vh = _heads(q, heads), _heads(kv[..., :d], heads), _heads(kv[..., d:], heads)
    p = torch.softmax(qh @ kh.transpose(-1, -2) / math.sqrt(hd), -1)
    if mask is not None:
        p = p * mask
    return (p @ vh).transpose(1, 2).reshape(B, T, d)


def case(d: int, heads: int, C: int, K: int, T: int, Mc: int, seed: int = 0):
    """fp64 inputs of one case: q, kv_ctx, kv_tok, dO.  Scores of O(1) spread, so that the softmax is neither flat nor one-hot."""
    g = torch.Generator().manual_seed(1000 * seed + 7 * d + 131 * K + 17 * T + Mc)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)   # noqa: E731
    hd = d // heads
    q = r(C * K, T, d) * (hd ** -0.25) * 1.5
    kv_ctx = r(C, Mc, 2 * d)
    kv_tok = r(C * K, 1, 2 * d)
    kv_ctx[..., :d] *= (hd ** -0.25) * 1.5
    kv_tok[..., :d] *= (hd ** -0.25) * 1.5
    return q, kv_ctx, kv_tok, r(C * K, T, d)
