"""fp64 numpy restatement of ``sd_select_medoid`` (csrc/sd_session.hip): the representative of each context's draws.

x (C, G, T, J) or (C * G, T, J) with the draws of a context contiguous.  score[c, i] = sum_k |x[c, i] - x[c, k]|^2 in float64,
index[c] = the lowest i with the smallest score.  ``margins`` is what a test needs to know before it compares an fp32 kernel's choice
with this one: how far the runner-up's score lies above the best."""

import numpy as np


def _draws(x, G):
    x = np.asarray(x, dtype=np.float64)
    if x.ndim == 3:
        x = x.reshape(x.shape[0] // G, G, *x.shape[1:])
    if x.ndim != 4 or x.shape[1] != G:
        raise ValueError(f"expected (C, {G}, T, J) or (C * {G}, T, J), got {x.shape}")
    return x.reshape(x.shape[0], G, -1)


def scores(x, G):
    """(C, G) float64: summed squared distance of every draw to the draws of its context (itself included: zero)."""
    v = _draws(x, G)
    diff = v[:, :, None, :] - v[:, None, :, :]          # (C, G, G, T * J)
    return np.einsum("cikn,cikn->cik", diff, diff).sum(axis=2)


def medoid(x, G):
    """(C,) int64: argmin of ``scores`` per context, ties to the lowest index (numpy's argmin)."""
    return np.argmin(scores(x, G), axis=1)


def margins(x, G):
    """(C,) float64: (runner-up score - best score) / best score per context; inf for G = 1 or a best score of zero with a distinct
    runner-up, 0 for an exact tie."""
    s = np.sort(scores(x, G), axis=1)
    if G == 1:
        return np.full(s.shape[0], np.inf)
    with np.errstate(divide="ignore", invalid="ignore"):
        m = (s[:, 1] - s[:, 0]) / s[:, 0]
    return np.where(s[:, 1] == s[:, 0], 0.0, m)
