"""fp64 numpy restatement of ``sd_select_coherent`` (csrc/sd_session.hip): the draw of each context that continues its previous plan.

x (C, G, T, J) or (C * G, T, J) with the draws of a context contiguous; prev (Cp, T, J), context c reads prev[robots[c]] (prev[c] without
``robots``), NaN = no plan there; shift = S, R = T - S; w (T,) row weights >= 0, only w[:R] matter; lam >= 0.

    coh[c, g]  = sum over tau < R, j of w[tau] * (x[c, g, tau, j] - prev[., tau + S, j])^2, an element LEFT OUT where prev is NaN or w[tau] == 0
    med[c, g]  = draws_ref.scores
    cost[c, g] = coh + lam * med  where the context has a plan (an element that is not left out), else med
    index[c]   = the lowest g with the smallest cost

Everything here is float64 on the values the kernel reads: the fp32 x, prev and w as they are, and ``lam`` as the fp32 number the Python
layer hands to the kernel (``ops.coherence_lambda``).

The error of the kernel's fp32 cost against this, relative to the cost (u = 2^-24; every term is >= 0, so relative errors of sums do not
grow by cancellation; first order in u, the second-order terms are below 1e-6 of it at these sizes):
  * a coherence term: the difference rounds (u on d, 2 u on d^2), the square rounds (u), the weight multiply rounds (u): 4 u, one ulp more
    than a medoid distance term (3 u);
  * its sum: a lane adds at most ceil(R J / 64) terms in sequence and the butterfly adds 6 levels: (ceil(R J / 64) + 6) u;
  * med: the same with T J elements and 3 u per term, plus the G - 1 additions of the score: (ceil(T J / 64) + 8 + G) u;
  * cost: lam * med rounds (u) and the sum rounds (u); the relative error of a sum of non-negative parts is at most the larger part's.
  Altogether at most (ceil(T J / 64) + G + 10) u.  The project's bound for these sums (tests/test_gpu_draws.py) is (T J + G) 2^-23 =
  2 (T J + G) u, which covers it - the extra ulp of the weight multiply included - as soon as T J >= 11; the smallest case the tests
  use has T J = 21.  ``bound(T, J, G)`` is that project bound, unchanged."""

import numpy as np

import draws_ref


def _draws(x, G):
    x = np.asarray(x, dtype=np.float64)
    if x.ndim == 3:
        x = x.reshape(x.shape[0] // G, G, *x.shape[1:])
    if x.ndim != 4 or x.shape[1] != G:
        raise ValueError(f"expected (C, {G}, T, J) or (C * {G}, T, J), got {x.shape}")
    return x


def _overlap(x, G, prev, shift, w, robots):
    """x (C, G, R, J), the plan rows they meet (C, R, J), the weights (R,) and which elements count (C, R, J)."""
    x = _draws(x, G)
    Cn, _, T, J = x.shape
    prev = np.asarray(prev, dtype=np.float64)
    if robots is not None:
        prev = prev[np.asarray(robots, dtype=np.int64)]
    if prev.shape != (Cn, T, J) or not 0 <= shift < T:
        raise ValueError(f"prev {prev.shape} / shift {shift} do not fit x {x.shape}")
    R = T - shift
    w = np.asarray(w, dtype=np.float64)[:R]
    p = prev[:, shift:]
    counts = ~np.isnan(p) & (w > 0)[None, :, None]
    return x[:, :, :R], p, w, counts


def has_plan(x, G, prev, shift, w, robots=None):
    """(C,) bool: the context has an overlap element with a positive weight and a plan that is not NaN."""
    return _overlap(x, G, prev, shift, w, robots)[3].any(axis=(1, 2))


def coherence(x, G, prev, shift, w, robots=None):
    """(C, G) float64: the weighted squared distance of every draw to its context's plan over the rows both describe."""
    xo, p, w, counts = _overlap(x, G, prev, shift, w, robots)
    d = xo - np.where(counts, p, 0.0)[:, None]
    term = w[None, None, :, None] * (d * d)
    return np.where(counts[:, None], term, 0.0).sum(axis=(2, 3))


def costs(x, G, prev, shift, w, lam, robots=None):
    """(C, G) float64: what the selection compares."""
    coh = coherence(x, G, prev, shift, w, robots)
    plan = has_plan(x, G, prev, shift, w, robots)
    if np.all(plan) and lam == 0:
        return coh
    med = draws_ref.scores(_draws(x, G), G)
    return np.where(plan[:, None], coh + np.float64(lam) * med, med)


def choose(x, G, prev, shift, w, lam, robots=None):
    """(C,) int64: the lowest argmin of ``costs`` per context (numpy's argmin)."""
    return np.argmin(costs(x, G, prev, shift, w, lam, robots), axis=1)


def margins(x, G, prev, shift, w, lam, robots=None):
    """(C,) float64: ``draws_ref.margins`` on these costs - (runner-up - best) / best; inf for G = 1, 0 for an exact tie."""
    s = np.sort(costs(x, G, prev, shift, w, lam, robots), axis=1)
    if G == 1:
        return np.full(s.shape[0], np.inf)
    with np.errstate(divide="ignore", invalid="ignore"):
        m = (s[:, 1] - s[:, 0]) / s[:, 0]
    return np.where(s[:, 1] == s[:, 0], 0.0, m)


def bound(T, J, G):
    """The relative error allowed on an fp32 cost: the project's (T J + G) 2^-23 (see the module docstring for why it covers the weights)."""
    return (T * J + G) * 2.0 ** -23
