"""sd_select_coherent / ops.select_coherent on the GPU against tests/coherent_ref.py: costs within the derived bound, the choice in every
context, the bitwise properties (gather, read-only inputs, repeatability, robots, independence of C), NaN plans, the medoid fallback, ties
and zero weights."""

import numpy as np
import pytest
import torch

import coherent_ref
import draws_ref

pytestmark = pytest.mark.gpu
MARGIN = 1e-3   # the project's (test_gpu_draws.py): the fp32 costs carry at most (T J + G) 2^-23 relative error, far below

# (C, G, T, J, S) -> the seed whose float64 margin exceeds MARGIN in every context for every (contrast, decay) below (picked on the CPU)
CASES = {
    (3, 2, 10, 20, 5): 0,      # baseline
    (3, 5, 10, 20, 1): 0,      # odd draw count, nine overlap rows
    (2, 8, 10, 20, 9): 1,      # one overlap row, 20 elements: lanes with nothing to add
    (1, 64, 10, 20, 3): 0,     # the largest G: the whole LDS table
    (2, 5, 3, 7, 1): 0,        # 14 elements, J not a multiple of 4
    (2, 3, 100, 32, 50): 0,    # 1600 elements, 25 per lane
    (2, 1, 10, 20, 5): 0,      # G = 1: index 0
}
CONTRASTS, DECAYS = (0.0, 1.0), (0.5, 1.0)


def _inputs(case, seed=None):
    """Draws at different distances from their context's centre (as test_gpu_draws._medoid_inputs builds them), and a plan whose
    overlapping rows are the centre's plus small noise: prev[:, S + tau] ~ centre[:, tau].  The rows before S are unrelated."""
    Cn, G, T, J, S = case
    g = torch.Generator().manual_seed(9000 + 7 * sum(case) + (CASES[case] if seed is None else seed))
    centre = torch.randn(Cn, 1, T, J, generator=g)
    spread = 0.5 + torch.rand(Cn, G, 1, 1, generator=g)
    x = centre + spread * torch.randn(Cn, G, T, J, generator=g)
    prev = torch.randn(Cn, T, J, generator=g)
    prev[:, S:] = centre[:, 0, :T - S] + 0.1 * torch.randn(Cn, T - S, J, generator=g)
    return x.contiguous(), prev.contiguous()


def _setting(case, contrast, decay):
    from soccerdiffusion_amd import ops

    _, G, T, J, S = case
    w = ops.coherence_weights_host(T, decay)
    return w, ops.coherence_lambda(contrast, w, S, G, T, J)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _rel(got, want):
    want = np.asarray(want, dtype=np.float64)
    return np.abs(got.double().cpu().numpy() - want) / want


@pytest.mark.parametrize("decay", DECAYS)
@pytest.mark.parametrize("contrast", CONTRASTS)
@pytest.mark.parametrize("case", list(CASES), ids=lambda c: "-".join(map(str, c)))
def test_costs_and_choice_equal_the_fp64_reference(case, contrast, decay):
    from soccerdiffusion_amd import ops

    Cn, G, T, J, S = case
    x, prev = _inputs(case)
    w, lam = _setting(case, contrast, decay)
    want_cost = coherent_ref.costs(x.numpy(), G, prev.numpy(), S, w, lam)
    want = coherent_ref.choose(x.numpy(), G, prev.numpy(), S, w, lam)
    margin = coherent_ref.margins(x.numpy(), G, prev.numpy(), S, w, lam)
    assert (margin > MARGIN).all(), margin          # every context, none skipped: the seeds are chosen for it
    assert coherent_ref.has_plan(x.numpy(), G, prev.numpy(), S, w).all()
    xg, pg = x.cuda(), prev.cuda()
    wg = torch.from_numpy(w).cuda()
    keep = [t.clone() for t in (xg, pg, wg)]
    index, chosen, cost = ops.select_coherent(xg, G, pg, S, decay=decay, contrast=contrast, cost=True)
    err = _rel(cost, want_cost).max()
    print(f"select_coherent {case} contrast {contrast} decay {decay}: worst relative cost error {err:.3e} (bound {coherent_ref.bound(T, J, G):.3e}), "
          f"smallest fp64 margin {margin.min():.3e}")
    assert index.dtype == torch.int32 and cost.shape == (Cn, G)
    assert err <= coherent_ref.bound(T, J, G)
    assert index.cpu().tolist() == want.tolist()
    assert torch.equal(_bits(chosen), _bits(torch.stack([xg[c, int(want[c])] for c in range(Cn)])))
    for t, k in zip((xg, pg, wg), keep):          # the inputs are only read
        assert torch.equal(_bits(t), _bits(k))
    # the explicit weights are the default ones; the sampler's flat layout; no gather, no cost; and the same bits a second time
    index2, none, cost2 = ops.select_coherent(xg.view(Cn * G, T, J), G, pg, S, row_weights=wg, contrast=contrast, gather=False, cost=True)
    assert none is None and torch.equal(index, index2) and torch.equal(_bits(cost), _bits(cost2))
    index3, chosen3, no_cost = ops.select_coherent(xg, G, pg, S, decay=decay, contrast=contrast)
    assert no_cost is None and torch.equal(index, index3) and torch.equal(_bits(chosen), _bits(chosen3))
    if G == 1:
        assert index.cpu().tolist() == [0] * Cn


@pytest.mark.parametrize("contrast", CONTRASTS)
def test_robots_reads_the_named_plans(contrast):
    from soccerdiffusion_amd import ops

    case = (3, 5, 10, 20, 1)
    Cn, G, T, J, S = case
    x, prev = _inputs(case)
    xg = x.cuda()
    more = torch.cat([prev, torch.randn(2, T, J, generator=torch.Generator().manual_seed(1))]).cuda()      # five plans, three contexts
    perm = [4, 0, 2]
    a = ops.select_coherent(xg, G, more, S, contrast=contrast, robots=perm, cost=True)
    b = ops.select_coherent(xg, G, more[perm].contiguous(), S, contrast=contrast, cost=True)
    c = ops.select_coherent(xg, G, more, S, contrast=contrast, robots=torch.tensor(perm, dtype=torch.int32, device="cuda"), cost=True)
    for other in (b, c):
        assert torch.equal(a[0], other[0]) and torch.equal(_bits(a[1]), _bits(other[1])) and torch.equal(_bits(a[2]), _bits(other[2]))
    w, lam = _setting(case, contrast, 0.5)
    assert a[0].cpu().tolist() == coherent_ref.choose(x.numpy(), G, more.cpu().numpy(), S, w, lam, robots=perm).tolist()


@pytest.mark.parametrize("contrast", CONTRASTS)
def test_a_context_does_not_depend_on_the_others(contrast):
    from soccerdiffusion_amd import ops

    case = (3, 5, 10, 20, 1)
    _, G, _, _, S = case
    x, prev = _inputs(case)
    xg, pg = x.cuda(), prev.cuda()
    whole = ops.select_coherent(xg, G, pg, S, contrast=contrast, cost=True)
    first = ops.select_coherent(xg[:1].contiguous(), G, pg[:1].contiguous(), S, contrast=contrast, cost=True)
    assert torch.equal(whole[0][:1], first[0]) and torch.equal(_bits(whole[1][:1]), _bits(first[1])) and torch.equal(_bits(whole[2][:1]), _bits(first[2]))


@pytest.mark.parametrize("contrast", CONTRASTS)
def test_nan_rows_of_the_plan_are_left_out(contrast):
    from soccerdiffusion_amd import ops

    case = (2, 8, 10, 20, 3)
    Cn, G, T, J, S = case
    x, prev = _inputs(case, seed=0)
    holed = prev.clone()
    holed[1, S + 1] = float("nan")
    holed[1, S + 4] = float("nan")
    w, lam = _setting(case, contrast, 0.5)
    # the float64 reference with those rows left out: their weights set to zero for context 1 alone
    w_out = w.copy()
    w_out[[1, 4]] = 0.0
    want1 = coherent_ref.costs(x.numpy()[1:], G, prev.numpy()[1:], S, w_out, lam)
    want0 = coherent_ref.costs(x.numpy()[:1], G, prev.numpy()[:1], S, w, lam)
    np.testing.assert_allclose(coherent_ref.costs(x.numpy(), G, holed.numpy(), S, w, lam), np.concatenate([want0, want1]), rtol=1e-13)
    got = ops.select_coherent(x.cuda(), G, holed.cuda(), S, contrast=contrast, cost=True)
    clean = ops.select_coherent(x.cuda(), G, prev.cuda(), S, contrast=contrast, cost=True)
    assert torch.isfinite(got[2]).all()
    assert _rel(got[2][1:], want1).max() <= coherent_ref.bound(T, J, G)
    assert torch.equal(_bits(got[2][0]), _bits(clean[2][0])) and got[0][0] == clean[0][0]      # the other context is untouched
    assert not torch.equal(_bits(got[2][1]), _bits(clean[2][1]))
    margin = coherent_ref.margins(x.numpy(), G, holed.numpy(), S, w, lam)
    assert (margin > MARGIN).all(), margin
    assert got[0].cpu().tolist() == coherent_ref.choose(x.numpy(), G, holed.numpy(), S, w, lam).tolist()


@pytest.mark.parametrize("contrast", [0.0, 1.0, 3.5])
@pytest.mark.parametrize("G", [2, 5, 64])
def test_without_a_plan_the_choice_is_the_medoids(G, contrast):
    from soccerdiffusion_amd import ops

    Cn, T, J, S = 3, 10, 20, 5
    g = torch.Generator().manual_seed(9500 + G)
    x = (torch.randn(Cn, 1, T, J, generator=g) + (0.5 + torch.rand(Cn, G, 1, 1, generator=g)) * torch.randn(Cn, G, T, J, generator=g)).cuda()
    none = torch.full((Cn, T, J), float("nan"), device="cuda")
    want, chosen = ops.select_medoid(x, G)
    index, out, cost = ops.select_coherent(x, G, none, S, contrast=contrast, cost=True)
    assert torch.equal(index, want) and torch.equal(_bits(out), _bits(chosen))
    assert _rel(cost, draws_ref.scores(x.cpu().numpy(), G)).max() <= coherent_ref.bound(T, J, G)
    # a plan outside the overlap, or under zero weights, is no plan either
    early = none.clone()
    early[:, :S] = 1.0
    assert torch.equal(ops.select_coherent(x, G, early, S, contrast=contrast)[0], want)
    plan = torch.randn(Cn, T, J, generator=g).cuda()
    assert torch.equal(ops.select_coherent(x, G, plan, S, row_weights=torch.zeros(T, device="cuda"), contrast=contrast)[0], want)
    # one context with a plan beside two without: those two keep the medoid's index
    mixed = none.clone()
    mixed[1] = plan[1]
    assert torch.equal(ops.select_coherent(x, G, mixed, S, contrast=contrast)[0][[0, 2]], want[[0, 2]])


def test_exact_tie_goes_to_the_lowest_index():
    from soccerdiffusion_amd import ops

    T, J, S = 10, 20, 5
    g = torch.Generator().manual_seed(9600)
    x = 10 * torch.randn(2, 5, T, J, generator=g)
    prev = torch.randn(2, T, J, generator=g)
    x[:, 1, :T - S] = prev[:, S:] + 0.01 * torch.randn(2, T - S, J, generator=g)      # close to the plan: jointly best with its copy
    x[:, 3] = x[:, 1]
    for contrast in CONTRASTS:
        w, lam = _setting((2, 5, T, J, S), contrast, 0.5)
        s = coherent_ref.costs(x.numpy(), 5, prev.numpy(), S, w, lam)
        assert (s[:, 1] == s[:, 3]).all() and (np.delete(s, [1, 3], axis=1).min(axis=1) > s[:, 1] * (1 + MARGIN)).all()
        index, chosen, cost = ops.select_coherent(x.cuda(), 5, prev.cuda(), S, contrast=contrast, cost=True)
        assert index.cpu().tolist() == [1, 1] and torch.equal(chosen.cpu(), x[:, 1])
        assert torch.equal(_bits(cost[:, 1]), _bits(cost[:, 3]))


@pytest.mark.parametrize("case", list(CASES), ids=lambda c: "-".join(map(str, c)))
def test_the_chosen_draw_has_the_smallest_coherence(case):
    """contrast = 0, on the kernel's own numbers: no draw of a context has a smaller cost than the chosen one, and no earlier draw an equal one."""
    from soccerdiffusion_amd import ops

    Cn, G, _, _, S = case
    x, prev = _inputs(case)
    index, _, cost = ops.select_coherent(x.cuda(), G, prev.cuda(), S, contrast=0.0, cost=True)
    cost, index = cost.cpu(), index.cpu().long()
    best = cost.gather(1, index.view(Cn, 1))
    assert (best <= cost).all()
    for c in range(Cn):
        assert (cost[c, :int(index[c])] > best[c]).all()


@pytest.mark.parametrize("contrast", CONTRASTS)
def test_a_zero_weight_row_changes_no_bit(contrast):
    from soccerdiffusion_amd import ops

    case = (3, 5, 10, 20, 1)
    _, G, T, _, S = case
    x, prev = _inputs(case)
    w = torch.tensor([0.5 ** t for t in range(T)])
    w[2] = 0.0
    wild = prev.clone()
    wild[:, S + 2] = torch.tensor([1e30, -3e38, float("inf"), 1e-30] * 5)
    a = ops.select_coherent(x.cuda(), G, prev.cuda(), S, row_weights=w.cuda(), contrast=contrast, cost=True)
    b = ops.select_coherent(x.cuda(), G, wild.cuda(), S, row_weights=w.cuda(), contrast=contrast, cost=True)
    assert torch.isfinite(b[2]).all()
    assert torch.equal(a[0], b[0]) and torch.equal(_bits(a[1]), _bits(b[1])) and torch.equal(_bits(a[2]), _bits(b[2]))
