"""PolicySession(draws=G, select="coherent") on the GPU: the first tick is the medoid session's, later ticks commit the draw
tests/coherent_ref.py names on the draws the session returned; the carried seam, the captured tick, partial resets, subset ticks, the plan
written beside the commit only, everything switched on at once, and ``cli rollout --select coherent``."""

import math

import numpy as np
import pytest
import torch

import coherent_ref
import draws_ref
from test_gpu_session_carry import tiny_model  # noqa: F401 (fixture of calm_model)
from test_gpu_session_slew import AT_LIMIT, CONFIGS, LIMIT, _steps, _ulp, calm_model, v_rad  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu
MARGIN = 1e-3
SB, SG, ST, SJ, SSTEPS, ADV = 2, 4, 10, 20, 3, 5
SCALE = (1.0, 0.6, 1.4, 1.8)   # start noise of a different magnitude per draw: a robot's draws lie at clearly different distances


@pytest.fixture(scope="module")
def tiny256():
    """d = 256, L = 2, T = 10, no images: 13 context rows, the tuned trajectory kernels (as in test_gpu_draws.py)."""
    from test_gpu_session import TINY, _synthetic_model

    params = {**TINY, "hidden_dim": 256, "trajectory_prediction_length": ST}
    return _synthetic_model(params)[0], params


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _feed(sessions, g, S=SB, robots=None, n=ADV):
    q, r = (torch.rand(S, n, SJ, generator=g) - 0.5) * 6, torch.randn(S, n, 4, generator=g)
    for s in sessions:
        s.push_joint_state(q.cuda(), robots=robots)
        s.push_rotation(r.cuda(), robots=robots)


def _noise(g, S=SB):
    return (torch.randn(S, SG, ST, SJ, generator=g) * torch.tensor(SCALE).view(1, SG, 1, 1)).view(S * SG, ST, SJ).cuda()


def _back(model, published):
    """Published radians back in the space the sampler works in, where the distances are measured: (published + pi - mean) / std, float64."""
    return ((published.cpu().double() + math.pi - model.mean.cpu().double()) / model.std.cpu().double()).numpy()


def _setting(s):
    from soccerdiffusion_amd import ops

    w = ops.coherence_weights_host(s.T, s.coherence_decay)
    return w, ops.coherence_lambda(s.contrast, w, s.advance, s.draws, s.T, s.J)


def _check_tick(s, model, draws, index, prev_traj, what, robots=None):
    """The index and the costs of a tick against the float64 reference on the returned draws and the previous tick's trajectory
    (``prev_traj`` (S, T, J) published, NaN rows for a robot without a plan)."""
    w, lam = _setting(s)
    x, prev = _back(model, draws), _back(model, prev_traj)
    S = x.shape[0]
    want_cost = coherent_ref.costs(x, s.draws, prev, s.advance, w, lam)
    margin = coherent_ref.margins(x, s.draws, prev, s.advance, w, lam)
    sel = s.selection()
    assert sel["index"].shape == (S,) and sel["cost"].shape == (S, s.draws) and torch.equal(sel["index"], index)
    err = (np.abs(sel["cost"].double().cpu().numpy() - want_cost) / want_cost).max()
    print(f"{what}: index {index.cpu().tolist()}, fp64 margins {margin}, worst relative cost error {err:.3e} "
          f"(bound {coherent_ref.bound(s.T, s.J, s.draws):.3e})")
    assert (margin > MARGIN).all(), margin
    assert index.cpu().tolist() == coherent_ref.choose(x, s.draws, prev, s.advance, w, lam).tolist()
    assert err <= coherent_ref.bound(s.T, s.J, s.draws)
    return want_cost


@pytest.mark.parametrize("contrast", [0.0, 1.0])
def test_first_tick_is_the_medoids_and_the_second_continues_the_plan(tiny256, contrast):
    from soccerdiffusion_amd.session import PolicySession

    model, _ = tiny256
    kw = dict(num_inference_steps=SSTEPS, batch=SB, draws=SG, advance=ADV)
    c = PolicySession(model, select="coherent", contrast=contrast, **kw)
    m = PolicySession(model, select="medoid", **kw)
    assert bool(torch.isnan(c._plan).all()) and c._plan.shape == (SB, ST, SJ) and m._plan is None
    with pytest.raises(RuntimeError, match="no tick"):
        c.selection()
    with pytest.raises(RuntimeError, match="coherent"):
        m.selection()
    g = torch.Generator().manual_seed(61)
    _feed([c, m], g)
    x_T = _noise(g)
    t1, d1, i1 = c.step(x_T, return_draws=True)
    tm, dm, im = m.step(x_T, return_draws=True)
    assert _same_bits(t1, tm) and _same_bits(d1, dm) and torch.equal(i1, im)       # no plan yet: the medoid session, bit for bit
    none = torch.full((SB, ST, SJ), float("nan"))
    _check_tick(c, model, d1, i1, none, f"contrast {contrast} tick 1 (no plan: medoid scores)")
    assert bool(torch.isfinite(c._plan).all())
    assert np.allclose(c._plan.cpu().double().numpy(), _back(model, t1), rtol=0, atol=1e-4)    # the plan is the chosen draw as sampled
    _feed([c], g)
    t2, d2, i2 = c.step(_noise(g), return_draws=True)
    assert t2.shape == (SB, ST, SJ) and d2.shape == (SB, SG, ST, SJ) and i2.dtype == torch.int32
    for b in range(SB):
        assert _same_bits(t2[b], d2[b, int(i2[b])])                              # return_draws is unchanged
    cost = _check_tick(c, model, d2, i2, t1, f"contrast {contrast} tick 2")
    if contrast == 0.0:   # the only provable claim: from the same state, the committed draw's coherence is the smallest
        assert (cost[np.arange(SB), i2.cpu().numpy()] == cost.min(axis=1)).all()
    _feed([c], g)
    t3, d3, i3 = c.step(_noise(g), return_draws=True)
    _check_tick(c, model, d3, i3, t2, f"contrast {contrast} tick 3")
    c.reset()
    assert bool(torch.isnan(c._plan).all())


def test_carried_seam_stays_bitwise_and_contributes_nothing(tiny256):
    from soccerdiffusion_amd.session import PolicySession

    model, _ = tiny256
    K, A = 2, 4
    s = PolicySession(model, num_inference_steps=SSTEPS, batch=SB, draws=SG, carry=K, advance=A, select="coherent")
    g = torch.Generator().manual_seed(62)
    prev = None
    for tick in range(3):
        _feed([s], g, n=A)
        traj, draws, index = s.step(_noise(g), return_draws=True)
        if prev is not None:
            assert _same_bits(traj[:, :K], prev[:, A:A + K]), tick                 # the seam, as test_gpu_session_carry.py asserts it
            for k in range(SG):
                assert _same_bits(draws[:, k, :K], prev[:, A:A + K]), (tick, k)
            _check_tick(s, model, draws, index, prev, f"carry tick {tick + 1}")
            # the pinned rows equal the plan's rows bit for bit: the cost is that of the rows behind them alone
            w, lam = _setting(s)
            w_behind = w.copy()
            w_behind[:K] = 0.0
            full = coherent_ref.costs(_back(model, draws), SG, _back(model, prev), A, w, lam)
            assert np.array_equal(full, coherent_ref.costs(_back(model, draws), SG, _back(model, prev), A, w_behind, lam))
        prev = traj


def test_graph_equals_eager_with_one_capture(tiny256):
    from soccerdiffusion_amd.session import PolicySession

    model, _ = tiny256
    kw = dict(num_inference_steps=SSTEPS, batch=SB, draws=SG, advance=ADV, select="coherent", contrast=1.0)
    e, c = PolicySession(model, **kw), PolicySession(model, use_graph=True, **kw)
    g = torch.Generator().manual_seed(63)
    graph = None
    for tick in range(3):
        _feed([e, c], g)
        x_T = _noise(g)
        te, de, ie = e.step(x_T, return_draws=True)
        tc, dc, ic = c.step(x_T, return_draws=True)
        assert _same_bits(te, tc) and _same_bits(de, dc) and ie.tolist() == ic.tolist(), tick
        assert _same_bits(e.selection()["cost"], c.selection()["cost"]) and _same_bits(e._plan, c._plan), tick
        graph = graph or c._graph.graph
        assert c._graph.graph is graph, tick                                      # one capture
    # the graphed tick alone - no commit - leaves the plan as it is: a replay whose range guard trips is repeated under the OLD plan
    before = c._plan.clone()
    _feed([c], g)
    chosen = c._graph(_noise(g))[0]
    torch.cuda.synchronize()
    assert _same_bits(before, c._plan) and not _same_bits(chosen, before)


def test_partial_reset_and_subset_tick(tiny256):
    from soccerdiffusion_amd.session import PolicySession

    model, _ = tiny256
    s = PolicySession(model, num_inference_steps=SSTEPS, batch=SB, draws=SG, advance=ADV, select="coherent", use_graph=True)
    g = torch.Generator().manual_seed(64)
    _feed([s], g)
    t1 = s.step(_noise(g))
    graph = s._graph.graph
    s.reset(robots=[1])
    assert bool(torch.isnan(s._plan[1]).all()) and bool(torch.isfinite(s._plan[0]).all())
    _feed([s], g)
    t2, d2, i2 = s.step(_noise(g), return_draws=True)
    assert s._graph is not None and s._graph.graph is graph                       # the tick after a masked reset is still a replay
    prev = t1.clone().cpu()
    prev[1] = float("nan")
    _check_tick(s, model, d2, i2, prev, "after reset(robots=[1])")
    back = _back(model, d2)
    assert (draws_ref.margins(back[1:], SG) > MARGIN).all()
    assert int(i2[1]) == int(draws_ref.medoid(back[1:], SG)[0])                   # robot 1 has no plan: the medoid of its draws
    w, lam = _setting(s)
    assert int(i2[0]) == int(coherent_ref.choose(back[:1], SG, _back(model, t1[:1]), ADV, w, lam)[0])
    # a subset tick moves the ticked robot's plan only, and reads that robot's plan
    plan = s._plan.clone()
    _feed([s], g, S=1, robots=[0])
    t3, d3, i3 = s.step(_noise(g, 1), robots=[0], return_draws=True)
    assert _same_bits(s._plan[1], plan[1]) and not _same_bits(s._plan[0], plan[0])
    _check_tick(s, model, d3, i3, t2[:1], "subset tick of robot 0")
    _feed([s], g, S=1, robots=[1])
    t4, d4, i4 = s.step(_noise(g, 1), robots=[1], return_draws=True)
    _check_tick(s, model, d4, i4, t2[1:], "subset tick of robot 1")


def test_everything_switched_on(calm_model, v_rad):
    """test_gpu_session_slew.py's "all" configuration with select="coherent": three ticks, and the slew and limit properties that file
    checks still hold on the published rows."""
    from test_gpu_session_carry import ADVANCE, B, J, STEPS, T, _push, _sensors

    from soccerdiffusion_amd.session import PolicySession

    kw = {**CONFIGS["all"], "select": "coherent"}
    s = PolicySession(calm_model, num_inference_steps=STEPS, batch=B, seed=3, slew=v_rad, **kw)
    G, carry = kw["draws"], kw["carry"]
    s.hold([0], torch.tensor([0.75]))
    free = [j for j in range(J) if j not in (0, 1)]
    v, ulp = v_rad.double(), _ulp(calm_model, LIMIT)
    lo, hi = np.float32(-LIMIT), np.float32(LIMIT)
    g = torch.Generator().manual_seed(71)
    prev = None
    for tick in range(3):
        _push((s,), *_sensors(g, B))
        traj, draws, index = s.step(torch.randn(B * G, T, J, generator=g).cuda(), return_draws=True)
        assert torch.isfinite(traj).all() and float(traj[:, :, free].abs().max()) <= math.pi
        if prev is not None:
            assert _same_bits(traj[:, :carry], prev[:, ADVANCE:ADVANCE + carry]), tick
        d = _steps(traj)
        excess = float((d[:, :, free] - v[free]).max())
        near = ((d[:, :, free] - v[free]).abs() <= 4 * ulp[free]).float().mean()
        print(f"all + coherent tick {tick}: index {index.tolist()}, worst |step| - v_rad {excess:.3e}, {float(near):.2f} of the pairs within 4 ulp")
        assert excess <= 0, (tick, excess)
        assert float(near) >= AT_LIMIT, (tick, float(near))
        assert bool(((traj[:, :, free] >= lo) & (traj[:, :, free] <= hi)).all())
        assert bool((traj[:, :, 0] == traj[:, :1, 0]).all())
        sel = s.selection()
        assert torch.equal(sel["index"], index) and bool(torch.isfinite(sel["cost"]).all())
        best = sel["cost"].gather(1, index.long().view(B, 1))
        assert bool((best <= sel["cost"]).all())                                  # contrast = 0: the committed draw's coherence is the smallest
        for b in range(B):
            assert _same_bits(traj[b], draws[b, int(index[b])])
        prev = traj
    assert s._graph is not None


def test_cli_rollout_select(tiny256, tmp_path, capsys):
    from soccerdiffusion_amd import cli

    model, params = tiny256
    ckpt, out = str(tmp_path / "c.pt"), str(tmp_path / "r.pt")
    torch.save({"model_state_dict": model.state_dict(), "hyperparams": params}, ckpt)
    base = ["rollout", ckpt, "--synthetic", "2", "--ticks", "3", "--steps", "3", "--draws", "4", "--advance", "5", "-o", out]
    assert cli.main(base + ["--select", "coherent"]) == 0
    saved = torch.load(out, weights_only=True)
    assert saved["select"] == "coherent" and math.isfinite(saved["plan_change_rms"]) and saved["plan_change_rms"] > 0
    assert saved["plan_change_rms"] == pytest.approx(cli.plan_change_rms(saved["trajectories"], 5), rel=1e-12)
    assert "plan_change_rms" in capsys.readouterr().out
    assert cli.main(base) == 0                                                    # either selector reports it whenever ticks overlap
    medoid = torch.load(out, weights_only=True)
    assert medoid["select"] == "medoid" and math.isfinite(medoid["plan_change_rms"])
    assert cli.main(base[:-4] + ["-o", out]) == 0                                 # no overlap: the file of old
    assert "select" not in torch.load(out, weights_only=True)
    with pytest.raises(SystemExit, match="overlap"):
        cli.main(base[:-4] + ["--select", "coherent", "-o", out])
