"""Slew limits of the policy session on the GPU (``PolicySession(slew=...)``: sd_session_slew, sd_session_anchor, the slewed rollout
underneath): consecutive published rows differ by at most the given radians per row, evaluated in fp64 - inside a tick and from a tick's
last committed row to the next tick's first - with carried rows, a held joint, several draws, subset ticks, the captured tick, the
multistep solver and joint limits; a share of the pairs sits at the limit; ``reset(robots=...)`` frees the first row of the robots reset;
``set_slew`` between ticks without a new capture; ``cli evaluate --slew``."""

import json
import math

import numpy as np
import pytest
import torch

from test_gpu_session import _same_bits
from test_gpu_session_carry import ADVANCE, B, CARRY, J, STEPS, T, TINY10, _push, _sensors, tiny_model  # noqa: F401 (fixture)

pytestmark = pytest.mark.gpu
TICKS = 3
LIMIT = 1.5                      # radians as published: the calm model publishes beyond it, so the box binds as well
AT_LIMIT, BINDING = 0.10, 0.30   # the share of pairs within 4 ulp of the limit; the share an unlimited session has above it


def _steps(traj, prev_last=None):
    """|r[t + 1] - r[t]| of published rows (S, T, J) in fp64 (the difference of two fp32 values is exact there); with ``prev_last`` (S, J)
    the step from it to row 0 comes first."""
    r = traj.cpu().double()
    if prev_last is not None:
        r = torch.cat([prev_last.cpu().double().unsqueeze(1), r], 1)
    return (r[:, 1:] - r[:, :-1]).abs()


@pytest.fixture(scope="module")
def calm_model(tiny_model):
    """The tiny model with a normaliser that publishes inside +- pi, what the margin's derivation assumes of a session without
    ``limits``: mean pi, std 0.2 on every joint (the random weights' samples reach |x| ~ 12: published = 0.2 x)."""
    import copy

    m = copy.deepcopy(tiny_model)
    with torch.no_grad():
        m.mean.fill_(math.pi)
        m.std.fill_(0.2)
    return m


@pytest.fixture(scope="module")
def v_rad(calm_model):
    """Radians per row that bind: per joint the lower quartile of the |step| that three unlimited ticks publish; joint 1 unlimited."""
    from soccerdiffusion_amd.session import PolicySession

    tiny_model = calm_model
    s = PolicySession(tiny_model, num_inference_steps=STEPS, batch=B, seed=3)
    g = torch.Generator().manual_seed(70)
    steps, last = [], None
    for _ in range(TICKS):
        _push((s,), *_sensors(g, B))
        traj = s.step(torch.randn(B, T, J, generator=g).cuda())
        steps.append(_steps(traj, last).reshape(-1, J))
        last = traj[:, -1]
    d = torch.cat(steps)
    v = d.quantile(0.25, dim=0).float()
    v[1] = float("inf")
    limited = [j for j in range(J) if j != 1]
    share = float((d[:, limited] > v[limited].double()).float().mean())
    print(f"without slew: {share:.2f} of the pairs exceed v_rad")
    assert share >= BINDING                                  # the session WITHOUT slew exceeds it on at least 30 % of pairs
    return v.contiguous()


def _ulp(model, bound=math.pi):
    """One ulp of the commit's largest intermediate, per joint: |published| + pi + |mean| with |published| <= ``bound`` - the limits
    where they are given, pi otherwise (the unit tests/test_gpu_session_limits.py measures sd_session_limits' gap in)."""
    m = model.mean.detach().cpu().numpy().astype(np.float32)
    return torch.from_numpy(np.spacing(np.float32(bound + math.pi) + np.abs(m)).astype(np.float64))


CONFIGS = {
    "plain": dict(),
    "carry": dict(carry=CARRY, advance=ADVANCE),
    "hold": dict(holds=True),
    "draws": dict(draws=4, select="medoid"),
    "robots": dict(robots=True),
    "graph": dict(use_graph=True),
    "multistep": dict(solver="multistep"),
    "limits": dict(limits=LIMIT),
    "all": dict(carry=CARRY, advance=ADVANCE, holds=True, draws=4, select="medoid", use_graph=True, solver="multistep", limits=LIMIT),
}


@pytest.mark.parametrize("name", list(CONFIGS))
def test_consecutive_published_rows_differ_by_at_most_v_rad(calm_model, v_rad, name):
    from soccerdiffusion_amd.session import PolicySession

    tiny_model = calm_model

    kw = dict(CONFIGS[name])
    subset = [0, 2] if kw.pop("robots", False) else None
    s = PolicySession(tiny_model, num_inference_steps=STEPS, batch=B, seed=3, slew=v_rad, **kw)
    G, carry = kw.get("draws", 1), kw.get("carry", 0)
    free = [j for j in range(J) if j != 1]
    if kw.get("holds"):      # joint 0 held: it keeps the hold's value (constant over the rows: no step at all)
        s.hold([0], torch.tensor([0.75]))
        free = free[1:]
    v, ulp = v_rad.double(), _ulp(tiny_model, kw.get("limits", math.pi))
    if "limits" in kw:
        lo, hi = np.float32(-LIMIT), np.float32(LIMIT)
    g = torch.Generator().manual_seed(71)
    last = None
    for tick in range(TICKS):
        S = B if subset is None else len(subset)
        _push((s,), *_sensors(g, S), robots=subset)
        traj = s.step(torch.randn(S * G, T, J, generator=g).cuda(), robots=subset)
        assert torch.isfinite(traj).all() and float(traj[:, :, free].abs().max()) <= math.pi      # inside what the margin assumes
        if carry and last is not None:
            assert _same_bits(traj[:, :carry], prev[:, ADVANCE:ADVANCE + carry]), (name, tick)      # the seam stays exact
        d = _steps(traj, None if carry else last)            # with carry row 0 is pinned to the previous tick: the seam is inside it
        excess = float((d[:, :, free] - v[free]).max())
        near = ((d[:, :, free] - v[free]).abs() <= 4 * ulp[free]).float().mean()
        print(f"{name} tick {tick}: worst |step| - v_rad {excess:.3e}, {float(near):.2f} of the pairs within 4 ulp of the limit")
        assert excess <= 0, (name, tick, excess)
        assert float(near) >= AT_LIMIT, (name, tick, float(near))
        if "limits" in kw:
            assert bool(((traj[:, :, free] >= lo) & (traj[:, :, free] <= hi)).all())
        if kw.get("holds"):
            assert bool((traj[:, :, 0] == traj[:, :1, 0]).all())
        prev = traj
        last = traj[:, (s.advance if carry else T) - 1]       # the last committed row
    if kw.get("use_graph"):
        assert s._graph is not None


def test_reset_of_one_robot_frees_its_first_row_only(calm_model, v_rad):
    from soccerdiffusion_amd.session import PolicySession

    tiny_model = calm_model

    s = PolicySession(tiny_model, num_inference_steps=STEPS, batch=B, seed=3, slew=v_rad)
    assert bool(torch.isnan(s._anchor).all())
    g = torch.Generator().manual_seed(72)
    _push((s,), *_sensors(g, B))
    first = s.step(torch.randn(B, T, J, generator=g).cuda())
    assert bool(torch.isfinite(s._anchor[:, :J]).all()) and bool(torch.isnan(s._anchor[:, J:]).all())
    s.reset(robots=[0])
    assert bool(torch.isnan(s._anchor[0]).all()) and bool(torch.isfinite(s._anchor[1:, :J]).all())
    _push((s,), *_sensors(g, B))
    second = s.step(torch.randn(B, T, J, generator=g).cuda())
    free = [j for j in range(J) if j != 1]
    seam = (second[:, 0].cpu().double() - first[:, -1].cpu().double()).abs()[:, free] - v_rad.double()[free]
    assert bool((seam[1:] <= 0).all()) and bool((seam[0] > 0).any())       # robot 1 and 2 are anchored, robot 0's first row is free
    s.reset()
    assert bool(torch.isnan(s._anchor).all())


def test_set_slew_takes_effect_without_a_new_capture(calm_model, v_rad):
    from soccerdiffusion_amd.session import PolicySession

    tiny_model = calm_model

    graphed = PolicySession(tiny_model, num_inference_steps=STEPS, batch=B, seed=3, slew=v_rad, use_graph=True)
    eager = PolicySession(tiny_model, num_inference_steps=STEPS, batch=B, seed=3, slew=v_rad)
    g = torch.Generator().manual_seed(73)
    array, graph = graphed._slew_v.data_ptr(), None
    for tick, new in enumerate((None, {0: float(v_rad[0]) / 2}, 1e9)):
        want = v_rad.double()
        if isinstance(new, dict):
            want = torch.full((J,), float("inf"), dtype=torch.float64)
            want[0] = new[0]
        elif new is not None:
            want = torch.full((J,), new, dtype=torch.float64)
        if new is not None:
            for s in (graphed, eager):
                s.set_slew(new)
        _push((graphed, eager), *_sensors(g, B))
        x_T = torch.randn(B, T, J, generator=g).cuda()
        a, b = graphed.step(x_T), eager.step(x_T)
        assert _same_bits(a, b) and bool((_steps(a) <= want).all()), tick
        graph = graph or graphed._graph.graph
        assert graphed._graph.graph is graph and graphed._slew_v.data_ptr() == array
    with pytest.raises(RuntimeError, match="without slew"):
        PolicySession(tiny_model, num_inference_steps=STEPS, batch=B).set_slew(1.0)
    with pytest.raises(ValueError, match="margin"):
        eager.set_slew(1e-7)
    with pytest.raises(ValueError, match="negative"):
        eager.set_slew(-1.0)
    # a session without slew is the session of before
    plain = PolicySession(tiny_model, num_inference_steps=STEPS, batch=B, seed=3)
    assert plain._slew_v is None and plain._anchor is None and plain._lim() == {}


def test_session_slew_matches_its_host_model():
    from soccerdiffusion_amd import ops

    Jn = 32
    g = torch.Generator().manual_seed(74)
    mean, std = (torch.rand(Jn, generator=g) * 6).float(), (torch.rand(Jn, generator=g) * 2 + 0.01).float()
    v = (torch.rand(Jn, generator=g) * 0.5 + 1e-3).float()
    v[3] = float("inf")
    bound = np.full(Jn, math.pi, dtype=np.float32)
    out = ops.session_slew(ops.joint_slew({}, J=Jn, device="cuda"), v.numpy(), bound, mean.cuda(), std.cuda(), Jn).cpu().numpy()
    want = ops.session_slew_host(v.numpy(), bound, mean.numpy(), std.numpy())
    assert out[3] == np.inf and np.array_equal(np.delete(out, 3), np.delete(want, 3))


# ---- the command line -------------------------------------------------------------------------------------------------------------------
def test_cli_evaluate_reports_max_step_by_joint_within_slew(tiny_model, tmp_path, capsys):
    from soccerdiffusion_amd import cli

    ckpt = str(tmp_path / "c.pt")
    torch.save({"model_state_dict": tiny_model.state_dict(), "hyperparams": TINY10}, ckpt)
    capsys.readouterr()
    # (--clip: the margin of the conversion is derived for denormalised values inside a bound, and this model's random weights leave [0, 2 pi))
    assert cli.main(["evaluate", ckpt, "--synthetic", "8", "--all", "--steps", "4", "--clip", "7.0"]) == 0
    free = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert "slew" not in free and len(free["max_step_by_joint"]) == J
    v = float(np.float32(min(free["max_step_by_joint"]) / 4))
    assert cli.main(["evaluate", ckpt, "--synthetic", "8", "--all", "--steps", "4", "--clip", "7.0", "--slew", repr(v)]) == 0
    rep = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    print(f"cli evaluate --slew {v}: max_step_by_joint - v in [{min(rep['max_step_by_joint']) - v:.3e}, {max(rep['max_step_by_joint']) - v:.3e}]")
    assert rep["slew"] == [v] * J and max(rep["max_step_by_joint"]) <= v          # the limit held: no slack
    assert max(rep["max_step_by_joint"]) >= v - 1e-5 and math.isfinite(rep["rmse_medoid"])   # ... and it binds
    # rollout: radians per row as published, exactly
    out = str(tmp_path / "r.pt")
    assert cli.main(["rollout", ckpt, "--synthetic", "3", "--ticks", "2", "--steps", "4", "--seed", "5", "--slew", "0.05", "-o", out]) == 0
    saved = torch.load(out, weights_only=True)
    traj = saved["trajectories"]
    assert saved["slew"] == 0.05 and traj.shape == (2, 3, T, J)
    flat = torch.cat([traj[0], traj[1]], 1)                  # the two ticks of a robot back to back: the seam is a pair like any other
    assert float(_steps(flat).max()) <= float(np.float32(0.05))
    with pytest.raises(SystemExit, match="joint indices"):
        cli.main(["sample", ckpt, "--synthetic", "8", "--slew", f"{J}=0.1"])
