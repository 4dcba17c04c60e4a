"""The policy session on a DISTILLED decoder on the GPU (``PolicySession(distilled=True, limits=, slew=, holds=, draws=, select=,
use_graph=)``: model.sample_direct - the direct launch - under the session's device-side pieces as they are): eager ticks against
replayed ones bit for bit, the published radians inside the limits, consecutive published rows within the slew limit in fp64 - from the
last committed row too - the held joints exact, the selection the argmin of its costs, the session without options as it was, and carry
still refused.  hidden_dim 64 runs the eps launches and the projection kernel, 128 the generic family's direct twin."""

import math

import numpy as np
import pytest
import torch

from test_gpu_session import TINY, _same_bits, _synthetic_model

pytestmark = pytest.mark.gpu
B, T, J, G, ADVANCE = 3, 10, 20, 4, 5
JOINTS = [0, 1]                    # held for every robot
V = torch.tensor([0.3, -0.7])      # radians as published
FREE = [j for j in range(J) if j not in JOINTS]
_cache: dict = {}


def _model(d):
    """Joint states + IMU, no images, no action history, no game state; a normaliser that publishes inside +- pi (mean pi, std 0.2), what
    the slew margin's derivation assumes."""
    if d not in _cache:
        params = {**TINY, "hidden_dim": d, "trajectory_prediction_length": T, "use_action_history": False, "use_gamestate": False,
                  "distilled_decoder": True}
        m = _synthetic_model(params)[0]
        with torch.no_grad():
            m.mean.fill_(math.pi)
            m.std.fill_(0.2)
        _cache[d] = (m, params)
    return _cache[d]


def _sensors(g, S, n=ADVANCE):
    return (torch.rand(S, n, J, generator=g) - 0.5) * 6, torch.randn(S, n, 4, generator=g)


def _push(sessions, q, r, robots=None):
    for s in sessions:
        s.push_joint_state(q.cuda(), robots=robots)
        s.push_rotation(r.cuda(), robots=robots)


def _constraints(d):
    """Limits and slew limits in radians that bind, from what the session WITHOUT options publishes: per joint the 25 % / 75 % quantiles,
    and the lower quartile of |step|."""
    from soccerdiffusion_amd.session import PolicySession

    key = ("c", d)
    if key not in _cache:
        m, params = _model(d)
        s = PolicySession(m, batch=B, hyperparams=params, seed=3)
        g = torch.Generator().manual_seed(80)
        rows = []
        for _ in range(3):
            _push((s,), *_sensors(g, B, T))
            rows.append(s.step(torch.randn(B, T, J, generator=g).cuda()).cpu().double())
        flat = torch.cat(rows).reshape(-1, J)
        lo, hi = flat.quantile(0.25, dim=0).float(), flat.quantile(0.75, dim=0).float()
        steps = torch.cat([(r[:, 1:] - r[:, :-1]).abs().reshape(-1, J) for r in rows])
        _cache[key] = (lo.contiguous(), hi.contiguous(), steps.quantile(0.25, dim=0).float().contiguous())
    return _cache[key]


@pytest.mark.parametrize("d", [64, 128])
def test_default_distilled_session_is_forward_with_context_and_the_commit(d):
    from soccerdiffusion_amd.session import PolicySession

    m, params = _model(d)
    s = PolicySession(m, batch=B, hyperparams=params)
    assert s.distilled and not s._direct and s._lim() == {} and s._limits is None and s._plan is None
    g = torch.Generator().manual_seed(81)
    for tick in range(2):
        _push((s,), *_sensors(g, B, T))
        x_T = torch.randn(B, T, J, generator=g).cuda()
        with torch.no_grad():
            x = m.forward_with_context(s._context(), x_T, torch.zeros(B, dtype=torch.int64, device="cuda"))
        assert _same_bits(s.step(x_T), (x * m.std + m.mean) - math.pi), tick
    plain = PolicySession(m, batch=B, hyperparams=params, direct=True)      # the flag alone changes no launch either
    assert plain.direct and not plain._direct
    for bad in (dict(carry=1), dict(solver="multistep"), dict(limits=1.0, reproject=True)):      # refused with the flag as without it
        with pytest.raises(ValueError, match="distilled"):
            PolicySession(m, batch=B, hyperparams=params, direct=True, **bad)
    for old in (dict(limits=1.0), dict(slew=0.1), dict(holds=True), dict(draws=2), dict(use_graph=True)):   # without it: the session of before
        with pytest.raises(ValueError, match="direct=True"):
            PolicySession(m, batch=B, hyperparams=params, **old)
    with pytest.raises(ValueError, match="direct"):
        PolicySession(m, batch=B, hyperparams={**params, "distilled_decoder": False}, direct=True)


@pytest.mark.parametrize("d", [64, 128])
def test_eager_and_replayed_ticks_under_every_option(d):
    from soccerdiffusion_amd import _lib
    from soccerdiffusion_amd.session import PolicySession

    m, params = _model(d)
    Mc = 2 * (20 // 5)
    assert _lib.sampler_route(d, 4, T, Mc, J, 2, B * G, 3) == ("CHAINS_F32" if d == 64 else "TRAJ_GENERIC")
    lo, hi, v_rad = _constraints(d)
    kw = dict(batch=B, hyperparams=params, seed=3, direct=True, limits=(lo, hi), slew=v_rad, holds=True, draws=G, select="coherent", advance=ADVANCE)
    eager, graphed = PolicySession(m, **kw), PolicySession(m, use_graph=True, **kw)
    assert eager._direct and graphed._direct and eager.distilled
    for s in (eager, graphed):
        s.hold(JOINTS, V)
    mean, std = m.mean.cpu()[JOINTS], m.std.cpu()[JOINTS]
    held = ((((V + math.pi) - mean) / std) * std + mean) - math.pi      # the hold's radians as the commit publishes them
    g = torch.Generator().manual_seed(82)
    last = torch.full((B, J), float("nan"), dtype=torch.float64)          # the robots' last committed rows
    graph, moved = None, []
    for tick, robots in enumerate((None, None, None, [0, 2])):
        if tick == 2:
            for s in (eager, graphed):
                s.reset(robots=[1])
            last[1] = float("nan")                                        # the limit does not reach across the reset
        idx = list(range(B)) if robots is None else robots
        S = len(idx)
        _push((eager, graphed), *_sensors(g, S), robots=robots)
        x_T = torch.randn(S * G, T, J, generator=g).cuda()
        a, b = eager.step(x_T, robots=robots), graphed.step(x_T, robots=robots)
        assert _same_bits(a, b), tick
        sa, sb = eager.selection(), graphed.selection()
        assert torch.equal(sa["index"], sb["index"]) and _same_bits(sa["cost"], sb["cost"]), tick
        assert torch.equal(sa["cost"].argmin(1).int().cpu(), sa["index"].cpu()), tick            # the committed draw has the lowest cost
        if robots is None:
            graph = graph or graphed._graph.graph
            assert graphed._graph.graph is graph                          # captured once; reset(robots=...) keeps the capture
        pub = a.cpu()
        assert torch.isfinite(pub).all()
        # limits: every free published element inside the given radians
        assert bool(((pub[:, :, FREE] >= lo[FREE]) & (pub[:, :, FREE] <= hi[FREE])).all()), tick
        # holds: the held joints are the hold's radians, every row, every robot ticked
        assert _same_bits(pub[:, :, JOINTS], held.expand(S, T, 2).contiguous()), tick
        # slew: consecutive published rows, and the last committed row to this tick's first, in fp64 (exact on fp32 values)
        r = torch.cat([last[idx].unsqueeze(1), pub.double()], 1)
        step = (r[:, 1:] - r[:, :-1]).abs()[:, :, FREE]
        step = torch.where(torch.isnan(step), torch.zeros((), dtype=torch.float64), step)        # no anchor: row 0 is free
        excess = float((step - v_rad.double()[FREE]).max())
        moved.append(float(((step - v_rad.double()[FREE]).abs() <= 1e-5).double().mean()))
        print(f"d {d} tick {tick} robots {robots}: worst |step| - v_rad {excess:.3e}, {moved[-1]:.2f} of the pairs at the limit")
        assert excess <= 0, (tick, excess)
        last[idx] = pub[:, ADVANCE - 1].double()
    assert max(moved) > 0.05                                              # the limit binds: the case tests something
    # set_limits / set_slew / release keep the capture and take effect in both
    for s in (eager, graphed):
        s.set_limits(float(hi.abs().max()) * 4)
        s.set_slew(1e9)
        s.release()
    _push((eager, graphed), *_sensors(g, B))
    x_T = torch.randn(B * G, T, J, generator=g).cuda()
    a, b = eager.step(x_T), graphed.step(x_T)
    assert _same_bits(a, b) and graphed._graph.graph is graph
    assert not _same_bits(a.cpu()[:, :, JOINTS], held.expand(B, T, 2).contiguous())


def test_cli_on_a_distilled_checkpoint(tmp_path, capsys):
    """sample, rollout and evaluate take --clip, --slew, --hold, --draws and --select on a distilled checkpoint; --carry, --solver multistep
    and --reproject exit with a message."""
    import json

    from soccerdiffusion_amd import cli

    m, params = _model(128)
    ckpt = str(tmp_path / "student.pt")
    torch.save({"model_state_dict": m.state_dict(), "hyperparams": params}, ckpt)
    out = str(tmp_path / "s.pt")
    assert cli.main(["sample", ckpt, "--synthetic", "6", "--num_samples", "3", "--draws", "4", "--clip", "3.5", "--slew", "0.05", "--hold", "0=3.3", "-o", out]) == 0
    saved = torch.load(out, weights_only=True)
    traj = saved["trajectories"]
    assert tuple(traj.shape) == (3, G, T, J) and saved["draws"] == G and saved["medoid"].shape == (3,)
    assert float(traj[..., 1:].abs().max()) <= 3.5 * (1 + 1e-6)          # (the file's space: x * std + mean rounds once more)
    assert bool((traj[..., 0] == traj[0, 0, 0, 0]).all()) and abs(float(traj[0, 0, 0, 0]) - 3.3) < 1e-6
    assert float((traj[:, :, 1:, 1:] - traj[:, :, :-1, 1:]).double().abs().max()) <= float(np.float32(0.05))
    assert not torch.equal(traj[:, 0], traj[:, 1])                       # G noises: G trajectories
    out = str(tmp_path / "r.pt")
    assert cli.main(["rollout", ckpt, "--synthetic", "3", "--ticks", "3", "--seed", "5", "--slew", "0.05", "--clip", "1.0", "--draws", "4", "--select", "coherent",
                     "--advance", "5", "--hold", "0=0.25", "-o", out]) == 0
    saved = torch.load(out, weights_only=True)
    pub = saved["trajectories"]
    assert pub.shape == (3, 3, T, J) and saved["select"] == "coherent" and float(pub.abs().max()) <= 1.0
    flat = torch.cat([pub[k][:, :ADVANCE] for k in range(3)], 1)[:, :, 1:]   # the committed rows of a robot back to back
    assert float((flat[:, 1:] - flat[:, :-1]).double().abs().max()) <= float(np.float32(0.05))
    capsys.readouterr()
    assert cli.main(["evaluate", ckpt, "--synthetic", "8", "--all", "--draws", "2", "--clip", "7.0", "--slew", "0.04"]) == 0
    rep = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    v = float(np.float32(0.04))                                          # (the report quotes the fp32 value the sampler was given)
    assert rep["val_loss"] is None and rep["slew"] == [v] * J and max(rep["max_step_by_joint"]) <= v
    for bad, what in ((["--carry", "2"], "--carry"), (["--solver", "multistep"], "--solver"), (["--clip", "1.0", "--reproject"], "--reproject")):
        with pytest.raises(SystemExit, match=what):
            cli.main(["rollout", ckpt, "--synthetic", "2", "--ticks", "1", *bad])
    with pytest.raises(SystemExit, match="--reproject"):
        cli.main(["sample", ckpt, "--synthetic", "4", "--clip", "1.0", "--reproject"])
    with pytest.raises(SystemExit, match="--solver"):
        cli.main(["evaluate", ckpt, "--synthetic", "4", "--all", "--solver", "multistep"])
