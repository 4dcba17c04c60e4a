"""Joint limits of the policy session on the GPU (``PolicySession(limits=...)``: sd_session_limits, the limited rollout underneath): every
published value inside the given radians bit for bit - with carried rows, a held joint, several draws, subset ticks and the captured tick -
the carry seam, ``set_limits`` between ticks without a new capture, sd_session_limits' bounds under both roundings of the commit's
expression, and the session without ``limits`` as it was."""

import math

import numpy as np
import pytest
import torch

from test_gpu_session import _same_bits
from test_gpu_session_carry import ADVANCE, B, CARRY, J, STEPS, T, _push, _sensors, tiny_model  # noqa: F401 (fixture)

pytestmark = pytest.mark.gpu
INF = float("inf")
TICKS = 3


@pytest.fixture(scope="module")
def radians(tiny_model):
    """Limits in radians as published that clamp: per joint the 30 % and 70 % quantiles of what three unlimited ticks publish; joint 1
    unlimited, joint 2 without a lower bound."""
    from soccerdiffusion_amd.session import PolicySession

    s = PolicySession(tiny_model, num_inference_steps=STEPS, batch=B, seed=3)
    g = torch.Generator().manual_seed(60)
    out = []
    for _ in range(TICKS):
        _push((s,), *_sensors(g, B))
        out.append(s.step(torch.randn(B, T, J, generator=g).cuda()).cpu())
    v = torch.cat(out).reshape(-1, J)
    lo, hi = v.quantile(0.3, dim=0), v.quantile(0.7, dim=0)
    lo[1], hi[1] = -INF, INF
    lo[2] = -INF
    return lo.contiguous(), hi.contiguous()


def _inside(traj, lo, hi, joints=None):
    t = traj.reshape(-1, J).cpu()
    ok = (t >= lo) & (t <= hi)
    return bool(ok.all() if joints is None else ok[:, joints].all())


def _at_a_limit(traj, lo, hi):
    t = traj.reshape(-1, traj.shape[-1]).cpu()
    return float(((t == lo) | (t == hi)).float().mean())


CONFIGS = {
    "plain": dict(),
    "reproject": dict(reproject=True),
    "carry": dict(carry=CARRY, advance=ADVANCE),
    "hold": dict(holds=True),
    "draws": dict(draws=4, select="medoid"),
    "graph": dict(use_graph=True),
    "multistep": dict(solver="multistep"),
    "all": dict(carry=CARRY, advance=ADVANCE, holds=True, draws=4, select="medoid", use_graph=True, solver="multistep"),
}


@pytest.mark.parametrize("name", list(CONFIGS))
def test_every_published_value_lies_inside_the_limits(tiny_model, radians, name):
    from soccerdiffusion_amd.session import PolicySession

    kw = CONFIGS[name]
    lo, hi = radians
    s = PolicySession(tiny_model, num_inference_steps=STEPS, batch=B, seed=3, limits=(lo, hi), **kw)
    G, carry = kw.get("draws", 1), kw.get("carry", 0)
    free = list(range(J))
    if kw.get("holds"):      # joint 0 held outside its limits: it keeps the hold's value, every other joint its limits
        held_at = float(hi[0]) + 0.5
        s.hold([0], torch.tensor([held_at]))
        free = free[1:]
    g = torch.Generator().manual_seed(61)
    prev = None
    for tick in range(TICKS):
        _push((s,), *_sensors(g, B))
        traj, draws, index = s.step(torch.randn(B * G, T, J, generator=g).cuda(), return_draws=True)
        assert torch.isfinite(traj).all()
        assert _inside(traj, lo, hi, free), (name, tick)
        assert _inside(draws, lo, hi, free), (name, tick)                      # every draw, not only the committed one
        share = _at_a_limit(traj[:, :, free], lo[free], hi[free])
        print(f"{name} tick {tick}: {share:.2f} of the published free elements equal a limit")
        assert share > 0.05, (name, tick)                                       # the limits bind: a clamped element equals its limit
        if kw.get("holds"):
            assert not _inside(traj, lo, hi, [0]) and (traj[:, :, 0] > hi[0]).all()
        if carry and prev is not None:
            assert _same_bits(traj[:, :carry], prev[:, ADVANCE:ADVANCE + carry]), (name, tick)      # the seam stays exact
            assert not _same_bits(traj[:, carry], prev[:, ADVANCE + carry])
        prev = traj
    # a subset tick, eager on the same rings
    _push((s,), *_sensors(g, 2), robots=[0, 2])
    sub = s.step(torch.randn(2 * G, T, J, generator=g).cuda(), robots=[0, 2])
    assert sub.shape == (2, T, J) and _inside(sub, lo, hi, free), name
    if kw.get("use_graph"):
        assert s._graph is not None


def test_set_limits_takes_effect_without_a_new_capture(tiny_model, radians):
    from soccerdiffusion_amd.session import PolicySession

    lo, hi = radians
    graphed = PolicySession(tiny_model, num_inference_steps=STEPS, batch=B, seed=3, limits=(lo, hi), use_graph=True)
    eager = PolicySession(tiny_model, num_inference_steps=STEPS, batch=B, seed=3, limits=(lo, hi))
    g = torch.Generator().manual_seed(62)
    arrays = tuple(t.data_ptr() for t in graphed._limits)
    graph = None
    mid = (lo[0] + hi[0]) / 2
    for tick, new in enumerate((None, {0: (float(lo[0]), float(mid))}, 1e9)):
        want_lo, want_hi = lo, hi
        if isinstance(new, dict):
            want_lo, want_hi = torch.full((J,), -INF), torch.full((J,), INF)
            want_lo[0], want_hi[0] = lo[0], mid
        elif new is not None:
            want_lo, want_hi = torch.full((J,), -new), torch.full((J,), new)
        if new is not None:
            for s in (graphed, eager):
                s.set_limits(new)
        _push((graphed, eager), *_sensors(g, B))
        x_T = torch.randn(B, T, J, generator=g).cuda()
        a, b = graphed.step(x_T), eager.step(x_T)
        assert _same_bits(a, b) and _inside(a, want_lo, want_hi), tick
        if tick == 1:
            assert not _inside(a, lo, hi) and _at_a_limit(a[:, :, :1], want_lo[:1], want_hi[:1]) > 0.05      # only joint 0 is limited now
        graph = graph or graphed._graph.graph
        assert graphed._graph.graph is graph and tuple(t.data_ptr() for t in graphed._limits) == arrays
    with pytest.raises(RuntimeError, match="without limits"):
        PolicySession(tiny_model, num_inference_steps=STEPS, batch=B).set_limits(1.0)
    with pytest.raises(ValueError, match="lo"):
        eager.set_limits([1.0] * J, [0.0] * J)


def test_a_session_without_limits_is_the_session_of_before(tiny_model):
    from soccerdiffusion_amd.session import PolicySession

    for kw in (dict(), dict(carry=CARRY, advance=ADVANCE), dict(use_graph=True)):
        a = PolicySession(tiny_model, num_inference_steps=STEPS, batch=B, seed=3, **kw)
        b = PolicySession(tiny_model, num_inference_steps=STEPS, batch=B, seed=3, limits=None, **kw)
        assert a._limits is None and b._limits is None and b._lim() == {}
        g = torch.Generator().manual_seed(63)
        for tick in range(2):
            _push((a, b), *_sensors(g, B))
            x_T = torch.randn(B, T, J, generator=g).cuda()
            assert _same_bits(a.step(x_T), b.step(x_T)), (kw, tick)


def test_session_limits_bounds_hold_under_both_roundings_of_the_commit():
    """sd_session_limits on random means, stds (small ones too: many normalised values per published one) and limits, checked on the host:
    fma(x, std, mean) - pi (the product exact in fp64, one rounding to fp32) and (x * std + mean) - pi, in fp32."""
    from soccerdiffusion_amd import ops

    Jn = 32
    g = torch.Generator().manual_seed(64)
    pi32 = np.float32(math.pi)
    for scale in (1.0, 0.05, 7.0):
        mean = (torch.rand(Jn, generator=g) * 6).float()
        std = (torch.rand(Jn, generator=g) * scale + 0.01 * scale).float()
        lo = ((torch.rand(Jn, generator=g) - 0.5) * 6).float()
        hi = lo + torch.rand(Jn, generator=g) * 2 + 1e-3
        lo[3], hi[4] = -INF, INF
        lim = ops.joint_limits({}, J=Jn, device="cuda")
        ops.session_limits(lim, lo.numpy(), hi.numpy(), mean.cuda(), std.cuda(), Jn)
        m, s = mean.numpy(), std.numpy()
        for x, side in ((lim.lo.cpu().numpy(), "lo"), (lim.hi.cpu().numpy(), "hi")):
            finite = np.isfinite(x)
            assert finite.tolist() == np.isfinite(lo.numpy() if side == "lo" else hi.numpy()).tolist()
            fused = (x.astype(np.float64) * s.astype(np.float64) + m.astype(np.float64)).astype(np.float32) - pi32
            plain = ((x * s).astype(np.float32) + m).astype(np.float32) - pi32
            for v in (fused, plain):
                assert (v[finite] >= lo.numpy()[finite]).all() and (v[finite] <= hi.numpy()[finite]).all(), (scale, side)
            # and no further inside than the commit's resolution asks for: the inverse and the commit are six roundings of half an ulp each
            # at the largest intermediate, |bound| + pi + |mean|, and the last inward step adds at most one more
            bound = lo.numpy() if side == "lo" else hi.numpy()
            gap = np.abs(plain[finite] - bound[finite])
            assert (gap <= 8 * np.spacing(np.abs(bound[finite]) + pi32 + np.abs(m[finite]))).all(), (scale, side, float(gap.max()))
        assert (lim.lo.cpu() <= lim.hi.cpu()).all()


# ---- the command line -------------------------------------------------------------------------------------------------------------------
def test_cli_rollout_sample_and_evaluate_take_limits(tiny_model, tmp_path, capsys):
    import json

    from test_gpu_session_carry import TINY10

    from soccerdiffusion_amd import cli

    ckpt = str(tmp_path / "c.pt")
    torch.save({"model_state_dict": tiny_model.state_dict(), "hyperparams": TINY10}, ckpt)
    # rollout: radians as published, inside bit for bit
    out = str(tmp_path / "r.pt")
    assert cli.main(["rollout", ckpt, "--synthetic", "3", "--ticks", "2", "--steps", "4", "--seed", "5", "--clip", "0.5", "-o", out]) == 0
    saved = torch.load(out, weights_only=True)
    traj = saved["trajectories"]
    assert saved["limits"] == 0.5 and traj.shape == (2, 3, T, J) and bool(((traj >= -0.5) & (traj <= 0.5)).all())
    assert float(((traj == -0.5) | (traj == 0.5)).float().mean()) > 0.05
    # sample: the space of the file's trajectories (x * std + mean), as --hold; the file's denormalisation is a rounding of its own
    out = str(tmp_path / "s.pt")
    assert cli.main(["sample", ckpt, "--steps", "4", "--num_samples", "4", "--synthetic", "8", "--limits", "0=2.9:3.1,3=:3.0", "--reproject", "-o", out]) == 0
    saved = torch.load(out, weights_only=True)
    x = saved["trajectories"]
    assert saved["limits"] == {0: (2.9, 3.1), 3: (-INF, 3.0)}
    assert bool(((x[..., 0] >= 2.9 - 1e-5) & (x[..., 0] <= 3.1 + 1e-5)).all()) and bool((x[..., 3] <= 3.0 + 1e-5).all())
    out2 = str(tmp_path / "s2.pt")
    assert cli.main(["sample", ckpt, "--steps", "4", "--num_samples", "4", "--synthetic", "8", "-o", out2]) == 0
    free = torch.load(out2, weights_only=True)
    assert "limits" not in free and not bool(((free["trajectories"][..., 0] >= 2.9) & (free["trajectories"][..., 0] <= 3.1)).all())
    # evaluate: what the limits cost in rmse
    capsys.readouterr()
    assert cli.main(["evaluate", ckpt, "--synthetic", "8", "--all", "--steps", "4", "--clip", "3.0"]) == 0
    rep = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert rep["limits"] == [[-3.0, 3.0]] * J and rep["reproject"] is False and math.isfinite(rep["rmse_medoid"])
    assert cli.main(["evaluate", ckpt, "--synthetic", "8", "--all", "--steps", "4"]) == 0
    assert "limits" not in json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    for argv, what in ((["rollout", ckpt, "--synthetic", "1", "--ticks", "1", "--clip", "1", "--limits", "0=0:1"], "exclude"),
                       (["sample", ckpt, "--synthetic", "8", "--reproject"], "--reproject"),
                       (["sample", ckpt, "--synthetic", "8", "--limits", f"{J}=0:1"], "joint indices")):
        with pytest.raises(SystemExit, match=what):
            cli.main(argv)
