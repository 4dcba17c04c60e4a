"""Held joints of the policy session on the GPU (``PolicySession(holds=True)``: sd_session_hold, sd_session_hold_mask, the rollout with
held elements underneath): the published joints bit for bit, against ``model.sample(hold=...)``, with carried rows, across resets and
releases, in the captured tick, the session without ``holds`` as it was, and ``cli rollout --hold``."""

import math
import os
import subprocess
import sys

import pytest
import torch

from conftest import REPO, rel_err
from test_gpu_session import _same_bits
from test_gpu_session_carry import ADVANCE, B, CARRY, J, STEPS, T, _push, _sensors, default_model, tiny_model  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu
FAMILY_TOL = 2e-5   # two instantiations on the same inputs: tests/test_gpu_generic_traj.py:77
JOINTS, ROBOTS = [0, 1], [0, 2]
V = torch.tensor([0.3, -0.7])


def _normalised(model, v, joints):
    """The session's expression on the host, one rounding per operation: ((v + pi) - mean) / std."""
    mean, std = model.mean.cpu()[joints], model.std.cpu()[joints]
    return ((v + math.pi) - mean) / std


def _published(model, v, joints):
    """... and the commit's of it: (normalised * std + mean) - pi."""
    mean, std = model.mean.cpu()[joints], model.std.cpu()[joints]
    return (_normalised(model, v, joints) * std + mean) - math.pi


def _held_everywhere(traj, want, robots=ROBOTS, joints=JOINTS):
    got = traj.cpu()[robots][:, :, joints]
    return _same_bits(got, want.expand_as(got).contiguous())


def test_held_joints_are_published_exactly_and_the_tick_is_model_sample(tiny_model):
    from soccerdiffusion_amd.session import PolicySession

    m = tiny_model
    s = PolicySession(m, num_inference_steps=STEPS, batch=B, holds=True)
    assert s.holds and s._held.tolist() == [0] * B and not s._carrying
    s.hold(JOINTS, V, robots=ROBOTS)
    assert s._held.tolist() == [3, 0, 3]
    assert _same_bits(s._pin_x0.cpu()[ROBOTS][:, :, JOINTS], _normalised(m, V, JOINTS).expand(2, T, 2).contiguous())
    assert not s._pin_x0[1].any() and not s._pin_x0[:, :, 2:].any()
    want = _published(m, V, JOINTS)
    mask = torch.zeros(B, T, J, dtype=torch.bool)
    for b in ROBOTS:
        mask[b, :, JOINTS] = True
    g = torch.Generator().manual_seed(51)
    for tick in range(2):
        q, r = _sensors(g, B, T)
        _push((s,), q, r)
        x_T = torch.randn(B, T, J, generator=g).cuda()
        with torch.no_grad():   # (as step() encodes it; reads the rings, moves nothing)
            ctx = s._context()
        x = m.sample(ctx, x_T, STEPS, max_mode=3, hold=(s._pin_x0.clone(), mask))
        traj = s.step(x_T)
        assert _held_everywhere(traj, want), tick
        assert torch.equal(s._mask.cpu(), mask.long().mul(1 << torch.arange(J)).sum(-1).int())
        assert not (traj.cpu()[1][:, JOINTS] == want).any()                 # robot 1 is free
        assert not (traj.cpu()[ROBOTS][:, :, 2:] == want[0]).any()          # so are the other joints
        assert _same_bits(traj, (x * m.std + m.mean) - math.pi), tick       # the commit's expression of model.sample's result
    # per-robot and per-row values; a release; a subset tick gathers its robots' mask rows
    per_row = torch.rand(2, T, 2, generator=g) - 0.5
    s.hold(JOINTS, per_row, robots=ROBOTS)
    s.hold([5], torch.tensor([[0.1], [0.2], [0.3]]))
    assert s._held.tolist() == [35, 32, 35]
    s.release([5], robots=[0, 1])
    assert s._held.tolist() == [3, 0, 35]
    x_S = torch.randn(2, T, J, generator=g).cuda()
    traj = s.step(x_S, robots=[2, 1]).cpu()
    assert _same_bits(traj[0][:, JOINTS], _published(m, per_row[1], JOINTS))
    assert _same_bits(traj[0][:, 5], _published(m, torch.tensor([0.3]), [5]).expand(T).contiguous())
    assert not (traj[1][:, 5] == _published(m, torch.tensor([0.2]), [5])).any()
    s.release()
    assert s._held.tolist() == [0] * B
    traj = s.step(torch.randn(B, T, J, generator=g).cuda()).cpu()
    assert not (traj[:, :, 5] == _published(m, torch.tensor([0.3]), [5])).any()
    for bad in (([J], V[:1]), (JOINTS, V[:1]), (JOINTS, torch.zeros(B + 1, 2)), ([0, 0], V)):
        with pytest.raises(ValueError):
            s.hold(*bad)


def test_carry_and_hold_compose_and_a_hold_survives_resets(tiny_model):
    from soccerdiffusion_amd.session import PolicySession

    m = tiny_model
    s = PolicySession(m, num_inference_steps=STEPS, batch=B, carry=CARRY, advance=ADVANCE, holds=True)
    s.hold(JOINTS, V, robots=ROBOTS)
    with pytest.raises(ValueError, match="carry"):
        s.hold(JOINTS, torch.zeros(B, T, 2))
    want = _published(m, V, JOINTS)
    g = torch.Generator().manual_seed(52)
    prev = None

    def tick():
        q, r = _sensors(g, B)
        _push((s,), q, r)
        return s.step(torch.randn(B, T, J, generator=g).cuda())

    for k in range(3):
        traj = tick()
        assert _held_everywhere(traj, want), k                              # in carried and free rows alike
        if prev is not None:
            assert _same_bits(traj[:, :CARRY], prev[:, ADVANCE:ADVANCE + CARRY]), k      # the seam stays exact
            assert not _same_bits(traj[:, CARRY], prev[:, ADVANCE + CARRY])
            full = (1 << J) - 1
            assert s._mask.tolist() == [[full] * CARRY + [held] * (T - CARRY) for held in (3, 0, 3)]
        prev = traj
    s.reset(robots=[0])      # robot 0's episode ends: its carried rows go, its hold stays
    assert s._pin_rows.tolist() == [0, CARRY, CARRY] and s._held.tolist() == [3, 0, 3]
    traj = tick()
    assert _held_everywhere(traj, want)
    assert _same_bits(traj[1:, :CARRY], prev[1:, ADVANCE:ADVANCE + CARRY]) and not _same_bits(traj[0, :CARRY], prev[0, ADVANCE:ADVANCE + CARRY])
    assert s._mask[0].tolist() == [3] * T
    s.reset()                # a whole reset: new rings, the held joints stay held (a switched-off motor stays off)
    assert s._pin_rows.tolist() == [0] * B and s._held.tolist() == [3, 0, 3]
    assert _held_everywhere(tick(), want)


def test_after_release_the_tick_is_the_session_without_holds(tiny_model):
    from soccerdiffusion_amd.session import PolicySession

    s = PolicySession(tiny_model, num_inference_steps=STEPS, batch=B, holds=True)
    plain = PolicySession(tiny_model, num_inference_steps=STEPS, batch=B)
    s.hold(JOINTS, V, robots=ROBOTS)
    s.release(joints=[0], robots=[0])
    assert s._held.tolist() == [2, 0, 3]
    s.release()
    g = torch.Generator().manual_seed(53)
    q, r = _sensors(g, B, T)
    _push((s, plain), q, r)
    x_T = torch.randn(B, T, J, generator=g).cuda()
    err = rel_err(s.step(x_T), plain.step(x_T))
    print(f"a holds=True session after release() against a session without holds: {err:.3e}")
    assert err < FAMILY_TOL


def test_graphed_session_equals_eager_bitwise_across_hold_release_and_reset(default_model):
    from soccerdiffusion_amd.session import PolicySession

    model, params = default_model
    kw = dict(num_inference_steps=STEPS, batch=B, hyperparams=params, seed=9, carry=CARRY, advance=ADVANCE, holds=True)
    eager, graphed = PolicySession(model, **kw), PolicySession(model, use_graph=True, **kw)
    both = (eager, graphed)
    want = _published(model, V, JOINTS)
    g = torch.Generator().manual_seed(54)
    captured, prev = None, None
    for tick in range(4):
        q, r = _sensors(g, B)
        _push(both, q, r)
        x_T = torch.randn(B, T, J, generator=g).cuda() if tick % 2 else None     # the sessions' own generators as well
        out = [s.step(x_T) for s in both]
        assert _same_bits(out[0], out[1]) and torch.isfinite(out[0]).all(), tick
        captured = captured or graphed._graph
        assert captured is not None and graphed._graph is captured and eager._graph is None      # no re-capture
        if tick == 0:
            assert not _held_everywhere(out[0], want)
            for s in both:
                s.hold(JOINTS, V, robots=ROBOTS)
        if tick == 1:
            assert _held_everywhere(out[0], want)
            # the seam: exact wherever nothing was newly held between the two ticks - a hold takes the carried rows' joints too
            assert _same_bits(out[0][1, :CARRY], prev[1, ADVANCE:ADVANCE + CARRY])
            assert _same_bits(out[0][:, :CARRY, 2:], prev[:, ADVANCE:ADVANCE + CARRY, 2:])
            for s in both:
                s.release(joints=[1], robots=[2])
                s.reset(robots=[1])
            assert graphed._pin_rows.tolist() == [CARRY, 0, CARRY] and graphed._held.tolist() == [3, 0, 1]
        if tick == 2:
            assert _held_everywhere(out[0], want, robots=[0]) and _held_everywhere(out[0], want[:1], robots=[2], joints=[0])
            assert _same_bits(out[0][[0, 2], :CARRY], prev[[0, 2], ADVANCE:ADVANCE + CARRY])
            for s in both:
                s.release()
        if tick == 3:
            assert not _held_everywhere(out[0], want, robots=[0])
        prev = out[0]
    x_S = torch.randn(2, T, J, generator=g).cuda()       # a subset tick of the graphed session runs eagerly on the same buffers
    assert _same_bits(eager.step(x_S, robots=[2, 0]), graphed.step(x_S, robots=[2, 0]))


def test_with_draws_every_draw_holds_the_robots_values(tiny_model):
    from soccerdiffusion_amd.session import PolicySession

    G = 3
    s = PolicySession(tiny_model, num_inference_steps=STEPS, batch=B, draws=G, holds=True)
    s.hold(JOINTS, V, robots=ROBOTS)
    g = torch.Generator().manual_seed(55)
    q, r = _sensors(g, B, T)
    _push((s,), q, r)
    traj, every, index = s.step(torch.randn(B * G, T, J, generator=g).cuda(), return_draws=True)
    want = _published(tiny_model, V, JOINTS)
    assert _held_everywhere(traj, want)
    assert all(_held_everywhere(every[:, i], want) for i in range(G))
    assert s._mask.tolist() == [[held] * T for held in (3, 0, 3) for _ in range(G)]


def test_a_session_without_holds_makes_the_calls_it_made(tiny_model):
    from soccerdiffusion_amd.session import PolicySession

    m = tiny_model
    s = PolicySession(m, num_inference_steps=STEPS, batch=B, carry=CARRY, advance=ADVANCE)
    assert not s.holds and not hasattr(s, "_held") and not hasattr(s, "_mask") and set(s._cond()) == {"pin"}
    with pytest.raises(RuntimeError, match="holds=True"):
        s.hold(JOINTS, V)
    with pytest.raises(RuntimeError, match="holds=True"):
        s.release()
    g = torch.Generator().manual_seed(56)
    for tick in range(2):
        q, r = _sensors(g, B)
        _push((s,), q, r)
        x_T = torch.randn(B, T, J, generator=g).cuda()
        with torch.no_grad():   # (as step() encodes it)
            ctx = s._context()
        x = m.sample(ctx, x_T, STEPS, max_mode=3, pin=(s._pin_x0.clone(), s._pin_rows.clone()))      # the parent's arguments
        assert _same_bits(s.step(x_T), (x * m.std + m.mean) - math.pi), tick
    with pytest.raises(ValueError, match="distilled"):
        PolicySession(m, batch=B, holds=True, distilled=True)


def test_cli_rollout_with_hold(tmp_path):
    from test_gpu_cli import CFG

    from soccerdiffusion_amd import cli

    params = dict(CFG, trajectory_prediction_length=10)
    torch.manual_seed(3)
    model = cli.build_model(params)      # an untrained checkpoint: the command line is under test, not the policy
    ckpt = tmp_path / "model.pth"
    torch.save({"hyperparams": params, "model_state_dict": model.state_dict()}, ckpt)
    out = tmp_path / "hold.pt"
    run = lambda *flags: subprocess.run([sys.executable, "-m", "soccerdiffusion_amd.cli", "rollout", str(ckpt), "--synthetic", "2", *flags],
                                        cwd=REPO, env=dict(os.environ, PYTHONPATH=REPO), capture_output=True, text=True, timeout=240)
    r = run("--ticks", "3", "--steps", "4", "--seed", "5", "--carry", "4", "--advance", "5", "--hold", "0=0.25,3=-1.5", "-o", str(out))
    assert r.returncode == 0, r.stderr[-2000:]
    saved = torch.load(out, weights_only=True)
    assert saved["hold"] == {0: 0.25, 3: -1.5}
    traj = saved["trajectories"]
    assert traj.shape == (3, 2, 10, CFG["num_joints"]) and torch.isfinite(traj).all()
    want = _published(model, torch.tensor([0.25, -1.5]), [0, 3])
    assert _same_bits(traj[:, :, :, [0, 3]], want.expand(3, 2, 10, 2).contiguous())
    assert not (traj[:, :, :, 1] == want[0]).any()
    for k in range(1, 3):
        assert _same_bits(traj[k][:, :4], traj[k - 1][:, 5:9]), k
    bad = run("--ticks", "1", "--hold", f"{CFG['num_joints']}=0.5")
    assert bad.returncode != 0 and "--hold" in bad.stderr
    # cli sample --hold: the values are in the space of the file's trajectories (x * std + mean)
    samples = tmp_path / "samples.pt"
    r = subprocess.run([sys.executable, "-m", "soccerdiffusion_amd.cli", "sample", str(ckpt), "--steps", "4", "--num_samples", "3", "--synthetic", "16",
                        "--hold", "2=1.5", "-o", str(samples)], cwd=REPO, env=dict(os.environ, PYTHONPATH=REPO), capture_output=True, text=True,
                       timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    saved = torch.load(samples, weights_only=True)
    mean, std = model.mean[2], model.std[2]
    assert saved["hold"] == {2: 1.5}
    assert _same_bits(saved["trajectories"][:, :, 2], (((torch.tensor(1.5) - mean) / std) * std + mean).expand(3, 10).contiguous())
    assert not (saved["trajectories"][:, :, 3] == saved["trajectories"][:, :, 2]).any()
