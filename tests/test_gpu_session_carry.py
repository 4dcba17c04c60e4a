"""Overlapping ticks of the policy session on the GPU (``PolicySession(carry=K, advance=S)``: sd_session_commit_carry(_at),
sd_session_reset_carry, the pinned rollout underneath): the seam between two ticks bit for bit, the action ring against a host model,
subset ticks, partial resets, the captured tick, and the session without carry as the yardstick."""

import pytest
import torch

from conftest import rel_err
from test_gpu_session import TINY, _same_bits, _synthetic_model
from test_gpu_session_robots import TINY_SHAPES, Robots

pytestmark = pytest.mark.gpu
FAMILY_TOL = 2e-5   # two kernel families on the same inputs: tests/test_gpu_generic_traj.py:77
B, T, J, CARRY, ADVANCE, STEPS = 3, 10, 20, 4, 5, 4
TINY10 = {**TINY, "trajectory_prediction_length": T}


@pytest.fixture(scope="module")
def tiny_model():
    """hidden_dim 64: the rollout runs the unfused chains, the pinned rows are ddim_pin_kernel's."""
    return _synthetic_model(TINY10)[0]


@pytest.fixture(scope="module")
def default_model():
    """default.yaml's shape without images: the rollout runs the generic trajectory kernels' pinned instantiation."""
    from test_gpu_reference_configs import BASE, CONFIGS

    params = {**BASE, **CONFIGS["default"]}
    return _synthetic_model(params)[0], params


def _sensors(g, S, n=ADVANCE):
    return (torch.rand(S, n, J, generator=g) - 0.5) * 6, torch.randn(S, n, 4, generator=g)


def _push(sessions, q, r, robots=None):
    for s in sessions:
        s.push_joint_state(q.cuda(), robots=robots)
        s.push_rotation(r.cuda(), robots=robots)


def test_seam_is_bitwise_and_the_ring_takes_the_committed_rows(tiny_model):
    from soccerdiffusion_amd.session import PolicySession

    s = PolicySession(tiny_model, num_inference_steps=STEPS, batch=B, carry=CARRY, advance=ADVANCE)
    plain = PolicySession(tiny_model, num_inference_steps=STEPS, batch=B)
    assert (s.carry, s.advance) == (CARRY, ADVANCE) and (plain.carry, plain.advance) == (0, T) and not plain._carrying
    host = Robots(B, TINY_SHAPES)
    g = torch.Generator().manual_seed(41)
    prev = None
    for tick in range(3):
        q, r = _sensors(g, B)
        _push((s,) if tick else (s, plain), q, r)
        host.append("joint_state", range(B), q)
        host.append("rotation", range(B), r)
        x_T = torch.randn(B, T, J, generator=g).cuda()
        traj = s.step(x_T)
        assert traj.shape == (B, T, J) and torch.isfinite(traj).all()
        if tick == 0:
            # nothing is pinned at a first tick: the session without carry on the same windows and noise
            err = rel_err(traj, plain.step(x_T))
            print(f"first tick of a carry={CARRY} session against a carry=0 session: {err:.3e}")
            assert err < FAMILY_TOL
        else:
            assert _same_bits(traj[:, :CARRY], prev[:, ADVANCE:ADVANCE + CARRY]), tick
            assert not _same_bits(traj[:, CARRY], prev[:, ADVANCE + CARRY])      # the rows behind the overlap are sampled
        assert s._pin_rows.tolist() == [CARRY] * B
        # the action ring holds this tick's first ADVANCE published rows, not all T
        host.append("joint_command_history", range(B), traj[:, :ADVANCE])
        got, want = s.windows(), host.batch(range(B), game_state=False)
        for k in TINY_SHAPES:
            assert _same_bits(got[k], want[k]), (tick, k)
        prev = traj


def test_advance_without_carry_commits_fewer_rows_of_the_same_trajectory(tiny_model):
    from soccerdiffusion_amd.session import PolicySession

    s = PolicySession(tiny_model, num_inference_steps=STEPS, batch=B, advance=ADVANCE)
    plain = PolicySession(tiny_model, num_inference_steps=STEPS, batch=B)
    host = Robots(B, TINY_SHAPES)
    g = torch.Generator().manual_seed(42)
    q, r = _sensors(g, B)
    _push((s, plain), q, r)
    x_T = torch.randn(B, T, J, generator=g).cuda()
    traj = s.step(x_T)
    assert _same_bits(traj, plain.step(x_T))             # no pinned rows: the very same launches up to the commit
    assert s._pin() is None and s._pin_rows.tolist() == [0] * B
    host.append("joint_command_history", range(B), traj[:, :ADVANCE])
    assert _same_bits(s.windows()["joint_command_history"], host.batch(range(B), game_state=False)["joint_command_history"])


def test_subset_ticks_and_partial_resets(tiny_model):
    from soccerdiffusion_amd.session import PolicySession

    s = PolicySession(tiny_model, num_inference_steps=STEPS, batch=B, carry=CARRY, advance=ADVANCE)
    g = torch.Generator().manual_seed(43)
    last = [None] * B

    def tick(robots=None):
        order = list(range(B)) if robots is None else robots
        q, r = _sensors(g, len(order))
        _push((s,), q, r, robots=robots)
        x_T = torch.randn(len(order), T, J, generator=g).cuda()
        traj = s.step(x_T) if robots is None else s.step(x_T, robots=robots)
        for i, b in enumerate(order):
            if last[b] is not None:
                assert _same_bits(traj[i, :CARRY], last[b][ADVANCE:ADVANCE + CARRY]), (robots, b)
            last[b] = traj[i]
        return q, r, x_T, traj

    tick()
    # a subset tick moves its own robots' carry only
    rows1, win1 = s._pin_x0[1].clone(), s.windows(robots=[1])
    tick([2, 0])
    assert _same_bits(s._pin_x0[1], rows1) and s._pin_rows.tolist() == [CARRY] * B
    after = s.windows(robots=[1])
    assert all(_same_bits(after[k], win1[k]) for k in win1)
    tick()          # robot 1 continues its own last trajectory, robots 0 and 2 theirs
    # a partial reset, by index and by device mask: robot 1's next tick is a first tick, robots 0 and 2 stay pinned
    for how in ("index", "mask"):
        s.reset(robots=[1] if how == "index" else torch.tensor([False, True, False]).cuda())
        assert s._pin_rows.tolist() == [CARRY, 0, CARRY], how
        last[1] = None
        q, r, x_T, traj = tick()
        fresh = PolicySession(tiny_model, num_inference_steps=STEPS, batch=B)
        _push((fresh,), q, r)
        err = rel_err(traj[1], fresh.step(x_T)[1])
        print(f"robot 1 after reset by {how} against a carry=0 session: {err:.3e}")
        assert err < FAMILY_TOL
        assert s._pin_rows.tolist() == [CARRY] * B
        tick()


def test_graphed_session_equals_eager_bitwise_across_a_partial_reset(default_model):
    from soccerdiffusion_amd.session import PolicySession

    model, params = default_model
    kw = dict(num_inference_steps=STEPS, batch=B, hyperparams=params, seed=9, carry=CARRY, advance=ADVANCE)
    eager, graphed = PolicySession(model, **kw), PolicySession(model, use_graph=True, **kw)
    g = torch.Generator().manual_seed(44)
    captured, prev = None, None
    for tick in range(3):
        q, r = _sensors(g, B)
        _push((eager, graphed), q, r)
        x_T = torch.randn(B, T, J, generator=g).cuda() if tick % 2 else None     # the sessions' own generators as well
        out = [s.step(x_T) for s in (eager, graphed)]
        assert _same_bits(out[0], out[1]) and torch.isfinite(out[0]).all(), tick
        captured = captured or graphed._graph
        assert captured is not None and graphed._graph is captured and eager._graph is None
        if tick == 1:
            assert _same_bits(out[0][:, :CARRY], prev[:, ADVANCE:ADVANCE + CARRY])
            eager.reset(robots=[1]); graphed.reset(robots=[1])
            assert graphed._pin_rows.tolist() == [CARRY, 0, CARRY]
        if tick == 2:
            assert _same_bits(out[0][[0, 2], :CARRY], prev[[0, 2], ADVANCE:ADVANCE + CARRY])
            assert not _same_bits(out[0][1, :CARRY], prev[1, ADVANCE:ADVANCE + CARRY])
        assert graphed._graph is captured
        we, wg = eager.windows(), graphed.windows()
        assert all(_same_bits(we[k], wg[k]) for k in we)
        prev = out[0]
    x_S = torch.randn(2, T, J, generator=g).cuda()       # a subset tick of the graphed session runs eagerly on the same buffers
    assert _same_bits(eager.step(x_S, robots=[2, 0]), graphed.step(x_S, robots=[2, 0]))


def test_carry_is_refused_for_a_distilled_decoder(tiny_model):
    from soccerdiffusion_amd.session import PolicySession

    with pytest.raises(ValueError, match="distilled"):
        PolicySession(tiny_model, batch=B, carry=CARRY, distilled=True)
    with pytest.raises(ValueError, match="exceeds"):
        PolicySession(tiny_model, batch=B, carry=CARRY, advance=T - CARRY + 1)
    PolicySession(tiny_model, batch=B, advance=ADVANCE, distilled=True)      # fewer committed rows alone need no rollout
