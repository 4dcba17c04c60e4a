"""The per-robot forms of the policy session on the GPU (``robots=`` on every entry point of soccerdiffusion_amd/session.py, the ``*_at``
kernels and ``sd_session_reset`` of csrc/sd_session.hip): robots that tick at their own times and episodes that end robot by robot, against
one list-based restatement of the reference's robot node (tests/test_gpu_session.py: HostNode) PER ROBOT."""

import numpy as np
import pytest
import torch

from conftest import rel_err
from test_gpu_session import TINY, HostNode, _reference_tick, _same_bits, _synthetic_model

pytestmark = pytest.mark.gpu
TOL = 1e-4          # tests/test_gpu_session.py: the session's tick against model.sample on the restated windows
TINY_SHAPES = {"joint_command_history": (20, (20,)), "rotation": (20, (4,)), "joint_state": (20, (20,))}


class Robots:
    """B robots, each with a HostNode of its own (B = 1): nothing one robot does can reach another's lists."""

    def __init__(self, B, shapes):
        self.shapes = dict(shapes)
        self.nodes = [HostNode(1, shapes) for _ in range(B)]

    def append(self, key, robots, rows):
        """rows (S, n, ...): block s goes to robot robots[s]."""
        for s, b in enumerate(robots):
            self.nodes[b].append(key, rows[s:s + 1])

    def reset(self, robots):
        for b in robots:
            self.nodes[b] = HostNode(1, self.shapes)

    def stacked(self, key, robots):
        return torch.cat([self.nodes[b].stacked(key) for b in robots]) if len(robots) else torch.zeros(0, self.shapes[key][0], *self.shapes[key][1])

    def batch(self, robots, game_state=True):
        """The batch of ros.py:265-275 for those robots, in their order."""
        parts = [self.nodes[b].batch(game_state) for b in robots]
        if not parts:
            return {k: self.stacked(k, []) for k in self.shapes}
        return {k: torch.cat([p[k] for p in parts]) for k in parts[0]}


def _check(session, host, keys, subsets=()):
    B = len(host.nodes)
    for robots in (None, *subsets):
        got = session.windows() if robots is None else session.windows(robots=robots)
        want = host.batch(range(B) if robots is None else robots, game_state=False)
        for k in keys:
            assert _same_bits(got[k], want[k]), (k, robots)


@pytest.fixture(scope="module")
def tiny_model():
    return _synthetic_model(TINY)[0]


@pytest.fixture(scope="module")
def default_model():
    """default.yaml's shape without images (tests/test_gpu_reference_configs.py), synthetic weights."""
    from test_gpu_reference_configs import BASE, CONFIGS

    params = {**BASE, **CONFIGS["default"]}
    return _synthetic_model(params)[0], params


@pytest.fixture(scope="module")
def image_model():
    """The sim_scratch-like shape of tests/test_gpu_session.py: ResNet-18 on 64 x 64 frames, non-trivial BatchNorm statistics."""
    from test_gpu_reference_configs import BASE, CONFIGS

    params = {**BASE, **CONFIGS["sim_scratch"], "use_images": True, "image_resolution": 64, "image_use_final_avgpool": False,
              "num_decoder_layers": 3}
    torch.manual_seed(0)
    model, _ = _synthetic_model(params)
    model.train()
    with torch.no_grad():
        model.image_sequence_encoder.image_encoder(torch.rand(2, 2, 3, 64, 64, device="cuda"))
    model.eval()
    return model, params


# ---- 1. bare rings -------------------------------------------------------------------------
def test_ring_ops_on_subsets_against_one_list_per_robot():
    """sd_ring_push_at / sd_ring_window_at on bare rings: the 16-byte window path (128 columns), a subtrahend, a long ring; no robot, one
    robot, two out of order and all of them; 0, 1, L - 1, L and L + 7 rows per push and seeded random ones.  After every push the compact
    window of the subset and the full window equal the lists, and whatever belongs to a robot that was not named kept its bits."""
    from soccerdiffusion_amd import ops

    g = torch.Generator().manual_seed(31)
    for (B, L, C), with_sub in (((5, 10, 128), False), ((3, 7, 20), True), ((2, 100, 22), False)):
        ring = torch.zeros(B, L, C, device="cuda")
        head = torch.zeros(B, dtype=torch.int32, device="cuda")
        sub = torch.randn(C, generator=g) if with_sub else None
        host = Robots(B, {"x": (L, (C,))})
        subsets = ([], [B // 2], [min(3, B - 1), 0], list(range(B)))
        pushes = [(n, robots) for n in (0, 1, L - 1, L, L + 7) for robots in subsets]
        pushes += [(n, subsets[i % 4]) for i, n in enumerate(torch.randint(0, 2 * L, (12,), generator=g).tolist())]
        for n, robots in pushes:
            rows = torch.randn(len(robots), n, C, generator=g)
            ring0, head0 = ring.clone(), head.clone()
            ops.ring_push(ring, head, rows.cuda(), None if sub is None else sub.cuda(), robots=robots)
            host.append("x", robots, rows if sub is None else rows - sub)
            case = (B, L, C, n, robots)
            assert _same_bits(ops.ring_window(ring, head, robots=robots), host.stacked("x", robots)), case
            assert _same_bits(ops.ring_window(ring, head), host.stacked("x", range(B))), case
            others = [b for b in range(B) if b not in robots]
            assert _same_bits(ring[others], ring0[others]) and torch.equal(head[others], head0[others]), case
            assert int(head.min()) >= 0 and int(head.max()) < L, case
        # the robots argument of a launch may already be on the device (the upload of ops.robot_index)
        dev = ops.robot_index(subsets[2], B).cuda()
        assert _same_bits(ops.ring_window(ring, head, robots=dev), host.stacked("x", subsets[2]))
        out = torch.empty(2, L, C, device="cuda")
        assert ops.ring_window(ring, head, out=out, robots=dev) is out and _same_bits(out, host.stacked("x", subsets[2]))
        with pytest.raises(ValueError, match="twice"):
            ops.ring_push(ring, head, torch.zeros(2, 1, C, device="cuda"), robots=[0, 0])
        with pytest.raises(ValueError, match="rows"):
            ops.ring_push(ring, head, torch.zeros(B, 1, C, device="cuda"), robots=[0])


def test_session_commit_and_reset_ops_on_bare_rings():
    """sd_session_commit_at writes the rows of sd_session_commit, into the named robots' rings only; sd_session_reset fills the selected
    robots' rings (zeros, or a fill row), zeroes their heads and writes their game state, in one launch for several rings."""
    from soccerdiffusion_amd import ops

    g = torch.Generator().manual_seed(32)
    B, L, T, J = 4, 7, 5, 20
    mean, std = torch.randn(J, generator=g).cuda(), (torch.rand(J, generator=g) + 0.5).cuda()
    ring, head = torch.zeros(B, L, J, device="cuda"), torch.zeros(B, dtype=torch.int32, device="cuda")
    full, full_head = ring.clone(), head.clone()
    robots = [2, 0]
    for _ in range(3):    # 15 rows into 7: the heads wrap
        x = torch.randn(B, T, J, generator=g).cuda()
        want = ops.session_commit(x, mean, std, full, full_head)
        got = ops.session_commit(x[robots].contiguous(), mean, std, ring, head, robots=robots)
        assert _same_bits(got, want[robots])
    assert _same_bits(ring[robots], full[robots]) and torch.equal(head[robots], full_head[robots])
    assert not ring[[1, 3]].any() and not head[[1, 3]].any()
    # reset: two rings of different shapes, one with a fill row
    other, other_head = torch.randn(B, 3, 8, generator=g).cuda(), torch.tensor([1, 2, 0, 2], dtype=torch.int32).cuda()
    fill = torch.randn(8, generator=g).cuda()
    state = torch.tensor([0, 1, 3, 1]).cuda()
    keep = [t.clone() for t in (full, full_head, other, other_head, state)]
    mask = torch.tensor([False, True, False, True]).cuda()
    ops.session_reset([(full, full_head, None), (other, other_head, fill)], mask, state, 2)
    for t, k in zip((full, full_head, other, other_head, state), keep):
        assert _same_bits(t[[0, 2]], k[[0, 2]]) if t.is_floating_point() else torch.equal(t[[0, 2]], k[[0, 2]])
    assert not full[[1, 3]].any() and not full_head[[1, 3]].any() and not other_head[[1, 3]].any()
    assert _same_bits(other[[1, 3]], fill.expand(2, 3, 8)) and state.tolist() == [0, 2, 3, 2]
    ops.session_reset([(full, full_head, None)], None, None)      # no mask: every robot; no game state
    assert not full.any() and not full_head.any() and state.tolist() == [0, 2, 3, 2]


# ---- 2. reset of a part of the batch -------------------------------------------------------
def test_partial_reset_by_device_mask_and_by_list(tiny_model):
    """After pushes and ticks, reset(robots=...) puts the selected robots - and nothing else - back to a freshly constructed session's
    state (the wrap of 0 is float(3 pi) % float(2 pi)), in place."""
    from soccerdiffusion_amd.session import PolicySession

    B, L, J, T = 3, 20, 20, 16
    s = PolicySession(tiny_model, num_inference_steps=4, batch=B)
    fresh = PolicySession(tiny_model, num_inference_steps=4, batch=B).windows()
    assert float(fresh["joint_state"][0, 0, 0]) == float(np.float32(3 * np.pi) % np.float32(2 * np.pi))
    ptrs = [t.data_ptr() for pair in (*s._rings.values(), s._action) for t in pair] + [s._game_state.data_ptr()]
    g = torch.Generator().manual_seed(33)
    keys = list(TINY_SHAPES)
    for selected, as_mask in (([1], "cuda"), ([2, 0], None), ([0, 1, 2], "cpu"), ([], "cuda")):
        for n in (3, 13, 9):   # 25 rows and three ticks of 16: every ring has wrapped
            s.push_joint_state((torch.rand(B, n, J, generator=g) - 0.5).cuda() * 8)
            s.push_rotation(torch.randn(B, n, 4, generator=g).cuda())
            s.step(torch.randn(B, T, J, generator=g).cuda())
        s.set_game_state([0, 1, 3])
        before = s.windows()
        assert not any(_same_bits(before[k][b], fresh[k][b]) for k in keys for b in range(B))
        if as_mask is None:
            s.reset(robots=selected)
        else:
            mask = torch.zeros(B, dtype=torch.bool)
            mask[selected] = True
            s.reset(robots=mask.to(as_mask))
        after = s.windows()
        for b in range(B):
            want = fresh if b in selected else before
            for k in keys:
                assert _same_bits(after[k][b], want[k][b]), (selected, b, k)
        assert after["game_state"].tolist() == [2 if b in selected else v for b, v in enumerate([0, 1, 3])]
        assert ptrs == [t.data_ptr() for pair in (*s._rings.values(), s._action) for t in pair] + [s._game_state.data_ptr()]
        s.set_game_state(2)
    s.set_game_state([3, 1], robots=[2, 0])
    assert s.windows()["game_state"].tolist() == [1, 2, 3] and s.windows(robots=[2, 1])["game_state"].tolist() == [3, 2]
    for bad in ([0, 0], [3], torch.zeros(B + 1, dtype=torch.bool), torch.zeros(B, 1, dtype=torch.bool)):
        with pytest.raises(ValueError):
            s.reset(robots=bad)


# ---- 3. robots that tick at their own times ------------------------------------------------
def test_staggered_closed_loop(tiny_model):
    """Eight ticks of three robots: robot 0 is pushed to and ticks at every tick; robot 1 ticks at every tick, is pushed to on odd ticks
    only and is reset after tick 3; robot 2 is pushed to and ticks on even ticks only.  The windows bitwise against the per-robot lists
    at every tick, the trajectories against model.sample on the same S-robot batch (1e-4)."""
    from soccerdiffusion_amd.session import PolicySession

    model = tiny_model
    B, J, T = 3, 20, 16
    s = PolicySession(model, num_inference_steps=4, batch=B)
    host = Robots(B, TINY_SHAPES)
    keys = list(TINY_SHAPES)
    g = torch.Generator().manual_seed(34)
    for tick in range(8):
        even = tick % 2 == 0
        pushed = [2, 0] if even else [0, 1]
        n = 1 if tick == 5 else 7
        q = (torch.rand(len(pushed), n, J, generator=g) - 0.5) * 8 * np.pi
        r = torch.randn(len(pushed), n, 4, generator=g)
        s.push_joint_state(q[:, 0].cuda() if n == 1 else q.cuda(), robots=pushed)    # (S, J) is the one-row form
        host.append("joint_state", pushed, q)
        s.push_rotation(r.cuda(), robots=pushed)
        host.append("rotation", pushed, r)
        ticking = ([2, 0, 1] if tick != 4 else None) if even else ([0, 1] if tick != 3 else [1, 0])
        order = list(range(B)) if ticking is None else ticking
        _check(s, host, keys, ([], order, [1]))
        x_T = torch.randn(len(order), T, J, generator=g)
        history2 = s.windows(robots=[2])["joint_command_history"]
        traj = s.step(x_T.cuda()) if ticking is None else s.step(x_T.cuda(), robots=ticking)
        assert traj.shape == (len(order), T, J)
        err = rel_err(traj, _reference_tick(model, host.batch(order), x_T, steps=4))
        print(f"staggered loop, tick {tick}, robots {order}: rel err vs model.sample {err:.3e}")
        assert err < TOL, (tick, err)
        host.append("joint_command_history", order, traj)
        if not even:   # robot 2 did not act: no row of its action history moved
            assert _same_bits(s.windows(robots=[2])["joint_command_history"], history2)
        _check(s, host, keys, (order,))
        if tick == 3:
            s.reset(robots=[1])
            host.reset([1])
            _check(s, host, keys, ([1],))
    assert s.step(robots=[]).shape == (0, T, J)
    with pytest.raises(ValueError, match=r"push_rotation: expected \(2, 4\) or \(2, n, 4\)"):
        s.push_rotation(torch.zeros(B, 4, device="cuda"), robots=[0, 1])
    with pytest.raises(ValueError, match="x_T"):
        s.step(torch.zeros(B, T, J, device="cuda"), robots=[0, 1])
    with pytest.raises(ValueError, match="twice"):
        s.step(robots=[1, 1])


# ---- 4. a captured tick survives partial resets ----------------------------------------------
def test_graph_stays_captured_across_partial_resets(default_model):
    """use_graph=True against eager, six ticks with a partial reset after tick 2 and a device-mask reset after tick 4: bitwise equal at
    every tick, and the graph object is the one captured at the first tick.  A subset tick of the graphed session runs eagerly on the
    same rings."""
    from soccerdiffusion_amd.session import PolicySession

    model, params = default_model
    B = 3
    eager = PolicySession(model, num_inference_steps=30, batch=B, hyperparams=params, seed=9)
    graphed = PolicySession(model, num_inference_steps=30, batch=B, hyperparams=params, seed=9, use_graph=True)
    g = torch.Generator().manual_seed(35)
    captured = None
    for tick in range(6):
        r = torch.randn(B, 10, 4, generator=g).cuda()
        q = (torch.rand(B, 10, 20, generator=g) - 0.5).cuda()
        x_T = torch.randn(B, 10, 20, generator=g).cuda() if tick % 2 else None     # the sessions' own generators as well
        out = []
        for s in (eager, graphed):
            s.push_rotation(r)
            s.push_joint_state(q)
            out.append(s.step(x_T))
        assert _same_bits(out[0], out[1]) and torch.isfinite(out[0]).all(), tick
        captured = captured or graphed._graph
        assert captured is not None and graphed._graph is captured and eager._graph is None
        if tick == 2:
            eager.reset(robots=[1]); graphed.reset(robots=[1])
        if tick == 4:
            mask = torch.tensor([True, False, True]).cuda()
            eager.reset(robots=mask); graphed.reset(robots=mask)
            x_S = torch.randn(2, 10, 20, generator=g).cuda()
            assert _same_bits(eager.step(x_S, robots=[2, 0]), graphed.step(x_S, robots=[2, 0]))
        assert graphed._graph is captured
        we, wg = eager.windows(), graphed.windows()
        assert all(_same_bits(we[k], wg[k]) for k in we)
    zeros = PolicySession(model, num_inference_steps=30, batch=B, hyperparams=params).windows()
    assert _same_bits(wg["rotation"][1, :70], zeros["rotation"][1, :70]) and not _same_bits(wg["rotation"][1, 70:], zeros["rotation"][1, 70:])


# ---- 5. images -------------------------------------------------------------------------------
def test_push_image_and_reset_of_one_robot(image_model, monkeypatch):
    """push_image(frames, robots=[1]) hands the backbone exactly those frames and moves robot 1's token ring only; reset(robots=[1]) writes
    the kept zero-frame token - a fresh session's token window, bit for bit - without running the backbone."""
    from soccerdiffusion_amd import ops
    from soccerdiffusion_amd.session import PolicySession

    model, params = image_model
    B, R = 3, 64
    s = PolicySession(model, num_inference_steps=4, batch=B, hyperparams=params)
    fresh = PolicySession(model, num_inference_steps=4, batch=B, hyperparams=params).windows()["image_tokens"]
    g = torch.Generator().manual_seed(36)
    s.push_image(torch.rand(B, 4, 3, R, R, generator=g).cuda())
    before = s.windows()["image_tokens"]
    seen = []
    stem = ops.stem_conv_bn_relu_pool

    def counting(x, *a, **kw):
        seen.append(int(x.shape[0]))
        return stem(x, *a, **kw)

    monkeypatch.setattr(ops, "stem_conv_bn_relu_pool", counting)
    frames = torch.rand(1, 3, 3, R, R, generator=g).cuda()
    s.push_image(frames, robots=[1])
    assert seen == [3]
    s.push_image(frames[:, 0], robots=[1])                     # (S, 3, R, R): one frame
    assert seen == [3, 1]
    after = s.windows()["image_tokens"]
    assert _same_bits(after[[0, 2]], before[[0, 2]])
    with torch.no_grad():
        tokens = model.image_sequence_encoder.image_encoder(torch.cat([frames, frames[:, :1]], dim=1))
    assert _same_bits(after[1, :6], before[1, 4:]) and rel_err(after[1, 6:], tokens[0]) < 1e-5   # (tests/test_gpu_session.py: TOKEN_TOL)
    del seen[:]
    s.reset(robots=[1])
    again = s.windows()["image_tokens"]
    assert seen == []
    assert _same_bits(again[1], fresh[1]) and _same_bits(again[[0, 2]], before[[0, 2]])
    assert _same_bits(s.windows(robots=[2, 1])["image_tokens"], again[[2, 1]])
    traj = s.step(robots=[1, 2])
    assert seen == [] and traj.shape == (2, 10, 20) and torch.isfinite(traj).all()
    with pytest.raises(ValueError, match=r"push_image: expected \(1, 3, 64, 64\)"):
        s.push_image(torch.zeros(B, 3, R, R, device="cuda"), robots=[1])


# ---- 6. stale weights --------------------------------------------------------------------------
def test_partial_reset_refuses_stale_weights():
    """A part of the batch cannot adopt new weights: reset(robots=...) raises what step raises, and the whole reset() clears it."""
    from soccerdiffusion_amd.session import PolicySession

    model, _ = _synthetic_model(TINY)          # this test changes weights: a model of its own
    s = PolicySession(model, num_inference_steps=4, batch=2)
    s.reset(robots=[0])
    with torch.no_grad():
        model.diffusion_action_generator.fc_out.bias.add_(0.25)
    for robots in ([0], torch.tensor([True, False]).cuda()):
        with pytest.raises(RuntimeError, match=r"reset\(\)"):
            s.reset(robots=robots)
    with pytest.raises(RuntimeError, match=r"reset\(\)"):
        s.step(robots=[1])
    s.reset()
    s.reset(robots=[0])
    assert torch.isfinite(s.step(robots=[1])).all()


# ---- 7. command line -----------------------------------------------------------------------------
def test_cli_rollout_with_episodes_that_end_robot_by_robot(tmp_path):
    import yaml
    from test_gpu_cli import CFG, _run

    cfg = tmp_path / "cfg.yaml"
    cfg.write_text(yaml.safe_dump(dict(CFG, epochs=1)))
    ckpt = tmp_path / "model.pth"
    r = _run("train", "-c", str(cfg), "-o", str(ckpt), "--synthetic", "128")
    assert r.returncode == 0, r.stderr[-2000:]
    common = ("rollout", str(ckpt), "--synthetic", "3", "--ticks", "5", "--steps", "10", "--seed", "5")
    r = _run(*common, "--episode-ticks", "2,3", "-o", str(tmp_path / "episodes.pt"))
    assert r.returncode == 0, r.stderr[-2000:]
    r = _run(*common, "-o", str(tmp_path / "plain.pt"))
    assert r.returncode == 0, r.stderr[-2000:]
    episodes, plain = torch.load(tmp_path / "episodes.pt", weights_only=True), torch.load(tmp_path / "plain.pt", weights_only=True)
    assert set(plain) == {"trajectories", "ticks", "steps", "seed"} and set(episodes) == set(plain) | {"resets"}
    traj = episodes["trajectories"]
    assert traj.shape == (5, 3, CFG["trajectory_prediction_length"], CFG["num_joints"]) and torch.isfinite(traj).all()
    # robots 0 and 2: episodes of 2 ticks (reset after ticks 1 and 3); robot 1: 3 ticks (after tick 2)
    want = torch.tensor([[False, False, False], [True, False, True], [False, True, False], [True, False, True], [False, False, False]])
    assert episodes["resets"].dtype == torch.bool and torch.equal(episodes["resets"], want)
    # until the first reset the two runs are the same run; after it the reset robots see another history
    assert _same_bits(traj[:2], plain["trajectories"][:2]) and not torch.equal(traj[2], plain["trajectories"][2])
