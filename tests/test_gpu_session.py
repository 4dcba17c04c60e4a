"""The closed-loop policy session (soccerdiffusion_amd/session.py, csrc/sd_session.hip) on the GPU against a list-based restatement of the
reference's robot node (soccer_diffusion/ml/inference/ros.py:87-106 initial buffers, 203 / 256-257 / 316-318 append and trim, 265-275 the
batch of a tick, 293-313 rollout and denormalisation, 317 / 327 the published trajectory)."""

import os

import numpy as np
import pytest
import torch

from conftest import rel_err

pytestmark = pytest.mark.gpu
TOL = 1e-4          # tests/test_gpu_reference_configs.py
TOKEN_TOL = 1e-5    # tests/test_gpu_image_path.py: one backbone, two batch compositions

TINY = dict(hidden_dim=64, action_context_length=20, trajectory_prediction_length=16, epochs=1, batch_size=4, lr=1e-3,
            train_denoising_timesteps=1000, image_context_length=0, imu_context_length=20, num_imu_encoder_layers=1,
            joint_state_context_length=20, num_normalization_samples=10, num_joints=20, use_action_history=True,
            num_action_history_encoder_layers=1, use_imu=True, imu_orientation_embedding_method="quaternion", use_joint_states=True,
            joint_state_encoder_layers=1, use_images=False, image_sequence_encoder_type="transformer", image_encoder_type="resnet18",
            num_image_sequence_encoder_layers=1, num_decoder_layers=2, distill_teacher_inference_steps=30, use_gamestate=True,
            encoder_patch_size=5)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


class HostNode:
    """ros.py's buffers: per stream a Python list of per-sample CPU tensors (here (B, C) each: B robots in lockstep), initialised with
    ``context_length`` zero rows, appended to and trimmed to the last ``context_length`` entries."""

    def __init__(self, B, shapes):
        self.B, self.shapes = B, dict(shapes)
        self.lists = {k: [torch.zeros(B, *c)] * L for k, (L, c) in self.shapes.items()}

    def append(self, key, rows):
        """rows (B, n, ...), oldest first."""
        rows = rows.detach().cpu()
        for i in range(rows.shape[1]):
            self.lists[key].append(rows[:, i].clone())
        self.lists[key] = self.lists[key][-self.shapes[key][0]:]

    def stacked(self, key):
        return torch.stack(list(self.lists[key]), dim=1)

    def batch(self, game_state=True):
        """The batch of ros.py:265-275 (CPU tensors)."""
        out = {}
        for key in self.lists:
            x = self.stacked(key)
            out[key] = (x + 3 * np.pi) % (2 * np.pi) if key in ("joint_state", "joint_command_history") else x
        if game_state:
            out["game_state"] = torch.zeros(self.B, dtype=torch.long) + 2
        return out


def _synthetic_model(params, seed=21):
    from test_gpu_reference_configs import _state_dict_for

    from soccerdiffusion_amd import cli

    sd = _state_dict_for(params)
    model = cli.build_model(params).cuda().eval()
    model.load_state_dict(sd, strict=not params["use_images"])   # (the image path keeps its seeded initialisation)
    return model, sd


def _check_windows(session, host, keys):
    got = session.windows()
    want = host.batch(game_state=False)
    for k in keys:
        assert _same_bits(got[k], want[k]), k


@pytest.fixture(scope="module")
def default_model():
    """default.yaml's shape without images (tests/test_gpu_reference_configs.py), synthetic weights."""
    from test_gpu_reference_configs import BASE, CONFIGS

    params = {**BASE, **CONFIGS["default"]}
    model, sd = _synthetic_model(params)
    return model, sd, params


@pytest.fixture(scope="module")
def image_model():
    """A sim_scratch-like shape: action history + five-dimensional IMU at patch 5, ResNet-18 on 64 x 64 frames without the final avgpool,
    one sequence-encoder layer, d = 256; non-trivial BatchNorm statistics and normaliser."""
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


# ---- 1. ring semantics -------------------------------------------------------------------
def test_ring_ops_against_list_buffers():
    """sd_ring_push / sd_ring_window on bare rings: a token-like ring (128 columns: the 16-byte path) and a joint-like one with a
    subtrahend; 0, 1, L - 1, L and L + 7 rows per push and several wraps."""
    from soccerdiffusion_amd import ops

    g = torch.Generator().manual_seed(11)
    for (B, L, C), with_sub in (((2, 10, 128), False), ((3, 7, 20), True), ((1, 100, 22), False)):
        ring = torch.zeros(B, L, C, device="cuda")
        head = torch.zeros(B, dtype=torch.int32, device="cuda")
        sub = torch.randn(C, generator=g) if with_sub else None
        host = HostNode(B, {"x": (L, (C,))})
        for n in [0, 1, L - 1, L, L + 7] + torch.randint(0, 2 * L, (12,), generator=g).tolist():
            rows = torch.randn(B, n, C, generator=g)
            ops.ring_push(ring, head, rows.cuda(), None if sub is None else sub.cuda())
            host.append("x", rows if sub is None else rows - sub)
            assert _same_bits(ops.ring_window(ring, head), host.stacked("x")), (B, L, C, n)
            assert int(head.min()) >= 0 and int(head.max()) < L and int(head.min()) == int(head.max())


def test_session_windows_follow_ros_buffers():
    """After every push (and every tick) windows() equals ros.py's append-and-trim buffers: rotation bitwise (a copy), joint state and
    action history bitwise equal to torch's CPU (x + 3 * np.pi) % (2 * np.pi)."""
    from soccerdiffusion_amd.session import PolicySession

    model, _ = _synthetic_model(TINY)
    B, L, J, T = 3, 20, 20, 16
    s = PolicySession(model, num_inference_steps=4, batch=B)
    host = HostNode(B, {"joint_command_history": (L, (J,)), "rotation": (L, (4,)), "joint_state": (L, (J,))})
    keys = list(host.lists)
    _check_windows(s, host, keys)   # context_length rows of zeros: the wrap of 0 is float(3 pi) % float(2 pi)
    g = torch.Generator().manual_seed(12)
    counts = [0, 1, L - 1, L, L + 7]
    schedule = list(zip(counts, reversed(counts))) + [tuple(v) for v in torch.randint(0, 2 * L, (10, 2), generator=g).tolist()]
    special = torch.tensor([0.0, -0.0, np.pi, -np.pi, 3 * np.pi, -3 * np.pi])
    for tick, (nj, nr) in enumerate(schedule):
        q = (torch.rand(B, nj, J, generator=g) - 0.5) * 8 * np.pi
        if nj:
            q[:, :, :6] = special       # the wrap's edge cases travel through the ring as well
        r = torch.randn(B, nr, 4, generator=g)
        s.push_joint_state(q[:, 0].cuda() if nj == 1 else q.cuda())    # (B, J) is the one-row form
        host.append("joint_state", q)
        _check_windows(s, host, keys)
        s.push_rotation(r[:, 0].cuda() if nr == 1 else r.cuda())
        host.append("rotation", r)
        _check_windows(s, host, keys)
        if tick % 2 == 1:   # T = 16 rows into the 20-row action ring: it wraps at every second tick
            traj = s.step(torch.randn(B, T, J, generator=g).cuda())
            assert torch.isfinite(traj).all()
            host.append("joint_command_history", traj)
            _check_windows(s, host, keys)
    with pytest.raises(RuntimeError, match="switched off"):
        s.push_image(torch.zeros(B, 3, 64, 64, device="cuda"))
    with pytest.raises(ValueError):
        s.push_rotation(torch.zeros(B, 5, device="cuda"))
    s.reset()
    _check_windows(s, HostNode(B, host.shapes), keys)


# ---- 2. closed loop, teacher-forced ------------------------------------------------------
def _reference_tick(model, batch, x_T, steps=30):
    """The tick on the existing public API: encode the full stacked windows, sample, denormalise, - pi."""
    from soccerdiffusion_amd import ops

    with torch.no_grad():
        x = model.sample(model.encode_input_data({k: v.cuda().contiguous() for k, v in batch.items()}), x_T.cuda(), steps)
        return ops.normalize(x.contiguous(), model.mean, model.std, inverse=True) - np.pi


def test_closed_loop_default_shape_without_images(default_model):
    """12 ticks at B = 3: the action ring (100 rows, 10 per tick) wraps.  Every tick against model.sample on the restated windows (1e-4),
    the windows bitwise, and the first three ticks against the CPU oracle (1e-4)."""
    from oracle import ddim_ref
    from oracle import denoiser_ref as ref

    from soccerdiffusion_amd.session import PolicySession

    model, sd, params = default_model
    B, T, J = 3, 10, 20
    s = PolicySession(model, num_inference_steps=30, batch=B)
    host = HostNode(B, {"joint_command_history": (100, (J,)), "rotation": (100, (4,)), "joint_state": (100, (J,))})
    keys = list(host.lists)
    g = torch.Generator().manual_seed(13)
    acp = ddim_ref.alphas_cumprod()
    for tick in range(12):
        q = (torch.rand(B, T, J, generator=g) - 0.5) * 2 * np.pi
        r = torch.randn(B, T, 4, generator=g)
        s.push_joint_state(q.cuda()); host.append("joint_state", q)
        s.push_rotation(r.cuda()); host.append("rotation", r)
        x_T = torch.randn(B, T, J, generator=g)
        batch = host.batch()
        _check_windows(s, host, keys)
        traj = s.step(x_T.cuda())
        want = _reference_tick(model, batch, x_T)
        err = rel_err(traj, want)
        print(f"default shape, tick {tick}: rel err vs model.sample {err:.3e}")
        assert err < TOL, (tick, err)
        if tick < 3:
            ctx = ref.encode_input_data(sd, batch)
            x0 = ddim_ref.sample(lambda xx, t: ref.forward_with_context(sd, ctx, xx, torch.full((B,), t, dtype=torch.int64)), x_T, 30, acp)[-1]
            oracle = ref.denormalize(x0, sd["mean"], sd["std"]) - np.pi
            err = rel_err(traj, oracle)
            print(f"default shape, tick {tick}: rel err vs CPU oracle {err:.3e}")
            assert err < TOL, (tick, err)
        host.append("joint_command_history", traj)   # teacher forcing: the session's own published trajectory
    _check_windows(s, host, keys)


def test_closed_loop_with_cached_image_tokens(image_model):
    """12 ticks at B = 2 with two new frames per tick: the token ring (10 tokens) and the action ring both wrap.  The cached tokens
    against the backbone run on the whole restated frame window (1e-5), the trajectory against model.sample on it (1e-4), the other
    windows bitwise."""
    from soccerdiffusion_amd.session import PolicySession

    model, params = image_model
    B, T, J, R, S = 2, 10, 20, 64, 10
    s = PolicySession(model, num_inference_steps=30, batch=B, hyperparams=params)
    host = HostNode(B, {"joint_command_history": (100, (J,)), "rotation": (100, (5,)), "image_data": (S, (3, R, R))})
    keys = ["joint_command_history", "rotation"]
    g = torch.Generator().manual_seed(14)
    for tick in range(12):
        r = torch.randn(B, T, 5, generator=g)
        frames = torch.rand(B, 2, 3, R, R, generator=g)
        s.push_rotation(r.cuda()); host.append("rotation", r)
        s.push_image(frames.cuda()); host.append("image_data", frames)
        x_T = torch.randn(B, T, J, generator=g)
        batch = host.batch(game_state=False)
        _check_windows(s, host, keys)
        with torch.no_grad():
            tokens = model.image_sequence_encoder.image_encoder(batch["image_data"].cuda())
        err_tok = rel_err(s.windows()["image_tokens"], tokens)
        traj = s.step(x_T.cuda())
        err = rel_err(traj, _reference_tick(model, batch, x_T))
        print(f"image shape, tick {tick}: token window rel err {err_tok:.3e}, trajectory rel err {err:.3e}")
        assert err_tok < TOKEN_TOL, (tick, err_tok)
        assert err < TOL, (tick, err)
        host.append("joint_command_history", traj)
    _check_windows(s, host, keys)
    with pytest.raises(RuntimeError, match="switched off"):
        s.push_joint_state(torch.zeros(B, J, device="cuda"))


# ---- 3. only new frames reach the backbone -------------------------------------------------
def test_only_new_frames_reach_the_backbone(image_model, monkeypatch):
    from soccerdiffusion_amd import ops
    from soccerdiffusion_amd.session import PolicySession

    model, params = image_model
    B, R = 2, 64
    s = PolicySession(model, num_inference_steps=4, batch=B, hyperparams=params)
    seen = []
    stem = ops.stem_conv_bn_relu_pool

    def counting(x, *a, **kw):
        seen.append(int(x.shape[0]))
        return stem(x, *a, **kw)

    monkeypatch.setattr(ops, "stem_conv_bn_relu_pool", counting)
    g = torch.Generator().manual_seed(15)
    s.push_image(torch.rand(B, 2, 3, R, R, generator=g).cuda())     # k = 2 frames in one push
    assert seen == [2 * B]
    s.push_image(torch.rand(B, 3, R, R, generator=g).cuda())        # one frame, twice
    s.push_image(torch.rand(B, 1, 3, R, R, generator=g).cuda())
    assert seen == [2 * B, B, B]
    del seen[:]
    s.step()
    s.step()
    assert seen == []                                               # a tick never runs the backbone
    with torch.no_grad():                                           # (the counter does see the full-window route)
        model.encode_input_data({"joint_command_history": torch.zeros(B, 100, 20, device="cuda"), "rotation": torch.zeros(B, 100, 5, device="cuda"),
                                 "image_data": torch.zeros(B, 10, 3, R, R, device="cuda")})
    assert seen == [10 * B]


# ---- 4. distilled route --------------------------------------------------------------------
def test_distilled_route_is_one_forward_at_t0(default_model):
    from soccerdiffusion_amd import ops
    from soccerdiffusion_amd.session import PolicySession

    model, _, _ = default_model
    B, T, J = 3, 10, 20
    s = PolicySession(model, batch=B, distilled=True)
    assert PolicySession(model, batch=B, hyperparams={"distilled_decoder": True}).distilled and not PolicySession(model, batch=B).distilled
    host = HostNode(B, {"joint_command_history": (100, (J,)), "rotation": (100, (4,)), "joint_state": (100, (J,))})
    g = torch.Generator().manual_seed(16)
    for tick in range(2):
        q, r = (torch.rand(B, T, J, generator=g) - 0.5) * 2 * np.pi, torch.randn(B, T, 4, generator=g)
        s.push_joint_state(q.cuda()); host.append("joint_state", q)
        s.push_rotation(r.cuda()); host.append("rotation", r)
        x_T = torch.randn(B, T, J, generator=g).cuda()
        traj = s.step(x_T)
        with torch.no_grad():
            ctx = model.encode_input_data({k: v.cuda().contiguous() for k, v in host.batch().items()})
            x = model.forward_with_context(ctx, x_T, torch.zeros(B, device="cuda"))
            want = ops.normalize(x.contiguous(), model.mean, model.std, inverse=True) - np.pi
        assert rel_err(traj, want) < TOL
        host.append("joint_command_history", traj)


# ---- 5. stale weights ----------------------------------------------------------------------
def test_stale_weights_raise_until_reset(image_model):
    from soccerdiffusion_amd.session import PolicySession
    from soccerdiffusion_amd.training import FusedAdamW

    from soccerdiffusion_amd import cli

    shared, params = image_model
    model = cli.build_model(params).cuda().eval()          # this test changes weights: a model of its own
    model.load_state_dict(shared.state_dict())
    B, R = 2, 64
    frames = torch.rand(B, 3, R, R, generator=torch.Generator().manual_seed(17)).cuda()
    opt = FusedAdamW(model.parameters(), lr=1e-3)   # re-points the parameters into its flat buffer: before the session is built
    s = PolicySession(model, num_inference_steps=4, batch=B, hyperparams=params)
    s.push_image(frames)
    first = s.step()
    # a plain in-place update of a decoder parameter
    with torch.no_grad():
        model.diffusion_action_generator.fc_out.bias.add_(0.25)
    with pytest.raises(RuntimeError, match=r"reset\(\)"):
        s.step()
    with pytest.raises(RuntimeError, match=r"reset\(\)"):
        s.push_image(frames)
    s.reset()
    s.push_image(frames)
    second = s.step()
    assert torch.isfinite(second).all() and not torch.equal(first, second)
    # ... of a backbone parameter
    with torch.no_grad():
        model.image_sequence_encoder.image_encoder.encoder.conv1.weight.mul_(1.01)
    with pytest.raises(RuntimeError, match=r"reset\(\)"):
        s.push_image(frames)
    s.reset()
    s.push_image(frames)
    # one FusedAdamW step: the flat buffer is rewritten by a kernel, no version counter moves
    opt.flat_grad.fill_(0.01)
    opt.step()
    with pytest.raises(RuntimeError, match=r"reset\(\)"):
        s.step()
    with pytest.raises(RuntimeError, match=r"reset\(\)"):
        s.push_image(frames)
    s.reset()
    s.push_image(frames)
    assert torch.isfinite(s.step()).all()
    # and a model put back into train() mode is refused
    model.train()
    with pytest.raises(RuntimeError, match=r"train\(\) mode"):
        s.step()
    model.eval()


# ---- 6. inputs and outputs -----------------------------------------------------------------
def test_inputs_are_only_read_and_outputs_are_fresh(image_model):
    from soccerdiffusion_amd.session import PolicySession

    model, params = image_model
    B, T, J, R = 2, 10, 20, 64
    s = PolicySession(model, num_inference_steps=4, batch=B, hyperparams=params, seed=3)
    g = torch.Generator().manual_seed(18)
    r, frames, x_T = torch.randn(B, T, 5, generator=g).cuda(), torch.rand(B, 2, 3, R, R, generator=g).cuda(), torch.randn(B, T, J, generator=g).cuda()
    keep = [t.clone() for t in (r, frames, x_T)]
    s.push_rotation(r)
    s.push_image(frames)
    a = s.step(x_T)
    a_copy = a.clone()
    b = s.step(x_T)
    for t, k in zip((r, frames, x_T), keep):
        assert _same_bits(t, k)
    assert a.data_ptr() != b.data_ptr() and _same_bits(a, a_copy)
    assert not torch.equal(a, b)        # the action history moved between the ticks
    # the session's own generator: the same seed gives the same ticks
    runs = []
    for _ in range(2):
        s.reset()
        s.push_rotation(r)
        s.push_image(frames)
        runs.append([s.step(), s.step()])
    assert _same_bits(runs[0][0], runs[1][0]) and _same_bits(runs[0][1], runs[1][1])


# ---- 7. graph replay -------------------------------------------------------------------------
def test_graph_replay_equals_eager_ticks_bitwise(image_model, default_model):
    """Ten ticks with use_graph=True (windows, encoders and rollout replayed from one hipGraph) equal ten eager ticks bit for bit, on both
    shapes; after reset() the graph is captured again on the new rings."""
    from soccerdiffusion_amd.session import PolicySession

    for (model, params), B, rot in ((image_model, 2, 5), (default_model[::2], 3, 4)):
        images = params["use_images"]
        eager = PolicySession(model, num_inference_steps=30, batch=B, hyperparams=params, seed=9)
        graphed = PolicySession(model, num_inference_steps=30, batch=B, hyperparams=params, seed=9, use_graph=True)
        for round_ in range(2):
            g = torch.Generator().manual_seed(19 + round_)
            for tick in range(10 if round_ == 0 else 3):
                r = torch.randn(B, 10, rot, generator=g).cuda()
                q = (torch.rand(B, 10, 20, generator=g) - 0.5).cuda()
                frames = torch.rand(B, 2, 3, 64, 64, generator=g).cuda()
                x_T = torch.randn(B, 10, 20, generator=g).cuda() if tick % 2 else None     # the sessions' own generators as well
                out = []
                for s in (eager, graphed):
                    s.push_rotation(r)
                    if images:
                        s.push_image(frames)
                    else:
                        s.push_joint_state(q)
                    out.append(s.step(x_T))
                assert _same_bits(out[0], out[1]), (B, round_, tick)
                assert torch.isfinite(out[0]).all()
            we, wg = eager.windows(), graphed.windows()
            assert all(_same_bits(we[k], wg[k]) for k in we if k != "game_state")
            eager.reset(); graphed.reset()
    with pytest.raises(ValueError, match="distilled"):
        PolicySession(default_model[0], batch=1, distilled=True, use_graph=True)


# ---- the image encoder without a sequence encoder ------------------------------------------
def test_image_tokens_without_sequence_encoder():
    """SequenceEncoderType.NONE: the per-frame tokens are the context rows as they are; the ring length comes from the hyperparameters."""
    from soccerdiffusion_amd.session import PolicySession

    params = dict(TINY, hidden_dim=128, use_images=True, image_context_length=4, image_resolution=64, image_use_final_avgpool=True,
                  image_sequence_encoder_type="none", use_joint_states=False, trajectory_prediction_length=10)
    torch.manual_seed(1)
    model, _ = _synthetic_model(params)
    B, T, J, R = 2, 10, 20, 64
    with pytest.raises(ValueError, match="image_resolution"):
        PolicySession(model, batch=B)
    s = PolicySession(model, num_inference_steps=10, batch=B, hyperparams=params)
    host = HostNode(B, {"joint_command_history": (20, (J,)), "rotation": (20, (4,)), "image_data": (4, (3, R, R))})
    g = torch.Generator().manual_seed(20)
    for tick in range(4):      # two frames per tick into four slots: the token ring wraps
        r, frames = torch.randn(B, T, 4, generator=g), torch.rand(B, 2, 3, R, R, generator=g)
        s.push_rotation(r.cuda()); host.append("rotation", r)
        s.push_image(frames.cuda()); host.append("image_data", frames)
        x_T = torch.randn(B, T, J, generator=g)
        batch = host.batch()
        with torch.no_grad():
            tokens = model.image_sequence_encoder(batch["image_data"].cuda())
        assert rel_err(s.windows()["image_tokens"], tokens) < TOKEN_TOL
        traj = s.step(x_T.cuda())
        assert rel_err(traj, _reference_tick(model, batch, x_T, steps=10)) < TOL
        host.append("joint_command_history", traj)


def test_swin_image_encoder_tokens_are_cached():
    """push_image runs whatever image encoder the model holds: Swin-T under a sequence encoder, three-token ring, four ticks."""
    from soccerdiffusion_amd.session import PolicySession

    params = dict(TINY, hidden_dim=128, use_images=True, image_context_length=3, image_resolution=64, image_use_final_avgpool=True,
                  image_encoder_type="swin_transformer_tiny", use_joint_states=False, use_imu=False, trajectory_prediction_length=10)
    torch.manual_seed(2)
    model, _ = _synthetic_model(params)
    B, T, J, R = 2, 10, 20, 64
    s = PolicySession(model, num_inference_steps=10, batch=B, hyperparams=params)
    host = HostNode(B, {"joint_command_history": (20, (J,)), "image_data": (3, (3, R, R))})
    g = torch.Generator().manual_seed(21)
    for tick in range(4):
        frames = torch.rand(B, 2, 3, R, R, generator=g)
        s.push_image(frames.cuda()); host.append("image_data", frames)
        x_T = torch.randn(B, T, J, generator=g)
        batch = host.batch()
        with torch.no_grad():
            tokens = model.image_sequence_encoder.image_encoder(batch["image_data"].cuda())
        assert rel_err(s.windows()["image_tokens"], tokens) < TOKEN_TOL
        traj = s.step(x_T.cuda())
        assert rel_err(traj, _reference_tick(model, batch, x_T, steps=10)) < TOL
        host.append("joint_command_history", traj)


# ---- 8. command line -----------------------------------------------------------------------
def test_cli_rollout_from_a_trained_checkpoint(tmp_path):
    import yaml
    from test_gpu_cli import CFG, _run

    cfg = tmp_path / "cfg.yaml"
    cfg.write_text(yaml.safe_dump(dict(CFG, epochs=1)))
    ckpt = tmp_path / "model.pth"
    r = _run("train", "-c", str(cfg), "-o", str(ckpt), "--synthetic", "128")
    assert r.returncode == 0, r.stderr[-2000:]
    outs = []
    for name in ("a.pt", "b.pt"):
        r = _run("rollout", str(ckpt), "--synthetic", "3", "--ticks", "4", "--steps", "10", "--seed", "5", "-o", str(tmp_path / name))
        assert r.returncode == 0, r.stderr[-2000:]
        outs.append(torch.load(tmp_path / name, weights_only=True))
    traj = outs[0]["trajectories"]
    assert traj.shape == (4, 3, CFG["trajectory_prediction_length"], CFG["num_joints"]) and torch.isfinite(traj).all()
    assert not torch.equal(traj[0], traj[1])
    assert _same_bits(traj, outs[1]["trajectories"])
    r = _run("rollout", str(ckpt), "--ticks", "2", "-o", str(tmp_path / "c.pt"))
    assert r.returncode != 0 and "--synthetic" in r.stderr
    assert os.path.exists(tmp_path / "a.pt") and not os.path.exists(tmp_path / "c.pt")
