"""CPU-only checks of the closed-loop policy session (soccerdiffusion_amd/session.py, csrc/sd_session.hip): argument errors of the four
entry points without a device, the session's refusals, the ring plan of the shipped YAML shapes, and the angle-wrap specification the
windows kernel is written to."""

import ctypes as C

import numpy as np
import pytest
import torch

BASE = dict(action_context_length=100, trajectory_prediction_length=10, epochs=1, batch_size=4, lr=1e-4, train_denoising_timesteps=1000,
            image_context_length=10, imu_context_length=100, joint_state_context_length=100, num_normalization_samples=10, num_joints=20,
            use_images=True, image_sequence_encoder_type="transformer", image_encoder_type="resnet18", image_resolution=224,
            image_use_final_avgpool=False, num_image_sequence_encoder_layers=1, distill_teacher_inference_steps=30)
# the reference's five shipped YAMLs (ml/training/config/*.yaml), the values that shape the session
SHIPPED = {
    "default": dict(hidden_dim=128, use_action_history=True, num_action_history_encoder_layers=2, use_imu=True,
                    imu_orientation_embedding_method="quaternion", num_imu_encoder_layers=2, use_joint_states=True,
                    joint_state_encoder_layers=2, num_decoder_layers=4, use_gamestate=True, encoder_patch_size=1),
    "decoder_only": dict(hidden_dim=256, use_action_history=False, num_action_history_encoder_layers=2, use_imu=False,
                         imu_orientation_embedding_method="quaternion", num_imu_encoder_layers=2, use_joint_states=False,
                         joint_state_encoder_layers=2, use_images=False, num_decoder_layers=4, use_gamestate=False, encoder_patch_size=10),
    "larger_model": dict(hidden_dim=512, use_action_history=True, num_action_history_encoder_layers=4, use_imu=True,
                         imu_orientation_embedding_method="quaternion", num_imu_encoder_layers=4, use_joint_states=True,
                         joint_state_encoder_layers=4, num_decoder_layers=8, use_gamestate=True, encoder_patch_size=1),
    "larger_model_distill": dict(hidden_dim=512, use_action_history=True, num_action_history_encoder_layers=4, use_imu=True,
                                 imu_orientation_embedding_method="quaternion", num_imu_encoder_layers=4, use_joint_states=True,
                                 joint_state_encoder_layers=4, num_decoder_layers=8, use_gamestate=True, encoder_patch_size=1),
    "sim_scratch": dict(hidden_dim=256, use_action_history=True, num_action_history_encoder_layers=4, use_imu=True,
                        imu_orientation_embedding_method="five_dim", num_imu_encoder_layers=2, use_joint_states=False,
                        joint_state_encoder_layers=4, num_decoder_layers=6, use_gamestate=False, encoder_patch_size=5),
}


@pytest.fixture(scope="module")
def lib():
    from soccerdiffusion_amd import build

    build.build()
    from soccerdiffusion_amd import _lib

    return _lib


def test_session_entry_points_reject_null_pointers_without_gpu(lib):
    h = lib.load()
    assert h.sd_ring_push(None, None, None, None, 1, 10, 4, 1, None) == -1
    assert b"sd_ring_push" in h.sd_last_error()
    assert h.sd_ring_window(None, None, None, 1, 10, 4, None) == -1
    assert b"sd_ring_window" in h.sd_last_error()
    assert h.sd_session_windows(None, 1, 1, None) == -1
    assert b"sd_session_windows" in h.sd_last_error()
    views = (lib.RingView * 2)()   # two views of null pointers
    views[0].L = views[1].L = 10
    views[0].C = views[1].C = 4
    assert h.sd_session_windows(views, 2, 1, None) == -1
    assert h.sd_session_windows(views, 4, 1, None) == -1      # more than SD_SESSION_MAX_RINGS
    assert h.sd_session_commit(None, None, None, None, None, None, 1, 10, 20, 100, None) == -1
    assert b"sd_session_commit" in h.sd_last_error()
    # sizes are checked before any launch as well (a host buffer stands in for the pointers: nothing is launched)
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    assert h.sd_ring_push(p, p, p, None, 1, 0, 4, 1, None) == -1
    assert h.sd_ring_push(p, p, p, None, 1, 4, 4, -1, None) == -1
    assert h.sd_ring_window(p, p, p, 0, 4, 4, None) == -1
    assert h.sd_session_commit(p, p, p, p, p, p, 1, 0, 4, 4, None) == -1
    assert C.sizeof(lib.RingView) == 3 * 8 + 4 * 4


def test_session_refuses_cpu_and_train_mode_models():
    from soccerdiffusion_amd import cli
    from soccerdiffusion_amd.session import PolicySession

    params = {**BASE, **SHIPPED["sim_scratch"], "use_images": False}
    model = cli.build_model(params)
    with pytest.raises(RuntimeError, match=r"train\(\) mode"):
        PolicySession(model.train())
    with pytest.raises(RuntimeError, match="on the CPU"):
        PolicySession(model.eval())


def test_plan_of_the_shipped_yaml_shapes():
    """Context rows + the step token: default / larger_model(_distill) 100 + 100 + 100 (patch 1) + 10 image tokens + the game state
    = 311 + 1 (the 312 memory rows of DESIGN.md section 1), decoder_only 0 + 1, sim_scratch 20 + 20 (patch 5) + 10 = 50 + 1."""
    from soccerdiffusion_amd.session import PolicySession

    want = {"default": 311, "decoder_only": 0, "larger_model": 311, "larger_model_distill": 311, "sim_scratch": 50}
    for name, over in SHIPPED.items():
        params = {**BASE, **over}
        plan = PolicySession.plan(params)
        assert plan["context_rows"] == want[name] and plan["memory_rows"] == want[name] + 1, name
        assert plan["trajectory"] == (10, 20)
        d = params["hidden_dim"]
        if name == "decoder_only":
            assert plan["rings"] == {}
        elif name == "sim_scratch":
            assert plan["rings"] == {"joint_command_history": (100, 20), "rotation": (100, 5), "image_tokens": (10, d)}
        else:
            assert plan["rings"] == {"joint_command_history": (100, 20), "rotation": (100, 4), "joint_state": (100, 20), "image_tokens": (10, d)}


def wrap_spec(x: np.ndarray) -> np.ndarray:
    """The formula of csrc/sd_session.hip (wrap_angle) in numpy fp32."""
    assert x.dtype == np.float32
    three_pi, two_pi = np.float32(3 * np.pi), np.float32(2 * np.pi)
    a = x + three_pi
    r = np.fmod(a, two_pi)
    r = np.where((r != 0) & (r < 0), r + two_pi, r)
    assert a.dtype == np.float32 and r.dtype == np.float32
    return r


def test_angle_wrap_formula_equals_torch_bitwise():
    """(x + 3 * np.pi) % (2 * np.pi) of ros.py:266-273 as torch evaluates it on an fp32 CPU tensor, against the three-line fp32 formula
    the windows kernel implements - bit for bit, signed zeros included."""
    g = torch.Generator().manual_seed(5)
    pi = np.pi
    special = torch.tensor([0.0, -0.0, pi, -pi, 3 * pi, -3 * pi, 2 * pi, -2 * pi, 5 * pi, -5 * pi, 1e-30, -1e-30, 100.0, -100.0, 1e6, -1e6],
                           dtype=torch.float32)
    near = torch.tensor([-3 * pi, -pi, pi], dtype=torch.float64).repeat_interleave(41)
    near = (near + torch.arange(-20, 21, dtype=torch.float64).repeat(3) * 2.0 ** -21).float()   # fp32 neighbours of the wrap points
    x = torch.cat([special, near, (torch.rand(200_000, generator=g) - 0.5) * 8 * pi, torch.randn(50_000, generator=g) * 30])
    want = (x + 3 * np.pi) % (2 * np.pi)
    got = wrap_spec(x.numpy())
    assert want.dtype == torch.float32
    assert np.array_equal(got.view(np.int32), want.numpy().view(np.int32))
    assert float(want.min()) >= 0.0 and float(want.max()) <= float(np.float32(2 * np.pi))
