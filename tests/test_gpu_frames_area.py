"""The image feed's area-resampling kernel (ops.frames_area, csrc/sd_frames.hip) on the GPU: bit for bit against the numpy fp32
restatement of OpenCV's INTER_AREA paths (tests/test_cpu_frames_area.py) and against the host feed where that reproduces OpenCV,
the dataset's items and batches at default.yaml's image_resolution 224 against the reference's per-item query, and `cli train` /
`cli sample --db` with the image settings of the reference's default.yaml and sim_scratch.yaml."""

import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch
import yaml

from conftest import REPO
from test_cpu_frames_area import cv2_area_restated, frame_patterns, normalize_restated

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


def _bits(x) -> np.ndarray:
    x = x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else x
    return np.ascontiguousarray(x, dtype=np.float32).view(np.int32)


@pytest.fixture(scope="module")
def store():
    frames = np.stack(list(frame_patterns(3).values()))            # random, 0, 255, stripes, checkerboards
    return frames, torch.from_numpy(frames).to(DEV)


@pytest.mark.parametrize("R", [224, 200, 300, 479, 17, 1, 96, 7])
def test_kernel_is_bit_exact_against_the_restated_opencv_paths(store, R):
    from soccerdiffusion_amd import ops

    frames, dev_frames = store
    n = len(frames)
    index = torch.tensor([[0, 1, -1, 2], [3, 4, 0, -1], [-1, -1, 4, 3]], dtype=torch.int64, device=DEV)   # repeats and padding slots
    got = ops.frames_area(dev_frames, index, R)
    assert got.shape == (3, 4, 3, R, R) and got.dtype == torch.float32
    want = normalize_restated(np.stack([cv2_area_restated(f, R) for f in frames]))
    for (i, j), f in np.ndenumerate(index.cpu().numpy()):
        if f < 0:
            assert float(got[i, j].abs().max()) == 0.0
        else:
            assert np.array_equal(_bits(got[i, j]), _bits(want[f])), (R, i, j, f)
    # an index past the store is a zero frame too (no read outside the store)
    assert float(ops.frames_area(dev_frames, torch.tensor([n, 10**9], device=DEV), R).abs().max()) == 0.0


@pytest.mark.parametrize("R", [480, 240, 160, 120, 96])
def test_kernel_is_bit_identical_to_the_host_feed(store, R):
    from soccerdiffusion_amd import ops
    from soccerdiffusion_amd.dataset import SoccerDiffusionDataset

    frames, dev_frames = store
    host = SoccerDiffusionDataset._preprocess(types.SimpleNamespace(image_resolution=R), torch.from_numpy(frames))
    got = ops.frames_area(dev_frames, torch.arange(len(frames), device=DEV), R)
    assert np.array_equal(_bits(got), _bits(host)), R


def test_two_runs_give_identical_bytes(store):
    from soccerdiffusion_amd import ops

    _, dev_frames = store
    idx = torch.randint(-1, len(dev_frames), (64, 10), generator=torch.Generator().manual_seed(5)).to(DEV)
    a, b = ops.frames_area(dev_frames, idx, 224), ops.frames_area(dev_frames, idx, 224)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_bad_arguments_raise_value_error(store):
    from soccerdiffusion_amd import ops

    _, dev_frames = store
    idx = torch.zeros(2, dtype=torch.int64, device=DEV)
    bad = [
        (dev_frames.cpu(), idx, 224),                                   # frames on the host
        (dev_frames.float(), idx, 224),                                 # not uint8
        (dev_frames[:, :240], idx, 224),                                # not 480 x 480 frames (and a strided view)
        (dev_frames.reshape(-1, 480, 240, 6), idx, 224),                # not rgb8 rows
        (dev_frames, idx.int(), 224),                                   # int32 index
        (dev_frames, idx.cpu(), 224),                                   # index on the host
        (dev_frames, torch.zeros(2, 2, dtype=torch.int64, device=DEV)[:, 0], 224),   # strided index
        (dev_frames, idx, 0), (dev_frames, idx, 481), (dev_frames, idx, 224.0), (dev_frames, idx, True),
    ]
    for args in bad:
        with pytest.raises(ValueError):
            ops.frames_area(*args)
    with pytest.raises(ValueError):
        ops.frames_area(dev_frames, idx, 224, out=torch.empty(2, 3, 224, 223, device=DEV))
    assert ops.frames_area(dev_frames, torch.zeros(0, 10, dtype=torch.int64, device=DEV), 224).shape == (0, 10, 3, 224, 224)


def _reference_images_area(con, rid, stamp, F, fps, R):
    """query_image_data (dataset/pytorch.py:173-229) restated as tests/test_cpu_dataset.py does, with cv2.resize INTER_AREA restated for
    any R (tests/test_cpu_frames_area.py)."""
    ctx = (F + 1) / fps
    rows = con.execute("SELECT stamp, data FROM Image WHERE recording_id = ? AND stamp BETWEEN ? - ? AND ? ORDER BY stamp ASC",
                       (rid, stamp, ctx, stamp)).fetchall()
    rows = rows[-F:] if len(rows) > F else rows
    frames = [normalize_restated(cv2_area_restated(np.frombuffer(d, dtype=np.uint8).reshape(480, 480, 3), R)) for _, d in rows]
    stamps = [st for st, _ in rows]
    pad = F - len(frames)
    frames = [np.zeros((3, R, R), np.float32)] * pad + frames
    stamps = [stamp - ctx] * pad + stamps
    return np.asarray(stamps, np.float32), np.stack(frames).astype(np.float32)


@pytest.mark.parametrize("R", [224, 120])
def test_dataset_items_and_batches_on_the_device(tmp_path, R):
    from test_cpu_dataset import _make_db

    from soccerdiffusion_amd.dataset import SoccerDiffusionDataset

    con = _make_db(str(tmp_path / "db.sqlite3"))
    F, fps = 3, 2
    ds = SoccerDiffusionDataset(con, num_samples_imu=5, num_samples_joint_states=5, num_samples_joint_trajectory=5,
                                num_samples_joint_trajectory_future=4, sampling_rate=50, num_joints=22, use_images=True,
                                num_frames_video=F, max_fps_video=fps, image_resolution=R, device=DEV)
    assert ds._frames.is_cuda and ds._frames.shape == (11, 480, 480, 3) and ds._rec[2]["img"].data_ptr() == ds._frames[9].data_ptr()
    picks = [0, 20, 60, 100, 175, 176 + 3, 176 + 60, 20]     # start-up padding, both recordings, a repeat
    batch = ds.batch(torch.tensor(picks))
    assert batch["image_data"].shape == (len(picks), F, 3, R, R) and batch["image_data"].is_cuda
    for n, idx in enumerate(picks):
        for start, end, rid in ds.sample_boundaries:
            if start <= idx < end:
                break
        want_st, want = _reference_images_area(con, rid, (idx - start) / 50, F, fps, R)
        item = ds[idx]
        for got_st, got in ((item.image_stamps, item.image_data), (batch["image_stamps"][n], batch["image_data"][n])):
            assert np.allclose(got_st.cpu().numpy(), want_st, atol=1e-6)
            assert np.array_equal(_bits(got), _bits(want)), (R, idx)
    assert float(batch["image_data"][0].abs().max()) == 0.0
    # the rest of the batch is the host feed's
    host = SoccerDiffusionDataset(con, num_samples_imu=5, num_samples_joint_states=5, num_samples_joint_trajectory=5,
                                  num_samples_joint_trajectory_future=4, sampling_rate=50, num_joints=22, use_images=False)
    hb = host.batch(torch.tensor(picks))
    for k, v in hb.items():
        assert torch.equal(batch[k].cpu(), v), k
    if R == 120:   # a host dataset moved to the GPU afterwards takes the kernel as well
        moved = SoccerDiffusionDataset(con, num_samples_imu=5, num_samples_joint_states=5, num_samples_joint_trajectory=5,
                                       num_samples_joint_trajectory_future=4, sampling_rate=50, num_joints=22, use_images=True,
                                       num_frames_video=F, max_fps_video=fps, image_resolution=R).to(DEV)
        assert torch.equal(moved.batch(torch.tensor(picks))["image_data"], batch["image_data"])


# the image settings of the reference's default.yaml and sim_scratch.yaml (ml/training/config/), epochs 1
DEFAULT_YAML = dict(hidden_dim=128, action_context_length=100, trajectory_prediction_length=10, epochs=1, batch_size=64, lr=1e-4,
                    train_denoising_timesteps=1000, image_context_length=10, imu_context_length=100, joint_state_context_length=100,
                    num_normalization_samples=1000, num_joints=20, use_action_history=True, num_action_history_encoder_layers=2,
                    use_imu=True, imu_orientation_embedding_method="quaternion", num_imu_encoder_layers=2, use_joint_states=True,
                    joint_state_encoder_layers=2, use_images=True, image_sequence_encoder_type="transformer", image_encoder_type="resnet18",
                    image_resolution=224, image_use_final_avgpool=False, num_image_sequence_encoder_layers=1, num_decoder_layers=4,
                    distill_teacher_inference_steps=30, use_gamestate=True, encoder_patch_size=1)
SIM_SCRATCH_YAML = dict(DEFAULT_YAML, hidden_dim=256, batch_size=16, num_normalization_samples=100, num_action_history_encoder_layers=4,
                        imu_orientation_embedding_method="five_dim", use_joint_states=False, joint_state_encoder_layers=4,
                        num_decoder_layers=6, use_gamestate=False, encoder_patch_size=5)


def _run(*argv):
    env = dict(os.environ, PYTHONPATH=REPO, MIOPEN_FIND_MODE="FAST")
    return subprocess.run([sys.executable, "-m", "soccerdiffusion_amd.cli", *argv], cwd=REPO, env=env, capture_output=True, text=True)


@pytest.mark.timeout(900)
@pytest.mark.parametrize("cfg", [DEFAULT_YAML, SIM_SCRATCH_YAML], ids=["default", "sim_scratch"])
def test_cli_train_and_sample_from_database_at_224(tmp_path, cfg):
    from test_cpu_dataset import _make_db

    db = tmp_path / "db.sqlite3"
    _make_db(str(db)).close()
    path = tmp_path / "cfg.yaml"
    path.write_text(yaml.safe_dump(cfg))
    ckpt = tmp_path / "m.pth"
    r = _run("train", "-c", str(path), "-o", str(ckpt), "--db", str(db))
    assert r.returncode == 0, r.stderr[-3000:]
    losses = [float(l.split("Loss:")[1].split(",")[0]) for l in r.stdout.splitlines() if "Loss:" in l]
    assert losses and all(np.isfinite(losses))
    sd = torch.load(ckpt, weights_only=True)["model_state_dict"]
    fc = sd["image_sequence_encoder.image_encoder.encoder.fc.weight"]
    assert fc.shape == (cfg["hidden_dim"], 1568)    # 32 x 7 x 7: the no-avgpool head at 224 (a reference checkpoint's shape)
    r = _run("sample", str(ckpt), "--steps", "10", "--num_samples", "5", "-o", str(tmp_path / "s.pt"), "--db", str(db))
    assert r.returncode == 0, r.stderr[-3000:]
    out = torch.load(tmp_path / "s.pt", weights_only=True)["trajectories"]
    assert out.shape == (5, 10, 20) and torch.isfinite(out).all()
