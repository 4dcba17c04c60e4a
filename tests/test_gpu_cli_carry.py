"""``cli rollout --carry K --advance S`` end to end, in a child process of its own."""

import os
import subprocess
import sys

import pytest
import torch

from conftest import REPO
from test_gpu_cli import CFG
from test_gpu_session import _same_bits

pytestmark = pytest.mark.gpu


def test_cli_rollout_with_carry(tmp_path):
    from soccerdiffusion_amd import cli

    params = dict(CFG, trajectory_prediction_length=10)
    torch.manual_seed(3)
    model = cli.build_model(params)      # an untrained checkpoint: the command line is under test, not the policy
    ckpt = tmp_path / "model.pth"
    torch.save({"hyperparams": params, "model_state_dict": model.state_dict()}, ckpt)
    out = tmp_path / "carry.pt"
    r = subprocess.run([sys.executable, "-m", "soccerdiffusion_amd.cli", "rollout", str(ckpt), "--synthetic", "3", "--ticks", "4", "--steps", "4",
                        "--seed", "5", "--carry", "4", "--advance", "5", "-o", str(out)],
                       cwd=REPO, env=dict(os.environ, PYTHONPATH=REPO), capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    saved = torch.load(out, weights_only=True)
    assert saved["carry"] == 4 and saved["advance"] == 5
    traj = saved["trajectories"]
    assert traj.shape == (4, 3, 10, CFG["num_joints"]) and torch.isfinite(traj).all()
    for k in range(1, 4):      # every seam: the first 4 rows of a tick are rows 5 .. 8 of the tick before, bit for bit
        assert _same_bits(traj[k][:, :4], traj[k - 1][:, 5:9]), k
    bad = subprocess.run([sys.executable, "-m", "soccerdiffusion_amd.cli", "rollout", str(ckpt), "--synthetic", "1", "--ticks", "1", "--carry", "4",
                          "--advance", "7"], cwd=REPO, env=dict(os.environ, PYTHONPATH=REPO), capture_output=True, text=True, timeout=240)
    assert bad.returncode != 0 and "exceeds" in bad.stderr
