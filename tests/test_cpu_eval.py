"""Held-out evaluation, everything that needs no GPU: the split, the default loss grid, the report assembled from hand-made marginals, the
argument checks of the three commands (before any device call), the new exports."""

import math

import pytest
import torch

from soccerdiffusion_amd import cli, evaluation


@pytest.mark.parametrize("split", ["tail", "random"])
@pytest.mark.parametrize("n", [2, 3, 10, 101])
@pytest.mark.parametrize("fraction", [0.01, 0.5, 0.99])
def test_holdout_split_properties(n, fraction, split):
    train, val = evaluation.holdout_split(n, fraction, 5, split)
    assert train.dtype == val.dtype == torch.int64
    assert len(val) == min(n - 1, max(1, round(n * fraction))) and len(train) == n - len(val) >= 1
    for t in (train, val):
        assert torch.equal(t, t.sort().values)
    assert torch.equal(torch.cat([train, val]).sort().values, torch.arange(n))   # disjoint, and the union is the range
    again = evaluation.holdout_split(n, fraction, 5, split)
    assert torch.equal(again[0], train) and torch.equal(again[1], val)
    if split == "tail":
        assert torch.equal(val, torch.arange(n - len(val), n))


def test_holdout_split_sizes_and_seed():
    sizes = {(n, f): len(evaluation.holdout_split(n, f, 0)[1]) for n in (2, 3, 10) for f in (0.01, 0.5, 0.99)}
    assert sizes == {(2, 0.01): 1, (2, 0.5): 1, (2, 0.99): 1, (3, 0.01): 1, (3, 0.5): 2, (3, 0.99): 2, (10, 0.01): 1, (10, 0.5): 5, (10, 0.99): 9}
    a, b = evaluation.holdout_split(1000, 0.1, 1, "random")[1], evaluation.holdout_split(1000, 0.1, 2, "random")[1]
    assert not torch.equal(a, b) and not torch.equal(a, torch.arange(900, 1000))
    for bad in (0.0, 1.0, -0.1, float("nan"), True, "0.5"):
        with pytest.raises(ValueError):
            evaluation.holdout_split(10, bad, 0)
    with pytest.raises(ValueError):
        evaluation.holdout_split(10, 0.5, 0, "by-recording")
    with pytest.raises(ValueError):
        evaluation.holdout_split(1, 0.5, 0)


def test_default_grid():
    assert evaluation.default_timesteps(8) == [62, 187, 312, 437, 562, 687, 812, 937]
    assert evaluation.default_timesteps(1) == [500]
    assert evaluation.default_timesteps(1000) == list(range(1000))
    for bad in (0, 1001, 2.0, True):
        with pytest.raises(ValueError):
            evaluation.default_timesteps(bad)
    assert evaluation.check_timesteps([0, 999]) == [0, 999]
    for bad in ([], [-1], [1000], [1.5]):
        with pytest.raises(ValueError):
            evaluation.check_timesteps(bad)


def test_report_from_hand_made_marginals():
    """Two batches (two windows, then one), G = 2, T = 2, J = 3: every entry worked out by hand."""
    a = {"loss": torch.tensor([[1.0, 3.0], [2.0, 6.0]]), "err": torch.tensor([[4.0, 1.0], [9.0, 16.0]]),
         "row_err": torch.tensor([[[4.0, 4.0], [1.0, 1.0]], [[9.0, 9.0], [16.0, 16.0]]]),
         "joint_err": torch.tensor([[[4.0, 4.0, 4.0], [0.0, 1.0, 2.0]], [[9.0, 9.0, 9.0], [16.0, 16.0, 16.0]]]),
         "best": torch.tensor([1, 0], dtype=torch.int32), "medoid": torch.tensor([1, 1], dtype=torch.int32), "spread": torch.tensor([[1.0, 0.0], [4.0, 0.0]])}
    b = {"loss": torch.tensor([[3.0, 9.0]]), "err": torch.tensor([[2.0, 25.0]]), "row_err": torch.tensor([[[1.0, 3.0], [25.0, 25.0]]]),
         "joint_err": torch.tensor([[[2.0, 2.0, 2.0], [25.0, 25.0, 25.0]]]), "best": torch.tensor([0], dtype=torch.int32),
         "medoid": torch.tensor([0], dtype=torch.int32), "spread": torch.tensor([[0.0, 7.0]])}
    r = evaluation.assemble_report([a, b], timesteps=[250, 750], steps=3, draws=2, max_mode=3, angular=True)
    assert r["n_windows"] == 3
    assert r["val_loss_by_t"] == [[250, 2.0], [750, 6.0]] and r["val_loss"] == 4.0
    assert r["rmse_first_draw"] == math.sqrt((4 + 9 + 2) / 3)
    assert r["rmse_medoid"] == math.sqrt((1 + 16 + 2) / 3)          # err[c, medoid[c]]
    assert r["rmse_best_of_G"] == math.sqrt((1 + 9 + 2) / 3)
    assert r["rmse_by_row"] == [math.sqrt((1 + 16 + 1) / 3), math.sqrt((1 + 16 + 3) / 3)]
    assert r["rmse_by_joint"] == [math.sqrt((0 + 16 + 2) / 3), math.sqrt((1 + 16 + 2) / 3), math.sqrt((2 + 16 + 2) / 3)]
    assert r["spread"] == math.sqrt(12 / 6)
    assert (r["steps"], r["draws"], r["max_mode"], r["angular"]) == (3, 2, 3, True)
    assert r["rmse_best_of_G"] <= r["rmse_medoid"] and r["rmse_best_of_G"] <= r["rmse_first_draw"]
    import json

    assert json.loads(json.dumps(r)) == r   # plain floats, ints and lists
    # a distilled decoder predicts no noise
    r = evaluation.assemble_report([{**a, "loss": None}], timesteps=[250, 750], steps=1, draws=2, max_mode=3, angular=False)
    assert r["val_loss"] is None and r["val_loss_by_t"] is None and r["n_windows"] == 2 and r["angular"] is False


@pytest.mark.parametrize("argv", [
    ["train", "-c", "cfg.yaml", "--synthetic", "8", "--val-fraction", "0"],
    ["train", "-c", "cfg.yaml", "--synthetic", "8", "--val-fraction", "1"],
    ["train", "-c", "cfg.yaml", "--synthetic", "8", "--val-fraction", "0.5", "--val-draws", "0"],
    ["train", "-c", "cfg.yaml", "--synthetic", "8", "--val-fraction", "0.5", "--val-draws", "65"],
    ["train", "-c", "cfg.yaml", "--synthetic", "8", "--val-fraction", "0.5", "--val-every", "0"],
    ["distill", "cfg.yaml", "teacher.pth", "--synthetic", "8", "--val-fraction", "1.5"],
    ["distill", "cfg.yaml", "teacher.pth", "--synthetic", "8", "--val-fraction", "0.5", "--val-draws", "100"],
    ["evaluate", "ckpt.pth", "--synthetic", "8", "--val-fraction", "-0.25"],
    ["evaluate", "ckpt.pth", "--synthetic", "8", "--all", "--draws", "65"],
    ["evaluate", "ckpt.pth", "--synthetic", "8", "--all", "--timesteps", "10,1000"],
    ["evaluate", "ckpt.pth", "--synthetic", "8", "--all", "--timesteps", "-1"],
    ["evaluate", "ckpt.pth", "--synthetic", "8", "--all", "--timesteps", "a,b"],
    ["evaluate", "ckpt.pth", "--synthetic", "8", "--all", "--grid", "0"],
])
def test_bad_arguments_end_the_command_before_any_device_call(argv, monkeypatch):
    """None of the files exists and no device may be asked for: the argument check comes first."""
    def no_device(*a, **k):
        raise AssertionError("the device was touched before the arguments were checked")

    monkeypatch.setattr(torch.cuda, "is_available", no_device)
    monkeypatch.setattr(torch.cuda, "set_device", no_device)
    monkeypatch.setattr(torch, "load", no_device)
    with pytest.raises(SystemExit) as e:
        cli.main(argv)
    assert e.value.code not in (0, None)


def test_parser_keeps_the_old_commands_as_they_were():
    ap = cli.build_parser()
    tr = ap.parse_args(["train", "-c", "cfg.yaml", "--synthetic", "8"])
    assert tr.val_fraction is None and tr.val_split == "tail" and tr.val_every == 1 and tr.val_draws == 1 and tr.val_steps == 30 and tr.seed == 0
    ev = ap.parse_args(["evaluate", "ckpt.pth", "--synthetic", "8"])
    assert (ev.steps, ev.draws, ev.grid, ev.timesteps, ev.val_fraction, ev.val_split, ev.all, ev.ema, ev.seed) == (30, 1, 8, None, None, None, False, False, None)
    assert ap.parse_args(["sample", "ckpt.pth"]).seed == 0


def test_new_exports_and_signatures():
    import ctypes as C
    import os

    from soccerdiffusion_amd import _lib

    for name, n in (("sd_sampler_prepare_draws", 11), ("sd_sampler_eps_draws", 13), ("sd_eval_sqerr_rows", 6), ("sd_eval_trajectory_errors", 14)):
        assert len(_lib.SIGNATURES[name][1]) == n, name
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "soccerdiffusion_hip.h")).read()
    for name in ("sd_sampler_prepare_draws", "sd_sampler_eps_draws", "sd_eval_sqerr_rows", "sd_eval_trajectory_errors"):
        assert f"int {name}(" in header
    assert "#define SD_ABI_VERSION 1" in header   # additive: the version stays
    lib = _lib.load()
    buf = (C.c_float * 16)()
    # argument checks return SD_E_BADARG before any launch (no device needed)
    assert lib.sd_eval_sqerr_rows(None, buf, buf, 1, 1, None) == -1
    assert lib.sd_eval_sqerr_rows(buf, buf, buf, 0, 1, None) == -1 and lib.sd_eval_sqerr_rows(buf, buf, buf, 1, 0, None) == -1
    for Cn, G, T, J in ((0, 1, 1, 1), (1, 0, 1, 1), (1, 65, 1, 1), (1, 1, 0, 1), (1, 1, 1, 0), (1, 1, 1, 33)):
        assert lib.sd_eval_trajectory_errors(buf, buf, buf, buf, buf, None, None, None, Cn, G, T, J, 1, None) == -1, (Cn, G, T, J)
    assert lib.sd_eval_trajectory_errors(buf, buf, buf, buf, None, None, None, None, 1, 1, 1, 1, 1, None) == -1
