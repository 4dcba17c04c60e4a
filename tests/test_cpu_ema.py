"""Weight EMA without a GPU: the schedule of its update weights, the argument checks of the two fused entry points, the commands that
ask for EMA weights a checkpoint does not hold, and the flag's parsing."""

import pytest
import torch

from conftest import REPO  # noqa: F401  (sys.path side effect)


def _tiny_optimizer(**kw):
    from soccerdiffusion_amd import training

    torch.manual_seed(0)
    lin = torch.nn.Linear(4, 3)
    return lin, training.FusedAdamW(lin.parameters(), lr=1e-3, **kw)


def test_schedule_with_warmup():
    _, opt = _tiny_optimizer(ema_decay=0.9999)
    assert opt.flat_ema is not None and torch.equal(opt.flat_ema, opt.flat_param) and opt.flat_ema.data_ptr() != opt.flat_param.data_ptr()
    assert opt.ema_weight_for_step(0) == pytest.approx(1 - 1 / 10, abs=1e-15)
    assert opt.ema_weight_for_step(1) == pytest.approx(1 - 2 / 11, abs=1e-15)
    assert opt.ema_weight_for_step(9) == pytest.approx(1 - 10 / 19, abs=1e-15)
    # (1 + t) / (10 + t) reaches 0.9999 at t = 89 990: one update earlier the warmup still rules, from there on the cap does
    assert opt.ema_weight_for_step(89_989) == pytest.approx(9 / 89_999, rel=1e-9)
    assert opt.ema_weight_for_step(89_989) > 1e-4 * (1 + 1e-6)
    assert opt.ema_weight_for_step(89_990) == pytest.approx(1e-4, rel=1e-9)
    assert opt.ema_weight_for_step(10 ** 7) == 1 - 0.9999
    # a small decay caps at once
    assert _tiny_optimizer(ema_decay=0.05)[1].ema_weight_for_step(0) == 0.95


def test_schedule_without_warmup_and_off():
    _, opt = _tiny_optimizer(ema_decay=0.9999, ema_warmup=False)
    assert [opt.ema_weight_for_step(t) for t in (0, 1, 9, 89_989, 89_990)] == [1 - 0.9999] * 5
    assert opt.ema_state() == {"decay": 0.9999, "warmup": False, "num_updates": 0}
    _, off = _tiny_optimizer()
    assert off.flat_ema is None and off.ema_decay is None
    with pytest.raises(RuntimeError, match="no EMA"):
        off.ema_weight_for_step(0)
    with pytest.raises(RuntimeError, match="no EMA"):
        off.ema_state_dict(torch.nn.Linear(2, 2))
    for bad in (0.0, 1.0, -0.5, 1.5):
        with pytest.raises(ValueError, match="ema_decay"):
            _tiny_optimizer(ema_decay=bad)


def test_ema_state_dict_and_exchange_on_host_buffers():
    """The plumbing around the kernel, which torch does: EMA views for owned tensors, live ones for the rest; the exchange restores."""
    lin, opt = _tiny_optimizer(ema_decay=0.9)
    holder = torch.nn.Module()
    holder.lin, holder.frozen = lin, torch.nn.Parameter(torch.ones(2), requires_grad=False)
    holder.register_buffer("mean", torch.full((3,), 7.0))
    opt.flat_ema.mul_(2.0)
    sd = opt.ema_state_dict(holder)
    assert set(sd) == set(holder.state_dict())
    assert torch.equal(sd["lin.weight"], 2 * lin.weight) and torch.equal(sd["lin.bias"], 2 * lin.bias)
    assert sd["mean"].data_ptr() == holder.mean.data_ptr() and sd["frozen"].data_ptr() == holder.frozen.data_ptr()
    p0, e0 = opt.flat_param.clone(), opt.flat_ema.clone()
    with pytest.raises(KeyError):
        with opt.ema_weights():
            assert torch.equal(opt.flat_param, e0) and torch.equal(opt.flat_ema, p0) and torch.equal(lin.weight.reshape(-1), e0[:12])
            raise KeyError("inside")
    assert torch.equal(opt.flat_param, p0) and torch.equal(opt.flat_ema, e0)
    # resume plumbing
    lin2, opt2 = _tiny_optimizer(ema_decay=0.9)
    holder2 = torch.nn.Module()
    holder2.lin, holder2.frozen = lin2, torch.nn.Parameter(torch.zeros(2), requires_grad=False)
    holder2.register_buffer("mean", torch.zeros(3))
    opt2.load_ema_state_dict(holder2, {k: v.clone() for k, v in sd.items()}, 5)
    assert torch.equal(opt2.flat_ema, e0) and opt2.ema_updates == 5 and opt2.ema_state()["num_updates"] == 5


def test_argument_errors_without_gpu():
    from soccerdiffusion_amd import _lib, build

    build.build()
    h = _lib.load()
    x = 16   # any non-null address: the checks come before anything is read or launched
    assert h.sd_adamw_ema_step(x, x, x, x, None, 4, 1e-3, 0.9, 0.999, 1e-8, 1e-2, 1, 0.1, None) == -1
    assert b"sd_adamw_ema_step" in h.sd_last_error()
    for w in (-0.01, 1.01, float("nan")):
        assert h.sd_adamw_ema_step(x, x, x, x, x, 4, 1e-3, 0.9, 0.999, 1e-8, 1e-2, 1, w, None) == -1
    assert h.sd_adamw_ema_step_dev(x, x, x, x, None, 4, x, x, None) == -1
    assert b"sd_adamw_ema_step_dev" in h.sd_last_error()
    assert h.sd_adamw_ema_step_dev(x, x, x, x, x, 4, x, None, None) == -1
    assert h.sd_adamw_ema_step_dev(x, x, x, x, x, 4, None, x, None) == -1
    assert h.sd_abi_version() == 1


@pytest.fixture()
def plain_checkpoint(tmp_path):
    path = tmp_path / "plain.pth"
    torch.save({"model_state_dict": {}, "optimizer_state_dict": {}, "lr_scheduler_state_dict": {}, "hyperparams": {"num_joints": 4},
                "current_epoch": 0}, path)
    return str(path)


@pytest.mark.parametrize("argv,flag", [
    (["sample", "CKPT", "--ema"], "--ema"),
    (["rollout", "CKPT", "--synthetic", "2", "--ticks", "1", "--ema"], "--ema"),
    (["distill", "cfg.yaml", "CKPT", "--ema-teacher", "--synthetic", "8"], "--ema-teacher"),
])
def test_commands_that_want_ema_weights_refuse_a_checkpoint_without(plain_checkpoint, argv, flag, monkeypatch):
    from soccerdiffusion_amd import cli

    def no_gpu(*a, **k):
        raise AssertionError("the GPU was touched before the checkpoint was checked")

    for name in ("is_available", "set_device", "current_device", "init"):
        monkeypatch.setattr(torch.cuda, name, no_gpu)
    with pytest.raises(SystemExit) as e:
        cli.main([plain_checkpoint if a == "CKPT" else a for a in argv])
    msg = str(e.value)
    assert flag in msg and "ema_model_state_dict" in msg and plain_checkpoint in msg


def test_session_from_checkpoint_names_the_missing_key(plain_checkpoint):
    from soccerdiffusion_amd.session import PolicySession

    with pytest.raises(ValueError, match="ema_model_state_dict"):
        PolicySession.from_checkpoint(plain_checkpoint, ema=True)


@pytest.mark.parametrize("command", ["train", "distill"])
@pytest.mark.parametrize("value", ["1.0", "0", "-0.1", "abc"])
def test_ema_decay_outside_the_open_interval_is_refused(command, value, capsys):
    from soccerdiffusion_amd import cli

    argv = ["train", "-c", "cfg.yaml"] if command == "train" else ["distill", "cfg.yaml", "ckpt.pth"]
    with pytest.raises(SystemExit) as e:
        cli.main(argv + ["--synthetic", "8", "--ema-decay", value])
    assert e.value.code == 2 and "--ema-decay" in capsys.readouterr().err
