"""Gradient-norm clipping and the non-finite guard, the parts that need no GPU: the reference definition (tests/clip_ref.py) against
``torch.nn.utils.clip_grad_norm_``, the new entry points in the header, in _lib.SIGNATURES and in the built library, their argument errors
without a device, the command-line flag and the optimizer's argument check."""

import ctypes as C
import math
import os
import re

import pytest
import torch

import clip_ref
from conftest import REPO

NEW = {"sd_grad_norm_workspace_doubles": 0, "sd_grad_norm": 7, "sd_adamw_clip_step": 15, "sd_adamw_clip_step_dev": 10}
SPLITS = (1000, 37, 4096, 1, 2867)   # the flat gradient as several parameters


@pytest.fixture(scope="module")
def lib():
    from soccerdiffusion_amd import build

    build.build()
    from soccerdiffusion_amd import _lib

    return _lib


def _flat(scale, seed=0):
    return torch.randn(sum(SPLITS), generator=torch.Generator().manual_seed(seed)) * scale


def _torch_clipped(flat, max_norm):
    params = [torch.nn.Parameter(torch.zeros(k)) for k in SPLITS]
    for p, chunk in zip(params, flat.split(SPLITS)):
        p.grad = chunk.clone()
    total = torch.nn.utils.clip_grad_norm_(params, max_norm)
    return torch.cat([p.grad for p in params]), total


# ---- 1. the reference definition against torch's utility ----------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [1e-3, 1.0, 30.0])
def test_reference_equals_clip_grad_norm_when_it_binds(scale):
    """torch sums the squares in fp32 and per parameter; the reference in fp64 over the flat buffer.  The coefficient is ONE scalar, so the
    clipped gradients differ by the rounding of two fp32 norms (and of the division): 2e-6 relative."""
    flat = _flat(scale)
    norm, _, ok = clip_ref.norm_coef(flat, math.inf)
    max_norm = 0.5 * float(norm)
    norm, coef, ok = clip_ref.norm_coef(flat, max_norm)
    assert ok and float(coef) < 1.0
    want, total = _torch_clipped(flat, max_norm)
    got = flat * coef
    rel = float(((got - want).double().abs() / want.double().abs().clamp_min(1e-300)).max())
    print(f"scale {scale}: norm {float(norm):.9g} (torch {float(total):.9g}), coef {float(coef):.9g}, max relative difference {rel:.3e}")
    assert abs(float(total) - float(norm)) <= 2e-6 * float(norm)
    assert rel <= 2e-6
    # the clipped norm is max_norm norm / (norm + 1e-6) (torch's 1e-6), to the roundings of coef and of the products (2^-24 each)
    want_norm = max_norm * float(norm) / (float(norm) + 1e-6)
    assert abs(float(got.double().norm()) - want_norm) <= 2.0 ** -22 * want_norm


def test_reference_keeps_the_bits_below_max_norm():
    flat = _flat(1e-3, seed=1)
    norm, coef, ok = clip_ref.norm_coef(flat, 2.0 * float(clip_ref.norm_coef(flat, math.inf)[0]))
    assert ok and float(coef) == 1.0
    want, _ = _torch_clipped(flat, 2.0 * float(norm))
    assert torch.equal(flat * coef, flat) and torch.equal(want, flat)
    assert float(clip_ref.norm_coef(flat, math.inf)[1]) == 1.0                       # inf: guard and norm only
    assert float(clip_ref.norm_coef(torch.zeros(5), 1.0)[1]) == 1.0                  # norm 0
    for bad in (math.nan, math.inf):
        g = flat.clone()
        g[3] = bad
        assert clip_ref.norm_coef(g, 1.0)[1:] == (None, False)
    big, small = clip_ref.norm_coef(flat * 1e20, 1.0), clip_ref.norm_coef(flat * 1e-25, 1.0)   # squares leave fp32's range, not fp64's
    assert big[2] and math.isfinite(float(big[0])) and float(small[0]) > 0.0


def test_reference_adamw_equals_torch_adamw():
    n, hyper = 513, dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=1e-2)
    g = torch.Generator().manual_seed(2)
    p0 = torch.randn(n, generator=g)
    tp = torch.nn.Parameter(p0.clone())
    topt = torch.optim.AdamW([tp], lr=hyper["lr"])
    p, m, v = p0.clone(), torch.zeros(n), torch.zeros(n)
    for step in range(1, 4):
        grad = torch.randn(n, generator=g)
        max_norm = 0.5 * float(clip_ref.norm_coef(grad, math.inf)[0])
        _, coef, ok = clip_ref.clipped_adamw(p, grad, m, v, max_norm, step=step, **hyper)
        assert ok and float(coef) < 1.0
        tp.grad = grad * coef
        topt.step()
        assert torch.equal(p, tp.detach()) and torch.equal(m, topt.state[tp]["exp_avg"]) and torch.equal(v, topt.state[tp]["exp_avg_sq"])
    before = (p.clone(), m.clone(), v.clone())
    grad[0] = math.nan
    assert clip_ref.clipped_adamw(p, grad, m, v, 1.0, step=4, **hyper)[2] is False
    assert torch.equal(p, before[0]) and torch.equal(m, before[1]) and torch.equal(v, before[2])


# ---- 2. exports ---------------------------------------------------------------------------------------------------------------------------
def test_new_entry_points_are_declared_registered_and_exported(lib):
    with open(os.path.join(REPO, "include", "soccerdiffusion_hip.h")) as f:
        header = f.read()
    h = lib.load()
    for name, nargs in NEW.items():
        args = re.search(r"^int " + name + r"\((.*?)\);", header, re.M | re.S).group(1)
        count = 0 if args.strip() == "void" else len(args.split(","))
        assert count == nargs == len(lib.SIGNATURES[name][1]), name
        assert getattr(h, name) is not None
    assert "#define SD_ABI_VERSION 1" in header and h.sd_abi_version() == 1   # additive: the version stays
    assert lib.SIGNATURES["sd_grad_norm"][1][5] is C.c_float
    # the clip forms: their neighbours' arguments, ema nullable in the fifth place, clip2 in front of the stream
    ema = lib.SIGNATURES["sd_adamw_ema_step"][1]
    assert lib.SIGNATURES["sd_adamw_clip_step"][1] == ema[:-1] + [C.c_void_p] + ema[-1:]
    ema_dev = lib.SIGNATURES["sd_adamw_ema_step_dev"][1]
    assert lib.SIGNATURES["sd_adamw_clip_step_dev"][1] == ema_dev[:-1] + [C.c_void_p] + ema_dev[-1:]
    assert h.sd_grad_norm_workspace_doubles() >= 256 and h.sd_grad_norm_workspace_doubles() % 2 == 0


def test_new_entry_points_reject_bad_arguments_without_gpu(lib):
    """SD_E_BADARG before anything is launched: the pointers are host memory, a launch on them could not succeed."""
    h = lib.load()
    buf = lambda n=64: C.cast((C.c_float * n)(), C.c_void_p)   # noqa: E731
    g, ws, clip, skipped = buf(), C.cast((C.c_double * 1024)(), C.c_void_p), buf(2), C.cast((C.c_int * 1)(), C.c_void_p)
    for args in ((None, 64, ws, clip, skipped, 1.0), (g, 64, None, clip, skipped, 1.0), (g, 64, ws, None, skipped, 1.0),
                 (g, 64, ws, clip, None, 1.0), (g, 0, ws, clip, skipped, 1.0), (g, -3, ws, clip, skipped, 1.0),
                 (g, 64, ws, clip, skipped, -1.0), (g, 64, ws, clip, skipped, -0.5), (g, 64, ws, clip, skipped, math.nan)):
        assert h.sd_grad_norm(*args, None) == -1, args
        assert b"sd_grad_norm" in h.sd_last_error()
    p, m, v, ema, hyper, w = buf(), buf(), buf(), buf(), buf(8), buf(1)
    ok = dict(p=p, g=g, m=m, v=v, ema=ema, n=64, step=1, ema_weight=0.5, clip=clip, hyper=hyper, w=w)

    def host(**kw):
        a = dict(ok, **kw)
        return h.sd_adamw_clip_step(a["p"], a["g"], a["m"], a["v"], a["ema"], a["n"], 1e-3, 0.9, 0.999, 1e-8, 1e-2, a["step"], a["ema_weight"],
                                    a["clip"], None)

    def dev(**kw):
        a = dict(ok, **kw)
        return h.sd_adamw_clip_step_dev(a["p"], a["g"], a["m"], a["v"], a["ema"], a["n"], a["hyper"], a["w"], a["clip"], None)

    for bad in (dict(p=None), dict(g=None), dict(m=None), dict(v=None), dict(clip=None), dict(n=0), dict(n=-1)):
        assert host(**bad) == -1 and b"sd_adamw_clip_step:" in h.sd_last_error(), bad
        assert dev(**bad) == -1 and b"sd_adamw_clip_step_dev" in h.sd_last_error(), bad
    assert host(step=0) == -1 and host(ema_weight=1.5) == -1 and host(ema_weight=math.nan) == -1
    assert dev(hyper=None) == -1 and dev(w=None) == -1   # (with an EMA its weight is an operand; without one it is not read)


def test_bindings_check_their_arguments():
    from soccerdiffusion_amd import ops

    cpu = torch.zeros(8)
    for bad in (-1.0, math.nan, -math.inf):
        with pytest.raises(ValueError, match="max_norm"):
            ops.grad_norm(cpu, torch.zeros(1024, dtype=torch.float64), torch.zeros(2), torch.zeros(1, dtype=torch.int32), bad)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.grad_norm(cpu, torch.zeros(1024, dtype=torch.float64), torch.zeros(2), torch.zeros(1, dtype=torch.int32), 1.0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.adamw_clip_step(cpu, cpu, cpu, cpu, None, torch.zeros(2), 1e-3, 0.9, 0.999, 1e-8, 1e-2, 1)
    with pytest.raises(ValueError, match="ema_weight"):
        ops.adamw_clip_step_dev(cpu, cpu, cpu, cpu, cpu, torch.zeros(2), torch.zeros(7))
    assert ops.grad_norm_workspace_doubles() >= 256


# ---- 3. the optimizer's argument ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [-1.0, math.nan, -math.inf])
def test_optimizer_refuses_a_bad_max_grad_norm_before_any_device_work(bad):
    from soccerdiffusion_amd import training

    p = torch.nn.Parameter(torch.zeros(4, 4))   # a CPU parameter: nothing here can reach a device
    with pytest.raises(ValueError, match="max_grad_norm"):
        training.FusedAdamW([p], max_grad_norm=bad)
    assert p.grad is None   # refused before the parameter was re-pointed to a flat buffer


# ---- 4. the command line --------------------------------------------------------------------------------------------------------------------
def _parse(*argv):
    from soccerdiffusion_amd import cli

    return cli.build_parser().parse_args(list(argv))


@pytest.mark.parametrize("command", [("train", "-c", "cfg.yaml"), ("distill", "cfg.yaml", "teacher.pth")])
def test_parser_takes_clip_grad_norm(command, capsys):
    assert _parse(*command).clip_grad_norm is None
    assert _parse(*command, "--clip-grad-norm", "1.0").clip_grad_norm == 1.0
    assert _parse(*command, "--clip-grad-norm", "0").clip_grad_norm == 0.0
    assert _parse(*command, "--clip-grad-norm", "inf").clip_grad_norm == math.inf
    for bad in ("-1", "nan", "-inf", "much"):
        with pytest.raises(SystemExit):
            _parse(*command, "--clip-grad-norm", bad)
        assert "--clip-grad-norm" in capsys.readouterr().err
