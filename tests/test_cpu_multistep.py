"""CPU-only checks of the second-order multistep solver (sd_ddim_sample_multistep, sd_multistep_step): ops.multistep_weights against the
reference's own float64 weights, the CPU reference tests/multistep_ref.py against oracle/ddim_ref.py and tests/hold_ref.py, what the second
order buys on the oracle denoiser in fp64, the new entry points in the header, in _lib.SIGNATURES and in the built library, their argument
errors without a device, and the Python-side validation that needs none."""

import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import hold_ref
import multistep_ref
from conftest import REPO
from oracle import ddim_ref
from oracle import denoiser_ref as ref
from test_cpu_pin import _toy_denoiser

NEW = ("sd_ddim_sample_multistep", "sd_multistep_step")


@pytest.fixture(scope="module")
def lib():
    from soccerdiffusion_amd import build

    build.build()
    from soccerdiffusion_amd import _lib

    return _lib


# ---- 1. weights --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [4, 5, 10, 30, 50])
def test_weights_equal_the_reference_to_one_ulp(n):
    from soccerdiffusion_amd import ops

    ts = ops.ddim_timesteps(n)
    assert ts == ddim_ref.timesteps(n).tolist()
    w = ops.multistep_weights(ts, ops.alphas_cumprod(), n)
    want = multistep_ref.weights(n)
    assert w.dtype == np.float32 and w.shape == (n,) and len(want) == n
    assert w[0] == 0 and w[-1] == 0 and want[0] == 0 and want[-1] == 0
    assert all(v < 0 for v in w[1:-1])                       # expm1(-h) < 0: the term extrapolates from x0 of the step before through x0
    for i in range(n):
        ulp = float(np.spacing(np.float32(abs(want[i])))) if want[i] else 0.0
        assert abs(float(w[i]) - want[i]) <= ulp, (i, float(w[i]), want[i])


def test_weights_need_the_consecutive_leading_grid():
    from soccerdiffusion_amd import ops

    acp = ops.alphas_cumprod()
    for bad in ([900, 700, 600], [900, 800, 800], [0, 100, 200], [900, 801]):
        with pytest.raises(ValueError, match="consecutive"):
            ops.multistep_weights(bad, acp, 10)
    # a tail of the grid is a grid (the first weight is 0 wherever it starts); a single step has no history at all
    w = ops.multistep_weights([300, 200, 100, 0], acp, 10)
    assert w[0] == 0 and w[-1] == 0 and w[1] != 0 and w[2] == ops.multistep_weights(ops.ddim_timesteps(10), acp, 10)[8]
    assert ops.multistep_weights([500], acp, 10).tolist() == [0.0]


# ---- 2. the reference itself ---------------------------------------------------------------------------------------------------------
def test_zero_weights_are_ddim_ref_and_an_empty_mask_ignores_known():
    B, T, J, n = 3, 10, 7, 5
    g = torch.Generator().manual_seed(3)
    x_T, known = torch.randn(B, T, J, generator=g), torch.randn(B, T, J, generator=g)
    den = _toy_denoiser(4, J)
    want = ddim_ref.sample(den, x_T, n)
    got, _, _ = multistep_ref.sample(den, x_T, None, None, n, [0.0] * n)
    assert len(got) == n and all(torch.equal(a, b) for a, b in zip(want, got))
    # zero weights with a mask: hold_ref.sample
    mask = torch.rand(B, T, J, generator=g) < 0.3
    for a, b in zip(hold_ref.sample(den, x_T, known, mask, n), multistep_ref.sample(den, x_T, known, mask, n, [0.0] * n)):
        assert all(torch.equal(u, v) for u, v in zip(a, b))
    # nonzero weights, nothing held: known is never read
    w = multistep_ref.weights(n)
    empty = torch.zeros(B, T, J, dtype=torch.bool)
    one = multistep_ref.sample(den, x_T, known, empty, n, w)[0]
    other = multistep_ref.sample(den, x_T, known * 3 + 1, empty, n, w)[0]
    none = multistep_ref.sample(den, x_T, None, None, n, w)[0]
    assert all(torch.equal(a, b) and torch.equal(a, c) for a, b, c in zip(one, other, none))
    assert not torch.equal(one[-1], want[-1]) and torch.equal(one[0], want[0])       # the first step is DDIM's, the rollout is not
    # held elements take the hold's value, exactly known at the end; the free ones read them
    got, held, _ = multistep_ref.sample(den, x_T, known, mask, n, w)
    assert all(torch.equal(x[mask], p[mask]) for x, p in zip(got, held)) and torch.equal(got[-1][mask], known[mask])
    assert not torch.equal(got[-1][~mask], one[-1][~mask])


# ---- 3. second order pays ---------------------------------------------------------------------------------------------------------------
def test_second_order_pays_on_the_oracle_denoiser_in_fp64():
    """DDIM and the 2M update on the same n leading-spaced steps against a 901-step DDIM solve (one timestep per step) from t = 900, all
    in fp64 on the oracle denoiser.  The bar is 1.5 at n = 10.  Measured: 2.74 at n = 10 (901-step fine solve from t = 900) and 2.44 at n = 5 (801 steps from t = 800)."""
    d, J, L, B, T, Mc = 64, 20, 1, 4, 10, 5
    sd = {k: v.double() for k, v in ref.synthetic_state_dict(d, J, L, seed=97).items()}
    g = torch.Generator().manual_seed(0)
    x_T = torch.randn(B, T, J, generator=g).double()
    ctx = torch.randn(B, Mc, d, generator=g).double()
    acp = ddim_ref.alphas_cumprod()

    def den(x, t):
        return ref.forward_with_context(sd, [ctx], x, torch.full((B,), t, dtype=torch.int64))

    ratios = {}
    for n in (10, 5):
        start = int(ddim_ref.timesteps(n)[0])      # 900 at n = 10 (the 901-step fine solve), 800 at n = 5: x_T is x at the first timestep
        fine = x_T
        for t in range(start, -1, -1):
            fine = ddim_ref.step(den(fine, t), t, fine, 1000, acp)
        first = ddim_ref.sample(den, x_T, n, acp)[-1]
        second = multistep_ref.sample(den, x_T, None, None, n, multistep_ref.weights(n, acp), acp)[0][-1]
        e1, e2 = float((first - fine).norm()), float((second - fine).norm())
        ratios[n] = e1 / e2
        print(f"n = {n}: {start + 1}-step fine solve; DDIM error {e1:.4e}, multistep error {e2:.4e}, ratio {ratios[n]:.2f}")
    assert ratios[10] >= 1.5, ratios


# ---- 4. exports ------------------------------------------------------------------------------------------------------------------------
def _declared(header):
    return set(re.findall(r"^(?:int|size_t|const char \*)\s*(sd_\w+)\(", header, re.M))


def test_new_entry_points_are_declared_registered_and_exported(lib):
    with open(os.path.join(REPO, "include", "soccerdiffusion_hip.h")) as f:
        header = f.read()
    declared = _declared(header)
    h = lib.load()
    for name in NEW:
        assert name in declared, name
        assert name in lib.SIGNATURES, name
        assert getattr(h, name) is not None
    assert "#define SD_ABI_VERSION 1" in header and h.sd_abi_version() == 1   # additive: the version stays
    # sd_ddim_sample_multistep = sd_ddim_sample_hold's arguments with the weights and the history in front of the stream
    hold = lib.SIGNATURES["sd_ddim_sample_hold"][1]
    assert lib.SIGNATURES["sd_ddim_sample_multistep"][1] == hold[:-1] + [lib.c_float_p, C.c_void_p] + hold[-1:]


def test_new_entry_points_reject_bad_arguments_without_gpu(lib):
    h = lib.load()
    p = C.cast((C.c_float * 64)(), C.c_void_p)
    other = C.cast((C.c_float * 64)(), C.c_void_p)
    hist = C.cast((C.c_float * 64)(), C.c_void_p)
    coef = (C.c_float * 16)()
    msw = (C.c_float * 4)(0.0, -0.1, -0.2, 0.0)
    w = lib.DenoiserWeights()

    def call(x0=None, noise=None, mask=None, draws=1, weights=msw, history=hist, x=p):
        return h.sd_ddim_sample_multistep(C.byref(w), p, p, coef, x, None, None, p, 2, 10, 1, 4, None, 3, x0, noise, mask, draws, weights, history, None)

    # the first step has no history
    assert call(weights=(C.c_float * 4)(-0.1, -0.1, -0.2, 0.0)) == -1
    assert b"msw[0]" in h.sd_last_error()
    assert call(weights=None) == -1 and call(history=None) == -1
    # the hold triple: all three or none
    for x0, noise, mask in ((None, other, other), (other, None, other), (other, other, None), (other, None, None)):
        assert call(x0, noise, mask) == -1
        assert b"together" in h.sd_last_error()
    # the history aliases neither x nor a hold buffer
    assert call(history=p) == -1
    assert b"alias" in h.sd_last_error()
    for x0, noise, mask in ((hist, other, other), (other, hist, other), (other, other, hist)):
        assert call(x0, noise, mask) == -1
        assert b"alias" in h.sd_last_error()
    assert call(other, p, other) == -1            # hold_noise == x
    assert b"alias" in h.sd_last_error()
    for draws in (0, -1, 3):
        assert call(draws=draws) == -1
        assert b"draws" in h.sd_last_error()
    # J <= 32 only when a mask is given: without one the call goes on to the weights (all NULL here: refused there, by another message)
    w.J = 33
    assert call(other, other, other) == -1
    assert b"J must be <= 32" in h.sd_last_error()
    assert call() == -1
    assert b"J must be <= 32" not in h.sd_last_error() and b"sd_ddim_sample_multistep" not in h.sd_last_error()
    # the loop form's step
    c4 = (C.c_float * 4)(0.5, 0.5, 0.6, 0.4)
    for args in ((None, p, p, hist, c4), (p, None, p, hist, c4), (p, p, None, hist, c4), (p, p, p, None, c4), (p, p, p, hist, None)):
        assert h.sd_multistep_step(*args, 0.0, 64, None) == -1
        assert b"sd_multistep_step" in h.sd_last_error()
    assert h.sd_multistep_step(p, p, p, hist, c4, 0.0, 0, None) == -1
    for args in ((hist, p, p, hist, c4), (p, hist, other, hist, c4), (p, other, hist, hist, c4)):
        assert h.sd_multistep_step(*args, -0.1, 64, None) == -1
        assert b"alias" in h.sd_last_error()


# ---- 5. Python-side validation that needs no device --------------------------------------------------------------------------------------
def test_multistep_argument_is_validated_before_any_device_work():
    from soccerdiffusion_amd import ops

    x, toks = torch.zeros(2, 4, 7), torch.zeros(4, 8)
    for bad, what in (([0.0, -0.1, 0.0], "expected"), ([-0.1, -0.1, -0.1, 0.0], r"w\[0\]"), ([0.0, float("nan"), 0.0, 0.0], "finite"),
                      ("abcd", "expected"), (np.zeros((4, 1)), "expected")):
        with pytest.raises(ValueError, match=what):
            ops.ddim_sample(None, None, toks, None, x, multistep=bad)
        with pytest.raises(ValueError, match=what):
            ops.ddim_sample_guarded(None, None, toks, None, x, multistep=bad)
    with pytest.raises(ValueError, match="exclude"):   # pin beside hold stays refused; a pin alone is folded into a mask
        ops.ddim_sample(None, None, toks, None, x, pin=(x, 1), hold=(x, torch.zeros(7, dtype=torch.bool)), multistep=[0.0] * 4)


def test_solver_is_validated_without_a_device():
    from test_cpu_session import BASE, SHIPPED

    from soccerdiffusion_amd import cli
    from soccerdiffusion_amd.scheduler import DDIMScheduler, MultistepScheduler
    from soccerdiffusion_amd.session import PolicySession

    assert PolicySession.check_solver() == "ddim" and PolicySession.check_solver("multistep", 22, 4) == "multistep"
    assert PolicySession.check_solver("multistep", 40, 0) == "multistep"          # no carry, no mask: any joint count
    with pytest.raises(ValueError, match="solver"):
        PolicySession.check_solver("heun")
    with pytest.raises(ValueError, match="distilled"):
        PolicySession.check_solver("multistep", 22, 0, distilled=True)
    with pytest.raises(ValueError, match="32"):
        PolicySession.check_solver("multistep", 33, 4)
    params = {**BASE, **SHIPPED["sim_scratch"], "use_images": False}
    model = cli.build_model(params).eval()
    with pytest.raises(ValueError, match="solver"):
        PolicySession(model, solver="euler")
    with pytest.raises(ValueError, match="distilled"):
        PolicySession(model, solver="multistep", distilled=True)
    with pytest.raises(RuntimeError, match="on the CPU"):
        PolicySession(model, solver="multistep")
    # model.sample: the solver's name, and not with the dropout loop
    x = torch.zeros(2, params["trajectory_prediction_length"], params["num_joints"])
    with pytest.raises(ValueError, match="solver"):
        model.sample([], x, 4, solver="heun")
    with pytest.raises(ValueError, match="with_dropout"):
        model.sample([], x, 4, solver="multistep", with_dropout=True)
    # the scheduler of the loop form: DDIMScheduler's surface, weights from multistep_weights, history cleared by set_timesteps
    sch = MultistepScheduler(beta_schedule="squaredcos_cap_v2", clip_sample=False)
    assert isinstance(sch, DDIMScheduler) and torch.equal(sch.alphas_cumprod, DDIMScheduler().alphas_cumprod)
    with pytest.raises(ValueError, match="set_timesteps"):
        sch.step(x, 900, x)
    sch.set_timesteps(10)
    assert sch.timesteps.tolist() == ddim_ref.timesteps(10).tolist()
    assert np.array_equal(sch._weights, ops_weights(10)) and sch._hist is None and sch._next == 0
    with pytest.raises(ValueError, match="order"):
        sch.step(x, 800, x)
    with pytest.raises(NotImplementedError):
        MultistepScheduler(beta_schedule="linear")


def ops_weights(n):
    from soccerdiffusion_amd import ops

    return ops.multistep_weights(ops.ddim_timesteps(n), ops.alphas_cumprod(), n)


def test_cli_solver_flag():
    from soccerdiffusion_amd import cli

    ap = cli.build_parser()
    assert ap.parse_args(["sample", "ckpt.pt"]).solver == "ddim"
    assert ap.parse_args(["sample", "ckpt.pt", "--solver", "multistep"]).solver == "multistep"
    assert ap.parse_args(["rollout", "ckpt.pt", "--synthetic", "2", "--ticks", "1", "--solver", "multistep"]).solver == "multistep"
    assert ap.parse_args(["evaluate", "ckpt.pt", "--synthetic", "8", "--all", "--solver", "multistep", "--steps", "5"]).solver == "multistep"
    assert ap.parse_args(["evaluate", "ckpt.pt", "--synthetic", "8", "--all"]).solver == "ddim"
    with pytest.raises(SystemExit):
        ap.parse_args(["sample", "ckpt.pt", "--solver", "heun"])
    assert not hasattr(ap.parse_args(["train", "-c", "cfg.yaml"]), "solver")       # --val-* of train is left alone
