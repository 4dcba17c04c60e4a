"""CPU-only checks of the per-joint limits (sd_ddim_sample_limits, sd_ddim_limit_step, sd_session_limits): ops.joint_limits' validation
and padding, the scheduler's clip_sample, PolicySession.check_limits, the new entry points in the header, in _lib.SIGNATURES and in the
built library, their argument errors without a device, and the CPU reference tests/limits_ref.py in fp64 - infinite limits against
tests/multistep_ref.py, the last step inside the limits, a NaN that reaches the output."""

import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

import limits_ref
import multistep_ref
from conftest import REPO
from test_cpu_pin import _toy_denoiser

NEW = ("sd_ddim_sample_limits", "sd_ddim_limit_step", "sd_session_limits")
INF = float("inf")


@pytest.fixture(scope="module")
def lib():
    from soccerdiffusion_amd import build

    build.build()
    from soccerdiffusion_amd import _lib

    return _lib


# ---- 1. ops.joint_limits ------------------------------------------------------------------------------------------------------------------
def test_joint_limits_pads_to_32_floats_with_infinities():
    from soccerdiffusion_amd import ops

    J = 7
    lo = torch.tensor([-1.0, -INF, -1.0, -0.5, 0.0, -2.0, 0.25])
    hi = [1.0, INF, 0.0, 0.5, 0.0, INF, 1.0]
    lim = ops.joint_limits(lo, hi, J=J, device="cpu")
    assert isinstance(lim, ops.Limits) and len(lim) == 2
    for t in lim:
        assert t.dtype == torch.float32 and tuple(t.shape) == (32,) and t.is_contiguous()
    assert lim.lo[:J].tolist() == lo.tolist() and lim.hi[:J].tolist() == hi
    assert (lim.lo[J:] == -INF).all() and (lim.hi[J:] == INF).all()
    # one range on every joint; a dict for some joints
    r = ops.joint_limits(0.75, J=J, device="cpu")
    assert r.lo[:J].tolist() == [-0.75] * J and r.hi[:J].tolist() == [0.75] * J and (r.lo[J:] == -INF).all() and (r.hi[J:] == INF).all()
    d = ops.joint_limits({2: (-1.0, 0.0), 6: (0.25, INF)}, J=J, device="cpu")
    assert d.lo.tolist() == [-INF, -INF, -1.0, -INF, -INF, -INF, 0.25] + [-INF] * 25
    assert d.hi.tolist() == [INF, INF, 0.0] + [INF] * 29
    assert (ops.joint_limits({}, J=32, device="cpu").lo == -INF).all()
    # what a sampler call makes of its limits= argument
    assert ops._limits_req(lim, J, "cpu") is lim
    assert torch.equal(ops._limits_req((lo, hi), J, "cpu").hi, lim.hi) and torch.equal(ops._limits_req(0.75, J, "cpu").lo, r.lo)


def test_joint_limits_refuses_bad_limits():
    from soccerdiffusion_amd import ops

    J = 4
    ok = [0.0] * J
    for lo, hi, what in (([0.0] * 3, ok, "lo"), (ok, [0.0] * 5, "hi"), ([float("nan")] + ok[1:], [1.0] * J, "NaN"), (ok, [1.0, 1.0, float("nan"), 1.0], "NaN"),
                         ([0.0, 0.0, 0.5, 0.0], [1.0, 1.0, 0.25, 1.0], r"lo\[2\]"), (torch.zeros(J, 1), ok, "lo")):
        with pytest.raises(ValueError, match=what):
            ops.joint_limits(lo, hi, J=J, device="cpu")
    for bad, what in ((-1.0, "range"), (float("nan"), "range"), ({4: (0.0, 1.0)}, "out of range"), ({-1: (0.0, 1.0)}, "out of range"),
                      ({0: (1.0, 0.0)}, r"lo\[0\]"), ({0: 1.0}, "expected"), ("abc", "expected")):
        with pytest.raises(ValueError, match=what):
            ops.joint_limits(bad, J=J, device="cpu")
    with pytest.raises(ValueError, match="32 joints"):
        ops.joint_limits(1.0, J=33, device="cpu")
    with pytest.raises(ValueError, match="J and device"):
        ops.joint_limits(1.0)
    # a Limits from another shape or dtype is not taken as it is
    with pytest.raises(ValueError, match="joint_limits"):
        ops._limits_req(ops.Limits((torch.zeros(20), torch.ones(20))), 20, "cpu")


# ---- 2. the scheduler ---------------------------------------------------------------------------------------------------------------------
def test_scheduler_accepts_clip_sample():
    from soccerdiffusion_amd.scheduler import DDIMScheduler, MultistepScheduler

    for cls in (DDIMScheduler, MultistepScheduler):
        s = cls(beta_schedule="squaredcos_cap_v2", clip_sample=True)
        assert s.config["clip_sample"] is True and s.config["clip_sample_range"] == 1.0 and s._limits_spec == 1.0
        s = cls(clip_sample=True, clip_sample_range=2.5)
        assert s.config["clip_sample_range"] == 2.5 and s._limits_spec == 2.5
        lim = s._limits(torch.zeros(2, 3, 5))
        assert lim.lo[:5].tolist() == [-2.5] * 5 and lim.hi[:5].tolist() == [2.5] * 5 and (lim.hi[5:] == INF).all()
        assert s._limits(torch.zeros(1, 5)) is lim            # built once per (device, J)
        off = cls(beta_schedule="squaredcos_cap_v2", clip_sample=False)
        assert off.config["clip_sample"] is False and off._limits(torch.zeros(2, 3, 5)) is None      # the call of before
        per_joint = cls(limits={1: (-0.5, 0.25)})
        assert per_joint._limits(torch.zeros(2, 3)).hi[:3].tolist() == [INF, 0.25, INF]
        with pytest.raises(ValueError, match="clip_sample_range"):
            cls(clip_sample=True, clip_sample_range=-1.0)
        with pytest.raises(NotImplementedError):
            cls(beta_schedule="linear", clip_sample=True)


# ---- 3. the session -----------------------------------------------------------------------------------------------------------------------
def test_policy_session_check_limits_needs_no_device():
    from soccerdiffusion_amd.session import PolicySession

    assert PolicySession.check_limits(None, 20) is None
    lo, hi = PolicySession.check_limits(([-1.0] * 20, [1.0] * 20), 20)
    assert lo.dtype == np.float32 and lo.shape == (32,) and lo[:20].tolist() == [-1.0] * 20 and (hi[20:] == np.inf).all()
    lo, hi = PolicySession.check_limits({3: (-0.5, 0.5)}, 20, carry=4)
    assert lo[3] == -0.5 and hi[3] == 0.5 and np.isinf(lo[:3]).all()
    with pytest.raises(ValueError, match="distilled"):
        PolicySession.check_limits(1.0, 20, distilled=True)
    with pytest.raises(ValueError, match="carry"):
        PolicySession.check_limits(1.0, 33, carry=2)
    with pytest.raises(ValueError, match="32 joints"):
        PolicySession.check_limits(1.0, 33)
    with pytest.raises(ValueError, match=r"lo\[0\]"):
        PolicySession.check_limits(([1.0] * 20, [0.0] * 20), 20)
    with pytest.raises(ValueError, match="NaN"):
        PolicySession.check_limits({0: (float("nan"), 1.0)}, 20)


# ---- 4. exports ---------------------------------------------------------------------------------------------------------------------------
def test_new_entry_points_are_declared_registered_and_exported(lib):
    with open(os.path.join(REPO, "include", "soccerdiffusion_hip.h")) as f:
        header = f.read()
    declared = set(re.findall(r"^(?:int|size_t|const char \*)\s*(sd_\w+)\(", header, re.M))
    h = lib.load()
    for name in NEW:
        assert name in declared, name
        assert name in lib.SIGNATURES, name
        assert getattr(h, name) is not None
        args = re.search(r"^int " + name + r"\((.*?)\);", header, re.M | re.S).group(1)
        assert len(args.split(",")) == len(lib.SIGNATURES[name][1]), name
    assert "#define SD_ABI_VERSION 1" in header and h.sd_abi_version() == 1   # additive: the version stays
    # sd_ddim_sample_limits = sd_ddim_sample_multistep's arguments with lo, hi and reproject in front of the stream
    ms = lib.SIGNATURES["sd_ddim_sample_multistep"][1]
    assert lib.SIGNATURES["sd_ddim_sample_limits"][1] == ms[:-1] + [C.c_void_p, C.c_void_p, C.c_int] + ms[-1:]
    assert len(lib.SIGNATURES["sd_ddim_sample_limits"][1]) == 24 and len(lib.SIGNATURES["sd_ddim_limit_step"][1]) == 12
    assert len(lib.SIGNATURES["sd_session_limits"][1]) == 8


def test_new_entry_points_reject_bad_arguments_without_gpu(lib):
    h = lib.load()
    p = C.cast((C.c_float * 64)(), C.c_void_p)
    other = C.cast((C.c_float * 64)(), C.c_void_p)
    hist = C.cast((C.c_float * 64)(), C.c_void_p)
    lo = C.cast((C.c_float * 32)(), C.c_void_p)
    hi = C.cast((C.c_float * 32)(), C.c_void_p)
    coef = (C.c_float * 16)()
    msw = (C.c_float * 4)(0.0, -0.1, -0.2, 0.0)
    w = lib.DenoiserWeights()

    def call(x0=None, noise=None, mask=None, draws=1, weights=msw, history=hist, x=p, lo=lo, hi=hi):
        return h.sd_ddim_sample_limits(C.byref(w), p, p, coef, x, None, None, p, 2, 10, 1, 4, None, 3, x0, noise, mask, draws, weights, history, lo, hi, 0,
                                       None)

    assert call(lo=None) == -1 and b"lo and hi" in h.sd_last_error()
    assert call(hi=None) == -1 and b"lo and hi" in h.sd_last_error()
    # the hold triple: all three or none
    for x0, noise, mask in ((None, other, other), (other, None, other), (other, other, None), (other, None, None)):
        assert call(x0, noise, mask) == -1
        assert b"together" in h.sd_last_error()
    # msw needs a history; the first step has no history
    assert call(history=None) == -1 and b"history" in h.sd_last_error()
    assert call(weights=(C.c_float * 4)(-0.1, -0.1, -0.2, 0.0)) == -1 and b"msw[0]" in h.sd_last_error()
    # the aliasing cases of the multistep call
    assert call(history=p) == -1 and b"alias" in h.sd_last_error()
    for x0, noise, mask in ((hist, other, other), (other, hist, other), (other, other, hist)):
        assert call(x0, noise, mask) == -1
        assert b"alias" in h.sd_last_error()
    assert call(other, p, other) == -1 and b"alias" in h.sd_last_error()            # hold_noise == x
    for draws in (0, -1, 3):
        assert call(draws=draws) == -1
        assert b"draws" in h.sd_last_error()
    # no msw is DDIM under limits, with a history buffer or without: the call goes on to the weights (all NULL here: refused there, by
    # another message)
    for history in (None, hist):
        assert call(weights=None, history=history) == -1
        assert b"sd_ddim_sample_limits" not in h.sd_last_error()
    w.J = 33
    assert call() == -1 and b"32 joints" in h.sd_last_error()
    # the loop form's step
    c4 = (C.c_float * 4)(0.5, 0.5, 0.6, 0.4)

    def step(eps=p, x=p, out=p, history=hist, c=c4, wt=0.0, lo=lo, hi=hi, n=64, J=16):
        return h.sd_ddim_limit_step(eps, x, out, history, c, wt, lo, hi, 1, n, J, None)

    for kw in (dict(eps=None), dict(x=None), dict(out=None), dict(c=None), dict(lo=None), dict(hi=None), dict(n=0), dict(J=0), dict(J=33), dict(n=63)):
        assert step(**kw) == -1, kw
        assert b"sd_ddim_limit_step" in h.sd_last_error()
    assert step(history=None, wt=-0.1) == -1 and b"history" in h.sd_last_error()
    for kw in (dict(eps=hist), dict(x=hist, out=other), dict(out=hist, x=other)):
        assert step(**kw, wt=-0.1) == -1, kw
        assert b"alias" in h.sd_last_error()
    # the session's conversion
    f32 = (C.c_float * 32)
    good_lo, good_hi = f32(*([-1.0] * 32)), f32(*([1.0] * 32))
    for args in ((None, hi, good_lo, good_hi, p, p, 20), (lo, None, good_lo, good_hi, p, p, 20), (lo, hi, None, good_hi, p, p, 20),
                 (lo, hi, good_lo, None, p, p, 20), (lo, hi, good_lo, good_hi, None, p, 20), (lo, hi, good_lo, good_hi, p, None, 20),
                 (lo, hi, good_lo, good_hi, p, p, 0), (lo, hi, good_lo, good_hi, p, p, 33)):
        assert h.sd_session_limits(*args, None) == -1
        assert b"sd_session_limits" in h.sd_last_error()
    assert h.sd_session_limits(lo, hi, good_hi, good_lo, p, p, 20, None) == -1 and b"lo[j] <= hi[j]" in h.sd_last_error()
    assert h.sd_session_limits(lo, hi, f32(*([float("nan")] * 32)), good_hi, p, p, 20, None) == -1 and b"NaN" in h.sd_last_error()


# ---- 5. the reference itself, in fp64 -----------------------------------------------------------------------------------------------------
def _inputs(B=3, T=10, J=7, seed=3):
    g = torch.Generator().manual_seed(seed)
    x_T, known = torch.randn(B, T, J, generator=g).double(), torch.randn(B, T, J, generator=g).double()
    mask = torch.rand(B, T, J, generator=g) < 0.3
    den32 = _toy_denoiser(4, J)
    return x_T, known, mask, (lambda x, t: den32(x.float(), t).double())


def test_infinite_limits_are_multistep_ref_exactly():
    n = 5
    x_T, known, mask, den = _inputs()
    lo, hi = torch.full((7,), -INF), torch.full((7,), INF)
    for w in ([0.0] * n, multistep_ref.weights(n)):
        for k, m in ((None, None), (known, mask)):
            want = multistep_ref.sample(den, x_T, k, m, n, w)
            for reproject in (False, True):
                got = limits_ref.sample(den, x_T, k, m, n, w, lo, hi, reproject)
                assert all(torch.equal(a, b) for a, b in zip(want[0], got[0])) and all(torch.equal(a, b) for a, b in zip(want[2], got[2]))
                assert not any((h != 0).any() for h in got[3])
    assert all(torch.equal(a, b) for a, b in zip(limits_ref.sample(den, x_T, None, None, n, None, lo, hi)[0], multistep_ref.sample(den, x_T, None, None, n, [0.0] * n)[0]))


def test_the_last_step_leaves_the_free_elements_inside_the_limits():
    n, J = 4, 7
    x_T, known, mask, den = _inputs()
    lo = torch.tensor([-1.0, -INF, -1.0, -1.0, -1.0, -1.0, 0.25]).double()
    hi = torch.tensor([1.0, INF, 0.0, 1.0, 1.0, 1.0, 1.0]).double()
    for w in (None, multistep_ref.weights(n)):
        for reproject in (False, True):
            for k, m in ((None, None), (known * 3, mask)):
                out, held, eps, side = limits_ref.sample(den, x_T, k, m, n, w, lo, hi, reproject)
                hit = [s != 0 for s in side]
                free = torch.ones_like(mask) if m is None else ~m
                x = out[-1]
                assert ((x >= lo) & (x <= hi))[free].all()
                assert hit[-1][free].any() and torch.equal(x[hit[-1] & free], limits_ref.clamp(x, lo, hi)[hit[-1] & free])
                # a clamped element equals its limit bit for bit after the last step
                at_limit = (x == lo) | (x == hi)
                assert at_limit[hit[-1] & free].all()
                if m is not None:      # held elements keep the hold's value whatever the limits say
                    assert torch.equal(x[m], (known * 3)[m]) and not ((x >= lo) & (x <= hi))[m].all()
                # reproject changes the steps before the last, not what the last step returns for a clamped element
            a = limits_ref.sample(den, x_T, None, None, n, w, lo, hi, False)[0]
            b = limits_ref.sample(den, x_T, None, None, n, w, lo, hi, True)[0]
            assert not torch.equal(a[0], b[0])


def test_a_nan_prediction_reaches_the_output():
    n, J = 4, 7
    x_T, _, _, den = _inputs()
    lo, hi = torch.full((J,), -1.0).double(), torch.full((J,), 1.0).double()

    def poisoned(x, t):
        e = den(x, t).clone()
        if t == 0:      # the last step of the leading grid
            e[1, 2, 3] = float("nan")
        return e

    for reproject in (False, True):
        out = limits_ref.sample(poisoned, x_T, None, None, n, multistep_ref.weights(n), lo, hi, reproject)[0][-1]
        nan = torch.isnan(out)
        assert bool(nan[1, 2, 3]) and int(nan.sum()) == 1
        assert math.isnan(float(limits_ref.clamp(torch.tensor([float("nan")]).double(), lo[:1], hi[:1])))
