"""CPU-only checks of the per-joint slew limits (sd_ddim_sample_slew, sd_ddim_slew_step, sd_session_slew): the CPU reference
tests/slew_ref.py - the box (P1), the slew bound with its exemption (P2), infinite v against tests/limits_ref.py (P3), non-expansiveness
(P4), idempotence (P5), held transitions (P6), NaN - ops.joint_slew's validation and padding, the ``slew=`` forms, the schedulers,
PolicySession.check_slew, the new entry points in the header, in _lib.SIGNATURES and in the built library, and a host model of the
session's conversion from radians per row."""

import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

import limits_ref
import slew_ref
from conftest import REPO
from test_cpu_pin import _toy_denoiser

NEW = ("sd_ddim_sample_slew", "sd_ddim_slew_step", "sd_session_slew", "sd_session_anchor", "sd_eval_max_step")
INF, NAN = float("inf"), float("nan")


@pytest.fixture(scope="module")
def lib():
    from soccerdiffusion_amd import build

    build.build()
    from soccerdiffusion_amd import _lib

    return _lib


def _inputs(seed, B=3, T=12, J=7, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    x0 = torch.randn(B, T, J, generator=g).to(dtype)
    known = (torch.randn(B, T, J, generator=g) * 2).to(dtype)
    mask = torch.rand(B, T, J, generator=g) < 0.25
    v = torch.rand(J, generator=g).to(dtype) * 0.5
    v[1] = INF
    start = (0.5 * torch.randn(B, J, generator=g)).to(dtype)
    start[:, 3] = NAN
    lo, hi = torch.full((J,), -1.0, dtype=dtype), torch.full((J,), 1.0, dtype=dtype)
    lo[2], hi[2] = -INF, INF
    return x0, known, mask, v, start, lo, hi


# ---- 1. the scan's properties ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_scan_keeps_the_box_and_the_slew_bound_bitwise(dtype):
    for seed in range(6):
        x0, known, mask, v, start, lo, hi = _inputs(seed, dtype=dtype)
        inf = torch.full_like(lo, INF)
        for masked in (False, True):
            for box in ((lo, hi), (-inf, inf)):
                for st in (start, None):
                    z, side = slew_ref.scan(x0, v, st, *box, known if masked else None, mask if masked else None)
                    free = ~mask if masked else torch.ones_like(mask)
                    p1, p2 = slew_ref.check_properties(z, v, st, *box, free)
                    assert p1 and p2, (seed, masked, st is None)                                  # P1, P2 with the exemption
                    if masked:
                        assert torch.equal(z[mask], known[mask])                                  # P6: a held element is the hold's value
                    z2, _ = slew_ref.scan(z, v, st, *box, known if masked else None, mask if masked else None)
                    assert torch.equal(z2, z)                                                     # P5: idempotent
                    assert bool((side != 0).any())


def test_the_exemption_is_needed_and_a_jump_into_a_held_element_is_not_limited():
    x0 = torch.zeros(1, 4, 1)
    known = torch.full((1, 4, 1), 5.0)
    mask = torch.zeros(1, 4, 1, dtype=torch.bool)
    mask[0, 1] = True
    v, lo, hi = torch.tensor([0.5]), torch.tensor([-1.0]), torch.tensor([1.0])
    z, _ = slew_ref.scan(x0, v, None, lo, hi, known, mask)
    # row 1 is held at 5 (outside the box, a jump of 5 from row 0); row 2 wants 0, the slew limit says 4.5, the box says 1: the box wins
    assert z.flatten().tolist() == [0.0, 5.0, 1.0, 0.5]
    p1, p2 = slew_ref.check_properties(z, v, None, lo, hi, ~mask)
    assert p1 and p2
    # an anchor outside the box: the same
    z, _ = slew_ref.scan(x0, v, torch.tensor([[-3.0]]), lo, hi)
    assert z.flatten().tolist() == [-1.0, -0.5, 0.0, 0.0]


def test_infinite_v_without_start_is_limits_ref_exactly():
    B, T, J, n = 3, 10, 7, 4
    g = torch.Generator().manual_seed(1)
    x_T, known = torch.randn(B, T, J, generator=g), torch.randn(B, T, J, generator=g) * 2
    mask = torch.rand(B, T, J, generator=g) < 0.3
    den = _toy_denoiser(2, J)
    lo, hi = torch.full((J,), -0.75), torch.full((J,), 0.5)
    v = torch.full((J,), INF)
    for w in (None, [0.0, 0.3, 0.2, 0.0]):
        for m, k in ((None, None), (mask, known)):
            for reproject in (False, True):
                want = limits_ref.sample(den, x_T, k, m, n, w, lo, hi, reproject)
                got = slew_ref.sample(den, x_T, k, m, n, w, v, None, lo, hi, reproject)
                for a, b in zip(want[:3], got[:3]):
                    assert all(torch.equal(p.view(torch.int32), q.view(torch.int32)) for p, q in zip(a, b))     # P3
                assert not any(bool(s.any()) for s in got[3])


def test_the_scan_is_non_expansive_in_the_sup_norm():
    for seed in range(8):
        x0, known, mask, v, start, lo, hi = _inputs(seed, dtype=torch.float64)
        g = torch.Generator().manual_seed(100 + seed)
        for scale in (1e-6, 1e-2, 1.0):
            x1 = x0 + scale * torch.randn(x0.shape, generator=g, dtype=torch.float64)
            for masked in (False, True):
                a, _ = slew_ref.scan(x0, v, start, lo, hi, known if masked else None, mask if masked else None)
                b, _ = slew_ref.scan(x1, v, start, lo, hi, known if masked else None, mask if masked else None)
                both = torch.isfinite(a) & torch.isfinite(b)
                assert float((a - b)[both].abs().max()) <= float((x0 - x1).abs().max()) * (1 + 1e-12)           # P4


def test_nan_stays_nan_and_limits_nothing_downstream():
    x0 = torch.tensor([0.0, 0.125, NAN, 3.0, 3.0, 0.0]).view(1, 6, 1)
    v, lo, hi = torch.tensor([0.25]), torch.tensor([-INF]), torch.tensor([INF])
    z, side = slew_ref.scan(x0, v, torch.tensor([[1.0]]), lo, hi)
    assert z.flatten()[:2].tolist() == [0.75, 0.5] and math.isnan(float(z[0, 2, 0]))
    assert z.flatten()[3:].tolist() == [3.0, 3.0, 2.75]      # row 3 follows a NaN: free; rows 4, 5 follow row 3 again
    assert side.flatten().tolist() == [-1, -1, 0, 0, 0, -1]
    # a NaN start leaves row 0 free
    z, _ = slew_ref.scan(x0[:, :2], v, torch.tensor([[NAN]]), lo, hi)
    assert z.flatten().tolist() == [0.0, 0.125]


def test_the_last_step_of_the_rollout_returns_the_scan():
    B, T, J, n = 2, 10, 5, 4
    g = torch.Generator().manual_seed(9)
    x_T = torch.randn(B, T, J, generator=g)
    v, start = torch.full((J,), 0.2), torch.zeros(B, J)
    lo, hi = torch.full((J,), -1.0), torch.full((J,), 1.0)
    out, _, _, side, clean = slew_ref.sample(_toy_denoiser(3, J), x_T, None, None, n, [0.0, 0.4, 0.3, 0.0], v, start, lo, hi, True)
    assert torch.equal(out[-1], clean[-1]) and all(bool(s.any()) for s in side)
    assert slew_ref.check_properties(out[-1], v, start, lo, hi, torch.ones(B, T, J, dtype=torch.bool)) == (True, True)


# ---- 2. ops.joint_slew and the slew= forms ----------------------------------------------------------------------------------------------------
def test_joint_slew_pads_to_32_floats_with_infinity():
    from soccerdiffusion_amd import ops

    J = 7
    v = ops.joint_slew([0.5, INF, 0.25, 0.0, 1.0, 2.0, 3.0], J=J, device="cpu")
    assert v.dtype == torch.float32 and tuple(v.shape) == (32,) and v[:J].tolist() == [0.5, INF, 0.25, 0.0, 1.0, 2.0, 3.0] and (v[J:] == INF).all()
    assert ops.joint_slew(0.75, J=J, device="cpu").tolist() == [0.75] * J + [INF] * 25
    assert ops.joint_slew({2: 0.5, 6: 0.0}, J=J, device="cpu").tolist() == [INF, INF, 0.5, INF, INF, INF, 0.0] + [INF] * 25
    assert (ops.joint_slew({}, J=32, device="cpu") == INF).all()
    assert torch.equal(ops.joint_slew(torch.full((J,), 0.5), J=J, device="cpu")[:J], torch.full((J,), 0.5))


def test_joint_slew_refuses_bad_values():
    from soccerdiffusion_amd import ops

    J = 4
    for bad, what in (([0.5] * 3, "shape"), ([0.5, NAN, 0.5, 0.5], "NaN"), ([0.5, -0.1, 0.5, 0.5], "negative"), (-1.0, "negative"), (NAN, "NaN"),
                      ({4: 0.5}, "out of range"), ({-1: 0.5}, "out of range"), ({0: (0.0, 1.0)}, "one number"), ("abc", "expected"),
                      (torch.zeros(J, 1), "shape")):
        with pytest.raises(ValueError, match=what):
            ops.joint_slew(bad, J=J, device="cpu")
    with pytest.raises(ValueError, match="32 joints"):
        ops.joint_slew(1.0, J=33, device="cpu")
    with pytest.raises(ValueError, match="J and device"):
        ops.joint_slew(1.0)


def test_the_slew_argument_of_a_sampler_call():
    from soccerdiffusion_amd import ops

    B, J = 3, 5
    v, start = ops._slew_req(0.5, B, J, "cpu")
    assert v[:J].tolist() == [0.5] * J and start is None
    ready = ops.joint_slew({1: 0.25}, J=J, device="cpu")
    assert ops._slew_req(ready, B, J, "cpu")[0] is ready                       # the padded array as it is
    st = torch.arange(B * J, dtype=torch.float32).view(B, J)
    v, start = ops._slew_req(([0.5] * J, st), B, J, "cpu")
    assert tuple(start.shape) == (B, 32) and torch.equal(start[:, :J], st) and bool(torch.isnan(start[:, J:]).all())
    padded = torch.full((B, 32), NAN)
    assert ops._slew_req((ready, padded), B, J, "cpu")[1] is padded            # ... and a padded start
    for bad, what in ((([0.5] * J, torch.zeros(B + 1, J)), "start"), (([0.5] * J, torch.zeros(B, J + 1)), "start"), (([0.5] * J, torch.zeros(J)), "start"),
                      ((-0.5, None), "negative")):
        with pytest.raises(ValueError, match=what):
            ops._slew_req(bad, B, J, "cpu")
    with pytest.raises(ValueError, match="32 joints"):
        ops._slew_req(0.5, B, 33, "cpu")


def test_schedulers_accept_slew():
    from soccerdiffusion_amd.scheduler import DDIMScheduler, MultistepScheduler

    for cls in (DDIMScheduler, MultistepScheduler):
        s = cls(beta_schedule="squaredcos_cap_v2", slew={1: 0.25})
        v, start = s._slew(torch.zeros(2, 3, 5))
        assert v[:5].tolist() == [INF, 0.25, INF, INF, INF] and start is None and s._limits(torch.zeros(2, 3, 5)) is None
        assert s._slew(torch.zeros(2, 9, 5))[0] is v                           # built once per (device, B, J)
        with pytest.raises(ValueError, match="whole"):
            s._slew(torch.zeros(6, 5))
        assert cls()._slew(torch.zeros(2, 3, 5)) is None                       # the call of before


# ---- 3. the session ---------------------------------------------------------------------------------------------------------------------------
def test_policy_session_check_slew_needs_no_device():
    from soccerdiffusion_amd.session import PolicySession

    assert PolicySession.check_slew(None, 20) is None
    v = PolicySession.check_slew(0.16, 20)
    assert v.dtype == np.float32 and v.shape == (32,) and np.allclose(v[:20], 0.16) and (v[20:] == np.inf).all()
    assert PolicySession.check_slew({3: 0.5}, 20, carry=4)[3] == 0.5
    assert PolicySession.check_slew([0.1] * 20, 20)[19] == np.float32(0.1)
    for bad, what in ((-0.1, "negative"), ([0.1] * 19, "shape"), ({20: 0.1}, "out of range"), (NAN, "NaN")):
        with pytest.raises(ValueError, match=what):
            PolicySession.check_slew(bad, 20)
    with pytest.raises(ValueError, match="distilled"):
        PolicySession.check_slew(0.1, 20, distilled=True)
    with pytest.raises(ValueError, match="32 joints"):
        PolicySession.check_slew(0.1, 33)


def test_host_model_of_the_session_conversion_keeps_published_steps_within_v_rad():
    """sd_session_slew's arithmetic (ops.session_slew_host) on random joints: x[t + 1] is the worst the scan allows, fl(x[t] +- v_n); both
    roundings of the commit's expression - fma(x, std, mean) - pi and (x * std + mean) - pi - publish values whose difference, in fp64,
    stays within v_rad.  Published values lie in [-pi, pi]."""
    from soccerdiffusion_amd import ops

    n = 200_000
    rng = np.random.default_rng(0)
    mean = rng.uniform(0.0, 2 * math.pi, n).astype(np.float32)
    std = np.exp(rng.uniform(math.log(1e-2), math.log(3.0), n)).astype(np.float32)
    v_rad = np.exp(rng.uniform(math.log(1e-4), math.log(1.0), n)).astype(np.float32)
    pi32 = np.float32(math.pi)
    v_n = ops.session_slew_host(v_rad, np.full(n, math.pi, dtype=np.float32), mean, std)
    assert v_n.dtype == np.float32 and (v_n > 0).all() and (v_n.astype(np.float64) * std < v_rad).all()
    # the conversion gives away next to nothing: the margin is a few ulps of pi
    assert (v_rad.astype(np.float64) - v_n.astype(np.float64) * std <= 1e-5).all()

    def fused(x):   # fma(x, std, mean) - pi: the product and the sum exactly in fp64 (24 + 24 bits), one rounding to fp32
        return ((x.astype(np.float64) * std.astype(np.float64) + mean.astype(np.float64)).astype(np.float32) - pi32).astype(np.float32)

    def plain(x):
        return ((x * std).astype(np.float32) + mean).astype(np.float32) - pi32

    r0 = rng.uniform(-math.pi, math.pi, n)
    x = (((r0 + math.pi) - mean) / std).astype(np.float32)
    worst = 0.0
    for sign in (1.0, -1.0):
        nxt = (x + np.float32(sign) * v_n).astype(np.float32)
        for commit in (fused, plain):
            a, b = commit(x).astype(np.float64), commit(nxt).astype(np.float64)
            keep = (np.abs(a) <= math.pi) & (np.abs(b) <= math.pi)
            assert keep.sum() > 0.8 * n
            excess = np.abs(b - a) - v_rad.astype(np.float64)
            worst = max(worst, float(excess[keep].max()))
            assert (excess[keep] <= 0).all(), (sign, commit.__name__, float(excess[keep].max()))
    # and the margin is not idle: without it the plain v_rad / std breaks the bound somewhere
    naive = (v_rad / std).astype(np.float32)
    nxt = (x + naive).astype(np.float32)
    assert (np.abs(plain(nxt).astype(np.float64) - plain(x).astype(np.float64)) > v_rad.astype(np.float64)).any()
    # a v_rad below its margin comes out as 0; the margin follows the bound
    assert ops.session_slew_host([1e-7], [math.pi], [3.0], [1.0])[0] == 0.0
    assert ops.session_slew_margin([10.0], [0.0], [1.0])[0] > ops.session_slew_margin([math.pi], [0.0], [1.0])[0] > 0


def test_host_model_of_the_denormalised_conversion_keeps_steps_within_v():
    """evaluation.normalised_slew on random joints: x[t + 1] is the worst the scan allows, fl(x[t] +- v_n); the denormalised values
    x * std + mean, in fp32 with one rounding per operation (ops.max_step, ops.normalize) or one (fma), differ by at most v, exactly."""
    from soccerdiffusion_amd.evaluation import normalised_slew

    n = 100_000
    rng = np.random.default_rng(1)
    mean = rng.uniform(0.0, 2 * math.pi, n).astype(np.float32)
    std = np.exp(rng.uniform(math.log(1e-2), math.log(3.0), n)).astype(np.float32)
    v = np.exp(rng.uniform(math.log(1e-4), math.log(1.0), n)).astype(np.float32)
    v_n = np.concatenate([normalised_slew(v[i:i + 32], torch.from_numpy(mean[i:i + 32]), torch.from_numpy(std[i:i + 32])).numpy()
                          for i in range(0, n, 32)])
    assert v_n.dtype == np.float32 and (v_n > 0).all()
    r0 = rng.uniform(0.0, 2 * math.pi, n)
    x = ((r0 - mean) / std).astype(np.float32)
    plain = lambda u: ((u * std).astype(np.float32) + mean).astype(np.float32)
    fused = lambda u: (u.astype(np.float64) * std.astype(np.float64) + mean.astype(np.float64)).astype(np.float32)
    for sign in (1.0, -1.0):
        nxt = (x + np.float32(sign) * v_n).astype(np.float32)
        for den in (plain, fused):
            a, b = den(x).astype(np.float64), den(nxt).astype(np.float64)
            keep = (np.abs(a) <= 2 * math.pi) & (np.abs(b) <= 2 * math.pi)
            assert keep.sum() > 0.7 * n and (np.abs(b - a)[keep] <= v.astype(np.float64)[keep]).all(), sign
    with pytest.raises(ValueError, match="margin"):
        normalised_slew(1e-8, torch.zeros(4), torch.ones(4))


# ---- 4. the entry points ------------------------------------------------------------------------------------------------------------------------
def test_new_entry_points_are_declared_bound_and_exported(lib):
    header = open(os.path.join(REPO, "include", "soccerdiffusion_hip.h")).read()
    handle = lib.load()
    for name in NEW:
        assert re.search(rf"\bint {name}\(", header), name
        assert name in lib.SIGNATURES and hasattr(handle, name), name


def test_argument_errors_need_no_device(lib):
    handle = lib.load()
    f4 = (C.c_float * 4)(0.8, 0.6, 0.9, 0.4)
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    bad = lib.SD_E_BADARG if hasattr(lib, "SD_E_BADARG") else None
    rc = handle.sd_ddim_slew_step(p, p, p, None, f4, 0.0, p, p, 0, None, None, None, None, 1, 2, 4, None)       # v NULL
    assert rc != 0 and (bad is None or rc == bad)
    assert handle.sd_ddim_slew_step(p, p, p, None, f4, 0.5, p, p, 0, p, None, None, None, 1, 2, 4, None) != 0    # w without hist
    assert handle.sd_ddim_slew_step(p, p, p, None, f4, 0.0, p, p, 0, p, None, p, None, 1, 2, 4, None) != 0       # hold_x0 without a mask
    assert handle.sd_ddim_slew_step(p, p, p, None, f4, 0.0, p, p, 0, p, None, None, None, 1, 2, 33, None) != 0   # J > 32
    v = (C.c_float * 4)(0.1, -0.1, 0.1, 0.1)
    r = (C.c_float * 4)(3.0, 3.0, 3.0, 3.0)
    assert handle.sd_session_slew(p, v, r, p, p, 4, None) != 0                                                   # a negative v_rad
    assert handle.sd_session_anchor(p, p, None, 2, 1, 4, 4, 0, 1, None) != 0                                     # S > B
    assert handle.sd_eval_max_step(p, p, p, None, 1, 4, 4, None) != 0                                            # out NULL
