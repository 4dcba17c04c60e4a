"""CPU-only checks of the per-joint acceleration limits (sd_ddim_sample_accel, sd_ddim_accel_step, sd_direct_project_accel,
sd_session_accel, sd_session_anchor2, sd_max_accel): the CPU reference tests/accel_ref.py - the box and the slew bound (P1, P2), the
acceleration interval with its exemption (P3), infinite a against tests/slew_ref.py (P4), NaN (P5) - the interval-intersection argument
behind P3's exemption by brute force, ops.joint_accel's validation and padding, the ``accel=`` forms, the schedulers,
PolicySession.check_accel, the cli parser, the new entry points in the header, in _lib.SIGNATURES and in the built library, and a host
model of the session's conversion from radians per row^2."""

import ctypes as C
import itertools
import math
import os
import re

import numpy as np
import pytest
import torch

import accel_ref
import slew_ref
from conftest import REPO
from test_cpu_pin import _toy_denoiser

NEW = ("sd_ddim_sample_accel", "sd_ddim_accel_step", "sd_direct_sample_accel", "sd_direct_project_accel", "sd_session_accel", "sd_session_anchor2", "sd_max_accel")
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
    a = torch.rand(J, generator=g).to(dtype) * 0.5
    a[1], a[4] = INF, 0.0
    v = torch.rand(J, generator=g).to(dtype) * 0.75
    v[2], v[4] = INF, INF
    start = (0.5 * torch.randn(B, J, generator=g)).to(dtype)
    start[:, 3] = NAN
    start2 = start + (0.25 * torch.randn(B, J, generator=g)).to(dtype)
    start2[:, 5] = NAN
    lo, hi = torch.full((J,), -1.0, dtype=dtype), torch.full((J,), 1.0, dtype=dtype)
    lo[2], hi[2] = -INF, INF
    lo[4], hi[4] = -INF, INF
    return x0, known, mask, a, start2, v, start, lo, hi


# ---- 1. the scan's properties ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_scan_keeps_the_box_the_slew_bound_and_the_acceleration_interval_bitwise(dtype):
    moved = 0
    for seed in range(6):
        x0, known, mask, a, start2, v, start, lo, hi = _inputs(seed, dtype=dtype)
        inf = torch.full_like(lo, INF)
        for masked in (False, True):
            for box in ((lo, hi), (-inf, inf)):
                for vv in (v, inf):
                    for st, st2 in ((start, start2), (start, None), (None, None)):
                        z, side = accel_ref.scan(x0, a, st2, vv, st, *box, known if masked else None, mask if masked else None)
                        free = ~mask if masked else torch.ones_like(mask)
                        p1, p2, p3 = accel_ref.check_properties(z, a, st2, vv, st, *box, free)
                        assert p1 and p2 and p3, (seed, masked, st is None, st2 is None, p1, p2, p3)      # P1, P2, P3
                        if masked:
                            assert torch.equal(z[mask], known[mask])                                     # a held element is the hold's value
                        moved += int((side != 0).sum())
                        assert bool((side < 0).any()) and bool((side > 0).any())
    assert moved > 0


def test_a_zero_limit_continues_at_constant_velocity_and_the_box_wins():
    """a = 0 and v = inf from start == start2: the joint does not move; from a moving start it runs at that velocity into the box, which
    wins - the second difference at that row exceeds a (no braking ahead of the box), and the rows after it stay on the bound."""
    x0 = torch.randn(1, 8, 1, generator=torch.Generator().manual_seed(0))
    a, v, lo, hi = torch.tensor([0.0]), torch.tensor([INF]), torch.tensor([-1.0]), torch.tensor([1.0])
    z, _ = accel_ref.scan(x0, a, torch.tensor([[0.25]]), v, torch.tensor([[0.25]]), lo, hi)
    assert z.flatten().tolist() == [0.25] * 8
    z, _ = accel_ref.scan(x0, a, torch.tensor([[0.0]]), v, torch.tensor([[0.25]]), lo, hi)
    assert z.flatten().tolist() == [0.5, 0.75, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0]
    assert accel_ref.check_properties(z, a, torch.tensor([[0.0]]), v, torch.tensor([[0.25]]), lo, hi, torch.ones(1, 8, 1, dtype=torch.bool)) == (True, True, True)
    # the row where the box won: 1.0 - 2 * 1.0 + 0.75 = -0.25, beyond a = 0 - exempt, because A = [1.25, 1.25] misses the box
    # ... and without a box or a slew limit the scan runs away from the prediction: the velocity is never taken back
    z, _ = accel_ref.scan(torch.zeros(1, 50, 1), torch.tensor([0.01]), torch.tensor([[0.0]]), v, torch.tensor([[1.0]]), torch.tensor([-INF]), torch.tensor([INF]))
    assert float(z.max()) > 10.0


def test_a_held_row_enters_the_state_as_the_holds_value():
    x0 = torch.zeros(1, 5, 1)
    known = torch.full((1, 5, 1), 2.0)
    mask = torch.zeros(1, 5, 1, dtype=torch.bool)
    mask[0, 1] = True
    a, v, lo, hi = torch.tensor([0.5]), torch.tensor([INF]), torch.tensor([-INF]), torch.tensor([INF])
    z, _ = accel_ref.scan(x0, a, torch.tensor([[0.0]]), v, torch.tensor([[0.0]]), lo, hi, known, mask)
    # row 0: p = 0, stays 0.  row 1 held at 2 (a jump the scan does not limit).  row 2: p = 2 + (2 - 0) = 4, x0 = 0 is raised to 3.5.
    # row 3: p = 3.5 + 1.5 = 5 -> 4.5.  row 4: p = 4.5 + 1 = 5.5 -> 5.0: the velocity the hold brought in decays by a per row.
    assert z.flatten().tolist() == [0.0, 2.0, 3.5, 4.5, 5.0]
    assert accel_ref.check_properties(z, a, torch.tensor([[0.0]]), v, torch.tensor([[0.0]]), lo, hi, ~mask) == (True, True, True)


def test_infinite_a_without_start2_is_slew_ref_exactly():
    B, T, J, n = 3, 10, 7, 4
    g = torch.Generator().manual_seed(1)
    x_T, known = torch.randn(B, T, J, generator=g), torch.randn(B, T, J, generator=g) * 2
    mask = torch.rand(B, T, J, generator=g) < 0.3
    den = _toy_denoiser(2, J)
    lo, hi = torch.full((J,), -0.75), torch.full((J,), 0.5)
    v, start = torch.full((J,), 0.3), 0.5 * torch.randn(B, J, generator=g)
    a = torch.full((J,), INF)
    for w in (None, [0.0, 0.3, 0.2, 0.0]):
        for m, k in ((None, None), (mask, known)):
            for reproject in (False, True):
                want = slew_ref.sample(den, x_T, k, m, n, w, v, start, lo, hi, reproject)
                got = accel_ref.sample(den, x_T, k, m, n, w, a, None, v, start, lo, hi, reproject)
                for p, q in zip(want[:3] + want[4:], got[:3] + got[4:]):
                    assert all(torch.equal(s.view(torch.int32), t.view(torch.int32)) for s, t in zip(p, q))     # P4, at every step
                assert not any(bool(s.any()) for s in got[3])
    # a finite a is another rollout
    other = accel_ref.sample(den, x_T, None, None, n, None, torch.full((J,), 0.05), None, v, start, lo, hi)
    assert not torch.equal(other[0][-1], slew_ref.sample(den, x_T, None, None, n, None, v, start, lo, hi)[0][-1])


def test_nan_stays_nan_and_lifts_the_acceleration_limit_for_two_rows():
    x0 = torch.tensor([0.0, 0.0, NAN, 3.0, -3.0, 0.0, 0.0]).view(1, 7, 1)
    a, v, lo, hi = torch.tensor([0.25]), torch.tensor([INF]), torch.tensor([-INF]), torch.tensor([INF])
    z, side = accel_ref.scan(x0, a, torch.tensor([[1.0]]), v, torch.tensor([[1.0]]), lo, hi)
    # rows 0, 1: p = 1, 0.75 + (0.75 - 1) = 0.5.  row 2 NaN.  rows 3 and 4 have a NaN among their two predecessors: free.
    # row 5: p = -3 + (-3 - 3) = -9 -> -8.75.  row 6: p = -8.75 - 5.75 = -14.5 -> -14.25
    assert z.flatten()[:2].tolist() == [0.75, 0.25] and math.isnan(float(z[0, 2, 0]))
    assert z.flatten()[3:].tolist() == [3.0, -3.0, -8.75, -14.25]
    assert side.flatten().tolist() == [-1, -1, 0, 0, 0, 1, 1]                                                    # P5
    # a NaN start2 leaves row 0 free of the acceleration limit; the slew limit from start still holds
    # (row 0: 0 is raised to 1 - 0.5 by the slew limit alone; row 1: p = 0.5 + (0.5 - 1) = 0, x0 = 2 is lowered to 0.25)
    z, _ = accel_ref.scan(torch.tensor([0.0, 2.0]).view(1, 2, 1), a, torch.tensor([[NAN]]), torch.tensor([0.5]), torch.tensor([[1.0]]), lo, hi)
    assert z.flatten().tolist() == [0.5, 0.25]


def test_the_last_step_of_the_rollout_returns_the_scan():
    B, T, J, n = 2, 10, 5, 4
    g = torch.Generator().manual_seed(9)
    x_T = torch.randn(B, T, J, generator=g)
    a, v, start, start2 = torch.full((J,), 0.1), torch.full((J,), 0.3), torch.zeros(B, J), torch.full((B, J), 0.05)
    lo, hi = torch.full((J,), -1.0), torch.full((J,), 1.0)
    out, _, _, side, clean = accel_ref.sample(_toy_denoiser(3, J), x_T, None, None, n, [0.0, 0.4, 0.3, 0.0], a, start2, v, start, lo, hi, True)
    assert torch.equal(out[-1], clean[-1]) and all(bool(s.any()) for s in side)
    assert accel_ref.check_properties(out[-1], a, start2, v, start, lo, hi, torch.ones(B, T, J, dtype=torch.bool)) == (True, True, True)


def test_sequential_clamping_lands_in_the_intersection_by_brute_force():
    """P3's exemption: for intervals A, S and the box on a grid, clamp(clamp(clamp(x, A), S), box) lies in A whenever the three have a
    common point (and then in all three); where it leaves A, they have none."""
    grid = [-2.0, -1.0, -0.5, 0.0, 0.5, 1.0, 2.0]
    ivs = [(lo, hi) for lo in grid for hi in grid if lo <= hi]
    clamp = lambda x, iv: iv[0] if x < iv[0] else (iv[1] if x > iv[1] else x)
    met = missed = 0
    for A, S in itertools.product(ivs, ivs):
        for box in ivs[::3]:
            common = max(A[0], S[0], box[0]) <= min(A[1], S[1], box[1])
            for x in (-3.0, -0.75, 0.25, 3.0):
                z = clamp(clamp(clamp(x, A), S), box)
                assert box[0] <= z <= box[1]
                if common:
                    met += 1
                    assert A[0] <= z <= A[1] and S[0] <= z <= S[1], (A, S, box, x, z)
                else:
                    missed += not (A[0] <= z <= A[1])
    assert met > 1000 and missed > 1000


# ---- 2. ops.joint_accel and the accel= forms --------------------------------------------------------------------------------------------------
def test_joint_accel_pads_to_32_floats_with_infinity_and_refuses_bad_values():
    from soccerdiffusion_amd import ops

    J = 7
    a = ops.joint_accel([0.5, INF, 0.25, 0.0, 1.0, 2.0, 3.0], J=J, device="cpu")
    assert a.dtype == torch.float32 and tuple(a.shape) == (32,) and a[:J].tolist() == [0.5, INF, 0.25, 0.0, 1.0, 2.0, 3.0] and (a[J:] == INF).all()
    assert ops.joint_accel(0.75, J=J, device="cpu").tolist() == [0.75] * J + [INF] * 25
    assert ops.joint_accel({2: 0.5, 6: 0.0}, J=J, device="cpu").tolist() == [INF, INF, 0.5, INF, INF, INF, 0.0] + [INF] * 25
    assert (ops.joint_accel({}, J=32, device="cpu") == INF).all()
    J = 4
    for bad, what in (([0.5] * 3, "shape"), ([0.5, NAN, 0.5, 0.5], "NaN"), ([0.5, -0.1, 0.5, 0.5], "negative"), (-1.0, "negative"), (NAN, "NaN"),
                      ({4: 0.5}, "out of range"), ({-1: 0.5}, "out of range"), ({0: (0.0, 1.0)}, "one number"), ("abc", "expected"),
                      (torch.zeros(J, 1), "shape")):
        with pytest.raises(ValueError, match=what) as e:
            ops.joint_accel(bad, J=J, device="cpu")
        assert str(e.value).startswith("accel:")
    with pytest.raises(ValueError, match="32 joints"):
        ops.joint_accel(1.0, J=33, device="cpu")
    with pytest.raises(ValueError, match="J and device"):
        ops.joint_accel(1.0)


def test_the_accel_argument_of_a_sampler_call():
    from soccerdiffusion_amd import ops

    B, J = 3, 5
    a, start2 = ops._accel_req(0.5, B, J, "cpu")
    assert a[:J].tolist() == [0.5] * J and start2 is None
    ready = ops.joint_accel({1: 0.25}, J=J, device="cpu")
    assert ops._accel_req(ready, B, J, "cpu")[0] is ready                      # the padded array as it is
    st = torch.arange(B * J, dtype=torch.float32).view(B, J)
    a, start2 = ops._accel_req(([0.5] * J, st), B, J, "cpu")
    assert tuple(start2.shape) == (B, 32) and torch.equal(start2[:, :J], st) and bool(torch.isnan(start2[:, J:]).all())
    padded = torch.full((B, 32), NAN)
    assert ops._accel_req((ready, padded), B, J, "cpu")[1] is padded           # ... and a padded start2
    for bad, what in ((([0.5] * J, torch.zeros(B + 1, J)), "start2"), (([0.5] * J, torch.zeros(B, J + 1)), "start2"), (([0.5] * J, torch.zeros(J)), "start2"),
                      ((-0.5, None), "negative")):
        with pytest.raises(ValueError, match=what):
            ops._accel_req(bad, B, J, "cpu")
    with pytest.raises(ValueError, match="32 joints"):
        ops._accel_req(0.5, B, 33, "cpu")
    # the entry points of the feature exist with the accel keyword (before anything touches a device)
    import inspect
    for fn in (ops.ddim_sample, ops.ddim_sample_guarded, ops.direct_sample, ops.direct_sample_guarded, ops.direct_project):
        assert "accel" in inspect.signature(fn).parameters, fn.__name__
    assert callable(ops.accel_step) and callable(ops.max_accel) and "accel" in inspect.signature(ops.GraphedSampler.__init__).parameters


def test_schedulers_accept_accel():
    from soccerdiffusion_amd.scheduler import DDIMScheduler, MultistepScheduler

    for cls in (DDIMScheduler, MultistepScheduler):
        s = cls(beta_schedule="squaredcos_cap_v2", accel={1: 0.25})
        a, start2 = s._accel(torch.zeros(2, 3, 5))
        assert a[:5].tolist() == [INF, 0.25, INF, INF, INF] and start2 is None and s._limits(torch.zeros(2, 3, 5)) is None
        v, start = s._slew(torch.zeros(2, 3, 5))                               # an acceleration step carries the slew arrays: infinite ones
        assert bool((v == INF).all()) and start is None
        assert s._accel(torch.zeros(2, 9, 5))[0] is a                          # built once per (device, B, J)
        with pytest.raises(ValueError, match="whole"):
            s._accel(torch.zeros(6, 5))
        assert cls()._accel(torch.zeros(2, 3, 5)) is None and cls()._slew(torch.zeros(2, 3, 5)) is None   # the call of before


# ---- 3. the session and the cli -----------------------------------------------------------------------------------------------------------------
def test_policy_session_check_accel_needs_no_device():
    from soccerdiffusion_amd.session import PolicySession

    box = PolicySession.check_limits(2.0, 20)
    assert PolicySession.check_accel(None, 20) is None
    a = PolicySession.check_accel(0.05, 20, limits=box)
    assert a.dtype == np.float32 and a.shape == (32,) and np.allclose(a[:20], 0.05) and (a[20:] == np.inf).all()
    assert PolicySession.check_accel({3: 0.5}, 20, carry=4, limits=PolicySession.check_limits({3: (-1.0, 1.0)}, 20))[3] == 0.5
    for bad, what in ((-0.1, "negative"), ([0.1] * 19, "shape"), ({20: 0.1}, "out of range"), (NAN, "NaN")):
        with pytest.raises(ValueError, match=what):
            PolicySession.check_accel(bad, 20, limits=box)
    with pytest.raises(ValueError, match="distilled"):
        PolicySession.check_accel(0.1, 20, distilled=True, limits=box)
    assert PolicySession.check_accel(0.1, 20, distilled=True, direct=True, limits=box)[0] == np.float32(0.1)
    with pytest.raises(ValueError, match="32 joints"):
        PolicySession.check_accel(0.1, 33, limits=box)
    # a finite a needs a box that is finite on both sides for that joint
    for limits in (None, PolicySession.check_limits({3: (-1.0, INF)}, 20), PolicySession.check_limits({2: (-1.0, 1.0)}, 20)):
        with pytest.raises(ValueError, match="finite box"):
            PolicySession.check_accel({3: 0.5}, 20, limits=limits)
    assert PolicySession.check_accel({}, 20) is not None                       # nothing limited: nothing to bound


def test_cli_parses_accel():
    from soccerdiffusion_amd import cli

    p = cli.build_parser()
    assert p.parse_args(["sample", "c.pth", "--accel", "0.05"]).accel == 0.05
    assert p.parse_args(["evaluate", "c.pth", "--synthetic", "4", "--accel", "2=0.5,3=0.25"]).accel == {2: 0.5, 3: 0.25}
    assert p.parse_args(["rollout", "c.pth", "--synthetic", "1", "--ticks", "2", "--accel", "0=0"]).accel == {0: 0.0}
    assert p.parse_args(["sample", "c.pth"]).accel is None
    for bad in ("-0.1", "2=0.5,2=0.25", "x", "2=", "-1=0.5", "nan"):
        with pytest.raises(SystemExit):
            p.parse_args(["sample", "c.pth", "--accel", bad])
    args = p.parse_args(["sample", "c.pth", "--accel", "7=0.5"])
    with pytest.raises(SystemExit, match="--accel"):
        cli._accel_arg(args, {"num_joints": 7})
    assert cli._accel_arg(args, {"num_joints": 8}) == {7: 0.5}


def test_host_model_of_the_session_conversion_keeps_published_second_differences_within_a_rad():
    """sd_session_accel's arithmetic (ops.session_accel_host) on random joints, bounds, means and stds.  Triples in normalised space are
    the worst the scan allows: x2 = fl(p +- a_n) with p = fl(y1 + fl(y1 - y2)), the host model of accel_row, all three inside the box.
    Both roundings of the commit's expression - fma(x, std, mean) - pi and (x * std + mean) - pi - publish values whose second difference,
    in exact fp64, stays within a_rad; some triples come within 8 ulp of a_rad, so the margin is not slack by orders of magnitude; and
    without the margin the plain a_rad / std breaks the bound somewhere."""
    from soccerdiffusion_amd import ops

    n = 400_000
    rng = np.random.default_rng(0)
    mean = rng.uniform(0.0, 2 * math.pi, n).astype(np.float32)
    std = np.exp(rng.uniform(math.log(1e-2), math.log(3.0), n)).astype(np.float32)
    R = np.exp(rng.uniform(math.log(0.25), math.log(math.pi), n)).astype(np.float32)
    a_rad = (R * np.exp(rng.uniform(math.log(1e-3), math.log(2.0), n))).astype(np.float32)
    pi32 = np.float32(math.pi)
    a_n = ops.session_accel_host(a_rad, R, mean, std)
    margin = ops.session_accel_margin(R, mean, std)
    assert a_n.dtype == np.float32 and (a_n > 0).all() and (a_n.astype(np.float64) * std <= a_rad.astype(np.float64) - margin).all()
    assert (margin <= 2e-5).all()        # a few ulps of pi

    def fused(x):   # fma(x, std, mean) - pi: the product and the sum exactly in fp64 (24 + 24 bits), one rounding to fp32
        return ((x.astype(np.float64) * std.astype(np.float64) + mean.astype(np.float64)).astype(np.float32) - pi32).astype(np.float32)

    def plain(x):
        return ((x * std).astype(np.float32) + mean).astype(np.float32) - pi32

    def triples(limit):
        r1 = rng.uniform(-1.0, 1.0, n) * R
        r2 = np.clip(r1 + rng.uniform(-0.5, 0.5, n) * R, -R, R)
        y1 = (((r1 + math.pi) - mean) / std).astype(np.float32)
        y2 = (((r2 + math.pi) - mean) / std).astype(np.float32)
        p = (y1 + (y1 - y2).astype(np.float32)).astype(np.float32)
        for sign in (1.0, -1.0):
            yield sign, y2, y1, (p + np.float32(sign) * limit).astype(np.float32)

    ulp = np.spacing(a_rad).astype(np.float64)
    near = 0
    for sign, y2, y1, x in triples(a_n):
        for commit in (fused, plain):
            r2, r1, r0 = (commit(u).astype(np.float64) for u in (y2, y1, x))
            keep = (np.abs(r0) <= R) & (np.abs(r1) <= R) & (np.abs(r2) <= R)         # the margin's premise: every value inside the box
            assert keep.sum() > 0.2 * n
            excess = np.abs(r0 - 2.0 * r1 + r2) - a_rad.astype(np.float64)
            assert (excess[keep] <= 0).all(), (sign, commit.__name__, float(excess[keep].max()))
            near += int((excess[keep] >= -8 * ulp[keep]).sum())
    assert near > 0
    broke = False
    naive = (a_rad / std).astype(np.float32)
    for sign, y2, y1, x in triples(naive):
        r2, r1, r0 = (plain(u).astype(np.float64) for u in (y2, y1, x))
        broke |= bool((np.abs(r0 - 2.0 * r1 + r2) > a_rad.astype(np.float64)).any())
    assert broke
    # an a_rad below its margin comes out as 0; the margin follows the bound
    assert ops.session_accel_host([1e-7], [math.pi], [3.0], [1.0])[0] == 0.0
    assert ops.session_accel_margin([10.0], [0.0], [1.0])[0] > ops.session_accel_margin([math.pi], [0.0], [1.0])[0] > 0
    assert ops.session_accel_margin([math.pi], [3.0], [1.0])[0] > ops.session_slew_margin([math.pi], [3.0], [1.0])[0]


def test_normalised_accel_follows_normalised_slew():
    from soccerdiffusion_amd.evaluation import normalised_accel

    mean, std = torch.full((4,), 3.0), torch.tensor([0.5, 1.0, 2.0, 1.0])
    a = normalised_accel({1: 0.5, 3: 0.25}, mean, std)
    assert a.dtype == torch.float32 and a[0] == INF and a[2] == INF and 0.499 < float(a[1]) < 0.5 and 0.249 < float(a[3]) < 0.25
    with pytest.raises(ValueError, match="margin"):
        normalised_accel(1e-8, torch.zeros(4), torch.ones(4))


# ---- 4. the entry points ------------------------------------------------------------------------------------------------------------------------
def test_new_entry_points_are_declared_bound_and_exported(lib):
    header = open(os.path.join(REPO, "include", "soccerdiffusion_hip.h")).read()
    handle = lib.load()
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in lib.SIGNATURES, name
        fn = getattr(handle, name)
        assert fn.restype is C.c_int
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", header).group(1)
        assert len(lib.SIGNATURES[name][1]) == decl.count(",") + 1, name       # one ctypes type per declared parameter


def test_bad_arguments_are_refused_before_any_launch(lib):
    handle = lib.load()
    assert handle.sd_ddim_accel_step(None, None, None, None, None, 0.0, None, None, 0, None, None, None, None, None, None, 1, 1, 1, None) != 0
    assert handle.sd_direct_project_accel(None, None, None, None, None, None, None, None, None, None, 1, 1, 1, None) != 0
    assert handle.sd_max_accel(None, None, None, None, 1, 1, 1, None) != 0
    assert handle.sd_direct_sample_accel(None, None, None, None, None, None, None, 1, 1, 1, None, 3, None, None, 1, None, None, None, None, None, None, None) != 0
    assert handle.sd_session_anchor2(None, None, None, None, 1, 1, 1, 1, 0, 1, None) != 0
    one = (C.c_float * 1)(1.0)
    assert handle.sd_session_accel(None, one, one, None, None, 1, None) != 0
