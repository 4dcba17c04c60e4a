"""A distilled one-step decoder under limits, slew limits and holds, the parts that need no GPU: the numpy restatement tests/direct_ref.py
against tests/slew_ref.py's last step and on special values; the quantile construction of the GPU tests' constraints; what PolicySession
and the command line accept and still refuse for a distilled decoder; the two entry points in the header and in the built library."""

import argparse
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import direct_ref
import slew_ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF, NAN = np.float32(np.inf), np.float32(np.nan)


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.int32)


# ---- 1. the reference ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(3, 10, 20), (2, 33, 22), (4, 100, 7)])
def test_direct_ref_is_the_last_step_of_slew_ref(shape):
    """slew_ref's step with c2 = 1, c3 = 0 returns x0c itself: on finite random inputs the two restatements agree bit for bit."""
    B, T, J = shape
    g = torch.Generator().manual_seed(B * T + J)
    x0, e, known = torch.randn(B, T, J, generator=g), torch.randn(B, T, J, generator=g), torch.randn(B, T, J, generator=g) * 3
    mask = torch.rand(B, T, J, generator=g) < 0.3
    v = torch.rand(J, generator=g) * 0.5
    v[1] = float("inf")
    start = torch.randn(B, J, generator=g)
    start[::2] = float("nan")
    lo, hi = -torch.rand(J, generator=g) - 0.1, torch.rand(J, generator=g) + 0.1
    lo[2], hi[3] = -float("inf"), float("inf")
    for kn, m in ((known, mask), (None, None)):
        for st in (start, None):
            x0c, _ = slew_ref.scan(x0, v, st, lo, hi, kn, m)
            last = 1.0 * x0c + 0.0 * e                      # the update of the last step: c2 x0c + c3 e
            got = direct_ref.project(x0.numpy(), None if kn is None else kn.numpy(), None if m is None else m.numpy(), lo.numpy(), hi.numpy(),
                                     v.numpy(), None if st is None else st.numpy())
            assert np.array_equal(_bits(got), _bits(last.numpy())) and np.array_equal(_bits(got), _bits(x0c.numpy()))
    # no slew limit at all is the box alone
    box = torch.where(x0 < lo, lo, torch.where(x0 > hi, hi, x0))
    assert np.array_equal(_bits(direct_ref.project(x0.numpy(), lo=lo.numpy(), hi=hi.numpy())), _bits(box.numpy()))
    # nothing set: the identity on the bits
    assert np.array_equal(_bits(direct_ref.project(x0.numpy())), _bits(x0.numpy()))


def test_nan_stays_nan_and_limits_nothing_after_it():
    raw = np.array([[[0.0], [NAN], [5.0], [5.2], [9.0]]], dtype=np.float32)
    out = direct_ref.project(raw, lo=[-10.0], hi=[10.0], v=[0.5], start=np.array([[0.1]], dtype=np.float32))
    assert out[0, 0, 0] == 0.0 and np.isnan(out[0, 1, 0])
    assert out[0, 2, 0] == 5.0                               # the row behind the NaN is free: a NaN y limits nothing
    assert out[0, 3, 0] == 5.2 and out[0, 4, 0] == np.float32(np.float32(5.2) + np.float32(0.5))
    # ... and the box does not turn it into a number either
    assert np.isnan(direct_ref.project(raw, lo=[-1.0], hi=[1.0])[0, 1, 0])


def test_negative_zero_is_kept():
    raw = np.array([[[-0.0, -0.0, -0.0, 0.0]]], dtype=np.float32)
    out = direct_ref.project(raw, lo=[-1.0, 0.0, -INF, 0.0], hi=[0.0, 1.0, INF, 0.0], v=[INF, 1.0, 1.0, INF],
                             start=np.array([[0.0, 0.0, NAN, NAN]], dtype=np.float32))
    assert np.array_equal(_bits(out), _bits(raw))            # -0 < +0 and -0 > +0 are both false: no bound replaces it
    assert np.signbit(out[0, 0, :3]).all() and not np.signbit(out[0, 0, 3])


def test_infinite_prediction_comes_out_as_its_limit():
    raw = np.array([[[INF, -INF, INF, -INF]], [[INF, -INF, INF, -INF]]], dtype=np.float32)
    out = direct_ref.project(raw, lo=[-2.0, -3.0, -INF, -INF], hi=[2.0, 3.0, INF, INF])
    assert out[0, 0].tolist() == [2.0, -3.0, np.inf, -np.inf]             # the box; an open side leaves the infinity
    start = np.array([[1.0, 1.0, 1.0, NAN], [NAN, NAN, NAN, NAN]], dtype=np.float32)
    out = direct_ref.project(raw, lo=[-2.0, -3.0, -INF, -INF], hi=[2.0, 3.0, INF, INF], v=[0.5, 0.5, 0.5, 0.5], start=start)
    assert out[0, 0].tolist() == [1.5, 0.5, 1.5, -np.inf]                 # the scan's bound where there is an anchor
    assert out[1, 0].tolist() == [2.0, -3.0, np.inf, -np.inf]
    assert np.isfinite(out[:, :, :2]).all()


def test_held_element_is_known_whatever_the_limits_say():
    raw = np.zeros((1, 4, 2), dtype=np.float32)
    known = np.full((1, 4, 2), 7.0, dtype=np.float32)
    known[0, 2, 0] = NAN
    mask = np.zeros((1, 4, 2), dtype=bool)
    mask[0, 1:3, 0] = True
    out = direct_ref.project(raw, known, mask, lo=[-1.0, -1.0], hi=[1.0, 1.0], v=[0.25, 0.25], start=np.zeros((1, 2), dtype=np.float32))
    assert out[0, 1, 0] == 7.0 and np.isnan(out[0, 2, 0])    # outside the box and beyond v: the hold's value as it stands
    assert out[0, 3, 0] == 0.0                               # (a NaN held value limits nothing behind it)
    assert (out[0, :, 1] == 0.0).all() and out[0, 0, 0] == 0.0
    # a free row behind a held one is limited from the held value, then by the box
    known[0, 2, 0] = 7.0
    out = direct_ref.project(raw, known, mask, lo=[-1.0, -1.0], hi=[1.0, 1.0], v=[0.25, 0.25])
    assert out[0, 3, 0] == 1.0


@pytest.mark.parametrize("shape", [(5, 10, 20), (5, 33, 20), (5, 100, 20), (5, 10, 22), (5, 17, 20), (6, 33, 20)])
def test_quantile_constraints_bind_on_any_scale(shape):
    """The condition the GPU tests assert on their inputs - the projection moves between 10 % and 90 % of the free elements - is met by the
    construction itself, whatever the scale of the prediction."""
    for seed, scale in enumerate((1e-3, 1.0, 40.0)):
        raw = (np.random.default_rng(seed).standard_normal(shape) * scale).astype(np.float32)
        c = direct_ref.constraints_from(raw, seed)
        out = direct_ref.project(raw, **c)
        share = direct_ref.moved_share(raw, out, c["mask"])
        assert 0.10 <= share <= 0.90, (shape, scale, share)
        free = ~c["mask"]
        assert ((out >= c["lo"]) & (out <= c["hi"]))[free].all()
        assert np.array_equal(out[c["mask"]].view(np.int32), c["known"][c["mask"]].view(np.int32))
        assert c["mask"][:, :, 1].all() and 0.15 < c["mask"][:, :, 2:].mean() < 0.25
        assert np.isnan(c["start"][0::2]).all() and np.isfinite(c["start"][1::2]).all()


# ---- 2. the session and the command line -------------------------------------------------------------------------------------------------------
def test_policy_session_accepts_a_distilled_decoder_with_direct():
    """With ``direct=True`` the checks no longer raise for a distilled decoder; without it they refuse as they always did, so that no
    existing call behaves differently, and the message names the flag."""
    from soccerdiffusion_amd.session import PolicySession

    D = dict(distilled=True, direct=True)
    assert PolicySession.check_draws(4, "coherent", **D) == (4, "coherent")
    assert PolicySession.check_hold(True, 20, **D) is True
    lo, hi = PolicySession.check_limits(1.5, 20, **D)
    assert lo[0] == -1.5 and hi[19] == 1.5 and np.isinf(hi[20])
    assert PolicySession.check_slew(0.1, 20, **D)[5] == np.float32(0.1)
    assert PolicySession.check_carry(10, 0, 5, distilled=True) == (0, 5)
    assert PolicySession.check_reproject(False, True) is False and PolicySession.check_reproject(True, False) is True
    assert PolicySession.check_direct(True, True) is True and PolicySession.check_direct(False, True) is False
    with pytest.raises(ValueError, match="32"):              # the other checks stand
        PolicySession.check_hold(True, 33, **D)
    with pytest.raises(ValueError, match="negative"):
        PolicySession.check_slew(-0.1, 20, **D)
    for call in (lambda: PolicySession.check_draws(4, "coherent", distilled=True), lambda: PolicySession.check_hold(True, 20, distilled=True),
                 lambda: PolicySession.check_limits(1.5, 20, distilled=True), lambda: PolicySession.check_slew(0.1, 20, distilled=True)):
        with pytest.raises(ValueError, match="distilled.*direct=True"):
            call()
    with pytest.raises(ValueError, match="predicts noise"):
        PolicySession.check_direct(True, distilled=False)


def test_policy_session_still_refuses_carry_multistep_and_reproject():
    from soccerdiffusion_amd.session import PolicySession

    with pytest.raises(ValueError, match="distilled"):
        PolicySession.check_carry(10, 1, None, distilled=True)
    with pytest.raises(ValueError, match="distilled"):
        PolicySession.check_solver("multistep", 20, 0, distilled=True)
    with pytest.raises(ValueError, match="distilled.*no eps"):
        PolicySession.check_reproject(True, distilled=True)

    class Model:   # the constructor validates before it looks at a device: no parameters are touched
        trajectory_prediction_length = 10
        num_joints = 20

    with pytest.raises(ValueError, match="carry"):
        PolicySession(Model(), carry=1, distilled=True, direct=True)
    with pytest.raises(ValueError, match="solver"):
        PolicySession(Model(), solver="multistep", draws=4, holds=True, limits=1.0, slew=0.1, distilled=True, direct=True)
    with pytest.raises(ValueError, match="reproject"):
        PolicySession(Model(), limits=1.0, reproject=True, direct=True, hyperparams={"distilled_decoder": True})
    with pytest.raises(ValueError, match="direct=True"):
        PolicySession(Model(), limits=1.0, hyperparams={"distilled_decoder": True})


def test_cli_accepts_and_refuses_for_a_distilled_checkpoint():
    from soccerdiffusion_amd import cli

    student = {"distilled_decoder": True, "num_joints": 20}
    ns = lambda **kw: argparse.Namespace(**{"limits": None, "clip": None, "reproject": False, "slew": None, "solver": "ddim", "carry": 0, **kw})
    assert cli._limits_arg(ns(clip=1.5), student) == 1.5
    assert cli._limits_arg(ns(limits=[(3, -1.0, 1.0)]), student) == {3: (-1.0, 1.0)}
    assert cli._slew_arg(ns(slew=0.1), student) == 0.1 and cli._slew_arg(ns(slew={2: 0.1}), student) == {2: 0.1}
    assert cli._distilled_arg(ns(clip=1.5, slew=0.1), student) is None
    with pytest.raises(SystemExit, match="--reproject"):
        cli._limits_arg(ns(clip=1.5, reproject=True), student)
    with pytest.raises(SystemExit, match="--reproject"):
        cli._distilled_arg(ns(clip=1.5, reproject=True), student)
    with pytest.raises(SystemExit, match="--solver"):
        cli._distilled_arg(ns(solver="multistep"), student)
    with pytest.raises(SystemExit, match="--carry"):
        cli._distilled_arg(ns(carry=4), student)
    with pytest.raises(SystemExit, match="joint indices"):   # the other argument errors stand
        cli._slew_arg(ns(slew={20: 0.1}), student)
    # a teacher's checkpoint is refused nothing
    assert cli._distilled_arg(ns(solver="multistep", carry=4, reproject=True), {"num_joints": 20}) is None
    # the parsers take the options on every command (which checkpoint they meet is decided at run time)
    a = cli.build_parser().parse_args(["rollout", "c.pt", "--synthetic", "2", "--draws", "4", "--select", "coherent", "--advance", "5", "--slew", "0.1",
                                       "--clip", "1.5", "--hold", "0=0.3", "--coherence-decay", "0.5", "--contrast", "0.1"])
    assert a.draws == 4 and a.select == "coherent" and a.slew == 0.1 and a.clip == 1.5


# ---- 3. the ABI --------------------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_direct_entry_points():
    from soccerdiffusion_amd import _lib, build

    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "soccerdiffusion_hip.h")).read(), flags=re.S)
    for name in ("sd_direct_sample", "sd_direct_project"):
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert name in _lib.SIGNATURES
    build.build()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (sd_[a-z0-9_]+)", out))
    assert {"sd_direct_sample", "sd_direct_project"} <= exported
    h = _lib.load()
    # argument errors are answered before anything touches a device
    assert h.sd_direct_project(None, None, None, None, None, None, None, None, 1, 1, 1, None) == -1
    assert b"sd_direct_project" in h.sd_last_error()
    assert h.sd_direct_sample(None, None, None, None, None, None, None, 1, 1, 1, None, 3, None, None, 1, None, None, None, None, None) == -1
    assert b"sd_direct_sample" in h.sd_last_error()
