"""A distilled one-step decoder under held elements, joint limits and slew limits on the GPU (sd_direct_sample: the direct instantiations
of both trajectory step-kernel families; direct_project_kernel behind the eps launches of the other routes and on its own) against the
numpy restatement tests/direct_ref.py - BITWISE: given the prediction, the projection is compares, selects and one fp32 add and one
subtract per row.  The prediction itself is ``forward_with_context(ctx, x_T, zeros)`` bit for bit."""

import numpy as np
import pytest
import torch

import direct_ref
from test_gpu_session import TINY, _synthetic_model

pytestmark = pytest.mark.gpu
B = 5
CASES = [
    # route, (d, L, Mc, J, T)
    ("TRAJ_TUNED", (256, 2, 12, 20, 10)),          # one token tile
    ("TRAJ_TUNED", (256, 2, 12, 20, 33)),          # three tiles, the last partial: the scan crosses two wave boundaries
    ("TRAJ_TUNED", (256, 2, 12, 20, 100)),         # seven tiles
    ("TRAJ_TUNED_WIDE", (256, 2, 40, 20, 10)),
    ("TRAJ_TUNED_WIDE", (256, 2, 40, 20, 33)),
    ("TRAJ_GENERIC", (128, 2, 70, 22, 10)),        # J & 3: the element-by-element path
    ("TRAJ_GENERIC", (512, 1, 12, 20, 17)),
]
IDS = [f"{c[0]}-d{c[1][0]}-Mc{c[1][2]}-J{c[1][3]}-T{c[1][4]}" for c in CASES]
_models: dict = {}


def _bits(t):
    t = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t, dtype=np.float32)
    return np.ascontiguousarray(t).view(np.int32)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _model(d, L, J):
    """One model per (hidden_dim, layers, joints), horizon 100 (48 at hidden_dim 512: the generic family's cap): shorter horizons read
    the leading rows of its positional table."""
    key = (d, L, J)
    if key not in _models:
        params = {**TINY, "hidden_dim": d, "num_decoder_layers": L, "num_joints": J, "trajectory_prediction_length": 48 if d == 512 else 100}
        _models[key] = _synthetic_model(params)[0]
    return _models[key]


def _case(shape, seed=0, n_ctx=B):
    d, L, Mc, J, T = shape
    g = torch.Generator().manual_seed(7 * T + Mc + d + J + seed)
    return _model(d, L, J), torch.randn(B, T, J, generator=g).cuda(), torch.randn(n_ctx, Mc, d, generator=g).cuda()


def _device_args(c):
    """direct_ref.constraints_from's dictionary as the keyword arguments of ops.direct_sample / model.sample_direct."""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return dict(hold=(t(c["known"]), t(c["mask"])), limits=(t(c["lo"]), t(c["hi"])), slew=(t(c["v"]), t(c["start"])))


@pytest.mark.parametrize("route,shape", CASES, ids=IDS)
def test_direct_sample_is_forward_with_context_then_the_reference_projection(route, shape):
    from soccerdiffusion_amd import _lib, ops

    d, L, Mc, J, T = shape
    assert _lib.sampler_route(d, 4, T, Mc, J, L, B, 3) == route
    model, x_T, ctx = _case(shape)
    x_before = x_T.clone()
    with torch.no_grad():
        want_raw = model.forward_with_context([ctx], x_T, torch.zeros(B, dtype=torch.int64, device="cuda"))
        # 1. / 2.: nothing set - out is raw is forward_with_context, bit for bit
        out, raw = model.sample_direct([ctx], x_T, raw=True)
    assert _same(raw, want_raw), "raw != forward_with_context"
    assert _same(out, raw), "out != raw with nothing set"
    assert _same(model.sample_direct([ctx], x_T), out)           # the call without the raw buffer is the same call
    # 3. constraints chosen from raw itself
    c = direct_ref.constraints_from(raw.cpu().numpy(), seed=T)
    kw = _device_args(c)
    with torch.no_grad():
        out, raw2 = model.sample_direct([ctx], x_T, raw=True, **kw)
    assert _same(raw2, raw) and _same(x_T, x_before)             # the prediction is written for every row, held or not; x is only read
    want = direct_ref.project(raw.cpu().numpy(), **c)
    assert _same(out, want), f"{int((_bits(out) != _bits(want)).sum())} elements differ from direct_ref"
    o, free = out.cpu().numpy(), ~c["mask"]
    assert bool(((o >= c["lo"]) & (o <= c["hi"]))[free].all())
    assert np.array_equal(o[c["mask"]].view(np.int32), c["known"][c["mask"]].view(np.int32))
    share = direct_ref.moved_share(raw.cpu().numpy(), o, c["mask"])
    print(f"{route} {shape}: the projection moved {share:.2f} of the free elements")
    assert 0.10 <= share <= 0.90, share
    # each constraint alone and pairs of them: the kernel's branches (no mask, no scan, a scan without an anchor)
    packed = model.diffusion_action_generator.packed()
    token = ops.step_token(torch.zeros(1, dtype=torch.int64, device="cuda"), model.step_encoding._freq, model.step_encoding.token.detach())
    for keys in (("limits",), ("hold",), ("slew",), ("hold", "limits"), ("limits", "slew")):
        sub = {k: kw[k] for k in keys}
        ref_kw = dict(lo=c["lo"], hi=c["hi"]) if "limits" in keys else {}
        if "hold" in keys:
            ref_kw.update(known=c["known"], mask=c["mask"])
        if "slew" in keys:
            ref_kw.update(v=c["v"], start=c["start"])
        got = ops.direct_sample(packed, ctx, token, x_T, **sub)
        assert _same(got, direct_ref.project(raw.cpu().numpy(), **ref_kw)), keys
    got = ops.direct_sample(packed, ctx, token, x_T, slew=kw["slew"][0])             # v without start
    assert _same(got, direct_ref.project(raw.cpu().numpy(), v=c["v"]))
    # 6. the projection alone equals the fused launch: the two implementations of the scan agree
    assert _same(ops.direct_project(raw, **kw), out)


@pytest.mark.parametrize("route,shape", CASES, ids=IDS)
def test_draws_share_the_context_bitwise(route, shape):
    d, L, Mc, J, T = shape
    model, x_T, ctx = _case(shape, seed=1, n_ctx=2)
    x6 = x_T.repeat(2, 1, 1)[:6].contiguous() + torch.arange(6, device="cuda").view(6, 1, 1) * 0.125
    with torch.no_grad():
        raw = model.sample_direct([ctx.repeat_interleave(3, 0)], x6)
        c = direct_ref.constraints_from(raw.cpu().numpy(), seed=3)
        kw = _device_args(c)
        wide = model.sample_direct([ctx.repeat_interleave(3, 0)], x6, raw=True, **kw)
        shared = model.sample_direct([ctx], x6, draws=3, raw=True, **kw)
    assert _same(shared[0], wide[0]) and _same(shared[1], wide[1])
    assert not _same(shared[0][0], shared[0][1])                  # G noises give G different trajectories


@pytest.mark.parametrize("route,shape", CASES, ids=IDS)
def test_eps_then_projection_route(route, shape):
    """max_mode = 2: no trajectory kernel - the eps launches, then direct_project_kernel; the repeat after a tripped guard runs this."""
    from soccerdiffusion_amd import _lib, ops

    d, L, Mc, J, T = shape
    assert not _lib.sampler_route(d, 4, T, Mc, J, L, B, 2).startswith("TRAJ_")
    model, x_T, ctx = _case(shape, seed=2)
    packed = model.diffusion_action_generator.packed()
    token = ops.step_token(torch.zeros(1, dtype=torch.int64, device="cuda"), model.step_encoding._freq, model.step_encoding.token.detach())
    status = torch.ones(1, dtype=torch.int32, device="cuda")
    out, raw = ops.direct_sample(packed, ctx, token, x_T, raw=True, max_mode=2, status=status)
    assert _same(out, raw) and int(status.item()) == 0
    c = direct_ref.constraints_from(raw.cpu().numpy(), seed=T + 1)
    kw = _device_args(c)
    out, raw2 = ops.direct_sample(packed, ctx, token, x_T, raw=True, max_mode=2, status=status, **kw)
    assert _same(raw2, raw) and int(status.item()) == 0
    assert _same(out, direct_ref.project(raw.cpu().numpy(), **c))
    assert _same(ops.direct_sample(packed, ctx, token, x_T, max_mode=2, **kw), out)   # without a raw buffer: the prediction in the workspace
    fused = ops.direct_sample(packed, ctx, token, x_T, max_mode=3)
    err = float((fused - raw).abs().max() / raw.abs().max())
    print(f"{route} {shape}: mode 3 against mode 2, max abs error / max |raw| = {err:.3e}")
    assert err < 1e-4                                             # the project's parity bar between two routes of the same network


def test_direct_project_special_values():
    """Planted NaN, -0 and +-inf: a NaN stays NaN and limits nothing after it, -0 is kept, an infinite prediction comes out as its limit
    (or stays infinite where that side has none)."""
    from soccerdiffusion_amd import ops

    rng = np.random.default_rng(5)
    Bn, T, J = 4, 37, 22
    raw = rng.standard_normal((Bn, T, J)).astype(np.float32)
    raw[0, 3, 0], raw[0, 20, 5], raw[1, 0, 2] = np.nan, np.nan, np.nan
    raw[1, 5, 1], raw[2, 0, 7] = -0.0, -0.0
    raw[2, 9, 3], raw[3, 30, 21], raw[3, 31, 21], raw[0, 0, 9] = np.inf, -np.inf, np.inf, np.inf
    c = direct_ref.constraints_from(np.nan_to_num(raw, nan=0.0, posinf=3.0, neginf=-3.0), seed=9)
    c["lo"][1], c["hi"][1], c["v"][1] = -1.0, 0.0, np.inf        # -0 inside [-1, 0]: kept
    c["mask"][:, :, 1] = False
    c["mask"][:, :, 4] = True
    c["lo"][7], c["v"][7] = 0.0, np.inf                           # -0 at its lower limit +0: -0 < 0 is false, kept
    c["hi"][9], c["lo"][21] = np.inf, -np.inf                     # no limit on the side the infinity lies
    c["mask"][1, 5, 1] = c["mask"][2, 0, 7] = c["mask"][2, 9, 3] = c["mask"][3, 30, 21] = c["mask"][3, 31, 21] = c["mask"][0, 0, 9] = False
    c["mask"][0, 3, 0] = c["mask"][0, 20, 5] = c["mask"][1, 0, 2] = False
    want = direct_ref.project(raw, **c)
    got = ops.direct_project(torch.from_numpy(raw).cuda(), **_device_args(c))
    assert _same(got, want)
    g = got.cpu().numpy()
    assert np.isnan(g[0, 3, 0]) and np.isnan(g[0, 20, 5]) and np.isnan(g[1, 0, 2])
    assert np.signbit(g[1, 5, 1]) and g[1, 5, 1] == 0 and np.signbit(g[2, 0, 7]) and g[2, 0, 7] == 0
    assert np.isfinite(g[2, 9, 3]) and g[2, 9, 3] <= c["hi"][3]   # the scan's upper bound or the box, whichever is lower
    assert np.isfinite(g[3, 30, 21]) and np.isfinite(g[3, 31, 21])
    assert g[0, 0, 9] == np.inf                                   # row 0 of an even trajectory is free, and that side has no limit
    # with nothing set the projection is the identity on the bits
    assert _same(ops.direct_project(torch.from_numpy(raw).cuda()), raw)
    # limits alone: the infinite predictions come out as the limits
    only = ops.direct_project(torch.from_numpy(raw).cuda(), limits=(torch.from_numpy(c["lo"]), torch.from_numpy(c["hi"]))).cpu().numpy()
    assert only[2, 9, 3] == c["hi"][3] and only[3, 31, 21] == c["hi"][21] and only[0, 0, 9] == np.inf and only[3, 30, 21] == -np.inf
    assert _same(only, direct_ref.project(raw, lo=c["lo"], hi=c["hi"]))


def test_guarded_call_and_argument_errors():
    from soccerdiffusion_amd import ops

    shape = CASES[0][1]
    model, x_T, ctx = _case(shape, seed=4)
    packed = model.diffusion_action_generator.packed()
    token = ops.step_token(torch.zeros(1, dtype=torch.int64, device="cuda"), model.step_encoding._freq, model.step_encoding.token.detach())
    assert _same(ops.direct_sample_guarded(packed, ctx, token, x_T, limits=0.5), ops.direct_sample(packed, ctx, token, x_T, limits=0.5))
    assert float(ops.direct_sample(packed, ctx, token, x_T, limits=0.5).abs().max()) <= 0.5
    with pytest.raises(ValueError, match="draws"):
        ops.direct_sample(packed, ctx, token, x_T, draws=2)
    with pytest.raises(ValueError, match="token"):
        ops.direct_sample(packed, ctx, torch.zeros(2, shape[0], device="cuda"), x_T)
    with pytest.raises(ValueError, match="negative"):
        ops.direct_sample(packed, ctx, token, x_T, slew=-1.0)
    with pytest.raises(ValueError, match="lo"):
        ops.direct_project(x_T, limits=(torch.ones(shape[3]), torch.zeros(shape[3])))
