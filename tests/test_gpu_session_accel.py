"""Acceleration limits of the policy session on the GPU (``PolicySession(accel=...)``: sd_session_accel, sd_session_anchor2, the
acceleration-limited rollout or direct launch underneath).

Plumbing: eager and replayed ticks are the same bit for bit under every composition (limits + slew + accel, two held joints, draws = 4
coherent, a partial reset, a subset tick; rollout and ``direct=True``), and the committed rows are ``ops.ddim_sample`` /
``ops.direct_sample`` called with the session's own device arrays and anchors.

Property: every published triple of consecutive rows - inside a tick and across two ticks - is in one of three cases: its last value lies
within the box margin of a published bound, its last step lies within the slew margin of +- v_rad, or its second difference is <= a_rad
in exact fp64.  (A row that the scan leaves outside its acceleration interval was moved there by the slew clamp or by the box clamp, so it
lies on one of their edges: the three cases are all there are.)  The conditions that keep this honest: at most 25 % of the triples use an
exemption and at least 10 % lie within 8 ulp of a_rad (ulp: of the commit's largest intermediate, the unit of tests/test_gpu_session_slew.py).
The limits are constants, fixed once from what the session WITHOUT options publishes (three ticks, measured on an MI355X; per joint the
90 % quantile of |step| is 1.05 - 1.77 rad on the rollout and 0.10 - 0.28 on the direct decoder, the 25 % quantile of |second difference|
0.29 - 0.76 and 0.03 - 0.10): the box +- 1.5 rad, v_rad = 1.25 / 0.14 and a_rad = 0.4 / 0.05 on every joint - an unlimited session exceeds
a_rad on about three triples in four.  They do not adapt to what the code under test gives.  A CPU restatement of the whole session
(encoders included) does not exist in this repository, so the shares are asserted on the GPU; the shares measured with these constants
are written at the constants below."""

import math

import numpy as np
import pytest
import torch

from test_gpu_session import _same_bits
from test_gpu_session_direct import ADVANCE, B, FREE, G, J, JOINTS, T, V, _model, _push, _sensors

pytestmark = pytest.mark.gpu
STEPS = 4
LIMIT = 1.5                       # radians as published: the box every joint with a finite a needs
EXEMPT, AT_LIMIT = 0.25, 0.10     # at most that share of the triples uses an exemption; at least that share lies within 8 ulp of a_rad
V_RAD = {False: 1.25, True: 0.14}   # [direct]: radians per row as published, every joint (see the module docstring)
A_RAD = {False: 0.4, True: 0.05}    # [direct]: radians per row^2 as published, every joint
# measured with these constants on an MI355X, 1836 triples per case over four ticks: rollout 3.2 - 4.0 % exempt and 24 - 26 % within 8 ulp
# of a_rad (hidden_dim 128 / 64); direct 0.0 % exempt and 66 % within 8 ulp


def _params(d, direct):
    m, params = _model(d)
    return m, (params if direct else {**params, "distilled_decoder": False})


def _constraints(d, direct):
    """(v_rad, a_rad) of a case, (J,) fp32 each: the constants above on every joint."""
    return torch.full((J,), V_RAD[direct]), torch.full((J,), A_RAD[direct])


def _ulp(model, bound):
    """One ulp of the commit's largest intermediate, per joint (tests/test_gpu_session_slew.py's unit)."""
    m = model.mean.detach().cpu().numpy().astype(np.float32)
    return torch.from_numpy(np.spacing(np.float32(bound + math.pi) + np.abs(m)).astype(np.float64))


@pytest.mark.parametrize("direct", [False, True], ids=["rollout", "direct"])
@pytest.mark.parametrize("d", [64, 128])
def test_eager_and_replayed_ticks_and_the_published_triples(d, direct):
    from soccerdiffusion_amd import ops
    from soccerdiffusion_amd.session import PolicySession

    m, params = _params(d, direct)
    v_rad, a_rad = _constraints(d, direct)
    kw = dict(batch=B, hyperparams=params, seed=3, limits=LIMIT, slew=v_rad, accel=a_rad, holds=True, draws=G, select="coherent", advance=ADVANCE)
    kw.update(dict(direct=True) if direct else dict(num_inference_steps=STEPS))
    eager, graphed = PolicySession(m, **kw), PolicySession(m, use_graph=True, **kw)
    assert eager._accel_a is not None and bool(torch.isnan(eager._anchor2).all()) and eager.distilled == direct
    for s in (eager, graphed):
        s.hold(JOINTS, V)
    ulp = _ulp(m, LIMIT)[FREE]
    v, a = v_rad.double()[FREE], a_rad.double()[FREE]
    mean, std = m.mean.detach().cpu().numpy()[:J], m.std.detach().cpu().numpy()[:J]
    slew_margin = torch.from_numpy(ops.session_slew_margin(np.full(J, LIMIT), mean, std))[FREE]
    g = torch.Generator().manual_seed(92)
    last = torch.full((B, 2, J), float("nan"), dtype=torch.float64)          # the robots' last two committed rows
    graph, triples, exempt, near = None, 0, 0, 0
    for tick, robots in enumerate((None, None, None, [0, 2])):
        if tick == 2:
            for s in (eager, graphed):
                s.reset(robots=[1])
            last[1] = float("nan")                                        # the limit does not reach across the reset
            assert bool(torch.isnan(eager._anchor2.view(B, -1)[1]).all()) and bool(torch.isfinite(eager._anchor2.view(B, G, 32)[0, :, :J]).all())
        idx = list(range(B)) if robots is None else robots
        S = len(idx)
        _push((eager, graphed), *_sensors(g, S), robots=robots)
        x_T = torch.randn(S * G, T, J, generator=g).cuda()
        p, q = eager.step(x_T, robots=robots), graphed.step(x_T, robots=robots)
        assert _same_bits(p, q), tick
        assert _same_bits(eager._anchor, graphed._anchor) and _same_bits(eager._anchor2, graphed._anchor2), tick
        if robots is None:
            graph = graph or graphed._graph.graph
            assert graphed._graph.graph is graph                          # captured once; reset(robots=...) keeps the capture
        pub = p.cpu()
        assert torch.isfinite(pub).all() and bool((pub[:, :, FREE].abs() <= LIMIT).all()), tick
        r = torch.cat([last[idx], pub.double()], 1)[:, :, FREE]              # rows -2, -1, 0 .. T-1
        second = (r[:, 2:] - 2 * r[:, 1:-1] + r[:, :-2]).abs()
        step = (r[:, 2:] - r[:, 1:-1]).abs()
        there = ~torch.isnan(second)                                      # (no anchors: the first two rows are free)
        # the box margin: sd_session_limits takes the first normalised value whose commit lies inside, so a value on the bound is published
        # within one step of the commit's grid of it - one ulp of x times std, below one ulp of the largest intermediate - plus the
        # commit's three roundings of half such an ulp on either side: 4 ulp
        at_box = (r[:, 2:].abs() >= LIMIT - 4 * ulp)
        # the slew margin: v_n std <= v_rad - margin, rounded toward zero (one fp32 ulp of v_n, times std), and a step at the limit is
        # published within the margin of v_n std (the margin is what the scan's and the commit's roundings can add - or take away)
        at_slew = step >= v - 2 * slew_margin - torch.from_numpy(std[FREE].astype(np.float64) * np.spacing((v_rad.numpy()[FREE] / std[FREE]).astype(np.float32)))
        inside = second <= a
        assert bool((inside | at_box | at_slew | ~there).all()), (tick, float((second - a)[there & ~at_box & ~at_slew].max()))
        triples += int(there.sum())
        exempt += int((there & ~inside).sum())
        near += int((there & inside & (second >= a - 8 * ulp)).sum())
        last[idx] = pub[:, ADVANCE - 2:ADVANCE].double()
    print(f"d {d} {'direct' if direct else 'rollout'}: {triples} triples, {exempt / triples:.3f} use an exemption, {near / triples:.3f} within 8 ulp of a_rad")
    assert exempt / triples <= EXEMPT and near / triples >= AT_LIMIT, (exempt / triples, near / triples)
    # set_accel keeps the capture and takes effect in both
    for s in (eager, graphed):
        s.set_accel(1e9)
    _push((eager, graphed), *_sensors(g, B))
    x_T = torch.randn(B * G, T, J, generator=g).cuda()
    assert _same_bits(eager.step(x_T), graphed.step(x_T)) and graphed._graph.graph is graph


@pytest.mark.parametrize("direct", [False, True], ids=["rollout", "direct"])
def test_committed_rows_are_the_sampler_call_on_the_sessions_own_arrays(direct):
    from soccerdiffusion_amd import ops
    from soccerdiffusion_amd.session import PolicySession

    d = 128
    m, params = _params(d, direct)
    v_rad, a_rad = _constraints(d, direct)
    kw = dict(batch=B, hyperparams=params, seed=3, limits=LIMIT, slew=v_rad, accel=a_rad, advance=ADVANCE)
    kw.update(dict(direct=True) if direct else dict(num_inference_steps=STEPS))
    s = PolicySession(m, **kw)
    packed = m.diffusion_action_generator.packed()
    ts = ops.ddim_timesteps(STEPS)
    g = torch.Generator().manual_seed(93)
    for tick in range(3):
        _push((s,), *_sensors(g, B))
        x_T = torch.randn(B, T, J, generator=g).cuda()
        anchor, anchor2 = s._anchor.clone(), s._anchor2.clone()
        with torch.no_grad():
            ctx = torch.cat(s._context(), dim=1).contiguous()
            if direct:
                token = ops.step_token(s._t0[:1], m.step_encoding._freq, m.step_encoding.token.detach()).view(1, m.hidden_dim)
                x = ops.direct_sample(packed, ctx, token, x_T, limits=s._limits, slew=(s._slew_v, anchor), accel=(s._accel_a, anchor2))
            else:
                x = ops.ddim_sample(packed, ctx, m.step_encoding.table(ts, "cuda"), ops.ddim_coefficients(ts, ops.alphas_cumprod(), STEPS), x_T,
                                    limits=s._limits, slew=(s._slew_v, anchor), accel=(s._accel_a, anchor2))
        pub = s.step(x_T)
        assert _same_bits(pub, (x * m.std + m.mean) - math.pi), tick
        # the anchors of the next tick: the last two committed rows, in normalised space as sampled
        assert _same_bits(s._anchor[:, :J], x[:, ADVANCE - 1]) and _same_bits(s._anchor2[:, :J], x[:, ADVANCE - 2]), tick
        assert bool(torch.isnan(s._anchor2[:, J:]).all())
        assert tick == 0 or bool(torch.isfinite(anchor2[:, :J]).all())


def test_a_session_without_a_finite_box_raises_and_reset_frees_the_next_two_rows():
    from soccerdiffusion_amd.session import PolicySession

    m, params = _params(64, False)
    v_rad, a_rad = _constraints(64, False)
    for limits in (None, {0: (-1.0, 1.0)}, (torch.full((J,), -1.0), torch.full((J,), float("inf")))):
        with pytest.raises(ValueError, match="finite box"):
            PolicySession(m, num_inference_steps=STEPS, batch=B, hyperparams=params, limits=limits, accel=a_rad)
    s = PolicySession(m, num_inference_steps=STEPS, batch=B, hyperparams=params, seed=3, limits=LIMIT, accel=a_rad)
    assert s._slew_v is not None and bool((s._slew_v == float("inf")).all())     # the acceleration call carries infinite slew arrays
    with pytest.raises(ValueError, match="finite box"):
        s.set_limits({0: (-1.0, 1.0)})                                            # ... and the box may not be taken away afterwards
    with pytest.raises(ValueError, match="margin"):
        s.set_accel(1e-7)
    with pytest.raises(RuntimeError, match="without accel"):
        PolicySession(m, num_inference_steps=STEPS, batch=B, hyperparams=params).set_accel(1.0)
    g = torch.Generator().manual_seed(94)
    a = a_rad.double()
    ticks = []
    for tick in range(3):
        if tick == 2:
            s.reset(robots=[0])
            assert bool(torch.isnan(s._anchor[0]).all()) and bool(torch.isnan(s._anchor2[0]).all())
            assert bool(torch.isfinite(s._anchor[1:, :J]).all()) and bool(torch.isfinite(s._anchor2[1:, :J]).all())
        _push((s,), *_sensors(g, B, T))
        ticks.append(s.step(torch.randn(B, T, J, generator=g).cuda()).cpu().double())
    # across the seam of ticks 1 | 2 robot 0 is free on its first two rows, robots 1 and 2 are not (inside the box: no exemption applies)
    r = torch.cat([ticks[1][:, -2:], ticks[2][:, :2]], 1)
    second = (r[:, 2:] - 2 * r[:, 1:-1] + r[:, :-2]).abs()
    off_box = (r[:, 2:].abs() < LIMIT - 1e-5)
    assert bool(((second <= a) | ~off_box)[1:].all()) and bool(((second > a) & off_box)[0].any())
    s.reset()
    assert bool(torch.isnan(s._anchor).all()) and bool(torch.isnan(s._anchor2).all())
    plain = PolicySession(m, num_inference_steps=STEPS, batch=B, hyperparams=params, seed=3)   # a session without accel is the session of before
    assert plain._accel_a is None and plain._anchor2 is None and plain._lim() == {}


def test_session_accel_matches_its_host_model_and_anchor2_shifts_the_anchors():
    from soccerdiffusion_amd import ops

    Jn = 32
    g = torch.Generator().manual_seed(95)
    mean, std = (torch.rand(Jn, generator=g) * 6).float(), (torch.rand(Jn, generator=g) * 2 + 0.01).float()
    a = (torch.rand(Jn, generator=g) * 0.5 + 1e-3).float()
    a[3] = float("inf")
    bound = np.full(Jn, math.pi, dtype=np.float32)
    out = ops.session_accel(ops.joint_accel({}, J=Jn, device="cuda"), a.numpy(), bound, mean.cuda(), std.cuda(), Jn).cpu().numpy()
    want = ops.session_accel_host(a.numpy(), bound, mean.numpy(), std.numpy())
    assert out[3] == np.inf and np.array_equal(np.delete(out, 3), np.delete(want, 3))
    with pytest.raises(ValueError, match="margin"):
        ops.session_accel(ops.joint_accel({}, J=Jn, device="cuda"), np.full(Jn, 1e-7, dtype=np.float32), bound, mean.cuda(), std.cuda(), Jn)
    # sd_session_anchor2: row >= 1 takes rows (row - 1, row); row == 0 moves the old anchor down; only the robots named; slots [J, 32) stay
    S, Bn, Tn, Jx, draws = 2, 3, 5, 7, 2
    x = torch.randn(S, Tn, Jx, generator=g).cuda()
    first = torch.randn(Bn * draws, 32, generator=g).cuda()
    second = torch.randn(Bn * draws, 32, generator=g).cuda()
    for row in (3, 0):
        a1, a2 = first.clone(), second.clone()
        ops.session_anchor2(a1, a2, x, row, draws, robots=[2, 0])
        for s_, b in enumerate((2, 0)):
            for k in range(draws):
                at = b * draws + k
                assert torch.equal(a1[at, :Jx], x[s_, row]) and torch.equal(a2[at, :Jx], x[s_, row - 1] if row else first[at, :Jx])
                assert torch.equal(a1[at, Jx:], first[at, Jx:]) and torch.equal(a2[at, Jx:], second[at, Jx:])
        assert torch.equal(a1[draws:2 * draws], first[draws:2 * draws]) and torch.equal(a2[draws:2 * draws], second[draws:2 * draws])   # robot 1
