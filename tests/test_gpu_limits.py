"""Per-joint limits on the GPU (sd_ddim_sample_limits: the limits instantiations of the trajectory step kernels, ddim_limit_step_kernel
behind the row-panel and chain routes and in the loop form) against the CPU reference tests/limits_ref.py, after EVERY denoising step, on
every route ``sampler_plan`` can return; the last step bitwise inside the limits; infinite limits against the multistep call; held elements;
several draws per context; the captured graph with ``set_limits``; the two trajectory families against each other; the schedulers'
``clip_sample`` in the reference's loop form; and a NaN prediction, which must come out as NaN."""

import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":   # the child of the family test: this file's directory is on the path, the repository is not
    sys.path.insert(0, REPO)

import limits_ref
from conftest import rel_err
from oracle import ddim_ref
from oracle import denoiser_ref as ref

TOL = 1e-4          # the project's parity bar (rel_err of conftest): tests/test_gpu_hold.py
FAMILY_TOL = 2e-5   # two instantiations on the same inputs: tests/test_gpu_hold.py
N_STEPS = 4
INF = float("inf")

CASES = [
    # route, (d, T, Mc, J, L, B), max_mode
    ("TRAJ_TUNED", (256, 10, 10, 20, 2, 3), 3),
    ("TRAJ_TUNED", (256, 20, 10, 20, 1, 3), 3),             # rows 15 | 16 across two token tiles
    ("TRAJ_TUNED", (256, 100, 10, 20, 1, 2), 3),            # the ragged seventh tile
    ("TRAJ_TUNED", (256, 10, 10, 7, 1, 2), 3),              # ragged joints: the scalar path
    ("TRAJ_TUNED_WIDE", (256, 10, 50, 20, 2, 2), 3),
    ("TRAJ_GENERIC", (128, 10, 311, 22, 2, 3), 3),
    ("TRAJ_GENERIC", (128, 10, 40, 32, 1, 2), 3),           # joint 31 limited
    ("TRAJ_GENERIC", (512, 17, 70, 20, 1, 2), 3),
    ("CHAINS_F32", (64, 10, 5, 20, 1, 2), 3),
    ("FUSED_FOLD_F16", (256, 100, 10, 20, 1, 2), 2),
    ("FUSED_FOLD", (256, 100, 10, 20, 1, 2), 1),
    ("FUSED", (256, 100, 10, 20, 1, 2), 0),
]
FAMILY_SHAPE = (256, 10, 10, 20, 2, 3)


def _limits(J):
    """+- 1 on every joint but: joint 1 unlimited, hi[2] = 0, lo[J - 1] = 0.25 - the bounds straddle a group of four and an n-tile."""
    lo, hi = torch.full((J,), -1.0), torch.full((J,), 1.0)
    lo[1], hi[1] = -INF, INF
    hi[2] = 0.0
    lo[J - 1] = 0.25
    return lo, hi


def _mask(B, T, J, seed=1):
    m = torch.rand(B, T, J, generator=torch.Generator().manual_seed(seed)) < 0.3
    m[0, 0] = True             # a whole row, an empty row and a single element in it
    m[0, 1] = False
    m[0, 1, J - 1] = True
    return m


def _host(shape, seed=0, n_ctx=None):
    """tests/test_gpu_hold.py's _setup recipe, the host part: (sd, ts, acp, x_T, known, ctx).  known is scaled by 3: many held values lie
    outside the limits."""
    d, T, Mc, J, L, B = shape
    sd = ref.synthetic_state_dict(d, J, L, seed=23 + T + d)
    g = torch.Generator().manual_seed(T * 5 + Mc + d + J + seed)
    x_T, known = torch.randn(B, T, J, generator=g), torch.randn(B, T, J, generator=g) * 3
    ctx = torch.randn(B if n_ctx is None else n_ctx, Mc, d, generator=g)
    return sd, ddim_ref.timesteps(N_STEPS).tolist(), ddim_ref.alphas_cumprod(), x_T, known, ctx


def _setup(shape, seed=0, n_ctx=None):
    """... and the packed denoiser: (sd, packed, toks, coef, w, acp, x_T, known, ctx)."""
    from soccerdiffusion_amd import ops

    d = shape[0]
    sd, ts, acp, x_T, known, ctx = _host(shape, seed, n_ctx)
    packed = ops.pack_denoiser(sd, "cuda", max_len=shape[1])
    toks = ops.step_token(torch.tensor(ts).cuda(), ops.step_frequencies(d).cuda(), sd["step_encoding.token"].cuda()).reshape(N_STEPS, d)
    coef = ops.ddim_coefficients(ts, acp, N_STEPS)
    w = ops.multistep_weights(ts, acp, N_STEPS)
    assert w[0] == 0 and w[-1] == 0 and (w[1:-1] != 0).all()
    return sd, packed, toks, coef, w, acp, x_T, known, ctx


def reference(shape, w, masked, reproject, host=None):
    """limits_ref.sample in fp32 on the oracle denoiser for one combination, and the check that the case tests something: every step clamps
    between 5 % and 80 % of the free elements and hits both a lower and an upper bound."""
    d, T, Mc, J, L, B = shape
    sd, ts, acp, x_T, known, ctx = host or _host(shape)
    lo, hi = _limits(J)
    mask = _mask(B, T, J) if masked else None
    out = limits_ref.sample(lambda x, t: ref.forward_with_context(sd, [ctx], x, torch.full((B,), t, dtype=torch.int64)), x_T,
                            known if masked else None, mask, N_STEPS, None if w is None else [float(v) for v in w], lo, hi, reproject, acp)
    free = torch.ones(B, T, J, dtype=torch.bool) if mask is None else ~mask
    fractions = []
    for i, side in enumerate(out[3]):
        fractions.append(float((side != 0)[free].float().mean()))
        assert 0.05 <= fractions[-1] <= 0.80, (shape, i, fractions)
        assert bool((side[free] < 0).any()) and bool((side[free] > 0).any()), (shape, i)
    return out, mask, free, fractions


COMBOS = [(ms, masked, reproject) for ms in (False, True) for masked in (False, True) for reproject in (False, True)]

pytestmark = pytest.mark.gpu


def _inside(x, lo, hi, free):
    J = x.shape[-1]
    return bool(((x >= lo.to(x.device)[:J]) & (x <= hi.to(x.device)[:J]))[free.to(x.device)].all())


# ---- 1. every step against the reference --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route,shape,max_mode", CASES, ids=[f"{c[0]}-{'x'.join(map(str, c[1]))}-m{c[2]}" for c in CASES])
def test_limited_rollout_every_step(route, shape, max_mode):
    from soccerdiffusion_amd import _lib, ops

    d, T, Mc, J, L, B = shape
    assert _lib.sampler_route(d, 4, T, Mc, J, L, B, max_mode) == route
    sd, packed, toks, coef, w, acp, x_T, known, ctx = _setup(shape)
    host = (sd, ddim_ref.timesteps(N_STEPS).tolist(), acp, x_T, known, ctx)
    lo, hi = _limits(J)
    lim = ops.joint_limits(lo, hi, J=J, device="cuda")
    lim_before = [t.clone() for t in lim]
    x_dev, known_dev, ctx_dev = x_T.cuda(), known.cuda(), ctx.cuda()
    for ms, masked, reproject in COMBOS:
        (want, want_held, want_eps, _), mask, free, fractions = reference(shape, w if ms else None, masked, reproject, host)
        # the final step returns the clamped x0 itself: both kinds of bound are met there
        assert bool(((want[-1] == lo) & free).any()) and bool(((want[-1] == hi) & free).any())
        words = ops.hold_mask(mask, B, T, J, "cuda") if masked else None
        hold = (known_dev, words) if masked else None
        status = torch.ones(1, dtype=torch.int32, device="cuda")
        xm, trm, epm = ops.ddim_sample(packed, ctx_dev, toks, coef, x_dev, trace=True, eps_trace=True, max_mode=max_mode, status=status, hold=hold,
                                       multistep=w if ms else None, limits=lim, reproject=reproject)
        # inputs are only read
        assert torch.equal(x_dev.cpu(), x_T) and torch.equal(known_dev.cpu(), known) and all(torch.equal(a, b) for a, b in zip(lim, lim_before))
        assert not masked or torch.equal(words, ops.hold_mask(mask, B, T, J, "cuda"))
        trm, epm = trm.cpu(), epm.cpu()
        for i in range(N_STEPS):
            e_x = rel_err(torch.where(free, trm[i], torch.zeros(())), torch.where(free, want[i], torch.zeros(())))
            e_eps = rel_err(epm[i], want_eps[i])
            print(f"{route} {shape} multistep={ms} mask={masked} reproject={reproject} step {i}: clamped {fractions[i]:.2f}, free elements {e_x:.3e}, "
                  f"eps {e_eps:.3e}")
            assert e_x < TOL and e_eps < TOL, (ms, masked, reproject, i, e_x, e_eps)
        final = trm[-1]
        assert _inside(final, lo, hi, free), (ms, masked, reproject)       # bitwise inside: the last step returns the clamped x0 itself
        if masked:   # held elements keep the hold's value whatever the limits say: bit for bit at the end, also outside the limits
            assert torch.equal(final[mask].view(torch.int32), known[mask].view(torch.int32))
            assert not _inside(final, lo, hi, mask)
            for i in range(N_STEPS):      # before: c2 K + c3 N, three roundings each, with or without contraction (tests/test_gpu_multistep.py)
                c2, c3 = float(coef[i, 2]), float(coef[i, 3])
                bound = 2.0 ** -21 * ((c2 * known.double()).abs() + (c3 * x_T.double()).abs())
                assert (((trm[i].double() - want_held[i].double()).abs() - bound)[mask] <= 0).all(), (ms, reproject, i)
        assert torch.equal(xm.cpu(), final) and int(status.item()) == 0 and torch.isfinite(xm).all()
    # the call without the traces is the same call (the last combination)
    assert torch.equal(ops.ddim_sample(packed, ctx_dev, toks, coef, x_dev, max_mode=max_mode, hold=hold, multistep=w, limits=lim, reproject=True), xm)


# ---- 2. infinite limits are the multistep call, bit for bit --------------------------------------------------------------------------------
ROUTES = [("TRAJ_TUNED", (256, 20, 10, 20, 1, 3), 3), ("TRAJ_TUNED", (256, 10, 10, 7, 1, 2), 3), ("TRAJ_TUNED_WIDE", (256, 10, 50, 20, 2, 2), 3),
          ("TRAJ_GENERIC", (128, 10, 311, 22, 2, 3), 3), ("CHAINS_F32", (64, 10, 5, 20, 1, 2), 3), ("FUSED_FOLD_F16", (256, 100, 10, 20, 1, 2), 2)]


@pytest.mark.parametrize("route,shape,max_mode", ROUTES, ids=[f"{c[0]}-J{c[1][3]}" for c in ROUTES])
def test_infinite_limits_are_the_multistep_call_bitwise(route, shape, max_mode):
    from soccerdiffusion_amd import _lib, ops

    d, T, Mc, J, L, B = shape
    assert _lib.sampler_route(d, 4, T, Mc, J, L, B, max_mode) == route
    _, packed, toks, coef, w, _, x_T, known, ctx = _setup(shape, seed=1)
    x_dev, ctx_dev = x_T.cuda(), ctx.cuda()
    hold = (known.cuda(), ops.hold_mask(_mask(B, T, J, 3), B, T, J, "cuda"))
    zero = np.zeros(N_STEPS, dtype=np.float32)
    for h in (None, hold):
        for weights in (w, zero):
            want = ops.ddim_sample(packed, ctx_dev, toks, coef, x_dev, trace=True, eps_trace=True, max_mode=max_mode, hold=h, multistep=weights)
            for reproject in (False, True):
                got = ops.ddim_sample(packed, ctx_dev, toks, coef, x_dev, trace=True, eps_trace=True, max_mode=max_mode, hold=h, multistep=weights,
                                      limits={}, reproject=reproject)
                assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(want, got)), (h is not None, reproject)
        # no weights at all (first-order DDIM under limits, no history buffer) is the zero-weight multistep call
        got = ops.ddim_sample(packed, ctx_dev, toks, coef, x_dev, trace=True, eps_trace=True, max_mode=max_mode, hold=h, limits={})
        assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(want, got))
    # and finite limits are another rollout
    assert not torch.equal(ops.ddim_sample(packed, ctx_dev, toks, coef, x_dev, max_mode=max_mode, limits=1.0), want[0])


# ---- 3. draws -------------------------------------------------------------------------------------------------------------------------------
DRAWS = [("TRAJ_TUNED", (256, 10, 10, 20, 1, 8)), ("TRAJ_GENERIC", (128, 10, 40, 22, 1, 8))]


@pytest.mark.parametrize("route,shape", DRAWS, ids=[c[0] for c in DRAWS])
def test_draws_equal_the_repeated_context_bitwise(route, shape):
    from soccerdiffusion_amd import _lib, ops

    d, T, Mc, J, L, B = shape
    G = 4
    assert _lib.sampler_route_draws(d, 4, T, Mc, J, L, B, G, 3) == route
    _, packed, toks, coef, w, _, x_T, known, ctx = _setup(shape, seed=2, n_ctx=B // G)
    lim = ops.joint_limits(*_limits(J), J=J, device="cuda")
    for hold in (None, (known.cuda(), ops.hold_mask(_mask(B, T, J, 6), B, T, J, "cuda"))):
        for weights in (None, w):
            shared, trs = ops.ddim_sample(packed, ctx.cuda(), toks, coef, x_T.cuda(), trace=True, hold=hold, draws=G, multistep=weights, limits=lim)
            repeated, trr = ops.ddim_sample(packed, ctx.cuda().repeat_interleave(G, 0).contiguous(), toks, coef, x_T.cuda(), trace=True, hold=hold,
                                            multistep=weights, limits=lim)
            assert torch.equal(trs, trr) and torch.equal(shared, repeated) and torch.isfinite(shared).all()


# ---- 4. the captured graph ------------------------------------------------------------------------------------------------------------------
def test_graphed_sampler_follows_set_limits_without_a_new_capture():
    from test_gpu_loop_form import _model

    from soccerdiffusion_amd import ops

    shape = (256, 10, 10, 20, 2, 3)
    d, T, Mc, J, L, B = shape
    _, packed, toks, coef, w, _, x_T, known, ctx = _setup(shape, seed=6)
    first, second = _limits(J), {0: (-0.5, 0.5), J - 1: (-INF, 0.0)}
    g = torch.Generator().manual_seed(8)
    for weights in (None, w):
        gs = ops.GraphedSampler(packed, B, T, Mc, toks, coef, multistep=weights, limits=True, reproject=True)
        graph = gs.graph
        for limits in (first, second):
            gs.set_limits(limits)
            x = torch.randn(B, T, J, generator=g).cuda()
            eager = ops.ddim_sample(packed, ctx.cuda(), toks, coef, x, multistep=weights, limits=limits, reproject=True)
            assert torch.equal(gs(ctx.cuda(), x), eager) and gs.graph is graph
            lim = ops._limits_req(limits, J, "cuda")
            assert _inside(eager, lim.lo, lim.hi, torch.ones(B, T, J, dtype=torch.bool))
    # a graph captured without limits takes none
    with pytest.raises(ValueError, match="limits=True"):
        ops.GraphedSampler(packed, B, T, Mc, toks, coef).set_limits(1.0)
    # pin=True on a limits graph: the pin travels as a mask
    gp = ops.GraphedSampler(packed, B, T, Mc, toks, coef, pin=True, limits=True)
    gp.set_limits(first)
    x = torch.randn(B, T, J, generator=g).cuda()
    assert torch.equal(gp(ctx.cuda(), x, pin=(known.cuda(), [3, 0, 10])), ops.ddim_sample(packed, ctx.cuda(), toks, coef, x, pin=(known.cuda(), [3, 0, 10]), limits=first))
    # model.sample(limits=...): eager equals graphed; one capture serves both sets of limits
    m, _ = _model(d, J, L, T)
    c = [torch.randn(B, Mc, d, generator=g).cuda()]
    graphs = set()
    for limits in (first, second):
        x = torch.randn(B, T, J, generator=g).cuda()
        eager = m.sample(c, x, N_STEPS, limits=limits, solver="multistep")
        assert torch.equal(eager, m.sample(c, x, N_STEPS, limits=limits, solver="multistep", use_graph=True))
        assert not torch.equal(eager, m.sample(c, x, N_STEPS, solver="multistep")) and torch.isfinite(eager).all()
        from soccerdiffusion_amd.ml.model import model as mm
        graphs |= {id(v) for v in mm._model_cache(m, "graphs").values()}
    assert len(graphs) == 1
    x2, trace = m.sample(c, x, N_STEPS, limits=second, solver="multistep", return_trace=True)
    assert torch.equal(x2, eager) and torch.equal(trace[-1], eager)


# ---- 5. the two trajectory families -----------------------------------------------------------------------------------------------------------
def _family_run():
    """The family shape under limits, every combination of solver and reproject with a mask: the traces, in the family this process's
    environment selects."""
    from soccerdiffusion_amd import _lib, ops

    d, T, Mc, J, L, B = FAMILY_SHAPE
    _, packed, toks, coef, w, _, x_T, known, ctx = _setup(FAMILY_SHAPE, seed=7)
    lim = ops.joint_limits(*_limits(J), J=J, device="cuda")
    hold = (known.cuda(), ops.hold_mask(_mask(B, T, J, 9), B, T, J, "cuda"))
    out = {"route": _lib.sampler_route(d, 4, T, Mc, J, L, B, 3)}
    for ms in (False, True):
        for reproject in (False, True):
            out[f"{int(ms)}{int(reproject)}"] = ops.ddim_sample(packed, ctx.cuda(), toks, coef, x_T.cuda(), trace=True, hold=hold, multistep=w if ms else None,
                                                                limits=lim, reproject=reproject)[1].cpu()
    return out


def test_tuned_and_generic_family_agree():
    assert "SD_TRAJ_MAXROWS" not in os.environ
    tuned = _family_run()
    env = {k: v for k, v in os.environ.items() if not k.startswith("SD_")}
    env.update(SD_TRAJ_MAXROWS="0", PYTHONPATH=REPO)      # no memory rows on the tuned family: the generic kernels take the shape
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "generic.pt")
        subprocess.run([sys.executable, os.path.abspath(__file__), path], env=env, check=True, cwd=REPO)
        generic = torch.load(path, map_location="cpu", weights_only=True)
    assert tuned.pop("route") == "TRAJ_TUNED" and generic.pop("route") == "TRAJ_GENERIC"
    for key, trace in tuned.items():
        for i in range(N_STEPS):
            err = rel_err(trace[i], generic[key][i])
            print(f"multistep, reproject = {key} step {i}: tuned against generic {err:.3e}")
            assert err < FAMILY_TOL, (key, i, err)


# ---- 6. the loop form ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,T,Mc,J,L,B", [(256, 10, 10, 20, 2, 3), (128, 10, 40, 22, 1, 2)], ids=["TRAJ_TUNED", "TRAJ_GENERIC"])
def test_schedulers_with_clip_sample_in_the_loop_form(d, T, Mc, J, L, B):
    from test_gpu_loop_form import _model

    from soccerdiffusion_amd.scheduler import DDIMScheduler, MultistepScheduler

    m, _ = _model(d, J, L, T)
    g = torch.Generator().manual_seed(d + T)
    x_T, ctx = torch.randn(B, T, J, generator=g).cuda(), [torch.randn(B, Mc, d, generator=g).cuda()]
    lo, hi = _limits(J)
    for sched, kw in ((DDIMScheduler(beta_schedule="squaredcos_cap_v2", clip_sample=True), dict(limits=1.0)),
                      (DDIMScheduler(clip_sample=True, clip_sample_range=0.5), dict(limits=0.5)),
                      (MultistepScheduler(limits=(lo, hi)), dict(limits=(lo, hi), solver="multistep"))):
        for reproject in (False, True):
            native, trace = m.sample(ctx, x_T, N_STEPS, return_trace=True, reproject=reproject, **kw)
            sched.set_timesteps(N_STEPS)
            traj = x_T
            with torch.no_grad():
                for i, t in enumerate(sched.timesteps):
                    eps = m.forward_with_context(ctx, traj, torch.full((B,), int(t), device="cuda"))
                    traj = sched.step(eps, t, traj, use_clipped_model_output=reproject).prev_sample
                    err = rel_err(traj, trace[i])
                    print(f"d = {d} {type(sched).__name__} reproject={reproject} step {i}: loop form against the native call {err:.3e}")
                    assert err < FAMILY_TOL, (i, err)
            lim = sched._limits(traj)
            assert _inside(traj, lim.lo, lim.hi, torch.ones(B, T, J, dtype=torch.bool))
            assert not torch.equal(native, m.sample(ctx, x_T, N_STEPS, solver=kw.get("solver", "ddim")))
    # clip_sample=False stays the call of before
    off = DDIMScheduler(beta_schedule="squaredcos_cap_v2", clip_sample=False)
    off.set_timesteps(N_STEPS)
    from soccerdiffusion_amd import ops
    eps = torch.randn(B, T, J, generator=g).cuda()
    t0 = int(off.timesteps[0])
    assert torch.equal(off.step(eps, t0, x_T).prev_sample, ops.ddim_step(eps, x_T, ops.ddim_coefficients([t0], off.alphas_cumprod, N_STEPS)[0]))


def test_a_nan_prediction_comes_out_of_step_as_nan_at_that_element_only():
    from soccerdiffusion_amd.scheduler import DDIMScheduler, MultistepScheduler

    B, T, J = 2, 10, 22
    g = torch.Generator().manual_seed(11)
    for cls in (DDIMScheduler, MultistepScheduler):
        for reproject in (False, True):
            sched = cls(beta_schedule="squaredcos_cap_v2", clip_sample=True)
            sched.set_timesteps(N_STEPS)
            x = torch.randn(B, T, J, generator=g).cuda() * 2
            for i, t in enumerate(sched.timesteps):
                eps = torch.randn(B, T, J, generator=g).cuda()
                eps[1, 3, 21] = float("nan")
                out = sched.step(eps, t, x, use_clipped_model_output=reproject).prev_sample
                nan = torch.isnan(out)
                assert bool(nan[1, 3, 21]) and int(nan.sum()) == 1, (cls.__name__, reproject, i)
                x = torch.where(nan, torch.zeros_like(out), out)
            assert bool(((x >= -1) & (x <= 1))[~nan].all())


def test_a_nan_prediction_comes_out_of_the_step_kernels_as_nan():
    """The clamp inside the step kernels of both families: a NaN element of x_T has a NaN x0 at every step whatever the network predicts,
    and the limited rollout returns NaN there, not a limit; the other trajectory is finite and inside the limits."""
    from soccerdiffusion_amd import ops

    for shape in ((256, 10, 10, 20, 1, 2), (128, 10, 40, 22, 1, 2)):
        d, T, Mc, J, L, B = shape
        _, packed, toks, coef, w, _, x_T, _, ctx = _setup(shape, seed=8)
        x_T = x_T.clone()
        x_T[1, 4, 5] = float("nan")
        for reproject in (False, True):
            out = ops.ddim_sample(packed, ctx.cuda(), toks, coef, x_T.cuda(), multistep=w, limits=1.0, reproject=reproject)
            assert bool(torch.isnan(out[1, 4, 5])) and torch.isfinite(out[0]).all() and bool(((out[0] >= -1) & (out[0] <= 1)).all())


if __name__ == "__main__":   # the child of the family test: the same run in the family its environment selects -> argv[1]
    torch.save(_family_run(), sys.argv[1])
    sys.exit(0)
