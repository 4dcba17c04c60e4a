"""Per-joint acceleration limits on the GPU (sd_ddim_sample_accel: the acceleration instantiations of the trajectory step kernels,
ddim_accel_step_kernel behind the row-panel and chain routes and in the loop form, direct_project_accel_kernel, max_accel_kernel) against
the CPU reference tests/accel_ref.py.

The yardstick of a rollout is a bitwise chain, not a rollout tolerance: the scan's bounds are 2 y1 - y2, so the map from the predicted
noise to the sample is not non-expansive (at T = 100 with the acceleration limit alone a 1e-6 relative perturbation of every step's eps
moves the final sample by 0.5: the runaway), and the parity bar of the slew tests does not carry over to the sample.  Per step i of every
route: (a) eps_i against the oracle denoiser evaluated at the GPU's own x_{i-1} - no scan sits between the two, so the project's bar
(rel_err < 1e-4) carries over - and (b) x_i == ops.accel_step(eps_i, x_{i-1}, coef[i], ...) bit for bit with the history chained, where
ops.accel_step is itself held to accel_ref.scan bit for bit on the kernel's own x0.  The last step satisfies P1 to P3 bitwise.

The scan can run away from the prediction where neither a box nor a slew limit holds it: in the T = 100 case with held elements (scaled
by 3) the sample reaches max |x| = 1.44e6 after step 0 and 3.3e6 later - on the CPU reference too.  The step kernels split x into fp16 parts
as it stands at the embedding, so the acceleration twins scale every row of x by a power of two there once its max |x| reaches 2^15
(x_token_scale, sd_common.h; test 8b below); in range the scale is 1 and the embedding is the slew twins' bit for bit (test 3).

Measured on an MI355X: on all twelve routes and all sixteen combinations every step's chain is bitwise and eps is within 1.1e-6 of the
oracle (bar 1e-4), the runaway combinations included."""

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

import accel_ref
from conftest import rel_err
from oracle import ddim_ref
from oracle import denoiser_ref as ref
from test_gpu_limits import CASES, FAMILY_SHAPE, N_STEPS, _host, _limits, _mask, _setup
from test_gpu_slew import _slew

TOL = 1e-4          # the project's parity bar (rel_err of conftest), for eps at the GPU's own x: teacher-forced, no scan in between
FAMILY_TOL = 2e-5   # two instantiations on the same inputs: tests/test_gpu_limits.py
INF = float("inf")
NAN = float("nan")
# (multistep, mask, box, finite slew, reproject): DDIM / multistep x mask x box x slew-finite / slew-infinite, reproject on in one combination
COMBOS = [(ms, masked, box, sl, ms and masked and box and sl) for ms in (False, True) for masked in (False, True) for box in (False, True)
          for sl in (False, True)]


def _accel(shape, seed=0):
    """a = 0.5 on every joint but a[1] = inf and a[2] = 0.25; start2 = start + 0.25 randn(B, J) with start2[:, 4] = NaN."""
    d, T, Mc, J, L, B = shape
    a = torch.full((J,), 0.5)
    a[1], a[2] = INF, 0.25
    _, start = _slew(shape, seed)
    start2 = start + 0.25 * torch.randn(B, J, generator=torch.Generator().manual_seed(200 + seed + J + B))
    start2[:, 4] = NAN
    return a, start2


def _box(J, box):
    return _limits(J) if box else (torch.full((J,), -INF), torch.full((J,), INF))


def _v(shape, finite):
    v, start = _slew(shape)
    return (v if finite else torch.full_like(v, INF)), start


def reference(shape, w, masked, box, finite, reproject, host):
    """The check that the case tests something, on the CPU reference alone (accel_ref.sample in fp32 on the oracle denoiser): at every
    step between 5 % and 95 % of the free elements are moved by the acceleration clamp, and both sides occur.  Returns the shares."""
    d, T, Mc, J, L, B = shape
    sd, ts, acp, x_T, known, ctx = host
    a, start2 = _accel(shape)
    v, start = _v(shape, finite)
    lo, hi = _box(J, box)
    mask = _mask(B, T, J) if masked else None
    out = accel_ref.sample(lambda x, t: ref.forward_with_context(sd, [ctx], x, torch.full((B,), t, dtype=torch.int64)), x_T,
                           known if masked else None, mask, N_STEPS, None if w is None else [float(u) for u in w], a, start2, v, start, lo, hi,
                           reproject, acp)
    free = torch.ones(B, T, J, dtype=torch.bool) if mask is None else ~mask
    fractions = []
    for i, side in enumerate(out[3]):
        fractions.append(float((side != 0)[free].float().mean()))
        assert 0.05 <= fractions[-1] <= 0.95, (shape, i, fractions)
        assert bool((side[free] < 0).any()) and bool((side[free] > 0).any()), (shape, i)
    return fractions


def _pad(t, B, J):
    out = torch.full((B, 32), NAN)
    out[:, :J] = t
    return out.cuda()


def _bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


pytestmark = pytest.mark.gpu


# ---- 1. the elementwise kernel: ops.accel_step is the reference scan, bit for bit ----------------------------------------------------------------
def test_accel_step_is_the_reference_scan_bitwise():
    """ops.accel_step against accel_ref.scan on the kernel's own x0.  torch on the CPU has no fp32 fma, so x0 = fma(-c1, e, x) / c0 is taken
    from the kernel (infinite a and v, no box: the history then holds x0 itself); the scan after it has no fma - compares and rounded sums
    and differences - and x0c is compared bit for bit.  x = fma(c2, x0c, c3 e) + w (hist - x0c) is held to 2 ulp of its fp64 value's
    magnitude."""
    from soccerdiffusion_amd import ops

    g = torch.Generator().manual_seed(5)
    for B, T, J in ((3, 10, 20), (2, 100, 7), (5, 17, 32)):
        eps, x, hist0 = (torch.randn(B, T, J, generator=g) for _ in range(3))
        known = torch.randn(B, T, J, generator=g) * 2
        mask = _mask(B, T, J, 4)
        shape = (0, T, 0, J, 0, B)
        v, start = _slew(shape, seed=1)
        a, start2 = _accel(shape, seed=1)
        lo, hi = _limits(J)
        coef4, w = (0.8, 0.6, 0.9, 0.43588989), 0.37
        for masked in (False, True):
            hold = (known.cuda(), ops.hold_mask(mask, B, T, J, "cuda")) if masked else None
            x0 = torch.empty(B, T, J).cuda()
            ops.accel_step(eps.cuda(), x.cuda(), coef4, INF, hist=x0)
            x0 = x0.cpu()
            want, _ = accel_ref.scan(x0, a, start2, v, start, lo, hi, known if masked else None, mask if masked else None)
            hist = hist0.clone().cuda()
            out = ops.accel_step(eps.cuda(), x.cuda(), coef4, (a, start2), slew=(v, start), limits=(lo, hi), hist=hist, w=w, hold=hold).cpu()
            assert _bits(hist.cpu(), want), (B, T, J, masked)
            c = [torch.tensor(u, dtype=torch.float32).double() for u in coef4]
            exact = c[2] * want.double() + c[3] * eps.double() + torch.tensor(w, dtype=torch.float32).double() * (hist0.double() - want.double())
            scale = (c[2] * want.double()).abs() + (c[3] * eps.double()).abs() + (hist0.double() - want.double()).abs()
            assert bool(((out.double() - exact).abs() <= 2 * 2.0 ** -23 * scale).all()), (B, T, J, masked)
            assert (want != x0).float().mean() > 0.05
            # the acceleration limit is what moved some of them: the slew call gives another x0c
            only_slew = torch.empty(B, T, J).cuda()
            ops.slew_step(eps.cuda(), x.cuda(), coef4, (v, start), limits=(lo, hi), hist=only_slew, hold=hold)
            assert not torch.equal(only_slew.cpu(), want)


# ---- 2. every route: the bitwise chain and the teacher-forced eps ---------------------------------------------------------------------------------
@pytest.mark.parametrize("route,shape,max_mode", CASES, ids=[f"{c[0]}-{'x'.join(map(str, c[1]))}-m{c[2]}" for c in CASES])
def test_accelerated_rollout_is_a_bitwise_chain_of_steps(route, shape, max_mode):
    from soccerdiffusion_amd import _lib, ops

    d, T, Mc, J, L, B = shape
    assert _lib.sampler_route(d, 4, T, Mc, J, L, B, max_mode) == route
    sd, packed, toks, coef, w, acp, x_T, known, ctx = _setup(shape)
    ts = ddim_ref.timesteps(N_STEPS).tolist()
    host = (sd, ts, acp, x_T, known, ctx)
    a, start2 = _accel(shape)
    a_dev, start2_dev = ops.joint_accel(a, J=J, device="cuda"), _pad(start2, B, J)
    x_dev, known_dev, ctx_dev = x_T.cuda(), known.cuda(), ctx.cuda()
    bad = []   # every miss of every combination (the assertion stands at the end, so that one run reports them all)
    for ms, masked, box, finite, reproject in COMBOS:
        combo = f"multistep={ms} mask={masked} box={box} slew={finite} reproject={reproject}"
        fractions = reference(shape, w if ms else None, masked, box, finite, reproject, host)
        v, start = _v(shape, finite)
        v_dev, start_dev = ops.joint_slew(v, J=J, device="cuda"), _pad(start, B, J)
        before = [t.clone() for t in (a_dev, start2_dev, v_dev, start_dev)]
        lo, hi = _box(J, box)
        mask = _mask(B, T, J) if masked else None
        free = torch.ones(B, T, J, dtype=torch.bool) if mask is None else ~mask
        words = ops.hold_mask(mask, B, T, J, "cuda") if masked else None
        hold = (known_dev, words) if masked else None
        status = torch.ones(1, dtype=torch.int32, device="cuda")
        kw = dict(max_mode=max_mode, hold=hold, multistep=w if ms else None, limits=(lo, hi) if box else None, reproject=reproject,
                  slew=(v_dev, start_dev), accel=(a_dev, start2_dev))
        xm, trm, epm = ops.ddim_sample(packed, ctx_dev, toks, coef, x_dev, trace=True, eps_trace=True, status=status, **kw)
        # held elements never pass through the scan's result: they are the slew rollout's (sd_ddim_sample_slew, the same hold), bit for bit
        held_trace = ops.ddim_sample(packed, ctx_dev, toks, coef, x_dev, trace=True, **{k: u for k, u in kw.items() if k != "accel"})[1] if masked else None
        # inputs are only read
        assert torch.equal(x_dev.cpu(), x_T) and torch.equal(known_dev.cpu(), known)
        assert all(_bits(p, q) for p, q in zip((a_dev, start2_dev, v_dev, start_dev), before))
        assert not masked or torch.equal(words, ops.hold_mask(mask, B, T, J, "cuda"))
        # the entry of a held rollout: held elements start at c0[0] known + c1[0] x_T
        x_prev = x_dev
        if masked:
            entry = float(coef[0][0]) * known_dev + float(coef[0][1]) * x_dev
            x_prev = torch.where(mask.cuda(), entry, x_dev)
        hist = torch.empty_like(x_dev)
        for i in range(N_STEPS):
            # (a) eps_i against the oracle at the GPU's own x_{i-1}
            want_eps = ref.forward_with_context(sd, [ctx], x_prev.cpu(), torch.full((B,), ts[i], dtype=torch.int64))
            e_eps = rel_err(epm[i].cpu(), want_eps)
            # (b) x_i == accel_step(eps_i, x_{i-1}, coef[i]), history chained; a held element is the hold's own update
            step = ops.accel_step(epm[i], x_prev, coef[i], (a_dev, start2_dev), slew=(v_dev, start_dev), limits=(lo, hi), hist=hist,
                                  w=float(w[i]) if ms else 0.0, reproject=reproject, hold=hold)
            if masked:   # (accel_step cannot produce the hold launch's value: the slew rollout's held elements stand in, bit for bit)
                step = torch.where(mask.cuda(), held_trace[i], step)
            same = _bits(step, trm[i])   # every element, held ones included
            print(f"{route} {shape} {combo} step {i}: moved {fractions[i]:.2f}, eps {e_eps:.3e}, chain {'bitwise' if same else 'DIFFERS'}, "
                  f"max |x| {float(trm[i].abs().max()):.3g}")
            if not e_eps < TOL:
                bad.append((combo, i, "eps", e_eps))
            if not same:
                bad.append((combo, i, "chain"))
            if masked:   # ... and those are the hold's expression c2 known + c3 x_T, to rounding
                held = float(coef[i][2]) * known_dev + float(coef[i][3]) * x_dev
                if not rel_err(trm[i][mask.cuda()].cpu(), held[mask.cuda()].cpu()) < 1e-6:
                    bad.append((combo, i, "held"))
            x_prev = trm[i]
        final = trm[-1].cpu()
        p1, p2, p3 = accel_ref.check_properties(final, a, start2, v, start, lo, hi, free)     # bitwise: the last step returns x0c itself
        if not (p1 and p2 and p3):
            bad.append((combo, "P1 P2 P3", p1, p2, p3))
        if masked and not _bits(final[mask], known[mask]):   # held elements keep the hold's value, bit for bit at the end
            bad.append((combo, "held at the end"))
        if not (torch.equal(xm.cpu(), final) and int(status.item()) == 0):
            bad.append((combo, "status", int(status.item())))
        # the call without the traces is the same call
        if not _bits(ops.ddim_sample(packed, ctx_dev, toks, coef, x_dev, **kw), xm):
            bad.append((combo, "without traces"))
    assert not bad, bad


# ---- 3. P4: infinite a without start2 is the slew call, bit for bit ---------------------------------------------------------------------------------
ROUTES = [("TRAJ_TUNED", (256, 20, 10, 20, 1, 3), 3), ("TRAJ_TUNED_WIDE", (256, 10, 50, 20, 2, 2), 3), ("TRAJ_GENERIC", (128, 10, 311, 22, 2, 3), 3),
          ("FUSED_FOLD_F16", (256, 100, 10, 20, 1, 2), 2)]


@pytest.mark.parametrize("route,shape,max_mode", ROUTES, ids=[c[0] for c in ROUTES])
def test_infinite_accel_is_the_slew_call_bitwise(route, shape, max_mode):
    from soccerdiffusion_amd import _lib, ops

    d, T, Mc, J, L, B = shape
    assert _lib.sampler_route(d, 4, T, Mc, J, L, B, max_mode) == route
    _, packed, toks, coef, w, _, x_T, known, ctx = _setup(shape, seed=1)
    x_dev, ctx_dev = x_T.cuda(), ctx.cuda()
    hold = (known.cuda(), ops.hold_mask(_mask(B, T, J, 3), B, T, J, "cuda"))
    lim, slew = _limits(J), _slew(shape)
    for h in (None, hold):
        for weights in (None, w):
            for reproject in (False, True):
                kw = dict(trace=True, eps_trace=True, max_mode=max_mode, hold=h, multistep=weights, limits=lim, reproject=reproject, slew=slew)
                want = ops.ddim_sample(packed, ctx_dev, toks, coef, x_dev, **kw)
                got = ops.ddim_sample(packed, ctx_dev, toks, coef, x_dev, accel=INF, **kw)
                assert all(_bits(p, q) for p, q in zip(want, got)), (h is not None, weights is not None, reproject)
    # and a finite a gives another rollout
    assert not torch.equal(ops.ddim_sample(packed, ctx_dev, toks, coef, x_dev, max_mode=max_mode, limits=lim, slew=slew, accel=0.25),
                           ops.ddim_sample(packed, ctx_dev, toks, coef, x_dev, max_mode=max_mode, limits=lim, slew=slew))


# ---- 4. draws -------------------------------------------------------------------------------------------------------------------------------
DRAWS = [("TRAJ_TUNED", (256, 10, 10, 20, 1, 8)), ("TRAJ_GENERIC", (128, 10, 40, 22, 1, 8))]


@pytest.mark.parametrize("route,shape", DRAWS, ids=[c[0] for c in DRAWS])
def test_draws_equal_the_repeated_context_bitwise(route, shape):
    from soccerdiffusion_amd import _lib, ops

    d, T, Mc, J, L, B = shape
    G = 8
    assert _lib.sampler_route_draws(d, 4, T, Mc, J, L, B, G, 3) == route
    _, packed, toks, coef, w, _, x_T, known, ctx = _setup(shape, seed=2, n_ctx=B // G)
    slew, accel = _slew(shape), _accel(shape)
    for hold in (None, (known.cuda(), ops.hold_mask(_mask(B, T, J, 6), B, T, J, "cuda"))):
        for weights in (None, w):
            shared, trs = ops.ddim_sample(packed, ctx.cuda(), toks, coef, x_T.cuda(), trace=True, hold=hold, draws=G, multistep=weights, limits=_limits(J),
                                          slew=slew, accel=accel)
            repeated, trr = ops.ddim_sample(packed, ctx.cuda().repeat_interleave(G, 0).contiguous(), toks, coef, x_T.cuda(), trace=True, hold=hold,
                                            multistep=weights, limits=_limits(J), slew=slew, accel=accel)
            assert torch.equal(trs, trr) and torch.equal(shared, repeated) and torch.isfinite(shared).all()


# ---- 5. the captured graph ------------------------------------------------------------------------------------------------------------------
def test_graphed_sampler_follows_set_accel_without_a_new_capture():
    from soccerdiffusion_amd import ops

    shape = (256, 10, 10, 20, 2, 3)
    d, T, Mc, J, L, B = shape
    _, packed, toks, coef, w, _, x_T, known, ctx = _setup(shape, seed=6)
    same = 0.25 * torch.randn(B, J, generator=torch.Generator().manual_seed(3))
    first, second = _accel(shape), ({0: 0.125, J - 1: 0.0}, same)
    g = torch.Generator().manual_seed(8)
    for weights in (None, w):
        gs = ops.GraphedSampler(packed, B, T, Mc, toks, coef, multistep=weights, accel=True)
        graph = gs.graph
        for accel, slew in ((first, _slew(shape)), (second, (INF, same))):
            gs.set_slew(slew)
            gs.set_accel(accel)
            x = torch.randn(B, T, J, generator=g).cuda()
            eager = ops.ddim_sample(packed, ctx.cuda(), toks, coef, x, multistep=weights, slew=slew, accel=accel)
            assert torch.equal(gs(ctx.cuda(), x), eager) and gs.graph is graph
            a, start2 = ops._accel_req(accel, B, J, "cuda")
            v, start = ops._slew_req(slew, B, J, "cuda")
            p = accel_ref.check_properties(eager.cpu(), a[:J].cpu(), None if start2 is None else start2[:, :J].cpu(), v[:J].cpu(),
                                           None if start is None else start[:, :J].cpu(), torch.full((J,), -INF), torch.full((J,), INF),
                                           torch.ones(B, T, J, dtype=torch.bool))
            assert p == (True, True, True)
        # a = 0 and v = inf from start == start2: the joint does not move
        assert bool((eager[:, :, J - 1] == same[:, J - 1].cuda().unsqueeze(1)).all())
    # a graph captured without accel takes none
    with pytest.raises(ValueError, match="accel=True"):
        ops.GraphedSampler(packed, B, T, Mc, toks, coef, slew=True).set_accel(1.0)


def test_model_sample_with_accel_eager_equals_graphed_on_one_capture():
    from test_gpu_loop_form import _model

    shape = (256, 10, 10, 20, 2, 3)
    d, T, Mc, J, L, B = shape
    g = torch.Generator().manual_seed(8)
    m, _ = _model(d, J, L, T)
    c = [torch.randn(B, Mc, d, generator=g).cuda()]
    graphs = set()
    for accel in (_accel(shape), {0: 0.125, J - 1: 0.0}):
        x = torch.randn(B, T, J, generator=g).cuda()
        eager = m.sample(c, x, N_STEPS, accel=accel, limits=2.0, solver="multistep")
        assert torch.equal(eager, m.sample(c, x, N_STEPS, accel=accel, limits=2.0, solver="multistep", use_graph=True))
        assert not torch.equal(eager, m.sample(c, x, N_STEPS, limits=2.0, solver="multistep")) and torch.isfinite(eager).all()
        from soccerdiffusion_amd.ml.model import model as mm
        graphs |= {id(u) for u in mm._model_cache(m, "graphs").values()}
    assert len(graphs) == 1


# ---- 6. the two trajectory families -----------------------------------------------------------------------------------------------------------
def _family_run():
    """The family shape (T = 10) under acceleration limits with box and slew on, both solvers with a mask: the traces, in the family this
    process's environment selects."""
    from soccerdiffusion_amd import _lib, ops

    d, T, Mc, J, L, B = FAMILY_SHAPE
    _, packed, toks, coef, w, _, x_T, known, ctx = _setup(FAMILY_SHAPE, seed=7)
    hold = (known.cuda(), ops.hold_mask(_mask(B, T, J, 9), B, T, J, "cuda"))
    out = {"route": _lib.sampler_route(d, 4, T, Mc, J, L, B, 3)}
    for ms in (False, True):
        for reproject in (False, True):
            out[f"{int(ms)}{int(reproject)}"] = ops.ddim_sample(packed, ctx.cuda(), toks, coef, x_T.cuda(), trace=True, hold=hold, multistep=w if ms else None,
                                                                limits=_limits(J), reproject=reproject, slew=_slew(FAMILY_SHAPE),
                                                                accel=_accel(FAMILY_SHAPE))[1].cpu()
    return out


def test_tuned_and_generic_family_agree():
    """T = 10 with box and slew on: there the measured sensitivity of the sample to the predicted noise is the slew test's (2e-7 to 5e-5
    per 1e-6), so the slew test's bar is kept as it is."""
    assert "SD_TRAJ_MAXROWS" not in os.environ
    tuned = _family_run()
    env = {k: u for k, u in os.environ.items() if not k.startswith("SD_")}
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


# ---- 7. the loop form ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,T,Mc,J,L,B", [(256, 10, 10, 20, 2, 3), (128, 10, 40, 22, 1, 2)], ids=["TRAJ_TUNED", "TRAJ_GENERIC"])
def test_schedulers_with_accel_in_the_loop_form_bitwise(d, T, Mc, J, L, B):
    from test_gpu_loop_form import _model

    from soccerdiffusion_amd.scheduler import DDIMScheduler, MultistepScheduler

    m, _ = _model(d, J, L, T)
    g = torch.Generator().manual_seed(d + T)
    x_T, ctx = torch.randn(B, T, J, generator=g).cuda(), [torch.randn(B, Mc, d, generator=g).cuda()]
    shape = (d, T, Mc, J, L, B)
    slew, accel = _slew(shape), _accel(shape)
    lim = _limits(J)
    for sched, kw in ((DDIMScheduler(beta_schedule="squaredcos_cap_v2", accel=accel), dict(accel=accel)),
                      (DDIMScheduler(limits=lim, slew=slew, accel=accel), dict(limits=lim, slew=slew, accel=accel)),
                      (MultistepScheduler(limits=lim, slew=slew, accel=accel), dict(limits=lim, slew=slew, accel=accel, solver="multistep"))):
        for reproject in (False, True):
            native, trace = m.sample(ctx, x_T, N_STEPS, return_trace=True, reproject=reproject, **kw)
            sched.set_timesteps(N_STEPS)
            traj = x_T
            with torch.no_grad():
                for i, t in enumerate(sched.timesteps):
                    eps = m.forward_with_context(ctx, traj, torch.full((B,), int(t), device="cuda"))
                    traj = sched.step(eps, t, traj, use_clipped_model_output=reproject).prev_sample
                    assert _bits(traj, trace[i]), (type(sched).__name__, reproject, i)
            assert not torch.equal(native, m.sample(ctx, x_T, N_STEPS, solver=kw.get("solver", "ddim"), limits=kw.get("limits"), slew=kw.get("slew")))


# ---- 8. NaN ------------------------------------------------------------------------------------------------------------------------------------
def test_a_nan_prediction_stays_nan_and_lifts_the_limit_for_two_rows():
    from soccerdiffusion_amd import ops

    B, T, J = 2, 10, 22
    g = torch.Generator().manual_seed(11)
    eps, x = torch.randn(B, T, J, generator=g), torch.randn(B, T, J, generator=g) * 2
    eps[1, 3, 21] = NAN
    coef4 = (0.8, 0.6, 1.0, 0.0)
    hist = torch.empty(B, T, J).cuda()
    out = ops.accel_step(eps.cuda(), x.cuda(), coef4, 0.125, limits=1.0, hist=hist).cpu()
    nan = torch.isnan(out)
    assert bool(nan[1, 3, 21]) and int(nan.sum()) == 1
    x0 = torch.empty(B, T, J).cuda()
    ops.accel_step(eps.cuda(), x.cuda(), coef4, INF, hist=x0)
    x0 = x0.cpu()
    # rows 4 and 5 have the NaN among their two predecessors: limited by the box alone; row 6 .. are limited again (P3 on the whole sample)
    assert float(out[1, 4, 21]) == float(x0[1, 4, 21].clamp(-1, 1)) and float(out[1, 5, 21]) == float(x0[1, 5, 21].clamp(-1, 1))
    want, _ = accel_ref.scan(x0, torch.full((J,), 0.125), None, torch.full((J,), INF), None, torch.full((J,), -1.0), torch.full((J,), 1.0))
    keep = ~torch.isnan(want)
    assert torch.equal(torch.isnan(want), nan) and _bits(out[keep], want[keep])
    # ... and inside the step kernels' routes: a NaN element of x_T has a NaN x0 at every step
    for shape in ((256, 10, 10, 20, 1, 2), (128, 10, 40, 22, 1, 2)):
        d, T, Mc, J, L, B = shape
        _, packed, toks, coef, w, _, x_T, _, ctx = _setup(shape, seed=8)
        x_T = x_T.clone()
        x_T[1, 4, 5] = NAN
        out = ops.ddim_sample(packed, ctx.cuda(), toks, coef, x_T.cuda(), multistep=w, limits=1.0, slew=0.5, accel=0.25).cpu()
        assert bool(torch.isnan(out[1, 4, 5])) and torch.isfinite(out[0]).all()
        free = torch.ones(1, T, J, dtype=torch.bool)
        assert accel_ref.check_properties(out[:1], torch.full((J,), 0.25), None, torch.full((J,), 0.5), None, torch.full((J,), -1.0), torch.full((J,), 1.0),
                                          free) == (True, True, True)


# ---- 8b. a sample that ran away stays inside the step kernels' range -------------------------------------------------------------------------------
BIG = [("TRAJ_TUNED", (256, 10, 10, 20, 1, 2)), ("TRAJ_TUNED", (256, 100, 10, 20, 1, 2)), ("TRAJ_TUNED", (256, 10, 10, 7, 1, 2)),
       ("TRAJ_TUNED_WIDE", (256, 10, 50, 20, 2, 2)), ("TRAJ_GENERIC", (128, 10, 40, 22, 1, 2)), ("TRAJ_GENERIC", (512, 17, 70, 20, 1, 2))]


@pytest.mark.parametrize("route,shape", BIG, ids=[f"{c[0]}-{'x'.join(map(str, c[1]))}" for c in BIG])
def test_the_acceleration_twins_embed_rows_beyond_the_fp16_range(route, shape):
    """Without a box or a slew limit the scan can run away (max |x| = 1.44e6 after one step of the T = 100 case above), and the step
    kernels split x into fp16 parts as it stands: the acceleration twins scale every row (token) of x by a power of two at the embedding
    (x_token_scale, sd_common.h) once its max |x| reaches 2^15, and take the scale back after the product.  Rows of magnitude 1, 3e4, 7e4
    and 2e6 side by side in one trajectory: eps against the oracle denoiser at the same x within the project's bar.  (In range the
    scale is 1 and the embedding is the slew twins' bit for bit: test_infinite_accel_is_the_slew_call_bitwise.)"""
    from soccerdiffusion_amd import _lib, ops

    d, T, Mc, J, L, B = shape
    assert _lib.sampler_route(d, 4, T, Mc, J, L, B, 3) == route
    sd, packed, toks, coef, w, acp, x_T, known, ctx = _setup(shape, seed=9)
    scale = torch.tensor([1.0, 3e4, 7e4, 2e6])[torch.arange(T) % 4].view(1, T, 1)
    x_big = (x_T * scale).contiguous()
    x_big[0, 0, 0] = 4e6                                    # one large element in a row of small ones
    ts = ddim_ref.timesteps(N_STEPS).tolist()
    status = torch.ones(1, dtype=torch.int32, device="cuda")
    _, eps = ops.ddim_sample(packed, ctx.cuda(), toks, coef, x_big.cuda(), eps_trace=True, limits=1.0, accel=0.5, status=status)
    want = ref.forward_with_context(sd, [ctx], x_big, torch.full((B,), ts[0], dtype=torch.int64))
    err = rel_err(eps[0].cpu(), want)
    print(f"{route} {shape}: eps at rows of magnitude 1 .. 4e6 against the oracle {err:.3e}")
    assert err < TOL and int(status.item()) == 0, (err, int(status.item()))


# ---- 9. the one-step decoder ------------------------------------------------------------------------------------------------------------------
DIRECT = [("TRAJ_TUNED", (256, 10, 10, 20, 2, 3)), ("TRAJ_TUNED", (256, 33, 10, 20, 1, 2)), ("TRAJ_GENERIC", (128, 10, 311, 22, 2, 3))]


@pytest.mark.parametrize("route,shape", DIRECT, ids=[f"{c[0]}-T{c[1][1]}" for c in DIRECT])
def test_direct_sample_with_accel_is_the_projection_of_its_own_raw(route, shape):
    from soccerdiffusion_amd import _lib, ops

    d, T, Mc, J, L, B = shape
    assert _lib.sampler_route(d, 4, T, Mc, J, L, B, 3) == route
    sd, packed, toks, coef, w, acp, x_T, known, ctx = _setup(shape, seed=4)
    token = toks[-1:].contiguous()
    a, start2 = _accel(shape)
    v, start = _slew(shape)
    lo, hi = _limits(J)
    mask = _mask(B, T, J, 5)
    for masked in (False, True):
        hold = (known.cuda(), ops.hold_mask(mask, B, T, J, "cuda")) if masked else None
        status = torch.ones(1, dtype=torch.int32, device="cuda")
        out, raw = ops.direct_sample(packed, ctx.cuda(), token, x_T.cuda(), hold=hold, limits=(lo, hi), slew=(v, start), accel=(a, start2), raw=True,
                                     status=status)
        plain, plain_raw = ops.direct_sample(packed, ctx.cuda(), token, x_T.cuda(), raw=True)
        assert _bits(raw, plain_raw) and _bits(raw, plain) and int(status.item()) == 0          # the first launch is the plain direct launch
        want, side = accel_ref.scan(raw.cpu(), a, start2, v, start, lo, hi, known if masked else None, mask if masked else None)
        assert _bits(out.cpu(), want) and bool((side != 0).any())
        assert _bits(out, ops.direct_project(raw, hold=hold, limits=(lo, hi), slew=(v, start), accel=(a, start2)))
        free = ~mask if masked else torch.ones_like(mask)
        assert accel_ref.check_properties(out.cpu(), a, start2, v, start, lo, hi, free) == (True, True, True)
        # infinite a without start2 is the slew projection; without slew either, the box alone
        assert _bits(ops.direct_project(raw, hold=hold, limits=(lo, hi), slew=(v, start), accel=INF),
                     ops.direct_project(raw, hold=hold, limits=(lo, hi), slew=(v, start)))
        assert _bits(ops.direct_project(raw, hold=hold, limits=(lo, hi), accel=INF), ops.direct_project(raw, hold=hold, limits=(lo, hi)))


# ---- 10. ops.max_accel ---------------------------------------------------------------------------------------------------------------------------
def test_max_accel_equals_its_numpy_restatement_bitwise():
    from soccerdiffusion_amd import ops

    g = torch.Generator().manual_seed(12)
    for N, T, J in ((5, 10, 20), (3, 100, 7), (300, 3, 32), (2, 2, 4), (2, 1, 4)):
        x = torch.randn(N, T, J, generator=g)
        mean, std = torch.rand(J, generator=g) * 6, torch.rand(J, generator=g) + 0.1
        got = ops.max_accel(x.cuda(), mean.cuda(), std.cuda())
        assert torch.equal(got, ops.max_accel(x.cuda(), mean.cuda(), std.cuda()))       # two runs agree bit for bit
        r = (x.numpy() * std.numpy()).astype(np.float32) + mean.numpy()
        if T >= 3:
            second = ((r[:, 2:] - r[:, 1:-1]).astype(np.float32) - (r[:, 1:-1] - r[:, :-2]).astype(np.float32)).astype(np.float32)
            want = np.abs(second).max(1)
        else:
            want = np.zeros((N, J), dtype=np.float32)
        assert got.dtype == torch.float32 and np.array_equal(got.cpu().numpy().view(np.int32), want.view(np.int32)), (N, T, J)


if __name__ == "__main__":   # the child of the family test: the same run in the family its environment selects -> argv[1]
    torch.save(_family_run(), sys.argv[1])
    sys.exit(0)
