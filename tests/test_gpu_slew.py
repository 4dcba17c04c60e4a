"""Per-joint slew limits on the GPU (sd_ddim_sample_slew: the slew instantiations of the trajectory step kernels, ddim_slew_step_kernel
behind the row-panel and chain routes and in the loop form) against the CPU reference tests/slew_ref.py, after EVERY denoising step, on every
route ``sampler_plan`` can return; the last step bitwise inside the box and the slew limits; infinite v against the limits call; held
elements; several draws per context; the captured graph with ``set_slew``; the two trajectory families against each other; the
schedulers' ``slew`` in the reference's loop form; the elementwise kernel bit for bit; and a NaN prediction."""

import os
import subprocess
import sys
import tempfile

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":   # the child of the family test: this file's directory is on the path, the repository is not
    sys.path.insert(0, REPO)

import slew_ref
from conftest import rel_err
from oracle import ddim_ref
from oracle import denoiser_ref as ref
from test_gpu_limits import N_STEPS, _host, _limits, _mask, _setup

TOL = 1e-4          # the project's parity bar (rel_err of conftest): the map is non-expansive (P4), so the limits tests' bar carries over
FAMILY_TOL = 2e-5   # two instantiations on the same inputs: tests/test_gpu_limits.py
INF = float("inf")
NAN = float("nan")

CASES = [
    # route, (d, T, Mc, J, L, B), max_mode
    ("TRAJ_TUNED", (256, 10, 10, 20, 2, 3), 3),
    ("TRAJ_TUNED", (256, 20, 10, 20, 1, 3), 3),             # rows 15 | 16 belong to different waves: the scan crosses the tile boundary
    ("TRAJ_TUNED", (256, 100, 10, 20, 1, 2), 3),            # the ragged seventh tile (row panels below: six blocks of the scan and four rows)
    ("TRAJ_TUNED", (256, 10, 10, 7, 1, 2), 3),              # ragged joints: the scalar path
    ("TRAJ_TUNED_WIDE", (256, 10, 50, 20, 2, 2), 3),
    ("TRAJ_GENERIC", (128, 10, 311, 22, 2, 3), 3),
    ("TRAJ_GENERIC", (128, 10, 40, 32, 1, 2), 3),           # joint 31
    ("TRAJ_GENERIC", (512, 17, 70, 20, 1, 2), 3),
    ("CHAINS_F32", (64, 10, 5, 20, 1, 2), 3),
    ("FUSED_FOLD_F16", (256, 100, 10, 20, 1, 2), 2),
    ("FUSED_FOLD", (256, 100, 10, 20, 1, 2), 1),
    ("FUSED", (256, 100, 10, 20, 1, 2), 0),
]
FAMILY_SHAPE = (256, 10, 10, 20, 2, 3)
# (multistep, mask, box, reproject): DDIM / multistep x mask / none x box / infinite box, reproject on in one combination
COMBOS = [(ms, masked, box, ms and masked and box) for ms in (False, True) for masked in (False, True) for box in (False, True)]


def _slew(shape, seed=0):
    """v = 0.5 on every joint but v[1] = inf and v[2] = 0.25; start = 0.5 randn(B, J) with start[:, 3] = NaN."""
    d, T, Mc, J, L, B = shape
    v = torch.full((J,), 0.5)
    v[1], v[2] = INF, 0.25
    start = 0.5 * torch.randn(B, J, generator=torch.Generator().manual_seed(100 + seed + J + B))
    start[:, 3] = NAN
    return v, start


def _box(J, box):
    return _limits(J) if box else (torch.full((J,), -INF), torch.full((J,), INF))


def reference(shape, w, masked, box, reproject, host=None):
    """slew_ref.sample in fp32 on the oracle denoiser for one combination, and the check that the case tests something: at every step
    between 5 % and 95 % of the free elements are slewed, and both sides occur."""
    d, T, Mc, J, L, B = shape
    sd, ts, acp, x_T, known, ctx = host or _host(shape)
    v, start = _slew(shape)
    lo, hi = _box(J, box)
    mask = _mask(B, T, J) if masked else None
    out = slew_ref.sample(lambda x, t: ref.forward_with_context(sd, [ctx], x, torch.full((B,), t, dtype=torch.int64)), x_T,
                          known if masked else None, mask, N_STEPS, None if w is None else [float(u) for u in w], v, start, lo, hi, reproject, acp)
    free = torch.ones(B, T, J, dtype=torch.bool) if mask is None else ~mask
    fractions = []
    for i, side in enumerate(out[3]):
        fractions.append(float((side != 0)[free].float().mean()))
        assert 0.05 <= fractions[-1] <= 0.95, (shape, i, fractions)
        assert bool((side[free] < 0).any()) and bool((side[free] > 0).any()), (shape, i)
    return out, mask, free, fractions


pytestmark = pytest.mark.gpu


# ---- 1. every step against the reference --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route,shape,max_mode", CASES, ids=[f"{c[0]}-{'x'.join(map(str, c[1]))}-m{c[2]}" for c in CASES])
def test_slewed_rollout_every_step(route, shape, max_mode):
    from soccerdiffusion_amd import _lib, ops

    d, T, Mc, J, L, B = shape
    assert _lib.sampler_route(d, 4, T, Mc, J, L, B, max_mode) == route
    sd, packed, toks, coef, w, acp, x_T, known, ctx = _setup(shape)
    host = (sd, ddim_ref.timesteps(N_STEPS).tolist(), acp, x_T, known, ctx)
    v, start = _slew(shape)
    v_dev = ops.joint_slew(v, J=J, device="cuda")
    start_dev = torch.full((B, 32), NAN)
    start_dev[:, :J] = start
    start_dev = start_dev.cuda()
    before = [v_dev.clone(), start_dev.clone()]
    x_dev, known_dev, ctx_dev = x_T.cuda(), known.cuda(), ctx.cuda()
    for ms, masked, box, reproject in COMBOS:
        (want, want_held, want_eps, _, _), mask, free, fractions = reference(shape, w if ms else None, masked, box, reproject, host)
        lo, hi = _box(J, box)
        words = ops.hold_mask(mask, B, T, J, "cuda") if masked else None
        hold = (known_dev, words) if masked else None
        status = torch.ones(1, dtype=torch.int32, device="cuda")
        kw = dict(max_mode=max_mode, hold=hold, multistep=w if ms else None, limits=(lo, hi) if box else None, reproject=reproject,
                  slew=(v_dev, start_dev))
        xm, trm, epm = ops.ddim_sample(packed, ctx_dev, toks, coef, x_dev, trace=True, eps_trace=True, status=status, **kw)
        # inputs are only read
        assert torch.equal(x_dev.cpu(), x_T) and torch.equal(known_dev.cpu(), known)
        assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip((v_dev, start_dev), before))
        assert not masked or torch.equal(words, ops.hold_mask(mask, B, T, J, "cuda"))
        trm, epm = trm.cpu(), epm.cpu()
        for i in range(N_STEPS):
            e_x = rel_err(torch.where(free, trm[i], torch.zeros(())), torch.where(free, want[i], torch.zeros(())))
            e_eps = rel_err(epm[i], want_eps[i])
            print(f"{route} {shape} multistep={ms} mask={masked} box={box} reproject={reproject} step {i}: slewed {fractions[i]:.2f}, "
                  f"free elements {e_x:.3e}, eps {e_eps:.3e}")
            assert e_x < TOL and e_eps < TOL, (ms, masked, box, reproject, i, e_x, e_eps)
        final = trm[-1]
        p1, p2 = slew_ref.check_properties(final, v, start, lo, hi, free)     # bitwise: the last step returns x0c itself
        assert p1 and p2, (ms, masked, box, reproject, p1, p2)
        if masked:   # held elements keep the hold's value, bit for bit at the end
            assert torch.equal(final[mask].view(torch.int32), known[mask].view(torch.int32))
        assert torch.equal(xm.cpu(), final) and int(status.item()) == 0 and torch.isfinite(xm).all()
        # the call without the traces is the same call
        assert torch.equal(ops.ddim_sample(packed, ctx_dev, toks, coef, x_dev, **kw), xm)


# ---- 2. P3: infinite v without start is the limits call, bit for bit -------------------------------------------------------------------------
ROUTES = [("TRAJ_TUNED", (256, 20, 10, 20, 1, 3), 3), ("TRAJ_TUNED_WIDE", (256, 10, 50, 20, 2, 2), 3), ("TRAJ_GENERIC", (128, 10, 311, 22, 2, 3), 3),
          ("FUSED_FOLD_F16", (256, 100, 10, 20, 1, 2), 2)]


@pytest.mark.parametrize("route,shape,max_mode", ROUTES, ids=[c[0] for c in ROUTES])
def test_infinite_slew_is_the_limits_call_bitwise(route, shape, max_mode):
    from soccerdiffusion_amd import _lib, ops

    d, T, Mc, J, L, B = shape
    assert _lib.sampler_route(d, 4, T, Mc, J, L, B, max_mode) == route
    _, packed, toks, coef, w, _, x_T, known, ctx = _setup(shape, seed=1)
    x_dev, ctx_dev = x_T.cuda(), ctx.cuda()
    hold = (known.cuda(), ops.hold_mask(_mask(B, T, J, 3), B, T, J, "cuda"))
    lim = _limits(J)
    for h in (None, hold):
        for weights in (None, w):
            for reproject in (False, True):
                kw = dict(trace=True, eps_trace=True, max_mode=max_mode, hold=h, multistep=weights, limits=lim, reproject=reproject)
                want = ops.ddim_sample(packed, ctx_dev, toks, coef, x_dev, **kw)
                got = ops.ddim_sample(packed, ctx_dev, toks, coef, x_dev, slew=INF, **kw)
                assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(want, got)), (h is not None, weights is not None, reproject)
    # and a finite v is another rollout
    assert not torch.equal(ops.ddim_sample(packed, ctx_dev, toks, coef, x_dev, max_mode=max_mode, limits=lim, slew=0.25),
                           ops.ddim_sample(packed, ctx_dev, toks, coef, x_dev, max_mode=max_mode, limits=lim))


# ---- 3. draws -------------------------------------------------------------------------------------------------------------------------------
DRAWS = [("TRAJ_TUNED", (256, 10, 10, 20, 1, 8)), ("TRAJ_GENERIC", (128, 10, 40, 22, 1, 8))]


@pytest.mark.parametrize("route,shape", DRAWS, ids=[c[0] for c in DRAWS])
def test_draws_equal_the_repeated_context_bitwise(route, shape):
    from soccerdiffusion_amd import _lib, ops

    d, T, Mc, J, L, B = shape
    G = 8
    assert _lib.sampler_route_draws(d, 4, T, Mc, J, L, B, G, 3) == route
    _, packed, toks, coef, w, _, x_T, known, ctx = _setup(shape, seed=2, n_ctx=B // G)
    slew = _slew(shape)
    for hold in (None, (known.cuda(), ops.hold_mask(_mask(B, T, J, 6), B, T, J, "cuda"))):
        for weights in (None, w):
            shared, trs = ops.ddim_sample(packed, ctx.cuda(), toks, coef, x_T.cuda(), trace=True, hold=hold, draws=G, multistep=weights, limits=_limits(J),
                                          slew=slew)
            repeated, trr = ops.ddim_sample(packed, ctx.cuda().repeat_interleave(G, 0).contiguous(), toks, coef, x_T.cuda(), trace=True, hold=hold,
                                            multistep=weights, limits=_limits(J), slew=slew)
            assert torch.equal(trs, trr) and torch.equal(shared, repeated) and torch.isfinite(shared).all()


# ---- 4. the captured graph ------------------------------------------------------------------------------------------------------------------
def test_graphed_sampler_follows_set_slew_without_a_new_capture():
    from test_gpu_loop_form import _model

    from soccerdiffusion_amd import ops

    shape = (256, 10, 10, 20, 2, 3)
    d, T, Mc, J, L, B = shape
    _, packed, toks, coef, w, _, x_T, known, ctx = _setup(shape, seed=6)
    first, second = _slew(shape), {0: 0.125, J - 1: 0.0}
    g = torch.Generator().manual_seed(8)
    for weights in (None, w):
        gs = ops.GraphedSampler(packed, B, T, Mc, toks, coef, multistep=weights, slew=True)
        graph = gs.graph
        for slew in (first, second):
            gs.set_slew(slew)
            x = torch.randn(B, T, J, generator=g).cuda()
            eager = ops.ddim_sample(packed, ctx.cuda(), toks, coef, x, multistep=weights, slew=slew)
            assert torch.equal(gs(ctx.cuda(), x), eager) and gs.graph is graph
            v, start = ops._slew_req(slew, B, J, "cuda")
            p1, p2 = slew_ref.check_properties(eager.cpu(), v[:J].cpu(), None if start is None else start[:, :J].cpu(), *_box(J, False),
                                               torch.ones(B, T, J, dtype=torch.bool))
            assert p1 and p2
        assert bool((eager[:, 1:, J - 1] == eager[:, :-1, J - 1]).all())   # v = 0: the joint does not move between rows
    # a graph captured without slew takes none
    with pytest.raises(ValueError, match="slew=True"):
        ops.GraphedSampler(packed, B, T, Mc, toks, coef).set_slew(1.0)
    # model.sample(slew=...): eager equals graphed; one capture serves both
    m, _ = _model(d, J, L, T)
    c = [torch.randn(B, Mc, d, generator=g).cuda()]
    graphs = set()
    for slew in (first, second):
        x = torch.randn(B, T, J, generator=g).cuda()
        eager = m.sample(c, x, N_STEPS, slew=slew, solver="multistep")
        assert torch.equal(eager, m.sample(c, x, N_STEPS, slew=slew, solver="multistep", use_graph=True))
        assert not torch.equal(eager, m.sample(c, x, N_STEPS, solver="multistep")) and torch.isfinite(eager).all()
        from soccerdiffusion_amd.ml.model import model as mm
        graphs |= {id(u) for u in mm._model_cache(m, "graphs").values()}
    assert len(graphs) == 1


# ---- 5. the two trajectory families -----------------------------------------------------------------------------------------------------------
def _family_run():
    """The family shape under slew limits, both solvers with a mask and a box: the traces, in the family this process's environment selects."""
    from soccerdiffusion_amd import _lib, ops

    d, T, Mc, J, L, B = FAMILY_SHAPE
    _, packed, toks, coef, w, _, x_T, known, ctx = _setup(FAMILY_SHAPE, seed=7)
    hold = (known.cuda(), ops.hold_mask(_mask(B, T, J, 9), B, T, J, "cuda"))
    out = {"route": _lib.sampler_route(d, 4, T, Mc, J, L, B, 3)}
    for ms in (False, True):
        for reproject in (False, True):
            out[f"{int(ms)}{int(reproject)}"] = ops.ddim_sample(packed, ctx.cuda(), toks, coef, x_T.cuda(), trace=True, hold=hold, multistep=w if ms else None,
                                                                limits=_limits(J), reproject=reproject, slew=_slew(FAMILY_SHAPE))[1].cpu()
    return out


def test_tuned_and_generic_family_agree():
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


# ---- 6. the loop form ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,T,Mc,J,L,B", [(256, 10, 10, 20, 2, 3), (128, 10, 40, 22, 1, 2)], ids=["TRAJ_TUNED", "TRAJ_GENERIC"])
def test_schedulers_with_slew_in_the_loop_form_bitwise(d, T, Mc, J, L, B):
    from test_gpu_loop_form import _model

    from soccerdiffusion_amd.scheduler import DDIMScheduler, MultistepScheduler

    m, _ = _model(d, J, L, T)
    g = torch.Generator().manual_seed(d + T)
    x_T, ctx = torch.randn(B, T, J, generator=g).cuda(), [torch.randn(B, Mc, d, generator=g).cuda()]
    slew = _slew((d, T, Mc, J, L, B))
    lim = _limits(J)
    for sched, kw in ((DDIMScheduler(beta_schedule="squaredcos_cap_v2", slew=slew), dict(slew=slew)),
                      (DDIMScheduler(limits=lim, slew=slew), dict(limits=lim, slew=slew)),
                      (MultistepScheduler(limits=lim, slew=slew), dict(limits=lim, slew=slew, solver="multistep"))):
        for reproject in (False, True):
            native, trace = m.sample(ctx, x_T, N_STEPS, return_trace=True, reproject=reproject, **kw)
            sched.set_timesteps(N_STEPS)
            traj = x_T
            with torch.no_grad():
                for i, t in enumerate(sched.timesteps):
                    eps = m.forward_with_context(ctx, traj, torch.full((B,), int(t), device="cuda"))
                    traj = sched.step(eps, t, traj, use_clipped_model_output=reproject).prev_sample
                    assert torch.equal(traj.view(torch.int32), trace[i].view(torch.int32)), (type(sched).__name__, reproject, i)
            assert not torch.equal(native, m.sample(ctx, x_T, N_STEPS, solver=kw.get("solver", "ddim"), limits=kw.get("limits")))


# ---- 7. the elementwise kernel ----------------------------------------------------------------------------------------------------------------
def test_slew_step_is_the_reference_scan_bitwise():
    """ops.slew_step against slew_ref.scan on the kernel's own x0.  torch on the CPU has no fp32 fma, so x0 = fma(-c1, e, x) / c0 is taken
    from the kernel (infinite v, no box: the history then holds x0 itself); the scan after it has no fma - compares and one rounded
    y +- v - and x0c is compared bit for bit.  x = fma(c2, x0c, c3 e) + w (hist - x0c) is held to 2 ulp of its fp64 value's magnitude."""
    from soccerdiffusion_amd import ops

    g = torch.Generator().manual_seed(5)
    for B, T, J in ((3, 10, 20), (2, 100, 7), (5, 17, 32)):
        eps, x, hist0 = (torch.randn(B, T, J, generator=g) for _ in range(3))
        known = torch.randn(B, T, J, generator=g) * 2
        mask = _mask(B, T, J, 4)
        v, start = _slew((0, T, 0, J, 0, B), seed=1)
        lo, hi = _limits(J)
        coef4, w = (0.8, 0.6, 0.9, 0.43588989), 0.37
        for masked in (False, True):
            hold = (known.cuda(), ops.hold_mask(mask, B, T, J, "cuda")) if masked else None
            x0 = torch.empty(B, T, J).cuda()
            ops.slew_step(eps.cuda(), x.cuda(), coef4, INF, hist=x0)
            x0 = x0.cpu()
            want, _ = slew_ref.scan(x0, v, start, lo, hi, known if masked else None, mask if masked else None)
            hist = hist0.clone().cuda()
            out = ops.slew_step(eps.cuda(), x.cuda(), coef4, (v, start), limits=(lo, hi), hist=hist, w=w, hold=hold).cpu()
            assert torch.equal(hist.cpu().view(torch.int32), want.view(torch.int32)), (B, T, J, masked)
            c = [torch.tensor(u, dtype=torch.float32).double() for u in coef4]
            exact = c[2] * want.double() + c[3] * eps.double() + torch.tensor(w, dtype=torch.float32).double() * (hist0.double() - want.double())
            scale = (c[2] * want.double()).abs() + (c[3] * eps.double()).abs() + (hist0.double() - want.double()).abs()
            assert bool(((out.double() - exact).abs() <= 2 * 2.0 ** -23 * scale).all()), (B, T, J, masked)
            assert (want != x0).float().mean() > 0.05


# ---- 8. NaN ------------------------------------------------------------------------------------------------------------------------------------
def test_a_nan_prediction_comes_out_as_nan_and_limits_nothing_downstream():
    from soccerdiffusion_amd import ops

    B, T, J = 2, 10, 22
    g = torch.Generator().manual_seed(11)
    eps, x = torch.randn(B, T, J, generator=g), torch.randn(B, T, J, generator=g) * 2
    eps[1, 3, 21] = NAN
    coef4 = (0.8, 0.6, 1.0, 0.0)
    hist = torch.empty(B, T, J).cuda()
    out = ops.slew_step(eps.cuda(), x.cuda(), coef4, 0.125, limits=1.0, hist=hist).cpu()
    nan = torch.isnan(out)
    assert bool(nan[1, 3, 21]) and int(nan.sum()) == 1
    x0 = torch.empty(B, T, J).cuda()
    ops.slew_step(eps.cuda(), x.cuda(), coef4, INF, hist=x0)
    # row 4 follows a NaN: it is limited by the box alone, rows 5 .. follow row 4 again
    assert float(out[1, 4, 21]) == float(x0[1, 4, 21].clamp(-1, 1))
    assert bool(((out[1, 5:, 21] <= out[1, 4:-1, 21] + 0.125) & (out[1, 5:, 21] >= out[1, 4:-1, 21] - 0.125)).all())
    # ... and inside the step kernels' routes: a NaN element of x_T has a NaN x0 at every step
    for shape in ((256, 10, 10, 20, 1, 2), (128, 10, 40, 22, 1, 2)):
        d, T, Mc, J, L, B = shape
        _, packed, toks, coef, w, _, x_T, _, ctx = _setup(shape, seed=8)
        x_T = x_T.clone()
        x_T[1, 4, 5] = NAN
        out = ops.ddim_sample(packed, ctx.cuda(), toks, coef, x_T.cuda(), multistep=w, limits=1.0, slew=0.25)
        assert bool(torch.isnan(out[1, 4, 5])) and torch.isfinite(out[0]).all() and bool(((out[0] >= -1) & (out[0] <= 1)).all())
        assert bool(((out[0, 1:] <= out[0, :-1] + 0.25) & (out[0, 1:] >= out[0, :-1] - 0.25)).all())


if __name__ == "__main__":   # the child of the family test: the same run in the family its environment selects -> argv[1]
    torch.save(_family_run(), sys.argv[1])
    sys.exit(0)
