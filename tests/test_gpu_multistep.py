"""The second-order multistep solver on the GPU (sd_ddim_sample_multistep: the multistep instantiations of the trajectory step kernels,
ddim_multistep_kernel behind the row-panel and chain routes and in the loop form) against the CPU reference tests/multistep_ref.py, after
EVERY denoising step, on every route ``sampler_plan`` can return; the history buffer where the weight is zero; zero weights against the
DDIM call; several draws per context; the captured graph; ``MultistepScheduler`` in the reference's loop form; the policy session with
carried rows; and ``cli evaluate --solver multistep``."""

import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import hold_ref
import multistep_ref
from conftest import REPO, rel_err
from oracle import ddim_ref
from oracle import denoiser_ref as ref

pytestmark = pytest.mark.gpu
TOL = 1e-4          # the project's parity bar: tests/test_gpu_hold.py
FAMILY_TOL = 2e-5   # two instantiations on the same inputs: tests/test_gpu_hold.py
N_STEPS = 5         # w = (0, w1, w2, w3, 0): three steps carry a history term


def _random(p, seed):
    def make(B, T, J):
        m = torch.rand(B, T, J, generator=torch.Generator().manual_seed(seed)) < p
        m[0, 0] = True             # with a whole row, an empty row and a single element in it
        m[0, 1] = False
        m[0, 1, J - 1] = True
        return m
    return make


def _joint_31(B, T, J):
    m = torch.zeros(B, T, J, dtype=torch.bool)
    m[:, :, 31] = True
    m[1, :5, 0] = True
    return m


CASES = [
    # route, (d, T, Mc, J, L, B), mask or None, max_mode
    ("TRAJ_TUNED", (256, 10, 10, 20, 2, 3), None, 3),             # one tile
    ("TRAJ_TUNED", (256, 20, 10, 20, 1, 3), None, 3),             # rows 15 | 16 across two tiles
    ("TRAJ_TUNED", (256, 100, 10, 20, 1, 2), None, 3),            # the ragged seventh tile
    ("TRAJ_TUNED", (256, 10, 10, 7, 1, 2), None, 3),              # J = 7: the scalar path
    ("TRAJ_TUNED_WIDE", (256, 10, 50, 20, 2, 2), _random(0.35, 1), 3),
    ("TRAJ_GENERIC", (128, 10, 311, 22, 2, 3), None, 3),
    ("TRAJ_GENERIC", (128, 10, 40, 32, 1, 2), _joint_31, 3),      # bit 31
    # no mask, no J <= 32 limit of the call: the generic family's own limit is 32 joints (its embedding pads the joints to one 32-wide
    # k-step), so this is its largest; J = 33 runs the unfused chains, below
    ("TRAJ_GENERIC", (128, 10, 40, 32, 1, 2), None, 3),
    ("TRAJ_GENERIC", (512, 17, 70, 20, 1, 2), None, 3),
    ("CHAINS_F32", (64, 10, 5, 20, 1, 2), None, 3),
    ("FUSED_FOLD_F16", (256, 100, 10, 20, 1, 2), None, 2),
    ("FUSED_FOLD", (256, 100, 10, 20, 1, 2), None, 1),
    ("FUSED", (256, 100, 10, 20, 1, 2), None, 0),
    (None, (128, 10, 40, 33, 1, 2), None, 3),                     # J = 33 without a mask: whatever route the plan gives it, not a trajectory one
]


def _setup(shape, seed=0, n_ctx=None):
    """The packed synthetic denoiser of a shape with inputs on the host: (sd, packed, toks, coef, w, acp, x_T, known, ctx)."""
    from soccerdiffusion_amd import ops

    d, T, Mc, J, L, B = shape
    sd = ref.synthetic_state_dict(d, J, L, seed=23 + T + d)
    g = torch.Generator().manual_seed(T * 5 + Mc + d + J + seed)
    x_T, known = torch.randn(B, T, J, generator=g), torch.randn(B, T, J, generator=g)
    ctx = torch.randn(B if n_ctx is None else n_ctx, Mc, d, generator=g)
    acp = ddim_ref.alphas_cumprod()
    ts = ddim_ref.timesteps(N_STEPS).tolist()
    packed = ops.pack_denoiser(sd, "cuda", max_len=T)
    toks = ops.step_token(torch.tensor(ts).cuda(), ops.step_frequencies(d).cuda(), sd["step_encoding.token"].cuda()).reshape(N_STEPS, d)
    coef = ops.ddim_coefficients(ts, acp, N_STEPS)
    w = ops.multistep_weights(ts, acp, N_STEPS)
    assert w[0] == 0 and w[-1] == 0 and (w[1:-1] != 0).all()
    return sd, packed, toks, coef, w, acp, x_T, known, ctx


def _id(c):
    return f"{c[0]}-{'x'.join(map(str, c[1]))}-{'mask' if c[2] else 'nomask'}-m{c[3]}"


# ---- 1. every step against the reference -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route,shape,make_mask,max_mode", CASES, ids=[_id(c) for c in CASES])
def test_multistep_rollout_every_step(route, shape, make_mask, max_mode):
    from soccerdiffusion_amd import _lib, ops

    d, T, Mc, J, L, B = shape
    got_route = _lib.sampler_route(d, 4, T, Mc, J, L, B, max_mode)
    if route is None:
        assert not got_route.startswith("TRAJ"), got_route
    else:
        assert got_route == route
    sd, packed, toks, coef, w, acp, x_T, known, ctx = _setup(shape)
    mask = make_mask(B, T, J) if make_mask else None
    want, want_held, want_eps = multistep_ref.sample(lambda x, t: ref.forward_with_context(sd, [ctx], x, torch.full((B,), t, dtype=torch.int64)),
                                                     x_T, known if mask is not None else None, mask, N_STEPS, [float(v) for v in w], acp)
    status = torch.ones(1, dtype=torch.int32, device="cuda")
    x_dev, known_dev = x_T.cuda(), known.cuda()
    hold = None if mask is None else (known_dev, ops.hold_mask(mask, B, T, J, "cuda"))
    xm, trm, epm = ops.ddim_sample(packed, ctx.cuda(), toks, coef, x_dev, trace=True, eps_trace=True, max_mode=max_mode, status=status, hold=hold,
                                   multistep=w)
    assert torch.equal(x_dev.cpu(), x_T) and torch.equal(known_dev.cpu(), known)   # inputs are only read
    trm, epm = trm.cpu(), epm.cpu()
    free = torch.ones(B, T, J, dtype=torch.bool) if mask is None else ~mask
    for i in range(N_STEPS):
        e_x = rel_err(torch.where(free, trm[i], torch.zeros(())), torch.where(free, want[i], torch.zeros(())))
        e_eps = rel_err(epm[i], want_eps[i])
        line = f"{got_route} {shape} step {i} (w = {float(w[i]):+.4f}): free elements {e_x:.3e}, eps {e_eps:.3e}"
        if mask is not None:
            # held elements, elementwise: two evaluations of c2 K + c3 N with three roundings each, with or without contraction
            c2, c3 = float(coef[i, 2]), float(coef[i, 3])
            bound = 2.0 ** -21 * ((c2 * known.double()).abs() + (c3 * x_T.double()).abs())
            excess = ((trm[i].double() - want_held[i].double()).abs() - bound)[mask]
            line += f", held elements worst |diff| - bound {float(excess.max()):.3e}"
        print(line)
        assert e_x < TOL and e_eps < TOL, (i, e_x, e_eps)
        if mask is not None:
            assert (excess <= 0).all(), (i, float(excess.max()))
    if mask is not None:
        assert torch.equal(trm[-1][mask].view(torch.int32), known[mask].view(torch.int32))      # the last step leaves known itself, bit for bit
    assert torch.equal(xm.cpu(), trm[-1])
    assert int(status.item()) == 0 and torch.isfinite(xm).all()
    # the call without the traces is the same call
    assert torch.equal(ops.ddim_sample(packed, ctx.cuda(), toks, coef, x_dev, max_mode=max_mode, hold=hold, multistep=w), xm)


# ---- 2. the history is never read where w == 0 -------------------------------------------------------------------------------------------
ROUTES = [("TRAJ_TUNED", (256, 20, 10, 20, 1, 3), 3), ("TRAJ_TUNED", (256, 10, 10, 7, 1, 2), 3), ("TRAJ_TUNED_WIDE", (256, 10, 50, 20, 2, 2), 3),
          ("TRAJ_GENERIC", (128, 10, 311, 22, 2, 3), 3), ("CHAINS_F32", (64, 10, 5, 20, 1, 2), 3), ("FUSED_FOLD_F16", (256, 100, 10, 20, 1, 2), 2)]


@pytest.mark.parametrize("route,shape,max_mode", ROUTES, ids=[f"{c[0]}-J{c[1][3]}" for c in ROUTES])
def test_a_nan_history_changes_nothing(route, shape, max_mode):
    from soccerdiffusion_amd import _lib, ops

    d, T, Mc, J, L, B = shape
    assert _lib.sampler_route(d, 4, T, Mc, J, L, B, max_mode) == route
    _, packed, toks, coef, w, _, x_T, _, ctx = _setup(shape, seed=4)
    ws = ops.workspace(_lib.load().sd_workspace_floats(B, T, Mc, d, L, N_STEPS), "cuda")
    outs = []
    for fill in (0.0, float("nan")):
        x, hist = x_T.cuda(), torch.full((B, T, J), fill, device="cuda")
        ops._ddim_sample_native(packed, ctx.cuda(), toks, coef, x, None, None, ws, None, max_mode, None, 1, None, (w, hist))
        assert torch.isfinite(x).all() and torch.isfinite(hist).all()      # every step leaves its x0 there, the last one included
        outs.append((x, hist))
    assert torch.equal(outs[0][0].view(torch.int32), outs[1][0].view(torch.int32))
    assert torch.equal(outs[0][1].view(torch.int32), outs[1][1].view(torch.int32))
    # all weights zero: no step reads it
    x, hist = x_T.cuda(), torch.full((B, T, J), float("nan"), device="cuda")
    ops._ddim_sample_native(packed, ctx.cuda(), toks, coef, x, None, None, ws, None, max_mode, None, 1, None, (np.zeros(N_STEPS, dtype=np.float32), hist))
    assert torch.isfinite(x).all() and not torch.equal(x, outs[0][0])


# ---- 3. zero weights are the DDIM call ------------------------------------------------------------------------------------------------------
ZERO = [("TRAJ_TUNED", (256, 20, 10, 20, 1, 3)), ("TRAJ_TUNED_WIDE", (256, 10, 50, 20, 2, 2)), ("TRAJ_GENERIC", (128, 10, 311, 22, 2, 3))]


@pytest.mark.parametrize("route,shape", ZERO, ids=[c[0] for c in ZERO])
def test_zero_weights_are_the_ddim_call(route, shape):
    """Within FAMILY_TOL after every step, the noise prediction of step 0 bit for bit.  Whether the WHOLE output is bitwise equal is printed,
    not asserted (DESIGN.md records what an MI355X gave)."""
    from soccerdiffusion_amd import _lib, ops

    d, T, Mc, J, L, B = shape
    assert _lib.sampler_route(d, 4, T, Mc, J, L, B, 3) == route
    _, packed, toks, coef, _, _, x_T, _, ctx = _setup(shape, seed=1)
    zero = np.zeros(N_STEPS, dtype=np.float32)
    xm, trm, epm = ops.ddim_sample(packed, ctx.cuda(), toks, coef, x_T.cuda(), trace=True, eps_trace=True, multistep=zero)
    xd, trd, epd = ops.ddim_sample(packed, ctx.cuda(), toks, coef, x_T.cuda(), trace=True, eps_trace=True)
    for i in range(N_STEPS):
        err = rel_err(trm[i], trd[i])
        print(f"{route} {shape} step {i}: zero weights against DDIM {err:.3e}, bitwise equal: {torch.equal(trm[i], trd[i])}")
        assert err < FAMILY_TOL, (i, err)
    assert torch.equal(epm[0].view(torch.int32), epd[0].view(torch.int32))
    print(f"{route} {shape}: whole output of the zero-weight multistep call bitwise equal to the DDIM call: {torch.equal(xm, xd)}")


# ---- 4. draws ----------------------------------------------------------------------------------------------------------------------------
DRAWS = [("TRAJ_TUNED", (256, 10, 10, 20, 1, 6)), ("TRAJ_GENERIC", (128, 10, 40, 22, 1, 6))]


@pytest.mark.parametrize("route,shape", DRAWS, ids=[c[0] for c in DRAWS])
def test_draws_equal_the_repeated_context_bitwise(route, shape):
    from soccerdiffusion_amd import _lib, ops

    d, T, Mc, J, L, B = shape
    G = 3
    assert _lib.sampler_route_draws(d, 4, T, Mc, J, L, B, G, 3) == route
    _, packed, toks, coef, w, _, x_T, known, ctx = _setup(shape, seed=2, n_ctx=B // G)
    for hold in (None, (known.cuda(), ops.hold_mask(_random(0.35, 6)(B, T, J), B, T, J, "cuda"))):
        shared, trs = ops.ddim_sample(packed, ctx.cuda(), toks, coef, x_T.cuda(), trace=True, hold=hold, draws=G, multistep=w)
        repeated, trr = ops.ddim_sample(packed, ctx.cuda().repeat_interleave(G, 0).contiguous(), toks, coef, x_T.cuda(), trace=True, hold=hold,
                                        multistep=w)
        assert torch.equal(trs, trr) and torch.equal(shared, repeated) and torch.isfinite(shared).all()
    assert not torch.equal(shared, ops.ddim_sample(packed, ctx.cuda(), toks, coef, x_T.cuda(), hold=hold, draws=G))   # (it is not the DDIM rollout)


# ---- the pin is a mask of leading rows ---------------------------------------------------------------------------------------------------------
def test_a_pin_is_folded_into_the_mask():
    from soccerdiffusion_amd import ops

    shape = (256, 20, 10, 20, 1, 3)
    d, T, Mc, J, L, B = shape
    _, packed, toks, coef, w, _, x_T, known, ctx = _setup(shape, seed=5)
    rows = [16, 17, 0]
    x_T, known, ctx = x_T.cuda(), known.cuda(), ctx.cuda()
    pinned = ops.ddim_sample(packed, ctx, toks, coef, x_T, pin=(known, rows), multistep=w)
    words = ops.hold_mask(torch.zeros(J, dtype=torch.bool), B, T, J, "cuda", rows=rows)
    assert torch.equal(pinned, ops.ddim_sample(packed, ctx, toks, coef, x_T, hold=(known, words), multistep=w))
    mask = hold_ref.rows_mask(torch.tensor(rows), B, T, J).cuda()
    assert torch.equal(pinned[mask].view(torch.int32), known[mask].view(torch.int32))
    assert torch.equal(ops.ddim_sample_guarded(packed, ctx, toks, coef, x_T, pin=(known, rows), multistep=w), pinned)
    m4 = ops.ddim_sample(packed, ctx, toks, coef, x_T, max_mode=4, status=torch.zeros(1, dtype=torch.int32, device="cuda"), multistep=w)
    assert torch.equal(m4, ops.ddim_sample(packed, ctx, toks, coef, x_T, max_mode=3, multistep=w))      # max_mode 4 reads as 3


# ---- 5. the captured graph -----------------------------------------------------------------------------------------------------------------
def test_graphed_sampler_carries_no_history_over():
    from test_gpu_loop_form import _model

    from soccerdiffusion_amd import ops

    shape = (256, 10, 10, 20, 2, 3)
    d, T, Mc, J, L, B = shape
    _, packed, toks, coef, w, _, x_T, known, ctx = _setup(shape, seed=6)
    gs = ops.GraphedSampler(packed, B, T, Mc, toks, coef, multistep=w)
    g = torch.Generator().manual_seed(8)
    for _ in range(2):
        x = torch.randn(B, T, J, generator=g).cuda()
        assert torch.equal(gs(ctx.cuda(), x), ops.ddim_sample(packed, ctx.cuda(), toks, coef, x, multistep=w))
    # pin=True on a multistep graph: the pin travels as a mask
    gp = ops.GraphedSampler(packed, B, T, Mc, toks, coef, pin=True, multistep=w)
    for rows in ([3, 0, 10], 2):
        x = torch.randn(B, T, J, generator=g).cuda()
        assert torch.equal(gp(ctx.cuda(), x, pin=(known.cuda(), rows)), ops.ddim_sample(packed, ctx.cuda(), toks, coef, x, pin=(known.cuda(), rows), multistep=w))
    # model.sample(solver="multistep"): eager equals graphed, and is not the DDIM sample
    m, _ = _model(d, J, L, T)
    c = [torch.randn(B, Mc, d, generator=g).cuda()]
    for _ in range(2):
        x = torch.randn(B, T, J, generator=g).cuda()
        eager = m.sample(c, x, N_STEPS, solver="multistep")
        assert torch.equal(eager, m.sample(c, x, N_STEPS, solver="multistep", use_graph=True))
        assert not torch.equal(eager, m.sample(c, x, N_STEPS)) and torch.isfinite(eager).all()
    x2, trace = m.sample(c, x, N_STEPS, solver="multistep", return_trace=True)
    assert torch.equal(x2, eager) and torch.equal(trace[-1], eager)
    assert torch.equal(m.sample(c, x, N_STEPS, use_graph=True), m.sample(c, x, N_STEPS))      # the default solver is another graph


# ---- 6. the loop form -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,T,Mc,J,L,B", [(256, 10, 10, 20, 2, 3), (128, 10, 40, 22, 1, 2)], ids=["TRAJ_TUNED", "TRAJ_GENERIC"])
def test_multistep_scheduler_in_the_loop_form(d, T, Mc, J, L, B):
    from test_gpu_loop_form import _model

    from soccerdiffusion_amd import _lib
    from soccerdiffusion_amd.scheduler import MultistepScheduler

    assert _lib.sampler_route(d, 4, T, Mc, J, L, B, 3) == ("TRAJ_TUNED" if d == 256 else "TRAJ_GENERIC")
    m, _ = _model(d, J, L, T)
    g = torch.Generator().manual_seed(d + T)
    x_T, ctx = torch.randn(B, T, J, generator=g).cuda(), [torch.randn(B, Mc, d, generator=g).cuda()]
    native, trace = m.sample(ctx, x_T, N_STEPS, solver="multistep", return_trace=True)
    sched = MultistepScheduler(beta_schedule="squaredcos_cap_v2", clip_sample=False)
    sched.config["num_train_timesteps"] = 1000
    for rollout in range(2):      # set_timesteps clears the history: the second rollout is the first
        sched.set_timesteps(N_STEPS)
        traj = x_T
        with torch.no_grad():
            for i, t in enumerate(sched.timesteps):
                eps = m.forward_with_context(ctx, traj, torch.full((B,), int(t), device="cuda"))
                traj = sched.step(eps, t, traj).prev_sample
                err = rel_err(traj, trace[i])
                print(f"d = {d} rollout {rollout} step {i}: loop form against the native call {err:.3e}, bitwise equal: {torch.equal(traj, trace[i])}")
                assert err < FAMILY_TOL, (rollout, i, err)
    assert not torch.equal(native, m.sample(ctx, x_T, N_STEPS))


# ---- 7. the policy session ----------------------------------------------------------------------------------------------------------------------
def test_policy_session_multistep_with_carry():
    from test_gpu_reference_configs import BASE, CONFIGS
    from test_gpu_session import _same_bits, _synthetic_model

    from soccerdiffusion_amd.session import PolicySession

    params = {**BASE, **CONFIGS["default"]}
    model = _synthetic_model(params)[0]
    B, T, J, CARRY, ADVANCE = 2, model.trajectory_prediction_length, model.num_joints, 4, 5
    kw = dict(num_inference_steps=N_STEPS, batch=B, hyperparams=params, seed=9, carry=CARRY, advance=ADVANCE, solver="multistep")
    eager, graphed = PolicySession(model, **kw), PolicySession(model, use_graph=True, **kw)
    ddim = PolicySession(model, **{**kw, "solver": "ddim"})
    g = torch.Generator().manual_seed(44)
    prev = None
    for tick in range(2):
        q, r = (torch.rand(B, ADVANCE, J, generator=g) - 0.5) * 6, torch.randn(B, ADVANCE, 4, generator=g)
        for s in (eager, graphed, ddim):
            s.push_joint_state(q.cuda())
            s.push_rotation(r.cuda())
        x_T = torch.randn(B, T, J, generator=g).cuda()
        out = [s.step(x_T) for s in (eager, graphed)]
        assert _same_bits(out[0], out[1]) and torch.isfinite(out[0]).all(), tick
        if tick == 0:
            assert not _same_bits(out[0], ddim.step(x_T))
        else:
            assert _same_bits(out[0][:, :CARRY], prev[:, ADVANCE:ADVANCE + CARRY])      # the seam: the committed rows, bit for bit
            assert not _same_bits(out[0][:, CARRY], prev[:, ADVANCE + CARRY])
        prev = out[0]
    assert graphed._graph is not None and eager._graph is None


# ---- 8. the command line ------------------------------------------------------------------------------------------------------------------------
def test_cli_evaluate_with_the_multistep_solver(tmp_path):
    from test_gpu_cli import CFG

    from soccerdiffusion_amd import cli

    params = dict(CFG, trajectory_prediction_length=10)
    torch.manual_seed(3)
    model = cli.build_model(params)      # an untrained checkpoint: the command line is under test, not the policy
    ckpt = tmp_path / "model.pth"
    torch.save({"hyperparams": params, "model_state_dict": model.state_dict()}, ckpt)
    r = subprocess.run([sys.executable, "-m", "soccerdiffusion_amd.cli", "evaluate", str(ckpt), "--solver", "multistep", "--steps", "5", "--synthetic", "8",
                        "--all"], cwd=REPO, env=dict(os.environ, PYTHONPATH=REPO), capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    rep = json.loads(r.stdout.strip().splitlines()[-1])
    assert rep["solver"] == "multistep" and rep["steps"] == 5 and rep["n_windows"] == 8
    for k in ("val_loss", "rmse_first_draw", "rmse_medoid", "rmse_best_of_G", "spread"):
        assert math.isfinite(rep[k]), k
    assert all(math.isfinite(v) for v in rep["rmse_by_row"] + rep["rmse_by_joint"])
