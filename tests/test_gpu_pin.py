"""Pinned leading rows of the sampler on the GPU (sd_ddim_sample_pin: the pinned instantiations of the trajectory step kernels,
ddim_pin_kernel behind the row-panel and chain routes) against the CPU reference tests/pin_ref.py, after EVERY denoising step, on every
route ``sampler_plan`` can return; and through ``End2EndDiffusionTransformer.sample(pin=...)``, eager and from a captured graph."""

import pytest
import torch

import pin_ref
from conftest import rel_err
from oracle import ddim_ref
from oracle import denoiser_ref as ref

pytestmark = pytest.mark.gpu
TOL = 1e-4          # the project's parity bar: tests/test_gpu_generic_traj.py
FAMILY_TOL = 2e-5   # two kernel families on the same inputs: tests/test_gpu_generic_traj.py:77
N_STEPS = 4

CASES = [
    # route, (d, T, Mc, J, L, B), rows, max_mode
    ("TRAJ_TUNED", (256, 10, 10, 20, 2, 3), [0, 3, 10], 3),        # none / some / all rows pinned
    ("TRAJ_TUNED", (256, 20, 10, 20, 1, 3), [16, 17, 1], 3),       # the token-tile edge, second tile on the odd waves
    ("TRAJ_TUNED", (256, 100, 10, 20, 1, 2), [97, 100], 3),        # into the ragged last tile of NTT = 7
    ("TRAJ_TUNED", (256, 10, 10, 7, 1, 2), [4, 0], 3),             # the ragged J & 3 path
    ("TRAJ_TUNED_WIDE", (256, 10, 50, 20, 2, 2), [5, 2], 3),       # sim_scratch's memory length
    ("TRAJ_GENERIC", (128, 10, 311, 22, 2, 3), [0, 3, 10], 3),     # default.yaml, J = 22
    ("TRAJ_GENERIC", (512, 17, 70, 20, 1, 2), [16, 17], 3),
    ("TRAJ_GENERIC", (128, 33, 40, 7, 1, 2), [17, 32], 3),
    ("CHAINS_F32", (64, 10, 5, 20, 1, 2), [3, 0], 3),
    ("FUSED_FOLD_F16", (256, 100, 10, 20, 1, 2), [97, 0], 2),
    ("FUSED_FOLD", (256, 100, 10, 20, 1, 2), [97, 0], 1),          # the fp32 rerun path of ops.ddim_sample_guarded
    ("FUSED", (256, 100, 10, 20, 1, 2), [97, 0], 0),
]


@pytest.mark.parametrize("route,shape,rows,max_mode", CASES, ids=[f"{c[0]}-{'x'.join(map(str, c[1]))}-m{c[3]}" for c in CASES])
def test_pinned_rollout_every_step(route, shape, rows, max_mode):
    from soccerdiffusion_amd import _lib, ops

    d, T, Mc, J, L, B = shape
    assert _lib.sampler_route(d, 4, T, Mc, J, L, B, max_mode) == route
    sd = ref.synthetic_state_dict(d, J, L, seed=23 + T + d)
    g = torch.Generator().manual_seed(T * 5 + Mc + d + J)
    x_T, known = torch.randn(B, T, J, generator=g), torch.randn(B, T, J, generator=g)
    ctx = torch.randn(B, Mc, d, generator=g)
    rows_t = torch.tensor(rows)
    acp = ddim_ref.alphas_cumprod()
    ts = ddim_ref.timesteps(N_STEPS).tolist()
    want, want_pin, want_eps = pin_ref.sample(lambda x, t: ref.forward_with_context(sd, [ctx], x, torch.full((B,), t, dtype=torch.int64)),
                                              x_T, known, rows_t, N_STEPS, acp)
    packed = ops.pack_denoiser(sd, "cuda", max_len=T)
    toks = ops.step_token(torch.tensor(ts).cuda(), ops.step_frequencies(d).cuda(), sd["step_encoding.token"].cuda()).reshape(N_STEPS, d)
    coef = ops.ddim_coefficients(ts, acp, N_STEPS)
    status = torch.ones(1, dtype=torch.int32, device="cuda")
    x_dev, known_dev = x_T.cuda(), known.cuda()
    xm, trm, epm = ops.ddim_sample(packed, ctx.cuda(), toks, coef, x_dev, trace=True, eps_trace=True, max_mode=max_mode, status=status,
                                   pin=(known_dev, rows_t))
    assert torch.equal(x_dev.cpu(), x_T) and torch.equal(known_dev.cpu(), known)      # inputs are only read
    trm, epm = trm.cpu(), epm.cpu()
    mask = pin_ref.pin_mask(rows_t, B, T).expand(B, T, J)
    free = ~mask
    for i in range(N_STEPS):
        # unpinned rows and the noise prediction of ALL rows: the parity bar
        e_x = rel_err(torch.where(free, trm[i], torch.zeros(())), torch.where(free, want[i], torch.zeros(())))
        e_eps = rel_err(epm[i], want_eps[i])
        # pinned rows, elementwise: two evaluations of c2 K + c3 N with three roundings each, with or without contraction
        c2, c3 = float(coef[i, 2]), float(coef[i, 3])
        bound = 2.0 ** -21 * ((c2 * known.double()).abs() + (c3 * x_T.double()).abs())
        excess = ((trm[i].double() - want_pin[i].double()).abs() - bound)[mask]
        print(f"{route} {shape} step {i}: free rows {e_x:.3e}, eps {e_eps:.3e}, pinned rows worst |diff| - bound {float(excess.max()):.3e}")
        assert e_x < TOL and e_eps < TOL, (i, e_x, e_eps)
        assert (excess <= 0).all(), (i, float(excess.max()))
    assert torch.equal(trm[-1][mask].view(torch.int32), known[mask].view(torch.int32))      # the last step leaves known itself, bit for bit
    assert torch.equal(xm.cpu(), trm[-1])
    assert int(status.item()) == 0 and torch.isfinite(xm).all()
    # trajectories without pinned rows: the same call without a pin
    unpinned = [b for b in range(B) if rows[b] == 0]
    if unpinned:
        plain = ops.ddim_sample(packed, ctx.cuda(), toks, coef, x_dev, max_mode=max_mode).cpu()
        err = rel_err(xm.cpu()[unpinned], plain[unpinned])
        print(f"{route} {shape}: rows = 0 trajectories against the call without a pin {err:.3e}")
        assert err < FAMILY_TOL


def test_pin_arguments_on_the_device():
    """What the call checks itself: rows outside [0, T] as an int or a host tensor, shapes, and a mode-4 cap running the mode-3 kernels."""
    from soccerdiffusion_amd import ops

    d, T, Mc, J, L, B = 256, 10, 10, 20, 1, 2
    sd = ref.synthetic_state_dict(d, J, L, seed=5)
    g = torch.Generator().manual_seed(6)
    x_T, known, ctx = torch.randn(B, T, J, generator=g).cuda(), torch.randn(B, T, J, generator=g).cuda(), torch.randn(B, Mc, d, generator=g).cuda()
    ts = ddim_ref.timesteps(N_STEPS).tolist()
    packed = ops.pack_denoiser(sd, "cuda", max_len=T)
    toks = ops.step_token(torch.tensor(ts).cuda(), ops.step_frequencies(d).cuda(), sd["step_encoding.token"].cuda()).reshape(N_STEPS, d)
    coef = ops.ddim_coefficients(ts, ddim_ref.alphas_cumprod(), N_STEPS)
    for bad in ((known, T + 1), (known, -1), (known, torch.tensor([0, 11])), (known[:, :5], 3), (known.cpu(), 3), known):
        with pytest.raises((ValueError, RuntimeError)):
            ops.ddim_sample(packed, ctx, toks, coef, x_T, pin=bad)
    rows = torch.tensor([4, 0], dtype=torch.int32).cuda()     # a device tensor is used as it is
    m3 = ops.ddim_sample(packed, ctx, toks, coef, x_T, max_mode=3, pin=(known, rows))
    m4 = ops.ddim_sample(packed, ctx, toks, coef, x_T, max_mode=4, pin=(known, rows))     # no pinned twin of mode 4: the mode-3 kernels
    assert torch.equal(m3, m4)
    inplace = x_T.clone()
    out = ops.ddim_sample(packed, ctx, toks, coef, inplace, max_mode=3, inplace=True, pin=(known, rows))     # a private copy of the noise
    assert out.data_ptr() == inplace.data_ptr() and torch.equal(out, m3)
    guarded = ops.ddim_sample_guarded(packed, ctx, toks, coef, x_T, pin=(known, [4, 0]))
    assert torch.equal(guarded, m3)


def test_model_sample_pin():
    """model.sample(pin=...): eager and use_graph=True bitwise equal; another rows / known goes through the same captured graph; the
    trace form carries the pin as well."""
    from test_gpu_loop_form import _model

    from soccerdiffusion_amd.ml.model.model import _model_cache

    d, J, L, T, B, Mc = 256, 20, 2, 10, 3, 10
    m, _ = _model(d, J, L, T)
    g = torch.Generator().manual_seed(11)
    graphs = []
    for rows in ([0, 3, 10], torch.tensor([4, 4, 0]), 2):
        x_T, known = torch.randn(B, T, J, generator=g).cuda(), torch.randn(B, T, J, generator=g).cuda()
        ctx = [torch.randn(B, Mc, d, generator=g).cuda()]
        eager = m.sample(ctx, x_T, N_STEPS, pin=(known, rows))
        graphed = m.sample(ctx, x_T, N_STEPS, use_graph=True, pin=(known, rows))
        assert torch.equal(eager, graphed)
        mask = pin_ref.pin_mask(rows, B, T).expand(B, T, J).cuda()
        assert torch.equal(eager[mask], known[mask]) and not torch.equal(eager[~mask], known[~mask])
        graphs.append(next(iter(_model_cache(m, "graphs").values())))
        x, trace = m.sample(ctx, x_T, N_STEPS, return_trace=True, pin=(known, rows))
        assert torch.equal(x, eager) and torch.equal(trace[-1], eager)
    assert graphs[0] is graphs[1] is graphs[2] and graphs[0].pin is not None
    # the call without a pin is another graph, and what it was before
    plain = m.sample(ctx, x_T, N_STEPS, use_graph=True)
    assert torch.equal(plain, m.sample(ctx, x_T, N_STEPS))
    assert next(iter(_model_cache(m, "graphs").values())).pin is None
