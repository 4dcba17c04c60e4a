"""Held elements of the sampler on the GPU (sd_ddim_sample_hold: the hold instantiations of the trajectory step kernels, ddim_hold_kernel
behind the row-panel and chain routes) against the CPU reference tests/hold_ref.py, after EVERY denoising step, on every route
``sampler_plan`` can return; against the pinned call where the mask is one of leading rows; with several draws per context; and through
``End2EndDiffusionTransformer.sample(hold=...)``, eager and from a captured graph."""

import pytest
import torch

import hold_ref
from conftest import rel_err
from oracle import ddim_ref
from oracle import denoiser_ref as ref

pytestmark = pytest.mark.gpu
TOL = 1e-4          # the project's parity bar: tests/test_gpu_generic_traj.py
FAMILY_TOL = 2e-5   # two instantiations on the same inputs: tests/test_gpu_generic_traj.py:77
N_STEPS = 4


def _m(B, T, J):
    return torch.zeros(B, T, J, dtype=torch.bool)


def _none_joints01_lastrow_all(B, T, J):
    m = _m(B, T, J)
    m[1, :, :2] = True
    m[1, -1] = True
    m[2] = True
    return m


def _tile_edge_rows_group_edge_joints(B, T, J):
    """rows 15 and 16 (two token tiles) with joints {3, 4} (two groups of four), {15, 16} (two n-tiles), and all four"""
    m = _m(B, T, J)
    for b, joints in enumerate(([3, 4], [15, 16], [3, 4, 15, 16])):
        for t in (15, 16):
            m[b, t, joints] = True
    return m


def _ragged_tile_rows(B, T, J):
    m = _m(B, T, J)
    m[0, 96:100] = True            # the ragged tile of NTT = 7, whole rows
    m[1, 96:100, 1:3] = True       # ... and two joints of them: bits 0110 of a group
    return m


def _ragged_joints(B, T, J):
    m = _m(B, T, J)
    m[:, :, [2, 6]] = True         # J = 7: joint 6 is the last group's only second element
    m[0, -1] = True
    return m


def _random(p, seed):
    def make(B, T, J):
        m = torch.rand(B, T, J, generator=torch.Generator().manual_seed(seed)) < p
        m[0, 0] = True             # with a whole row, an empty row and a single element in it
        m[0, 1] = False
        m[0, 1, J - 1] = True
        return m
    return make


def _last_two_joints(B, T, J):
    m = _m(B, T, J)
    m[1, :, [J - 2, J - 1]] = True
    m[2, :, [J - 2, J - 1]] = True
    m[2, 0] = True
    return m


def _joint_31(B, T, J):
    m = _m(B, T, J)
    m[:, :, 31] = True
    m[1, :5, 0] = True
    return m


def _rows_16_and_17(B, T, J):
    m = _m(B, T, J)
    m[0, 15:17] = True             # the sixteenth and seventeenth row: the last of tile 0 and the only one of tile 1
    m[1, 16, :10] = True
    return m


CASES = [
    # route, (d, T, Mc, J, L, B), mask, max_mode
    ("TRAJ_TUNED", (256, 10, 10, 20, 2, 3), _none_joints01_lastrow_all, 3),
    ("TRAJ_TUNED", (256, 20, 10, 20, 1, 3), _tile_edge_rows_group_edge_joints, 3),
    ("TRAJ_TUNED", (256, 100, 10, 20, 1, 2), _ragged_tile_rows, 3),
    ("TRAJ_TUNED", (256, 10, 10, 7, 1, 2), _ragged_joints, 3),
    ("TRAJ_TUNED_WIDE", (256, 10, 50, 20, 2, 2), _random(0.35, 1), 3),
    ("TRAJ_GENERIC", (128, 10, 311, 22, 2, 3), _last_two_joints, 3),
    ("TRAJ_GENERIC", (128, 10, 40, 32, 1, 2), _joint_31, 3),
    ("TRAJ_GENERIC", (512, 17, 70, 20, 1, 2), _rows_16_and_17, 3),
    ("CHAINS_F32", (64, 10, 5, 20, 1, 2), _random(0.35, 2), 3),
    ("FUSED_FOLD_F16", (256, 100, 10, 20, 1, 2), _random(0.35, 3), 2),
    ("FUSED_FOLD", (256, 100, 10, 20, 1, 2), _random(0.35, 4), 1),
    ("FUSED", (256, 100, 10, 20, 1, 2), _random(0.35, 5), 0),
]


def _setup(shape, seed=0, n_ctx=None):
    """The packed synthetic denoiser of a shape with inputs on the host: (sd, packed, toks, coef, ts, acp, x_T, known, ctx)."""
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
    return sd, packed, toks, coef, ts, acp, x_T, known, ctx


@pytest.mark.parametrize("route,shape,make_mask,max_mode", CASES, ids=[f"{c[0]}-{'x'.join(map(str, c[1]))}-m{c[3]}" for c in CASES])
def test_held_rollout_every_step(route, shape, make_mask, max_mode):
    from soccerdiffusion_amd import _lib, ops

    d, T, Mc, J, L, B = shape
    assert _lib.sampler_route(d, 4, T, Mc, J, L, B, max_mode) == route
    sd, packed, toks, coef, ts, acp, x_T, known, ctx = _setup(shape)
    mask = make_mask(B, T, J)
    assert mask.any() and not mask.all()
    want, want_held, want_eps = hold_ref.sample(lambda x, t: ref.forward_with_context(sd, [ctx], x, torch.full((B,), t, dtype=torch.int64)),
                                                x_T, known, mask, N_STEPS, acp)
    status = torch.ones(1, dtype=torch.int32, device="cuda")
    x_dev, known_dev, words = x_T.cuda(), known.cuda(), ops.hold_mask(mask, B, T, J, "cuda")
    assert torch.equal(words.cpu(), hold_ref.pack(mask))
    words_before = words.clone()
    xm, trm, epm = ops.ddim_sample(packed, ctx.cuda(), toks, coef, x_dev, trace=True, eps_trace=True, max_mode=max_mode, status=status,
                                   hold=(known_dev, words))
    assert torch.equal(x_dev.cpu(), x_T) and torch.equal(known_dev.cpu(), known) and torch.equal(words, words_before)   # inputs are only read
    trm, epm = trm.cpu(), epm.cpu()
    free = ~mask
    for i in range(N_STEPS):
        # free elements and the noise prediction of ALL elements: the parity bar
        e_x = rel_err(torch.where(free, trm[i], torch.zeros(())), torch.where(free, want[i], torch.zeros(())))
        e_eps = rel_err(epm[i], want_eps[i])
        # held elements, elementwise: two evaluations of c2 K + c3 N with three roundings each, with or without contraction
        c2, c3 = float(coef[i, 2]), float(coef[i, 3])
        bound = 2.0 ** -21 * ((c2 * known.double()).abs() + (c3 * x_T.double()).abs())
        excess = ((trm[i].double() - want_held[i].double()).abs() - bound)[mask]
        print(f"{route} {shape} step {i}: free elements {e_x:.3e}, eps {e_eps:.3e}, held elements worst |diff| - bound {float(excess.max()):.3e}")
        assert e_x < TOL and e_eps < TOL, (i, e_x, e_eps)
        assert (excess <= 0).all(), (i, float(excess.max()))
    assert torch.equal(trm[-1][mask].view(torch.int32), known[mask].view(torch.int32))      # the last step leaves known itself, bit for bit
    assert torch.equal(xm.cpu(), trm[-1])
    assert int(status.item()) == 0 and torch.isfinite(xm).all()
    # the bool mask and the packed words are the same call
    again = ops.ddim_sample(packed, ctx.cuda(), toks, coef, x_dev, max_mode=max_mode, hold=(known_dev, mask.cuda()))
    assert torch.equal(again, xm)


LEADING = [
    ("TRAJ_TUNED", (256, 20, 10, 20, 1, 3), [16, 17, 1]),
    ("TRAJ_TUNED_WIDE", (256, 10, 50, 20, 2, 2), [5, 2]),
    ("TRAJ_GENERIC", (128, 10, 311, 22, 2, 3), [0, 3, 10]),
]


@pytest.mark.parametrize("route,shape,rows", LEADING, ids=[c[0] for c in LEADING])
def test_leading_rows_mask_is_the_pinned_call(route, shape, rows):
    """Within FAMILY_TOL after every step, bit for bit on the held rows at the last one.  Whether the WHOLE output is bitwise equal is
    printed, not asserted; measured on an MI355X it is, on all three routes, and so is the all-zero mask against the call without a pin
    (DESIGN.md 5.7.1)."""
    from soccerdiffusion_amd import _lib, ops

    d, T, Mc, J, L, B = shape
    assert _lib.sampler_route(d, 4, T, Mc, J, L, B, 3) == route
    _, packed, toks, coef, _, _, x_T, known, ctx = _setup(shape, seed=1)
    x_dev, known_dev, ctx_dev = x_T.cuda(), known.cuda(), ctx.cuda()
    none = torch.zeros(J, dtype=torch.bool)
    words = ops.hold_mask(none, B, T, J, "cuda", rows=rows)
    assert torch.equal(words.cpu(), hold_ref.pack(hold_ref.rows_mask(torch.tensor(rows), B, T, J)))
    held, trh = ops.ddim_sample(packed, ctx_dev, toks, coef, x_dev, trace=True, hold=(known_dev, words))
    pinned, trp = ops.ddim_sample(packed, ctx_dev, toks, coef, x_dev, trace=True, pin=(known_dev, rows))
    mask = hold_ref.rows_mask(torch.tensor(rows), B, T, J).cuda()
    for i in range(N_STEPS):
        err = rel_err(trh[i], trp[i])
        print(f"{route} {shape} step {i}: leading-rows hold against the pin {err:.3e}, bitwise equal: {torch.equal(trh[i], trp[i])}")
        assert err < FAMILY_TOL, (i, err)
    assert torch.equal(held[mask].view(torch.int32), pinned[mask].view(torch.int32))
    assert torch.equal(held[mask].view(torch.int32), known_dev[mask].view(torch.int32))
    print(f"{route} {shape}: whole output of the leading-rows hold bitwise equal to the pinned call: {torch.equal(held, pinned)}")
    # nothing held: the call without a pin
    empty = ops.ddim_sample(packed, ctx_dev, toks, coef, x_dev, hold=(known_dev, none.cuda()))
    plain = ops.ddim_sample(packed, ctx_dev, toks, coef, x_dev)
    err = rel_err(empty, plain)
    print(f"{route} {shape}: all-zero mask against the call without a pin {err:.3e}, bitwise equal: {torch.equal(empty, plain)}")
    assert err < FAMILY_TOL


DRAWS = [("TRAJ_TUNED", (256, 10, 10, 20, 1, 6), _random(0.35, 6)), ("TRAJ_GENERIC", (128, 10, 40, 22, 1, 6), _random(0.35, 7))]


@pytest.mark.parametrize("route,shape,make_mask", DRAWS, ids=[c[0] for c in DRAWS])
def test_draws_equal_the_hold_on_the_repeated_context_bitwise(route, shape, make_mask):
    from soccerdiffusion_amd import _lib, ops

    d, T, Mc, J, L, B = shape
    G = 3
    assert _lib.sampler_route_draws(d, 4, T, Mc, J, L, B, G, 3) == route
    _, packed, toks, coef, _, _, x_T, known, ctx = _setup(shape, seed=2, n_ctx=B // G)
    hold = (known.cuda(), ops.hold_mask(make_mask(B, T, J), B, T, J, "cuda"))
    shared, trs = ops.ddim_sample(packed, ctx.cuda(), toks, coef, x_T.cuda(), trace=True, hold=hold, draws=G)
    repeated, trr = ops.ddim_sample(packed, ctx.cuda().repeat_interleave(G, 0).contiguous(), toks, coef, x_T.cuda(), trace=True, hold=hold)
    assert torch.equal(trs, trr) and torch.equal(shared, repeated) and torch.isfinite(shared).all()
    mask = make_mask(B, T, J).cuda()
    assert torch.equal(shared[mask].view(torch.int32), hold[0][mask].view(torch.int32))
    with pytest.raises(ValueError, match="draws"):
        ops.ddim_sample(packed, ctx.cuda(), toks, coef, x_T.cuda(), hold=hold, draws=4)


def test_hold_arguments_on_the_device():
    """What the call checks itself: shapes, devices, pin beside hold, J > 32; a mode-4 cap runs the mode-3 kernels; the guarded and the
    in-place forms."""
    from soccerdiffusion_amd import ops

    shape = (256, 10, 10, 20, 1, 2)
    d, T, Mc, J, L, B = shape
    _, packed, toks, coef, _, _, x_T, known, ctx = _setup(shape, seed=3)
    x_T, known, ctx = x_T.cuda(), known.cuda(), ctx.cuda()
    mask = _random(0.35, 8)(B, T, J)
    for bad in ((known, mask[:, :5]), (known[:, :5], mask), (known.cpu(), mask), (known, mask.float()), known, (known, None)):
        with pytest.raises((ValueError, RuntimeError)):
            ops.ddim_sample(packed, ctx, toks, coef, x_T, hold=bad)
    with pytest.raises(ValueError, match="exclude"):
        ops.ddim_sample(packed, ctx, toks, coef, x_T, hold=(known, mask), pin=(known, 2))
    m3 = ops.ddim_sample(packed, ctx, toks, coef, x_T, max_mode=3, hold=(known, mask))
    m4 = ops.ddim_sample(packed, ctx, toks, coef, x_T, max_mode=4, hold=(known, mask))     # no hold twin of mode 4: the mode-3 kernels
    assert torch.equal(m3, m4)
    inplace = x_T.clone()
    out = ops.ddim_sample(packed, ctx, toks, coef, inplace, max_mode=3, inplace=True, hold=(known, mask))     # a private copy of the noise
    assert out.data_ptr() == inplace.data_ptr() and torch.equal(out, m3)
    assert torch.equal(ops.ddim_sample_guarded(packed, ctx, toks, coef, x_T, hold=(known, mask)), m3)
    # J > 32 is refused before anything is launched (the library's own SD_E_BADARG: tests/test_cpu_hold.py)
    x40 = torch.zeros(B, T, 40, device="cuda")
    for m40 in (torch.zeros(B, T, 40, dtype=torch.bool), torch.zeros(B, T, dtype=torch.int32, device="cuda")):
        with pytest.raises(ValueError, match="32"):
            ops.ddim_sample(packed, ctx, toks, coef, x40, hold=(x40, m40))


def test_model_sample_hold():
    """model.sample(hold=...): eager and use_graph=True bitwise equal; three masks go through one captured graph; the trace and draws
    forms carry the hold as well; the call without a hold is another graph and what it was before."""
    from test_gpu_loop_form import _model

    from soccerdiffusion_amd.ml.model.model import _model_cache

    d, J, L, T, B, Mc = 256, 20, 2, 10, 3, 10
    m, _ = _model(d, J, L, T)
    g = torch.Generator().manual_seed(11)
    graphs = []
    joints = torch.zeros(J, dtype=torch.bool)
    joints[[0, 1]] = True
    for mask in (_none_joints01_lastrow_all(B, T, J), joints, _random(0.35, 9)(B, T, J)):
        x_T, known = torch.randn(B, T, J, generator=g).cuda(), torch.randn(B, T, J, generator=g).cuda()
        ctx = [torch.randn(B, Mc, d, generator=g).cuda()]
        eager = m.sample(ctx, x_T, N_STEPS, hold=(known, mask))
        graphed = m.sample(ctx, x_T, N_STEPS, use_graph=True, hold=(known, mask))
        assert torch.equal(eager, graphed)
        full = mask.expand(B, T, J).cuda()
        assert torch.equal(eager[full], known[full]) and not torch.equal(eager[~full], known[~full])
        graphs.append(next(iter(_model_cache(m, "graphs").values())))
        x, trace = m.sample(ctx, x_T, N_STEPS, return_trace=True, hold=(known, mask))
        assert torch.equal(x, eager) and torch.equal(trace[-1], eager)
    assert graphs[0] is graphs[1] is graphs[2] and graphs[0].hold is not None and graphs[0].pin is None
    # draws: the context of one observation for all three trajectories
    one = [ctx[0][:1].contiguous()]
    shared = m.sample(one, x_T, N_STEPS, hold=(known, mask), draws=3)
    assert torch.equal(shared, m.sample([one[0].expand(3, Mc, d).contiguous()], x_T, N_STEPS, hold=(known, mask)))
    assert torch.equal(shared, m.sample(one, x_T, N_STEPS, use_graph=True, hold=(known, mask), draws=3))
    with pytest.raises(ValueError, match="exclude"):
        m.sample(ctx, x_T, N_STEPS, hold=(known, mask), pin=(known, 2))
    # the call without a hold is another graph, and what it was before
    plain = m.sample(ctx, x_T, N_STEPS, use_graph=True)
    assert torch.equal(plain, m.sample(ctx, x_T, N_STEPS))
    assert next(iter(_model_cache(m, "graphs").values())).hold is None
