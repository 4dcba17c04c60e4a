"""Several draws per observation on the GPU: sd_ddim_sample_draws (C contexts, G draws each, trajectory b reads context b // G, prepared once
per context) against the call on the repeated context, bit for bit on every route; pinned rows; the fp64 oracle; sd_select_medoid against
tests/draws_ref.py; PolicySession(draws=G) and the command line.  Seeded synthetic weights everywhere."""

import ctypes as C
import math

import numpy as np
import pytest
import torch

import draws_ref
import parity

pytestmark = pytest.mark.gpu
HEADS, L, STEPS, CN = 4, 2, 3, 3

# name -> (d, Mc, T, J, n_steps, max_mode, extra keywords, route, launches of the step-kernel class per call or None where it has none)
ROUTES = {
    "tuned-fused": (256, 9, 10, 20, STEPS, 3, {}, "TRAJ_TUNED", 1),
    "tuned-steps": (256, 9, 10, 20, STEPS, 3, {"trace": True}, "TRAJ_TUNED", STEPS),
    "tuned-2p": (256, 9, 10, 20, STEPS, 4, {}, "TRAJ_TUNED_2P", 1),
    "wide": (256, 20, 10, 20, STEPS, 3, {}, "TRAJ_TUNED_WIDE", STEPS),
    "generic128": (128, 30, 10, 20, STEPS, 3, {"eps_trace": True}, "TRAJ_GENERIC", STEPS),
    "generic512": (512, 5, 10, 20, STEPS, 3, {}, "TRAJ_GENERIC", STEPS),
    "panel": (256, 9, 10, 20, STEPS, 1, {}, None, None),
}
LARGE = {"T100-J22": (256, 9, 100, 22, STEPS, 3, {}, "TRAJ_TUNED", 1)}   # the largest NTT and the scalar-load path of J & 3
CHUNK = {"chunk65": (256, 9, 10, 20, 65, 3, {}, "TRAJ_TUNED", 2)}        # the 64-step chunk boundary re-derives the context index


class Setup:
    """Weights, step tokens and coefficients of one (d, J, n_steps), packed once per module."""
    cache = {}

    def __init__(self, d, J, n_steps):
        from oracle import ddim_ref
        from oracle import denoiser_ref as ref
        from soccerdiffusion_amd import ops

        self.sd = ref.synthetic_state_dict(d, J, L, seed=33)
        self.packed = ops.pack_denoiser(self.sd, "cuda", heads=HEADS, max_len=100)
        self.acp = ddim_ref.alphas_cumprod()
        self.ts = ddim_ref.timesteps(n_steps).tolist()
        self.toks = ops.step_token(torch.tensor(self.ts).cuda(), ops.step_frequencies(d).cuda(), self.sd["step_encoding.token"].cuda()).reshape(n_steps, d)
        self.coef = ops.ddim_coefficients(self.ts, self.acp, n_steps)

    @classmethod
    def get(cls, d, J, n_steps):
        key = (d, J, n_steps)
        if key not in cls.cache:
            cls.cache[key] = cls(d, J, n_steps)
        return cls.cache[key]


def _inputs(seed, Cn, G, d, Mc, T, J):
    """Noise (C * G, T, J), and C contexts of distinct magnitudes (context c scaled by 2^c): a kernel that reads another context's planes
    cannot pass by accident, and the abs-max shared by the contexts is set by the last one alone."""
    g = torch.Generator().manual_seed(seed)
    x_T = torch.randn(Cn * G, T, J, generator=g)
    ctx = torch.randn(Cn, Mc, d, generator=g) * (2.0 ** torch.arange(Cn, dtype=torch.float32)).view(Cn, 1, 1)
    known = torch.randn(Cn * G, T, J, generator=g)
    return x_T.cuda(), ctx.cuda(), known.cuda()


def _call(setup, ctx, x_T, mode, draws, **kw):
    """(outputs as a tuple, status word, launches of the step-kernel class)"""
    from soccerdiffusion_amd import _lib, ops

    lib = _lib.load()
    ncls = len(_lib.KERNEL_CLASSES)
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    lib.sd_profile_enable(1)
    try:
        out = ops.ddim_sample(setup.packed, ctx, setup.toks, setup.coef, x_T, status=status, max_mode=mode, draws=draws, **kw)
        torch.cuda.synchronize()
    finally:
        lib.sd_profile_enable(0)
    ms, cnt = (C.c_double * ncls)(), (C.c_long * ncls)()
    _lib.check(lib.sd_profile_collect(ms, cnt, ncls), "sd_profile_collect")
    out = out if isinstance(out, tuple) else (out,)
    return out, int(status.item()), int(cnt[_lib.KERNEL_CLASSES.index("traj_step_kernel")])


def _shared_equals_repeated(case, G, seed, pin_rows=None):
    from soccerdiffusion_amd import _lib

    d, Mc, T, J, n_steps, mode, kw, route, launches = case
    setup = Setup.get(d, J, n_steps)
    x_T, ctx, known = _inputs(seed, CN, G, d, Mc, T, J)
    kw = dict(kw)
    if pin_rows is not None:
        rows = torch.tensor(pin_rows(T, CN * G), dtype=torch.int32)
        kw["pin"] = (known, rows)
    if route is not None:
        assert _lib.sampler_route_draws(d, HEADS, T, Mc, J, L, CN * G, G, mode) == route
    shared, st_s, n_s = _call(setup, ctx, x_T, mode, G, **kw)
    repeated, st_r, n_r = _call(setup, ctx.repeat_interleave(G, 0).contiguous(), x_T, mode, 1, **kw)
    assert len(shared) == len(repeated) == 1 + len([k for k in kw if k in ("trace", "eps_trace")])
    for a, b in zip(shared, repeated):
        assert a.shape == b.shape and torch.isfinite(a).all()
        assert torch.equal(a, b)
    assert st_s == st_r
    if launches is not None and pin_rows is None:
        assert n_s == n_r == launches, (n_s, n_r)    # the same rollout form on both sides: fused stays fused
    elif pin_rows is not None and route is not None:
        assert n_s == n_r == n_steps                 # a pinned shared call stays one launch per step
    # the draws of a context differ from one another, and the contexts matter: not a constant, not one context for all
    x0 = shared[0].view(CN, G, T, J)
    assert not torch.equal(x0[:, 0], x0[:, 1])
    return shared[0], kw.get("pin")


@pytest.mark.parametrize("G", [2, 5])
@pytest.mark.parametrize("name", list(ROUTES))
def test_shared_equals_repeated_bit_for_bit(name, G):
    _shared_equals_repeated(ROUTES[name], G, 7000 + 10 * list(ROUTES).index(name) + G)


def test_shared_reads_its_own_context():
    """The check above cannot be passed by reading context 0 for everybody: with the contexts swapped the samples move with them."""
    d, Mc, T, J, n_steps, mode, kw, _, _ = ROUTES["tuned-fused"]
    setup = Setup.get(d, J, n_steps)
    x_T, ctx, _ = _inputs(7100, CN, 2, d, Mc, T, J)
    a = _call(setup, ctx, x_T, mode, 2)[0][0].view(CN, 2, T, J)
    b = _call(setup, ctx.flip(0).contiguous(), x_T, mode, 2)[0][0].view(CN, 2, T, J)
    assert not torch.equal(a[0], b[0]) and not torch.equal(a[2], b[2])
    assert torch.equal(a[1], b[1])   # the middle context keeps its place, and the shared scale words are the same maxima


def test_largest_horizon_and_ragged_joint_count():
    _shared_equals_repeated(LARGE["T100-J22"], 2, 7200)


def test_chunk_boundary_of_the_fused_rollout():
    _shared_equals_repeated(CHUNK["chunk65"], 2, 7300)


def _counted(call):
    """Launches of the step-kernel class made by call() (a native entry point through ctypes; its return code is checked)."""
    from soccerdiffusion_amd import _lib

    lib = _lib.load()
    ncls = len(_lib.KERNEL_CLASSES)
    torch.cuda.synchronize()
    lib.sd_profile_enable(1)
    try:
        _lib.check(call(), "native sampler call")
        torch.cuda.synchronize()
    finally:
        lib.sd_profile_enable(0)
    ms, cnt = (C.c_double * ncls)(), (C.c_long * ncls)()
    _lib.check(lib.sd_profile_collect(ms, cnt, ncls), "sd_profile_collect")
    return int(cnt[_lib.KERNEL_CLASSES.index("traj_step_kernel")])


def test_one_draw_through_the_new_entry_point_is_the_old_call():
    """ops.ddim_sample and GraphedSampler always go through sd_ddim_sample_draws, so the "old call" side is made here, through ctypes: every
    older entry point against sd_ddim_sample_draws(draws = 1) and against ops.ddim_sample, bit for bit and launch for launch - unpinned
    (the fused rollout form: one launch) and pinned (one launch per step)."""
    from soccerdiffusion_amd import _lib, ops

    d, Mc, T, J, n_steps, mode, _, _, _ = ROUTES["tuned-fused"]
    assert (d, L, T, J, Mc, CN, n_steps, mode) == (256, 2, 10, 20, 9, 3, 3, 3)
    setup = Setup.get(d, J, n_steps)
    x_T, ctx, known = _inputs(7400, CN, 1, d, Mc, T, J)
    lib = _lib.load()
    ws = ops.workspace(lib.sd_workspace_floats(CN, T, Mc, d, L, n_steps), x_T.device)
    head = (C.byref(setup.packed.struct), ctx.data_ptr(), setup.toks.data_ptr(), setup.coef.ctypes.data_as(_lib.c_float_p))
    shape, st = (CN, T, Mc, n_steps), torch.cuda.current_stream().cuda_stream

    # unpinned
    want, _, n_ops = _call(setup, ctx, x_T, mode, 1)
    assert n_ops == 1
    calls = {
        "sd_ddim_sample": lambda x: lib.sd_ddim_sample(*head, x, None, ws.data_ptr(), *shape, st),
        "sd_ddim_sample_ex": lambda x: lib.sd_ddim_sample_ex(*head, x, None, ws.data_ptr(), *shape, None, mode, st),
        "sd_ddim_sample_eps": lambda x: lib.sd_ddim_sample_eps(*head, x, None, None, ws.data_ptr(), *shape, None, mode, st),
        "sd_ddim_sample_draws": lambda x: lib.sd_ddim_sample_draws(*head, x, None, None, ws.data_ptr(), *shape, None, mode, None, None, None, 1, st),
    }
    for name, fn in calls.items():
        x = x_T.clone()
        assert _counted(lambda: fn(x.data_ptr())) == 1, name
        assert torch.equal(x, want[0]), name

    # pinned
    rows = torch.tensor([0, 3, 10], dtype=torch.int32, device="cuda")
    want, _, n_ops = _call(setup, ctx, x_T, mode, 1, pin=(known, rows), eps_trace=True)
    assert n_ops == n_steps and len(want) == 2
    pins = (known.data_ptr(), x_T.data_ptr(), rows.data_ptr())
    calls = {
        "sd_ddim_sample_pin": lambda x, et: lib.sd_ddim_sample_pin(*head, x, None, et, ws.data_ptr(), *shape, None, mode, *pins, st),
        "sd_ddim_sample_draws": lambda x, et: lib.sd_ddim_sample_draws(*head, x, None, et, ws.data_ptr(), *shape, None, mode, *pins, 1, st),
    }
    for name, fn in calls.items():
        x, et = x_T.clone(), torch.empty(n_steps, CN, T, J, device="cuda")
        assert _counted(lambda: fn(x.data_ptr(), et.data_ptr())) == n_steps, name
        assert torch.equal(x, want[0]) and torch.equal(et, want[1]), name
    assert torch.equal(want[0][1, :3], known[1, :3]) and torch.equal(want[0][2], known[2])

    # the captured form of the pinned call
    graphed = ops.GraphedSampler(setup.packed, CN, T, Mc, setup.toks, setup.coef, max_mode=mode, pin=True)
    assert torch.equal(graphed(ctx, x_T, pin=(known, rows)), want[0])


def _mixed_rows(T, B):
    return [(0, 3, T, 1, 0, 5, 2, T - 1, 0, 4)[b % 10] for b in range(B)]


@pytest.mark.parametrize("name", ["tuned-fused", "wide", "generic128"])
def test_pin_and_draws(name):
    case = ROUTES[name]
    case = case[:6] + ({},) + case[7:]
    G = 2
    x0, (known, rows) = _shared_equals_repeated(case, G, 7500 + list(ROUTES).index(name), pin_rows=_mixed_rows)
    assert 0 in rows.tolist() and max(rows.tolist()) == case[2]
    for b, r in enumerate(rows.tolist()):
        assert torch.equal(x0[b, :r], known[b, :r]), b
        if r < case[2]:
            assert not torch.equal(x0[b, r], known[b, r]), b


def test_shared_call_against_the_fp64_oracle():
    """The project's bar on a sampler call - 1e-4 relative on each of parity.py's figures - for one shared call: d = 256, Mc = 9, C = 2, G = 3."""
    from oracle import ddim_ref
    from oracle import denoiser_ref as ref

    d, Mc, T, J, Cn, G = 256, 9, 10, 20, 2, 3
    setup = Setup.get(d, J, STEPS)
    x_T, ctx, _ = _inputs(7600, Cn, G, d, Mc, T, J)
    got = _call(setup, ctx, x_T, 3, G)[0][0].cpu()
    mem = ctx.cpu().repeat_interleave(G, 0).double()
    denoise = lambda x, t: ref.forward_with_context(setup.sd, [mem], x, torch.full((Cn * G,), t, dtype=torch.int64), dtype=torch.float64)
    want64 = ddim_ref.sample(denoise, x_T.cpu().double(), STEPS, setup.acp)[-1]
    e = parity.errors(got, want64)
    print(f"shared call against the fp64 oracle: glob {e.glob:.3e} traj {e.traj:.3e} row {e.row:.3e}")
    assert e.glob < 1e-4 and e.traj < 1e-4 and e.row < 1e-4, e


# ---- the medoid ------------------------------------------------------------------------------------------------------------------------
MEDOID_T, MEDOID_J, MEDOID_C = 10, 20, 4
MEDOID_SEEDS = {1: 0, 2: 0, 5: 0, 64: 1}   # seeds whose fp64 runner-up margin passes the check below in every context (checked on the CPU)
MARGIN = 1e-3   # the fp32 sums carry at most (T J + G) 2^-23 ~ 3e-5 relative error: 30 x below


def _medoid_inputs(G):
    g = torch.Generator().manual_seed(8000 + 100 * G + MEDOID_SEEDS[G])
    # draws at different distances from their context's centre: the scores of a context are spread, as a policy's draws are
    centre = torch.randn(MEDOID_C, 1, MEDOID_T, MEDOID_J, generator=g)
    spread = 0.5 + torch.rand(MEDOID_C, G, 1, 1, generator=g)
    return centre + spread * torch.randn(MEDOID_C, G, MEDOID_T, MEDOID_J, generator=g)


@pytest.mark.parametrize("G", [1, 2, 5, 64])
def test_medoid_equals_the_fp64_reference(G):
    from soccerdiffusion_amd import ops

    x = _medoid_inputs(G)
    want = draws_ref.medoid(x.numpy(), G)
    margin = draws_ref.margins(x.numpy(), G)
    if G >= 3:
        assert (margin > MARGIN).all(), margin      # every context, none skipped: the seeds are chosen for it
    elif G == 2:
        assert (margin == 0).all() and (want == 0).all()   # two draws are equidistant from each other: an exact tie in any arithmetic, index 0
    xg = x.cuda().contiguous()
    index, chosen = ops.select_medoid(xg, G)
    assert index.dtype == torch.int32 and index.cpu().tolist() == want.tolist()
    assert torch.equal(chosen.cpu(), torch.stack([x[c, int(want[c])] for c in range(MEDOID_C)]))
    index2, none = ops.select_medoid(xg.view(MEDOID_C * G, MEDOID_T, MEDOID_J), G, gather=False)    # the sampler's layout; no gather
    assert none is None and torch.equal(index, index2)
    if G == 1:
        assert index.cpu().tolist() == [0] * MEDOID_C


def test_medoid_exact_tie_goes_to_the_lowest_index():
    from soccerdiffusion_amd import ops

    g = torch.Generator().manual_seed(8900)
    x = 10 * torch.randn(2, 5, MEDOID_T, MEDOID_J, generator=g)
    x[:, 1] = 0.01 * torch.randn(2, MEDOID_T, MEDOID_J, generator=g)    # near the centre of the other three: jointly best with its copy
    x[:, 3] = x[:, 1]
    s = draws_ref.scores(x.numpy(), 5)
    assert (s[:, 1] == s[:, 3]).all() and (np.delete(s, [1, 3], axis=1).min(axis=1) > s[:, 1] * (1 + MARGIN)).all()
    index, chosen = ops.select_medoid(x.cuda(), 5)
    assert index.cpu().tolist() == [1, 1] and torch.equal(chosen.cpu(), x[:, 1])


# ---- the session -----------------------------------------------------------------------------------------------------------------------
SB, SG, ST, SSTEPS = 2, 4, 10, 3


@pytest.fixture(scope="module")
def tiny256():
    """d = 256, L = 2, T = 10, no images: 13 context rows, the tuned trajectory kernels."""
    from test_gpu_session import TINY, _synthetic_model

    params = {**TINY, "hidden_dim": 256, "trajectory_prediction_length": ST}
    return _synthetic_model(params)[0], params


def _feed(sessions, g, S=SB, robots=None, n=5):
    q, r = (torch.rand(S, n, 20, generator=g) - 0.5) * 6, torch.randn(S, n, 4, generator=g)
    for s in sessions:
        s.push_joint_state(q.cuda(), robots=robots)
        s.push_rotation(r.cuda(), robots=robots)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def test_session_returns_the_medoid_of_its_draws(tiny256, monkeypatch):
    from soccerdiffusion_amd.session import PolicySession

    model, _ = tiny256
    s = PolicySession(model, num_inference_steps=SSTEPS, batch=SB, draws=SG)
    seen = []
    real = model.sample
    monkeypatch.setattr(model, "sample", lambda ctx, x_T, *a, **k: (seen.append(([tuple(c.shape) for c in ctx], tuple(x_T.shape), k.get("draws"))), real(ctx, x_T, *a, **k))[1])
    g = torch.Generator().manual_seed(51)
    _feed([s], g)
    # start noise of a different magnitude per draw: the draws of a robot then lie at clearly different distances from one another
    x_T = (torch.randn(SB, SG, ST, 20, generator=g) * torch.tensor([1.0, 0.6, 1.4, 1.8]).view(1, SG, 1, 1)).view(SB * SG, ST, 20).cuda()
    traj, draws, index = s.step(x_T, return_draws=True)
    assert traj.shape == (SB, ST, 20) and draws.shape == (SB, SG, ST, 20) and index.shape == (SB,) and index.dtype == torch.int32
    for b in range(SB):
        assert _same_bits(traj[b], draws[b, int(index[b])])
    # the selection is the reference's on the draws the session returned, taken back to the space the sampler works in (the distances
    # are measured there; the model's std differs from joint to joint): (published + pi - mean) / std in float64
    back = (draws.cpu().double() + math.pi - model.mean.cpu().double()) / model.std.cpu().double()
    margin = draws_ref.margins(back.numpy(), SG)
    print(f"session draws: index {index.cpu().tolist()}, fp64 margins {margin}")
    assert (margin > MARGIN).all(), margin
    assert index.cpu().tolist() == draws_ref.medoid(back.numpy(), SG).tolist()
    # the context encoders ran once per robot: SB rows of context for SB * SG trajectories
    (ctx_shapes, x_shape, k_draws), = seen
    assert all(c[0] == SB for c in ctx_shapes) and x_shape == (SB * SG, ST, 20) and k_draws == SG


def test_session_with_one_draw_is_the_session_of_old(tiny256):
    from soccerdiffusion_amd.session import PolicySession

    model, _ = tiny256
    a, b = PolicySession(model, num_inference_steps=SSTEPS, batch=SB, draws=1), PolicySession(model, num_inference_steps=SSTEPS, batch=SB)
    g = torch.Generator().manual_seed(52)
    for tick in range(3):
        _feed([a, b], g)
        ta, tb = a.step(), b.step()
        assert _same_bits(ta, tb), tick
    t, d, i = a.step(return_draws=True)
    assert _same_bits(d[:, 0], t) and i.tolist() == [0] * SB


def test_session_carry_takes_the_selected_draws_rows(tiny256):
    from soccerdiffusion_amd.session import PolicySession

    model, _ = tiny256
    K, ADV = 3, 5
    s = PolicySession(model, num_inference_steps=SSTEPS, batch=SB, draws=SG, carry=K, advance=ADV)
    g = torch.Generator().manual_seed(53)
    prev = None
    for tick in range(3):
        _feed([s], g)
        traj, draws, index = s.step(return_draws=True)
        if prev is not None:
            assert _same_bits(traj[:, :K], prev[:, ADV:ADV + K]), tick
            for k in range(SG):   # all draws share the seam
                assert _same_bits(draws[:, k, :K], prev[:, ADV:ADV + K]), (tick, k)
            assert not _same_bits(draws[:, 0, K:], draws[:, 1, K:])
        prev = traj


def test_session_graph_equals_eager(tiny256):
    from soccerdiffusion_amd.session import PolicySession

    model, _ = tiny256
    e = PolicySession(model, num_inference_steps=SSTEPS, batch=SB, draws=SG, carry=3, advance=5)
    c = PolicySession(model, num_inference_steps=SSTEPS, batch=SB, draws=SG, carry=3, advance=5, use_graph=True)
    g = torch.Generator().manual_seed(54)
    for tick in range(3):
        _feed([e, c], g)
        x_T = torch.randn(SB * SG, ST, 20, generator=g).cuda()
        te, de, ie = e.step(x_T, return_draws=True)
        tc, dc, ic = c.step(x_T, return_draws=True)
        assert _same_bits(te, tc) and _same_bits(de, dc) and ie.tolist() == ic.tolist(), tick
    assert c._graph is not None


def test_session_subset_tick_leaves_the_other_robot_alone(tiny256):
    from soccerdiffusion_amd.session import PolicySession

    model, _ = tiny256
    s = PolicySession(model, num_inference_steps=SSTEPS, batch=SB, draws=SG, carry=3, advance=5)
    g = torch.Generator().manual_seed(55)
    _feed([s], g)
    s.step()
    before = {k: v.clone() for k, v in s.windows(robots=[0]).items()}
    pin0 = s._pin_x0[0].clone()
    _feed([s], g, S=1, robots=[1])
    traj, draws, index = s.step(robots=[1], return_draws=True)
    assert traj.shape == (1, ST, 20) and draws.shape == (1, SG, ST, 20) and index.shape == (1,)
    assert _same_bits(traj[0], draws[0, int(index[0])])
    after = s.windows(robots=[0])
    for k in before:
        assert torch.equal(before[k], after[k]), k
    assert torch.equal(pin0, s._pin_x0[0])
    s.reset(robots=[1])
    assert s._pin_rows.tolist() == [3, 0]


# ---- the command line ------------------------------------------------------------------------------------------------------------------
def test_cli_sample_draws(tiny256, tmp_path):
    from soccerdiffusion_amd import cli

    model, params = tiny256
    ckpt, out3, out1 = str(tmp_path / "c.pt"), str(tmp_path / "s3.pt"), str(tmp_path / "s1.pt")
    torch.save({"model_state_dict": model.state_dict(), "hyperparams": params}, ckpt)
    assert cli.main(["sample", ckpt, "--steps", "3", "--num_samples", "4", "--synthetic", "8", "--draws", "3", "-o", out3]) == 0
    assert cli.main(["sample", ckpt, "--steps", "3", "--num_samples", "4", "--synthetic", "8", "-o", out1]) == 0
    s3, s1 = torch.load(out3, weights_only=True), torch.load(out1, weights_only=True)
    assert set(s1) == {"trajectories", "noise", "steps", "indices"} and s1["trajectories"].shape == (4, ST, 20)
    assert set(s3) == set(s1) | {"draws", "medoid"} and s3["draws"] == 3
    assert s3["trajectories"].shape == (4, 3, ST, 20) and s3["noise"].shape == (12, ST, 20) and s3["medoid"].shape == (4,)
    assert torch.isfinite(s3["trajectories"]).all() and ((0 <= s3["medoid"]) & (s3["medoid"] < 3)).all()
