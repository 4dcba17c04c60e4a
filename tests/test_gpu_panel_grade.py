"""The row-panel decoder routes (CHAINS_F32, CHAINS_F16, FUSED, FUSED_FOLD, FUSED_FOLD_F16: csrc/sd_kernels.hip, csrc/sd_f16x3.h) held to
fp32 grade row by row (tests/parity.py) - the routes every guarded call repeats on after SD_STATUS_NONFINITE, that sd_denoiser_forward
runs and that serve every shape the trajectory families decline.  Cases and oracles: tests/panel_cases.py; their routes are pinned without
a GPU in tests/test_cpu_panel_grade.py.  Plain rollouts with traces only: no pins, holds, limits or draws.

The yardstick is always the fp32 CPU oracle's own error against the fp64 oracle on the same inputs, at 4 x + 1e-7 on the whole tensor, per
trajectory and per row.  Every gated tensor prints one line (python -m pytest -s; profiles/panel_parity.txt is that output)."""

import functools
import warnings

import pytest
import torch

import panel_cases as pc
from oracle import ddim_ref
from parity import FACTOR, FLOOR, assert_fp32_grade, errors, report

gpu = pytest.mark.gpu
NAN = float("nan")


@functools.lru_cache(maxsize=2)
def _packed(shape):
    """(packed weights, step tokens, DDIM coefficients) of a case on the device - shared by its caps."""
    from soccerdiffusion_amd import ops

    d, T = shape[0], shape[1]
    sd = pc.inputs(shape)[0]
    toks, coef = pc.gpu_tokens(ops, sd, d, pc.N_STEPS)
    return ops.pack_denoiser(sd, "cuda", max_len=T), toks, coef


def _sample(packed, ctx, toks, coef, x, cap):
    """One call of the sampler capped at `cap`: (x trace, noise-prediction trace, status word)."""
    from soccerdiffusion_amd import ops

    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    _, tr, et = ops.ddim_sample(packed, ctx.cuda() if ctx is not None else None, toks, coef, x.cuda(), trace=True, eps_trace=True,
                                max_mode=cap, status=status)
    return tr.cpu(), et.cpu(), int(status.item())


def _route(shape, cap):
    from soccerdiffusion_amd import _lib

    d, T, Mc, J, L, B = shape
    return _lib.sampler_route(d, pc.HEADS, T, Mc, J, L, B, cap)


def _grade_rollout(name, tr, et, oracles):
    x64, eps64, x32, eps32 = oracles
    n = len(x64)
    assert_fp32_grade(et[0], eps64[0], eps32[0], factor=FACTOR, floor=FLOOR, label=f"{name} eps t=980")
    assert_fp32_grade(et[n - 1], eps64[-1], eps32[-1], factor=FACTOR, floor=FLOOR, label=f"{name} eps step {n - 1}")
    for i in range(n):
        assert_fp32_grade(tr[i], x64[i], x32[i], factor=FACTOR, floor=FLOOR, label=f"{name} x after step {i}")


# ------------------------------------------------------------------------------------------------------------------------------------
# 1. fp32 grade of every (case, cap), and of sd_denoiser_forward
# ------------------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("shape,cap", pc.CASE_CAPS, ids=pc.cap_id)
def test_panel_rollout_is_fp32_grade_row_by_row(shape, cap):
    """Four DDIM steps from t = 980 at max_mode = cap: the first and the last noise prediction and x after every step, each within
    4 x (fp32 CPU oracle's error vs fp64) + 1e-7 on the global, the per-trajectory and the per-row figure, status word 0."""
    route = _route(shape, cap)
    assert route == pc.ROUTES[shape][cap]
    _, x_T, ctx = pc.inputs(shape)
    packed, toks, coef = _packed(shape)
    tr, et, status = _sample(packed, ctx, toks, coef, x_T, cap)
    assert status == 0
    _grade_rollout(f"{pc.case_id(shape)} cap {cap} {route}", tr, et, pc.oracles(shape))


@gpu
@pytest.mark.parametrize("shape", pc.CASES, ids=pc.case_id)
def test_denoiser_forward_is_fp32_grade_row_by_row(shape):
    """sd_denoiser_forward (the loop form's fallback; its plan is cap 0): one evaluation, the step token at t = 980 appended to the memory."""
    from soccerdiffusion_amd import ops

    _, x_T, _ = pc.inputs(shape)
    _, eps64, _, eps32 = pc.oracles(shape)
    got = ops.denoiser_forward(_packed(shape)[0], x_T.cuda(), pc.memory(shape).cuda()).cpu()
    assert_fp32_grade(got, eps64[0], eps32[0], factor=FACTOR, floor=FLOOR, label=f"{pc.case_id(shape)} forward {_route(shape, 0)}")


# ------------------------------------------------------------------------------------------------------------------------------------
# 2. the rerun of the guarded call, end to end, and the rescalings on the capped routes
# ------------------------------------------------------------------------------------------------------------------------------------
RERUN_PAIRS = [(p,) for p in pc.PAIRS if p != "memory"] + [tuple(pc.PAIRS)]   # k = -12: what raises SD_STATUS_NONFINITE on mode 3
ALL_K = [-12, -8, -4, 4, 8]
GRADE_K = [-4, 4]


def _rescale_id(v):
    return "+".join(v) if isinstance(v, tuple) and isinstance(v[0], str) else pc.case_id(v) if isinstance(v, tuple) else None


def _one_step(shape):
    """The DDIM coefficients of the step at t = 980 and both oracles' x after it, from rescale_base's (unscaled) noise predictions."""
    from soccerdiffusion_amd import ops

    _, x, _, _, want64, want32 = pc.rescale_base(shape)
    acp, ts = pc.schedule()
    coef = ops.ddim_coefficients(ts, acp, pc.N_SCHEDULE)[:1]
    x64 = ddim_ref.step(want64, ts[0], x.double(), pc.N_SCHEDULE, acp)
    x32 = ddim_ref.step(want32, ts[0], x, pc.N_SCHEDULE, acp)
    assert x64.dtype == torch.float64 and x32.dtype == torch.float32
    return coef, x64, x32


@gpu
@pytest.mark.parametrize("pairs", RERUN_PAIRS, ids=_rescale_id)
@pytest.mark.parametrize("shape", pc.RESCALE_SHAPES, ids=pc.case_id)
def test_rerun_after_the_range_guard_is_fp32_grade(shape, pairs):
    """Producers x 4096 (k = -12): mode 3 overflows fp16 and says so; what ops.ddim_sample_guarded then returns - the rollout repeated at
    max_mode 1, FUSED_FOLD / CHAINS_F32 here - is fp32 grade against the UNSCALED fp64 oracle."""
    from soccerdiffusion_amd import ops

    d, T, Mc, J, L, B = shape
    sd, x, ctx, tok = pc.rescaled(shape, pairs, -12)
    coef, x64, x32 = _one_step(shape)
    packed = ops.pack_denoiser(sd, "cuda", max_len=T)
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    ops.ddim_sample(packed, ctx.cuda(), tok.reshape(1, d).cuda(), coef, x.cuda(), max_mode=3, status=status)
    assert int(status.item()) != 0
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        _, tr = ops.ddim_sample_guarded(packed, ctx.cuda(), tok.reshape(1, d).cuda(), coef, x.cuda(), trace=True)
    assert any("fp32-MFMA" in str(w.message) for w in seen)
    assert_fp32_grade(tr[0].cpu(), x64, x32, factor=FACTOR, floor=FLOOR,
                      label=f"{pc.case_id(shape)} {'+'.join(pairs)} k=-12 guarded rerun {_route(shape, 1)}")


@gpu
@pytest.mark.parametrize("k", ALL_K, ids=lambda k: f"k{k:+d}")
@pytest.mark.parametrize("cap", pc.CAPS, ids=lambda c: f"cap{c}")
@pytest.mark.parametrize("shape", pc.RESCALE_SHAPES, ids=pc.case_id)
def test_power_of_two_rescaling_on_the_capped_routes(shape, cap, k):
    """Every pair rescaled by 2^k, the function unchanged.  Caps 0 and 1 (fp32 MFMA, no fixed activation scale): fp32 grade at every k.
    Cap 2 (F16_ACT_SCALE of csrc/sd_f16x3.h): k = +/-4 is fp32 grade; k = -12, -8, +8 within 1e-4 on all three figures or a non-zero status
    word (the contract of test_power_of_two_rescaling_keeps_fp32_grade_or_says_so)."""
    from soccerdiffusion_amd import ops

    d, T, Mc, J, L, B = shape
    _, _, _, _, want64, want32 = pc.rescale_base(shape)
    sd, x, ctx, tok = pc.rescaled(shape, tuple(pc.PAIRS), k)
    coef, _, _ = _one_step(shape)
    packed = ops.pack_denoiser(sd, "cuda", max_len=T)
    _, et, status = _sample(packed, ctx, tok.reshape(1, d).cuda(), coef, x, cap)
    label = f"{pc.case_id(shape)} every pair k={k:+d} cap {cap} {_route(shape, cap)}"
    if cap < 2 or k in GRADE_K:
        assert status == 0
        assert_fp32_grade(et[0], want64, want32, factor=FACTOR, floor=FLOOR, label=label)
    else:
        e, e32 = errors(et[0], want64), errors(want32, want64)
        print(report(f"{label} status {status}", e, e32))
        assert status != 0 or max(e) < 1e-4, (status, e)


# ------------------------------------------------------------------------------------------------------------------------------------
# 3. a quiet trajectory beside a loud one
# ------------------------------------------------------------------------------------------------------------------------------------
LOUD_SHAPES = [(256, 100, 10, 20, 2, 3), (256, 10, 40, 20, 2, 3)]   # caps 1 / 2: FUSED_FOLD / FUSED_FOLD_F16 and CHAINS_F32 / CHAINS_F16
LOUD_SCALES = {100: (1.0, 100.0, 0.01), 10000: (1.0, 1e4, 1e-4)}


@functools.lru_cache(maxsize=None)
def _loud_case(shape, apart):
    d, T, Mc, J, L, B = shape
    sd = pc.ref.synthetic_state_dict(d, J, L, seed=29 + T + d)
    g = torch.Generator().manual_seed(d + T + Mc)
    x_T = torch.randn(B, T, J, generator=g)
    ctx = torch.randn(B, Mc, d, generator=g) * torch.tensor(LOUD_SCALES[apart])[:, None, None]
    return sd, x_T, ctx, pc.oracle_rollout(sd, ctx, x_T, torch.float64, pc.N_STEPS) + pc.oracle_rollout(sd, ctx, x_T, torch.float32, pc.N_STEPS)


@gpu
@pytest.mark.parametrize("apart", sorted(LOUD_SCALES))
@pytest.mark.parametrize("cap", [1, 2], ids=lambda c: f"cap{c}")
@pytest.mark.parametrize("shape", LOUD_SHAPES, ids=pc.case_id)
def test_quiet_trajectory_beside_a_loud_one(shape, cap, apart):
    """Three trajectories whose context rows are scaled 1, 100 and 1 / 100: EACH of them fp32 grade on its own - graded as a batch the
    maxima over b of the kernel's and of the oracle's error would both be the loud trajectory's, and a quiet one could lose a hundred times
    its own fp32 error unseen.  f16_prepare packs G and V' of ALL trajectories of a layer with one abs-max word, so the quiet one's operands
    sit 2^-13 below the loud one's in the same fp16 planes.  Every line is printed before the first miss is raised.  At 1e4 apart the
    figures are printed, not gated."""
    from soccerdiffusion_amd import ops

    d, T = shape[0], shape[1]
    assert [_route(shape, 1), _route(shape, 2)] == ([pc.FOLD, pc.FOLD16] if T == 100 else [pc.F32, pc.F16])
    sd, x_T, ctx, (x64, eps64, x32, eps32) = _loud_case(shape, apart)
    toks, coef = pc.gpu_tokens(ops, sd, d, pc.N_STEPS)
    tr, et, status = _sample(ops.pack_denoiser(sd, "cuda", max_len=T), ctx, toks, coef, x_T, cap)
    name = f"{pc.case_id(shape)} context 1 | {apart:g} | 1/{apart:g} cap {cap} {_route(shape, cap)}"
    if apart == 100:
        assert status == 0
        missed = []
        for b in range(3):
            one = [[t[b:b + 1] for t in ts] for ts in (x64, eps64, x32, eps32)]
            try:
                _grade_rollout(f"{name} b={b}", tr[:, b:b + 1], et[:, b:b + 1], one)
            except AssertionError as e:
                missed.append(str(e))
        assert not missed, "\n".join(missed)
        return
    for b in range(3):   # recorded only
        print(report(f"{name} status {status} b={b} eps t=980", errors(et[0][b:b + 1], eps64[0][b:b + 1]), errors(eps32[0][b:b + 1], eps64[0][b:b + 1])))
        print(report(f"{name} status {status} b={b} x after step {pc.N_STEPS - 1}", errors(tr[-1][b:b + 1], x64[-1][b:b + 1]),
                     errors(x32[-1][b:b + 1], x64[-1][b:b + 1])))


# ------------------------------------------------------------------------------------------------------------------------------------
# 4. non-finite neighbours
# ------------------------------------------------------------------------------------------------------------------------------------
def _same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def _with_nan(x_T, ctx, bad):
    x, c = x_T.clone(), ctx.clone()
    x[bad] = NAN
    c[bad] = NAN
    return x, c


def _sample_nan(packed, x_T, ctx, bad, toks, coef, cap):
    x, c = _with_nan(x_T, ctx, bad)
    return _sample(packed, c, toks, coef, x, cap)


@gpu
@pytest.mark.parametrize("cap", [1, 2], ids=lambda c: f"cap{c}")
def test_chain_routes_keep_a_trajectory_whose_neighbours_are_nan(cap):
    """CHAINS_F32 / CHAINS_F16, three trajectories of 10 rows in ONE 64-row panel: with every other trajectory NaN (inputs and context),
    each trajectory keeps its bits - the GEMMs are row-local, the attention cores per trajectory - and the call says so in its status."""
    from soccerdiffusion_amd import ops

    shape = (256, 10, 40, 20, 2, 3)
    d, T, Mc, J, L, B = shape
    assert _route(shape, cap) == (pc.F32, pc.F16)[cap - 1]
    sd = pc.ref.synthetic_state_dict(d, J, L, seed=7)
    g = torch.Generator().manual_seed(5)
    x_T, ctx = torch.randn(B, T, J, generator=g), torch.randn(B, Mc, d, generator=g)
    toks, coef = pc.gpu_tokens(ops, sd, d, 2)
    packed = ops.pack_denoiser(sd, "cuda", max_len=T)
    tr0, et0, status = _sample(packed, ctx, toks, coef, x_T, cap)
    assert status == 0 and torch.isfinite(tr0).all()
    for keep in range(B):
        bad = [b for b in range(B) if b != keep]
        tr, et, status = _sample_nan(packed, x_T, ctx, bad, toks, coef, cap)
        assert status != 0
        assert torch.isnan(tr[:, bad]).all()
        assert _same_bits(tr[:, keep], tr0[:, keep]) and _same_bits(et[:, keep], et0[:, keep]), keep


@gpu
@pytest.mark.parametrize("cap", [0, 1], ids=lambda c: f"cap{c}")
def test_fused_routes_keep_the_trajectories_of_other_panels(cap):
    """FUSED / FUSED_FOLD, four trajectories of 100 rows: trajectory 0 (rows 0 .. 99) NaN.  Trajectory 1 shares the panel of rows 64 .. 127
    with it - its masked keys get p = 0, but their V rows still enter the PV MFMA and 0 x NaN = NaN (panel_cross_attention, panel_folded_pv) -
    so nothing is asserted of it; trajectories 2 and 3 (rows 200 .. 399, panels from row 192 on) share no panel with it and keep their bits.
    The status word is non-zero: the guarded callers raise on it."""
    from soccerdiffusion_amd import ops

    shape = (256, 100, 10, 20, 2, 4)
    d, T, Mc, J, L, B = shape
    assert _route(shape, cap) == (pc.FUSED, pc.FOLD)[cap]
    sd = pc.ref.synthetic_state_dict(d, J, L, seed=7)
    g = torch.Generator().manual_seed(11)
    x_T, ctx = torch.randn(B, T, J, generator=g), torch.randn(B, Mc, d, generator=g)
    toks, coef = pc.gpu_tokens(ops, sd, d, 2)
    packed = ops.pack_denoiser(sd, "cuda", max_len=T)
    tr0, et0, status = _sample(packed, ctx, toks, coef, x_T, cap)
    assert status == 0 and torch.isfinite(tr0).all()
    tr, et, status = _sample_nan(packed, x_T, ctx, [0], toks, coef, cap)
    assert status != 0 and torch.isnan(tr[:, 0]).all()
    shared = bool(torch.isnan(tr[:, 1]).any())
    print(f"{pc.case_id(shape)} cap {cap} {_route(shape, cap)}: trajectory 0 NaN; trajectory 1 (shares rows 64 .. 127's panel) "
          f"{'has NaN rows: ' + str(sorted(set(torch.isnan(tr[-1, 1]).any(-1).nonzero().flatten().tolist()))[:3]) + ' ...' if shared else 'stays finite'}")
    for keep in (2, 3):
        assert _same_bits(tr[:, keep], tr0[:, keep]) and _same_bits(et[:, keep], et0[:, keep]), keep
