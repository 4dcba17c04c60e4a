"""Held-out evaluation on the GPU: the loop form with a group size (sd_sampler_prepare_draws / sd_sampler_eps_draws) against the call on the
repeated context, bit for bit on every route; ops.noise_loss_grid against the fp64 / fp32 oracle; the two kernels of csrc/sd_eval.hip against
tests/eval_ref.py within its derived bounds; evaluation.evaluate end to end; no side effect on a training run; the command line."""

import ctypes as C
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import yaml

import eval_ref
import parity
from conftest import REPO
from test_gpu_draws import CN, HEADS, L, Setup, _inputs

pytestmark = pytest.mark.gpu

# name -> (d, Mc, T, J, max_mode, route)
ROUTES = {
    "tuned": (256, 9, 10, 20, 3, "TRAJ_TUNED"),
    "tuned-2p": (256, 9, 10, 20, 4, "TRAJ_TUNED_2P"),
    "wide": (256, 20, 10, 20, 3, "TRAJ_TUNED_WIDE"),
    "generic128": (128, 30, 10, 20, 3, "TRAJ_GENERIC"),
    "generic512": (512, 5, 10, 20, 3, "TRAJ_GENERIC"),
}
LARGE = (256, 9, 100, 22, 3, "TRAJ_TUNED")   # the largest token-tile count and the ragged joint path
K_DISTINCT = 3


def _tokens(setup, d, B, per_traj):
    """(n_tok, d) step tokens: one, or B of them that repeat K_DISTINCT timesteps (so that the dedup map is used)."""
    from soccerdiffusion_amd import ops

    ts = [980, 437, 0]
    steps = torch.tensor([ts[b % K_DISTINCT] for b in range(B)] if per_traj else [437]).cuda()
    return ops.step_token(steps, ops.step_frequencies(d).cuda(), setup.sd["step_encoding.token"].cuda()).reshape(len(steps), d).contiguous()


def _loop_eps(setup, ctx, x, tokens, mode, draws):
    """(eps, status word) of one ops.LoopSampler evaluation; the sampler must take the shape."""
    from soccerdiffusion_amd import ops

    B, T, _ = x.shape
    ls = ops.LoopSampler(setup.packed, B, T, ctx.shape[1], tokens.shape[0], "cuda", max_mode=mode, draws=draws)
    assert ls.supported and ls.draws == draws
    eps = ls.eps(setup.packed, [ctx], tokens, x, None)
    assert eps is not None and ls.prepares == 1
    torch.cuda.synchronize()
    return eps, (int(ls.status.item()) if ls.status is not None else 0)


def _group_equals_repeated(case, G, per_traj, seed):
    from soccerdiffusion_amd import _lib

    d, Mc, T, J, mode, route = case
    setup = Setup.get(d, J, 3)
    x, ctx, _ = _inputs(seed, CN, G, d, Mc, T, J)
    assert _lib.sampler_route_draws(d, HEADS, T, Mc, J, L, CN * G, G, mode) == route
    tokens = _tokens(setup, d, CN * G, per_traj)
    shared, st_s = _loop_eps(setup, ctx, x, tokens, mode, G)
    repeated, st_r = _loop_eps(setup, ctx.repeat_interleave(G, 0).contiguous(), x, tokens, mode, 1)
    assert shared.shape == x.shape and torch.isfinite(shared).all()
    assert torch.equal(shared, repeated) and st_s == st_r
    e = shared.view(CN, G, T, J)
    assert not torch.equal(e[:, 0], e[:, 1]) and not torch.equal(e[0], e[1])
    return setup, x, ctx, tokens, shared


@pytest.mark.parametrize("per_traj", [False, True], ids=["one-token", "token-per-trajectory"])
@pytest.mark.parametrize("G", [2, 5])
@pytest.mark.parametrize("name", list(ROUTES))
def test_group_equals_repeated_bit_for_bit(name, G, per_traj):
    _group_equals_repeated(ROUTES[name], G, per_traj, 8000 + 10 * list(ROUTES).index(name) + G)


def test_group_largest_horizon_and_ragged_joint_count():
    _group_equals_repeated(LARGE, 2, True, 8100)


def test_group_reads_its_own_context():
    """With the contexts swapped the predictions move with them; the middle context keeps its place (the shared scale words are the same maxima)."""
    d, Mc, T, J, mode, _ = ROUTES["tuned"]
    setup, x, ctx, tokens, a = _group_equals_repeated(ROUTES["tuned"], 2, True, 8200)
    b, _ = _loop_eps(setup, ctx.flip(0).contiguous(), x, tokens, mode, 2)
    a, b = a.view(CN, 2, T, J), b.view(CN, 2, T, J)
    assert not torch.equal(a[0], b[0]) and not torch.equal(a[2], b[2])
    assert torch.equal(a[1], b[1])


def _counted(call):
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


@pytest.mark.parametrize("per_traj", [False, True])
def test_one_draw_through_the_new_entry_points_is_the_old_call(per_traj):
    from soccerdiffusion_amd import _lib, ops

    d, Mc, T, J, mode, _ = ROUTES["tuned"]
    setup = Setup.get(d, J, 3)
    x, ctx, _ = _inputs(8300, CN, 1, d, Mc, T, J)
    tokens = _tokens(setup, d, CN, per_traj)
    n_tok = tokens.shape[0]
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    w = C.byref(setup.packed.struct)
    what = ops.PREPARE_WEIGHTS | ops.PREPARE_CONTEXT
    out = {}
    for name in ("old", "new"):
        ws = ops.workspace(lib.sd_workspace_floats(CN, T, Mc, d, L, n_tok), x.device).clone()
        eps = torch.empty_like(x)
        if name == "old":
            _lib.check(lib.sd_sampler_prepare(w, ctx.data_ptr(), ws.data_ptr(), CN, T, Mc, n_tok, what, mode, st), "sd_sampler_prepare")
            n = _counted(lambda: lib.sd_sampler_eps(w, tokens.data_ptr(), x.data_ptr(), eps.data_ptr(), ws.data_ptr(), CN, T, Mc, n_tok, None, mode, st))
        else:
            _lib.check(lib.sd_sampler_prepare_draws(w, ctx.data_ptr(), ws.data_ptr(), CN, T, Mc, n_tok, what, mode, 1, st), "sd_sampler_prepare_draws")
            n = _counted(lambda: lib.sd_sampler_eps_draws(w, tokens.data_ptr(), x.data_ptr(), eps.data_ptr(), ws.data_ptr(), CN, T, Mc, n_tok, None, mode, 1, st))
        out[name] = (eps, n)
    assert out["old"][1] == out["new"][1] == 1
    assert torch.equal(out["old"][0], out["new"][0]) and torch.isfinite(out["new"][0]).all()


def test_bad_group_sizes_launch_nothing():
    from soccerdiffusion_amd import _lib, ops

    d, Mc, T, J, mode, _ = ROUTES["tuned"]
    setup = Setup.get(d, J, 3)
    B = 6
    x, ctx, _ = _inputs(8400, 3, 2, d, Mc, T, J)
    tokens = _tokens(setup, d, B, True)
    lib = _lib.load()
    ws = ops.workspace(lib.sd_workspace_floats(B, T, Mc, d, L, B), x.device)
    eps = torch.full_like(x, 7.0)
    w, st = C.byref(setup.packed.struct), torch.cuda.current_stream().cuda_stream
    for draws in (0, -1, 4, 5, 7):
        assert lib.sd_sampler_prepare_draws(w, ctx.data_ptr(), ws.data_ptr(), B, T, Mc, B, 3, mode, draws, st) == -1, draws
        assert _counted(lambda: lib.sd_sampler_eps_draws(w, tokens.data_ptr(), x.data_ptr(), eps.data_ptr(), ws.data_ptr(), B, T, Mc, B, None, mode,
                                                         draws, st) + 1) == 0, draws
    torch.cuda.synchronize()
    assert bool((eps == 7.0).all())
    with pytest.raises(ValueError):
        ops.LoopSampler(setup.packed, B, T, Mc, B, "cuda", draws=4)


# ---- ops.noise_loss_grid against the oracle ------------------------------------------------------------------------------------------
def _decoder_model(d, J, T, seed=5):
    from test_gpu_loop_form import _model

    return _model(d, J, L, T, seed=seed)


@pytest.mark.parametrize("d,Mc", [(256, 9), (128, 9)], ids=["tuned-256", "generic-128"])
def test_noise_loss_grid_against_the_oracle(d, Mc):
    from oracle import denoiser_ref as ref
    from soccerdiffusion_amd import ops
    from soccerdiffusion_amd.ml.model import model as mm

    Cn, K, T, J = 2, 3, 10, 20
    m, sd = _decoder_model(d, J, T)
    g = torch.Generator().manual_seed(8500 + d)
    ctx = torch.randn(Cn, Mc, d, generator=g)
    x0n = torch.randn(Cn, T, J, generator=g)
    noise = torch.randn(Cn * K, T, J, generator=g)
    ts = torch.tensor([62, 500, 937])
    loss, eps = ops.noise_loss_grid(m, [ctx.cuda()], x0n.cuda(), noise.cuda(), ts.cuda(), return_eps=True)
    assert loss.shape == (Cn, K) and eps.shape == noise.shape
    ls = list(mm._model_cache(m, "loop").values())
    assert len(ls) == 1 and ls[0].supported and ls[0].draws == K and ls[0].prepares == 1 and ls[0].shape == (Cn * K, T, Mc, Cn * K)
    # the oracle on the device's own noisy inputs (ops.ddim_add_noise is tested elsewhere), the context repeated
    t_all = ts.repeat(Cn)
    x_t = ops.ddim_add_noise(x0n.repeat_interleave(K, 0).cuda().contiguous(), noise.cuda(), t_all.cuda(), ops.alphas_cumprod().cuda()).cpu()
    ctx_rep = ctx.repeat_interleave(K, 0)
    sd64 = {k: v.double() if v.is_floating_point() else v for k, v in sd.items()}
    e64 = ref.forward_with_context(sd64, [ctx_rep.double()], x_t.double(), t_all, dtype=torch.float64)
    e32 = ref.forward_with_context(sd, [ctx_rep], x_t, t_all, dtype=torch.float32)
    l64 = ((e64 - noise.double()) ** 2).mean(dim=(1, 2)).view(Cn, K)
    l32 = ((e32 - noise) ** 2).mean(dim=(1, 2)).view(Cn, K)
    loss = loss.cpu()
    for c in range(Cn):
        for k in range(K):
            parity.assert_loss_fp32_grade(loss[c, k], l64[c, k], l32[c, k], factor=4, floor=1e-7, label=f"noise_loss_grid d={d} window {c} t={int(ts[k])}")


# ---- sd_eval_sqerr_rows ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per", [1, 23, 200, 2200])
@pytest.mark.parametrize("rows", [1, 5])
def test_sqerr_rows(rows, per):
    from soccerdiffusion_amd import ops

    g = torch.Generator().manual_seed(8600 + 7 * rows + per)
    a = torch.randn(rows, per, generator=g) * 3.0
    b = a + torch.randn(rows, per, generator=g) * (10.0 ** torch.randint(-3, 1, (rows, 1), generator=g).float())
    got = ops.sqerr_rows(a.cuda(), b.cuda())
    again = ops.sqerr_rows(a.cuda(), b.cuda())
    assert got.shape == (rows,) and torch.equal(got, again)
    want, bound = eval_ref.sqerr_rows(a, b)
    err = np.abs(got.cpu().double().numpy() - want)
    print(f"sqerr_rows rows={rows} per={per}: max error / bound {float((err / bound).max()):.3f}")
    assert (want > 0).all() and (err <= bound).all(), (err, bound)


# ---- sd_eval_trajectory_errors -------------------------------------------------------------------------------------------------------
def _check_errors(x, target, mean, std, G, angular):
    """The four outputs against fp64 within eval_ref's bounds; returns (device outputs, references)."""
    from soccerdiffusion_amd import ops

    dev = [t.cuda() for t in (x, target, mean, std)]
    got = ops.trajectory_errors(*dev, draws=G, angular=angular)
    again = ops.trajectory_errors(*dev, draws=G, angular=angular)
    assert all(torch.equal(a, b) for a, b in zip(got, again))
    want = eval_ref.trajectory_errors(x, target, mean, std, G, angular)
    Cn, T, J = target.shape
    for name, t, shape in (("err", got[0], (Cn, G)), ("row_err", got[1], (Cn, G, T)), ("joint_err", got[2], (Cn, G, J))):
        assert tuple(t.shape) == shape
        ref, bound = want[name]
        err = np.abs(t.cpu().double().numpy() - ref)
        assert (err <= bound).all(), (name, float((err / np.maximum(bound, 1e-300)).max()))
    assert got[3].dtype == torch.int32 and tuple(got[3].shape) == (Cn,)
    return got, want


@pytest.mark.parametrize("J", [1, 20, 23])
@pytest.mark.parametrize("T", [1, 10, 17])
@pytest.mark.parametrize("Cn,G", [(1, 1), (3, 2), (3, 5), (1, 64)])
def test_trajectory_errors(Cn, G, T, J):
    g = torch.Generator().manual_seed(8700 + 1000 * Cn + 100 * G + 10 * T + J)
    mean = math.pi + 0.3 * torch.randn(J, generator=g)
    std = 0.2 + torch.rand(J, generator=g)
    target = torch.rand(Cn, T, J, generator=g) * 2 * math.pi                     # radians in [0, 2 pi)
    # draw g of a window lies 0.05 (g + 1) sigma off the target plus a draw-specific offset well above the bounds, so that best is decided
    offs = torch.randperm(G, generator=g).float().view(1, G, 1, 1) * 0.02 + 0.01
    x = ((target[:, None] - mean) / std) + offs / std + 0.001 * torch.randn(Cn, G, T, J, generator=g)
    for angular in (True, False):
        got, want = _check_errors(x.reshape(Cn * G, T, J), target, mean, std, G, angular)
        ref, bound = want["err"]
        order = np.sort(ref, axis=1)
        if G > 1:   # the runner-up exceeds the winner by more than the sum of both bounds: the choice is decided, the case cannot go soft
            assert (order[:, 1] - order[:, 0] > 2 * bound.max(axis=1)).all()
        assert np.array_equal(got[3].cpu().numpy(), want["best"])


def test_trajectory_errors_wrap_cases():
    """Differences placed by hand, once modulo 2 pi and once not."""
    d = torch.tensor([0.0, math.pi - 0.01, -(math.pi - 0.01), math.pi + 0.01, -(math.pi + 0.01), 2 * math.pi - 0.01, -(2 * math.pi - 0.01),
                      3 * math.pi, -3 * math.pi], dtype=torch.float64)
    J = len(d)
    mean, std = torch.zeros(J), torch.ones(J)
    target = torch.full((1, 2, J), 1.0)
    x = (target.double() + d.view(1, 1, J)).float()
    wrapped = [0.0, math.pi - 0.01, math.pi - 0.01, math.pi - 0.01, math.pi - 0.01, 0.01, 0.01, math.pi, math.pi]
    for angular, want in ((True, wrapped), (False, d.abs().tolist())):
        got, _ = _check_errors(x, target, mean, std, 1, angular)
        joint = got[2].cpu().view(J)
        for j in range(J):   # (x is rounded to fp32 around 1 + d: 2^-22 absolute)
            assert abs(math.sqrt(float(joint[j])) - want[j]) < 4e-6, (angular, j, float(joint[j]), want[j])


def test_trajectory_errors_ties_go_to_the_lower_index():
    from soccerdiffusion_amd import ops

    g = torch.Generator().manual_seed(8800)
    Cn, G, T, J = 2, 4, 10, 20
    mean, std = math.pi + torch.zeros(J), torch.ones(J)
    target = torch.rand(Cn, T, J, generator=g) * 2 * math.pi
    x = torch.randn(Cn, G, T, J, generator=g) * 0.5 + (target[:, None] - mean)
    x[0, 3] = (target[0] - mean) + 0.001      # the winner of window 0 ...
    x[0, 1] = x[0, 3]                         # ... twice, bit for bit: the lower index is chosen
    x[1, 2] = (target[1] - mean) + 0.001
    err, _, _, best = ops.trajectory_errors(x.cuda(), target.cuda(), mean.cuda(), std.cuda(), draws=G)
    assert float(err[0, 1]) == float(err[0, 3]) and best.tolist() == [1, 2]


# ---- evaluation.evaluate ---------------------------------------------------------------------------------------------------------------
PARAMS = dict(hidden_dim=256, action_context_length=20, trajectory_prediction_length=10, epochs=1, batch_size=16, lr=1e-3,
              train_denoising_timesteps=1000, image_context_length=0, imu_context_length=20, num_imu_encoder_layers=1,
              joint_state_context_length=20, num_normalization_samples=30, num_joints=20, use_action_history=True,
              num_action_history_encoder_layers=1, use_imu=True, imu_orientation_embedding_method="quaternion",
              use_joint_states=True, joint_state_encoder_layers=1, use_images=False, image_sequence_encoder_type="transformer",
              image_encoder_type="resnet18", num_image_sequence_encoder_layers=1, num_decoder_layers=2,
              distill_teacher_inference_steps=3, use_gamestate=True, encoder_patch_size=5)


def _tiny_model_and_source(n=6):
    from soccerdiffusion_amd import cli
    from soccerdiffusion_amd.dataset import fit_normalizer

    torch.manual_seed(3)
    data = cli.synthetic_dataset(n, PARAMS, seed=1)
    m = cli.build_model(PARAMS).cuda().eval()
    mean, std = fit_normalizer(data["joint_command"])
    m.mean.copy_(mean)
    m.std.copy_(std)
    return m, cli.DataSource(tensors=data, device="cuda")


def _close(got, want, rel, label):
    assert abs(got - want) <= rel * abs(want) + 1e-12, (label, got, want, rel)


def test_evaluate_end_to_end():
    from soccerdiffusion_amd import evaluation

    m, source = _tiny_model_and_source(6)
    kw = dict(steps=3, draws=3, grid=2, batch=4, seed=11)          # two batches: 4 + 2 windows
    state = torch.cuda.get_rng_state()
    cpu_state = torch.get_rng_state()
    keep = []
    report = evaluation.evaluate(m, source, torch.arange(6), keep=keep, **kw)
    assert torch.equal(torch.cuda.get_rng_state(), state) and torch.equal(torch.get_rng_state(), cpu_state)   # nobody else's generator moved
    assert evaluation.evaluate(m, source, torch.arange(6), **kw) == report
    assert report["n_windows"] == 6 and [t for t, _ in report["val_loss_by_t"]] == [250, 750] and len(keep) == 2
    assert (report["steps"], report["draws"], report["max_mode"], report["angular"]) == (3, 3, 3, True)
    assert len(report["rmse_by_row"]) == 10 and len(report["rmse_by_joint"]) == 20
    assert json.loads(json.dumps(report)) == report
    # the reference report from the device's own samples and predictions, and how far an fp32 evaluation may be from it
    want = eval_ref.report(keep, timesteps=[250, 750], steps=3, draws=3, max_mode=3, angular=True, mean=m.mean, std=m.std)
    from soccerdiffusion_amd import ops

    rel = rel_loss = 0.0
    for p in keep:
        e = eval_ref.trajectory_errors(p["x"], p["target"], m.mean, m.std, 3, True)
        rel = max([rel] + [float((e[k][1] / e[k][0]).max()) for k in ("err", "row_err", "joint_err")])
        lref, lbound = eval_ref.sqerr_rows(p["eps"], p["noise"])
        rel_loss = max(rel_loss, float((lbound / lref).max()))
        # the spread: the same kernel against the denormalised medoid, nothing wrapped
        med = ops.normalize(p["medoid_x"], m.mean, m.std, inverse=True)
        s = eval_ref.trajectory_errors(p["x"], med, m.mean, m.std, 3, False)["err"]
        assert (np.abs(p["spread"].cpu().double().numpy() - s[0]) <= s[1]).all()
    assert rel < 1e-3 and rel_loss < 1e-3
    for key in ("rmse_first_draw", "rmse_medoid", "rmse_best_of_G"):
        _close(report[key], want[key], rel, key)
    for key in ("rmse_by_row", "rmse_by_joint"):
        for a, b in zip(report[key], want[key]):
            _close(a, b, rel, key)
    _close(report["val_loss"], want["val_loss"], rel_loss, "val_loss")
    for (t, a), (_, b) in zip(report["val_loss_by_t"], want["val_loss_by_t"]):
        _close(a, b, rel_loss, f"val_loss at {t}")
    _close(report["spread"], want["spread"], 1e-3, "spread")
    assert report["rmse_best_of_G"] <= min(report["rmse_medoid"], report["rmse_first_draw"]) and report["spread"] > 0
    # another seed: other draws
    assert evaluation.evaluate(m, source, torch.arange(6), **dict(kw, seed=12))["rmse_first_draw"] != report["rmse_first_draw"]
    with pytest.raises(RuntimeError):
        evaluation.evaluate(m.train(), source, torch.arange(6), **kw)
    m.eval()
    # a distilled decoder: one forward at t = 0, no noise prediction to score
    r = evaluation.evaluate(m, source, torch.arange(6), distilled=True, **kw)
    assert r["val_loss"] is None and r["val_loss_by_t"] is None
    assert all(math.isfinite(r[k]) for k in ("rmse_first_draw", "rmse_medoid", "rmse_best_of_G", "spread"))


def test_evaluate_leaves_a_training_run_alone():
    """Three steps of a graph-replayed training step (dropout 0.1, EMA on), an evaluation of the last iterate and of the average after each:
    parameters, moments and the average end bit-equal to the same three steps without evaluation.
    The training batch is two windows: the step token's gradient is summed over the batch with float atomics (sd_op_colsum), whose order
    is fixed only up to two rows - with 8 rows two runs of these steps WITHOUT any evaluation differ in about 70 of the 128 moment values
    of step_encoding.token (and nowhere else).  The premise - the plain run repeats bit for bit - is asserted first."""
    from soccerdiffusion_amd import cli, evaluation, training
    from soccerdiffusion_amd.scheduler import DDIMScheduler

    d, J, T, B, Mc = 256, 20, 10, 2, 10
    g = torch.Generator().manual_seed(8900)
    x0 = torch.randn(B, T, J, generator=g).cuda()
    ctx = [torch.randn(B, Mc, d, generator=g).cuda()]
    source = cli.DataSource(tensors={"joint_command": math.pi + torch.randn(6, T, J, generator=g)}, device="cuda")

    def run(with_evaluation):
        m, _ = _decoder_model(d, J, T, seed=9)
        m.train().set_dropout(0.1, seed=77)
        opt = training.FusedAdamW(m.parameters(), lr=1e-3, ema_decay=0.9)
        sch = torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=1e-3, total_steps=10)
        ns = DDIMScheduler(beta_schedule="squaredcos_cap_v2", clip_sample=False)
        gen = torch.Generator(device="cuda").manual_seed(21)
        gs = training.GraphedTrainStep(m, opt, sch, ns, generator=gen, eager_steps=1)
        reports = []
        try:
            for k in range(3):
                assert torch.isfinite(gs(x0, context=ctx)).all()
                assert (gs.graph is not None) == (k >= 1)
                if with_evaluation:
                    m.eval()
                    reports.append(evaluation.evaluate(m, source, torch.arange(6), steps=2, draws=2, grid=2, seed=5))
                    with opt.ema_weights():
                        reports.append(evaluation.evaluate(m, source, torch.arange(6), steps=2, draws=2, grid=2, seed=5))
                    m.train()
                    assert m.diffusion_action_generator.dropout.p == pytest.approx(0.1)
            torch.cuda.synchronize()
        finally:
            gs.close()
        return opt.flat_param.clone(), opt.flat_ema.clone(), {"exp_avg": opt.flat_m.clone(), "exp_avg_sq": opt.flat_v.clone()}, reports

    p0, e0, s0, _ = run(False)
    p2, e2, s2, _ = run(False)
    assert torch.equal(p0, p2) and torch.equal(e0, e2) and all(torch.equal(s0[k], s2[k]) for k in s0)   # the premise
    p1, e1, s1, reports = run(True)
    for k in s0:
        print(f"{k}: differing {int((s0[k] != s1[k]).sum())} of {s0[k].numel()}")
    assert torch.equal(p0, p1) and torch.equal(e0, e1) and all(torch.equal(s0[k], s1[k]) for k in s0)
    assert not torch.equal(p0, e0) and float(s0["exp_avg_sq"].max()) > 0
    assert len(reports) == 6 and reports[0] != reports[1] and reports[0]["val_loss"] != reports[2]["val_loss"]   # the weights it read did move


# ---- the command line ------------------------------------------------------------------------------------------------------------------
def _run(*argv):
    env = dict(os.environ, PYTHONPATH=REPO)
    return subprocess.run([sys.executable, "-m", "soccerdiffusion_amd.cli", *argv], cwd=REPO, env=env, capture_output=True, text=True)


def test_train_with_validation_then_evaluate(tmp_path):
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text(yaml.safe_dump(PARAMS))
    ckpt = tmp_path / "model.pth"
    r = _run("train", "-c", str(cfg), "-o", str(ckpt), "--synthetic", "40", "--val-fraction", "0.25", "--val-steps", "3", "--val-draws", "2",
             "--ema-decay", "0.9")
    assert r.returncode == 0, r.stderr[-2000:]
    assert any("validation on 10 windows" in line for line in r.stdout.splitlines()), r.stdout
    back = torch.load(ckpt, weights_only=True)
    val = back["validation"]
    assert back["hyperparams"] == PARAMS
    assert (val["fraction"], val["split"], val["seed"], val["n_val"]) == (0.25, "tail", 0, 10) and len(val["history"]) == 1
    last = val["history"][-1]
    assert last["epoch"] == 0 and last["last"]["n_windows"] == 10 and last["last"]["draws"] == 2 and last["ema"] != last["last"]
    for flags, key in (((), "last"), (("--ema",), "ema")):
        out = tmp_path / f"report_{key}.json"
        r = _run("evaluate", str(ckpt), "--synthetic", "40", "--steps", "3", "--draws", "2", "-o", str(out), *flags)
        assert r.returncode == 0, r.stderr[-2000:]
        report = json.loads(r.stdout.strip().splitlines()[-1])
        assert report == json.loads(out.read_text()) == last[key], key
