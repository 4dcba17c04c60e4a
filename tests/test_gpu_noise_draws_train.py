"""Training with several noise draws per window (train_step(draws=K)): the whole step against the fp64 oracle on the EXPANDED context.

C windows are encoded once, C K noisy trajectories are denoised against them; the result has to be, to fp32 grade (tests/parity.py: 4 x the
fp32 CPU oracle's own error + 1e-7), the existing step on ``[c.repeat_interleave(K, 0) for c in context]``: prediction, loss, every parameter
gradient and the gradient into the context (summed over the K draws).  Every gated group prints one line (python -m pytest -s;
profiles/noise_draws_parity.txt is that output)."""

import functools

import pytest
import torch

from oracle import ddim_ref
from oracle import denoiser_ref as ref
from parity import FACTOR, FLOOR, assert_fp32_grade, assert_grads_fp32_grade, assert_loss_fp32_grade, grad_errors, zero_blocks
from test_gpu_reference_configs import BASE, CONFIGS, _state_dict_for
from test_gpu_training import _arm_fused

pytestmark = pytest.mark.gpu

C, K, T, J = 3, 4, 10, 20
STEPS = [980, 3, 500, 40, 999, 0, 250, 750, 10, 600, 333, 123]   # one per trajectory: C K = 12
# (hidden_dim, decoder layers, context rows, shared route expected)
SHAPES = [(128, 2, 12, True), (256, 2, 40, True), (64, 2, 12, True), (512, 2, 12, False)]
# Every figure is held to parity.FACTOR = 4.  The one exception is DESIGN.md section 3's precedent (tests/test_gpu_shipped_shapes_train_grade.py's
# ROUTE_FACTOR): the `row` figure of a 1-D parameter - its rows are single elements - may reach 8 x; every matrix stays at 4 on all three
# figures.  Measured at (256, 2, 40), shared route (profiles/noise_draws_parity.txt): layers.0.self_attn.in_proj_bias 5.05 x (element 728,
# v block; glob 4.6e-07 against 4 * 1.1e-07 + 1e-07), layers.1.norm1.weight 4.36 x (element 124).  The EXISTING step on the same inputs with
# the context expanded by hand shows the same 4.36 x at layers.1.norm1.weight (and its worst row of layer 0 at 4.00 x): the figure belongs
# to the d = 256 row chains at 120 trajectory rows, not to the shared kernels.  The other three shapes are within 4 everywhere.
ROW_FACTOR_1D = {(256, 2, 40): 8.0}


def _params(d, L):
    return {**BASE, **CONFIGS["decoder_only"], "hidden_dim": d, "num_decoder_layers": L, "trajectory_prediction_length": T, "num_joints": J}


@functools.lru_cache(maxsize=None)
def _inputs(d, L, Mc):
    sd = _state_dict_for(_params(d, L))
    g = torch.Generator().manual_seed(4000 + d + Mc)
    x0, eps = torch.randn(C, T, J, generator=g), torch.randn(C * K, T, J, generator=g)
    t = torch.tensor(STEPS)
    x_t = ddim_ref.add_noise(x0.repeat_interleave(K, 0), eps, t, ddim_ref.alphas_cumprod())
    return sd, x_t, t, eps, torch.randn(C, Mc, d, generator=g)


def _oracle(sd, x_t, t, eps, dtype, context=None, input_data=None):
    """(prediction, loss, parameter gradients, context gradient) of the CPU oracle on the context expanded to one copy per draw."""
    if dtype == torch.float64:
        sd = {k: v.double() if v.is_floating_point() else v for k, v in sd.items()}
    leaf = None
    if context is not None:
        leaf = context.detach().clone().to(dtype).requires_grad_()   # (a copy: the cached inputs stay as they are)
        context = [leaf.repeat_interleave(K, 0)]
    pred, loss, grads = ref.train_loss_and_grads(sd, x_t, t, eps, context=context, input_data=input_data, dtype=dtype)
    return pred, loss, grads, None if leaf is None else leaf.grad


@functools.lru_cache(maxsize=None)
def _references(d, L, Mc):
    sd, x_t, t, eps, ctx = _inputs(d, L, Mc)
    return _oracle(sd, x_t, t, eps, torch.float64, ctx), _oracle(sd, x_t, t, eps, torch.float32, ctx)


def _grads_gate(label, grads, g64, g32, row_factor_1d):
    zero = zero_blocks(g64)
    out = assert_grads_fp32_grade(grads, g64, g32, zero=zero, row_factor=row_factor_1d, label=label)
    if row_factor_1d is not None:   # the wider row bound is for 1-D parameters alone
        e32 = grad_errors(g32, g64, zero)
        late = [f"{label}: {k}: 'row' error {out[k].row:.3e} above {FACTOR:g} * {e32[k].row:.3e} + {FLOOR:g} (a matrix: no wider row bound)"
                for k in g64 if g64[k].dim() > 1 and out[k] is not None and not out[k].row <= FACTOR * e32[k].row + FLOOR]
        assert not late, "\n".join(late)


def _gate(label, got, want64, want32, row_factor_1d=None):
    pred, loss, grads, dctx = got
    failures = []
    checks = [lambda: assert_fp32_grade(pred, want64[0], want32[0], label=f"{label} prediction"),
              lambda: assert_loss_fp32_grade(loss, want64[1], want32[1], label=label),
              lambda: _grads_gate(label, grads, want64[2], want32[2], row_factor_1d)]
    if dctx is not None:
        checks.append(lambda: assert_fp32_grade(dctx, want64[3], want32[3], label=f"{label} context gradient"))
    for check in checks:
        try:   # every figure of the case is printed before the first miss is raised
            check()
        except AssertionError as exc:
            failures.append(str(exc))
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("d,L,Mc,shared", SHAPES, ids=lambda v: str(v))
def test_step_with_draws_is_the_step_on_the_expanded_context(d, L, Mc, shared):
    from soccerdiffusion_amd import cli, training

    sd, x_t, t, eps, ctx = _inputs(d, L, Mc)
    m = cli.build_model(_params(d, L)).cuda()
    m.load_state_dict(sd)
    m.set_dropout(0.0)
    m.train()
    _arm_fused(m, True)
    before = (training.SHARED_STACKS[0], training.EXPANDED_CONTEXTS[0], training.TRAJ_LAYERS[0])
    c = ctx.cuda().requires_grad_()
    pred = m.forward_with_context([c], x_t.cuda(), t.cuda(), draws=K)
    after = (training.SHARED_STACKS[0], training.EXPANDED_CONTEXTS[0], training.TRAJ_LAYERS[0])
    assert (after[0] - before[0], after[1] - before[1]) == ((1, 0) if shared else (0, 1))
    assert after[2] == before[2]   # sd_train_layer_fwd owns one trajectory and its memory: not under draws
    loss = training.mse_loss(pred, eps.cuda())
    loss.backward()
    grads = {k: v.grad.detach().cpu() for k, v in m.named_parameters() if v.grad is not None}
    assert tuple(c.grad.shape) == (C, Mc, d)
    _gate(f"draws d{d} L{L} Mc{Mc} {'shared' if shared else 'expanded'}", (pred.detach().cpu(), float(loss.detach()), grads, c.grad.cpu()),
          *_references(d, L, Mc), row_factor_1d=ROW_FACTOR_1D.get((d, L, Mc)))


def test_full_model_encodes_each_window_once():
    """m(input_data, x, t, draws=K): every context encoder sees C rows, not C K, and the step - the encoders' gradients through the
    shared memory included - is the oracle's on K times repeated windows."""
    from soccerdiffusion_amd import cli, training

    params = {**BASE, **CONFIGS["num_joints_22"], "num_joints": J}
    sd = _state_dict_for(params)
    data = cli.synthetic_dataset(C, params, seed=3)
    inp = {k: data[k] for k in cli.CONTEXT_KEYS if k in data}
    g = torch.Generator().manual_seed(77)
    x0, eps = torch.randn(C, T, J, generator=g), torch.randn(C * K, T, J, generator=g)
    t = torch.tensor(STEPS)
    x_t = ddim_ref.add_noise(x0.repeat_interleave(K, 0), eps, t, ddim_ref.alphas_cumprod())
    m = cli.build_model(params).cuda()
    m.load_state_dict(sd)
    m.set_dropout(0.0)
    m.train()
    _arm_fused(m, True)
    seen = {}
    for name in ("action_history_encoder", "joint_states_encoder", "game_state_encoder"):
        getattr(m, name).register_forward_hook(lambda mod, args, out, name=name: seen.setdefault(name, []).append(out.shape[0]))
    shared = training.SHARED_STACKS[0]
    pred = m({k: v.cuda() for k, v in inp.items()}, x_t.cuda(), t.cuda(), draws=K)
    assert seen == {"action_history_encoder": [C], "joint_states_encoder": [C], "game_state_encoder": [C]}
    assert training.SHARED_STACKS[0] == shared + 1
    assert tuple(pred.shape) == (C * K, T, J)
    loss = training.mse_loss(pred, eps.cuda())
    loss.backward()
    grads = {k: v.grad.detach().cpu() for k, v in m.named_parameters() if v.grad is not None}
    rep = {k: v.repeat_interleave(K, 0) for k, v in inp.items()}
    want64, want32 = (_oracle(sd, x_t, t, eps, dt, input_data=rep) for dt in (torch.float64, torch.float32))
    _gate("draws full model d128", (pred.detach().cpu(), float(loss.detach()), grads, None), want64, want32)


# ---- bit-level statements: at a shape where the eager step itself repeats bit for bit (one 32-row slab of trajectory rows, one of each
# memory segment: every fp32 atomic of the step then adds at most two terms; tests/test_gpu_ema.py's set-up) ----
def _tiny(p, draws_c=2, seed=5):
    from test_gpu_ema import _model

    from soccerdiffusion_amd import training
    from soccerdiffusion_amd.scheduler import DDIMScheduler

    d, Tt, Jt, mc = 128, 4, 4, 3
    m, _ = _model(d, Jt, 1, Tt, seed=seed)
    m.train().set_dropout(p, seed=99)
    opt = training.FusedAdamW(m.parameters(), lr=1e-3)
    g = torch.Generator().manual_seed(17)
    x0 = torch.randn(draws_c, Tt, Jt, generator=g).cuda()
    ctx = [torch.randn(draws_c, mc, d, generator=g).cuda()]
    ns = DDIMScheduler(beta_schedule="squaredcos_cap_v2", clip_sample=False)
    sch = torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=1e-3, total_steps=20)
    return m, opt, sch, ns, x0, ctx, torch.Generator(device="cuda").manual_seed(11)


def test_draws_1_is_the_call_without_the_argument():
    from soccerdiffusion_amd import training

    runs = []
    for kw in ({}, {"draws": 1}):
        m, opt, sch, ns, x0, ctx, gen = _tiny(0.1)
        stacks = (training.SHARED_STACKS[0], training.EXPANDED_CONTEXTS[0])
        losses = [float(training.train_step(m, opt, sch, ns, x0, context=ctx, generator=gen, **kw)) for _ in range(3)]
        assert (training.SHARED_STACKS[0], training.EXPANDED_CONTEXTS[0]) == stacks
        runs.append((losses, opt.flat_param.clone(), opt.flat_m.clone(), opt.flat_v.clone()))
    assert runs[0][0] == runs[1][0]
    assert all(torch.equal(a, b) for a, b in zip(runs[0][1:], runs[1][1:]))


def test_graphed_step_with_draws_replays_the_eager_steps_bit_for_bit():
    """Three GraphedTrainStep(draws=4) replays against three eager train_step(draws=4) calls, dropout 0.1, same generator stream.  A
    replay keys its masks by the call index frozen at capture plus the epoch word it uploads (GraphedTrainStep); the eager steps are given
    the same key - call index and epoch word - so that both draw the same masks: what is compared is the captured launches, not the keys."""
    from soccerdiffusion_amd import ops, training

    m, opt, sch, ns, x0, ctx, gen = _tiny(0.1)
    stacks = m.dropout_stacks()
    calls = [s.dropout.calls for s in stacks]
    word = torch.zeros(1, dtype=torch.float32, device="cuda")
    eager = []
    shared = training.SHARED_STACKS[0]
    try:
        ops.set_dropout_epoch(word)
        for k in range(1, 4):
            word.view(torch.int32)[0] = k
            for s, c in zip(stacks, calls):
                s.dropout.calls = c
            eager.append(float(training.train_step(m, opt, sch, ns, x0, context=ctx, generator=gen, draws=4)))
        torch.cuda.synchronize()
    finally:
        ops.set_dropout_epoch(None)
    assert training.SHARED_STACKS[0] == shared + 3
    assert len(set(eager)) == 3

    m2, opt2, sch2, _, _, _, gen2 = _tiny(0.1)
    gs = training.GraphedTrainStep(m2, opt2, sch2, ns, generator=gen2, eager_steps=0, draws=4)
    try:
        replayed = []
        for _ in range(3):
            replayed.append(float(gs(x0, context=ctx)))
            assert gs.graph is not None
    finally:
        gs.close()
    print("eager", eager, "replayed", replayed)
    assert replayed == eager
    assert torch.equal(opt2.flat_param, opt.flat_param) and torch.equal(opt2.flat_m, opt.flat_m) and torch.equal(opt2.flat_v, opt.flat_v)


def test_train_step_validates_draws_and_shapes():
    from soccerdiffusion_amd import training

    m, opt, sch, ns, x0, ctx, gen = _tiny(0.0)
    for bad in (0, -1, 2.0, True, "2"):
        with pytest.raises(ValueError, match="draws"):
            training.train_step(m, opt, sch, ns, x0, context=ctx, generator=gen, draws=bad)
    with pytest.raises(ValueError, match="noise"):
        training.train_step(m, opt, sch, ns, x0, context=ctx, noise=torch.zeros_like(x0), draws=2)
    with pytest.raises(ValueError, match="timesteps"):
        training.train_step(m, opt, sch, ns, x0, context=ctx, timesteps=torch.zeros(2, dtype=torch.int64, device="cuda"), draws=2)
    with pytest.raises(ValueError, match="context shape mismatch"):
        m.forward_with_context([ctx[0][:1]], torch.zeros(4, 4, 4, device="cuda"), torch.zeros(4, dtype=torch.int64, device="cuda"), draws=2)
    assert opt._step == 0


def test_cli_train_noise_draws_writes_and_resumes_the_checkpoint_key(tmp_path, capsys):
    """cli train --noise-draws K in this process: steps per epoch still count windows, the checkpoint gains noise_draws, and -p continues with it."""
    import yaml
    from test_gpu_eval import PARAMS

    from soccerdiffusion_amd import cli, training

    cfg, ckpt, ckpt2 = tmp_path / "cfg.yaml", tmp_path / "a.pth", tmp_path / "b.pth"
    cfg.write_text(yaml.safe_dump(PARAMS))
    ap = cli.build_parser()
    shared = training.SHARED_STACKS[0]
    assert cli.cmd_train(ap.parse_args(["train", "-c", str(cfg), "-o", str(ckpt), "--synthetic", "32", "--noise-draws", "3"])) == 0
    steps = training.SHARED_STACKS[0] - shared
    assert steps == 2   # 32 windows at batch_size 16: two steps, each on 48 trajectories
    saved = torch.load(ckpt, map_location="cpu", weights_only=True)
    assert saved["noise_draws"] == 3 and saved["lr_scheduler_state_dict"]["total_steps"] == 2
    assert cli.cmd_train(ap.parse_args(["train", "-p", str(ckpt), "-o", str(ckpt2), "--synthetic", "32"])) == 0
    assert training.SHARED_STACKS[0] - shared == 4
    assert torch.load(ckpt2, map_location="cpu", weights_only=True)["noise_draws"] == 3
    plain = tmp_path / "c.pth"
    assert cli.cmd_train(ap.parse_args(["train", "-c", str(cfg), "-o", str(plain), "--synthetic", "32"])) == 0
    assert "noise_draws" not in torch.load(plain, map_location="cpu", weights_only=True)
    assert training.SHARED_STACKS[0] - shared == 4


@pytest.mark.parametrize("B", [12, 96, 2048, 97])
def test_step_token_gradient_sums_its_rows_in_a_fixed_order(B):
    """The learned half of the step token under draws: the rows are added level by level in groups of up to 32 (97, a prime: one group) -
    the fp64 column sum to fp32 rounding, and the same bits on every run."""
    from soccerdiffusion_amd import training

    m = _tiny(0.0)[0]
    g = torch.Generator().manual_seed(B)
    steps = torch.randint(0, 1000, (B,), generator=g).cuda()
    dtok = torch.randn(B, 1, 128, generator=g).cuda()
    grads = []
    for _ in range(2):
        m.step_encoding.token.grad = None
        training.step_token_autograd(m.step_encoding, steps, fixed_order=True).backward(dtok)
        grads.append(m.step_encoding.token.grad.detach().clone().reshape(-1))
    assert torch.equal(grads[0], grads[1])
    half = grads[0].numel()
    want = dtok[:, 0, 128 - half :].double().sum(0).cpu()
    assert float((grads[0].double().cpu() - want).norm() / want.norm()) < 1e-6
