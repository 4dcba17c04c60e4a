"""The context encoders' inference route (sd_encoder_forward: patch_embed_kernel / patch_embed_bigk_kernel, panel_gemm16_kernel,
attention_kernel / attention_pipe_kernel<16 | 32 | 64 | 128>, chain_b_kernel in csrc/sd_kernels.hip) held to the row-by-row fp32 grade of
tests/parity.py: the error against an fp64 oracle, global, per sample and per token, at most parity.FACTOR = 4 x the error the fp32 CPU
oracle itself makes on the same inputs, + 1e-7.  The gates before this file were one L2 norm per tensor below 1e-4 - 300 to 700 x the fp32
oracle's own error at these shapes - at batches of 2 to 5, which never reach attention_pipe_kernel (64 samples and more).

Cases, inputs and oracles: tests/encoder_cases.py; the kernel each case names is pinned on the CPU by tests/test_cpu_encoder_grade.py.
    1. the attention op on both kernels at every head dim, and lse2 (the attention backward's input)
    2. sd_encoder_forward at the shipped encoders' shapes at 1, 3, 63, 64 and 65 samples; batch and scratch independence bit for bit;
       power-of-two rescaling of the layers
    3. patch_embed on each of its paths, row counts around the rows of a workgroup
    4. the model route at 64 robots: encode_input_data, the memory's order, a hidden_dim-512 image model, a PolicySession tick
The measured figures of a run: profiles/encoder_parity.txt (python -m pytest -s)."""

import math

import pytest
import torch

import encoder_cases as ec
import parity
from oracle import denoiser_ref as ref
from parity import assert_fp32_grade

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    from soccerdiffusion_amd import ops as o

    return o


def _bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ------------------------------------------------------------------------------------------------------------------------------------
# 1. the attention op
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ec.ATTENTION_CASES, ids=ec.attention_id)
def test_attention_is_fp32_grade_row_by_row(ops, case):
    """ops.attention against ref.attention in fp64, the yardstick ref.attention in fp32: global, per sample (one sample of every batch is at
    1e-3 of the others) and per query row.  At (Tq, S) = (1, 1) the output is v itself: the fp32 oracle's error is 0 and the bound is the
    floor 1e-7 alone - the kernels' arithmetic there is v * exp2(0) * (1 / 1), expected exact."""
    from soccerdiffusion_amd import _lib

    B, d, heads, tq, s, spike, kernel = case
    assert _lib.attention_route(B, tq, s) == kernel
    q, k, v = ec.attention_inputs(case)
    want64, want32 = ec.attention_oracles(case)
    got = ops.attention(q.cuda(), k.cuda(), v.cuda(), heads)
    assert_fp32_grade(got, want64, want32, label=f"{kernel}<{d // heads}> {ec.attention_id(case)}")


@pytest.mark.parametrize("case", ec.LSE_CASES, ids=ec.attention_id)
def test_attention_lse2_against_fp64(ops, case):
    """lse2 (B, heads, Tq) of ops.attention_lse without dropout - what the attention backward recomputes its probabilities from - against
    log2(e) * logsumexp(scores / sqrt(hd)) in fp64: at most 4 x the largest absolute error of the same expression in fp32 torch, plus one
    fp32 ulp at the largest |lse2| of the case.  `out` of the same call is graded like ops.attention's."""
    from soccerdiffusion_amd import _lib

    B, d, heads, tq, s, _, kernel = case
    assert _lib.attention_route(B, tq, s) == kernel
    q, k, v = ec.attention_inputs(case)
    want64, want32 = ec.attention_oracles(case)
    out, lse = ops.attention_lse(q.cuda(), k.cuda(), v.cuda(), heads)
    label = f"{kernel}<{d // heads}> lse {ec.attention_id(case)}"
    assert_fp32_grade(out, want64, want32, label=label)
    lse64 = ec.lse2_reference(q.double(), k.double(), heads)
    e32 = float((ec.lse2_reference(q, k, heads).double() - lse64).abs().max())
    e = (lse.cpu().double() - lse64).abs()
    e = float(torch.where(torch.isfinite(e), e, torch.full_like(e, float("inf"))).max())
    bound = parity.FACTOR * e32 + 2.0 ** -23 * float(lse64.abs().max())
    print(f"{label:58s} lse2 max abs err {e:8.2e}  fp32 {e32:8.2e}  bound {bound:8.2e}  max |lse2| {float(lse64.abs().max()):.3g}")
    assert tuple(lse.shape) == (B, heads, tq) and e <= bound, (e, bound)


# ------------------------------------------------------------------------------------------------------------------------------------
# 2. sd_encoder_forward
# ------------------------------------------------------------------------------------------------------------------------------------
def _packed(ops, case, sd=None):
    _, d, C, p, S, L, heads, B, _ = case
    return ops.pack_encoder(ec.encoder_weights(d, C, p, L) if sd is None else sd, "cuda", ec.PREFIX, heads=heads, max_len=S // p)


@pytest.mark.parametrize("case", ec.ENCODER_CASES, ids=ec.encoder_id)
def test_encoder_forward_is_fp32_grade_token_by_token(ops, case):
    """ops.encoder_forward against ref.encoder_forward in fp64 / fp32, (B, n, d) as parity.errors' (B, T, J): global, per robot - one stands
    still, one has the zero rings of a reset, one is at 1e-3 - and per token.  Factor 4 everywhere (measured figures and their history:
    profiles/encoder_parity.txt)."""
    _, d, C, p, S, L, heads, B, kernel = case
    want64, want32 = ec.encoder_oracles(case)
    got = ops.encoder_forward(_packed(ops, case), ec.encoder_input(C, S, B).cuda())
    assert_fp32_grade(got, want64, want32, label=f"{ec.encoder_id(case)} {kernel}<{d // heads}>")


@pytest.mark.parametrize("case", ec.PROPERTY_CASES, ids=ec.encoder_id)
def test_encoder_tokens_of_a_robot_do_not_depend_on_the_others(ops, case):
    """Every robot but one replaced by NaN, twice (a robot inside the batch, whose rows share 64-row panels with both neighbours at
    n = 100, and the last one): the remaining robot's tokens are finite and bit for bit those of the clean call - a key row or an LDS row
    read across a sample boundary turns up as NaN."""
    _, d, C, p, S, L, heads, B, _ = case
    packed, x = _packed(ops, case), ec.encoder_input(C, S, B).cuda()
    clean = ops.encoder_forward(packed, x)
    assert torch.isfinite(clean).all()
    for keep in (B // 2, B - 1):
        xn = torch.full_like(x, float("nan"))
        xn[keep] = x[keep]
        got = ops.encoder_forward(packed, xn)
        assert torch.isfinite(got[keep]).all() and _bits_equal(got[keep], clean[keep]), keep
        others = [b for b in range(B) if b != keep]
        assert torch.isnan(got[others]).any(dim=-1).all()   # (the NaN did reach the other robots' tokens)


@pytest.mark.parametrize("case", ec.PROPERTY_CASES, ids=ec.encoder_id)
def test_encoder_result_does_not_depend_on_its_scratch(ops, case):
    """ops.workspace(...) - the cached buffer the call receives - filled with NaN before the call: the same bits."""
    from soccerdiffusion_amd import _lib

    _, d, C, p, S, L, heads, B, _ = case
    packed, x = _packed(ops, case), ec.encoder_input(C, S, B).cuda()
    clean = ops.encoder_forward(packed, x).clone()
    ws = ops.workspace(_lib.load().sd_workspace_floats(B, S // p, 1, d, 1, 0), x.device)
    ws.fill_(float("nan"))
    got = ops.encoder_forward(packed, x)
    assert ops.workspace(1, x.device) is ws       # the call did receive this buffer
    assert torch.isfinite(got).all() and _bits_equal(got, clean)


@pytest.mark.parametrize("k", ec.RESCALE_K)
@pytest.mark.parametrize("case", ec.PROPERTY_CASES, ids=ec.encoder_id)
def test_power_of_two_rescaling_of_the_layers_keeps_fp32_grade(ops, case, k):
    """Section 4 of tests/test_gpu_shipped_shapes_grade.py for an encoder layer: LayerNorm outputs and attention values 2^k away from where
    they were, the function unchanged (tests/test_cpu_encoder_grade.py: the fp32 oracle keeps its bits, every GEMM weight below 256).
    panel_gemm16_kernel scales its activations per row and chain_b_kernel is fp32: the grade holds at every k - there is no status word on
    this path to excuse a miss."""
    _, d, C, p, S, L, heads, B, kernel = case
    want64, want32 = ec.encoder_oracles(case)
    sd = ec.rescaled_weights(ec.encoder_weights(d, C, p, L), L, k)
    assert ec.largest_gemm_weight(sd) < ec.W_LIMIT
    got = ops.encoder_forward(_packed(ops, case, sd), ec.encoder_input(C, S, B).cuda())
    assert_fp32_grade(got, want64, want32, label=f"{ec.encoder_id(case)} k={k:+d}")


# ------------------------------------------------------------------------------------------------------------------------------------
# 3. patch_embed
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ec.PATCH_CASES, ids=ec.patch_id)
def test_patch_embed_is_fp32_grade_row_by_row(ops, case):
    """ops.patch_embed against the patch GEMM + bias + positional rows in fp64, the yardstick the same expression in fp32."""
    d, C, p, B, S, path = case
    assert ec.patch_embed_path(C * p, d) == path
    x, w, b, pe = ec.patch_inputs(case)
    got = ops.patch_embed(x.cuda(), (w if p > 1 else w.reshape(d, C)).cuda(), b.cuda(), pe.cuda())
    assert_fp32_grade(got, ec.patch_oracle(case, torch.float64), ec.patch_oracle(case, torch.float32),
                      label=f"patch_embed {ec.patch_id(case)} [{path}]")


# ------------------------------------------------------------------------------------------------------------------------------------
# 4. the model route at 64 robots
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def default_model():
    """default.yaml's shape without images (tests/test_gpu_reference_configs.py), synthetic weights."""
    from test_gpu_reference_configs import BASE, CONFIGS, _state_dict_for

    from soccerdiffusion_amd import cli

    params = {**BASE, **CONFIGS["default"]}
    sd = _state_dict_for(params)
    model = cli.build_model(params).cuda().eval()
    model.load_state_dict(sd)
    return model, sd, params


def _grade_context(got, sd, inputs, label):
    """Every tensor of a context list against ref.encode_input_data in fp64 / fp32; the game-state token is the table row bit for bit."""
    want64, want32 = ref.encode_input_data(sd, inputs, torch.float64), ref.encode_input_data(sd, inputs, torch.float32)
    names = [n for n, key in (("action_history", "action_history_encoder"), ("imu", "imu_encoder"), ("joint_states", "joint_states_encoder"),
                              ("game_state", "game_state_encoder")) if key + ".embedding.weight" in sd]
    assert len(got) == len(want64) == len(names)
    for name, a, w64, w32 in zip(names, got, want64, want32):
        if name == "game_state":
            assert _bits_equal(a.cpu(), w32)
        else:
            assert_fp32_grade(a, w64, w32, label=f"{label} {name}")
    return want64, want32


def test_encode_input_data_at_64_robots_is_fp32_grade(default_model):
    """cli.build_model for default.yaml at B = 64: every tensor of model.encode_input_data graded, the game-state token bitwise the table row,
    and the memory forward_with_context assembles - context tensors in the oracle's order, the step token last - graded as one tensor."""
    from soccerdiffusion_amd import cli

    model, sd, params = default_model
    B, d = 64, params["hidden_dim"]
    data = cli.synthetic_dataset(B, params, seed=5)
    inp = {k: data[k] for k in cli.CONTEXT_KEYS if k in data}
    with torch.no_grad():
        ctx = model.encode_input_data({k: v.cuda() for k, v in inp.items()})
        want64, want32 = _grade_context(ctx, sd, inp, "default.yaml B=64")
        steps = torch.full((B,), 980, dtype=torch.int64)
        memory = model._assemble_memory(ctx, steps.cuda(), B, ctx[0].device)
    tok = ref.step_token(steps, sd["step_encoding.token"].float(), d)
    assert tuple(memory.shape) == (B, 301 + 1, d)
    assert_fp32_grade(memory, torch.cat(want64 + [tok.double()], 1), torch.cat(want32 + [tok], 1), label="default.yaml B=64 memory")
    assert _bits_equal(memory[:, 300].cpu(), sd["game_state_encoder.embedding.weight"][inp["game_state"]])


def _image_model_512():
    from soccerdiffusion_amd.ml.model.encoder.image import ImageEncoderType, SequenceEncoderType
    from soccerdiffusion_amd.ml.model.model import End2EndDiffusionTransformer

    torch.manual_seed(0)
    return End2EndDiffusionTransformer(
        num_joints=20, hidden_dim=512, use_action_history=True, num_action_history_encoder_layers=1,
        max_action_context_length=20, use_imu=False, imu_orientation_embedding_method="quaternion",
        num_imu_encoder_layers=1, imu_context_length=20, use_joint_states=False, joint_state_encoder_layers=1,
        joint_state_context_length=20, use_images=True, image_encoder_type=ImageEncoderType.RESNET18,
        image_sequence_encoder_type=SequenceEncoderType("transformer"), num_image_sequence_encoder_layers=1,
        image_context_length=10, image_use_final_avgpool=True, image_resolution=64, use_gamestate=True,
        num_decoder_layers=2, trajectory_prediction_length=12, encoder_patch_size=4).to("cuda")


def test_image_model_at_hidden_dim_512_encodes_and_trains_its_token_embedding():
    """larger_model.yaml's image path (hidden_dim 512, use_images: True): the image-sequence encoder is BaseEncoder(input_dim = 512,
    patch 1, 8 heads), its embedding a patch GEMM with K = 512 - more than patch_embed_kernel stages whole (it used to return SD_E_TOOBIG:
    no image model at hidden_dim 512 ran at all).  encode_input_data runs; the sequence encoder's tokens are graded against
    ref.encoder_forward(heads = 8) on the GPU backbone's own tokens (tests/test_gpu_image_path.py's construction at fp32 grade); and one
    forward + backward of the 512-wide token embedding through training._PatchEmbed against fp64 autograd."""
    from soccerdiffusion_amd.training import _PatchEmbed

    m = _image_model_512().eval()
    enc = m.image_sequence_encoder
    B, F, R, d = 2, 10, 64, 512
    g = torch.Generator().manual_seed(2)
    data = {"joint_command_history": torch.randn(B, 20, 20, generator=g).cuda(), "image_data": torch.rand(B, F, 3, R, R, generator=g).cuda(),
            "game_state": torch.randint(0, 4, (B,), generator=g).cuda()}
    with torch.no_grad():
        ctx = m.encode_input_data(data)
        assert [tuple(c.shape) for c in ctx] == [(B, 5, d), (B, F, d), (B, 1, d)] and all(torch.isfinite(c).all() for c in ctx)
        tokens = enc.image_encoder(data["image_data"])
        got = enc(data["image_data"])
    sd = {k: v.detach().cpu() for k, v in enc.transformer_encoder.state_dict().items()}
    want64 = ref.encoder_forward(sd, tokens.cpu(), "", torch.float64, heads=8)
    want32 = ref.encoder_forward(sd, tokens.cpu(), "", torch.float32, heads=8)
    assert_fp32_grade(got, want64, want32, label="image model d=512: sequence encoder tokens")
    # training: the same entry point (ops.patch_embed) and its backward, at tests/test_gpu_image_path.py's sizes, K = d = 512
    g = torch.Generator().manual_seed(5)
    Bt, S = 3, 7
    x = torch.randn(Bt, S, d, generator=g)
    W = torch.randn(d, d, 1, generator=g) / math.sqrt(d)
    b = torch.randn(d, generator=g)
    pe = torch.randn(S, d, generator=g)
    dy = torch.randn(Bt, S, d, generator=g)
    xg, Wg, bg = (t.cuda().requires_grad_() for t in (x, W, b))
    y = _PatchEmbed.apply(xg, Wg, bg, pe.cuda())
    y.backward(dy.cuda())
    grads = {}
    for dt in (torch.float64, torch.float32):
        x2, W2, b2 = (t.to(dt).requires_grad_() for t in (x, W, b))
        y2 = torch.nn.functional.conv1d(x2.transpose(1, 2), W2, b2).transpose(1, 2) + pe.to(dt)
        y2.backward(dy.to(dt))
        grads[dt] = (y2.detach(), x2.grad, W2.grad.view(1, d, d), b2.grad.view(1, 1, d))
    for name, a, w64, w32 in zip(("forward", "dX", "dW", "db"), (y.detach(), xg.grad, Wg.grad.view(1, d, d), bg.grad.view(1, 1, d)),
                                 grads[torch.float64], grads[torch.float32]):
        assert_fp32_grade(a, w64, w32, label=f"_PatchEmbed K=512 {name}")


def test_policy_session_tick_at_64_robots_against_three_at_a_time(default_model):
    """One PolicySession tick of default.yaml without images at 64 robots, and the same tick - a second session with the same pushes -
    with the robots taken three at a time (robots=): the context tokens of both are graded against the oracle on the session's own
    windows, and every robot's published trajectory of both is within the session tests' 1e-4 of the fp32 oracle's rollout
    (tests/test_gpu_session.py), per robot.  The 64-robot tick runs attention_pipe_kernel, the three-robot ticks attention_kernel."""
    import numpy as np

    from oracle import ddim_ref
    from soccerdiffusion_amd.session import PolicySession

    model, sd, params = default_model
    B, T, J, n_steps = 64, 10, 20, 4
    full = PolicySession(model, num_inference_steps=n_steps, batch=B, hyperparams=params, seed=3)
    parts = PolicySession(model, num_inference_steps=n_steps, batch=B, hyperparams=params, seed=3)
    g = torch.Generator().manual_seed(17)
    q = (torch.rand(B, 30, J, generator=g) - 0.5) * 2 * np.pi
    r = torch.randn(B, 30, 4, generator=g)
    state = torch.randint(0, 4, (B,), generator=g)
    x_T = torch.randn(B, T, J, generator=g)
    for s in (full, parts):
        s.push_joint_state(q.cuda())
        s.push_rotation(r.cuda())
        s.set_game_state(state.cuda())
    wins = {k: v.cpu() for k, v in full.windows().items()}
    with torch.no_grad():
        want64, want32 = _grade_context(full._context(), sd, wins, "session B=64")
    triples = [list(range(b, min(b + 3, B))) for b in range(0, B, 3)]
    for robots in triples:   # the last one is a single robot
        with torch.no_grad():
            ctx = parts._context(parts._subset(robots))
        for name, a, w64, w32 in zip(("action_history", "imu", "joint_states"), ctx, want64, want32):
            assert_fp32_grade(a, w64[robots], w32[robots], label=f"session robots {robots[0]}..{robots[-1]} {name}")
        assert _bits_equal(ctx[3].cpu(), want32[3][robots])
    acp = ddim_ref.alphas_cumprod()
    x0 = ddim_ref.sample(lambda xx, t: ref.forward_with_context(sd, want32, xx, torch.full((B,), t, dtype=torch.int64)), x_T, n_steps, acp)[-1]
    oracle = (ref.denormalize(x0, sd["mean"], sd["std"]) - np.pi).double()
    got_full = full.step(x_T.cuda()).cpu().double()
    got_parts = torch.cat([parts.step(x_T[robots].cuda(), robots=robots) for robots in triples]).cpu().double()
    per_robot = lambda a: ((a - oracle).flatten(1).norm(dim=1) / oracle.flatten(1).norm(dim=1)).max()
    e_full, e_parts = float(per_robot(got_full)), float(per_robot(got_parts))
    print(f"session tick, worst robot vs the fp32 oracle's rollout: 64 robots {e_full:.3e}, three at a time {e_parts:.3e}")
    assert e_full < 1e-4 and e_parts < 1e-4
    wf, wp = full.windows(), parts.windows()
    assert all(tuple(wf[k].shape) == tuple(wp[k].shape) for k in wf)
