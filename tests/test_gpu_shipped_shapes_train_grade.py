"""The training step held to fp32 grade (tests/parity.py) at the shapes the shipped YAML configs train at and at the edges of the routes
they take: the prediction row by row, the loss, and EVERY parameter gradient on three figures - the whole parameter, the q | k | v blocks
of the in-projections, the worst output row - where the other training suites gate one L2 norm per parameter at 1e-4 against the fp32
oracle, 150 - 300 x above what fp32 itself does there.

The yardstick is always the fp32 CPU oracle's own error against the fp64 oracle on the same inputs (oracle.denoiser_ref.train_loss_and_grads
in both types).  Every case has a CPU half that runs without a GPU: both oracles run, the blocks the fp64 oracle finds zero are exactly the
ones that are zero by construction, and the yardstick is neither zero nor infinite.  Every gated group prints one line
(python -m pytest -s; profiles/shipped_shapes_train_parity.txt is that output)."""

import functools
import math
import re
from typing import NamedTuple

import pytest
import torch

from oracle import ddim_ref
from oracle import denoiser_ref as ref
from parity import (FACTOR, assert_fp32_grade, assert_grads_fp32_grade, assert_loss_fp32_grade, errors, grad_blocks, grad_errors,
                    named_zero_blocks, zero_blocks)
from test_gpu_dropout import _decoder_masks
from test_gpu_reference_configs import BASE, CONFIGS, _state_dict_for
from test_gpu_training import _arm_fused, _check_grads

gpu = pytest.mark.gpu
HEADS = 4
LAYER = "diffusion_action_generator.transformer_decoder.layers.{}."


class Case(NamedTuple):
    kind: str      # full: m(input_data, x_t, t); pretrain / edge / dropout: forward_with_context on random context rows
    config: str    # the shipped config the model is built from (edges and dropout: decoder_only's flags around their own sizes)
    d: int
    L: int
    T: int
    Mc: int        # context rows handed to forward_with_context; -1: the config's encoders make them
    J: int
    B: int

    @property
    def id(self):
        if self.kind == "full":
            return f"{self.config}-J{self.J}-B{self.B}"
        if self.kind == "pretrain":
            return f"decoder_only-Mc{self.Mc}-J{self.J}"
        return f"{self.kind}-{self.d}-{self.T}-{self.Mc}-{self.J}"


def _full(config, J, B):
    c = CONFIGS[config]
    return Case("full", config, c["hidden_dim"], c["num_decoder_layers"], BASE["trajectory_prediction_length"], -1, J, B)


def _ctx(kind, shape, L=2, B=2):
    d, T, Mc, J = shape
    return Case(kind, "decoder_only", d, L, T, Mc, J, B)


FULL = [_full("default", 20, 2), _full("default", 22, 3), _full("larger_model", 20, 2), _full("sim_scratch", 20, 2),
        _full("sim_scratch", 22, 2)]
PRETRAIN = [_ctx("pretrain", (256, 10, 10, 20), L=4),    # decoder_only.yaml as train.py feeds it: 10 random context rows
            _ctx("pretrain", (256, 10, 10, 22), L=4),
            _ctx("pretrain", (256, 10, 0, 20), L=4)]     # no context at all: a memory of the step token alone
EDGES = [_ctx("edge", s) for s in [
    (128, 10, 310, 20), (128, 10, 311, 22), (128, 10, 312, 20),   # key width 311 / 312 / 313 around the attention backward's padding to 4
    (128, 1, 311, 20),                                            # a single token
    (256, 10, 15, 20), (256, 10, 16, 20),                         # M = 16 / 17: the last trajectory-owning forward, the first row chain
    (512, 10, 311, 22),                                           # the per-operation route
    (64, 16, 10, 20)]]                                            # d % 128 != 0: ungrouped weight gradients
# the route each edge's comment names (training.TrainRoute: stack, embed_head, traj_layers); the head launch needs d = 256 only
EDGE_ROUTES = [("chains", False, False)] * 4 + [("chains", True, True), ("chains", True, False), ("per_op", False, False), ("chains", False, False)]
DROPOUT = [_ctx("dropout", s) for s in [(128, 10, 311, 20), (512, 10, 311, 20), (256, 10, 40, 20)]]
DROPOUT_ROUTES = [("chains", False, False), ("per_op", False, False), ("chains", True, False)]   # 41 memory rows: row chains behind the head
DROPOUT_P = 0.1

# fused layer stacks a step runs once a FusedAdamW keeps split weight planes (training._fused_stack): the decoder and every sequence
# encoder of the config; none at hidden_dim 512 (training.train_route)
FULL_STACKS = {"default": 4, "sim_scratch": 3, "larger_model": 0}
# the blocks that are zero by construction are the attention count of the config (key bias of each): decoder layers x 2 + encoder layers
ZERO_COUNT = {"default": 14, "larger_model": 28, "sim_scratch": 18}

# Every figure of every route starts at parity.FACTOR = 4, and the prediction, the loss and the gradients' `glob` and `block` stay there.
# The routes named here by family and least decoder depth carry the convolution tests' 8 (tests/test_gpu_conv.py: e < 8 * e32 + 2e-7) on
# the gradients' `row` figure, as DEEP_FACTOR does in tests/test_gpu_shipped_shapes_grade.py; above 8 is a bug.
# Measured (profiles/shipped_shapes_train_parity.txt): the prediction is at 0.6 - 1.6 x the fp32 oracle's error everywhere; on `glob` and
# `block` the worst parameter of a case is at 1.4 - 4.0 x - the cost of 22-bit operands (fp16 hi + lo, no lo x lo product) in every GEMM
# of the backward.  What exceeds 4 is the `row` figure, at parameters whose rows are single elements or two-term sums:
#   * full model (the encoder stacks over 100 / 20 tokens and the decoder over their 302 / 41 memory rows): the LayerNorm weights and
#     biases in front of the attention in-projections (norm1 of the encoders, norm2 of the decoder) and an in_proj_bias at 4.0 - 5.6 x.
#     The site, taken apart for action_history_encoder layers.1.norm1.weight of default.yaml (5.6 x, element 30): that element belongs
#     to the feature with the loudest normalised column (rms 2.4 against a median 0.8 - the positional table drives it) and its gradient
#     is 5.8 x the RMS s of the parameter's elements, so the 4.2e-7 of ITS OWN value that the step's kernels are off by - a usual figure
#     for them - is 2.4e-6 .. 2.9e-6 of s (the atomics' order moves it from run to run), where the fp32 oracle happens to be within
#     7e-8 there and shows a worst element of 5.2e-7.  The LayerNorm backward kernel alone, on exact inputs, has its worst element
#     there too, at 5.5e-7 (plain fp32: row-strided partial sums, shared memory, atomics; rms 9e-8) where the same sums in torch show a
#     worst element of 3.0e-7 (rms 4e-8); the rest arrives with the incoming gradient.  No single kernel owns the excess and none
#     loses a term: the parameter's glob is 2.6 x.
#   * a horizon of one token (edge-128-1-311-20): fc_out.weight at 4.4 x (glob 2.6 x).  With B T = 2 rows each element of the weight
#     gradient is a sum of two products: the oracle rounds about once per element, so the operand format's 2^-22 is all that is seen.
# {(family, least number of decoder layers): factor of the row figure}
ROUTE_FACTOR = {
    ("full model, per-operation 128", 4): 8.0, ("full model, row chains 128", 4): 8.0,   # default.yaml: 5.6 x / 4.3 x
    ("full model, per-operation 256", 6): 8.0, ("full model, row chains 256", 6): 8.0,   # sim_scratch.yaml: 4.6 x / 5.1 x
    ("full model, per-operation 512", 8): 8.0,                                           # larger_model.yaml: 4.4 x
    ("one token, row chains 128", 2): 8.0,                                               # 4.4 x
}


def _route(case, fused):
    """training.train_route for the decoder of a case (the shipped configs have dim_feedforward = hidden_dim and fp32 weights; a FusedAdamW -
    `fused` - keeps every kind of plane).  The full models' memories have 41 / 302 rows: any count above 16 routes alike."""
    from soccerdiffusion_amd import training

    return training.train_route(decoder=True, d=case.d, heads=HEADS, T=case.T, M=41 if case.kind == "full" else case.Mc + 1, J=case.J,
                                ffn_is_d=True, params_ok=True, block_planes=fused, traj_planes=fused, x_differentiable=False)


def _family(case, fused):
    route = _route(case, fused)
    if route.stack == "per_op":
        route = f"per-operation {case.d}"
    elif route.traj_layers:
        route = "trajectory forward 256"
    else:
        route = f"row chains {case.d}"
    return ("full model, " if case.kind == "full" else "one token, " if case.T == 1 else "") + route


def _factor(case, fused):
    fam = _family(case, fused)
    return max([f for (name, depth), f in ROUTE_FACTOR.items() if name == fam and case.L >= depth], default=FACTOR)


def _params(case):
    return {**BASE, **CONFIGS[case.config], "hidden_dim": case.d, "num_decoder_layers": case.L, "trajectory_prediction_length": case.T,
            "num_joints": case.J}


@functools.lru_cache(maxsize=None)
def _inputs(case):
    """Weights, the noised trajectory x_t at t = (980, 3) or (980, 500, 3), the noise to predict and the conditioning: the synthetic
    dataset's fields for the full model, random context rows otherwise.  Built once per case and never written to."""
    from soccerdiffusion_amd import cli

    params = _params(case)
    sd = _state_dict_for(params)
    g = torch.Generator().manual_seed(1000 + case.d + 7 * case.T + case.Mc + case.J)
    x0, eps = torch.randn(case.B, case.T, case.J, generator=g), torch.randn(case.B, case.T, case.J, generator=g)
    t = torch.tensor([980, 3] if case.B == 2 else [980, 500, 3])
    assert t.shape[0] == case.B
    x_t = ddim_ref.add_noise(x0, eps, t, ddim_ref.alphas_cumprod())
    inp, ctx = None, None
    if case.kind == "full":
        data = cli.synthetic_dataset(case.B, params, seed=3)
        inp = {k: data[k] for k in cli.CONTEXT_KEYS if k in data}
    else:
        ctx = [torch.randn(case.B, case.Mc, case.d, generator=g)] if case.Mc else []
    return params, sd, x_t, t, eps, inp, ctx


def _oracle(case, dtype, masks=None):
    """(prediction, loss, {parameter: gradient}) of the CPU oracle in `dtype`; the fp64 run holds the same weights in float64, so that
    its gradients are not rounded to fp32 on the way out."""
    _, sd, x_t, t, eps, inp, ctx = _inputs(case)
    if dtype == torch.float64:
        sd = {k: v.double() if v.is_floating_point() else v for k, v in sd.items()}
    return ref.train_loss_and_grads(sd, x_t, t, eps, context=ctx, input_data=inp, dtype=dtype, dropout_masks=masks)


@functools.lru_cache(maxsize=None)
def _references(case):
    """Both oracles of a case without dropout, computed once and shared by its CPU half and its GPU runs."""
    return _oracle(case, torch.float64), _oracle(case, torch.float32)


def _cpu_masks(case):
    """Masks for the CPU half of a dropout case (the GPU test hands the oracles the masks the kernels regenerate instead): keep with
    probability 1 - p, scaled by 1 / (1 - p), fixed per (layer, site)."""
    def masks(layer, kind, shape):
        g = torch.Generator().manual_seed(77 + 16 * layer + kind)
        return (torch.rand(shape, generator=g) >= DROPOUT_P).double() / (1.0 - DROPOUT_P)

    return masks


def _named_zero(case, grads):
    return named_zero_blocks(grads, one_row_memory=case.kind != "full" and case.Mc == 0, one_token=case.T == 1)


# ------------------------------------------------------------------------------------------------------------------------------------
# 1. the gradient metric itself (no GPU)
# ------------------------------------------------------------------------------------------------------------------------------------
class _Grads:
    """What _check_grads reads of a model: named_parameters() whose .grad are the given gradients."""

    def __init__(self, grads):
        self.params = {}
        for k, g in grads.items():
            self.params[k] = torch.nn.Parameter(torch.zeros_like(g, dtype=torch.float32))
            self.params[k].grad = g.to(torch.float32)

    def named_parameters(self):
        return iter(self.params.items())


def test_gradient_gate_sees_one_bad_key_row_that_the_norm_rule_passes_and_never_passes_nan():
    case = EDGES[-1]
    (_, _, g64), (_, _, g32) = _references(case)
    d = case.d
    name = LAYER.format(1) + "multihead_attn.in_proj_weight"
    # the fp32 oracle against itself: every figure equals its yardstick
    assert_grads_fp32_grade(g32, g64, g32, factor=1, floor=0, label="fp32 oracle against itself")
    # one row of the K block, the loudest, moved by 1e-5 of its own norm
    row = d + int(g64[name][d : 2 * d].norm(dim=1).argmax())
    got = {k: v.clone() for k, v in g32.items()}
    u = torch.nn.functional.normalize(torch.randn(d, generator=torch.Generator().manual_seed(0), dtype=torch.float64), dim=0)
    got[name] = g64[name].clone()
    got[name][row] += 1e-5 * g64[name][row].norm() * u
    worst = _check_grads(_Grads(got), g32)                 # the rule of the 1e-4 suites passes, with a factor of 20 to spare
    assert worst < 5e-6
    e = grad_errors(got, g64)[name]
    assert e.row == pytest.approx(float(1e-5 * g64[name][row].norm() / g64[name].norm(dim=1).pow(2).mean().sqrt()), rel=1e-3)
    assert e.glob < 2e-6 < 1e-5 < e.row                    # what one norm over the parameter does not see
    with pytest.raises(AssertionError, match=re.escape(f"{name}, row {row} (block 'k')")):
        assert_grads_fp32_grade(got, g64, g32, label="one bad key row")
    # non-finite values, in a live block and in one that is zero by construction
    bias = LAYER.format(0) + "self_attn.in_proj_bias"
    for bad in (float("nan"), float("inf")):
        for key, at in ((name, (row, 3)), (bias, (d + 2,))):
            got = {k: v.clone() for k, v in g32.items()}
            got[key][at] = bad
            with pytest.raises(AssertionError, match=re.escape(key)):
                assert_grads_fp32_grade(got, g64, g32, label="non-finite")
    # a parameter that is zero as a whole is held absolutely: norm2 under a one-row memory
    (_, _, z64), (_, _, z32) = _references(PRETRAIN[2])
    n2 = LAYER.format(0) + "norm2.weight"
    assert grad_errors(z32, z64)[n2] is None
    got = {k: v.clone() for k, v in z32.items()}
    got[n2] = got[n2] + 1e-5 * max(float(v.norm()) for k, v in z64.items() if k.startswith(LAYER.format(0))) / math.sqrt(case.d)
    with pytest.raises(AssertionError, match="zero by construction"):
        assert_grads_fp32_grade(got, z64, z32, label="a loud zero")
    got[n2] = torch.full_like(got[n2], float("nan"))
    with pytest.raises(AssertionError, match="zero by construction"):
        assert_grads_fp32_grade(got, z64, z32, label="a NaN zero")
    # a missing key
    got = {k: v for k, v in g32.items() if k != name}
    with pytest.raises(AssertionError, match="key sets differ"):
        assert_grads_fp32_grade(got, g64, g32)


# ------------------------------------------------------------------------------------------------------------------------------------
# 2. the CPU half of every case (no GPU)
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", FULL + PRETRAIN + EDGES + DROPOUT, ids=lambda c: c.id)
def test_oracles_run_and_the_zero_set_is_the_named_one(case):
    """Both oracles run; the blocks the fp64 oracle finds zero (parity.zero_blocks) are exactly the ones that are zero by construction -
    the cap on what leaves the relative gate; every figure of the fp32 yardstick is finite and not zero (a zero would turn the gate
    into a bare floor)."""
    if case.kind == "dropout":
        masks = _cpu_masks(case)
        (p64, l64, g64), (p32, l32, g32) = _oracle(case, torch.float64, masks), _oracle(case, torch.float32, masks)
    else:
        (p64, l64, g64), (p32, l32, g32) = _references(case)
    assert set(g64) == set(g32) and all(v.dtype == torch.float64 for v in g64.values())
    zero = zero_blocks(g64)
    assert zero == _named_zero(case, g64)
    attentions = sum(k.endswith("in_proj_bias") for k in g64)
    if case.kind == "full":
        assert len(zero) == attentions == ZERO_COUNT[case.config]
    elif case.T == 1:
        assert len(zero) == 5 * case.L   # both key biases; the self-attention's q and k weight blocks and its q bias
    elif case.Mc:
        assert len(zero) == attentions == 2 * case.L
    else:
        assert len(zero) == 7 * case.L   # both key biases; the cross-attention's q and k blocks, weight and bias; norm2
    # zero in the oracles as well: <= 1e-18 of the largest gradient in fp64, rounding noise in fp32
    top = max(float(v.norm()) for v in g64.values())
    for k, lab in zero:
        sl = dict(grad_blocks(k, g64[k].shape[0]))[lab]
        assert float(g64[k][sl].norm()) <= 1e-15 * top and float(g32[k][sl].norm()) <= 1e-8 * top, (k, lab)
    e32 = grad_errors(g32, g64, zero)
    for k, e in e32.items():
        if e is None:
            assert all((k, lab) in zero for lab, _ in grad_blocks(k, g64[k].shape[0]))
            continue
        assert all(0.0 < v < 1e-4 for v in e), (k, e)
    assert all(0.0 < v < 1e-4 for v in errors(p32, p64))
    assert math.isfinite(float(l32)) and abs(float(l32) - float(l64)) / float(l64) < 1e-5


# ------------------------------------------------------------------------------------------------------------------------------------
# 3. the training step on the GPU
# ------------------------------------------------------------------------------------------------------------------------------------
def _gpu_step(case, fused, p=0.0):
    """One forward + backward of the model in train() mode: (model, prediction, loss, gradients, fused stacks run, trajectory layers run)."""
    from soccerdiffusion_amd import cli, training

    params, sd, x_t, t, eps, inp, ctx = _inputs(case)
    m = cli.build_model(params).cuda()
    m.load_state_dict(sd)
    m.set_dropout(p, seed=4242)
    m.train()
    _arm_fused(m, fused)
    stacks, layers = training.FUSED_STACKS[0], training.TRAJ_LAYERS[0]
    if case.kind == "full":
        pred = m({k: v.cuda() for k, v in inp.items()}, x_t.cuda(), t.cuda())
    else:
        pred = m.forward_with_context([c.cuda() for c in ctx], x_t.cuda(), t.cuda())
    stacks, layers = training.FUSED_STACKS[0] - stacks, training.TRAJ_LAYERS[0] - layers
    loss = training.mse_loss(pred, eps.cuda())
    loss.backward()
    grads = {k: v.grad.detach().cpu() for k, v in m.named_parameters() if v.grad is not None}
    return m, pred.detach().cpu(), float(loss.detach()), grads, stacks, layers


def _gate(case, fused, got, want64, want32):
    pred, loss, grads = got
    (p64, l64, g64), (p32, l32, g32) = want64, want32
    row_factor = _factor(case, fused)
    label = f"{case.id} {'fused' if fused else 'per-op'}" + ("" if row_factor == FACTOR else f" [row {row_factor:g} x]")
    zero = zero_blocks(g64)
    assert zero == _named_zero(case, g64)
    assert set(grads) == set(g64)
    failures = []
    for check in (lambda: assert_fp32_grade(pred, p64, p32, label=f"{label} prediction"),
                  lambda: assert_loss_fp32_grade(loss, l64, l32, label=label),
                  lambda: assert_grads_fp32_grade(grads, g64, g32, zero=zero, row_factor=row_factor, label=label)):
        try:   # every figure of the case is printed before the first miss is raised
            check()
        except AssertionError as exc:
            failures.append(str(exc))
    assert not failures, "\n".join(failures)


FULL_RUNS = [(c, f) for c in FULL for f in ((True,) if c.config == "larger_model" else (False, True))]
PRETRAIN_RUNS = [(PRETRAIN[0], False)] + [(c, True) for c in PRETRAIN]


def _run_id(v):
    return v.id if isinstance(v, Case) else ("fused" if v else "per-op")


@gpu
@pytest.mark.parametrize("case,fused", FULL_RUNS, ids=_run_id)
def test_full_model_step_is_fp32_grade(case, fused):
    """default.yaml, larger_model.yaml and sim_scratch.yaml (images off) through m(input_data, x_t, t): the decoder over the encoders'
    302 / 41 memory rows and the encoder stacks whose gradient arrives through the memory, at 20 joints (_EmbedHead's width rule) and at
    the database's 22 (_PatchEmbed), with the fused row chains and on the per-operation nodes."""
    m, pred, loss, grads, stacks, layers = _gpu_step(case, fused)
    assert (stacks, layers) == (FULL_STACKS[case.config] if fused else 0, 0)
    # row chains at 128 / 256, entered through the head launch at 256 x 20 joints; per-operation at 512 and without planes
    chains = fused and case.config != "larger_model"
    assert _route(case, fused) == (("chains", case.d == 256 and case.J == 20, False) if chains else ("per_op", False, False))
    _gate(case, fused, (pred, loss, grads), *_references(case))


@gpu
@pytest.mark.parametrize("case,fused", PRETRAIN_RUNS, ids=_run_id)
def test_decoder_pretraining_step_is_fp32_grade(case, fused):
    """decoder_only.yaml through forward_with_context on 10 random context rows - the only shipped shape on the trajectory-owning layer
    forward (csrc/sd_train_traj.hip) - and on no context at all: a memory of one row, where the cross-attention's probabilities are 1 and
    its query side has no gradient."""
    m, pred, loss, grads, stacks, layers = _gpu_step(case, fused)
    assert (stacks, layers) == ((1, case.L) if fused else (0, 0))
    assert _route(case, fused) == (("chains", case.J == 20, True) if fused else ("per_op", False, False))   # the head launch: J % 4 == 0
    _gate(case, fused, (pred, loss, grads), *_references(case))


@gpu
@pytest.mark.parametrize("case", EDGES, ids=lambda c: c.id)
def test_route_edges_are_fp32_grade(case):
    """Two layers on random context rows at the smallest shapes where the routes of the shipped configs can still go wrong, a
    FusedAdamW armed: the fused route wherever it exists."""
    m, pred, loss, grads, stacks, layers = _gpu_step(case, True)
    assert stacks == (0 if case.d == 512 else 1)
    assert layers == (case.L if case.d == 256 and case.Mc + 1 <= 16 else 0)
    assert _route(case, True) == EDGE_ROUTES[EDGES.index(case)]
    _gate(case, True, (pred, loss, grads), *_references(case))


@gpu
@pytest.mark.parametrize("case", DROPOUT, ids=lambda c: c.id)
def test_step_with_dropout_is_fp32_grade_under_the_same_masks(case):
    """p = 0.1, what the reference trains with: both oracles apply the masks the kernels regenerate (test_gpu_dropout._decoder_masks);
    fresh masks per call and eval() are test_gpu_dropout.py's."""
    from soccerdiffusion_amd import ops

    m, pred, loss, grads, stacks, layers = _gpu_step(case, True, p=DROPOUT_P)
    assert (stacks, layers) == (0 if case.d == 512 else 1, 0)
    assert _route(case, True) == DROPOUT_ROUTES[DROPOUT.index(case)]
    gen = m.diffusion_action_generator
    regenerate = _decoder_masks(ops, gen, gen.dropout.calls, case.B, case.T, case.Mc + 1, case.d, HEADS)
    seen = {}

    def masks(layer, kind, shape):
        key = (layer, kind, shape)
        if key not in seen:
            seen[key] = regenerate(layer, kind, shape)
        return seen[key]

    want64, want32 = _oracle(case, torch.float64, masks), _oracle(case, torch.float32, masks)
    assert len(seen) == 6 * case.L and all(float((v == 0).double().mean()) > 0.02 for v in seen.values())
    _gate(case, True, (pred, loss, grads), want64, want32)
