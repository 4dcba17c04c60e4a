"""What soccerdiffusion_amd/derived.py's rule buys at the model's boundary on the GPU: the captured rollout graph follows an optimizer
step that moves no version counter, and a model copies after its derived state (descriptor, loop sampler, graph) has been built."""

import copy

import pytest
import torch

from test_gpu_loop_form import _loop_cache, _model

pytestmark = pytest.mark.gpu
D, J, L, T, B, MC, N = 256, 20, 2, 16, 2, 5, 4


def _inputs(seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(B, MC, D, generator=g).cuda()], torch.randn(B, T, J, generator=g).cuda()


def test_graphed_sample_follows_an_optimizer_step():
    """The graph captures the step-token table by value.  FusedAdamW's update rewrites ``step_encoding.token`` through a raw pointer: neither
    its version counter nor its address moves, only ops.weights_generation() - which the graph's key has to contain."""
    from soccerdiffusion_amd.training import FusedAdamW

    m, _ = _model(D, J, L, T)
    ctx, x_T = _inputs(21)
    token = m.step_encoding.token
    token.requires_grad_(True)
    opt = FusedAdamW([token], lr=5e-2)   # (re-points the token into its flat buffer now: from here on the address stays)
    eager = m.sample(ctx, x_T, N)
    graphed = m.sample(ctx, x_T, N, use_graph=True)
    assert torch.equal(graphed, eager)
    version, ptr = token._version, token.data_ptr()
    token.grad.fill_(1.0)
    opt.step()
    assert (token._version, token.data_ptr()) == (version, ptr)
    eager2 = m.sample(ctx, x_T, N)
    graphed2 = m.sample(ctx, x_T, N, use_graph=True)
    assert torch.equal(graphed2, eager2)
    assert not torch.equal(graphed2, graphed)


def test_deepcopy_after_forward_and_sample():
    m, _ = _model(D, J, L, T)
    ctx, x_T = _inputs(22)
    step = torch.full((B,), 300).cuda()
    with torch.no_grad():
        eps = m.forward_with_context(ctx, x_T, step)
    x0 = m.sample(ctx, x_T, N)
    graphed = m.sample(ctx, x_T, N, use_graph=True)
    assert len(_loop_cache(m)) == 1
    twin = copy.deepcopy(m)
    assert len(_loop_cache(twin)) == 0
    assert twin.diffusion_action_generator.packed() is not m.diffusion_action_generator.packed()
    with torch.no_grad():
        assert torch.equal(twin.forward_with_context(ctx, x_T, step), eps)
    assert torch.equal(twin.sample(ctx, x_T, N), x0)
    assert torch.equal(twin.sample(ctx, x_T, N, use_graph=True), graphed)
    assert len(_loop_cache(twin)) == 1 and len(_loop_cache(m)) == 1
