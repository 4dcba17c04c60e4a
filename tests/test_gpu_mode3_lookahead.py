"""Sampler mode 3 (csrc/sd_traj.h, sa_head_precise) at the shapes where its early requests can go wrong: the Q | K and V biases, the
cross-attention's and the feed-forward's scales are requested a phase before the barrier they used to follow (across the projection
GEMM, across the scores on waves 4 - 7, across the last head into the next layer's first one), and the odd waves of a one-tile
trajectory have no V piece to add a bias to.  x after every DDIM step against the fp32 oracle, as
tests/test_gpu_denoiser.py::test_trajectory_step_kernel_every_step, with that file's tolerance.  Measured: worst relative error 2.7e-7."""

import pytest
import torch

from conftest import rel_err
from oracle import ddim_ref
from oracle import denoiser_ref as ref

pytestmark = pytest.mark.gpu
TOL = 1e-4
D, N_STEPS = 256, 2


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    from soccerdiffusion_amd import ops as o

    return o


def _problem(ops, T, Mc, J, L, B):
    from soccerdiffusion_amd import _lib

    assert _lib.load().sd_sampler_mode(D, 4, T, Mc, J) == 3
    sd = ref.synthetic_state_dict(D, J, L, seed=131 + T)
    g = torch.Generator().manual_seed(T * 11 + Mc)
    x_T = torch.randn(B, T, J, generator=g)
    ctx = torch.randn(B, Mc, D, generator=g) if Mc else None
    acp = ddim_ref.alphas_cumprod()
    ts = ddim_ref.timesteps(N_STEPS).tolist()
    packed = ops.pack_denoiser(sd, "cuda", max_len=T)
    toks = ops.step_token(torch.tensor(ts).cuda(), ops.step_frequencies(D).cuda(), sd["step_encoding.token"].cuda()).reshape(N_STEPS, D)
    coef = ops.ddim_coefficients(ts, acp, N_STEPS)

    def run():
        status = torch.zeros(1, dtype=torch.int32, device="cuda")
        x, trace = ops.ddim_sample(packed, ctx.cuda() if Mc else None, toks, coef, x_T.cuda(), trace=True, max_mode=3, status=status)
        assert int(status.item()) == 0
        return x.cpu(), [t.cpu() for t in trace]

    def oracle():
        return ddim_ref.sample(lambda x, t: ref.forward_with_context(sd, [ctx] if Mc else [], x, torch.full((B,), t, dtype=torch.int64)),
                               x_T, N_STEPS, acp)

    return run, oracle


@pytest.mark.parametrize("T,Mc,J,L,B", [
    # one token tile: the odd waves have no V piece
    (1, 10, 4, 1, 2), (16, 10, 20, 1, 2),
    # one tile on the odd waves: the smallest non-empty odd half
    (17, 10, 20, 2, 2),
    # the 7-tile instantiation with its shortest and its full last tile; two layers: requests that follow the last head of a layer
    (97, 10, 4, 2, 2), (100, 10, 20, 2, 2),
    # 17 memory rows: traj_step_wide_kernel runs the precise head too
    (10, 16, 20, 2, 2),
    # no context rows
    (100, 0, 4, 2, 2)])
def test_mode3_every_step_at_request_edges(ops, T, Mc, J, L, B):
    run, oracle = _problem(ops, T, Mc, J, L, B)
    want = oracle()
    x, trace = run()
    errs = [rel_err(trace[i], want[i]) for i in range(N_STEPS)]
    print("rel err per step", errs)
    assert all(e < TOL for e in errs), errs   # (max() would skip NaNs)
    assert torch.isfinite(x).all()


@pytest.mark.parametrize("T,Mc,J,L,B", [(100, 10, 20, 2, 2), (17, 10, 4, 2, 2)])
def test_mode3_repeat_call_same_bytes(ops, T, Mc, J, L, B):
    """A request issued before a barrier must not depend on what the previous launch left behind: two calls on the same inputs give
    the same bytes at every step."""
    run, _ = _problem(ops, T, Mc, J, L, B)
    x0, tr0 = run()
    x1, tr1 = run()
    assert torch.equal(x0, x1)
    assert all(torch.equal(a, b) for a, b in zip(tr0, tr1))
