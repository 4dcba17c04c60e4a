"""The route announced is the route that ran: for every row of tests/test_cpu_sampler_route.py's table that can launch (all but the
B = 32768 one) a two-step rollout at B = 2 under the library's per-class launch counter (sd_profile_enable / sd_profile_collect, as
bench.py uses it).  These shapes are the smallest at which each route is still selected."""

import ctypes as C

import pytest
import torch

from oracle import denoiser_ref as ref
from test_cpu_sampler_route import TABLE

gpu = pytest.mark.gpu
N_STEPS = 2
CASES = TABLE[:-1]
# launches per class (_lib.KERNEL_CLASSES order: panel_gemm, attention, patch_embed, fc_out, decoder_layer = the layer chains, decoder_head,
# traj_step) of each case, recorded from the library of the commit before the plan existed (same body, same visit)
PARENT_COUNTS = {
    (64, 4, 16, 10, 10, 2, 2, 3): (6, 8, 2, 2, 8, 0, 0),
    (128, 4, 16, 40, 8, 1, 2, 2): (2, 4, 0, 2, 4, 2, 0),
    (128, 4, 16, 40, 8, 1, 2, 1): (2, 4, 0, 2, 4, 2, 0),
    (128, 4, 16, 3, 8, 1, 2, 2): (2, 2, 0, 0, 2, 2, 0),
    (128, 4, 64, 3, 8, 1, 2, 2): (2, 2, 0, 0, 2, 2, 0),
    (256, 4, 64, 3, 8, 1, 2, 2): (2, 2, 0, 0, 2, 1, 0),
    (256, 4, 64, 3, 8, 1, 2, 1): (2, 2, 0, 0, 2, 2, 0),
    (256, 4, 64, 3, 8, 1, 2, 0): (2, 2, 0, 0, 2, 2, 0),
    (256, 4, 10, 3, 20, 2, 2, 3): (2, 0, 0, 0, 0, 0, 2),
    (256, 4, 10, 3, 20, 2, 2, 4): (2, 0, 0, 0, 0, 0, 2),
    (256, 4, 10, 15, 20, 2, 2, 3): (2, 0, 0, 0, 0, 0, 2),
    (256, 4, 10, 16, 20, 2, 2, 3): (2, 0, 0, 0, 0, 0, 2),
    (256, 4, 10, 16, 20, 2, 2, 4): (2, 0, 0, 0, 0, 0, 2),
    (256, 4, 10, 63, 20, 2, 2, 3): (2, 0, 0, 0, 0, 0, 2),
    (256, 4, 10, 64, 20, 2, 2, 3): (2, 0, 0, 0, 0, 0, 2),
    (256, 4, 100, 3, 20, 2, 2, 3): (2, 0, 0, 0, 0, 0, 2),
    (256, 4, 101, 3, 20, 2, 2, 3): (4, 4, 0, 0, 4, 1, 0),
    (128, 4, 10, 33, 22, 1, 2, 3): (1, 0, 0, 0, 0, 0, 2),
    (512, 4, 48, 10, 20, 2, 2, 3): (2, 0, 0, 0, 0, 0, 2),
    (512, 4, 49, 10, 20, 2, 2, 3): (4, 4, 0, 0, 4, 2, 0),
    (256, 4, 10, 3, 20, 9, 2, 3): (18, 18, 0, 0, 18, 2, 0),
    (256, 4, 10, 3, 33, 2, 2, 3): (6, 4, 2, 0, 4, 0, 0),
    (256, 8, 16, 3, 8, 1, 2, 2): (2, 4, 0, 2, 4, 2, 0),
}


def run_case(row):
    """(launches per class, sample, noise-prediction trace) of one rollout of N_STEPS steps at the row's shape and cap."""
    from soccerdiffusion_amd import _lib, ops

    d, heads, T, Mc, J, L, B, cap, _ = row
    lib = _lib.load()
    sd = ref.synthetic_state_dict(d, J, L, seed=5)
    packed = ops.pack_denoiser(sd, "cuda", heads=heads, max_len=T)
    g = torch.Generator().manual_seed(d + T + Mc)
    x_T = torch.randn(B, T, J, generator=g).cuda()
    ctx = torch.randn(B, Mc, d, generator=g).cuda()
    ts = ops.ddim_timesteps(N_STEPS)
    coef = ops.ddim_coefficients(ts, ops.alphas_cumprod(), N_STEPS)
    toks = ops.step_token(torch.tensor(ts).cuda(), ops.step_frequencies(d).cuda(), sd["step_encoding.token"].cuda()).reshape(N_STEPS, d)
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    lib.sd_profile_enable(1)
    try:
        x, et = ops.ddim_sample(packed, ctx, toks, coef, x_T, status=status, max_mode=cap, eps_trace=True)
        torch.cuda.synchronize()
    finally:
        lib.sd_profile_enable(0)
    n = len(_lib.KERNEL_CLASSES)
    ms, cnt = (C.c_double * n)(), (C.c_long * n)()
    _lib.check(lib.sd_profile_collect(ms, cnt, n), "sd_profile_collect")
    assert int(status.item()) == 0 and bool(torch.isfinite(x).all())
    return tuple(int(c) for c in cnt), x.cpu(), et.cpu()


@gpu
@pytest.mark.parametrize("row", CASES, ids=lambda r: "-".join(map(str, r)))
def test_announced_route_is_the_route_that_ran(row):
    from soccerdiffusion_amd import _lib

    route = _lib.sampler_route(*row[:8])
    assert route == row[8]
    counts, _, _ = run_case(row)
    by = dict(zip(_lib.KERNEL_CLASSES, counts))
    print(row, counts)
    if route.startswith("TRAJ_"):
        assert by["traj_step_kernel"] == N_STEPS and by["attention_kernel"] == 0 and by["decoder_layer_kernel"] == 0
    else:
        assert by["traj_step_kernel"] == 0
    assert counts == PARENT_COUNTS[row[:8]]
