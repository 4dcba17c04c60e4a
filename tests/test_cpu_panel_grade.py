"""The CPU halves of tests/test_gpu_panel_grade.py (cases in tests/panel_cases.py): every (case, cap) runs the row-panel route its table
names (sd_sampler_route - the plan the entry points themselves build, so a moved threshold fails here instead of silently taking a kernel
out of the suite), the list itself keeps every edge it was written for, the power-of-two rescalings are the same function bit for bit in
the fp32 oracle, and a CPU model of an out-projection accumulated in the residual registers against one with an accumulator of its own."""

import pytest
import torch

import panel_cases as pc
from oracle import denoiser_ref as ref
from parity import FACTOR, FLOOR, Errors, errors, report


@pytest.fixture(scope="module")
def lib():
    from soccerdiffusion_amd import build

    build.build()
    from soccerdiffusion_amd import _lib

    return _lib


def _route(lib, shape, cap):
    d, T, Mc, J, L, B = shape
    return lib.sampler_route(d, pc.HEADS, T, Mc, J, L, B, cap)


def test_case_runs_the_route_it_names(lib):
    for shape, want in pc.ROUTES.items():
        for cap in pc.CAPS:
            assert _route(lib, shape, cap) == want[cap], (shape, cap)
    for shape, want in pc.PANEL_ONLY.items():   # nothing else serves these: the default cap lands on the cap-2 route
        assert _route(lib, shape, 3) == want[2] and _route(lib, shape, -1) == want[2], shape
    for shape in pc.SHIPPED:                    # ... while the shipped shapes reach their row-panel routes through a cap (the rerun) alone
        assert _route(lib, shape, 3).startswith("TRAJ_"), shape
    for shape in pc.RESCALE_SHAPES:             # the rerun of the guarded calls, end to end
        assert _route(lib, shape, 3).startswith("TRAJ_")
    assert [_route(lib, s, 1) for s in pc.RESCALE_SHAPES] == [pc.FOLD, pc.F32]
    assert [_route(lib, s, 2) for s in pc.RESCALE_SHAPES] == [pc.FOLD16, pc.F16]


def test_the_list_keeps_every_edge_it_was_written_for():
    met = {}
    for shape, routes in pc.ROUTES.items():
        for r in routes:
            met.setdefault(r, set()).add(shape)
    # each of the five routes at every hidden_dim it exists for (the fp16 layer kernel is instantiated for 256 alone)
    for r in (pc.F32, pc.F16, pc.FUSED, pc.FOLD):
        assert {128, 256, 512} <= {s[0] for s in met[r]}, r
    assert {s[0] for s in met[pc.FOLD16]} == {256}
    assert 64 in {s[0] for s in met[pc.F32]}
    # 63 / 64 / 65 rows on both chain routes
    for r in (pc.F32, pc.F16):
        assert {63, 64, 65} <= {pc.rows(s) for s in met[r]}, r
    assert 1 in {pc.rows(s) for s in met[pc.FUSED]}
    # panel_cross_attention<D, 1> (<= 32 keys among a panel's trajectories) and <D, 2>, the latter at exactly 64 keys; one panel of
    # 64 trajectories; a last panel of one row
    unfolded = [s for s in pc.CASES if pc.ROUTES[s][0] == pc.FUSED]
    keys = {k for s in unfolded for _, k in pc.panels(s)}
    assert min(keys) == 1 and 32 in keys and 64 in keys and max(keys) == 64
    assert any(33 <= k for k in keys) and any(k <= 32 for k in keys)
    trajs = {n for s in unfolded for n, _ in pc.panels(s)}
    assert {1, 2, 3, 10, 64} <= trajs
    assert any(pc.rows(s) % 64 == 1 and pc.rows(s) > 64 for s in unfolded)
    assert any({k for _, k in pc.panels(s)} == {64, 32} for s in met[pc.FUSED])   # both instantiations inside one launch
    # the fold's conditions from both sides: 16 memory rows at 64 tokens; 63 tokens; 17 memory rows
    for d in (128, 256, 512):
        assert (d, 64, 15, 20, 2, 3) in met[pc.FOLD]
    assert (256, 63, 15, 20, 2, 3) not in met[pc.FOLD] and (256, 64, 16, 20, 2, 3) not in met[pc.FOLD]
    # the fused kernel's 64 keys from both sides
    assert (256, 100, 31, 20, 2, 2) in met[pc.FUSED] and (256, 100, 32, 20, 2, 2) in met[pc.F32]
    # joints: the MFMA head's J % 4, both fc_out tiles, the real robot's 22
    assert {4, 20, 22, 32, 33, 64} <= {s[3] for s in pc.CASES}
    assert {22, 33} <= {s[3] for s in met[pc.FOLD]} and {22, 33} <= {s[3] for s in met[pc.F32]} and 64 in {s[3] for s in met[pc.FOLD16]}
    # depth: the shipped 4 / 6 / 8 layers and one past the trajectory families' 8
    assert {1, 2, 4, 6, 8, 9} <= {s[4] for s in pc.CASES}
    # the fp16 self-attention's last horizon and the first past it
    assert {128, 129} <= {s[1] for s in met[pc.FOLD16]}
    assert len(pc.CASES) == 37 and all(len(r) == len(pc.CAPS) for r in pc.ROUTES.values())


RESCALE_K = [-12, -8, -4, 4, 8]
RESCALE_CASES = [(s, (p,), k) for s in pc.RESCALE_SHAPES for p in pc.PAIRS for k in (-12,)] + \
                [(s, tuple(pc.PAIRS), k) for s in pc.RESCALE_SHAPES for k in RESCALE_K]


def rescale_id(v):
    return "+".join(v) if isinstance(v, tuple) and isinstance(v[0], str) else pc.case_id(v) if isinstance(v, tuple) else f"k{v:+d}"


@pytest.mark.parametrize("shape,pairs,k", RESCALE_CASES, ids=rescale_id)
def test_power_of_two_rescaling_preserves_the_fp32_oracle_bitwise(shape, pairs, k):
    """The rescaled models the rerun tests hand to the GPU ARE the unscaled function: the fp32 oracle's output does not change by a bit."""
    _, _, _, _, _, want32 = pc.rescale_base(shape)
    sd, x, ctx, tok = pc.rescaled(shape, pairs, k)
    mem = torch.cat([ctx, tok.expand(x.shape[0], 1, shape[0])], 1)
    assert torch.equal(ref.denoiser_forward(sd, x, mem), want32)


def test_first_noise_prediction_is_the_forward_on_the_appended_step_token():
    """What lets sd_denoiser_forward share the rollout's oracles: forward_with_context at t = 980 is denoiser_forward on memory()."""
    shape = (128, 9, 20, 20, 1, 7)
    sd, x_T, ctx = pc.inputs(shape)
    _, _, _, eps32 = pc.oracles(shape)
    assert pc.schedule()[1][0] == 980
    assert torch.equal(ref.denoiser_forward(sd, x_T, pc.memory(shape)), eps32[0])
    assert pc.memory((128, 1, 0, 4, 1, 65)).shape == (65, 1, 128)


@pytest.mark.parametrize("d", [128, 256, 512])
def test_out_projection_in_the_residual_accumulator_against_its_own(d):
    """The site part 4 of the work rests on, modelled on the CPU: two layers of three sublayers h += LN(h) W^T + b in fp32, every product
    rounded into the accumulator as the 32x32x2 fp32 MFMA's fma chain does.  Accumulated INTO the residual (chain_a_kernel's and
    decoder_layer_kernel's form) each of the d roundings happens at the magnitude of the residual stream; in a zero accumulator that
    meets the residual in one addition (chain_b_kernel's form) they happen at the magnitude of the update.  Only the ordering is asserted,
    and that the own-accumulator form is fp32 grade; both figures are printed."""
    want64, want32, res, own = pc.out_projection_model(d)
    e32, e_res, e_own = errors(want32, want64), errors(res, want64), errors(own, want64)
    print(report(f"model d={d} accumulated in the residual", e_res, e32))
    print(report(f"model d={d} accumulator of its own", e_own, e32))
    for name, a, b, c in zip(Errors._fields, e_own, e_res, e32):
        assert a <= b, (name, e_own, e_res)
        assert a <= FACTOR * c + FLOOR, (name, e_own, e32)
