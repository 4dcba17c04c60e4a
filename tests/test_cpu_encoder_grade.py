"""The CPU halves of tests/test_gpu_encoder_grade.py (cases in tests/encoder_cases.py): every attention and encoder case runs the attention
kernel its table names (sd_attention_route - the predicate attention() itself asks, so a moved threshold fails here instead of silently
taking attention_pipe_kernel out of the suite again), every patch-embedding case the path it names (patch_embed()'s staging restated), and
the power-of-two rescaling of an encoder layer is the same function bit for bit in the fp32 oracle."""

import pytest
import torch

import encoder_cases as ec
from oracle import denoiser_ref as ref


@pytest.fixture(scope="module")
def lib():
    from soccerdiffusion_amd import build

    build.build()
    from soccerdiffusion_amd import _lib

    return _lib


def test_case_runs_the_kernel_it_names(lib):
    for c in ec.ATTENTION_CASES + ec.LSE_CASES:
        B, d, heads, tq, s, _, kernel = c
        assert lib.attention_route(B, tq, s) == kernel, ec.attention_id(c)
    for c in ec.ENCODER_CASES:
        _, d, C, p, S, L, heads, B, kernel = c
        assert lib.attention_route(B, S // p, S // p) == kernel, ec.encoder_id(c)
    # the threshold itself, and what keeps a call off the pipe kernel at any batch
    assert lib.attention_route(63, 100, 100) == ec.AK and lib.attention_route(64, 100, 100) == ec.PIPE
    assert lib.attention_route(64, 128, 312) == ec.PIPE and lib.attention_route(64, 129, 100) == ec.AK
    assert lib.attention_route(64, 100, 100, has_extra=True) == ec.AK and lib.attention_route(64, 100, 100, dropout=True) == ec.AK
    assert lib.attention_route(64, 10, 0, has_extra=True) == ec.AK
    assert lib.load().sd_attention_route(0, 10, 10, 0, 0) == -1 and lib.load().sd_attention_route(64, 10, 0, 0, 0) == -1


def test_every_head_dim_of_the_pipe_kernel_meets_every_shape_class():
    met = {}
    for B, d, heads, tq, s, spike, kernel in ec.ATTENTION_CASES:
        if kernel == ec.PIPE and not spike:
            met.setdefault((d // heads, B >= 65), set()).add((tq, s))
    for hd in ec.HEAD_DIMS:
        assert met.get((hd, False), set()) | met.get((hd, True), set()) == set(ec.TQ_S), hd
        assert met.get((hd, False)) and met.get((hd, True)), hd          # 64 samples and 65
    assert met[(16, False)] == met[(16, True)] == set(ec.TQ_S)            # <16> (V padded to LDV > HD): every class at both
    for hd, dims in ec.HEAD_DIMS.items():                                # attention_kernel: every width at every class, 129 x 129 at 64 samples
        for d, heads in dims:
            assert {(tq, s) for B, dd, hh, tq, s, sp, k in ec.ATTENTION_CASES if (B, dd, hh, sp, k) == (3, d, heads, False, ec.AK)} == set(ec.TQ_S)
        assert any(c[0] == 64 and c[1] // c[2] == hd and c[3:5] == (129, 129) and c[6] == ec.AK for c in ec.ATTENTION_CASES)
        assert sum(c[1] // c[2] == hd and c[5] for c in ec.ATTENTION_CASES) == 2
    assert {c[1] // c[2] for c in ec.LSE_CASES} == set(ec.HEAD_DIMS) and {c[0] for c in ec.LSE_CASES} == {3, 64}


def test_patch_embed_case_takes_the_path_it_names():
    paths = set()
    rows_of = {}
    for c in ec.PATCH_CASES:
        d, C, p, B, S, path = c
        assert ec.patch_embed_path(C * p, d) == path, ec.patch_id(c)
        RB, DC = ec.patch_embed_plan(C * p, d)
        assert DC == 0 or (DC % 32 == 0 and (RB * (C * p + 1) + C * p * DC) * 4 <= 60 * 1024), ec.patch_id(c)   # what the launch asks of the LDS
        paths.add(path)
        rows_of.setdefault(C * p, set()).add(B * (S // p))
    assert paths == {ec.ONE_COLUMN, ec.GENERIC, ec.GENERIC + ", " + ec.RAGGED, ec.RB16, ec.RB16 + ", " + ec.RAGGED, ec.K_CHUNKS}
    assert set(rows_of) == {4, 20, 22, 25, 64, 65, 100, 128, 200, 220, 256, 512}
    assert set().union(*rows_of.values()) == {1, 15, 16, 17, 63, 64, 65, 130}
    for K, rows in rows_of.items():   # below, at and above the K class's own rows per workgroup
        RB = 64 if K <= 64 else 16
        assert {RB - 1, RB, RB + 1} <= rows, (K, sorted(rows))
    assert {c[0] for c in ec.PATCH_CASES} == {64, 128, 256, 512}
    # the K = 64 | 65 switch, and the widest K patch_embed_kernel stages whole
    assert ec.patch_embed_plan(64, 128)[0] == 64 and ec.patch_embed_plan(65, 128)[0] == 16
    assert ec.patch_embed_plan(319, 64) == (16, 32) and ec.patch_embed_plan(320, 64) == (16, 0)


def test_every_shipped_embedding_has_a_kernel():
    """DC >= 32 for every shipped (hidden_dim, C, patch) - or, for the one that has none (larger_model.yaml's image tokens, K = 512: 16 patches
    of 513 floats leave room for 13 columns of W^T), the K-chunked kernel, which takes any K."""
    chunked = []
    for d, C, p in ec.SHIPPED_EMBEDDINGS:
        RB, DC = ec.patch_embed_plan(C * p, d)
        if DC < 32:
            assert (RB, DC) == (16, 0) and ec.patch_embed_path(C * p, d) == ec.K_CHUNKS
            chunked.append((d, C, p))
    assert chunked == [(512, 512, 1)]


@pytest.mark.parametrize("k", ec.RESCALE_K)
@pytest.mark.parametrize("case", [c for c in ec.PROPERTY_CASES if c[7] == 3], ids=ec.encoder_id)
def test_power_of_two_rescaling_of_an_encoder_layer_preserves_the_fp32_oracle_bitwise(case, k):
    """Producer x 2^-k, consumer x 2^k for norm1 | in_proj, norm2 | linear1 and the V rows | out_proj together: the same function, bit
    for bit in fp32 - and every weight of a GEMM stays below 256, where panel_gemm16_kernel's fixed weight scale 2^8 keeps its fp16
    halves finite (synthetic weights are at most 1 / sqrt(64), so 2^8 of them is at most 32)."""
    _, d, C, p, S, L, heads, B, _ = case
    sd0, x = ec.encoder_weights(d, C, p, L), ec.encoder_input(C, S, B)
    sd = ec.rescaled_weights(sd0, L, k)
    assert ec.largest_gemm_weight(sd) < ec.W_LIMIT
    assert any(not torch.equal(sd[key], sd0[key]) for key in sd if key.endswith(ec.GEMM_WEIGHTS))
    assert torch.equal(ref.encoder_forward(sd, x, ec.PREFIX, torch.float32, heads), ec.encoder_oracles(case)[1])


def test_inputs_hold_the_robots_they_promise():
    x = ec.encoder_input(20, 100, 64)
    assert torch.equal(x[ec.STILL], x[ec.STILL, :1].expand(100, 20)) and not x[ec.ZEROS].any()
    assert 3e-4 < float(x[ec.SMALL].std()) < 3e-3 and 0.9 < float(x[0].std()) < 1.1
    q = ec.encoder_input(4, 100, 3)
    assert torch.allclose(q[0].norm(dim=-1), torch.ones(100), atol=1e-6) and float(ec.encoder_input(5, 100, 3)[0].abs().max()) <= 1
    spiked = next(c for c in ec.ATTENTION_CASES if c[5] and c[0] == 64)
    qq, kk, _ = ec.attention_inputs(spiked)
    assert ec.SPIKE_KEY >= 64 and torch.equal(kk[0, ec.SPIKE_KEY], qq[0, 5] * 3)
    assert float(qq[ec.SMALL_SAMPLE].std()) < 1e-2 < float(qq[0].std())
