"""Swin-T / Swin-S image encoder inference on csrc/sd_swin.hip (reference option image_encoder_type "swin_transformer_tiny" / "_small":
soccer_diffusion/ml/model/encoder/image.py:11-20, 86-100).  Oracle: the same torch modules (ml/model/encoder/image.py, torchvision Swin V1
restated) deep-copied to float64 on the CPU; bar 1e-4 relative (max-abs error / max-abs value).  Parameters that default to trivial values
(LayerNorm 1 / 0, bias 0, a 0.02 relative-position table) are randomised so that a bias, mask or LayerNorm bug cannot hide."""

import copy
import math
import os

import pytest
import torch
import torch.nn.functional as F
from torch import nn

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _rel(got, want):
    want = want.double().cpu()
    return float((got.double().cpu() - want).abs().max() / want.abs().max())


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    from soccerdiffusion_amd import ops as o

    return o


def _randomise(mod: nn.Module, seed: int):
    from soccerdiffusion_amd.ml.model.encoder.image import _ShiftedWindowAttention

    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in mod.modules():
            if isinstance(m, nn.LayerNorm):
                m.weight.copy_(0.5 + torch.rand(m.weight.shape, generator=g))
                m.bias.copy_(0.5 * torch.randn(m.bias.shape, generator=g))
            elif isinstance(m, nn.Linear) and m.bias is not None:
                m.bias.copy_(0.3 * torch.randn(m.bias.shape, generator=g))
            elif isinstance(m, _ShiftedWindowAttention):
                m.relative_position_bias_table.copy_(torch.randn(m.relative_position_bias_table.shape, generator=g))
            elif isinstance(m, nn.Conv2d) and m.bias is not None:
                m.bias.copy_(0.3 * torch.randn(m.bias.shape, generator=g))
    return mod


# ---- token GEMM -------------------------------------------------------------------------------------
def _pairs():
    out = []
    for C in (96, 192, 384, 768):
        out += [(C, 3 * C, True, False), (C, C, False, False), (C, 4 * C, True, True), (4 * C, C, False, False)]
        if C < 768:
            out.append((4 * C, 2 * C, True, False))
    return out + [(768, 64, False, False), (768, 37, False, False)]


@pytest.mark.parametrize("K,N,ln,gelu", _pairs())
@pytest.mark.parametrize("R", [77, 200])
def test_token_linear_matches_fp64(ops, K, N, ln, gelu, R):
    g = torch.Generator().manual_seed(K * 7 + N + R)
    A = torch.randn(R, K, generator=g) * 2.0 + 0.5
    W = torch.randn(N, K, generator=g) * K ** -0.5
    b = torch.randn(N, generator=g)
    lw, lb = 0.5 + torch.rand(K, generator=g), torch.randn(K, generator=g)
    res = torch.randn(R, N, generator=g)
    x = F.layer_norm(A.double(), (K,), lw.double(), lb.double(), 1e-5) if ln else A.double()
    y = x @ W.double().T + b.double()
    if gelu:
        y = F.gelu(y)
    pk = ops.PackedTokenLinear(W.to(DEV))
    kw = dict(ln=(lw.to(DEV), lb.to(DEV), 1e-5) if ln else None, gelu=gelu)
    got = ops.token_linear(A.to(DEV), pk, b.to(DEV), **kw)
    assert _rel(got, y) < 1e-4
    # residual into a fresh output and in place (res is out)
    got2 = ops.token_linear(A.to(DEV), pk, b.to(DEV), res=res.to(DEV), **kw)
    assert _rel(got2, y + res.double()) < 1e-4
    io = res.to(DEV)
    out = ops.token_linear(A.to(DEV), pk, b.to(DEV), res=io, out=io, **kw)
    assert out.data_ptr() == io.data_ptr() and _rel(io, y + res.double()) < 1e-4
    torch.cuda.synchronize()


# ---- window attention -------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,heads,B", [(56, 56, 3, 2), (24, 24, 6, 2), (6, 6, 3, 3), (7, 14, 12, 2), (14, 7, 3, 1), (13, 9, 6, 2),
                                         (30, 40, 1, 1)])
@pytest.mark.parametrize("shift", [0, 3])
def test_window_attention_matches_fp64(ops, H, W, heads, B, shift):
    from soccerdiffusion_amd.ml.model.encoder.image import _ShiftedWindowAttention

    torch.manual_seed(H * W + heads + shift)
    C = 32 * heads
    m = _randomise(_ShiftedWindowAttention(C, 7, shift, heads), H + shift)
    x = torch.randn(B, H, W, C)
    ref = copy.deepcopy(m).double()
    ref.proj = nn.Identity()   # the kernel stops before proj
    with torch.no_grad():
        want = ref(x.double())
        qkv = (x.double() @ m.qkv.weight.double().T + m.qkv.bias.double()).float()
    md = m.to(DEV)
    got = ops.swin_window_attention(qkv.to(DEV).contiguous(), heads, 7, shift, md.qkv.bias.detach(), md.relative_position_bias_table.detach(),
                                    md.relative_position_index)
    assert got.shape == (B, H, W, C)
    assert _rel(got, want) < 1e-4


# ---- patch embedding, merging, head ------------------------------------------------------------------
@pytest.mark.parametrize("N,H,W", [(2, 224, 224), (3, 96, 100), (1, 31, 45)])
def test_patch_embed_matches_fp64(ops, N, H, W):
    from soccerdiffusion_amd.ml.model.encoder.image import _Permute

    g = torch.Generator().manual_seed(H + W)
    stem = _randomise(nn.Sequential(nn.Conv2d(3, 96, 4, 4), _Permute([0, 2, 3, 1]), nn.LayerNorm(96, eps=1e-5)), H)
    x = torch.rand(N, 3, H, W, generator=g) * 2.0 - 0.7
    with torch.no_grad():
        want = copy.deepcopy(stem).double()(x.double())
    s = stem.to(DEV)
    got = ops.swin_patch_embed(x.to(DEV), s[0].weight.detach(), s[0].bias.detach(), (s[2].weight.detach(), s[2].bias.detach(), 1e-5))
    assert got.shape == want.shape and _rel(got, want) < 1e-4


@pytest.mark.parametrize("H,W,C", [(56, 56, 96), (7, 5, 96), (13, 14, 192), (3, 3, 384), (1, 1, 96)])
def test_patch_merging_matches_fp64(ops, H, W, C):
    from soccerdiffusion_amd.ml.model.encoder.image import _PatchMerging

    torch.manual_seed(H * W + C)
    m = _randomise(_PatchMerging(C), C)
    x = torch.randn(2, H, W, C)
    with torch.no_grad():
        want = copy.deepcopy(m).double()(x.double())
    md = m.to(DEV)
    got = ops.token_merge_linear(x.to(DEV), ops.PackedTokenLinear(md.reduction.weight), (md.norm.weight, md.norm.bias, 1e-5))
    assert got.shape == want.shape and _rel(got, want) < 1e-4


@pytest.mark.parametrize("H,W,hidden", [(7, 7, 64), (4, 7, 128), (1, 1, 37)])
def test_head_matches_fp64(ops, H, W, hidden):
    torch.manual_seed(hidden + H)
    norm, head = _randomise(nn.LayerNorm(768, eps=1e-5), 1), _randomise(nn.Linear(768, hidden), 2)
    x = torch.randn(3, H, W, 768) + 0.3
    with torch.no_grad():
        want = head.double()(norm.double()(x.double()).mean(dim=(1, 2)))
    norm, head = norm.float().to(DEV), head.float().to(DEV)
    got = ops.swin_head(x.to(DEV), (norm.weight, norm.bias, 1e-5), ops.PackedTokenLinear(head.weight), head.bias)
    assert got.shape == (3, hidden) and _rel(got, want) < 1e-4


# ---- the encoder end to end ----------------------------------------------------------------------------
def _encoder(kind, R, seed):
    from soccerdiffusion_amd.ml.model.encoder.image import ImageEncoderType, image_encoder_factory

    torch.manual_seed(seed)
    return _randomise(image_encoder_factory(getattr(ImageEncoderType, kind), 64, True, R), seed).eval()


@pytest.mark.parametrize("kind,H,W", [("SWIN_TRANSFORMER_TINY", 224, 224), ("SWIN_TRANSFORMER_TINY", 96, 96), ("SWIN_TRANSFORMER_TINY", 224, 448),
                                      ("SWIN_TRANSFORMER_SMALL", 224, 224), ("SWIN_TRANSFORMER_SMALL", 96, 96)])
def test_swin_encoder_matches_fp64(kind, H, W):
    enc = _encoder(kind, H, H + W)
    x = torch.rand(2, 2, 3, H, W, generator=torch.Generator().manual_seed(5)) * 2.0 - 0.7
    with torch.no_grad():
        want = copy.deepcopy(enc).double()(x.double())
        got = enc.to(DEV)(x.to(DEV))
    assert got.shape == (2, 2, 64)
    assert _rel(got, want) < 1e-4


def test_swin_inference_runs_the_hip_route():
    """Launch counts per entry point, no torch linear / softmax / roll / layer_norm inside the forward, SD_SWIN=torch keeps the torch ops and
    agrees, a tape or train() keeps the torch ops and gradients flow."""
    from soccerdiffusion_amd import ops as o

    enc = _encoder("SWIN_TRANSFORMER_TINY", 96, 11).to(DEV)
    x = torch.rand(1, 3, 3, 96, 96, device=DEV)
    names = ("swin_patch_embed", "token_linear", "swin_window_attention", "token_merge_linear", "swin_head")
    calls = {n: 0 for n in names}
    orig = {n: getattr(o, n) for n in names}

    def wrap(n):
        def f(*a, **k):
            calls[n] += 1
            return orig[n](*a, **k)
        return f

    for n in names:
        setattr(o, n, wrap(n))
    try:
        with torch.no_grad():
            got = enc(x)
        counted = dict(calls)
        with torch.no_grad(), torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CPU]) as prof:
            enc(x)
        hip_during_tape = dict(calls)
        xg = x.clone().requires_grad_(True)
        enc(xg).square().sum().backward()       # a tape: the torch ops, gradients flow
        assert calls == hip_during_tape
        enc.train()
        with torch.no_grad():
            enc(x)
        enc.eval()
        assert calls == hip_during_tape
    finally:
        for n in names:
            setattr(o, n, orig[n])
    # Swin-T: 2 + 2 + 6 + 2 blocks, 3 mergings
    assert counted == {"swin_patch_embed": 1, "token_linear": 4 * 12 + 1, "swin_window_attention": 12, "token_merge_linear": 3, "swin_head": 1}
    ran = {e.key for e in prof.key_averages()}
    for op in ("aten::linear", "aten::softmax", "aten::roll", "aten::layer_norm", "aten::addmm", "aten::conv2d"):
        assert op not in ran, op
    assert xg.grad is not None and torch.isfinite(xg.grad).all() and xg.grad.abs().sum() > 0
    os.environ["SD_SWIN"] = "torch"
    try:
        with torch.no_grad():
            lib = enc(x)
    finally:
        del os.environ["SD_SWIN"]
    assert _rel(got, lib) < 1e-4


def test_weight_updates_are_seen():
    from soccerdiffusion_amd.training import FusedAdamW

    enc = _encoder("SWIN_TRANSFORMER_TINY", 64, 21).to(DEV)
    x = torch.rand(1, 2, 3, 64, 64, device=DEV)

    def torch_route():
        os.environ["SD_SWIN"] = "torch"
        try:
            with torch.no_grad():
                return enc(x)
        finally:
            del os.environ["SD_SWIN"]

    with torch.no_grad():
        before = enc(x)
        enc.encoder.features[1][0].attn.qkv.weight.mul_(1.5)   # an in-place edit: the version counter moves
        edited = enc(x)
    assert float((edited - before).abs().max()) > 1e-3 and _rel(edited, torch_route()) < 1e-4
    opt = FusedAdamW(enc.parameters(), lr=5e-2)   # version-less updates on raw pointers: ops.weights_generation() moves
    for p in enc.parameters():
        p.grad.normal_()
    opt.step()
    with torch.no_grad():
        after = enc(x)
    assert float((after - edited).abs().max()) > 1e-3 and _rel(after, torch_route()) < 1e-4


def test_inference_mode_matches_no_grad():
    enc = _encoder("SWIN_TRANSFORMER_TINY", 96, 31).to(DEV)
    x = torch.rand(2, 2, 3, 96, 96, device=DEV)
    with torch.no_grad():
        want = enc(x)
    with torch.inference_mode():
        xi = torch.rand(2, 2, 3, 96, 96, device=DEV)
        xi.copy_(x)
        got = enc(xi)
        got2 = enc(xi)
    assert torch.equal(got, want) and torch.equal(got2, want)


def test_bad_arguments_raise_value_error(ops):
    W = torch.randn(96, 96, device=DEV)
    pk = ops.PackedTokenLinear(W)
    A = torch.randn(10, 96, device=DEV)
    bad = [lambda: ops.PackedTokenLinear(torch.randn(96, 80, device=DEV)),              # K not a multiple of 32
           lambda: ops.PackedTokenLinear(W.double()),
           lambda: ops.token_linear(torch.randn(10, 64, device=DEV), pk),             # K mismatch
           lambda: ops.token_linear(A.cpu(), pk),
           lambda: ops.token_linear(A.half(), pk),
           lambda: ops.token_linear(torch.randn(96, 10, device=DEV).T, pk),           # strided
           lambda: ops.token_linear(A, pk, bias=torch.zeros(95, device=DEV)),
           lambda: ops.token_linear(A, pk, res=torch.zeros(10, 95, device=DEV)),
           lambda: ops.token_linear(A, pk, ln=(torch.ones(95, device=DEV), torch.zeros(96, device=DEV), 1e-5)),
           lambda: ops.swin_window_attention(torch.randn(1, 7, 7, 3 * 96, device=DEV), 4, 7, 3, torch.zeros(288, device=DEV),
                                             torch.zeros(169, 4, device=DEV), torch.zeros(2401, dtype=torch.int64, device=DEV)),   # head dim 24
           lambda: ops.swin_window_attention(torch.randn(1, 7, 7, 288, device=DEV), 3, 7, 3, torch.zeros(288, device=DEV),
                                             torch.zeros(169, 3, device=DEV), torch.zeros(2401, dtype=torch.int32, device=DEV)),
           lambda: ops.swin_window_attention(torch.randn(1, 7, 7, 288, device=DEV), 3, 9, 3, torch.zeros(288, device=DEV),
                                             torch.zeros(289, 3, device=DEV), torch.zeros(9 ** 4, dtype=torch.int64, device=DEV)),
           lambda: ops.swin_patch_embed(torch.rand(1, 4, 32, 32, device=DEV), torch.zeros(96, 3, 4, 4, device=DEV), torch.zeros(96, device=DEV),
                                        (torch.ones(96, device=DEV), torch.zeros(96, device=DEV), 1e-5)),
           lambda: ops.swin_patch_embed(torch.rand(1, 3, 32, 32, device=DEV), torch.zeros(96, 3, 2, 2, device=DEV), torch.zeros(96, device=DEV),
                                        (torch.ones(96, device=DEV), torch.zeros(96, device=DEV), 1e-5)),
           lambda: ops.token_merge_linear(torch.randn(1, 4, 4, 48, device=DEV), pk, (torch.ones(96, device=DEV), torch.zeros(96, device=DEV), 1e-5)),
           lambda: ops.swin_head(torch.randn(1, 7, 7, 96, device=DEV), (torch.ones(96, device=DEV), torch.zeros(96, device=DEV), 1e-5), pk, None)]
    for i, f in enumerate(bad):
        with pytest.raises(ValueError):
            f()
    torch.cuda.synchronize()
