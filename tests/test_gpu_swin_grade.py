"""The Swin inference kernels (csrc/sd_swin.hip) held to fp32 grade token by token: every figure of tests/parity.py - the whole tensor,
each image, each token - at most parity.FACTOR x the figure the fp32 CPU path makes against fp64 on the same inputs, + parity.FLOOR.
tests/test_gpu_swin.py gates max|got - want| / max|want| at 1e-4, about 1000 x above what the kernels' contract gives: a lost cross term,
a lost lo plane or a quiet row passes there or nearly so.  tests/test_cpu_swin_grade.py shows on the CPU that this gate is reachable by the
contract alone and fails on each of those defects.  Beyond the gate: the edges of the kernels' stated range (one row, a full tile, one
row past it; 1 / 31 / 32 / 33 / 37 columns; one k-step, the LayerNorm prologue's limit; windows 4 and 8; 24 heads; maps of one token), a
zero row, frames and rows that do not depend on their neighbours bit for bit, repeat calls, parameters at 4-byte aligned addresses.

Every gated tensor prints one line (python -m pytest -s; profiles/swin_parity.txt is that output)."""

import copy
import functools

import pytest
import torch
from torch import nn

import swin_cases as sc

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    from soccerdiffusion_amd import ops as o

    return o


def _dev(t):
    return None if t is None else t.to(DEV)


def _off1(t):
    """`t` on the device as a view that starts one float into a flat buffer: 4-byte aligned and not 16, as a parameter inside an
    optimizer's flat buffer."""
    flat = torch.empty(t.numel() + 1, dtype=t.dtype, device=DEV)
    v = flat[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


# ---- a. token GEMM -------------------------------------------------------------------------------------------------------------------
TOKEN = sc.token_cases()


def _run_token(ops, c, inplace=False, A=None, pk=None):
    pk = ops.PackedTokenLinear(c.W.to(DEV)) if pk is None else pk
    kw = dict(ln=(c.lw.to(DEV), c.lb.to(DEV), sc.EPS) if c.ln else None, gelu=c.gelu)
    A = c.A.to(DEV) if A is None else A
    if inplace:
        io = c.res.to(DEV)
        out = ops.token_linear(A, pk, _dev(c.b), res=io, out=io, **kw)
        assert out.data_ptr() == io.data_ptr()
        return out
    return ops.token_linear(A, pk, _dev(c.b), res=_dev(c.res), **kw)


@pytest.mark.parametrize("kw,inplace", [(kw, ip) for _, kw, ip in TOKEN], ids=[name for name, _, _ in TOKEN])
def test_token_linear_is_fp32_grade(ops, kw, inplace):
    c = sc.token_case(**kw)
    got = _run_token(ops, c, inplace)
    assert got.shape == (c.R, c.N)
    if c.zero is not None:   # a zero row: scale 1, accumulators 0 - the output row is the bias, bit for bit
        assert torch.equal(got[c.zero].cpu(), c.b)
    sc.grade(got, c.want64, c.want32, c.label + (" in place" if inplace else ""), row_self=c.row_self)


@pytest.mark.parametrize("H,W,C", [(7, 5, 96), (13, 14, 192), (1, 1, 96), (3, 3, 384)])
def test_patch_merging_is_fp32_grade(ops, H, W, C):
    from soccerdiffusion_amd.ml.model.encoder.image import _PatchMerging

    torch.manual_seed(H * W + C)
    m = sc.randomise(_PatchMerging(C), C)
    x = torch.randn(2, H, W, C)
    with torch.no_grad():
        want64, want32 = copy.deepcopy(m).double()(x.double()), m(x)
    md = m.to(DEV)
    got = ops.token_merge_linear(x.to(DEV), ops.PackedTokenLinear(md.reduction.weight), (md.norm.weight, md.norm.bias, 1e-5))
    assert got.shape == want64.shape
    sc.grade(got, want64, want32, f"merge {H}x{W} C{C}")


# ---- b. window attention ---------------------------------------------------------------------------------------------------------------
def _attention_cases():
    out = []
    for H, W, heads, B, kinds in [(1, 1, 3, 2, ("plain",)), (2, 3, 3, 2, ("plain",)), (7, 7, 24, 2, ("plain",)), (8, 8, 3, 2, ("plain",)),
                                  (13, 9, 6, 2, ("plain", "sharp")), (14, 14, 12, 1, ("plain",)), (28, 28, 6, 1, ("plain",))]:
        out += [(H, W, heads, B, 7, shift, kind) for kind in kinds for shift in (0, 3)]
    out += [(H, W, 3, 2, 8, shift, "plain") for H, W in ((16, 16), (9, 20)) for shift in (0, 4)]   # 64 tokens: no empty slot
    out += [(6, 10, 3, 2, 4, 2, "plain")]
    out += [(14, 14, 12, 3, 7, shift, "v_spread") for shift in (0, 3)]   # images 1e-2 / 1 / 1e2: the per-image figure is what matters
    return out


def _run_attention(ops, c, bias=None, table=None):
    m = c.module
    return ops.swin_window_attention(c.qkv.to(DEV), c.heads, c.window, c.shift, m.qkv.bias.detach().to(DEV) if bias is None else bias,
                                     m.relative_position_bias_table.detach().to(DEV) if table is None else table,
                                     m.relative_position_index.to(DEV))


@pytest.mark.parametrize("H,W,heads,B,window,shift,kind", _attention_cases(),
                         ids=lambda v: v if isinstance(v, str) else None)
def test_window_attention_is_fp32_grade(ops, H, W, heads, B, window, shift, kind):
    c = sc.attention_case(H, W, heads, B, window, shift, kind, seed=H * W + heads + shift)
    got = _run_attention(ops, c)
    assert got.shape == (B, H, W, c.C)
    sc.grade(got, c.want64, c.want32, c.label)


# ---- c. stem and head --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,H,W", [(1, 31, 45), (3, 96, 100)])
def test_patch_embed_is_fp32_grade(ops, N, H, W):
    from soccerdiffusion_amd.ml.model.encoder.image import _Permute

    g = torch.Generator().manual_seed(H + W)
    torch.manual_seed(H)
    stem = sc.randomise(nn.Sequential(nn.Conv2d(3, 96, 4, 4), _Permute([0, 2, 3, 1]), nn.LayerNorm(96, eps=1e-5)), H)
    x = torch.rand(N, 3, H, W, generator=g) * 2.0 - 0.7
    with torch.no_grad():
        want64, want32 = copy.deepcopy(stem).double()(x.double()), stem(x)
    s = stem.to(DEV)
    got = ops.swin_patch_embed(x.to(DEV), s[0].weight.detach(), s[0].bias.detach(), (s[2].weight.detach(), s[2].bias.detach(), 1e-5))
    assert got.shape == want64.shape
    sc.grade(got, want64, want32, f"patch embed {N}x{H}x{W}")


@pytest.mark.parametrize("H,W,hidden", [(7, 7, 64), (1, 1, 37)])
def test_head_is_fp32_grade(ops, H, W, hidden):
    torch.manual_seed(hidden + H)
    norm, head = sc.randomise(nn.LayerNorm(768, eps=1e-5), 1), sc.randomise(nn.Linear(768, hidden), 2)
    x = torch.randn(3, H, W, 768) + 0.3
    with torch.no_grad():
        want32 = head(norm(x).mean(dim=(1, 2)))
        want64 = copy.deepcopy(head).double()(copy.deepcopy(norm).double()(x.double()).mean(dim=(1, 2)))
    norm, head = norm.to(DEV), head.to(DEV)
    got = ops.swin_head(x.to(DEV), (norm.weight, norm.bias, 1e-5), ops.PackedTokenLinear(head.weight), head.bias)
    assert got.shape == (3, hidden)
    sc.grade(got.view(3, 1, hidden), want64.view(3, 1, hidden), want32.view(3, 1, hidden), f"head {H}x{W} -> {hidden}")


# ---- d. the encoder end to end -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _encoder(kind, seed):
    """(the encoder on the CPU, a copy on the device): parameters randomised, shared by the tests below and left unchanged."""
    from soccerdiffusion_amd.ml.model.encoder.image import ImageEncoderType, image_encoder_factory

    torch.manual_seed(seed)
    enc = sc.randomise(image_encoder_factory(getattr(ImageEncoderType, kind), 64, True, 96), seed).eval()
    return enc, copy.deepcopy(enc).to(DEV)


def _frames(*shape, seed=5):
    return torch.rand(*shape, generator=torch.Generator().manual_seed(seed)) * 2.0 - 0.7


@pytest.mark.parametrize("kind,H,W", [("SWIN_TRANSFORMER_TINY", 96, 96), ("SWIN_TRANSFORMER_TINY", 64, 128), ("SWIN_TRANSFORMER_SMALL", 96, 96)])
def test_swin_encoder_is_fp32_grade(kind, H, W):
    enc, dev = _encoder(kind, H + W)
    x = _frames(2, 2, 3, H, W)
    with torch.no_grad():
        want64, want32 = copy.deepcopy(enc).double()(x.double()), enc(x)
        got = dev(x.to(DEV))
    assert got.shape == (2, 2, 64)
    sc.grade(got.reshape(4, 1, 64), want64.reshape(4, 1, 64), want32.reshape(4, 1, 64), f"{kind.lower()} {H}x{W}")


# ---- e. / f. independence of the neighbours and repeat calls, bit for bit ----------------------------------------------------------------
def test_a_frames_token_does_not_depend_on_the_frames_beside_it():
    """PolicySession encodes a frame once, on arrival, in whatever batch it arrives in: six frames at once, one at a time and in reversed
    order give every frame's token the same bits (and so does the same call again)."""
    _, dev = _encoder("SWIN_TRANSFORMER_TINY", 192)
    x = _frames(1, 6, 3, 96, 96, seed=8).to(DEV)
    with torch.no_grad():
        together = dev(x)
        again = dev(x)
        alone = torch.cat([dev(x[:, i:i + 1]) for i in range(6)], 1)
        backwards = dev(x.flip(1).contiguous()).flip(1)
    assert together.shape == (1, 6, 64) and torch.isfinite(together).all()
    assert not torch.equal(together[0, 0], together[0, 1])   # (six different frames)
    assert torch.equal(together, again)
    assert torch.equal(together, alone)
    assert torch.equal(together, backwards)


@pytest.mark.parametrize("K,N,ln,gelu", [(96, 288, True, False), (384, 37, False, True), (3072, 768, False, False)])
def test_a_token_linear_row_does_not_depend_on_its_place(ops, K, N, ln, gelu):
    """Rows 0 .. 76 computed alone equal rows 100 .. 176 of a 200-row call that holds them there (another tile, another place in it,
    other neighbours), and a repeat call gives the same bytes."""
    c = sc.token_case(77, K, N, ln=ln, gelu=gelu, seed=K + N)
    pk = ops.PackedTokenLinear(c.W.to(DEV))
    big = torch.randn(200, K, generator=torch.Generator().manual_seed(1)) * 5.0
    big[100:177] = c.A
    alone, again = _run_token(ops, c, pk=pk), _run_token(ops, c, pk=pk)
    held = _run_token(ops, c, A=big.to(DEV), pk=pk)
    assert torch.equal(alone, again)
    assert torch.equal(alone, held[100:177])
    sc.grade(alone, c.want64, c.want32, c.label + " alone")


def test_window_attention_repeats_and_keeps_images_apart(ops):
    c = sc.attention_case(13, 9, 6, 3, 7, 3, "plain", seed=77)
    got, again = _run_attention(ops, c), _run_attention(ops, c)
    assert torch.equal(got, again)
    m = c.module
    one = ops.swin_window_attention(c.qkv[1:2].contiguous().to(DEV), c.heads, 7, 3, m.qkv.bias.detach().to(DEV),
                                    m.relative_position_bias_table.detach().to(DEV), m.relative_position_index.to(DEV))
    assert torch.equal(got[1:2], one)


# ---- g. parameters that are only 4-byte aligned -----------------------------------------------------------------------------------------
def test_unaligned_token_linear_parameters_give_the_same_bits(ops):
    for kw in (dict(R=77, K=96, N=37, ln=True, gelu=True), dict(R=65, K=384, N=96, res=True)):
        c = sc.token_case(seed=11, **kw)
        want = _run_token(ops, c)
        pk = ops.PackedTokenLinear(_off1(c.W))
        ln = (_off1(c.lw), _off1(c.lb), sc.EPS) if c.ln else None
        got = ops.token_linear(c.A.to(DEV), pk, _off1(c.b), ln=ln, gelu=c.gelu, res=_dev(c.res))
        assert torch.equal(got, want)
        pk.refresh(_off1(c.W))
        assert torch.equal(ops.token_linear(c.A.to(DEV), pk, _off1(c.b), ln=ln, gelu=c.gelu, res=_dev(c.res)), want)


def test_unaligned_attention_parameters_give_the_same_bits(ops):
    c = sc.attention_case(13, 9, 6, 2, 7, 3, "plain", seed=78)   # a padded map: the bias is read as the padding tokens' q / k / v
    want = _run_attention(ops, c)
    got = _run_attention(ops, c, bias=_off1(c.module.qkv.bias.detach()), table=_off1(c.module.relative_position_bias_table.detach()))
    assert torch.equal(got, want)


def test_unaligned_stem_merge_and_head_parameters_give_the_same_bits(ops):
    g = torch.Generator().manual_seed(3)
    x = (torch.rand(2, 3, 31, 45, generator=g) * 2.0 - 0.7).to(DEV)
    w, b = torch.randn(96, 3, 4, 4, generator=g) * 0.2, torch.randn(96, generator=g)
    lw, lb = 0.5 + torch.rand(96, generator=g), torch.randn(96, generator=g)
    want = ops.swin_patch_embed(x, w.to(DEV), b.to(DEV), (lw.to(DEV), lb.to(DEV), 1e-5))
    assert torch.equal(ops.swin_patch_embed(x, _off1(w), _off1(b), (_off1(lw), _off1(lb), 1e-5)), want)
    # patch merging: LayerNorm over 4 C and the reduction weight
    t = torch.randn(2, 7, 5, 96, generator=g).to(DEV)
    rw, nw, nb = torch.randn(192, 384, generator=g) * 0.05, 0.5 + torch.rand(384, generator=g), torch.randn(384, generator=g)
    want = ops.token_merge_linear(t, ops.PackedTokenLinear(rw.to(DEV)), (nw.to(DEV), nb.to(DEV), 1e-5))
    assert torch.equal(ops.token_merge_linear(t, ops.PackedTokenLinear(_off1(rw)), (_off1(nw), _off1(nb), 1e-5)), want)
    # the head: LayerNorm + mean, then the Linear
    h = torch.randn(3, 2, 3, 768, generator=g).to(DEV)
    hw, hb = torch.randn(37, 768, generator=g) * 0.03, torch.randn(37, generator=g)
    fw, fb = 0.5 + torch.rand(768, generator=g), torch.randn(768, generator=g)
    want = ops.swin_head(h, (fw.to(DEV), fb.to(DEV), 1e-5), ops.PackedTokenLinear(hw.to(DEV)), hb.to(DEV))
    assert torch.equal(ops.swin_head(h, (_off1(fw), _off1(fb), 1e-5), ops.PackedTokenLinear(_off1(hw)), _off1(hb)), want)
    torch.cuda.synchronize()
