"""The gate of tests/test_gpu_swin_grade.py tested on the CPU, against a torch emulation of the Swin kernels' precision contract
(tests/swin_cases.py): on every token-GEMM case of the GPU file and on the one-window attention cases the unbroken emulation passes
grade() - so the gate is reachable by the contract alone, measured against the fp32 CPU path and not against a kernel - and each single
lost term (one cross term of the token GEMM, the cross terms of q k^T, the lo plane of P or of V, one scale per 64-row tile where the
contract has one per row) fails it.  Cases wider than 768 columns run here on their first 768 (the suite without a GPU stays quick)."""

import pytest
import torch

import parity
import swin_cases as sc

N_MAX = 768
TOKEN = [(name, dict(kw, N=min(kw["N"], N_MAX))) for name, kw, _ in sc.token_cases()]
ONE_WINDOW = sc.ONE_WINDOW + [dict(H=7, W=7, heads=3, B=2, window=7, shift=0, kind="sharp", seed=71)]


@pytest.mark.parametrize("kw", [kw for _, kw in TOKEN], ids=[name for name, _ in TOKEN])
def test_token_gate_passes_the_contract_and_fails_every_lost_term(kw):
    c = sc.token_case(**kw)
    assert c.R <= 200 and c.N <= N_MAX
    sc.grade(sc.emulated_token_linear(c), c.want64, c.want32, c.label + " emulated", row_self=c.row_self)
    for drop in ("lo.hi", "hi.lo"):
        with pytest.raises(AssertionError):
            sc.grade(sc.emulated_token_linear(c, drop=drop), c.want64, c.want32, f"{c.label} without {drop}", row_self=c.row_self)
    if c.kind == "spread":
        # One scale per 64-row tile: fp16 is a floating-point format, so a row 2^-k below its tile's largest keeps hi's 11 bits down to
        # k = 28 and lo's down to k = 17 (5.1 decades).  The 1e-3 .. 1e3 case puts 4.97 decades into rows 0 .. 63: the defect costs the
        # quietest rows 1.7 - 6 x the contract's own figure there and stays inside fp32 grade (measured: 5.3e-7 against fp32's 3.0e-7).  At
        # 1e-6 .. 1e6 (9.9 decades in the tile) the quiet rows lose their lo plane and then hi's bits: that is the case that must fail.
        tile = sc.emulated_token_linear(c, row_scale="tile64")
        view = lambda t: t.reshape(-1, 1, c.N)   # noqa: E731
        assert parity.errors(view(tile), view(c.want64)).traj > parity.errors(view(sc.emulated_token_linear(c)), view(c.want64)).traj
        if kw.get("decades", 3.0) >= 6.0:
            with pytest.raises(AssertionError):
                sc.grade(tile, c.want64, c.want32, c.label + " one scale per 64 rows", row_self=True)
            # ... which the figures relative to the whole tensor do not see: the call on each row against itself is what catches it
            sc.grade(tile, c.want64, c.want32, c.label + " one scale per 64 rows, whole tensor")


@pytest.mark.parametrize("kw", ONE_WINDOW, ids=lambda kw: f"heads{kw['heads']}-{kw['kind']}")
def test_attention_gate_passes_the_contract_and_fails_every_lost_plane(kw):
    c = sc.attention_case(**kw)
    sc.grade(sc.emulated_attention(c), c.want64, c.want32, c.label + " emulated")
    for site in ("qk", "p_lo", "v_lo"):
        with pytest.raises(AssertionError):
            sc.grade(sc.emulated_attention(c, drop_site=site), c.want64, c.want32, f"{c.label} without {site}")


def test_a_nan_fails_the_gate():
    c = sc.token_case(R=5, K=32, N=7, seed=3)
    got = c.want32.clone()
    sc.grade(got, c.want64, c.want32, "the fp32 path against itself")
    got[2, 3] = float("nan")
    assert parity.errors(got[None], c.want64[None]).row == float("inf")
    with pytest.raises(AssertionError):
        sc.grade(got, c.want64, c.want32, "one NaN")
    with pytest.raises(AssertionError):
        sc.grade(got, c.want64, c.want32, "one NaN, row by row", row_self=True)


def test_scale_and_split_follow_the_kernels_rule():
    amax = torch.tensor([0.0, 1.0, 0.75, 8192.0, 16383.0, 16384.0, 3e-5, 1e30])
    s = sc.scale_of(amax)
    assert s[0] == 1.0
    prod = (amax * s)[1:]
    assert ((prod >= 8192) & (prod < 16384)).all()
    assert (torch.frexp(s)[0] == 0.5).all()                                  # powers of two
    x = torch.randn(1000) * 3.0
    hi, lo = sc.split(x, sc.scale_of(x.abs().amax()))
    xs = x.double() * float(sc.scale_of(x.abs().amax()))
    assert float(((hi + lo) - xs).abs().max()) <= 2.0 ** -11 * 2.0 ** -11 * 16384      # 22 bits of the row's largest value
    a, b = torch.randn(5, 64), torch.randn(64, 9)
    sa, sb = sc.scale_of(a.abs().amax(1, keepdim=True)), sc.scale_of(b.abs().amax(0, keepdim=True))
    full = sc.split_matmul(a, sa, b, sb)
    want = a.double() @ b.double()
    assert float((full - want).norm() / want.norm()) < 1e-6
    for drop in ("lo.hi", "hi.lo"):
        assert float((sc.split_matmul(a, sa, b, sb, drop) - want).norm() / want.norm()) > 1e-5


@pytest.mark.parametrize("H,W,window,shift", [(13, 9, 7, 3), (6, 10, 4, 2), (9, 20, 8, 0)])
def test_restated_window_attention_is_the_module(H, W, window, shift):
    """window_attention_from_qkv (the "v_spread" oracle) against _ShiftedWindowAttention on a padded, shifted map, in fp64."""
    c = sc.attention_case(H, W, 3, 2, window, shift, "plain", seed=5)
    got = sc.window_attention_from_qkv(c.module.double(), c.qkv.double())
    assert float((got - c.want64).abs().max()) < 1e-6     # qkv is the fp32 rounding of the module's own
    c.module.float()


def test_v_spread_scales_the_images_apart():
    c = sc.attention_case(14, 14, 12, 3, 7, 3, "v_spread", seed=9)
    norms = c.want64.flatten(1).norm(dim=1)
    assert 30 < float(norms[1] / norms[0]) < 300 and 30 < float(norms[2] / norms[1]) < 300   # 100 x apart, image by image
    assert torch.isfinite(c.want64).all()


def test_sharp_logits_reach_the_tens_and_fp32_stays_well_behaved():
    """The "sharp" case of the GPU file: its logits reach the tens, and the fp32 CPU path's own figures stay below 1e-5 (so SHARP_GAIN stands)."""
    c = sc.attention_case(13, 9, 6, 2, 7, 3, "sharp", seed=40)
    C = c.C
    q, k = c.qkv[..., :C].reshape(-1, 6, 32), c.qkv[..., C:2 * C].reshape(-1, 6, 32)
    logits = torch.einsum("thd,shd->hts", q, k) * 32 ** -0.5
    assert 10.0 < float(logits.abs().max()) < 200.0
    e32 = parity.errors(c.want32.reshape(c.B, -1, C), c.want64.reshape(c.B, -1, C))
    print(parity.report(c.label + " fp32 itself", e32, e32))
    assert max(e32) < 1e-5
