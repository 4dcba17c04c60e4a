"""Inputs, fp64 / fp32 CPU oracles and a torch emulation of the precision contract for the Swin inference kernels (csrc/sd_swin.hip) - a
plain helper module, not a conftest.  tests/test_cpu_swin_grade.py holds the gate itself to the emulation (the contract alone passes it,
every single lost term fails it); tests/test_gpu_swin_grade.py holds the kernels to the same gate on the same inputs.

The contract (sd_swin.hip): every product on split fp16 operands, x s = hi + lo with s a power of two, as lo.hi +
hi.lo + hi.hi; one scale per weight row, one per activation row, one per operand tile of a (window, head) in the attention; LayerNorm,
GELU and softmax in fp32.  The emulation accumulates in fp64, so what it measures is the contract's own error and no accumulation order."""

from __future__ import annotations

import copy
from types import SimpleNamespace

import torch
import torch.nn.functional as F
from torch import nn

import parity

EPS = 1e-5


# ---- the gate ----------------------------------------------------------------------------------------------------------------------
def grade(got, want64, want32, label, factor=parity.FACTOR, floor=parity.FLOOR, row_self=False):
    """parity.assert_fp32_grade on (images or 1, rows, features): the global, per-image and per-token figures of `got` against the fp32 CPU
    path's own on the same inputs.  A tensor of three or more dimensions is (images, ..., features), a matrix is one image.
    `row_self` adds the call on (rows, 1, features), whose `traj` figure is each row's error relative to that row itself - for cases
    without bias and residual only ("spread"): behind either a row's own norm says nothing about the product."""
    feat = want64.shape[-1]
    images = want64.shape[0] if want64.dim() >= 3 else 1
    view = lambda t: t.detach().cpu().reshape(images, -1, feat)   # noqa: E731
    e = parity.assert_fp32_grade(view(got), view(want64), view(want32), factor=factor, floor=floor, label=label)
    if row_self:
        rows = lambda t: t.detach().cpu().reshape(-1, 1, feat)   # noqa: E731
        parity.assert_fp32_grade(rows(got), rows(want64), rows(want32), factor=factor, floor=floor, label=label + " [row / itself]")
    return e


def randomise(mod: nn.Module, seed: int) -> nn.Module:
    """As test_gpu_swin._randomise: the parameters that default to trivial values get values a bias, mask or LayerNorm bug cannot hide behind."""
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


# ---- token GEMM --------------------------------------------------------------------------------------------------------------------
TOKEN_KINDS = ("plain", "spread", "offset", "zero_row")


def _token_ref(c, dt):
    x = c.A.to(dt)
    if c.ln:
        x = F.layer_norm(x, (c.K,), c.lw.to(dt), c.lb.to(dt), EPS)
    y = x @ c.W.to(dt).T
    if c.b is not None:
        y = y + c.b.to(dt)
    if c.gelu:
        y = F.gelu(y)
    if c.res is not None:
        y = y + c.res.to(dt)
    return y


def token_case(R, K, N, ln=False, gelu=False, res=False, kind="plain", seed=0, decades=3.0):
    """out (R, N) = [+ res] [gelu] (LayerNorm?(A) W^T + b): fp32 inputs, `want64` the operation in fp64 on the CPU, `want32` the same
    lines in fp32.  kind: "plain" A = 2 randn + 0.5; "spread" the rows of A times logspace(-decades, decades, R), no LayerNorm, bias or
    residual (the per-row scale's case, graded row by row against the row itself); "offset" A = 30 + randn under the LayerNorm (the row pass's
    two-pass statistics); "zero_row" plain with row R // 2 zeroed."""
    if kind not in TOKEN_KINDS:
        raise ValueError(kind)
    g = torch.Generator().manual_seed(seed)
    A = torch.randn(R, K, generator=g) * 2.0 + 0.5
    W = torch.randn(N, K, generator=g) * K ** -0.5
    b = torch.randn(N, generator=g)
    lw, lb = 0.5 + torch.rand(K, generator=g), torch.randn(K, generator=g)
    r = torch.randn(R, N, generator=g)
    zero = None
    if kind == "spread":
        if ln or res:
            raise ValueError("'spread' runs without LayerNorm, bias and residual")
        A = A * torch.logspace(-decades, decades, R)[:, None]
        b = None
    elif kind == "offset":
        if not ln:
            raise ValueError("'offset' is the LayerNorm prologue's case")
        A = 30.0 + torch.randn(R, K, generator=g)
    elif kind == "zero_row":
        zero = R // 2
        A[zero] = 0.0
    c = SimpleNamespace(R=R, K=K, N=N, ln=bool(ln), gelu=bool(gelu), kind=kind, A=A, W=W, b=b, lw=lw if ln else None, lb=lb if ln else None,
                        res=r if res else None, zero=zero, row_self=kind == "spread",
                        label=f"token R{R} K{K} N{N}{' ln' if ln else ''}{' gelu' if gelu else ''}{' res' if res else ''} {kind}"
                              + (f" 1e+-{decades:g}" if kind == "spread" and decades != 3.0 else ""))
    c.want64, c.want32 = _token_ref(c, torch.float64), _token_ref(c, torch.float32)
    return c


# ---- window attention --------------------------------------------------------------------------------------------------------------
ATTN_KINDS = ("plain", "sharp", "v_spread")
SHARP_GAIN = 4.0   # logits x 16: tens.  The fp32 CPU path's own error stays near 1e-6 at this gain (test_cpu_swin_grade checks < 1e-5)


def window_attention_from_qkv(m, qkv):
    """_ShiftedWindowAttention.forward before proj, restated from the qkv rows (B, H, W, 3 C) of the un-padded map (a padding position holds
    qkv(0) = the bias: the module pads behind norm1), in qkv's dtype.  The oracle of the "v_spread" case, where the kernel's input is
    no x W^T + b; test_cpu_swin_grade holds it to the module itself."""
    B, H, W, C3 = qkv.shape
    C, w, heads, dt = C3 // 3, m.window, m.heads, qkv.dtype
    pad_r, pad_b = (w - W % w) % w, (w - H % w) % w
    full = m.qkv.bias.detach().to(dt).expand(B, H + pad_b, W + pad_r, C3).clone()
    full[:, :H, :W] = qkv
    pH, pW = H + pad_b, W + pad_r
    sh = [0 if w >= pH else m.shift, 0 if w >= pW else m.shift]
    if sum(sh) > 0:
        full = torch.roll(full, shifts=(-sh[0], -sh[1]), dims=(1, 2))
    nW = (pH // w) * (pW // w)
    x = full.view(B, pH // w, w, pW // w, w, C3).permute(0, 1, 3, 2, 4, 5).reshape(B * nW, w * w, 3, heads, C // heads).permute(2, 0, 3, 1, 4)
    q, k, v = x[0] * (C // heads) ** -0.5, x[1], x[2]
    attn = q @ k.transpose(-2, -1)
    bias = m.relative_position_bias_table.detach().to(dt)[m.relative_position_index].view(w * w, w * w, -1).permute(2, 0, 1)
    attn = attn + bias.unsqueeze(0)
    if sum(sh) > 0:
        mask = full.new_zeros((pH, pW))
        count = 0
        for h0, h1 in ((0, -w), (-w, -sh[0]), (-sh[0], None)):
            for w0, w1 in ((0, -w), (-w, -sh[1]), (-sh[1], None)):
                mask[h0:h1, w0:w1] = count
                count += 1
        mask = mask.view(pH // w, w, pW // w, w).permute(0, 2, 1, 3).reshape(nW, w * w)
        mask = mask.unsqueeze(1) - mask.unsqueeze(2)
        mask = mask.masked_fill(mask != 0, -100.0).masked_fill(mask == 0, 0.0)
        attn = (attn.view(B, nW, heads, w * w, w * w) + mask.unsqueeze(1).unsqueeze(0)).view(-1, heads, w * w, w * w)
    o = (attn.softmax(dim=-1) @ v).transpose(1, 2).reshape(B * nW, w * w, C)
    o = o.view(B, pH // w, pW // w, w, w, C).permute(0, 1, 3, 2, 4, 5).reshape(B, pH, pW, C)
    if sum(sh) > 0:
        o = torch.roll(o, shifts=(sh[0], sh[1]), dims=(1, 2))
    return o[:, :H, :W, :].contiguous()


def attention_case(H, W, heads, B, window=7, shift=0, kind="plain", seed=0):
    """The shifted-window attention before proj on a (B, H, W, 32 heads) map.  Oracle: _ShiftedWindowAttention with proj = Identity,
    randomised, deep-copied to fp64 (`want64`) and run in fp32 (`want32`); the kernel's input is qkv = (x64 W64^T + b64).float().
    kind: "sharp" multiplies the q and k rows of qkv.weight by SHARP_GAIN; "v_spread" scales the v third of image n's qkv rows by
    10^(2 n - 2) and takes both oracles from that qkv through window_attention_from_qkv (what the kernel sees, exactly)."""
    from soccerdiffusion_amd.ml.model.encoder.image import _ShiftedWindowAttention

    if kind not in ATTN_KINDS:
        raise ValueError(kind)
    C = 32 * heads
    torch.manual_seed(seed)   # (the module's own initialisation)
    m = randomise(_ShiftedWindowAttention(C, window, shift, heads), seed + 1)
    m.proj = nn.Identity()   # the kernel stops before proj
    g = torch.Generator().manual_seed(seed + 2)
    x = torch.randn(B, H, W, C, generator=g)
    with torch.no_grad():
        if kind == "sharp":
            m.qkv.weight[: 2 * C] *= SHARP_GAIN
        m64 = copy.deepcopy(m).double()
        qkv64 = x.double() @ m64.qkv.weight.T + m64.qkv.bias
        if kind == "v_spread":
            qkv64[..., 2 * C:] *= (10.0 ** (2.0 * torch.arange(B, dtype=torch.float64) - 2.0)).view(B, 1, 1, 1)
            qkv = qkv64.float()
            want64, want32 = window_attention_from_qkv(m64, qkv.double()), window_attention_from_qkv(m, qkv)
        else:
            qkv = qkv64.float()
            want64, want32 = m64(x.double()), m(x)
    return SimpleNamespace(H=H, W=W, heads=heads, B=B, C=C, window=window, shift=shift, kind=kind, module=m, x=x, qkv=qkv.contiguous(),
                           want64=want64, want32=want32, label=f"attention {H}x{W} heads{heads} B{B} w{window} s{shift} {kind}")


# ---- the contract in torch on the CPU ------------------------------------------------------------------------------------------------
def scale_of(amax: torch.Tensor) -> torch.Tensor:
    """The power of two s with amax * s in [8192, 16384), 1 for zero (f16_scale_from_bits: amax = f 2^e, f in [0.5, 1): s = 2^(14 - e))."""
    amax = torch.as_tensor(amax, dtype=torch.float32)
    _, e = torch.frexp(amax)
    s = torch.ldexp(torch.ones_like(amax), 14 - e)
    return torch.where(amax > 0, s, torch.ones_like(s))


def split(x: torch.Tensor, s):
    """hi = fp16(x s), lo = fp16(x s - hi) of fp32 x (both steps before the roundings are exact in fp32), returned in fp64."""
    xs = x.float() * torch.as_tensor(s, dtype=torch.float32)
    hi = xs.half()
    lo = (xs - hi.float()).half()
    return hi.double(), lo.double()


DROPS = (None, "lo.hi", "hi.lo", "both")


def split_matmul(a, sa, b, sb, drop=None):
    """a (M, K) . b (K, N) on split operands, lo.hi + hi.lo + hi.hi accumulated in fp64 and un-scaled: `sa` broadcasts against a (one
    scale per row: (M, 1)), `sb` against b (one per column: (1, N)).  `drop` leaves one cross term out ("both": the two of them)."""
    if drop not in DROPS:
        raise ValueError(drop)
    ah, al = split(a, sa)
    bh, bl = split(b, sb)
    acc = ah @ bh
    if drop not in ("lo.hi", "both"):
        acc = acc + al @ bh
    if drop not in ("hi.lo", "both"):
        acc = acc + ah @ bl
    return acc / (torch.as_tensor(sa, dtype=torch.float64) * torch.as_tensor(sb, dtype=torch.float64))


def emulated_token_linear(c, drop=None, row_scale="row"):
    """token_gemm_kernel's arithmetic on a token_case: fp32 LayerNorm, the power-of-two scale of every (normalised) row - or, as the defect
    "tile64", one per 64-row tile - and of every weight row, the split product, the fp32 epilogue."""
    x = F.layer_norm(c.A, (c.K,), c.lw, c.lb, EPS) if c.ln else c.A
    amax = x.abs().amax(1, keepdim=True)
    if row_scale == "tile64":
        amax = torch.cat([t.amax().expand(t.shape[0], 1) for t in amax.split(64)])
    elif row_scale != "row":
        raise ValueError(row_scale)
    y = split_matmul(x, scale_of(amax), c.W.T, scale_of(c.W.abs().amax(1))[None, :], drop).float()
    if c.b is not None:
        y = y + c.b
    if c.gelu:
        y = F.gelu(y)
    if c.res is not None:
        y = y + c.res
    return y


DROP_SITES = (None, "qk", "p_lo", "v_lo")


def emulated_attention(c, drop_site=None):
    """swin_attention_kernel's arithmetic on an un-shifted one-window attention_case (map 7 x 7, window 7): per (image, head) one scale for
    each of q 32^-0.5, k and v, S = q k^T split, fp32 bias and softmax, P at the fixed scale 2^14, O = P V split.  drop_site: "qk" q k^T
    without its two cross terms, "p_lo" P without its lo plane, "v_lo" V without its lo plane."""
    if drop_site not in DROP_SITES:
        raise ValueError(drop_site)
    if (c.H, c.W, c.window, c.shift) != (7, 7, 7, 0):
        raise ValueError("the emulation covers one un-shifted window")
    m, T = c.module, 49
    bias = m.relative_position_bias_table.detach()[m.relative_position_index].view(T, T, -1).permute(2, 0, 1)   # (heads, T, T)
    rows = c.qkv.reshape(c.B, T, 3, c.heads, 32)
    out = torch.empty(c.B, T, c.C)
    for n in range(c.B):
        for h in range(c.heads):
            q, k, v = rows[n, :, 0, h] * torch.tensor(32 ** -0.5, dtype=torch.float32), rows[n, :, 1, h], rows[n, :, 2, h]
            sq, sk, sv = scale_of(q.abs().amax()), scale_of(k.abs().amax()), scale_of(v.abs().amax())
            S = split_matmul(q, sq, k.T, sk, "both" if drop_site == "qk" else None).float() + bias[h]
            x = torch.exp(S - S.amax(1, keepdim=True))
            p = x * (16384.0 / x.sum(1, keepdim=True))
            o = split_matmul(p, 1.0, v, sv, {"p_lo": "lo.hi", "v_lo": "hi.lo"}.get(drop_site)) / 16384.0
            out[n, :, 32 * h:32 * h + 32] = o.float()
    return out.view(c.B, 7, 7, c.C)


# ---- the cases both test files run ---------------------------------------------------------------------------------------------------
def token_cases():
    """[(id, token_case keywords, in place)]: the block's GEMMs at both ends of the network at R = 1 / 64 / 65 / 200 (one row, a full
    row tile, one row past it, a ragged fourth tile), the column edges around the 32 columns of a wave, the depth edges (one k-step, the
    LayerNorm prologue's limit, the deepest fc2) and the kinds."""
    out = []
    block = [(96, 288, dict(ln=True), False), (96, 96, dict(res=True), True), (96, 384, dict(ln=True, gelu=True), False),
             (384, 96, dict(res=True), False), (768, 2304, dict(ln=True), False), (3072, 768, dict(res=True), False)]
    for K, N, opt, inplace in block:
        for R in (1, 64, 65, 200):
            out.append((dict(R=R, K=K, N=N, **opt), inplace))
    for N in (1, 31, 32, 33, 37):
        out.append((dict(R=77, K=96, N=N), False))
    out += [(dict(R=77, K=32, N=96), False), (dict(R=77, K=1536, N=96, ln=True), False), (dict(R=77, K=3072, N=96), False),
            (dict(R=77, K=384, N=384, kind="spread"), False), (dict(R=77, K=3072, N=768, kind="spread"), False),
            (dict(R=77, K=384, N=384, kind="spread", decades=6.0), False),
            (dict(R=77, K=768, N=2304, ln=True, kind="offset"), False), (dict(R=77, K=384, N=96, kind="zero_row"), False)]
    named = []
    for i, (kw, inplace) in enumerate(out):
        kw = dict(dict(ln=False, gelu=False, res=False, kind="plain"), **kw, seed=1000 + i)
        name = f"R{kw['R']}-K{kw['K']}-N{kw['N']}" + "".join(f"-{o}" for o in ("ln", "gelu", "res") if kw[o]) + ("" if kw["kind"] == "plain" else "-" + kw["kind"]) + ("-wide" if "decades" in kw else "")
        named.append((name, kw, inplace))
    return named


ONE_WINDOW = [dict(H=7, W=7, heads=24, B=2, window=7, shift=0, kind="plain", seed=70)]   # the attention cases emulated_attention covers
