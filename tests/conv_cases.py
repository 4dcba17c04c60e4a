"""Inputs, fp64 / fp32 CPU oracles and a torch emulation of the precision contract for the ResNet backbone kernels (csrc/sd_conv.hip,
csrc/sd_conv_train.hip, csrc/sd_head.hip, conv_training.py) - a plain helper module, not a conftest.  tests/test_cpu_conv_grade.py holds
the gate itself to the emulation (the contract alone passes it on every case, every single defect fails it);
tests/test_gpu_conv_grade.py holds the kernels to the same gate on the same inputs.

The contract (sd_conv.hip's header): every product of a convolution on split fp16 operands, x s = hi + lo with s the
power of two that puts the TENSOR's abs-max into [8192, 16384) (f16_scale_from_bits on the abs-max word), as lo.hi + hi.lo + hi.hi.  Both
halves are rounded to nearest (f16_split4 and the pack kernels: `(f16)v`; the packed round-toward-zero split f16_split4_pk is not used
by these kernels - `rtz=True` emulates it), lo lands on fp16's subnormal quantum 2^-24 where it is small.  The per-wave weight gradient
without abs-max words takes one scale per operand, per 64-channel tile and per 32 output pixels of an image row instead.  The emulation
accumulates in fp64: it measures the contract's own error and no accumulation order.  BatchNorm, the pool and the heads are plain fp32
with double partial sums: the fp32 CPU operator is their yardstick directly.

All case tensors are NCHW / torch layout on the CPU in fp32; `want64` / `want32` are torch CPU operators in fp64 / fp32 on those tensors."""

from __future__ import annotations

from types import SimpleNamespace

import torch
import torch.nn.functional as F

import parity

EPS = 1e-5
FLOOR_SHORT = 2.0 ** -20   # contractions of fewer than SHORT_TERMS terms: two operands, each off by at most 2^-21 relative
SHORT_TERMS = 64


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def nchw(t):
    return t.permute(0, 3, 1, 2)


# ---- the gate ----------------------------------------------------------------------------------------------------------------------
def _views_act(t):
    """An NCHW activation as (image, pixel, channel) and as (image, channel, pixel)."""
    t = t.detach().cpu()
    n, c = t.shape[0], t.shape[1]
    v = t.reshape(n, c, -1)
    return v.transpose(1, 2), v


def grade(got, want64, want32, label, factor=parity.FACTOR, floor=parity.FLOOR):
    """An NCHW activation: parity.assert_fp32_grade on (image, pixel, channel) - whole tensor / image / pixel - and again on
    (image, channel, pixel), where one output channel of one image is a row."""
    g, w, w32 = _views_act(got), _views_act(want64), _views_act(want32)
    e = parity.assert_fp32_grade(g[0], w[0], w32[0], factor=factor, floor=floor, label=label)
    parity.assert_fp32_grade(g[1], w[1], w32[1], factor=factor, floor=floor, label=label + " [channel rows]")
    return e


def _views_dw(t):
    t = t.detach().cpu()
    co, ci = t.shape[0], t.shape[1]
    return t.permute(2, 3, 0, 1).reshape(-1, co, ci)   # (tap, co, ci): one tap is an "image"


def grade_dw(got, want64, want32, label, factor=parity.FACTOR, floor=parity.FLOOR, row_self=False):
    """A weight gradient (Cout, Cin, k, k): parity.assert_grads_fp32_grade (rows = output channels), then (tap, co, ci) through
    assert_fp32_grade so that one tap is an "image".  `row_self` ("quiet_channels") adds every output channel against itself."""
    parity.assert_grads_fp32_grade({"dw": got.detach().cpu()}, {"dw": want64}, {"dw": want32}, factor=factor, floor=floor, label=label)
    parity.assert_fp32_grade(_views_dw(got), _views_dw(want64), _views_dw(want32), factor=factor, floor=floor, label=label + " [taps]")
    if row_self:
        rows = lambda t: t.detach().cpu().reshape(t.shape[0], 1, -1)   # noqa: E731
        parity.assert_fp32_grade(rows(got), rows(want64), rows(want32), factor=factor, floor=floor, label=label + " [channel / itself]")


def grade_vec(got: dict, want64: dict, want32: dict, label, factor=parity.FACTOR, floor=parity.FLOOR):
    """Channel vectors (dgamma, dbeta, mean, rstd, running statistics) as 1-D parameters: rows = elements, relative to the vector's rms."""
    return parity.assert_grads_fp32_grade({k: v.detach().cpu() for k, v in got.items()}, want64, want32, factor=factor, floor=floor, label=label)


def tightness(pairs, factor=parity.FACTOR, floor=parity.FLOOR) -> float:
    """max over [(errors of got, errors of the fp32 oracle)] and their figures of error / (factor * fp32's + floor): <= 1 passes."""
    return max(a / (factor * b + floor) for e, e32 in pairs for a, b in zip(e, e32))


def act_pairs(got, want64, want32):
    g, w, w32 = _views_act(got), _views_act(want64), _views_act(want32)
    return [(parity.errors(g[i], w[i]), parity.errors(w32[i], w[i])) for i in (0, 1)]


def dw_pairs(got, want64, want32):
    ge = parity.grad_errors({"dw": got}, {"dw": want64})["dw"]
    ge32 = parity.grad_errors({"dw": want32}, {"dw": want64})["dw"]
    return [(ge, ge32), (parity.errors(_views_dw(got), _views_dw(want64)), parity.errors(_views_dw(want32), _views_dw(want64)))]


def word_value(word) -> float:
    """The float whose bits an abs-max word holds."""
    return float(torch.tensor([int(word.item())], dtype=torch.int32).view(torch.float32))


# ---- the contract in torch on the CPU ------------------------------------------------------------------------------------------------
def scale_of(amax) -> torch.Tensor:
    """f16_scale_from_bits: the power of two s with amax * s in [8192, 16384) from the biased exponent eb of amax (s = 2^(140 - eb)); zero,
    subnormal and < 2^-113 maxima (eb < 14) and non-finite ones (eb = 255) give 1."""
    amax = torch.as_tensor(amax, dtype=torch.float32)
    eb = (amax.contiguous().view(torch.int32) >> 23) & 0xFF
    s = torch.ldexp(torch.ones_like(amax), 140 - eb)
    return torch.where((eb >= 14) & (eb != 255), s, torch.ones_like(s))


def _toward_zero(xs: torch.Tensor) -> torch.Tensor:
    """fp16 of fp32 xs rounded toward zero: where rounding to nearest went away from zero, one step back on the bit pattern."""
    h = xs.half()
    away = h.float().abs() > xs.abs()
    return torch.where(away, (h.view(torch.int16) - 1).view(torch.float16), h)


def split(x: torch.Tensor, s, rtz: bool = False):
    """hi = fp16(x s), lo = fp16(x s - hi) of fp32 x (the subtraction is exact in fp32), in fp64.  fp16 conversion puts a small lo on the
    subnormal quantum 2^-24 as the hardware's does."""
    xs = x.float() * torch.as_tensor(s, dtype=torch.float32)
    cvt = _toward_zero if rtz else torch.Tensor.half
    hi = cvt(xs)
    lo = cvt(xs - hi.float())
    return hi.double(), lo.double()


DROPS = (None, "lo.hi", "hi.lo", "both")   # first operand = the activation / dY, second = the weight / X


def _assemble(prod, a, b, drop, masks):
    """hi.hi + lo.hi + hi.lo of the bilinear `prod` on the split operands a = (hi, lo), b = (hi, lo), minus the cross term(s) `drop`
    confined by masks = (on a, on b, on the output), each None or a 0 / 1 tensor."""
    if drop not in DROPS:
        raise ValueError(drop)
    (ah, al), (bh, bl) = a, b
    out = prod(ah, bh) + prod(al, bh) + prod(ah, bl)
    if drop is None:
        return out
    ma, mb, mo = masks
    m = lambda t, k: t if k is None else t * k   # noqa: E731
    lost = 0.0
    if drop in ("lo.hi", "both"):
        lost = lost + prod(m(al, ma), m(bh, mb))
    if drop in ("hi.lo", "both"):
        lost = lost + prod(m(ah, ma), m(bl, mb))
    return out - m(lost, mo)


def _where_conv(where, x, w, out_shape):
    """Masks of a forward-shaped product (activation x (N, C, H, W), weight w (Co, Ci, k, k)) for `where` = None or one of
    {"channel": co} {"tap": (ky, kx)} {"image": n} {"column": input column} {"pixel": (n, oy, ox)}."""
    ma = mb = mo = None
    if not where:
        return ma, mb, mo
    (key, val), = where.items()
    if key == "channel":
        mb = torch.zeros(w.shape[0], 1, 1, 1, dtype=torch.float64); mb[val] = 1
    elif key == "tap":
        mb = torch.zeros(1, 1, w.shape[2], w.shape[3], dtype=torch.float64); mb[0, 0, val[0], val[1]] = 1
    elif key == "image":
        ma = torch.zeros(x.shape[0], 1, 1, 1, dtype=torch.float64); ma[val] = 1
    elif key == "column":
        ma = torch.zeros(1, 1, 1, x.shape[3], dtype=torch.float64); ma[..., val] = 1
    elif key == "pixel":
        mo = torch.zeros(out_shape[0], 1, out_shape[2], out_shape[3], dtype=torch.float64); mo[val[0], 0, val[1], val[2]] = 1
    else:
        raise ValueError(where)
    return ma, mb, mo


def emulated_conv(x, w, stride=1, drop=None, where=None, rtz=False):
    """conv2d(x, w, stride, padding k // 2) on the contract: one scale per tensor, three products, fp64 accumulation -> fp64.  Any kernel
    size and stride: the 3 x 3 / 1 x 1 kernels of either stride, the data gradient on flipped transposed weights, the stem (k = 7)."""
    sx, sw = scale_of(x.abs().max()), scale_of(w.abs().max())
    prod = lambda a, b: F.conv2d(a, b, stride=stride, padding=w.shape[2] // 2)   # noqa: E731
    out_shape = prod(torch.zeros(x.shape, dtype=torch.float64), torch.zeros(w.shape, dtype=torch.float64)).shape
    acc = _assemble(prod, split(x, sx, rtz), split(w, sw, rtz), drop, _where_conv(where, x, w, out_shape))
    return acc / (sx.double() * sw.double())


def emulated_convt(dy, w, H, W, drop=None, where=None, rtz=False):
    """The input gradient (N, Cin, H, W) of conv2d(., w (Cout, Cin, k, k), stride 2, padding k // 2) from dy - sd_convt3x3_s2 / sd_convt1x1_s2:
    the transposed convolution on the contract (one scale per tensor).  `where`: "image" / "column" / "pixel" refer to dy and the output."""
    sy, sw = scale_of(dy.abs().max()), scale_of(w.abs().max())
    shape = (dy.shape[0], w.shape[1], H, W)
    prod = lambda a, b: torch.nn.grad.conv2d_input(shape, b, a, stride=2, padding=w.shape[2] // 2)   # noqa: E731
    acc = _assemble(prod, split(dy, sy, rtz), split(w, sw, rtz), drop, _where_conv(where, dy, w, shape))
    return acc / (sy.double() * sw.double())


def _where_dw(where, dy, wshape):
    ma = mb = mo = None
    if not where:
        return ma, mb, mo
    (key, val), = where.items()
    if key == "channel":
        ma = torch.zeros(1, dy.shape[1], 1, 1, dtype=torch.float64); ma[0, val] = 1
    elif key == "tap":
        mo = torch.zeros(1, 1, wshape[2], wshape[3], dtype=torch.float64); mo[0, 0, val[0], val[1]] = 1
    elif key == "image":
        ma = torch.zeros(dy.shape[0], 1, 1, 1, dtype=torch.float64); ma[val] = 1
    elif key == "column":
        ma = torch.zeros(1, 1, 1, dy.shape[3], dtype=torch.float64); ma[..., val] = 1
    elif key == "pixel":
        ma = torch.zeros(dy.shape[0], 1, dy.shape[2], dy.shape[3], dtype=torch.float64); ma[val[0], 0, val[1], val[2]] = 1
    else:
        raise ValueError(where)
    return ma, mb, mo


def emulated_wgrad(dy, x, wshape, stride=1, drop=None, where=None, rtz=False):
    """dW of conv2d(x, ., stride, padding k // 2) on the contract with ONE scale per tensor: the strip-walking kernel (3 x 3, both strides),
    the per-wave kernel with abs-max words, the stem (k = 7).  `where`: "channel" = output channel, "tap", "image", "column" / "pixel" of dy."""
    sy, sx = scale_of(dy.abs().max()), scale_of(x.abs().max())
    prod = lambda a, b: torch.nn.grad.conv2d_weight(b, wshape, a, stride=stride, padding=wshape[2] // 2)   # noqa: E731
    acc = _assemble(prod, split(dy, sy, rtz), split(x, sx, rtz), drop, _where_dw(where, dy, wshape))
    return acc / (sy.double() * sx.double())


def emulated_wgrad_blocks(dy, x, wshape, stride=1, drop=None, block="pixels32"):
    """conv_wgrad_kernel<false> (no abs-max words) as its code runs: a wave owns a 64 x 64 (co, ci) tile of ONE tap and walks the output rows
    (n, oy) 32 pixels at a time; per step ONE scale for the 32 x 64 block of dY and one for the 32 x 64 block of the SHIFTED X (padding reads
    zeros, a block of zeros scales by 1), the sub-accumulator un-scaled before it is added.  block="tensor" is the defect: one scale per operand."""
    if block not in ("pixels32", "tensor"):
        raise ValueError(block)
    Co, Ci, k, _ = wshape
    N, _, H, W = x.shape
    Ho, Wo = dy.shape[2], dy.shape[3]
    pad = k // 2
    nch = (Wo + 31) // 32
    Wp = nch * 32

    def blocks(t, C):   # (N, C, Ho, Wo) -> (N Ho nch, 32, C / 64, 64)
        t = F.pad(t, (0, Wp - Wo)).permute(0, 2, 3, 1).reshape(N * Ho * nch, 32, C // 64, 64)
        return t

    def planes(t):      # one scale per (block, channel tile), un-scaled planes in fp64 (the division by a power of two is exact)
        amax = t.abs().amax(dim=(1, 3), keepdim=True) if block == "pixels32" else t.abs().max().expand(1, 1, 1, 1)
        s = scale_of(amax)
        hi, lo = split(t, s)
        return hi / s.double(), lo / s.double()

    yh, yl = planes(blocks(dy, Co))
    xp = F.pad(x, (pad, pad + stride * Wp, pad, pad + stride))
    out = torch.zeros(Co, Ci, k, k, dtype=torch.float64)
    for ky in range(k):
        for kx in range(k):
            xs = xp[:, :, ky:ky + stride * Ho:stride, kx:kx + stride * Wo:stride]   # X[n, ci, oy s + ky - pad, ox s + kx - pad]
            xh, xl = planes(blocks(xs, Ci))
            mm = lambda a, b: torch.einsum("bpto,bpsi->tosi", a, b).reshape(Co, Ci)   # noqa: E731
            acc = mm(yh, xh)
            if drop not in ("lo.hi", "both"):
                acc = acc + mm(yl, xh)
            if drop not in ("hi.lo", "both"):
                acc = acc + mm(yh, xl)
            out[:, :, ky, kx] = acc
    return out


# ---- case builders ---------------------------------------------------------------------------------------------------------------------
SPREAD = 100.0   # neighbouring images of a "spread" batch lie this far apart (tests/test_cpu_conv_grade.py pins 100 in, 1000 out)


def _image_factors(N, spread):
    return spread ** (torch.arange(N, dtype=torch.float32) - (N - 1) / 2.0)   # N = 3: 1 / spread, 1, spread


def conv_case(Cin, Cout, N, H, W, k=3, stride=1, res=False, relu=False, kind="plain", seed=0, spread=SPREAD, fold=True):
    """y = relu?(conv(x) s + t (+ res)) as sd_conv3x3_bn_act / sd_conv1x1_bn_act / sd_conv_s2_bn_act compute it: post-ReLU activations,
    kaiming weights, s / t a folded inference BatchNorm (fold=False: s = 1, t = 0 - conv_raw).  kind "spread": image n times
    spread^(n - 1) with t = 0 and no residual (an image's own norm is then the product's); "zero_image": image N // 2 all zero."""
    if kind not in ("plain", "spread", "zero_image"):
        raise ValueError(kind)
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, Cin, H, W, generator=g).abs()
    w = torch.randn(Cout, Cin, k, k, generator=g) * (2.0 / (k * k * Cout)) ** 0.5
    gamma, beta = 0.5 + torch.rand(Cout, generator=g), 0.2 * torch.randn(Cout, generator=g)
    mean, var = 0.3 * torch.randn(Cout, generator=g), 0.5 + torch.rand(Cout, generator=g)
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    r = torch.randn(N, Cout, Ho, Wo, generator=g).abs() if res else None
    s = gamma * torch.rsqrt(var + EPS)
    t = beta - mean * s
    if not fold:
        s, t = torch.ones(Cout), torch.zeros(Cout)
    if kind == "spread":
        if res:
            raise ValueError("'spread' runs without residual")
        x = x * _image_factors(N, spread).view(N, 1, 1, 1)
        t = torch.zeros(Cout)
    elif kind == "zero_image":
        x[N // 2] = 0.0
    c = SimpleNamespace(Cin=Cin, Cout=Cout, N=N, H=H, W=W, k=k, stride=stride, relu=relu, kind=kind, x=x, w=w, s=s, t=t, res=r,
                        label=f"conv{k}x{k}/s{stride} {Cin}->{Cout} N{N} {H}x{W}{' res' if res else ''}{' relu' if relu else ''} {kind}"
                              + (f" x{spread:g}" if kind == "spread" and spread != SPREAD else ""))
    c.epilogue = lambda acc, dt=torch.float32: _epilogue(c, acc, dt)
    c.want64, c.want32 = (c.epilogue(F.conv2d(x.to(dt), w.to(dt), stride=stride, padding=k // 2), dt) for dt in (torch.float64, torch.float32))
    return c


def _epilogue(c, acc, dt):
    y = acc.to(dt) * c.s.to(dt).view(1, -1, 1, 1) + c.t.to(dt).view(1, -1, 1, 1)
    if c.res is not None:
        y = y + c.res.to(dt)
    return F.relu(y) if c.relu else y


def emulated_conv_case(c, drop=None, where=None):
    """The kernel's arithmetic on a conv_case: the split product in fp64, rounded to fp32, the fp32 epilogue."""
    return c.epilogue(emulated_conv(c.x, c.w, c.stride, drop, where).float())


def stem_case(N, H, W, kind="plain", seed=0, spread=10.0):
    """maxpool3x3/s2/p1(relu(conv7x7/s2/p3(x) s + t)) on normalised frames of both signs (sd_stem_conv_bn_relu_pool).  "spread": frame n
    times spread^(n - 1), t = 0."""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(N, 3, H, W, generator=g) * 2.0 - 0.7
    w = torch.randn(64, 3, 7, 7, generator=g) * (2.0 / (49 * 64)) ** 0.5
    gamma, beta = 0.5 + torch.rand(64, generator=g), 0.2 * torch.randn(64, generator=g)
    mean, var = 0.3 * torch.randn(64, generator=g), 0.5 + torch.rand(64, generator=g)
    s = gamma * torch.rsqrt(var + EPS)
    t = beta - mean * s
    if kind == "spread":
        x = x * _image_factors(N, spread).view(N, 1, 1, 1)
        t = torch.zeros(64)
    c = SimpleNamespace(N=N, H=H, W=W, kind=kind, x=x, w=w, s=s, t=t, label=f"stem N{N} {H}x{W} {kind}")
    c.epilogue = lambda acc, dt=torch.float32: F.max_pool2d(F.relu(acc.to(dt) * s.to(dt).view(1, -1, 1, 1) + t.to(dt).view(1, -1, 1, 1)), 3, 2, 1)
    c.want64, c.want32 = (c.epilogue(F.conv2d(x.to(dt), w.to(dt), stride=2, padding=3), dt) for dt in (torch.float64, torch.float32))
    return c


def emulated_stem_case(c, drop=None, where=None):
    return c.epilogue(emulated_conv(c.x, c.w, 2, drop, where).float())


def wgrad_case(Cin, Cout, N, H, W, k=3, stride=1, kind="plain", seed=0, spread=SPREAD):
    """dW of conv2d(x, ., stride, padding k // 2) from dy.  "spread": x of image n times c_n = spread^(n - 1) and dy by 1 / c_n, so every
    image weighs the same in the sum; "quiet_channels": dy's output channels times logspace(-2, 0) (rows of dW over two decades)."""
    if kind not in ("plain", "spread", "quiet_channels"):
        raise ValueError(kind)
    g = torch.Generator().manual_seed(seed)
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    x = torch.randn(N, Cin, H, W, generator=g)
    dy = torch.randn(N, Cout, Ho, Wo, generator=g)
    if kind == "spread":
        f = _image_factors(N, spread).view(N, 1, 1, 1)
        x, dy = x * f, dy / f
    elif kind == "quiet_channels":
        dy = dy * torch.logspace(-2.0, 0.0, Cout).view(1, Cout, 1, 1)
    wshape = (Cout, Cin, k, k)
    c = SimpleNamespace(Cin=Cin, Cout=Cout, N=N, H=H, W=W, k=k, stride=stride, kind=kind, x=x, dy=dy, wshape=wshape, terms=N * Ho * Wo,
                        row_self=kind == "quiet_channels",
                        label=f"wgrad{k}x{k}/s{stride} {Cin}->{Cout} N{N} {H}x{W} {kind}" + (f" x{spread:g}" if kind == "spread" and spread != SPREAD else ""))
    c.want64, c.want32 = (torch.nn.grad.conv2d_weight(x.to(dt), wshape, dy.to(dt), stride=stride, padding=k // 2) for dt in (torch.float64, torch.float32))
    return c


def stem_wgrad_case(N, H, W, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(N, 3, H, W, generator=g)
    dy = torch.randn(N, 64, (H - 1) // 2 + 1, (W - 1) // 2 + 1, generator=g)
    wshape = (64, 3, 7, 7)
    c = SimpleNamespace(N=N, H=H, W=W, k=7, stride=2, x=x, dy=dy, wshape=wshape, terms=N * dy.shape[2] * dy.shape[3], row_self=False,
                        label=f"stem wgrad N{N} {H}x{W}")
    c.want64, c.want32 = (torch.nn.grad.conv2d_weight(x.to(dt), wshape, dy.to(dt), stride=2, padding=3) for dt in (torch.float64, torch.float32))
    return c


def dgrad_case(Cin, Cout, N, H, W, k=3, stride=1, seed=0):
    """dx (N, Cin, H, W) of conv2d(x, w (Cout, Cin, k, k), stride, padding k // 2) from dy; wt = the flipped transposed weight the
    PackedPair's backward planes hold (stride 1: dx = conv2d(dy, wt))."""
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(Cout, Cin, k, k, generator=g) * 0.05
    dy = torch.randn(N, Cout, (H - 1) // stride + 1, (W - 1) // stride + 1, generator=g)
    c = SimpleNamespace(Cin=Cin, Cout=Cout, N=N, H=H, W=W, k=k, stride=stride, w=w, dy=dy, wt=w.flip(2, 3).transpose(0, 1).contiguous(),
                        label=f"dgrad{k}x{k}/s{stride} {Cin}->{Cout} N{N} {H}x{W}")
    c.want64, c.want32 = (torch.nn.grad.conv2d_input((N, Cin, H, W), w.to(dt), dy.to(dt), stride=stride, padding=k // 2)
                          for dt in (torch.float64, torch.float32))
    return c


def emulated_dgrad_case(c, drop=None, where=None):
    if c.stride == 1:
        return emulated_conv(c.dy, c.wt, 1, drop, where)
    return emulated_convt(c.dy, c.w, c.H, c.W, drop, where)


# ---- training-mode BatchNorm (plain fp32 kernels: no emulation) ------------------------------------------------------------------------
MASK_MARGIN = 2.0 ** -20   # every |z| that decides a ReLU bit and every gap that decides a pool winner exceeds this (relative to the
                           # tensor's largest value): 8 fp32 roundings of it - no fp32 evaluation order flips one (test_cpu_conv_grade)


def bn_affine(y, mean, rstd, gamma, beta):
    """(y - mean) (rstd gamma) + beta in y's dtype - bn_affine of sd_conv_train.hip, channels last in dimension 1."""
    v = lambda t: t.to(y.dtype).view(1, -1, 1, 1)   # noqa: E731
    return (y - v(mean)) * (v(rstd) * v(gamma)) + v(beta)


def bn_case(C, npix, relu=True, res=False, kind="plain", seed=0):
    """Training BatchNorm on a (1, C, 1, npix) tensor (the kernels see (npix, C)), forward and backward ON IDENTICAL TENSORS: the backward's
    inputs are the fp32 reference forward's z, mean and rstd, its oracles the backward formula in fp64 / fp32 on those.  "offset": the mean
    of every fourth channel up to 100 standard deviations from zero (bn_stats_kernel's pivoted sums)."""
    if kind not in ("plain", "offset"):
        raise ValueError(kind)
    g = torch.Generator().manual_seed(seed)
    y = torch.randn(1, C, 1, npix, generator=g) * 2.0 + 0.5 * torch.randn(1, C, 1, 1, generator=g)
    if kind == "offset":
        off = torch.zeros(C)
        off[::4] = torch.linspace(-200.0, 200.0, C // 4)     # sigma = 2: up to 100 sigma
        y = y + off.view(1, C, 1, 1)
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.5
    r = torch.randn(1, C, 1, npix, generator=g) if res else None
    dz = torch.randn(1, C, 1, npix, generator=g)
    rm, rv = torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.5
    c = SimpleNamespace(C=C, npix=npix, relu=relu, kind=kind, y=y, gamma=gamma, beta=beta, res=r, dz=dz, rm=rm, rv=rv,
                        label=f"bn C{C} npix{npix}{' res' if res else ''}{' relu' if relu else ''} {kind}")

    def fwd(dt):
        yy = y.to(dt)
        mean = yy.mean(dim=(0, 2, 3))
        var = yy.var(dim=(0, 2, 3), unbiased=False)
        rstd = torch.rsqrt(var + EPS)
        pre = bn_affine(yy, mean, rstd, gamma.to(dt), beta.to(dt))
        if r is not None:
            pre = pre + r.to(dt)
        n = float(npix)
        run_m = 0.9 * rm.to(dt) + 0.1 * mean
        run_v = 0.9 * rv.to(dt) + 0.1 * var * (n / (n - 1.0) if npix > 1 else 1.0)
        return SimpleNamespace(pre=pre, z=F.relu(pre) if relu else pre, vec={"mean": mean, "rstd": rstd, "running_mean": run_m, "running_var": run_v})

    c.f64, c.f32 = fwd(torch.float64), fwd(torch.float32)
    c.mask = c.f32.pre > 0 if relu else torch.ones_like(y, dtype=torch.bool)

    def bwd(dt):   # from the fp32 forward's tensors
        mean, rstd = c.f32.vec["mean"].to(dt), c.f32.vec["rstd"].to(dt)
        gg = dz.to(dt) * c.mask.to(dt)
        xh = (y.to(dt) - mean.view(1, -1, 1, 1)) * rstd.view(1, -1, 1, 1)
        s1, s2 = gg.sum(dim=(0, 2, 3)), (gg * xh).sum(dim=(0, 2, 3))
        dy = (gamma.to(dt) * rstd).view(1, -1, 1, 1) * (gg - s1.view(1, -1, 1, 1) / npix - xh * s2.view(1, -1, 1, 1) / npix)
        return SimpleNamespace(dy=dy, vec={"dgamma": s2, "dbeta": s1}, dres=gg)

    c.b64, c.b32 = bwd(torch.float64), bwd(torch.float32)
    return c


def pool_winners(v):
    """Winner byte of every 3 x 3 / stride 2 / padding 1 window of v (N, C, Hc, Wc) = BatchNorm's output BEFORE the ReLU: ATen's max_pool2d
    scans the window rows first and replaces its maximum only by a strictly greater value, so the FIRST maximum wins - position 0 .. 8 in
    scan order; 9 where the window holds no positive value (relu gives zeros: whichever element ATen picks, its gradient dies in the ReLU)."""
    N, C, Hc, Wc = v.shape
    Hp, Wp = (Hc - 1) // 2 + 1, (Wc - 1) // 2 + 1
    p = F.pad(v, (1, 2, 1, 2), value=float("-inf"))
    best = torch.zeros(N, C, Hp, Wp, dtype=v.dtype)
    idx = torch.full((N, C, Hp, Wp), 9, dtype=torch.int64)
    for ky in range(3):
        for kx in range(3):
            cand = p[:, :, ky:ky + 2 * Hp:2, kx:kx + 2 * Wp:2]
            win = cand > best
            best = torch.where(win, cand, best)
            idx = torch.where(win, torch.full_like(idx, ky * 3 + kx), idx)
    return best, idx


def winner_words(idx):
    """(N, C, Hp, Wp) winner bytes -> the kernels' int32 words (N, Hp, Wp, C / 4): channel 4 j + q in byte q."""
    b = idx.permute(0, 2, 3, 1).reshape(*idx.permute(0, 2, 3, 1).shape[:3], -1, 4).to(torch.int64)
    w = b[..., 0] | (b[..., 1] << 8) | (b[..., 2] << 16) | (b[..., 3] << 24)
    return w.to(torch.int32).contiguous()


def pool_case(N, Hc, Wc, C=64, seed=0):
    """maxpool(relu(BatchNorm_train(y))) forward and backward (sd_bn_relu_pool_fwd / _bwd); the backward on the fp32 reference's winners,
    mean and rstd, its oracles the scatter + BatchNorm backward formula in fp64 / fp32."""
    g = torch.Generator().manual_seed(seed)
    y = torch.randn(N, C, Hc, Wc, generator=g) * 1.5 + 0.3
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.5
    rm, rv = torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.5
    Hp, Wp = (Hc - 1) // 2 + 1, (Wc - 1) // 2 + 1
    dp = torch.randn(N, C, Hp, Wp, generator=g)
    c = SimpleNamespace(N=N, Hc=Hc, Wc=Wc, C=C, y=y, gamma=gamma, beta=beta, rm=rm, rv=rv, dp=dp, npix=N * Hc * Wc, label=f"bn+relu+pool N{N} {Hc}x{Wc} C{C}")

    def fwd(dt):
        yy = y.to(dt)
        mean, var = yy.mean(dim=(0, 2, 3)), yy.var(dim=(0, 2, 3), unbiased=False)
        rstd = torch.rsqrt(var + EPS)
        v = bn_affine(yy, mean, rstd, gamma.to(dt), beta.to(dt))
        p, idx = pool_winners(v)
        n = float(c.npix)
        return SimpleNamespace(v=v, p=p, idx=idx, vec={"mean": mean, "rstd": rstd, "running_mean": 0.9 * rm.to(dt) + 0.1 * mean,
                                                      "running_var": 0.9 * rv.to(dt) + 0.1 * var * (n / (n - 1.0) if c.npix > 1 else 1.0)})

    c.f64, c.f32 = fwd(torch.float64), fwd(torch.float32)

    def bwd(dt):
        gg = torch.zeros(N, C, Hc + 3, Wc + 3, dtype=dt)   # padded by (1, 2): window position (ky, kx) of pooled (i, j) = padded (2 i + ky, 2 j + kx)
        for ky in range(3):
            for kx in range(3):
                gg[:, :, ky:ky + 2 * Hp:2, kx:kx + 2 * Wp:2] += dp.to(dt) * (c.f32.idx == ky * 3 + kx).to(dt)
        gg = gg[:, :, 1:1 + Hc, 1:1 + Wc]
        mean, rstd = c.f32.vec["mean"].to(dt), c.f32.vec["rstd"].to(dt)
        xh = (y.to(dt) - mean.view(1, -1, 1, 1)) * rstd.view(1, -1, 1, 1)
        s1, s2 = gg.sum(dim=(0, 2, 3)), (gg * xh).sum(dim=(0, 2, 3))
        dy = (gamma.to(dt) * rstd).view(1, -1, 1, 1) * (gg - s1.view(1, -1, 1, 1) / c.npix - xh * s2.view(1, -1, 1, 1) / c.npix)
        return SimpleNamespace(dy=dy, vec={"dgamma": s2, "dbeta": s1})

    c.b64, c.b32 = bwd(torch.float64), bwd(torch.float32)
    return c


def decision_margin(c) -> float:
    """The smallest distance that decides a mask bit (bn_case: |pre|) or a winner (pool_case: the gap between a window's two largest values,
    and the largest value's distance from zero) in the fp64 reference, relative to the tensor's largest value."""
    if hasattr(c, "dp"):
        v = c.f64.v
        N, C, Hc, Wc = v.shape
        Hp, Wp = c.f64.p.shape[2:]
        p = F.pad(v, (1, 2, 1, 2), value=float("-inf"))
        win = torch.stack([p[:, :, ky:ky + 2 * Hp:2, kx:kx + 2 * Wp:2] for ky in range(3) for kx in range(3)], -1)
        top = win.clamp_min(0.0).topk(2, dim=-1).values     # (relu'd: below zero nothing is decided)
        gap = (top[..., 0] - top[..., 1])[top[..., 0] > 0]
        near0 = win[torch.isfinite(win)].abs().min()
        return float(min(gap.min() if gap.numel() else near0, near0) / v.abs().max())
    if not c.relu:
        return float("inf")
    return float(c.f64.pre.abs().min() / c.f64.pre.abs().max())


# ---- the encoder heads -----------------------------------------------------------------------------------------------------------------
def head_case(conv, C, H, W, d, N, seed=0):
    """Both ResNet encoder heads on the NHWC map x (N, H, W, C): fc(mean over H W), or fc(flatten_NCHW(Conv2d(C, 32, 1)(x))); forward and
    every gradient in fp64 / fp32 (plain fp32 kernels: no emulation)."""
    g = torch.Generator().manual_seed(seed)
    J = 32 * H * W if conv else C
    t = {"x": torch.relu(torch.randn(N, H, W, C, generator=g)), "fc_w": torch.randn(d, J, generator=g) / J ** 0.5, "fc_b": torch.randn(d, generator=g)}
    if conv:
        t["conv_w"] = torch.randn(32, C, 1, 1, generator=g) / C ** 0.5
        t["conv_b"] = torch.randn(32, generator=g)
    dy = torch.randn(N, d, generator=g)
    c = SimpleNamespace(conv=conv, C=C, H=H, W=W, d=d, N=N, t=t, dy=dy, label=f"head {'conv1x1' if conv else 'avgpool'} C{C} {H}x{W} d{d} N{N}")

    def run(dt):
        leaves = {k: v.detach().clone().to(dt).requires_grad_() for k, v in t.items()}
        x = leaves["x"]
        if conv:
            z = torch.einsum("nhwc,oc->nohw", x, leaves["conv_w"].reshape(32, C)) + leaves["conv_b"][None, :, None, None]
            feat = z.reshape(N, -1)
        else:
            feat = x.mean(dim=(1, 2))
        out = feat @ leaves["fc_w"].T + leaves["fc_b"]
        out.backward(dy.to(dt))
        return out.detach(), {k: v.grad for k, v in leaves.items()}

    (c.y64, c.g64), (c.y32, c.g32) = run(torch.float64), run(torch.float32)
    return c


# ---- the cases both test files run -----------------------------------------------------------------------------------------------------
MODES = {"res-relu": dict(res=True, relu=True), "relu": dict(res=False, relu=True), "bare": dict(res=False, relu=False)}


def conv3x3_cases():
    """[(id, conv_case keywords)]: maps of one pixel, one full 8 x 16 tile, one row and one column past it, one short of it; y_group 8 / 2 / 1
    (64 / 256 / 512 -> 512) at 1, 8 and 9 tiles (9 tiles = one idle slot beside 8 XCDs); the three epilogues; the kinds on three images."""
    shapes = [(64, 64, 1, 1, 1), (64, 128, 2, 8, 16), (128, 64, 2, 9, 17), (128, 128, 3, 7, 15),
              (64, 512, 1, 8, 16), (256, 512, 8, 8, 16), (512, 512, 9, 7, 15), (64, 512, 9, 9, 17)]
    out = []
    for i, (ci, co, n, h, w) in enumerate(shapes):
        for m, kw in MODES.items():
            out.append((f"{ci}-{co}-N{n}-{h}x{w}-{m}", dict(Cin=ci, Cout=co, N=n, H=h, W=w, seed=100 + i, **kw)))
    for i, (ci, co, h, w) in enumerate([(128, 128, 7, 15), (512, 512, 9, 17), (64, 512, 8, 16)]):
        for kind in ("spread", "zero_image"):
            out.append((f"{ci}-{co}-N3-{h}x{w}-{kind}", dict(Cin=ci, Cout=co, N=3, H=h, W=w, relu=True, kind=kind, seed=150 + i)))
    return out


def conv1x1_cases():
    out = []
    for i, (ci, co) in enumerate([(64, 256), (256, 64), (2048, 512)]):
        for m in ("res-relu", "bare"):
            out.append((f"{ci}-{co}-3x5-{m}", dict(Cin=ci, Cout=co, N=2, H=3, W=5, k=1, seed=200 + i, **MODES[m])))
    out.append(("256-64-3x5-spread", dict(Cin=256, Cout=64, N=3, H=3, W=5, k=1, relu=True, kind="spread", seed=209)))
    return out


def conv_s2_cases():
    out = []
    for k in (3, 1):
        for i, (h, w) in enumerate([(1, 1), (2, 3), (15, 21), (16, 32)]):
            for ci, co in ((64, 128), (256, 512)):
                out.append((f"k{k}-{ci}-{co}-{h}x{w}", dict(Cin=ci, Cout=co, N=2, H=h, W=w, k=k, stride=2, relu=k == 3, seed=300 + 10 * k + i)))
    out.append(("k3-64-128-15x21-spread", dict(Cin=64, Cout=128, N=3, H=15, W=21, k=3, stride=2, relu=True, kind="spread", seed=340)))
    return out


def stem_cases():
    return [(f"N{n}-{h}x{w}-{kind}", dict(N=n, H=h, W=w, kind=kind, seed=400 + i))
            for i, (n, h, w, kind) in enumerate([(1, 1, 1, "plain"), (2, 7, 9, "plain"), (1, 37, 53, "plain"), (2, 64, 64, "plain"), (3, 37, 53, "spread")])]


# Widened gates, decided by the emulation on the CPU (tests/test_cpu_conv_grade.py::test_widened_gates_are_the_justified_ones re-measures
# every entry): id -> (factor, floor, the unbroken emulation's tightness against the DEFAULT bound 4 x + 1e-7).
#   factor 8 (the existing convolution tests' 8 * e32 + 2e-7): where the emulation alone exceeds half the default bound on a contraction
#     of 64 terms or more - NO case of this file: with both halves rounded to nearest the contract stays below 0.5 on all of them;
#   floor 2^-20: contractions of fewer than 64 terms (weight gradients on tiny maps: an element is a handful of products of 22-bit
#     operands against fp32's single rounding each) - every such case, the emulation passes it at or below one half.
WIDE: dict = {
    "strip-s1-64-64-N1-1x1": (parity.FACTOR, FLOOR_SHORT, 0.71),   # 1 terms; 0.22 of 4 x + 2^-20
    "strip-s1-64-64-N3-1x1": (parity.FACTOR, FLOOR_SHORT, 0.49),   # 3 terms; 0.15 of 4 x + 2^-20
    "strip-s1-64-64-N1-2x1": (parity.FACTOR, FLOOR_SHORT, 0.78),   # 2 terms; 0.24 of 4 x + 2^-20
    "strip-s1-64-64-N3-2x1": (parity.FACTOR, FLOOR_SHORT, 0.41),   # 6 terms; 0.15 of 4 x + 2^-20
    "strip-s1-64-64-N1-9x1": (parity.FACTOR, FLOOR_SHORT, 0.29),   # 9 terms; 0.11 of 4 x + 2^-20
    "strip-s1-64-64-N3-9x1": (parity.FACTOR, FLOOR_SHORT, 0.16),   # 27 terms; 0.07 of 4 x + 2^-20
    "strip-s1-64-64-N1-1x31": (parity.FACTOR, FLOOR_SHORT, 0.20),   # 31 terms; 0.09 of 4 x + 2^-20
    "strip-s1-64-64-N1-2x31": (parity.FACTOR, FLOOR_SHORT, 0.14),   # 62 terms; 0.08 of 4 x + 2^-20
    "strip-s1-64-64-N1-1x32": (parity.FACTOR, FLOOR_SHORT, 0.15),   # 32 terms; 0.08 of 4 x + 2^-20
    "strip-s1-64-64-N1-1x33": (parity.FACTOR, FLOOR_SHORT, 0.17),   # 33 terms; 0.07 of 4 x + 2^-20
    "strip-s1-512-512-N1-9x5-empty-groups": (parity.FACTOR, FLOOR_SHORT, 0.19),   # 45 terms; 0.09 of 4 x + 2^-20
    "strip-s2-64-128-N1-1x1": (parity.FACTOR, FLOOR_SHORT, 0.89),   # 1 terms; 0.26 of 4 x + 2^-20
    "strip-s2-64-128-N2-2x3": (parity.FACTOR, FLOOR_SHORT, 0.60),   # 4 terms; 0.20 of 4 x + 2^-20
    "wave-k1-s1-words-128-64-1x1": (parity.FACTOR, FLOOR_SHORT, 0.47),   # 2 terms; 0.16 of 4 x + 2^-20
    "wave-k1-s1-words-64-256-1x1": (parity.FACTOR, FLOOR_SHORT, 0.42),   # 2 terms; 0.17 of 4 x + 2^-20
    "wave-k1-s1-blocks-128-64-1x1": (parity.FACTOR, FLOOR_SHORT, 0.65),   # 2 terms; 0.19 of 4 x + 2^-20
    "wave-k1-s1-blocks-64-256-1x1": (parity.FACTOR, FLOOR_SHORT, 0.54),   # 2 terms; 0.19 of 4 x + 2^-20
    "wave-k1-s2-words-128-128-1x1": (parity.FACTOR, FLOOR_SHORT, 0.53),   # 2 terms; 0.18 of 4 x + 2^-20
    "wave-k1-s2-words-64-256-1x1": (parity.FACTOR, FLOOR_SHORT, 0.64),   # 2 terms; 0.21 of 4 x + 2^-20
    "wave-k1-s2-blocks-128-128-1x1": (parity.FACTOR, FLOOR_SHORT, 0.64),   # 2 terms; 0.20 of 4 x + 2^-20
    "wave-k1-s2-blocks-64-256-1x1": (parity.FACTOR, FLOOR_SHORT, 0.54),   # 2 terms; 0.18 of 4 x + 2^-20
    "wave-k3-s1-blocks-128-64-1x1": (parity.FACTOR, FLOOR_SHORT, 0.61),   # 2 terms; 0.19 of 4 x + 2^-20
    "wave-k3-s1-blocks-64-256-1x1": (parity.FACTOR, FLOOR_SHORT, 0.65),   # 2 terms; 0.23 of 4 x + 2^-20
    "wave-k3-s2-blocks-128-128-1x1": (parity.FACTOR, FLOOR_SHORT, 0.60),   # 2 terms; 0.20 of 4 x + 2^-20
    "wave-k3-s2-blocks-64-256-1x1": (parity.FACTOR, FLOOR_SHORT, 0.54),   # 2 terms; 0.18 of 4 x + 2^-20
    "wave-k1-s2-words-128-128-8x8": (parity.FACTOR, FLOOR_SHORT, 0.21),   # 32 terms; 0.08 of 4 x + 2^-20
    "wave-k1-s2-words-64-256-8x8": (parity.FACTOR, FLOOR_SHORT, 0.18),   # 32 terms; 0.08 of 4 x + 2^-20
    "wave-k1-s2-blocks-128-128-8x8": (parity.FACTOR, FLOOR_SHORT, 0.21),   # 32 terms; 0.08 of 4 x + 2^-20
    "wave-k1-s2-blocks-64-256-8x8": (parity.FACTOR, FLOOR_SHORT, 0.22),   # 32 terms; 0.09 of 4 x + 2^-20
    "wave-k3-s2-blocks-128-128-8x8": (parity.FACTOR, FLOOR_SHORT, 0.18),   # 32 terms; 0.08 of 4 x + 2^-20
    "wave-k3-s2-blocks-64-256-8x8": (parity.FACTOR, FLOOR_SHORT, 0.17),   # 32 terms; 0.08 of 4 x + 2^-20
    "wave-k1-s2-words-128-128-10x12": (parity.FACTOR, FLOOR_SHORT, 0.17),   # 60 terms; 0.07 of 4 x + 2^-20
    "wave-k1-s2-words-64-256-10x12": (parity.FACTOR, FLOOR_SHORT, 0.16),   # 60 terms; 0.07 of 4 x + 2^-20
    "wave-k1-s2-blocks-128-128-10x12": (parity.FACTOR, FLOOR_SHORT, 0.15),   # 60 terms; 0.06 of 4 x + 2^-20
    "wave-k1-s2-blocks-64-256-10x12": (parity.FACTOR, FLOOR_SHORT, 0.17),   # 60 terms; 0.08 of 4 x + 2^-20
    "wave-k3-s2-blocks-128-128-10x12": (parity.FACTOR, FLOOR_SHORT, 0.15),   # 60 terms; 0.07 of 4 x + 2^-20
    "wave-k3-s2-blocks-64-256-10x12": (parity.FACTOR, FLOOR_SHORT, 0.12),   # 60 terms; 0.06 of 4 x + 2^-20
    "stemw-N2-2x2": (parity.FACTOR, FLOOR_SHORT, 0.37),   # 2 terms; 0.15 of 4 x + 2^-20
}


def gate_of(case_id: str):
    f, fl, _ = WIDE.get(case_id, (parity.FACTOR, parity.FLOOR, None))
    return dict(factor=f, floor=fl)


def wgrad_strip_cases():
    """3 x 3 with abs-max words (conv_wgrad3_kernel).  64 -> 64: one (co, ci) tile, so groups = steps and EVERY group is one step that starts
    mid-strip behind its two staging steps; W = 1 / 31 / 32 / 33 (one ragged strip, one full, one full + one pixel), H = 1 / 2 / 9, N = 1 / 3;
    N H ceil(W / 32) = 3 x 5 x 2 = 30 steps; 512 -> 512 at 1 x 9 x 5: 64 tiles -> 8 groups of 2 steps for 9 steps, three groups empty;
    stride 2 (four parity-class launches) at 1 x 1 (the odd classes empty), 2 x 3, 17 x 33; the kinds."""
    out = []
    i = 0
    for W in (1, 31, 32, 33):
        for H in (1, 2, 9):
            for N in (1, 3):
                out.append((f"s1-64-64-N{N}-{H}x{W}", dict(Cin=64, Cout=64, N=N, H=H, W=W, seed=500 + i)))
                i += 1
    out += [("s1-64-64-N3-5x33-steps30", dict(Cin=64, Cout=64, N=3, H=5, W=33, seed=540)),
            ("s1-512-512-N1-9x5-empty-groups", dict(Cin=512, Cout=512, N=1, H=9, W=5, seed=541)),
            ("s1-128-64-N3-9x33-spread", dict(Cin=128, Cout=64, N=3, H=9, W=33, kind="spread", seed=542)),
            ("s1-64-128-N1-9x33-quiet", dict(Cin=64, Cout=128, N=1, H=9, W=33, kind="quiet_channels", seed=543))]
    for j, (N, H, W) in enumerate([(1, 1, 1), (2, 2, 3), (1, 17, 33)]):
        out.append((f"s2-64-128-N{N}-{H}x{W}", dict(Cin=64, Cout=128, N=N, H=H, W=W, stride=2, seed=550 + j)))
    out.append(("s2-64-128-N3-17x33-spread", dict(Cin=64, Cout=128, N=3, H=17, W=33, stride=2, kind="spread", seed=554)))
    return out


def wgrad_wave_cases():
    """conv_wgrad_kernel: [(id, keywords, words)] - 1 x 1 at both strides with abs-max words (one scale per tensor) and without (per 32
    pixels), 3 x 3 without words; maps 1 x 1, 8 x 8, 10 x 12; 128 -> 64 and 64 -> 256 (stride 2 needs Cout % 128 == 0: 64 -> 128 there)."""
    out = []
    i = 0
    for (h, w) in ((1, 1), (8, 8), (10, 12)):
        for k, stride, words in ((1, 1, True), (1, 1, False), (1, 2, True), (1, 2, False), (3, 1, False), (3, 2, False)):
            for ci, co in ((128, 64), (64, 256)):
                if stride == 2 and co % 128:
                    co = 128
                out.append((f"k{k}-s{stride}-{'words' if words else 'blocks'}-{ci}-{co}-{h}x{w}",
                            dict(Cin=ci, Cout=co, N=2, H=h, W=w, k=k, stride=stride, seed=600 + i), words))
                i += 1
    out.append(("k1-s1-blocks-128-64-N3-8x8-spread", dict(Cin=128, Cout=64, N=3, H=8, W=8, k=1, kind="spread", seed=690), False))
    return out


def stem_wgrad_cases():
    return [(f"N{n}-{h}x{w}", dict(N=n, H=h, W=w, seed=700 + i)) for i, (n, h, w) in enumerate([(2, 2, 2), (1, 61, 64), (2, 61, 66)])]


def dgrad_cases():
    out = [(f"s1-k{k}-{ci}-{co}-{h}x{w}", dict(Cin=ci, Cout=co, N=2, H=h, W=w, k=k, stride=1, seed=800 + i))
           for i, (k, ci, co, h, w) in enumerate([(3, 64, 64, 9, 17), (3, 128, 64, 1, 1), (1, 64, 256, 3, 5)])]
    out += [(f"s2-k3-{ci}-{co}-{h}x{w}", dict(Cin=ci, Cout=co, N=2, H=h, W=w, k=3, stride=2, seed=810 + i))
            for i, (ci, co, h, w) in enumerate([(64, 128, 1, 1), (64, 128, 2, 3), (128, 128, 16, 32), (64, 128, 17, 33)])]
    out += [(f"s2-k1-{ci}-{co}-{h}x{w}", dict(Cin=ci, Cout=co, N=2, H=h, W=w, k=1, stride=2, seed=820 + i))
            for i, (ci, co, h, w) in enumerate([(64, 128, 1, 1), (64, 128, 2, 3), (64, 128, 17, 33)])]
    return out


def bn_cases():
    """C = 64 / 512 / 2048 (the last: two 1024-channel passes of channel_reduce) x npix = 2, 5 and one pixel either side of a workgroup's
    share of 65536 / C pixels x residual / ReLU / both x plain / offset: the full product, 72 cases.  Seeds: every case's decision_margin
    exceeds MASK_MARGIN (test_cpu_conv_grade.py::test_no_relu_mask_bit_is_left_to_luck), so masks are compared exactly on the GPU."""
    out = []
    i = 0
    for C in (64, 512, 2048):
        share = 65536 // C
        for npix in (2, 5, share - 1, share + 1):
            for m, (relu, res) in {"res": (False, True), "relu": (True, False), "res-relu": (True, True)}.items():
                for kind in ("plain", "offset"):
                    out.append((f"C{C}-npix{npix}-{m}-{kind}", dict(C=C, npix=npix, relu=relu, res=res, kind=kind, seed=BN_SEEDS.get(i, 900 + i))))
                    i += 1
    return out


# index -> seed, where the default seed left a |z| (a winner's gap) inside twice MASK_MARGIN: the first of seed + 100, + 200, ... that does not
BN_SEEDS: dict = {15: 1015, 16: 1116, 17: 1017, 22: 1022, 41: 1041, 44: 1244, 58: 1158, 63: 1063, 65: 1065, 71: 1171}
POOL_SEEDS: dict = {3: 1503}


def pool_cases():
    return [(f"N{n}-{h}x{w}", dict(N=n, Hc=h, Wc=w, seed=POOL_SEEDS.get(i, 1000 + i))) for i, (n, h, w) in enumerate([(2, 1, 1), (1, 2, 5), (3, 7, 9), (1, 31, 39)])]


def head_cases():
    out = []
    i = 0
    for conv in (False, True):
        for (h, w) in ((1, 1), (7, 7)):
            for d, n in ((37, 1), (64, 3), (37, 3)):
                out.append((f"{'conv1x1' if conv else 'avgpool'}-{h}x{w}-d{d}-N{n}", dict(conv=conv, C=512, H=h, W=w, d=d, N=n, seed=1100 + i)))
                i += 1
    return out
