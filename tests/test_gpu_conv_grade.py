"""The ResNet backbone kernels (csrc/sd_conv.hip, csrc/sd_conv_train.hip, csrc/sd_head.hip through ops.py / conv_training.py) held to fp32
grade image by image, pixel by pixel, output channel by output channel and tap by tap: every error figure of a kernel against the fp64 CPU
operator is bounded by 4 x the same figure of the fp32 CPU operator on the same inputs + 1e-7 (tests/parity.py; the cases, the oracles and
the few widened floors are tests/conv_cases.py's, fitted on the CPU by tests/test_cpu_conv_grade.py before any kernel is held to them).
Shapes are the smallest that reach the edge they name; the workload's own shapes stay in test_gpu_conv.py / test_gpu_conv_training.py.
Every training kernel runs on IDENTICAL tensors: the backward kernels read the fp32 reference forward's outputs, so masks and pool
winners are compared exactly and no element is left out.  `-s` prints one parity.report line per gated tensor
(profiles/resnet_parity.txt)."""

import copy

import pytest
import torch

import conv_cases as cc
import parity

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    from soccerdiffusion_amd import ops as o

    return o


@pytest.fixture(scope="module")
def ct():
    from soccerdiffusion_amd import conv_training

    return conv_training


def _word():
    return torch.zeros(1, dtype=torch.int32, device=DEV)


def _assert_word_is_the_max(word, y, label):
    """The abs-max word is a maximum of STORED values: bit for bit max |y| of the tensor the kernel wrote."""
    assert cc.word_value(word) == float(y.abs().max()), (label, cc.word_value(word), float(y.abs().max()))


# ---- inference (sd_conv.hip) ---------------------------------------------------------------------------------------------------------
def _run_conv(ops, c):
    xh = cc.nhwc(c.x).to(DEV)
    pk = ops.PackedConv3x3(c.w.to(DEV))
    xa, ya = ops.absmax_word(xh), _word()
    s, t = c.s.to(DEV), c.t.to(DEV)
    if c.stride == 1:
        rh = cc.nhwc(c.res).to(DEV) if c.res is not None else None
        y = ops.conv3x3_bn_act(xh, xa, pk, s, t, res=rh, relu=c.relu, y_amax=ya)
    else:
        y = ops.conv_s2_bn_act(xh, xa, pk, s, t, relu=c.relu, y_amax=ya)
    return y, ya


def _require(cond, what):
    if not cond:
        pytest.fail(what)


def _conv_test(ops, cid, kw):
    c = cc.conv_case(**kw)
    y, ya = _run_conv(ops, c)
    _require(tuple(y.shape) == tuple(cc.nhwc(c.want64).shape), c.label + ": shape")
    _require(cc.word_value(ya) == float(y.abs().max()), c.label + ": the abs-max word is not max |y| bit for bit")
    y2, ya2 = _run_conv(ops, c)
    _require(torch.equal(y, y2) and int(ya) == int(ya2), c.label + ": a repeat call gives other bits")   # deterministic
    if c.kind == "zero_image":                                   # an all-zero frame: exactly the epilogue of zero
        z = c.N // 2
        _require(torch.equal(cc.nchw(y)[z].cpu(), c.want32[z]), c.label + ": the all-zero frame is not the epilogue of zero")
    cc.grade(cc.nchw(y), c.want64, c.want32, c.label, **cc.gate_of("conv-" + cid))


@pytest.mark.parametrize("cid,kw", cc.conv3x3_cases(), ids=[c for c, _ in cc.conv3x3_cases()])
def test_conv3x3_bn_act_is_fp32_grade(ops, cid, kw):
    """(At Cin >= 512 the host picks the instantiation with cross-term accumulators of their own: with ONE accumulator for the 3 x 288 dependent
    MFMAs of K = 4608 the worst (image, output channel) row of the five 512 -> 512 cases measured 4.3 - 4.8 x fp32's.)"""
    _conv_test(ops, cid, kw)


@pytest.mark.parametrize("cid,kw", cc.conv1x1_cases(), ids=[c for c, _ in cc.conv1x1_cases()])
def test_conv1x1_bn_act_is_fp32_grade(ops, cid, kw):
    _conv_test(ops, cid, kw)


@pytest.mark.parametrize("cid,kw", cc.conv_s2_cases(), ids=[c for c, _ in cc.conv_s2_cases()])
def test_conv_s2_bn_act_is_fp32_grade(ops, cid, kw):
    _conv_test(ops, cid, kw)


@pytest.mark.parametrize("cid,kw", cc.stem_cases(), ids=[c for c, _ in cc.stem_cases()])
def test_stem_conv_bn_relu_pool_is_fp32_grade(ops, cid, kw):
    c = cc.stem_case(**kw)
    xd = c.x.to(DEV)
    pk = ops.PackedStem(c.w.to(DEV))

    def run():
        ya = _word()
        return ops.stem_conv_bn_relu_pool(xd, ops.absmax_word(xd), pk, c.s.to(DEV), c.t.to(DEV), y_amax=ya), ya

    y, ya = run()
    assert tuple(y.shape) == tuple(cc.nhwc(c.want64).shape)
    _assert_word_is_the_max(ya, y, c.label)
    cc.grade(cc.nchw(y), c.want64, c.want32, c.label, **cc.gate_of("stem-" + cid))
    y2, ya2 = run()
    assert torch.equal(y, y2) and int(ya) == int(ya2)


def _encoder(hidden, avgpool, H, W, seed):
    from soccerdiffusion_amd.ml.model.encoder.image import ImageEncoderType, image_encoder_factory

    torch.manual_seed(seed)
    enc = image_encoder_factory(ImageEncoderType.RESNET18, hidden, avgpool, H)
    enc.train()   # non-trivial running statistics (a fresh BatchNorm has mean 0 / var 1)
    with torch.no_grad():
        enc(torch.rand(2, 2, 3, H, W, generator=torch.Generator().manual_seed(seed + 1)))
    return enc.eval()


def _grade_tokens(got, want64, want32, label):
    v = lambda t: t.detach().cpu().reshape(-1, 1, t.shape[-1])   # noqa: E731  (frames, 1, hidden): 'traj' = each frame against itself
    return parity.assert_fp32_grade(v(got), v(want64), v(want32), label=label)


@pytest.mark.parametrize("avgpool,H,W", [(True, 64, 64), (False, 64, 64), (True, 64, 96)], ids=["avgpool-64x64", "conv1x1-64x64", "avgpool-64x96"])
def test_resnet18_encoder_eval_is_fp32_grade_frame_by_frame(avgpool, H, W):
    enc = _encoder(64, avgpool, H, W, seed=11)
    x = torch.rand(2, 2, 3, H, W, generator=torch.Generator().manual_seed(12))
    with torch.no_grad():
        want32 = enc(x)
        want64 = copy.deepcopy(enc).double()(x.double())
        g = copy.deepcopy(enc).to(DEV).eval()
        got = g(x.to(DEV))
        again = g(x.to(DEV))
    assert got.shape == (2, 2, 64) and torch.equal(got, again)
    _grade_tokens(got, want64, want32, f"resnet18 eval {'avgpool' if avgpool else 'conv1x1 head'} 2x2 frames {H}x{W}")


def test_a_frame_alone_and_in_a_batch_is_graded_not_bit_stable():
    """Six different frames (brightness 0.2 .. 1.2 of the brightest), each encoded alone and all together: BOTH results sit within the gate
    and a repeat call gives the same bits.  The two are NOT asserted equal to each other: every activation tensor takes ONE fp16 scale from its
    abs-max word, so the split of a frame's values depends on the frames beside it - a frame's token is graded, not
    bit-stable, across batch compositions."""
    enc = _encoder(64, True, 64, 64, seed=13)
    g = torch.Generator().manual_seed(14)
    x = torch.rand(1, 6, 3, 64, 64, generator=g) * torch.linspace(0.2, 1.2, 6).view(1, 6, 1, 1, 1)
    dev = copy.deepcopy(enc).to(DEV).eval()
    with torch.no_grad():
        want32, want64 = enc(x), copy.deepcopy(enc).double()(x.double())
        together = dev(x.to(DEV))
        alone = torch.cat([dev(x[:, f:f + 1].to(DEV)) for f in range(6)], dim=1)
        assert torch.equal(together, dev(x.to(DEV)))
        assert torch.equal(alone, torch.cat([dev(x[:, f:f + 1].to(DEV)) for f in range(6)], dim=1))
    _grade_tokens(together, want64, want32, "resnet18 eval six frames together")
    _grade_tokens(alone, want64, want32, "resnet18 eval six frames, each alone")


# ---- training-mode BatchNorm (sd_conv_train.hip) ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,kw", cc.bn_cases(), ids=[c for c, _ in cc.bn_cases()])
def test_bn_train_forward_and_backward_are_fp32_grade(ct, cid, kw):
    c = cc.bn_case(**kw)
    y, gamma, beta = cc.nhwc(c.y).to(DEV), c.gamma.to(DEV), c.beta.to(DEV)
    res = cc.nhwc(c.res).to(DEV) if c.res is not None else None

    def fwd():
        rm, rv = c.rm.to(DEV), c.rv.to(DEV)
        z, word, mean, rstd = ct.bn_train_fwd(y, gamma, beta, res, rm, rv, cc.EPS, 0.1, c.relu)
        return z, word, {"mean": mean, "rstd": rstd, "running_mean": rm, "running_var": rv}

    z, word, vec = fwd()
    _assert_word_is_the_max(word, z, c.label)
    cc.grade(cc.nchw(z), c.f64.z, c.f32.z, c.label + " z")
    if c.relu:
        assert torch.equal(cc.nchw(z).cpu() > 0, c.mask)         # the forward kernel's own mask: every bit
    cc.grade_vec(vec, c.f64.vec, c.f32.vec, c.label)
    z2, word2, vec2 = fwd()
    assert torch.equal(z, z2) and int(word) == int(word2) and all(torch.equal(vec[k], vec2[k]) for k in vec)
    # the backward on the fp32 reference forward's tensors (mask, mean, rstd): the kernels' own error and nothing upstream of them
    dz, z32 = cc.nhwc(c.dz).to(DEV), cc.nhwc(c.f32.z).to(DEV)
    mean32, rstd32 = c.f32.vec["mean"].to(DEV), c.f32.vec["rstd"].to(DEV)
    want_dres = c.res is not None

    def bwd(zz):
        return ct.bn_train_bwd(dz, zz, y, mean32, rstd32, gamma, c.relu, want_dres, beta)

    dy, dword, dgamma, dbeta, dres = bwd(z32 if c.relu else None)
    _assert_word_is_the_max(dword, dy, c.label + " dy")
    cc.grade(cc.nchw(dy), c.b64.dy, c.b32.dy, c.label + " dy")
    cc.grade_vec({"dgamma": dgamma, "dbeta": dbeta}, c.b64.vec, c.b32.vec, c.label)
    if want_dres:   # a copy behind the mask: exact
        assert torch.equal(cc.nchw(dres).cpu(), c.b32.dres)
    again = bwd(z32 if c.relu else None)
    assert all(torch.equal(a, b) for a, b in zip((dy, dword, dgamma, dbeta), again[:4]))
    if c.relu and not want_dres:
        # the recomputed-mask form (z = None: what a unit without residual operand runs): the SAME mask, so the same bits
        rec = bwd(None)
        assert all(torch.equal(a, b) for a, b in zip((dy, dword, dgamma, dbeta), rec[:4]))


@pytest.mark.parametrize("cid,kw", cc.pool_cases(), ids=[c for c, _ in cc.pool_cases()])
def test_bn_relu_pool_forward_and_backward_are_fp32_grade(ct, cid, kw):
    c = cc.pool_case(**kw)
    y, gamma, beta = cc.nhwc(c.y).to(DEV), c.gamma.to(DEV), c.beta.to(DEV)

    def fwd():
        rm, rv = c.rm.to(DEV), c.rv.to(DEV)
        p, word, idx, mean, rstd = ct.bn_relu_pool_fwd(y, gamma, beta, rm, rv, cc.EPS, 0.1)
        return p, word, idx, {"mean": mean, "rstd": rstd, "running_mean": rm, "running_var": rv}

    p, word, idx, vec = fwd()
    words32 = cc.winner_words(c.f32.idx)
    assert torch.equal(idx.cpu(), words32)                       # every winner byte, ATen's first-maximum rule; no element left out
    _assert_word_is_the_max(word, p, c.label)
    cc.grade(cc.nchw(p), c.f64.p, c.f32.p, c.label + " p")
    cc.grade_vec(vec, c.f64.vec, c.f32.vec, c.label)
    p2, word2, idx2, vec2 = fwd()
    assert torch.equal(p, p2) and torch.equal(idx, idx2) and int(word) == int(word2) and all(torch.equal(vec[k], vec2[k]) for k in vec)
    dp = cc.nhwc(c.dp).to(DEV)
    args = (dp, words32.to(DEV), y, c.f32.vec["mean"].to(DEV), c.f32.vec["rstd"].to(DEV), gamma)
    dy, dword, dgamma, dbeta = ct.bn_relu_pool_bwd(*args)
    _assert_word_is_the_max(dword, dy, c.label + " dy")
    cc.grade(cc.nchw(dy), c.b64.dy, c.b32.dy, c.label + " dy")
    cc.grade_vec({"dgamma": dgamma, "dbeta": dbeta}, c.b64.vec, c.b32.vec, c.label)
    assert all(torch.equal(a, b) for a, b in zip((dy, dword, dgamma, dbeta), ct.bn_relu_pool_bwd(*args)))


# ---- weight gradients ------------------------------------------------------------------------------------------------------------------
def _wgrad(ct, ops, c, words):
    dy, h = cc.nhwc(c.dy).to(DEV), cc.nhwc(c.x).to(DEV)
    if not words:
        return ct.conv_wgrad(dy, h, c.wshape, c.stride)
    return ct.conv_wgrad(dy, h, c.wshape, c.stride, ops.absmax_word(dy), ops.absmax_word(h))


def _wgrad_strip(ops, c):
    """sd_conv_wgrad on the strip-walking path with the TEST's scratch, handed over full of NaNs: -> (dW, scratch).  Every partial tile
    of the first launch - empty groups' included - must have been written (no NaN left), which also shows that this path ran: the per-wave
    kernel, which the host falls back to quietly on a misaligned pointer or under SD_WGRAD_SIMPLE, writes no scratch."""
    from soccerdiffusion_amd import _lib
    from soccerdiffusion_amd._lib import check

    lib = _lib.load()
    dy, h = cc.nhwc(c.dy).to(DEV), cc.nhwc(c.x).to(DEV)
    wy, wh = ops.absmax_word(dy), ops.absmax_word(h)
    n = lib.sd_conv_wgrad_scratch_floats(c.N, c.H, c.W, c.Cin, c.Cout, c.k, c.stride)
    assert n > 0
    scratch = torch.full((n,), float("nan"), dtype=torch.float32, device=DEV)
    dw = torch.zeros(*c.wshape, dtype=torch.float32, device=DEV)
    check(lib.sd_conv_wgrad(dy.data_ptr(), h.data_ptr(), wy.data_ptr(), wh.data_ptr(), dw.data_ptr(), scratch.data_ptr(), c.N, c.H, c.W, c.Cin,
                            c.Cout, c.k, c.stride, ops._stream()), "sd_conv_wgrad")
    return dw, scratch


@pytest.mark.parametrize("cid,kw", cc.wgrad_strip_cases(), ids=[c for c, _ in cc.wgrad_strip_cases()])
def test_conv_wgrad_strip_walking_is_fp32_grade(ct, ops, cid, kw):
    """conv_wgrad3_kernel + wgrad3_reduce_kernel: groups that start mid-strip, empty groups (their partial tiles are summed: the test's own
    scratch is handed over full of NaNs), the four parity-class launches of stride 2 with their empty classes."""
    c = cc.wgrad_case(**kw)
    dw, scratch = _wgrad_strip(ops, c)
    assert not torch.isnan(scratch).any()                        # the strip-walking path ran and wrote every partial tile, empty groups' too
    cc.grade_dw(dw, c.want64, c.want32, c.label, row_self=c.row_self, **cc.gate_of("strip-" + cid))
    assert torch.equal(dw, _wgrad_strip(ops, c)[0])             # no atomics: deterministic
    assert torch.equal(dw, _wgrad(ct, ops, c, True))            # ... and conv_training.conv_wgrad runs the same path


@pytest.mark.parametrize("cid,kw,words", cc.wgrad_wave_cases(), ids=[c for c, _, _ in cc.wgrad_wave_cases()])
def test_conv_wgrad_per_wave_is_fp32_grade(ct, ops, cid, kw, words):
    """conv_wgrad_kernel: 1 x 1 at both strides, 3 x 3 without abs-max words (fp32 atomics into dW: no bit-stability asserted)."""
    c = cc.wgrad_case(**kw)
    cc.grade_dw(_wgrad(ct, ops, c, words), c.want64, c.want32, c.label + (" words" if words else " blocks"), row_self=c.row_self,
                **cc.gate_of("wave-" + cid))


@pytest.mark.parametrize("cid,kw", cc.stem_wgrad_cases(), ids=[c for c, _ in cc.stem_wgrad_cases()])
def test_stem_wgrad_is_fp32_grade(ct, ops, cid, kw):
    c = cc.stem_wgrad_case(**kw)
    dy, x = cc.nhwc(c.dy).to(DEV), c.x.to(DEV)

    def run():
        return ct.stem_wgrad(dy, x, ops.absmax_word(dy), ops.absmax_word(x))

    dw = run()
    cc.grade_dw(dw, c.want64, c.want32, c.label, **cc.gate_of("stemw-" + cid))
    assert torch.equal(dw, run())


# ---- data gradients --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,kw", cc.dgrad_cases(), ids=[c for c, _ in cc.dgrad_cases()])
def test_data_gradients_are_fp32_grade(ct, ops, cid, kw):
    """conv_raw on the PackedPair's backward planes (stride 1), sd_convt3x3_s2 and sd_convt1x1_s2 (stride 2), graded per pixel: a parity
    class of the stride-2 result is a quarter of the pixels and not lost in a norm.  The 1 x 1 shortcut writes one class: the rest is zero."""
    c = cc.dgrad_case(**kw)
    _, bwd = ct.PackedPair().get(c.w.to(DEV))
    dy = cc.nhwc(c.dy).to(DEV)

    def run():
        word = ops.absmax_word(dy)
        if c.stride == 1:
            return ct.conv_raw(dy, word, bwd, 1)
        if c.k == 3:
            return ct.convt3x3_s2(dy, word, bwd, c.H, c.W)
        return ct.convt1x1_s2(dy, word, bwd, c.H, c.W)

    dx = run()
    assert tuple(dx.shape) == (c.N, c.H, c.W, c.Cin)
    cc.grade(cc.nchw(dx), c.want64, c.want32, c.label, **cc.gate_of("dgrad-" + cid))
    assert torch.equal(dx, run())
    if c.stride == 2 and c.k == 1:
        assert not dx[:, 1::2].any() and not dx[:, :, 1::2].any()   # the three unwritten parity classes: exact zeros


# ---- the encoder heads (sd_head.hip) -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,kw", cc.head_cases(), ids=[c for c, _ in cc.head_cases()])
def test_heads_forward_and_backward_are_fp32_grade(ct, cid, kw):
    c = cc.head_case(**kw)
    names = ("x", "conv_w", "conv_b", "fc_w", "fc_b")

    def run():
        leaves = [c.t[k].detach().to(DEV).requires_grad_() if k in c.t else None for k in names]
        for p in leaves[1:]:       # the kernels add into existing .grad buffers (an optimizer's): zeros, so the sum is the gradient
            if p is not None:
                p.grad = torch.zeros_like(p)
        y = ct.ResNetHead.apply(*leaves)
        y.backward(c.dy.to(DEV))
        return y.detach(), {k: p.grad for k, p in zip(names, leaves) if p is not None}

    y, grads = run()
    v = lambda t: t.detach().cpu().reshape(c.N, 1, c.d)   # noqa: E731  per image
    parity.assert_fp32_grade(v(y), v(c.y64), v(c.y32), label=c.label + " y")
    rows = lambda k, t: t.detach().cpu().reshape(-1, c.C) if k == "x" else t.detach().cpu()   # noqa: E731  x: rows = pixels
    parity.assert_grads_fp32_grade({k: rows(k, g) for k, g in grads.items()}, {k: rows(k, g) for k, g in c.g64.items()},
                                   {k: rows(k, g) for k, g in c.g32.items()}, label=c.label)
    y2, grads2 = run()
    assert torch.equal(y, y2) and all(torch.equal(grads[k], grads2[k]) for k in grads)
