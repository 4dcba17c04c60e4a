"""Fine-tuning on frozen BatchNorm statistics on the hand-written kernels (csrc/sd_conv_train.hip: sd_bn_frozen_*; conv_training.py:
FrozenConvBNUnit and the frozen stem twins; image.freeze_batchnorm): every result against the same tensors through tests/frozen_bn_ref.py /
the same torch modules on the CPU in fp64.  Bars: rel_err < 1e-5 per kernel (what test_gpu_conv_training.py holds the train-mode kernels
to); whole-network gradients: max(2e-5, 1.5 x the error of the same modules' fp32 CPU run against fp64)."""

import copy

import pytest
import torch
import torch.nn.functional as F

import frozen_bn_ref as ref
from conftest import rel_err

pytestmark = pytest.mark.gpu
EPS = 1e-5


def _word_value(word):
    return float(torch.tensor([int(word.item())], dtype=torch.int32).view(torch.float32))


def _bn_case(C, g):
    gamma = torch.rand(C, generator=g) + 0.5
    gamma[3], gamma[C // 2] = 0.0, -0.8   # a dead channel and a negative scale
    return gamma, torch.randn(C, generator=g), torch.randn(C, generator=g), torch.rand(C, generator=g) * 2 + 0.25


@pytest.mark.parametrize("affine_grad", [True, False], ids=["affine-trained", "affine-frozen"])
@pytest.mark.parametrize("N,H,W,C,relu,with_res", [(2, 9, 11, 64, True, True), (3, 8, 8, 128, False, False), (1, 5, 7, 512, True, False),
                                                    (2, 30, 40, 256, True, True)])
def test_frozen_bn_kernels_match_fp64(N, H, W, C, relu, with_res, affine_grad):
    from soccerdiffusion_amd import conv_training as ct

    g = torch.Generator().manual_seed(C + H)
    y = torch.randn(N, H, W, C, generator=g) * 2 + 3.0
    gamma, beta, rm, rv = _bn_case(C, g)
    res = torch.randn(N, H, W, C, generator=g) if with_res else None
    dz = torch.randn(N, H, W, C, generator=g)
    rm_g, rv_g = rm.cuda(), rv.cuda()
    s, t, rstd = ct.bn_frozen_fold(gamma.cuda(), beta.cuda(), rm_g, rv_g, EPS)
    s_ref, t_ref, rstd_ref = ref.fold(gamma, beta, rm, rv, EPS)
    assert rel_err(s, s_ref) < 1e-6 and rel_err(t, t_ref) < 1e-6 and rel_err(rstd, rstd_ref) < 1e-6
    assert float(s[3]) == 0.0 and float(s[C // 2]) < 0.0
    z, word = ct.bn_frozen_fwd(y.cuda(), s, t, res.cuda() if with_res else None, relu)
    assert torch.equal(rm_g.cpu(), rm) and torch.equal(rv_g.cpu(), rv)   # the statistics are read, never written
    want_z = ref.forward(y, gamma, beta, rm, rv, EPS, res, relu)
    assert rel_err(z, want_z) < 2e-6
    assert _word_value(word) == float(z.abs().max())
    # the backward on the GPU's own z (the mask is its sign): the kernels' error, free of a mask flipped by fp32 rounding upstream
    want_dy, want_dres, want_dgamma, want_dbeta = ref.backward(dz, z.cpu(), y, gamma, rm, rv, EPS, relu)

    def run(z_arg):
        return ct.bn_frozen_bwd(dz.cuda(), z_arg, y.cuda() if affine_grad else None, s, t, rm_g, rstd, relu, with_res, affine_grad)

    dy, dword, dgamma, dbeta, dres = run(z if relu else None)
    assert rel_err(dy, want_dy) < 1e-5
    assert int(dword.item()) == int(dy.abs().max().reshape(1).view(torch.int32).item())   # the abs-max word IS max |dy|, bit for bit
    assert bool((dy[..., 3] == 0).all())
    if with_res:
        assert torch.equal(dres.cpu(), want_dres.float())   # g is dz or 0: exact
    else:
        assert dres is None
    if affine_grad:
        assert rel_err(dgamma, want_dgamma) < 1e-5 and rel_err(dbeta, want_dbeta) < 1e-5
    else:
        assert dgamma is None and dbeta is None
    again = run(z if relu else None)
    for a, b in zip((dy, dword, dgamma, dbeta, dres), again):
        assert (a is None and b is None) or torch.equal(a, b)   # two runs: the same bits (no atomics in the sums)
    if affine_grad and relu and not with_res:   # the mask recomputed from y (z = None): the same mask, bit for bit
        for a, b in zip((dy, dword, dgamma, dbeta), run(None)):
            assert torch.equal(a, b)


CONV_UNITS = [(2, 5, 7, 64, 64, 3, 1, True, True), (2, 9, 11, 64, 128, 3, 2, True, False), (2, 9, 11, 64, 128, 1, 2, False, False)]


@pytest.mark.parametrize("affine_grad", [True, False], ids=["affine-trained", "affine-frozen"])
@pytest.mark.parametrize("N,H,W,Cin,Cout,k,stride,relu,with_res", CONV_UNITS, ids=["3x3-s1-res-relu", "3x3-s2-odd", "1x1-s2-shortcut"])
def test_frozen_conv_units_match_fp64(N, H, W, Cin, Cout, k, stride, relu, with_res, affine_grad):
    """conv + frozen BatchNorm (+ res) (+ ReLU) through conv_training.unit with pass_input: z, dW, dh (the passed-through input's gradient joined
    in the data-gradient epilogue), dres, dgamma, dbeta; the statistics untouched."""
    from soccerdiffusion_amd import conv_training as ct
    from soccerdiffusion_amd import ops

    g = torch.Generator().manual_seed(Cin + Cout + k + stride)
    h = torch.randn(N, H, W, Cin, generator=g)
    conv = torch.nn.Conv2d(Cin, Cout, k, stride=stride, padding=k // 2, bias=False)
    bn = torch.nn.BatchNorm2d(Cout, eps=EPS)
    gamma, beta, rm, rv = _bn_case(Cout, g)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, generator=g) * 0.05)
        bn.weight.copy_(gamma), bn.bias.copy_(beta), bn.running_mean.copy_(rm), bn.running_var.copy_(rv)
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    res = torch.randn(N, Ho, Wo, Cout, generator=g) if with_res else None
    wz, wp = torch.randn(N, Ho, Wo, Cout, generator=g), torch.randn(N, H, W, Cin, generator=g)
    # fp64 reference under autograd
    hd, wd = h.double().requires_grad_(), conv.weight.detach().double().requires_grad_()
    gd, bd = gamma.double().requires_grad_(), beta.double().requires_grad_()
    rd = res.double().requires_grad_() if with_res else None
    z_ref = ref.unit(hd, wd, gd, bd, rm.double(), rv.double(), EPS, stride, rd, relu)
    ((z_ref * wz.double()).sum() + (hd * wp.double()).sum()).backward()
    # ours
    conv, bn = conv.cuda(), bn.cuda().eval()
    bn.weight.requires_grad_(affine_grad), bn.bias.requires_grad_(affine_grad)
    hg = h.cuda().requires_grad_()
    rg = res.cuda().requires_grad_() if with_res else None
    z, word, hp = ct.unit(hg, ops.absmax_word(hg.detach()), conv, bn, rg, relu, ct.PackedPair(), pass_input=True)
    assert rel_err(z, z_ref) < 2e-6 and _word_value(word) == float(z.detach().abs().max())
    ((z * wz.cuda()).sum() + (hp * wp.cuda()).sum()).backward()
    assert rel_err(conv.weight.grad, wd.grad) < 1e-5
    assert rel_err(hg.grad, hd.grad) < 1e-5
    if with_res:
        assert rel_err(rg.grad, rd.grad) < 1e-6
    if affine_grad:
        assert rel_err(bn.weight.grad, gd.grad) < 1e-5 and rel_err(bn.bias.grad, bd.grad) < 1e-5
    else:
        assert bn.weight.grad is None and bn.bias.grad is None
    assert torch.equal(bn.running_mean.cpu(), rm) and torch.equal(bn.running_var.cpu(), rv) and int(bn.num_batches_tracked) == 0


@pytest.mark.parametrize("affine_grad", [True, False], ids=["affine-trained", "affine-frozen"])
def test_frozen_stem_matches_fp64(affine_grad):
    """The stem on frozen statistics: frames 2 x 3 x 37 x 45 through stem_pool_unit (sd_stem_conv_raw, the frozen BatchNorm + ReLU + max-pool
    twin, sd_stem_wgrad) and, on the same convolution output, through bn_pool_unit."""
    from soccerdiffusion_amd import conv_training as ct
    from soccerdiffusion_amd import ops

    g = torch.Generator().manual_seed(37)
    x = torch.rand(2, 3, 37, 45, generator=g)
    conv = torch.nn.Conv2d(3, 64, 7, stride=2, padding=3, bias=False)
    bn = torch.nn.BatchNorm2d(64, eps=EPS)
    gamma, beta, rm, rv = _bn_case(64, g)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, generator=g) * 0.1)
        bn.weight.copy_(gamma), bn.bias.copy_(beta * 0.3), bn.running_mean.copy_(rm * 0.3), bn.running_var.copy_(rv)
    beta, rm = beta * 0.3, rm * 0.3
    wd, gd, bd = conv.weight.detach().double().requires_grad_(), gamma.double().requires_grad_(), beta.double().requires_grad_()
    y_ref = F.conv2d(x.double(), wd, stride=2, padding=3)
    p_ref = F.max_pool2d(F.batch_norm(y_ref, rm.double(), rv.double(), gd, bd, training=False, eps=EPS).relu(), 3, 2, 1).permute(0, 2, 3, 1)
    dp = torch.randn(p_ref.shape, generator=g)
    p_ref.backward(dp.double())
    conv, bn = conv.cuda(), bn.cuda().eval()
    bn.weight.requires_grad_(affine_grad), bn.bias.requires_grad_(affine_grad)
    p, word = ct.stem_pool_unit(x.cuda(), conv, bn, ops.PackedStem(conv.weight))
    assert tuple(p.shape) == tuple(p_ref.shape) and rel_err(p, p_ref) < 2e-6 and _word_value(word) == float(p.abs().max())
    p.backward(dp.cuda())
    assert rel_err(conv.weight.grad, wd.grad) < 1e-5
    if affine_grad:
        assert rel_err(bn.weight.grad, gd.grad) < 1e-5 and rel_err(bn.bias.grad, bd.grad) < 1e-5
    else:
        assert bn.weight.grad is None and bn.bias.grad is None
    assert torch.equal(bn.running_mean.cpu(), rm) and torch.equal(bn.running_var.cpu(), rv) and int(bn.num_batches_tracked) == 0
    # the kernels alone, on one y: pooled map, winners (through dy) and the abs-max word against the reference's own formulas
    y = torch.randn(2, 19, 23, 64, generator=g) * 1.5 + 0.3
    s, t, rstd = ct.bn_frozen_fold(bn.weight.detach(), bn.bias.detach(), bn.running_mean, bn.running_var, EPS)
    pk, pword, idx = ct.bn_frozen_relu_pool_fwd(y.cuda(), s, t)
    want_p, _ = ref.pool_forward(y, gamma, beta, rm, rv, EPS)
    assert rel_err(pk, want_p) < 2e-6
    dpk = torch.randn(want_p.shape, generator=g)
    dy, dword, dgamma, dbeta = ct.bn_frozen_relu_pool_bwd(dpk.cuda(), idx, y.cuda(), s, bn.running_mean, rstd, affine_grad)
    want_dy, want_dgamma, want_dbeta = ref.pool_backward(dpk, y, gamma, beta, rm, rv, EPS)
    assert rel_err(dy, want_dy) < 1e-5 and int(dword.item()) == int(dy.abs().max().reshape(1).view(torch.int32).item())
    if affine_grad:
        assert rel_err(dgamma, want_dgamma) < 1e-5 and rel_err(dbeta, want_dbeta) < 1e-5
    dy2, dword2, dgamma2, dbeta2 = ct.bn_frozen_relu_pool_bwd(dpk.cuda(), idx, y.cuda(), s, bn.running_mean, rstd, affine_grad)
    assert torch.equal(dy2, dy) and torch.equal(dword2, dword) and (not affine_grad or (torch.equal(dgamma2, dgamma) and torch.equal(dbeta2, dbeta)))
    # ... and the same through BNPoolUnit's frozen twin (behind torch's convolution when the frames need a gradient)
    yg = y.cuda().requires_grad_()
    p2, _ = ct.bn_pool_unit(yg, bn)
    p2.backward(dpk.cuda())
    assert torch.equal(p2.detach(), pk) and torch.equal(yg.grad, dy)


# ---- whole encoders --------------------------------------------------------------------------------------------------------------
class _Counts:
    """Counts the calls of conv_training's launch wrappers and units while a block runs."""

    NAMES = ("bn_train_fwd", "bn_train_bwd", "bn_frozen_fwd", "bn_frozen_bwd", "bn_relu_pool_fwd", "bn_frozen_relu_pool_fwd", "bn_frozen_fold")
    UNITS = ("ConvBNUnit", "FrozenConvBNUnit", "StemPoolUnit", "FrozenStemPoolUnit")

    def __enter__(self):
        from soccerdiffusion_amd import conv_training as ct

        self.ct, self.n, self.saved, self.affine = ct, {k: 0 for k in self.NAMES + self.UNITS}, {}, []

        def spy(name, fn):
            def wrapped(*a, **k):
                self.n[name] += 1
                if name == "bn_frozen_bwd":
                    self.affine.append(a[-1])
                return fn(*a, **k)
            return wrapped

        for name in self.NAMES:
            self.saved[name] = getattr(ct, name)
            setattr(ct, name, spy(name, self.saved[name]))
        for name in self.UNITS:
            cls = getattr(ct, name)
            self.saved[name] = cls.apply
            cls.apply = spy(name, cls.apply)
        return self

    def __exit__(self, *exc):
        for name in self.NAMES:
            setattr(self.ct, name, self.saved[name])
        for name in self.UNITS:
            getattr(self.ct, name).apply = self.saved[name]


def _bns(net):
    return [m for m in net.modules() if isinstance(m, torch.nn.BatchNorm2d)]


def _stat_buffers(net):
    return {k: v.clone() for k, v in net.state_dict().items() if k.endswith(("running_mean", "running_var", "num_batches_tracked"))}


def _warm_encoder(avgpool, seed):
    """A ResNet-18 image encoder (CPU, fp32) with non-trivial affine pairs, its running statistics made non-trivial by one train-mode forward."""
    from soccerdiffusion_amd.ml.model.encoder.image import ImageEncoderType, ResNetImageEncoder

    torch.manual_seed(seed)
    enc = ResNetImageEncoder(ImageEncoderType.RESNET18, 32, avgpool, 64)
    with torch.no_grad():
        for m in _bns(enc):
            m.weight.uniform_(0.5, 1.5)
            m.bias.normal_(0, 0.2)
    enc.train()
    with torch.no_grad():
        enc(torch.rand(2, 2, 3, 64, 64, generator=torch.Generator().manual_seed(seed + 1)))
    return enc


def _run(enc, x, wr):
    tokens = enc(x)
    (tokens * wr).sum().backward()
    return tokens.detach()


def _compare_with_cpu(base, prepare, x, wr):
    """The encoder ``base`` prepared by ``prepare(copy)`` on the CPU in fp64 and fp32 and on the GPU: tokens, every parameter gradient under
    the rule max(2e-5, 1.5 x the fp32 CPU run's own error), -> (the GPU copy, its _Counts, the fp64 copy)."""
    r64, r32, gpu = prepare(copy.deepcopy(base).double()), prepare(copy.deepcopy(base)), prepare(copy.deepcopy(base).cuda())
    t64, t32 = _run(r64, x.double(), wr.double()), _run(r32, x, wr)
    with _Counts() as counts:
        tg = _run(gpu, x.cuda(), wr.cuda())
    p64, p32, pg = dict(r64.named_parameters()), dict(r32.named_parameters()), dict(gpu.named_parameters())
    own = {n: rel_err(p32[n].grad, p.grad) for n, p in p64.items() if p.grad is not None}
    bar = max(2e-5, 1.5 * max(own.values()))
    errs = {n: rel_err(pg[n].grad, p.grad) for n, p in p64.items() if p.grad is not None}
    print("token error", rel_err(tg, t64), "(fp32 CPU:", rel_err(t32, t64), ") bar", bar, "worst:", sorted(errs.items(), key=lambda kv: -kv[1])[:4])
    assert rel_err(tg, t64) < 1e-5
    for n, p in p64.items():
        assert (p.grad is None) == (pg[n].grad is None), n
    for n, e in errs.items():
        assert e < bar, (n, e, own[n], bar)
    return gpu, counts, r64


@pytest.mark.parametrize("affine", [False, True], ids=["stats", "all"])
@pytest.mark.parametrize("avgpool", [True, False], ids=["avgpool-head", "conv-head"])
def test_frozen_resnet18_encoder_matches_torch_cpu_fp64(avgpool, affine):
    """2 windows x 2 frames at 64 x 64 through ResNetImageEncoder in train() mode with every BatchNorm frozen: tokens, every parameter gradient,
    the statistics bitwise as they were, and which launches ran."""
    from soccerdiffusion_amd.ml.model.encoder.image import freeze_batchnorm

    base = _warm_encoder(avgpool, 11)
    x = torch.rand(2, 2, 3, 64, 64, generator=torch.Generator().manual_seed(12))
    wr = torch.randn(2, 2, 32, generator=torch.Generator().manual_seed(13))
    before = _stat_buffers(base)
    assert all(int(v) == 1 for k, v in before.items() if k.endswith("num_batches_tracked"))
    gpu, counts, _ = _compare_with_cpu(base, lambda e: freeze_batchnorm(e, affine=affine).train(), x, wr)
    assert gpu.encoder.training and all(not m.training for m in _bns(gpu))
    for k, v in _stat_buffers(gpu).items():
        assert torch.equal(v.cpu(), before[k]), k   # (on the parent commit these were overwritten with batch statistics)
    n = counts.n
    assert n["FrozenConvBNUnit"] == 19 and n["FrozenStemPoolUnit"] == 1 and n["ConvBNUnit"] == 0 and n["StemPoolUnit"] == 0
    assert n["bn_train_fwd"] == 0 and n["bn_train_bwd"] == 0 and n["bn_relu_pool_fwd"] == 0
    assert n["bn_frozen_bwd"] == 19 and n["bn_frozen_relu_pool_fwd"] == 1 and n["bn_frozen_fold"] == 20
    assert n["bn_frozen_fwd"] == (0 if affine else 19)   # all: the inference launch is the whole forward of a unit, no apply launch
    assert counts.affine == [not affine] * 19
    for m in _bns(gpu):
        assert (m.weight.grad is None) == affine and (m.bias.grad is None) == affine


def test_mixed_backbone_runs_unit_by_unit():
    """layer1 - 2 frozen, the stem and layer3 - 4 on batch statistics: the frozen layers' statistics stay, the others move as torch moves them."""
    from soccerdiffusion_amd.ml.model.encoder.image import freeze_batchnorm

    base = _warm_encoder(True, 21)
    x = torch.rand(2, 2, 3, 64, 64, generator=torch.Generator().manual_seed(22))
    wr = torch.randn(2, 2, 32, generator=torch.Generator().manual_seed(23))
    before = _stat_buffers(base)

    def prepare(e):
        freeze_batchnorm(e.encoder.layer1)
        freeze_batchnorm(e.encoder.layer2, affine=True)
        return e.train()

    gpu, counts, r64 = _compare_with_cpu(base, prepare, x, wr)
    n = counts.n
    assert n["FrozenConvBNUnit"] == 9 and n["ConvBNUnit"] == 10 and n["StemPoolUnit"] == 1 and n["FrozenStemPoolUnit"] == 0
    assert n["bn_train_fwd"] == 10 and n["bn_train_bwd"] == 10 and n["bn_frozen_fwd"] == 4 and n["bn_frozen_bwd"] == 9
    want = _stat_buffers(r64)
    for k, v in _stat_buffers(gpu).items():
        if k.startswith(("encoder.layer1", "encoder.layer2")):
            assert torch.equal(v.cpu(), before[k]), k
        elif k.endswith("num_batches_tracked"):
            assert int(v) == int(want[k]) == 2, k
        else:
            assert rel_err(v, want[k]) < 1e-5 and not torch.equal(v.cpu(), before[k]), k


@pytest.mark.parametrize("affine", [False, True], ids=["stats", "all"])
def test_frozen_bottleneck_stage_entry_block(affine):
    """ResNet-50's layer-2 entry block (1 x 1, 3 x 3 stride 2, 1 x 1 + the 1 x 1 stride-2 shortcut) frozen, through forward_train_nhwc."""
    from soccerdiffusion_amd import ops
    from soccerdiffusion_amd.ml.model.encoder.image import _Bottleneck, freeze_batchnorm

    torch.manual_seed(31)
    blk = _Bottleneck(256, 128, 2)
    g = torch.Generator().manual_seed(32)
    with torch.no_grad():
        for m in _bns(blk):
            m.weight.uniform_(0.5, 1.5), m.bias.normal_(0, 0.2), m.running_mean.normal_(0, 0.3), m.running_var.uniform_(0.5, 1.5)
    freeze_batchnorm(blk, affine=affine).train()
    before = _stat_buffers(blk)
    h = torch.randn(2, 9, 11, 256, generator=g)
    wz = torch.randn(2, 5, 6, 512, generator=g)
    r64 = copy.deepcopy(blk).double()
    hd = h.double().requires_grad_()
    out_ref = r64(hd.permute(0, 3, 1, 2)).permute(0, 2, 3, 1)
    (out_ref * wz.double()).sum().backward()
    gpu = copy.deepcopy(blk).cuda()
    assert gpu.training and all(not m.training for m in _bns(gpu))
    hg = h.cuda().requires_grad_()
    with _Counts() as counts:
        out, word = gpu.forward_train_nhwc(hg, ops.absmax_word(hg.detach()))
        (out * wz.cuda()).sum().backward()
    assert counts.n["FrozenConvBNUnit"] == 4 and counts.n["ConvBNUnit"] == 0 and counts.n["bn_frozen_fwd"] == (0 if affine else 4)
    assert rel_err(out, out_ref) < 1e-5 and _word_value(word) == float(out.abs().max())
    assert rel_err(hg.grad, hd.grad) < 2e-5
    pr = dict(r64.named_parameters())
    for name, p in gpu.named_parameters():
        if pr[name].grad is None:
            assert p.grad is None, name
        else:
            assert rel_err(p.grad, pr[name].grad) < 2e-5, name
    for k, v in _stat_buffers(gpu).items():
        assert torch.equal(v.cpu(), before[k]), k


def test_nothing_frozen_runs_what_it_ran_before():
    """A backbone whose BatchNorm layers are all in training mode: the same 19 bn_train_fwd / bn_train_bwd calls and the train-mode stem, no
    frozen launch; after unfreeze_batchnorm as well."""
    from soccerdiffusion_amd.ml.model.encoder.image import freeze_batchnorm, unfreeze_batchnorm

    base = _warm_encoder(True, 41)
    x = torch.rand(2, 2, 3, 64, 64, generator=torch.Generator().manual_seed(42)).cuda()
    wr = torch.randn(2, 2, 32, generator=torch.Generator().manual_seed(43)).cuda()
    plain = copy.deepcopy(base).cuda().train()
    thawed = unfreeze_batchnorm(freeze_batchnorm(copy.deepcopy(base).cuda(), affine=True)).train()
    tokens = []
    for enc in (plain, thawed):
        with _Counts() as counts:
            tokens.append(_run(enc, x, wr))
        n = counts.n
        assert n["bn_train_fwd"] == 19 and n["bn_train_bwd"] == 19 and n["ConvBNUnit"] == 19 and n["StemPoolUnit"] == 1 and n["bn_relu_pool_fwd"] == 1
        assert all(n[k] == 0 for k in ("bn_frozen_fwd", "bn_frozen_bwd", "bn_frozen_fold", "bn_frozen_relu_pool_fwd", "FrozenConvBNUnit", "FrozenStemPoolUnit"))
        assert all(int(m.num_batches_tracked) == 2 for m in _bns(enc))
    assert torch.equal(tokens[0], tokens[1])


def test_unsupported_batchnorm_keeps_torch_nn_for_the_whole_backbone():
    base = _warm_encoder(True, 51).cuda().train()
    x = torch.rand(1, 2, 3, 64, 64, generator=torch.Generator().manual_seed(52)).cuda()
    bn = base.encoder.layer3[0].bn1
    bn.momentum = None
    with _Counts() as counts:
        base(x).sum().backward()
    assert all(v == 0 for v in counts.n.values())
    bn.momentum = 0.1
    with _Counts() as counts:   # the decision follows the module's flags
        base(x).sum().backward()
    assert counts.n["ConvBNUnit"] == 19


@pytest.mark.parametrize("mode", ["all", "stats"])
def test_captured_step_with_freeze_bn_replays_the_eager_step(mode):
    """--freeze-bn on a tiny image-conditioned model: one eager step (it warms the lazy initialisations up, as GraphedTrainStep's callers
    do), then three GraphedTrainStep replays with the optimizer's updates in between leave losses, parameters and moments bit-equal to four
    eager train_steps.  The fold of s, t runs inside the capture: with "stats" the optimizer moves gamma and beta between the replays.
    The shape - two windows of one 8 x 8 frame - is the one at which the EAGER step itself repeats bit for bit: the 1 x 1 / stride-2
    shortcuts' weight gradient (sd_conv_wgrad's per-wave kernel) adds one partial tile per output image row with fp32 atomics, and only up
    to two of them add in a fixed order.  At 2 x 2 frames of 64 x 64 (32 rows at layer2's shortcut) two eager runs of this step differ in
    exactly those three gradients after the first step and in the last bit of the fourth loss - frozen or not, before and after this test's
    feature.  Two rows per shortcut here."""
    from test_gpu_image_path import _model

    from soccerdiffusion_amd import cli, training
    from soccerdiffusion_amd.scheduler import DDIMScheduler

    dev = torch.device("cuda:0")
    B, Fr, R = 2, 1, 8
    g = torch.Generator().manual_seed(61)
    data = {"joint_command_history": torch.randn(B, 20, 20, generator=g).to(dev), "image_data": torch.rand(B, Fr, 3, R, R, generator=g).to(dev),
            "game_state": torch.randint(0, 4, (B,), generator=g).to(dev)}
    target = torch.randn(B, 12, 20, generator=g).to(dev)

    def setup():
        m = _model(dev, R=R, F=Fr)
        with torch.no_grad():
            for bn in _bns(m):
                bn.running_mean.normal_(0, 0.1), bn.running_var.uniform_(0.5, 1.5)
        cli.apply_freeze_bn(m, mode)
        m.train().set_dropout(0.0)
        opt = training.FusedAdamW(m.parameters(), lr=1e-3)
        sch = DDIMScheduler(beta_schedule="squaredcos_cap_v2", clip_sample=False)
        return m, opt, sch, torch.Generator(device=dev).manual_seed(62)

    m, opt, sch, gen = setup()   # (_model seeds torch itself: both replicas start from the same weights and statistics)
    stats = _stat_buffers(m.image_sequence_encoder)
    eager = [float(training.train_step(m, opt, None, sch, target, input_data=data, generator=gen)) for _ in range(4)]
    for k, v in _stat_buffers(m.image_sequence_encoder).items():
        assert torch.equal(v, stats[k]), k
    m2, opt2, sch2, gen2 = setup()
    gs = training.GraphedTrainStep(m2, opt2, None, sch2, generator=gen2, eager_steps=1)
    try:
        replayed = []
        for k in range(4):
            replayed.append(float(gs(target, input_data=data)))
            assert (gs.graph is not None) == (k >= 1)
    finally:
        gs.close()
    print("eager", eager, "replayed", replayed)
    assert replayed == eager
    assert torch.equal(opt2.flat_param, opt.flat_param) and torch.equal(opt2.flat_m, opt.flat_m) and torch.equal(opt2.flat_v, opt.flat_v)
    for k, v in _stat_buffers(m2.image_sequence_encoder).items():
        assert torch.equal(v, stats[k]), k
