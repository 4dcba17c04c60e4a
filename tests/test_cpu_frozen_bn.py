"""Fine-tuning on frozen BatchNorm statistics, the parts that need no GPU: the per-unit route table (conv_training.bn_route), freeze_batchnorm /
unfreeze_batchnorm, the --freeze-bn / --pretrained-backbone flags and the checkpoint key, and the fp64 reference (tests/frozen_bn_ref.py)
against torch's own F.batch_norm(training=False) under autograd."""

import copy
import itertools

import pytest
import torch
import torch.nn.functional as F

import frozen_bn_ref as ref


def _facts(**kw):
    base = dict(training=False, affine=True, track_running_stats=True, has_running_stats=True, momentum_is_none=False, affine_requires_grad=True)
    base.update(kw)
    return base


def test_route_table():
    from soccerdiffusion_amd.conv_training import bn_route

    assert bn_route(**_facts(training=True)) == "train"
    assert bn_route(**_facts(training=True, affine_requires_grad=False)) == "train"
    assert bn_route(**_facts(training=True, track_running_stats=False, has_running_stats=False)) == "train"
    assert bn_route(**_facts(training=True, track_running_stats=False, has_running_stats=False, momentum_is_none=True)) == "train"
    assert bn_route(**_facts(training=True, momentum_is_none=True)) == "torch"          # a cumulative average
    assert bn_route(**_facts()) == "frozen_stats"                                        # torch's plain bn.eval()
    assert bn_route(**_facts(momentum_is_none=True)) == "frozen_stats"                   # (momentum plays no part on frozen statistics)
    assert bn_route(**_facts(affine_requires_grad=False)) == "frozen_all"
    assert bn_route(**_facts(track_running_stats=False, has_running_stats=False)) == "torch"   # eval() without statistics: batch statistics
    assert bn_route(**_facts(has_running_stats=False)) == "torch"
    # whatever else holds, a layer without an affine pair is not on the kernels; and the function is total over its facts
    for combo in itertools.product((False, True), repeat=5):
        t, tr, h, m, g = combo
        assert bn_route(training=t, affine=False, track_running_stats=tr, has_running_stats=h, momentum_is_none=m, affine_requires_grad=g) == "torch"
        assert bn_route(training=t, affine=True, track_running_stats=tr, has_running_stats=h, momentum_is_none=m,
                        affine_requires_grad=g) in ("train", "frozen_stats", "frozen_all", "torch")


def test_bn_facts_read_the_module():
    from soccerdiffusion_amd.conv_training import bn_facts, bn_route

    bn = torch.nn.BatchNorm2d(64)
    assert bn_route(**bn_facts(bn)) == "train"
    bn.eval()
    assert bn_route(**bn_facts(bn)) == "frozen_stats"
    bn.weight.requires_grad_(False)
    assert bn_route(**bn_facts(bn)) == "frozen_stats"   # the bias still needs its gradient
    bn.bias.requires_grad_(False)
    assert bn_route(**bn_facts(bn)) == "frozen_all"
    assert bn_route(**bn_facts(torch.nn.BatchNorm2d(64, track_running_stats=False).eval())) == "torch"
    assert bn_route(**bn_facts(torch.nn.BatchNorm2d(64, momentum=None))) == "torch"
    assert bn_route(**bn_facts(torch.nn.BatchNorm2d(64, affine=False).eval())) == "torch"


def _small_resnet():
    from soccerdiffusion_amd.ml.model.encoder.image import _BasicBlock, _ResNet

    torch.manual_seed(0)
    net = _ResNet(_BasicBlock, [1, 1, 1, 1])
    net.fc = torch.nn.Linear(512, 8)
    return net


def _bns(net):
    return [m for m in net.modules() if isinstance(m, torch.nn.BatchNorm2d)]


def test_freeze_is_sticky_and_leaves_the_statistics_alone():
    from soccerdiffusion_amd.ml.model.encoder.image import freeze_batchnorm

    net = _small_resnet()
    net.train()
    net(torch.rand(2, 3, 32, 32))   # non-trivial running statistics
    assert freeze_batchnorm(net) is net
    net.train()
    assert net.training and net.layer1[0].training and all(not m.training for m in _bns(net))
    outer = torch.nn.Sequential(net)   # a parent's train() reaches the backbone's
    outer.eval()
    outer.train()
    assert all(not m.training for m in _bns(net))
    assert all(not m.training for m in _bns(copy.deepcopy(net).train()))   # the mark travels with a copy
    before = {k: v.clone() for k, v in net.state_dict().items() if "running" in k or "num_batches" in k}
    out = net(torch.rand(2, 3, 32, 32))
    out.sum().backward()
    for k, v in before.items():
        assert torch.equal(net.state_dict()[k], v), k
    assert all(m.weight.grad is not None and m.bias.grad is not None for m in _bns(net))   # affine=False: the pair is still trained


def test_freeze_affine_and_unfreeze():
    from soccerdiffusion_amd.ml.model.encoder.image import freeze_batchnorm, unfreeze_batchnorm

    net = _small_resnet().train()
    net.bn1.bias.requires_grad_(False)   # a flag from before the freeze comes back as it was
    freeze_batchnorm(net.layer1)          # only a part of the backbone
    assert all(not m.training for m in _bns(net.layer1)) and net.bn1.training and all(m.training for m in _bns(net.layer2))
    net.train()
    assert all(not m.training for m in _bns(net.layer1)) and all(m.training for m in _bns(net.layer2))
    freeze_batchnorm(net, affine=True)
    assert all(not m.weight.requires_grad and not m.bias.requires_grad and not m.training for m in _bns(net))
    assert all(p.requires_grad for n, p in net.named_parameters() if "bn" not in n and "downsample.1" not in n)
    unfreeze_batchnorm(net)
    assert all(m.training for m in _bns(net))
    assert all(m.weight.requires_grad for m in _bns(net))
    assert not net.bn1.bias.requires_grad and all(m.bias.requires_grad for m in _bns(net) if m is not net.bn1)
    net.eval()
    net.train()
    assert all(m.training for m in _bns(net))
    net.eval()
    freeze_batchnorm(net)
    unfreeze_batchnorm(net)
    assert all(not m.training for m in _bns(net))   # unfrozen layers take their parent's mode


def _params(**kw):
    p = {"use_images": True, "image_encoder_type": "resnet18"}
    p.update(kw)
    return p


def test_freeze_bn_flag_parsing_and_refusals():
    from soccerdiffusion_amd import cli

    parser = cli.build_parser()
    assert parser.parse_args(["train", "-c", "x.yaml"]).freeze_bn is None
    assert parser.parse_args(["train", "-c", "x.yaml", "--freeze-bn", "stats"]).freeze_bn == "stats"
    args = parser.parse_args(["train", "-c", "x.yaml", "--freeze-bn", "all", "--pretrained-backbone", "r18.pt"])
    assert args.freeze_bn == "all" and args.pretrained_backbone == "r18.pt"
    assert parser.parse_args(["distill", "x.yaml", "teacher.pth", "--freeze-bn", "all"]).freeze_bn == "all"
    with pytest.raises(SystemExit):
        parser.parse_args(["train", "-c", "x.yaml", "--freeze-bn", "running"])
    assert cli.validate_freeze_bn(None, _params(use_images=False)) is None
    assert cli.validate_freeze_bn("stats", _params()) == "stats"
    assert cli.validate_freeze_bn("all", _params(image_encoder_type="resnet50")) == "all"
    with pytest.raises(SystemExit, match="no image encoder"):
        cli.validate_freeze_bn("stats", _params(use_images=False))
    for swin in ("swin_transformer_tiny", "swin_transformer_small"):
        with pytest.raises(SystemExit, match="no BatchNorm"):
            cli.validate_freeze_bn("all", _params(image_encoder_type=swin))
    with pytest.raises(SystemExit):
        cli.validate_freeze_bn("some", _params())


def test_checkpoint_key_round_trip(tmp_path):
    from soccerdiffusion_amd import cli

    assert cli._freeze_bn_checkpoint_keys(None) == {}
    path = tmp_path / "ckpt.pth"
    torch.save({"hyperparams": _params(), **cli._freeze_bn_checkpoint_keys("all")}, path)
    ckpt = torch.load(path, map_location="cpu", weights_only=True)
    assert ckpt["freeze_bn"] == "all"
    assert cli.validate_freeze_bn(ckpt.get("freeze_bn"), ckpt["hyperparams"]) == "all"   # what a resumed run does


def test_apply_freeze_bn_and_pretrained_backbone(tmp_path):
    from soccerdiffusion_amd import cli
    from soccerdiffusion_amd.ml.model.encoder.image import ImageEncoderType, ResNetImageEncoder

    class Model(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.image_sequence_encoder = ResNetImageEncoder(ImageEncoderType.RESNET18, 16, True, 64)

    torch.manual_seed(1)
    donor = Model().image_sequence_encoder.encoder
    with torch.no_grad():
        for m in _bns(donor):
            m.running_mean.normal_()
            m.running_var.uniform_(0.5, 2.0)
    state = dict(donor.state_dict())
    state["fc.weight"], state["fc.bias"] = torch.randn(1000, 512), torch.randn(1000)   # torchvision's classifier: another shape, and skipped by name
    state["layer9.0.conv1.weight"] = torch.zeros(3)                                    # a name the backbone does not have
    state["layer1.0.conv1.weight"] = torch.zeros(8, 8, 3, 3)                           # another shape: left as initialised
    path = tmp_path / "r18.pt"
    torch.save(state, path)
    torch.manual_seed(2)
    model = Model()
    backbone = model.image_sequence_encoder.encoder
    fc_before, conv_before = backbone.fc.weight.clone(), backbone.layer1[0].conv1.weight.clone()
    loaded, skipped = cli.load_pretrained_backbone(model, str(path))
    assert set(skipped) == {"fc.weight", "fc.bias", "layer9.0.conv1.weight", "layer1.0.conv1.weight"}
    assert len(loaded) == len(donor.state_dict()) - 3
    assert torch.equal(backbone.fc.weight, fc_before) and torch.equal(backbone.layer1[0].conv1.weight, conv_before)
    for k, v in donor.state_dict().items():
        if k in loaded:
            assert torch.equal(backbone.state_dict()[k], v), k
    fc_like = torch.nn.Linear(512, 16).state_dict()   # even a classifier of the encoder's own shape is not loaded
    torch.save({"fc.weight": fc_like["weight"], "fc.bias": fc_like["bias"]}, path)
    assert cli.load_pretrained_backbone(model, str(path)) == ([], ["fc.weight", "fc.bias"])
    assert torch.equal(backbone.fc.weight, fc_before)
    cli.apply_freeze_bn(model, "all")
    model.train()
    assert all(not m.training and not m.weight.requires_grad for m in _bns(model))
    assert backbone.conv1.weight.requires_grad and backbone.fc.weight.requires_grad
    cli.apply_freeze_bn(model, None)


@pytest.mark.parametrize("relu,with_res", [(True, True), (True, False), (False, False)])
def test_reference_equals_torch_batch_norm_eval_under_autograd(relu, with_res):
    g = torch.Generator().manual_seed(5)
    N, H, W, C = 2, 5, 7, 8
    y = torch.randn(N, H, W, C, generator=g, dtype=torch.float64) * 2 + 1
    gamma = torch.randn(C, generator=g, dtype=torch.float64)
    gamma[0], gamma[1] = 0.0, -0.7
    beta, rm = torch.randn(C, generator=g, dtype=torch.float64), torch.randn(C, generator=g, dtype=torch.float64)
    rv = torch.rand(C, generator=g, dtype=torch.float64) + 0.3
    res = torch.randn(N, H, W, C, generator=g, dtype=torch.float64) if with_res else None
    dz = torch.randn(N, H, W, C, generator=g, dtype=torch.float64)
    yd, gd, bd = y.clone().requires_grad_(), gamma.clone().requires_grad_(), beta.clone().requires_grad_()
    rd = res.clone().requires_grad_() if with_res else None
    rm0, rv0 = rm.clone(), rv.clone()
    out = F.batch_norm(yd.permute(0, 3, 1, 2), rm, rv, gd, bd, training=False, eps=1e-5).permute(0, 2, 3, 1)
    if with_res:
        out = out + rd
    if relu:
        out = out.relu()
    out.backward(dz)
    assert torch.equal(rm, rm0) and torch.equal(rv, rv0)
    z = ref.forward(y, gamma, beta, rm, rv, 1e-5, res, relu)
    dy, dres, dgamma, dbeta = ref.backward(dz, z, y, gamma, rm, rv, 1e-5, relu)
    for got, want in ((z, out), (dy, yd.grad), (dgamma, gd.grad), (dbeta, bd.grad)) + (((dres, rd.grad),) if with_res else ()):
        assert torch.allclose(got, want, rtol=1e-12, atol=1e-12)


def test_reference_stem_and_unit_equal_torch_under_autograd():
    g = torch.Generator().manual_seed(6)
    N, H, W, C = 2, 7, 9, 8
    y = torch.randn(N, H, W, C, generator=g, dtype=torch.float64)
    gamma, beta = torch.randn(C, generator=g, dtype=torch.float64), torch.randn(C, generator=g, dtype=torch.float64)
    rm, rv = torch.randn(C, generator=g, dtype=torch.float64), torch.rand(C, generator=g, dtype=torch.float64) + 0.3
    yd, gd, bd = y.clone().requires_grad_(), gamma.clone().requires_grad_(), beta.clone().requires_grad_()
    out = F.max_pool2d(F.batch_norm(yd.permute(0, 3, 1, 2), rm, rv, gd, bd, training=False, eps=1e-5).relu(), 3, 2, 1).permute(0, 2, 3, 1)
    dp = torch.randn(out.shape, generator=g, dtype=torch.float64)
    out.backward(dp)
    p, _ = ref.pool_forward(y, gamma, beta, rm, rv, 1e-5)
    dy, dgamma, dbeta = ref.pool_backward(dp, y, gamma, beta, rm, rv, 1e-5)
    for got, want in ((p, out), (dy, yd.grad), (dgamma, gd.grad), (dbeta, bd.grad)):
        assert torch.allclose(got, want, rtol=1e-12, atol=1e-12)
    # the conv unit: the same composition torch.nn runs for conv -> bn.eval() -> + res -> relu
    h = torch.randn(N, H, W, 4, generator=g, dtype=torch.float64)
    w = torch.randn(C, 4, 3, 3, generator=g, dtype=torch.float64)
    z = ref.unit(h, w, gamma, beta, rm, rv, 1e-5, 2, None, True)
    want = F.batch_norm(F.conv2d(h.permute(0, 3, 1, 2), w, stride=2, padding=1), rm, rv, gamma, beta, training=False, eps=1e-5).relu()
    assert torch.allclose(z.permute(0, 3, 1, 2), want, rtol=1e-12, atol=1e-12)
