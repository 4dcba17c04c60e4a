"""The ResNet encoder heads on csrc/sd_head.hip (ops.resnet_head / conv_training.ResNetHead): the avgpool head (mean over the map, fc) and the
no-avgpool head (Conv2d(C, 32, 1) + bias flattened in NCHW order, fc; reference ml/model/encoder/image.py:61-83), forward and every backward
output against fp64, the module routes (no torch head op left in an eval forward or a train forward + backward), SD_CONV=torch parity,
an optimizer step seen by the next forward, and default.yaml's encode_input_data against the CPU fp64 modules + the oracle."""

import copy
import os

import pytest
import torch

from conftest import rel_err

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
FORBIDDEN = ("aten::conv2d", "aten::addmm", "aten::mm", "aten::linear", "aten::mean", "aten::adaptive_avg_pool2d", "aten::convolution_backward")


def _head64(x, cw, cb, fw, fb):
    """fp64 reference on the NHWC map x (N, H, W, C)."""
    N, H, W, C = x.shape
    if cw is None:
        feat = x.mean(dim=(1, 2))
    else:
        z = torch.einsum("nhwc,oc->nohw", x, cw.reshape(32, C)) + cb[None, :, None, None]
        feat = z.reshape(N, -1)
    return feat @ fw.T + fb


@pytest.mark.parametrize("conv", [False, True], ids=["avgpool", "conv1x1"])
@pytest.mark.parametrize("C", [512, 2048])
@pytest.mark.parametrize("hw", [(7, 7), (15, 20), (1, 1)])
@pytest.mark.parametrize("d", [128, 512])
def test_head_forward_and_backward_against_fp64(conv, C, hw, d):
    from soccerdiffusion_amd import conv_training as ct

    g = torch.Generator().manual_seed(C + d + hw[0])
    N, (H, W) = 5, hw
    J = 32 * H * W if conv else C
    x = torch.relu(torch.randn(N, H, W, C, generator=g, dtype=torch.float64))
    cw = torch.randn(32, C, 1, 1, generator=g, dtype=torch.float64) / C ** 0.5 if conv else None
    cb = torch.randn(32, generator=g, dtype=torch.float64) if conv else None
    fw = torch.randn(d, J, generator=g, dtype=torch.float64) / J ** 0.5
    fb = torch.randn(d, generator=g, dtype=torch.float64)
    dy = torch.randn(N, d, generator=g, dtype=torch.float64)
    leaves64 = [t.clone().requires_grad_() if t is not None else None for t in (x, cw, cb, fw, fb)]
    _head64(*leaves64).backward(dy)
    want_y = _head64(x, cw, cb, fw, fb)

    leaves = [t.float().to(DEV).requires_grad_() if t is not None else None for t in (x, cw, cb, fw, fb)]
    pre = [torch.randn(t.shape, generator=g).to(DEV) if t is not None else None for t in leaves[1:]]
    for p, q in zip(leaves[1:], pre):      # existing .grad buffers (an optimizer's): the kernels add into them
        if p is not None:
            p.grad = q.clone()
    y = ct.ResNetHead.apply(*leaves)
    assert y.shape == (N, d) and rel_err(y, want_y) < 1e-5
    y.backward(dy.float().to(DEV))
    assert rel_err(leaves[0].grad, leaves64[0].grad) < 1e-5
    for p, q, w in zip(leaves[1:], pre, leaves64[1:]):
        if p is not None:
            assert rel_err(p.grad - q, w.grad) < 1e-5, tuple(p.shape)
    # deterministic: the same bytes again
    x2 = leaves[0].detach().clone().requires_grad_()
    ps = [p.detach().clone().requires_grad_() if p is not None else None for p in leaves[1:]]
    ps2 = [p.detach().clone().requires_grad_() if p is not None else None for p in leaves[1:]]
    x3 = leaves[0].detach().clone().requires_grad_()
    ct.ResNetHead.apply(x2, *ps).backward(dy.float().to(DEV))
    ct.ResNetHead.apply(x3, *ps2).backward(dy.float().to(DEV))
    assert torch.equal(x2.grad, x3.grad) and all(torch.equal(a.grad, b.grad) for a, b in zip(ps, ps2) if a is not None)


def _encoder(avgpool: bool, R: int):
    from soccerdiffusion_amd.ml.model.encoder.image import ImageEncoderType, ResNetImageEncoder

    torch.manual_seed(3)
    return ResNetImageEncoder(ImageEncoderType.RESNET18, 128, avgpool, R).to(DEV)


CASES = [(False, (224, 224)), (True, (96, 128))]


def _names(prof):
    return {e.name for e in prof.events()}


@pytest.mark.parametrize("avgpool,size", CASES, ids=["conv1x1_224", "avgpool_96x128"])
def test_module_routes_use_no_torch_head_op(avgpool, size):
    enc = _encoder(avgpool, size[0])
    frames = torch.rand(2, 3, 3, *size, generator=torch.Generator().manual_seed(1)).to(DEV)
    enc.eval()
    with torch.no_grad(), torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CPU]) as prof:
        y = enc(frames)
    assert y.shape == (2, 3, 128) and not (_names(prof) & set(FORBIDDEN)), _names(prof) & set(FORBIDDEN)
    enc.train()
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CPU]) as prof:
        y = enc(frames)
        (y * torch.linspace(-1, 1, 128, device=DEV)).sum().backward()
    assert not (_names(prof) & set(FORBIDDEN)), _names(prof) & set(FORBIDDEN)
    assert enc.encoder.fc.weight.grad is not None and enc.encoder.layer4[1].conv2.weight.grad.abs().sum() > 0
    if not avgpool:
        assert enc.encoder.avgpool.weight.grad.abs().sum() > 0 and enc.encoder.fc.in_features == 1568


@pytest.mark.parametrize("avgpool,size", CASES, ids=["conv1x1_224", "avgpool_96x128"])
def test_hip_head_agrees_with_torch_and_sees_an_optimizer_step(avgpool, size):
    from soccerdiffusion_amd import training

    enc = _encoder(avgpool, size[0])
    frames = torch.rand(2, 3, 3, *size, generator=torch.Generator().manual_seed(2)).to(DEV)

    def eval_pair():
        enc.eval()
        with torch.no_grad():
            hip = enc(frames)
            os.environ["SD_CONV"] = "torch"
            try:
                ref = enc(frames)
            finally:
                del os.environ["SD_CONV"]
        return hip, ref

    hip0, ref0 = eval_pair()
    assert rel_err(hip0, ref0) < 1e-5
    # one training step through FusedAdamW's flat buffers; the next eval forward sees the new weights on both routes
    opt = training.FusedAdamW(enc.parameters(), lr=1e-2)
    enc.train()
    opt.zero_grad()
    enc(frames).square().mean().backward()
    opt.step()
    hip1, ref1 = eval_pair()
    assert rel_err(hip1, ref1) < 1e-5 and rel_err(hip1, hip0) > 1e-3


def test_default_yaml_encode_input_data_against_cpu_fp64_and_oracle():
    from oracle import denoiser_ref as ref
    from test_gpu_frames_area import DEFAULT_YAML

    from soccerdiffusion_amd import cli

    params = dict(DEFAULT_YAML)
    torch.manual_seed(7)
    model = cli.build_model(params).to(DEV).eval()
    data = cli.synthetic_dataset(2, params, seed=4)
    inp = {k: v.to(DEV) for k, v in data.items() if k in ("joint_command_history", "rotation", "joint_state", "image_data", "game_state")}
    with torch.no_grad():
        ctx = model.encode_input_data(inp)
    assert len(ctx) == 5 and ctx[3].shape == (2, 10, 128)      # [action history, IMU, joint state, images, game state]
    assert model.image_sequence_encoder.image_encoder.encoder.fc.in_features == 1568
    backbone = copy.deepcopy(model.image_sequence_encoder.image_encoder).cpu().double().eval()
    with torch.no_grad():
        tokens = backbone(data["image_data"].double())
    sd = {k[len("image_sequence_encoder.transformer_encoder."):]: v.detach().cpu().double() for k, v in model.state_dict().items()
          if k.startswith("image_sequence_encoder.transformer_encoder.")}
    want = ref.encoder_forward(sd, tokens, "", dtype=torch.float64, heads=8)
    assert rel_err(ctx[3], want) < 1e-4
