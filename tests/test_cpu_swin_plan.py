"""CPU checks of the Swin window plan: ops.swin_window_plan and the C host code of sd_swin_window_attention (sd_swin_window_plan) agree with
what _ShiftedWindowAttention.forward (ml/model/encoder/image.py, torchvision Swin V1) does - padded size, shift per dimension, window count - and
a NumPy restatement of the kernel's region-id rule (csrc/sd_swin.hip: token_region) gives exactly the -100 / 0 mask the module builds."""

import ctypes as C

import numpy as np
import pytest
import torch
from torch import nn

MAPS = [(56, 56), (24, 24), (6, 6), (7, 14), (14, 7), (30, 40)]


def _module_plan(H, W, window=7, shift=3, monkeypatch=None):
    """Runs the torch module on a (1, H, W, 32) map and records the padded shape, the roll shifts, the window count and the final mask."""
    from soccerdiffusion_amd.ml.model.encoder.image import _ShiftedWindowAttention

    m = _ShiftedWindowAttention(32, window, shift, 1)
    seen = {"roll": [], "pad": [], "fill": []}
    roll, pad, fill = torch.roll, nn.functional.pad, torch.Tensor.masked_fill
    monkeypatch.setattr(torch, "roll", lambda x, shifts, dims: (seen["roll"].append(tuple(shifts)), roll(x, shifts, dims))[1])
    monkeypatch.setattr(nn.functional, "pad", lambda x, p: (lambda y: (seen["pad"].append(tuple(y.shape)), y)[1])(pad(x, p)))
    monkeypatch.setattr(torch.Tensor, "masked_fill", lambda self, *a: (lambda y: (seen["fill"].append(y), y)[1])(fill(self, *a)))
    m.qkv.register_forward_pre_hook(lambda mod, args: seen.update(rows=args[0].shape[0]))   # (B nW, w^2, C), B = 1
    with torch.no_grad():
        m(torch.randn(1, H, W, 32))
    monkeypatch.undo()
    _, pH, pW, _ = seen["pad"][0]
    sh, sw = (-seen["roll"][0][0], -seen["roll"][0][1]) if seen["roll"] else (0, 0)
    mask = seen["fill"][-1].numpy() if seen["fill"] else None
    return (pH, pW, sh, sw), seen["rows"], mask


def _region_mask(pH, pW, sh, sw, window):
    """The kernel's rule: region id 3 ry + rx of each window token on the rolled, padded map (rows: [0, pH - w) -> 0, [pH - w, pH - sh) -> 1,
    [pH - sh, pH) -> 2, and all rows 2 when sh = 0 - torchvision's last slice [-0:] covers the map; columns alike), -100 between different ids."""
    def region(n, s, v):
        return np.where(np.full_like(v, s == 0, dtype=bool), 2, np.where(v < n - window, 0, np.where(v < n - s, 1, 2)))

    nWy, nWx = pH // window, pW // window
    t = np.arange(window * window)
    masks = []
    for wy in range(nWy):
        for wx in range(nWx):
            y, x = wy * window + t // window, wx * window + t % window
            rid = 3 * region(pH, sh, y) + region(pW, sw, x)
            masks.append(np.where(rid[:, None] != rid[None, :], -100.0, 0.0))
    return np.stack(masks)


@pytest.mark.parametrize("H,W", MAPS)
def test_window_plan_matches_module(H, W, monkeypatch):
    from soccerdiffusion_amd import ops

    (pH, pW, sh, sw), rows, _ = _module_plan(H, W, monkeypatch=monkeypatch)
    plan = ops.swin_window_plan(H, W, 7, 3)
    assert plan[:4] == (pH, pW, sh, sw)
    assert plan[4] * plan[5] == rows and plan[4] == pH // 7 and plan[5] == pW // 7
    # the unshifted block of the same stage: no roll at all
    (pH0, pW0, sh0, sw0), _, mask0 = _module_plan(H, W, shift=0, monkeypatch=monkeypatch)
    assert ops.swin_window_plan(H, W, 7, 0)[:4] == (pH0, pW0, sh0, sw0) == (pH, pW, 0, 0) and mask0 is None


@pytest.mark.parametrize("H,W", MAPS)
def test_c_window_plan_matches_python(H, W):
    from soccerdiffusion_amd import _lib, build, ops

    build.build()
    out = (C.c_int * 6)()
    assert _lib.load().sd_swin_window_plan(H, W, 7, 3, out) == 0
    assert tuple(out) == ops.swin_window_plan(H, W, 7, 3)


@pytest.mark.parametrize("H,W", MAPS)
def test_region_mask_rule_matches_module_mask(H, W, monkeypatch):
    (pH, pW, sh, sw), _, mask = _module_plan(H, W, monkeypatch=monkeypatch)
    if sh == 0 and sw == 0:   # 6 x 6: one window covers the map, no mask
        assert mask is None
        return
    want = _region_mask(pH, pW, sh, sw, 7)
    assert mask.shape == want.shape
    np.testing.assert_array_equal(mask, want)
    assert (want != 0).any()


def test_window_plan_rejects_bad_arguments():
    from soccerdiffusion_amd import ops

    for args in ((0, 5, 7, 3), (5, 5, 0, 0), (5, 5, 7, -1)):
        with pytest.raises(ValueError):
            ops.swin_window_plan(*args)
