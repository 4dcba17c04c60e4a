#!/usr/bin/env python3
"""The workload of tools/profile_swin.sh: two Swin-T encoder forwards of 160 frames at 224 x 224 on the HIP route (the first packs the
weights).  The frames are drawn on the host and copied, so that no ATen kernel runs on the device."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from soccerdiffusion_amd.ml.model.encoder.image import ImageEncoderType, image_encoder_factory  # noqa: E402

torch.manual_seed(0)
enc = image_encoder_factory(ImageEncoderType.SWIN_TRANSFORMER_TINY, 256, True, 224).encoder.cuda().eval()
x = (torch.rand(160, 3, 224, 224) * 2.0 - 0.7).cuda()
with torch.no_grad():
    for _ in range(2):
        y = enc(x)
torch.cuda.synchronize()
print("tokens", tuple(y.shape), float(y.cpu().abs().max()))   # (on the host: no device kernel outside the forward)
