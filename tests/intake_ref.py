"""A numpy restatement of what the robot node does to a camera frame (soccer_diffusion/ml/inference/ros.py:186-200): cv2.resize(img, (R, R))
with the default INTER_LINEAR on 8-bit images (OpenCV's imgproc/src/resize.cpp, restated from the published source - cv2 is not a
dependency), ToDtype(float32, scale=True) and Normalize(ImageNet).  Whole-array numpy, written on its own: the tests hold
``ops.linear_taps`` and ``sd_camera_intake`` against it, so it shares no code with either."""

import numpy as np

MEAN = np.array([0.485, 0.456, 0.406], dtype=np.float32)
STD = np.array([0.229, 0.224, 0.225], dtype=np.float32)
COEF_BITS = 11   # INTER_RESIZE_COEF_BITS


def axis_positions(src, dst):
    """(first tap, fraction) of every output index of one axis in float64, before any rounding to fp32: the exact bilinear geometry with
    OpenCV's border rule (a position left of pixel 0 or at / right of the last pixel reads that pixel alone)."""
    scale = 1.0 / (dst / float(src))
    pos = (np.arange(dst, dtype=np.float64) + 0.5) * scale - 0.5
    first = np.floor(pos)
    frac = pos - first
    first = first.astype(np.int64)
    outside = (first < 0) | (first >= src - 1)
    frac[outside] = 0.0
    return np.clip(first, 0, src - 1), frac


def linear_table(src, dst):
    """resizeGeneric's table of one axis for INTER_LINEAR on uchar: first tap (dst,) int32, coefficient pairs (dst, 2) int16."""
    scale = 1.0 / (dst / float(src))
    pos = ((np.arange(dst, dtype=np.float64) + 0.5) * scale - 0.5).astype(np.float32)   # fx = (float)((dx + 0.5) * scale_x - 0.5)
    first = np.floor(pos)
    frac = (pos - first).astype(np.float32)                                              # fx -= sx, in fp32
    first = first.astype(np.int64)
    frac[first < 0] = 0
    first[first < 0] = 0
    frac[first >= src - 1] = 0
    first[first >= src - 1] = src - 1
    unit = np.float32(1 << COEF_BITS)
    pair = np.stack([(np.float32(1) - frac) * unit, frac * unit], axis=1)
    assert pair.dtype == np.float32
    return first.astype(np.int32), np.rint(pair).astype(np.int16)                        # cvRound: half to even


def resize_linear(img, R):
    """cv2.resize(img, (R, R)) of one (H, W, 3) uint8 image."""
    H, W, _ = img.shape
    src = img.astype(np.int32)
    if (H, W) == (R, R):
        return img.copy()
    if (H, W) == (2 * R, 2 * R):   # INTER_LINEAR at an exact factor 2 on both axes runs INTER_AREA's resizeAreaFast
        return ((src[0::2, 0::2] + src[0::2, 1::2] + src[1::2, 0::2] + src[1::2, 1::2] + 2) >> 2).astype(np.uint8)
    xs, xc = linear_table(W, R)
    ys, yc = linear_table(H, R)
    xc, yc = xc.astype(np.int32), yc.astype(np.int32)
    x2, y2 = np.minimum(xs + 1, W - 1), np.minimum(ys + 1, H - 1)
    rows = src[:, xs] * xc[None, :, 0, None] + src[:, x2] * xc[None, :, 1, None]         # HResizeLinear: (H, R, 3) int32
    top, bottom = rows[ys] >> 4, rows[y2] >> 4                                            # VResizeLinear
    v = (((yc[:, 0, None, None] * top) >> 16) + ((yc[:, 1, None, None] * bottom) >> 16) + 2) >> 2
    return np.clip(v, 0, 255).astype(np.uint8)


def bilinear_exact(img, R):
    """The float64 bilinear value at the same taps: what the fixed-point passes approximate."""
    H, W, _ = img.shape
    xs, fx = axis_positions(W, R)
    ys, fy = axis_positions(H, R)
    x2, y2 = np.minimum(xs + 1, W - 1), np.minimum(ys + 1, H - 1)
    s = img.astype(np.float64)
    rows = s[:, xs] * (1 - fx)[None, :, None] + s[:, x2] * fx[None, :, None]
    return rows[ys] * (1 - fy)[:, None, None] + rows[y2] * fy[:, None, None]


def preprocess(frames, R, bgr=False):
    """frames (..., H, W, 3) uint8 -> (..., 3, R, R) float32 as the node feeds the model: resize, / 255, (x - mean) / std, fp32 throughout."""
    lead = frames.shape[:-3]
    flat = frames.reshape(-1, *frames.shape[-3:])
    v = np.stack([resize_linear(f, R) for f in flat])
    if bgr:
        v = v[..., ::-1]
    x = v.astype(np.float32) / np.float32(255.0)
    x = (x - MEAN) / STD
    assert x.dtype == np.float32
    return np.ascontiguousarray(x.transpose(0, 3, 1, 2)).reshape(*lead, 3, R, R)


def banded_frames(n, H, W, seed):
    """Random uint8 frames with a saturated 0 band and a saturated 255 band (rows and columns): the fixed-point passes at their limits."""
    g = np.random.default_rng(seed)
    f = g.integers(0, 256, size=(n, H, W, 3), dtype=np.uint8)
    f[:, : max(1, H // 5)] = 255
    f[:, H - max(1, H // 6):, : max(1, W // 2)] = 0
    f[:, :, W - max(1, W // 7):] = 255
    f[:, H // 2, :, 1] = 0
    return f
