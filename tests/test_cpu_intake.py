"""The host side of the session's raw-sensor intake, without a GPU: ``ops.linear_taps`` against an independent numpy restatement of
cv2.resize's INTER_LINEAR tables (tests/intake_ref.py), that restatement against exact bilinear interpolation, the route choice and the
argument checks of ``ops.camera_intake``."""

import numpy as np
import pytest
import torch

import intake_ref as ref

TABLE_CASES = ((640, 224), (480, 224), (23, 9), (11, 16), (10, 7), (2, 5), (7, 7), (1, 3))
IMAGE_CASES = ((480, 640, 224), (17, 23, 9), (9, 11, 16), (1536, 2048, 224), (33, 47, 32), (10, 10, 7))


@pytest.mark.parametrize("src,dst", TABLE_CASES)
def test_linear_taps_equal_the_restated_tables(src, dst):
    from soccerdiffusion_amd import ops

    index, coef = ops.linear_taps(src, dst)
    want_index, want_coef = ref.linear_table(src, dst)
    assert index.dtype == np.int32 and index.shape == (dst,) and coef.dtype == np.int16 and coef.shape == (dst, 2)
    assert np.array_equal(index, want_index) and np.array_equal(coef, want_coef)
    assert (coef.astype(np.int32).sum(axis=1) == 2048).all()
    assert index.min() >= 0 and index.max() <= src - 1
    assert (coef[index == src - 1] == (2048, 0)).all()


def test_linear_taps_reject_empty_axes():
    from soccerdiffusion_amd import ops

    for src, dst in ((0, 4), (4, 0), (True, 4), (4.0, 4)):
        with pytest.raises(ValueError):
            ops.linear_taps(src, dst)


@pytest.mark.parametrize("H,W,R", IMAGE_CASES)
def test_restatement_stays_within_one_grey_level_of_exact_bilinear(H, W, R):
    """11-bit coefficients, h >> 4, two >> 16 and the final (+ 2) >> 2 lose less than one grey level against the float64 bilinear value at
    the same taps - a property of OpenCV's scheme, so a condition on the restatement and not a tolerance (measured: 0.67 - 0.80)."""
    frame = ref.banded_frames(1, H, W, seed=H * 31 + W)[0]
    got = ref.resize_linear(frame, R).astype(np.float64)
    err = np.abs(got - ref.bilinear_exact(frame, R)).max()
    print(f"{H} x {W} -> {R}: max |fixed point - exact bilinear| = {err:.3f} grey levels")
    assert got.shape == (R, R, 3) and err <= 1.0


def test_camera_route():
    from soccerdiffusion_amd import ops

    assert ops.camera_route(7, 7, 7) == "copy"
    assert ops.camera_route(14, 14, 7) == "area2"
    assert ops.camera_route(14, 15, 7) == "linear" and ops.camera_route(14, 14, 8) == "linear"
    # the restatement takes the same routes: identity tables at the same size, the block mean at factor 2
    frame = ref.banded_frames(1, 14, 14, seed=3)[0]
    assert np.array_equal(ref.resize_linear(frame[:7, :7], 7), frame[:7, :7])
    block = frame.astype(np.int32).reshape(7, 2, 7, 2, 3).sum(axis=(1, 3))
    assert np.array_equal(ref.resize_linear(frame, 7), (block + 2) >> 2)


def test_camera_intake_checks_its_arguments_before_it_needs_a_gpu(monkeypatch):
    from soccerdiffusion_amd import _lib, ops

    def no_library():
        raise AssertionError("the library was loaded before the arguments were checked")

    monkeypatch.setattr(_lib, "load", no_library)
    good = torch.zeros(2, 8, 9, 3, dtype=torch.uint8)
    for frames, R, order in ((good.float(), 4, "rgb"), (torch.zeros(2, 8, 9, 4, dtype=torch.uint8), 4, "rgb"), (good, 0, "rgb"),
                             (good, 4, "gbr"), (good, 4.0, "rgb"), (good, True, "rgb"), (good, 4097, "rgb"), (good, 4, "rgb")):
        with pytest.raises(ValueError):   # (the last one: every argument is right but the frames are not on the device)
            ops.camera_intake(frames, R, order=order)
