"""CPU-only checks of the per-robot forms of the policy session (soccerdiffusion_amd/session.py, csrc/sd_session.hip): the host-side
validation of a robot subset - the only validation there is: the kernels check nothing but the range - and the argument errors of the
``*_at`` entry points and of ``sd_session_reset`` without a device."""

import ctypes as C

import numpy as np
import pytest
import torch


@pytest.fixture(scope="module")
def lib():
    from soccerdiffusion_amd import build

    build.build()
    from soccerdiffusion_amd import _lib

    return _lib


def test_robot_index_accepts_permutations_and_subsets():
    from soccerdiffusion_amd import ops

    for robots, B, want in (([2, 0, 1], 3, [2, 0, 1]), ([3, 0], 5, [3, 0]), ([], 4, []), ((1,), 2, [1]), (range(3), 3, [0, 1, 2]),
                            (torch.tensor([4, 1]), 5, [4, 1]), (torch.tensor([0], dtype=torch.int32), 1, [0]), ([np.int64(1), 0], 2, [1, 0])):
        idx = ops.robot_index(robots, B)
        assert idx.dtype == torch.int32 and idx.device.type == "cpu" and idx.dim() == 1 and idx.tolist() == want


def test_robot_index_rejects_what_the_kernels_cannot_check():
    from soccerdiffusion_amd import ops

    B = 4
    for bad in ([1, 1], [0, 2, 0], [-1], [B], [0, B], torch.tensor([[0, 1]]), torch.tensor(1), torch.tensor([1, 1]), torch.tensor([-1]),
                torch.tensor([B]), [0.0], torch.tensor([0.0]), torch.tensor([True, False, False, False]), [[0]], 1):
        with pytest.raises(ValueError, match="robots"):
            ops.robot_index(bad, B)


def test_subset_entry_points_reject_bad_arguments_without_gpu(lib):
    h = lib.load()
    assert h.sd_ring_push_at(None, None, None, None, None, 1, 1, 10, 4, 1, None) == -1
    assert b"sd_ring_push_at" in h.sd_last_error()
    assert h.sd_ring_window_at(None, None, None, None, 1, 1, 10, 4, None) == -1
    assert b"sd_ring_window_at" in h.sd_last_error()
    assert h.sd_session_windows_at(None, 1, None, 1, 1, None) == -1
    assert b"sd_session_windows_at" in h.sd_last_error()
    assert h.sd_session_commit_at(None, None, None, None, None, None, None, 1, 1, 10, 20, 100, None) == -1
    assert b"sd_session_commit_at" in h.sd_last_error()
    assert h.sd_session_reset(None, 1, None, None, 2, 1, None) == -1
    assert b"sd_session_reset" in h.sd_last_error()
    # a host buffer stands in for the pointers: every call below fails its checks, or has nothing to do, before any launch
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    views = (lib.RingView * 2)()
    views[0].L = views[1].L = 10
    views[0].C = views[1].C = 4
    assert h.sd_session_windows_at(views, 2, p, 1, 1, None) == -1          # views of null pointers
    views[0].ring = views[0].head = views[0].out = views[1].ring = views[1].head = views[1].out = p
    assert h.sd_session_windows_at(views, 4, p, 1, 1, None) == -1          # more than SD_SESSION_MAX_RINGS
    assert h.sd_session_windows_at(views, 2, None, 1, 1, None) == -1       # robots missing
    assert h.sd_session_windows_at(views, 2, p, -1, 1, None) == -1
    assert h.sd_session_windows_at(views, 2, p, 1, 0, None) == -1
    assert h.sd_session_windows_at(views, 2, None, 0, 1, None) == 0        # S == 0: nothing to do
    assert h.sd_ring_push_at(p, p, p, None, None, 1, 1, 4, 4, 1, None) == -1   # robots missing
    assert h.sd_ring_push_at(p, p, None, None, p, 1, 1, 4, 4, 1, None) == -1   # src missing
    assert h.sd_ring_push_at(p, p, p, None, p, 1, 1, 0, 4, 1, None) == -1
    assert h.sd_ring_push_at(p, p, p, None, p, 1, 0, 4, 4, 1, None) == -1
    assert h.sd_ring_push_at(p, p, p, None, p, 1, 1, 4, 4, -1, None) == -1
    assert h.sd_ring_push_at(p, p, p, None, p, -1, 1, 4, 4, 1, None) == -1
    assert h.sd_ring_push_at(p, p, p, None, p, 0, 1, 4, 4, 1, None) == 0       # S == 0
    assert h.sd_ring_push_at(p, p, p, None, p, 1, 1, 4, 4, 0, None) == 0       # n == 0
    assert h.sd_ring_window_at(p, p, p, None, 1, 1, 4, 4, None) == -1
    assert h.sd_ring_window_at(p, p, p, p, 1, 0, 4, 4, None) == -1
    assert h.sd_ring_window_at(p, p, p, p, 1, 1, 4, 0, None) == -1
    assert h.sd_ring_window_at(p, p, p, p, 0, 1, 4, 4, None) == 0
    assert h.sd_session_commit_at(p, p, p, p, p, p, None, 1, 1, 4, 4, 4, None) == -1
    assert h.sd_session_commit_at(p, p, p, p, p, p, p, 1, 1, 0, 4, 4, None) == -1
    assert h.sd_session_commit_at(p, p, p, p, p, p, p, 1, 1, 4, 4, 0, None) == -1
    assert h.sd_session_commit_at(p, p, p, p, p, p, p, -1, 1, 4, 4, 4, None) == -1
    assert h.sd_session_commit_at(p, p, p, p, p, p, p, 0, 1, 4, 4, 4, None) == 0
    rings = (lib.RingReset * 6)()
    for r in rings:
        r.L, r.C = 10, 4
    assert h.sd_session_reset(rings, 1, None, None, 2, 1, None) == -1      # a ring of null pointers
    for r in rings:
        r.ring = r.head = p
    assert h.sd_session_reset(rings, 0, None, None, 2, 1, None) == -1
    assert h.sd_session_reset(rings, 6, None, None, 2, 1, None) == -1      # more than SD_SESSION_MAX_RESET_RINGS
    assert h.sd_session_reset(rings, 1, None, None, 2, 0, None) == -1
    rings[0].L = 0
    assert h.sd_session_reset(rings, 1, None, None, 2, 1, None) == -1
    assert C.sizeof(lib.RingReset) == 3 * 8 + 2 * 4
