"""CPU-only checks of the sampler's held elements and of the session's held joints (sd_ddim_sample_hold, sd_session_hold,
sd_session_hold_mask): ops.hold_mask's packing on host tensors, the CPU reference tests/hold_ref.py against tests/pin_ref.py, the new entry
points in the header, in _lib.SIGNATURES and in the built library, their argument errors without a device, and the Python-side validation
that needs none."""

import ctypes as C
import os
import re

import pytest
import torch

import hold_ref
import pin_ref
from conftest import REPO
from test_cpu_pin import _toy_denoiser

NEW = ("sd_ddim_sample_hold", "sd_session_hold", "sd_session_hold_mask")


@pytest.fixture(scope="module")
def lib():
    from soccerdiffusion_amd import build

    build.build()
    from soccerdiffusion_amd import _lib

    return _lib


def _bits(words):
    """The 32 bits of every int32 word as unsigned Python integers."""
    return [[int(w) & 0xffffffff for w in row] for row in words.tolist()]


def test_hold_mask_packs_bit_j_for_joint_j():
    from soccerdiffusion_amd import ops

    B, T, J = 3, 5, 22
    g = torch.Generator().manual_seed(1)
    mask = torch.rand(B, T, J, generator=g) < 0.4
    words = ops.hold_mask(mask, B, T, J, "cpu")
    assert words.dtype == torch.int32 and tuple(words.shape) == (B, T) and words.is_contiguous()
    assert torch.equal(words, hold_ref.pack(mask))
    for b in range(B):
        for t in range(T):
            for j in range(J):
                assert (_bits(words)[b][t] >> j) & 1 == int(mask[b, t, j])
    assert all(w >> J == 0 for row in _bits(words) for w in row)                      # no bit at or above J
    # the broadcast forms
    tj = torch.rand(T, J, generator=g) < 0.5
    assert torch.equal(ops.hold_mask(tj, B, T, J, "cpu"), hold_ref.pack(tj.expand(B, T, J)))
    joints = torch.zeros(J, dtype=torch.bool)
    joints[[0, 1, 21]] = True
    assert _bits(ops.hold_mask(joints, B, T, J, "cpu")) == [[(1 << 0) | (1 << 1) | (1 << 21)] * T] * B
    # words are returned as they are
    assert torch.equal(ops.hold_mask(words, B, T, J, "cpu"), words)
    assert _bits(ops.hold_mask(torch.zeros(J, dtype=torch.bool), B, T, J, "cpu")) == [[0] * T] * B


def test_hold_mask_rows_or_in_the_leading_rows():
    from soccerdiffusion_amd import ops

    B, T, J = 3, 6, 20
    joints = torch.zeros(J, dtype=torch.bool)
    joints[[3, 4]] = True
    rows = [0, 2, 6]
    words = ops.hold_mask(joints, B, T, J, "cpu", rows=rows)
    want = joints.expand(B, T, J) | hold_ref.rows_mask(torch.tensor(rows), B, T, J)
    assert torch.equal(words, hold_ref.pack(want))
    assert _bits(words)[1] == [(1 << J) - 1] * 2 + [(1 << 3) | (1 << 4)] * 4
    # a mask of the leading rows alone is the pin's description; an int counts for every trajectory; words take rows too
    none = torch.zeros(J, dtype=torch.bool)
    assert torch.equal(ops.hold_mask(none, B, T, J, "cpu", rows=rows), hold_ref.pack(hold_ref.rows_mask(torch.tensor(rows), B, T, J)))
    assert _bits(ops.hold_mask(none, B, T, J, "cpu", rows=1)) == [[(1 << J) - 1] + [0] * (T - 1)] * B
    assert torch.equal(ops.hold_mask(hold_ref.pack(joints.expand(B, T, J)), B, T, J, "cpu", rows=rows), words)
    with pytest.raises(ValueError, match="pin rows"):
        ops.hold_mask(none, B, T, J, "cpu", rows=T + 1)


def test_hold_mask_bit_31_through_the_signed_word():
    from soccerdiffusion_amd import ops

    B, T, J = 2, 3, 32
    top = torch.zeros(J, dtype=torch.bool)
    top[31] = True
    words = ops.hold_mask(top, B, T, J, "cpu")
    assert words.dtype == torch.int32 and words.tolist() == [[-2 ** 31] * T] * B and _bits(words) == [[1 << 31] * T] * B
    everything = ops.hold_mask(torch.ones(J, dtype=torch.bool), B, T, J, "cpu")
    assert everything.tolist() == [[-1] * T] * B
    mixed = torch.zeros(B, T, J, dtype=torch.bool)
    mixed[0, 1, [0, 31]] = True
    mixed[1, 2, 30] = True
    assert _bits(ops.hold_mask(mixed, B, T, J, "cpu")) == [[0, (1 << 31) | 1, 0], [0, 0, 1 << 30]]
    assert _bits(ops.hold_mask(torch.zeros(J, dtype=torch.bool), B, T, J, "cpu", rows=[1, 0])) == [[0xffffffff, 0, 0], [0, 0, 0]]
    assert torch.equal(ops.hold_mask(mixed, B, T, J, "cpu"), hold_ref.pack(mixed))


def test_hold_mask_rejects_more_than_32_joints_and_bad_shapes():
    from soccerdiffusion_amd import ops

    B, T, J = 2, 3, 22
    with pytest.raises(ValueError, match="32"):
        ops.hold_mask(torch.zeros(33, dtype=torch.bool), B, T, 33, "cpu")
    with pytest.raises(ValueError, match="32"):
        ops.hold_mask(torch.zeros(B, T, 33, dtype=torch.bool), B, T, 33, "cpu")
    for bad in (torch.zeros(J + 1, dtype=torch.bool), torch.zeros(T, J + 1, dtype=torch.bool), torch.zeros(B + 1, T, J, dtype=torch.bool),
                torch.zeros(B, T, dtype=torch.bool), torch.zeros(B, T, J), torch.zeros(B, T, dtype=torch.int64),
                torch.zeros(B, T + 1, dtype=torch.int32), [True] * J, None):
        with pytest.raises(ValueError, match="hold mask"):
            ops.hold_mask(bad, B, T, J, "cpu")


def test_hold_ref_with_a_leading_rows_mask_is_pin_ref_bit_for_bit():
    B, T, J, n = 3, 10, 7, 4
    g = torch.Generator().manual_seed(3)
    x_T, known = torch.randn(B, T, J, generator=g), torch.randn(B, T, J, generator=g)
    den = _toy_denoiser(4, J)
    for rows in (torch.tensor([0, 3, 10]), torch.tensor([0, 0, 0]), torch.tensor([10, 1, 9])):
        want = pin_ref.sample(den, x_T, known, rows, n)
        got = hold_ref.sample(den, x_T, known, hold_ref.rows_mask(rows, B, T, J), n)
        for a, b in zip(want, got):
            assert len(a) == len(b) == n and all(torch.equal(u, v) for u, v in zip(a, b))


def test_hold_ref_holds_elements_and_the_free_ones_read_them():
    B, T, J, n = 2, 6, 7, 4
    g = torch.Generator().manual_seed(5)
    x_T, known = torch.randn(B, T, J, generator=g), torch.randn(B, T, J, generator=g)
    den = _toy_denoiser(6, J)
    mask = torch.zeros(B, T, J, dtype=torch.bool)
    mask[1, :, [2, 6]] = True
    mask[1, -1] = True
    got, held, _ = hold_ref.sample(den, x_T, known, mask, n)
    assert all(torch.equal(x[mask], p[mask]) for x, p in zip(got, held))
    assert torch.equal(got[-1][mask], known[mask])                                    # exactly
    free = hold_ref.sample(den, x_T, known, torch.zeros_like(mask), n)[0][-1]
    assert torch.equal(got[-1][0], free[0])                                           # the trajectory without held elements
    assert not torch.equal(got[-1][1][~mask[1]], free[1][~mask[1]])                   # the free elements of the other read the held ones


def _declared(header):
    return set(re.findall(r"^(?:int|size_t|const char \*)\s*(sd_\w+)\(", header, re.M))


def test_new_entry_points_are_declared_registered_and_exported(lib):
    with open(os.path.join(REPO, "include", "soccerdiffusion_hip.h")) as f:
        header = f.read()
    declared = _declared(header)
    h = lib.load()
    for name in NEW:
        assert name in declared, name
        assert name in lib.SIGNATURES, name
        assert getattr(h, name) is not None
    # sd_ddim_sample_hold = sd_ddim_sample_draws's arguments, the three hold arrays where its pin arrays are
    assert lib.SIGNATURES["sd_ddim_sample_hold"] == lib.SIGNATURES["sd_ddim_sample_draws"]


def test_new_entry_points_reject_bad_arguments_without_gpu(lib):
    h = lib.load()
    p = C.cast((C.c_float * 64)(), C.c_void_p)
    other = C.cast((C.c_float * 64)(), C.c_void_p)
    coef = (C.c_float * 16)()
    w = lib.DenoiserWeights()
    # all three arrays must be given, and the noise must not alias x: refused before the weights are even looked at
    for x0, noise, mask in ((None, other, p), (other, None, p), (other, other, None)):
        assert h.sd_ddim_sample_hold(C.byref(w), p, p, coef, p, None, None, p, 2, 10, 1, 4, None, 3, x0, noise, mask, 1, None) == -1
        assert b"sd_ddim_sample_hold" in h.sd_last_error()
    assert h.sd_ddim_sample_hold(C.byref(w), p, p, coef, p, None, None, p, 2, 10, 1, 4, None, 3, other, p, other, 1, None) == -1
    assert b"alias" in h.sd_last_error()
    for draws in (0, -1, 3):
        assert h.sd_ddim_sample_hold(C.byref(w), p, p, coef, p, None, None, p, 2, 10, 1, 4, None, 3, other, other, other, draws, None) == -1
        assert b"draws" in h.sd_last_error()
    w.J = 33
    assert h.sd_ddim_sample_hold(C.byref(w), p, p, coef, p, None, None, p, 2, 10, 1, 4, None, 3, other, other, other, 1, None) == -1
    assert b"J must be <= 32" in h.sd_last_error()
    # the session's hold: the joints are read and checked on the host
    joints = (C.c_int32 * 2)(0, 1)
    assert h.sd_session_hold(p, None, p, 0, 0, joints, 2, p, p, None, 2, 2, 10, 20, 1, None) == -1
    assert b"sd_session_hold" in h.sd_last_error()
    assert h.sd_session_hold(p, p, p, 0, 0, None, 2, p, p, None, 2, 2, 10, 20, 1, None) == -1
    assert h.sd_session_hold(p, p, p, 0, 0, joints, 0, p, p, None, 2, 2, 10, 20, 1, None) == -1
    assert h.sd_session_hold(p, p, p, 0, 0, joints, 33, p, p, None, 2, 2, 10, 20, 1, None) == -1
    assert h.sd_session_hold(p, p, p, 0, 0, joints, 2, p, p, None, 2, 2, 10, 33, 1, None) == -1             # J > 32
    assert h.sd_session_hold(p, p, p, 0, 0, joints, 2, p, p, None, 1, 2, 10, 20, 1, None) == -1             # S != B without robots
    assert h.sd_session_hold(p, p, None, 0, 0, joints, 2, p, p, None, 2, 2, 10, 20, 1, None) == -1          # a hold needs values
    assert b"a hold needs" in h.sd_last_error()
    assert h.sd_session_hold(p, p, p, 0, 0, (C.c_int32 * 2)(0, 20), 2, p, p, None, 2, 2, 10, 20, 1, None) == -1
    assert b"out of range" in h.sd_last_error()
    assert h.sd_session_hold(p, p, p, 0, 0, (C.c_int32 * 2)(-1, 3), 2, None, None, None, 2, 2, 10, 20, 0, None) == -1
    assert h.sd_session_hold(p, p, None, 0, 0, joints, 2, None, None, p, 0, 2, 10, 20, 0, None) == 0        # S == 0: no launch
    # the mask's compose launch
    assert h.sd_session_hold_mask(None, p, None, None, 2, 2, 10, 20, 1, None) == -1
    assert b"sd_session_hold_mask" in h.sd_last_error()
    assert h.sd_session_hold_mask(p, None, None, None, 2, 2, 10, 20, 1, None) == -1
    assert h.sd_session_hold_mask(p, p, None, None, 2, 2, 10, 33, 1, None) == -1
    assert h.sd_session_hold_mask(p, p, None, None, 2, 2, 10, 20, 0, None) == -1
    assert h.sd_session_hold_mask(p, p, None, None, 1, 2, 10, 20, 1, None) == -1                            # S != B without robots
    assert h.sd_session_hold_mask(p, p, None, p, 0, 2, 10, 20, 1, None) == 0                                # S == 0: no launch


def test_hold_joints_are_validated_on_the_host():
    from soccerdiffusion_amd import ops

    assert ops.hold_joints([0, 1], 20) == [0, 1] and ops.hold_joints((31,), 32) == [31]
    assert ops.hold_joints(torch.tensor([3, 4]).tolist(), 7) == [3, 4]
    for bad, J in (([], 20), ([20], 20), ([-1], 20), ([1, 1], 20), ([True], 20), ([0.5], 20), (3, 20), ([0], 33)):
        with pytest.raises(ValueError):
            ops.hold_joints(bad, J)


def test_pin_and_hold_exclude_each_other_before_any_device_work():
    from soccerdiffusion_amd import ops

    x = torch.zeros(2, 4, 7)
    with pytest.raises(ValueError, match="exclude"):
        ops.ddim_sample(None, None, torch.zeros(4, 8), None, x, pin=(x, 1), hold=(x, torch.zeros(7, dtype=torch.bool)))
    with pytest.raises(ValueError, match="exclude"):
        ops.ddim_sample_guarded(None, None, torch.zeros(4, 8), None, x, pin=(x, 1), hold=(x, torch.zeros(7, dtype=torch.bool)))


def test_session_holds_are_validated_without_a_device():
    from test_cpu_session import BASE, SHIPPED

    from soccerdiffusion_amd import cli
    from soccerdiffusion_amd.session import PolicySession

    assert PolicySession.check_hold() is False and PolicySession.check_hold(False, 40, True) is False      # today's session
    assert PolicySession.check_hold(True, 22) is True and PolicySession.check_hold(True, 32) is True
    with pytest.raises(ValueError, match="distilled"):
        PolicySession.check_hold(True, 22, distilled=True)
    with pytest.raises(ValueError, match="32"):
        PolicySession.check_hold(True, 33)
    # the constructor checks it before it looks for a device: a CPU model reaches the ValueError, and with valid values the old refusal
    params = {**BASE, **SHIPPED["sim_scratch"], "use_images": False}
    model = cli.build_model(params).eval()
    with pytest.raises(ValueError, match="distilled"):
        PolicySession(model, holds=True, distilled=True)
    with pytest.raises(ValueError, match="distilled"):
        PolicySession(model, holds=True, hyperparams={**params, "distilled_decoder": True})
    with pytest.raises(RuntimeError, match="on the CPU"):
        PolicySession(model, holds=True)


def test_cli_hold_flag_is_parsed_and_checked():
    import argparse

    from soccerdiffusion_amd import cli

    ap = cli.build_parser()
    args = ap.parse_args(["rollout", "ckpt.pt", "--synthetic", "2", "--ticks", "1", "--hold", "0=0.5,3=-1.25"])
    assert args.hold == [(0, 0.5), (3, -1.25)]
    assert ap.parse_args(["rollout", "ckpt.pt", "--synthetic", "2", "--ticks", "1"]).hold is None
    assert ap.parse_args(["sample", "ckpt.pt", "--hold", "21=0"]).hold == [(21, 0.0)]
    for bad in ("", "0", "0=a", "x=1", "-1=0.5", "0=1,0=2", "0=1;1=2"):
        with pytest.raises(argparse.ArgumentTypeError):
            cli._hold(bad)
    assert cli._hold_joints([(0, 0.5), (3, -1.25)], 20) == ([0, 3], [0.5, -1.25])
    with pytest.raises(SystemExit):
        cli._hold_joints([(20, 0.5)], 20)
    with pytest.raises(SystemExit):
        cli._hold_joints([(0, 0.5)], 33)
