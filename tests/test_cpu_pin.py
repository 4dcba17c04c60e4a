"""CPU-only checks of the sampler's pinned leading rows and of the session's carry (sd_ddim_sample_pin, sd_session_commit_carry(_at),
sd_session_reset_carry): the CPU reference tests/pin_ref.py against oracle/ddim_ref.py, the new entry points in the header, in
_lib.SIGNATURES and in the built library, their argument errors without a device, and the Python-side validation that needs none."""

import ctypes as C
import os
import re

import pytest
import torch

import pin_ref
from conftest import REPO
from oracle import ddim_ref

NEW = ("sd_ddim_sample_pin", "sd_session_commit_carry", "sd_session_commit_carry_at", "sd_session_reset_carry")


@pytest.fixture(scope="module")
def lib():
    from soccerdiffusion_amd import build

    build.build()
    from soccerdiffusion_amd import _lib

    return _lib


def _toy_denoiser(seed, J):
    """A fixed non-linear map (B, T, J) -> (B, T, J) that mixes the rows of a trajectory, as self-attention does."""
    g = torch.Generator().manual_seed(seed)
    W = torch.randn(J, J, generator=g) / J ** 0.5

    def denoise(x, t):
        return torch.tanh(x @ W + x.mean(dim=1, keepdim=True)) * (1.0 + t / 1000.0)

    return denoise


def test_pin_ref_without_pinned_rows_is_ddim_ref_exactly():
    B, T, J, n = 3, 10, 7, 4
    g = torch.Generator().manual_seed(1)
    x_T, known = torch.randn(B, T, J, generator=g), torch.randn(B, T, J, generator=g)
    den = _toy_denoiser(2, J)
    want = ddim_ref.sample(den, x_T, n)
    for rows in (0, torch.zeros(B, dtype=torch.int64)):
        got, _, eps = pin_ref.sample(den, x_T, known, rows, n)
        assert len(got) == n == len(eps)
        assert all(torch.equal(a, b) for a, b in zip(got, want))


def test_pin_ref_pinned_rows_follow_the_forward_process_and_end_on_known():
    B, T, J, n = 3, 10, 7, 4
    g = torch.Generator().manual_seed(3)
    x_T, known = torch.randn(B, T, J, generator=g), torch.randn(B, T, J, generator=g)
    rows = torch.tensor([0, 3, 10])
    den = _toy_denoiser(4, J)
    acp = ddim_ref.alphas_cumprod()
    ts = ddim_ref.timesteps(n)
    seen = []
    got, pinned, _ = pin_ref.sample(lambda x, t: (seen.append(x.clone()), den(x, t))[1], x_T, known, rows, n)
    mask = pin_ref.pin_mask(rows, B, T).expand(B, T, J)
    assert mask.sum().item() == (0 + 3 + 10) * J
    # at the entry of every step the pinned rows are a training-time add_noise sample at that step's t (leading spacing: a_prev of step i
    # is a_t of step i + 1)
    for i, x in enumerate(seen):
        noised = ddim_ref.add_noise(known, x_T, torch.full((B,), int(ts[i])), acp)
        assert torch.equal(x[mask], noised[mask]), i
    assert all(torch.equal(x[mask], p[mask]) for x, p in zip(got, pinned))
    assert torch.equal(got[-1][mask], known[mask])                                   # exactly, not approximately
    free = ddim_ref.sample(den, x_T, n)[-1]
    assert torch.equal(got[-1][0], free[0])                                          # the unpinned trajectory of a mixed batch
    assert not torch.equal(got[-1][1, 3:], free[1, 3:])                              # the free rows of a pinned one read the pinned rows
    # the coefficient table the kernels get says the same: (c2, c3) of step i = (c0, c1) of step i + 1; the last step is (1, 0)
    from soccerdiffusion_amd import ops

    coef = ops.ddim_coefficients(ts.tolist(), acp, n)
    assert (coef[:-1, 2] == coef[1:, 0]).all() and (coef[:-1, 3] == coef[1:, 1]).all()
    assert coef[-1, 2] == 1.0 and coef[-1, 3] == 0.0


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
    assert "#define SD_ABI_VERSION 1" in header and h.sd_abi_version() == 1
    # sd_ddim_sample_pin = sd_ddim_sample_eps's arguments + pin_x0, pin_noise, pin_rows in front of the stream
    eps, pin = lib.SIGNATURES["sd_ddim_sample_eps"][1], lib.SIGNATURES["sd_ddim_sample_pin"][1]
    assert pin == eps[:-1] + [C.c_void_p] * 3 + eps[-1:]


def test_new_entry_points_reject_bad_arguments_without_gpu(lib):
    h = lib.load()
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    other = C.cast((C.c_float * 64)(), C.c_void_p)
    coef = (C.c_float * 16)()
    w = lib.DenoiserWeights()
    # null pin pointers and pin_noise == x are refused before the weights are even looked at
    for x0, noise, rows in ((None, other, p), (other, None, p), (other, other, None)):
        assert h.sd_ddim_sample_pin(C.byref(w), p, p, coef, p, None, None, p, 1, 10, 1, 4, None, 3, x0, noise, rows, None) == -1
        assert b"sd_ddim_sample_pin" in h.sd_last_error()
    assert h.sd_ddim_sample_pin(C.byref(w), p, p, coef, p, None, None, p, 1, 10, 1, 4, None, 3, other, p, other, None) == -1
    assert b"alias" in h.sd_last_error()
    # commit with carry: null pointers, advance + carry > T, negative counts
    assert h.sd_session_commit_carry(None, None, None, None, None, None, 1, 10, 20, 100, 5, 4, None, None, None) == -1
    assert b"sd_session_commit_carry" in h.sd_last_error()
    assert h.sd_session_commit_carry(p, p, p, p, p, p, 1, 10, 4, 4, 7, 4, p, p, None) == -1
    assert h.sd_session_commit_carry(p, p, p, p, p, p, 1, 10, 4, 4, -1, 4, p, p, None) == -1
    assert h.sd_session_commit_carry(p, p, p, p, p, p, 1, 10, 4, 4, 5, 4, None, p, None) == -1
    assert h.sd_session_commit_carry_at(p, p, p, p, p, p, None, 1, 1, 10, 4, 4, 5, 4, p, p, None) == -1
    assert b"sd_session_commit_carry_at" in h.sd_last_error()
    assert h.sd_session_commit_carry_at(p, p, p, p, p, p, p, 1, 1, 10, 4, 4, 5, 6, p, p, None) == -1
    assert h.sd_session_commit_carry_at(None, p, p, None, p, p, None, 0, 1, 10, 4, 4, 5, 4, p, p, None) == 0      # S == 0: no launch
    rings = (lib.RingReset * 1)()
    rings[0].ring, rings[0].head, rings[0].L, rings[0].C = p.value, p.value, 4, 4
    assert h.sd_session_reset_carry(rings, 1, None, None, 0, None, 1, None) == -1
    assert b"sd_session_reset_carry" in h.sd_last_error()
    assert h.sd_session_reset_carry(rings, 6, None, None, 0, p, 1, None) == -1
    assert h.sd_session_reset_carry(None, 1, None, None, 0, p, 1, None) == -1


def test_pin_rows_are_validated_on_the_host():
    from soccerdiffusion_amd import ops

    B, T = 3, 10
    assert ops.pin_rows(4, B, T, "cpu").tolist() == [4, 4, 4] and ops.pin_rows(4, B, T, "cpu").dtype == torch.int32
    assert ops.pin_rows(0, B, T, "cpu").tolist() == [0, 0, 0] and ops.pin_rows(T, B, T, "cpu").tolist() == [T] * B
    assert ops.pin_rows([0, 3, 10], B, T, "cpu").tolist() == [0, 3, 10]
    assert ops.pin_rows(torch.tensor([0, 3, 10]), B, T, "cpu").dtype == torch.int32
    for bad in (-1, T + 1, [0, 3, 11], torch.tensor([0, -1, 2]), torch.tensor([1, 2]), torch.tensor([1.0, 2.0, 3.0]), True, "3", [[1, 2, 3]]):
        with pytest.raises(ValueError, match="pin rows"):
            ops.pin_rows(bad, B, T, "cpu")


def test_session_carry_and_advance_are_validated_without_a_device():
    from test_cpu_session import BASE, SHIPPED

    from soccerdiffusion_amd import cli
    from soccerdiffusion_amd.session import PolicySession

    T = 10
    assert PolicySession.check_carry(T) == (0, 10)                      # today's session
    assert PolicySession.check_carry(T, 4) == (4, 6)                    # advance defaults to T - carry
    assert PolicySession.check_carry(T, 4, 5) == (4, 5)
    assert PolicySession.check_carry(T, 0, 3) == (0, 3)
    assert PolicySession.check_carry(T, 9) == (9, 1)
    for carry, advance, what in ((-1, None, "carry"), (4, 0, "advance"), (10, None, "advance"), (4, 7, "exceeds"), (0, 11, "exceeds")):
        with pytest.raises(ValueError, match=what):
            PolicySession.check_carry(T, carry, advance)
    with pytest.raises(ValueError, match="distilled"):
        PolicySession.check_carry(T, 4, 5, distilled=True)
    assert PolicySession.check_carry(T, 0, 5, distilled=True) == (0, 5)
    # the constructor checks them before it looks for a device: a CPU model reaches the ValueError, and with valid values the old refusal
    params = {**BASE, **SHIPPED["sim_scratch"], "use_images": False}
    model = cli.build_model(params).eval()
    with pytest.raises(ValueError, match="exceeds"):
        PolicySession(model, carry=4, advance=7)
    with pytest.raises(ValueError, match="distilled"):
        PolicySession(model, carry=4, distilled=True)
    with pytest.raises(ValueError, match="distilled"):
        PolicySession(model, carry=4, hyperparams={**params, "distilled_decoder": True})
    with pytest.raises(RuntimeError, match="on the CPU"):
        PolicySession(model, carry=4, advance=5)
