"""Tensor-level wrappers over the C ABI (include/soccerdiffusion_hip.h).

PyTorch is plumbing here: it owns device memory and the stream; every computation is a
HIP kernel behind ``libsoccerdiffusion_hip.so``.  All functions require contiguous fp32
CUDA(HIP) tensors and raise otherwise — there is no CPU path in this package.
"""

from __future__ import annotations

import ctypes as C
import functools
import math
import operator
import sys
from typing import Mapping, Optional, Sequence

import numpy as np
import torch

from . import _lib
from ._lib import DenoiserWeights, EncoderWeights, LayerWeights, check
from .derived import bump_weights_generation, current, version_key, weights_generation  # noqa: F401  (callers use ops.weights_generation())

Tensor = torch.Tensor
NUM_TRAIN_TIMESTEPS = 1000


def _ptr(t: Optional[Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _req(t: Tensor, name: str, dtype=torch.float32) -> Tensor:
    if not t.is_cuda:
        raise RuntimeError(f"{name}: expected a tensor on the MI355X (cuda) device, got {t.device}; "
                           "soccerdiffusion_amd has no CPU path")
    if t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name}: expected a contiguous tensor")
    return t


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


# --------------------------------------------------------------------------------------
# host-side tables, built exactly as the reference builds them (fp32 CPU ops)
# --------------------------------------------------------------------------------------
def positional_table(d_model: int, max_len: int) -> Tensor:
    """The ``pe`` buffer of PositionalEncoding (reference ml/model/misc.py:43-56), CPU fp32."""
    pe = torch.zeros(max_len, d_model)
    position = torch.arange(0, max_len, dtype=torch.float).unsqueeze(1)
    div_term = torch.exp(torch.arange(0, d_model, 2).float() * (-math.log(10000.0) / d_model))
    pe[:, 0::2] = torch.sin(position * div_term)
    pe[:, 1::2] = torch.cos(position * div_term)
    return pe


def step_frequencies(dim: int) -> Tensor:
    """Frequency table of StepToken (reference ml/model/misc.py:31-32), CPU fp32."""
    half_dim = dim // 4
    return torch.exp(torch.arange(half_dim) * -math.log(10000) / (half_dim - 1))


def alphas_cumprod(num_train_timesteps: int = NUM_TRAIN_TIMESTEPS) -> Tensor:
    """squaredcos_cap_v2 schedule of the scheduler the reference constructs at
    ml/training/train.py:185 (diffusers DDIMScheduler defaults)."""
    def alpha_bar(s):
        return math.cos((s + 0.008) / 1.008 * math.pi / 2) ** 2

    n = num_train_timesteps
    betas = torch.tensor([min(1 - alpha_bar((i + 1) / n) / alpha_bar(i / n), 0.999) for i in range(n)],
                         dtype=torch.float32)
    return torch.cumprod(1.0 - betas, dim=0)


def ddim_timesteps(num_inference_steps: int, num_train_timesteps: int = NUM_TRAIN_TIMESTEPS) -> list[int]:
    """``set_timesteps`` (leading spacing, offset 0): e.g. 50 -> 980, 960, ..., 0."""
    ratio = num_train_timesteps // num_inference_steps
    return [int(round(i * ratio)) for i in range(num_inference_steps)][::-1]


def ddim_coefficients(timesteps: Sequence[int], acp: Tensor, num_inference_steps: int,
                      num_train_timesteps: int = NUM_TRAIN_TIMESTEPS) -> np.ndarray:
    """Per step (sqrt a_t, sqrt(1-a_t), sqrt a_prev, sqrt(1-a_prev)) as fp32 (eta = 0,
    final_alpha_cumprod = 1).  Computed with fp32 tensor ops like the scheduler does."""
    acp = acp.detach().cpu().float()
    ratio = num_train_timesteps // num_inference_steps
    out = np.zeros((len(timesteps), 4), dtype=np.float32)
    one = torch.tensor(1.0)
    for i, t in enumerate(timesteps):
        prev = t - ratio
        a_t = acp[t]
        a_p = acp[prev] if prev >= 0 else one
        out[i] = [float(a_t.sqrt()), float((1 - a_t).sqrt()), float(a_p.sqrt()), float((1 - a_p).sqrt())]
    return out


def multistep_weights(timesteps: Sequence[int], acp: Tensor, num_inference_steps: int,
                      num_train_timesteps: int = NUM_TRAIN_TIMESTEPS) -> np.ndarray:
    """The history weights of the second-order multistep solver (DPM-Solver++ 2M in its x0 form) on the grid of ``ddim_coefficients``
    (the same ``prev = t - ratio`` convention): after the DDIM update of step i, ``x += w[i] * (x0[i - 1] - x0[i])`` with
    ``w[i] = sqrt(a_prev) * expm1(-h[i]) * h[i] / (2 h[i - 1])``, ``h[i] = lambda(a_prev) - lambda(a_t)``, ``lambda(a) = 0.5 log(a / (1 - a))``.
    lambda and h are Python float64 from the fp32 ``acp`` table, the weight is rounded once to fp32.  ``w[0] = 0`` (no history yet) and
    ``w[i] = 0`` wherever ``a_prev = 1`` (lambda is infinite there: that step is first order).  All zeros is DDIM itself.
    ValueError unless the timesteps are the consecutive leading grid, ``t[i] == t[i - 1] - ratio``: the history term is defined only there."""
    acp = acp.detach().cpu().float()
    ratio = num_train_timesteps // num_inference_steps
    ts = [int(t) for t in timesteps]
    for i in range(1, len(ts)):
        if ts[i] != ts[i - 1] - ratio:
            raise ValueError(f"multistep_weights: timesteps must be the consecutive leading grid (t[i] == t[i - 1] - {ratio}); "
                             f"got t[{i - 1}] = {ts[i - 1]}, t[{i}] = {ts[i]}")

    def lam(a: float) -> float:
        return 0.5 * math.log(a / (1.0 - a))

    out = np.zeros(len(ts), dtype=np.float32)
    h_prev = None
    for i, t in enumerate(ts):
        prev = t - ratio
        if prev < 0:   # a_prev = 1
            h_prev = None
            continue
        a_t, a_p = float(acp[t]), float(acp[prev])
        h = lam(a_p) - lam(a_t)
        if i > 0 and h_prev is not None:
            out[i] = np.float32(math.sqrt(a_p) * math.expm1(-h) * h / (2.0 * h_prev))
        h_prev = h
    return out


def _multistep_req(w, n_steps: int) -> np.ndarray:
    """``multistep`` of a sampler call, validated before any launch: (n_steps,) finite fp32 weights with w[0] == 0."""
    try:
        w = np.ascontiguousarray(w, dtype=np.float32)
    except (TypeError, ValueError):
        raise ValueError(f"multistep: expected ({n_steps},) weights (ops.multistep_weights), got {w!r}") from None
    if w.shape != (n_steps,):
        raise ValueError(f"multistep: expected ({n_steps},) weights (ops.multistep_weights), got shape {w.shape}")
    if not np.isfinite(w).all():
        raise ValueError("multistep: the weights must be finite")
    if w[0] != 0:
        raise ValueError(f"multistep: w[0] must be 0 (the first step has no history), got {float(w[0])}")
    return w


def multistep_step(eps: Tensor, x: Tensor, hist: Tensor, coef4, w: float) -> Tensor:
    """One step of the second-order multistep solver for a caller that evaluates the denoiser itself (``sd_multistep_step``):
    returns the DDIM update of (eps, x) with ``coef4`` plus ``w * (hist - x0)`` and leaves this step's x0 in ``hist`` (updated in place;
    not read when ``w == 0``)."""
    lib = _lib.load()
    _req(eps, "eps"); _req(x, "x"); _req(hist, "hist")
    if eps.shape != x.shape or hist.shape != x.shape:
        raise ValueError("multistep_step: eps, x and hist must have one shape")
    out = torch.empty_like(x)
    c = np.ascontiguousarray([float(v) for v in coef4], dtype=np.float32)
    if c.shape != (4,):
        raise ValueError("multistep_step: coef4 must hold 4 scalars")
    check(lib.sd_multistep_step(eps.data_ptr(), x.data_ptr(), out.data_ptr(), hist.data_ptr(), c.ctypes.data_as(_lib.c_float_p), float(w),
                                x.numel(), _stream()), "sd_multistep_step")
    return out


class Limits(tuple):
    """``(lo, hi)`` as ``joint_limits`` returns them: two (32,) fp32 device arrays, validated and padded - what the kernels read."""
    __slots__ = ()
    lo = property(lambda self: self[0])
    hi = property(lambda self: self[1])


def _limits_host(limits, J: int):
    """``limits`` - ``(lo, hi)``, one range r or ``{joint: (lo, hi)}`` - as two (32,) fp32 host arrays padded with -inf / +inf, validated:
    see ``joint_limits``."""
    lo, hi = limits if isinstance(limits, tuple) and len(limits) == 2 else (limits, None)
    if isinstance(J, bool) or not 1 <= int(J) <= 32:
        raise ValueError(f"limits: the 32-float limit arrays describe at most 32 joints, got J = {J}")
    J = int(J)
    out_lo, out_hi = np.full(32, -np.inf, dtype=np.float32), np.full(32, np.inf, dtype=np.float32)
    if isinstance(lo, Mapping) and hi is None:
        for j, pair in lo.items():
            if isinstance(j, bool) or not isinstance(j, (int, np.integer)) or not 0 <= int(j) < J:
                raise ValueError(f"limits: joint index {j!r} out of range 0 .. {J - 1}")
            try:
                a, b = pair
            except (TypeError, ValueError):
                raise ValueError(f"limits: joint {j}: expected (lo, hi), got {pair!r}") from None
            out_lo[int(j)], out_hi[int(j)] = a, b
    elif hi is None:
        try:
            r = float(lo)
        except (TypeError, ValueError):
            raise ValueError(f"limits: expected (lo, hi) arrays of {J} floats, one range r, or {{joint: (lo, hi)}}; got {lo!r}") from None
        if not r >= 0:
            raise ValueError(f"limits: a range must be >= 0 and not NaN, got {r}")
        out_lo[:J], out_hi[:J] = -r, r
    else:
        def arr(v, name):
            v = v.detach().cpu().numpy() if isinstance(v, Tensor) else v
            v = np.asarray(v, dtype=np.float32)
            if v.shape != (J,):
                raise ValueError(f"limits {name}: expected ({J},) floats, got shape {v.shape}")
            return v
        out_lo[:J], out_hi[:J] = arr(lo, "lo"), arr(hi, "hi")
    if np.isnan(out_lo).any() or np.isnan(out_hi).any():
        raise ValueError("limits: NaN is not a limit (use -inf / +inf for no limit on a side)")
    if not (out_lo <= out_hi).all():
        j = int(np.argmax(~(out_lo <= out_hi)))
        raise ValueError(f"limits: lo[{j}] = {out_lo[j]} > hi[{j}] = {out_hi[j]}")
    return out_lo, out_hi


def joint_limits(lo, hi=None, J: Optional[int] = None, device=None) -> Limits:
    """Per-joint limits of ``ddim_sample(limits=...)`` as the kernels read them (``sd_ddim_sample_limits``): two (32,) fp32 arrays on
    ``device``, entries [J, 32) padded with -inf / +inf.  All in the sampler's normalised space.  ``lo``, ``hi``: (J,) floats (tensors,
    arrays or lists) with ``lo[j] <= hi[j]``; -inf / +inf: no limit on that side.  ``joint_limits(r, J=J, device=...)``: one range,
    (-r, r) on every joint (diffusers' ``clip_sample_range``).  ``joint_limits({joint: (lo, hi)}, J=J, device=...)``: the named joints,
    every other unlimited.  ValueError for a wrong shape, a NaN, ``lo > hi``, a joint index outside 0 .. J - 1, or J > 32."""
    if J is None or device is None:
        raise ValueError("joint_limits: J and device must be given")
    out_lo, out_hi = _limits_host(lo if hi is None else (lo, hi), J)
    return Limits((torch.from_numpy(out_lo).to(device), torch.from_numpy(out_hi).to(device)))


def _limits_req(limits, J: int, device) -> Limits:
    """``limits`` of a sampler call, validated: a ``Limits`` on the device as it is; else ``(lo, hi)``, a range or a dict through
    ``joint_limits``."""
    if isinstance(limits, Limits):
        for t in limits:
            if not isinstance(t, Tensor) or tuple(t.shape) != (32,) or t.dtype != torch.float32 or t.device != torch.device(device) or not t.is_contiguous() or t.data_ptr() % 16:
                raise ValueError(f"limits: expected the two (32,) fp32 arrays of ops.joint_limits on {device}")
        if J > 32:
            raise ValueError(f"limits: the 32-float limit arrays describe at most 32 joints, got J = {J}")
        return limits
    return joint_limits(limits, J=J, device=device)


def limit_step(eps: Tensor, x: Tensor, coef4, limits: Limits, hist: Optional[Tensor] = None, w: float = 0.0, reproject: bool = False) -> Tensor:
    """One step under per-joint limits for a caller that evaluates the denoiser itself (``sd_ddim_limit_step``): x0 of (eps, x) with
    ``coef4`` is clamped to ``limits`` (joint = last dimension), the update is formed from the clamped x0 (``reproject``: a clamped
    element's eps is recomputed from it) plus ``w * (hist - x0c)``; the clamped x0 is left in ``hist`` where one is given."""
    lib = _lib.load()
    _req(eps, "eps"); _req(x, "x")
    if eps.shape != x.shape or (hist is not None and hist.shape != x.shape):
        raise ValueError("limit_step: eps, x and hist must have one shape")
    if hist is not None:
        _req(hist, "hist")
    limits = _limits_req(limits, x.shape[-1], x.device)
    out = torch.empty_like(x)
    c = np.ascontiguousarray([float(v) for v in coef4], dtype=np.float32)
    if c.shape != (4,):
        raise ValueError("limit_step: coef4 must hold 4 scalars")
    check(lib.sd_ddim_limit_step(eps.data_ptr(), x.data_ptr(), out.data_ptr(), _ptr(hist), c.ctypes.data_as(_lib.c_float_p), float(w),
                                 limits.lo.data_ptr(), limits.hi.data_ptr(), int(bool(reproject)), x.numel(), x.shape[-1], _stream()),
          "sd_ddim_limit_step")
    return out


def _slew_host(v, J: int) -> np.ndarray:
    """``v`` - (J,) floats, one number or ``{joint: v}`` - as the (32,) fp32 host array padded with +inf, validated: see ``joint_slew``."""
    if isinstance(J, bool) or not 1 <= int(J) <= 32:
        raise ValueError(f"slew: the 32-float array describes at most 32 joints, got J = {J}")
    J = int(J)
    out = np.full(32, np.inf, dtype=np.float32)
    if isinstance(v, Mapping):
        for j, val in v.items():
            if isinstance(j, bool) or not isinstance(j, (int, np.integer)) or not 0 <= int(j) < J:
                raise ValueError(f"slew: joint index {j!r} out of range 0 .. {J - 1}")
            try:
                out[int(j)] = float(val)
            except (TypeError, ValueError):
                raise ValueError(f"slew: joint {j}: expected one number, got {val!r}") from None
    else:
        arr = v.detach().cpu().numpy() if isinstance(v, Tensor) else v
        try:
            arr = np.asarray(arr, dtype=np.float32)
        except (TypeError, ValueError):
            raise ValueError(f"slew: expected ({J},) floats, one number or {{joint: v}}, got {v!r}") from None
        if arr.shape not in ((), (J,)):
            raise ValueError(f"slew: expected ({J},) floats or one number, got shape {arr.shape}")
        out[:J] = arr
    if np.isnan(out).any():
        raise ValueError("slew: NaN is not a limit (use +inf for no limit)")
    if not (out >= 0).all():
        j = int(np.argmax(~(out >= 0)))
        raise ValueError(f"slew: v[{j}] = {out[j]} is negative")
    return out


def joint_slew(v, J: Optional[int] = None, device=None) -> Tensor:
    """Per-joint slew limits of ``ddim_sample(slew=...)`` as the kernels read them (``sd_ddim_sample_slew``): one (32,) fp32 array on
    ``device``, entries [J, 32) padded with +inf.  ``v[j] >= 0`` is the largest change of joint j between consecutive rows of the
    trajectory, in the sampler's normalised space; +inf: none.  ``v``: (J,) floats, one number for every joint, or ``{joint: v}`` (every
    other joint unlimited).  ValueError for a NaN, a negative value, a wrong shape, a joint index outside 0 .. J - 1, or J > 32."""
    if J is None or device is None:
        raise ValueError("joint_slew: J and device must be given")
    return torch.from_numpy(_slew_host(v, J)).to(device)


def _is_dev32(t, device, rows: Optional[int] = None) -> bool:
    shape = (32,) if rows is None else (rows, 32)
    return (isinstance(t, Tensor) and tuple(t.shape) == shape and t.dtype == torch.float32 and t.device == torch.device(device)
            and t.is_contiguous() and t.data_ptr() % 16 == 0)


def _slew_req(slew, B: int, J: int, device) -> tuple:
    """``slew`` of a sampler call, validated: ``v`` or ``(v, start)`` -> (v (32,) on the device, start (B, 32) on the device or None).
    ``v``: a (32,) fp32 array of ``joint_slew`` on the device as it is, else through ``joint_slew``.  ``start``: (B, J) or (B, 32) floats,
    the value "before row 0" per trajectory (NaN: none); a contiguous (B, 32) fp32 device tensor is used as it is, anything else is padded
    with NaN into a new one."""
    pair = isinstance(slew, tuple) and len(slew) == 2 and (slew[1] is None or getattr(slew[1], "ndim", 0) >= 1)   # (v, start), not two floats
    v, start = slew if pair else (slew, None)
    if J > 32:
        raise ValueError(f"slew: the 32-float array describes at most 32 joints, got J = {J}")
    if not _is_dev32(v, device):
        v = joint_slew(v, J=J, device=device)
    if start is not None and not _is_dev32(start, device, B):
        st = start.detach() if isinstance(start, Tensor) else torch.as_tensor(np.asarray(start, dtype=np.float32))
        if st.dim() != 2 or st.shape[0] != B or st.shape[1] not in (J, 32):
            raise ValueError(f"slew start: expected ({B}, {J}) or ({B}, 32) floats, got {tuple(st.shape)}")
        start = torch.full((B, 32), float("nan"), dtype=torch.float32, device=device)
        start[:, :J] = st[:, :J].to(device=device, dtype=torch.float32)
    return v, start


def slew_step(eps: Tensor, x: Tensor, coef4, slew, limits=None, hist: Optional[Tensor] = None, w: float = 0.0, reproject: bool = False,
              hold=None) -> Tensor:
    """One step under per-joint slew limits for a caller that evaluates the denoiser itself (``sd_ddim_slew_step``): ``limit_step`` with
    the scan of ``ddim_sample(slew=...)`` over the rows of every trajectory.  ``eps``, ``x`` (and ``hist``): whole (B, T, J) samples.
    ``slew``: ``v`` or ``(v, start)``; ``limits``: as ``limit_step`` takes them (default: none).  ``hold = (known, mask)``: held elements
    enter the scan as ``known``; their returned value is the scan's update of it, which the caller's hold overwrites."""
    lib = _lib.load()
    _req(eps, "eps"); _req(x, "x")
    if x.dim() != 3 or eps.shape != x.shape or (hist is not None and hist.shape != x.shape):
        raise ValueError("slew_step: eps, x and hist must be whole (B, T, J) samples of one shape")
    if hist is not None:
        _req(hist, "hist")
    B, T, J = x.shape
    v, start = _slew_req(slew, B, J, x.device)
    limits = _limits_req({} if limits is None else limits, J, x.device)
    known, mask = (None, None) if hold is None else _hold_req(hold, B, T, J, x.device)
    out = torch.empty_like(x)
    c = np.ascontiguousarray([float(t) for t in coef4], dtype=np.float32)
    if c.shape != (4,):
        raise ValueError("slew_step: coef4 must hold 4 scalars")
    check(lib.sd_ddim_slew_step(eps.data_ptr(), x.data_ptr(), out.data_ptr(), _ptr(hist), c.ctypes.data_as(_lib.c_float_p), float(w),
                                limits.lo.data_ptr(), limits.hi.data_ptr(), int(bool(reproject)), v.data_ptr(), _ptr(start), _ptr(known), _ptr(mask),
                                B, T, J, _stream()), "sd_ddim_slew_step")
    return out


def _accel_host(a, J: int) -> np.ndarray:
    """``a`` - (J,) floats, one number or ``{joint: a}`` - as the (32,) fp32 host array padded with +inf, validated as ``joint_slew``
    validates ``v``: see ``joint_accel``."""
    try:
        return _slew_host(a, J)
    except ValueError as e:
        raise ValueError(str(e).replace("slew:", "accel:").replace("v[", "a[")) from None


def joint_accel(a, J: Optional[int] = None, device=None) -> Tensor:
    """Per-joint acceleration limits of ``ddim_sample(accel=...)`` as the kernels read them (``sd_ddim_sample_accel``): one (32,) fp32
    array on ``device``, entries [J, 32) padded with +inf.  ``a[j] >= 0`` is the largest second difference of joint j over three
    consecutive rows of the trajectory, in the sampler's normalised space; +inf: none.  ``a``: (J,) floats, one number for every joint, or
    ``{joint: a}`` (every other joint unlimited).  ValueError for a NaN, a negative value, a wrong shape, a joint index outside
    0 .. J - 1, or J > 32."""
    if J is None or device is None:
        raise ValueError("joint_accel: J and device must be given")
    return torch.from_numpy(_accel_host(a, J)).to(device)


def _accel_req(accel, B: int, J: int, device) -> tuple:
    """``accel`` of a sampler call, validated: ``a`` or ``(a, start2)`` -> (a (32,) on the device, start2 (B, 32) on the device or None),
    as ``_slew_req`` does it for ``(v, start)``; ``start2`` is the value two rows "before row 0" per trajectory (NaN: none)."""
    pair = isinstance(accel, tuple) and len(accel) == 2 and (accel[1] is None or getattr(accel[1], "ndim", 0) >= 1)   # (a, start2), not two floats
    a, start2 = accel if pair else (accel, None)
    if J > 32:
        raise ValueError(f"accel: the 32-float array describes at most 32 joints, got J = {J}")
    if not _is_dev32(a, device):
        a = joint_accel(a, J=J, device=device)
    if start2 is not None and not _is_dev32(start2, device, B):
        st = start2.detach() if isinstance(start2, Tensor) else torch.as_tensor(np.asarray(start2, dtype=np.float32))
        if st.dim() != 2 or st.shape[0] != B or st.shape[1] not in (J, 32):
            raise ValueError(f"accel start2: expected ({B}, {J}) or ({B}, 32) floats, got {tuple(st.shape)}")
        start2 = torch.full((B, 32), float("nan"), dtype=torch.float32, device=device)
        start2[:, :J] = st[:, :J].to(device=device, dtype=torch.float32)
    return a, start2


def accel_step(eps: Tensor, x: Tensor, coef4, accel, slew=None, limits=None, hist: Optional[Tensor] = None, w: float = 0.0,
               reproject: bool = False, hold=None) -> Tensor:
    """One step under per-joint acceleration limits for a caller that evaluates the denoiser itself (``sd_ddim_accel_step``):
    ``slew_step`` with the scan of ``ddim_sample(accel=...)`` over the rows of every trajectory.  ``accel``: ``a`` or ``(a, start2)``;
    ``slew`` (default: no slew limit and no anchor) and everything else as ``slew_step`` takes them."""
    lib = _lib.load()
    _req(eps, "eps"); _req(x, "x")
    if x.dim() != 3 or eps.shape != x.shape or (hist is not None and hist.shape != x.shape):
        raise ValueError("accel_step: eps, x and hist must be whole (B, T, J) samples of one shape")
    if hist is not None:
        _req(hist, "hist")
    B, T, J = x.shape
    a, start2 = _accel_req(accel, B, J, x.device)
    v, start = _slew_req({} if slew is None else slew, B, J, x.device)
    limits = _limits_req({} if limits is None else limits, J, x.device)
    known, mask = (None, None) if hold is None else _hold_req(hold, B, T, J, x.device)
    out = torch.empty_like(x)
    c = np.ascontiguousarray([float(t) for t in coef4], dtype=np.float32)
    if c.shape != (4,):
        raise ValueError("accel_step: coef4 must hold 4 scalars")
    check(lib.sd_ddim_accel_step(eps.data_ptr(), x.data_ptr(), out.data_ptr(), _ptr(hist), c.ctypes.data_as(_lib.c_float_p), float(w),
                                 limits.lo.data_ptr(), limits.hi.data_ptr(), int(bool(reproject)), v.data_ptr(), _ptr(start), a.data_ptr(),
                                 _ptr(start2), _ptr(known), _ptr(mask), B, T, J, _stream()), "sd_ddim_accel_step")
    return out


# --------------------------------------------------------------------------------------
# weight descriptors
# --------------------------------------------------------------------------------------
_DEC_KEYS = {
    "sa_in_w": "self_attn.in_proj_weight", "sa_in_b": "self_attn.in_proj_bias",
    "sa_out_w": "self_attn.out_proj.weight", "sa_out_b": "self_attn.out_proj.bias",
    "ca_in_w": "multihead_attn.in_proj_weight", "ca_in_b": "multihead_attn.in_proj_bias",
    "ca_out_w": "multihead_attn.out_proj.weight", "ca_out_b": "multihead_attn.out_proj.bias",
    "lin1_w": "linear1.weight", "lin1_b": "linear1.bias", "lin2_w": "linear2.weight", "lin2_b": "linear2.bias",
    "n1_w": "norm1.weight", "n1_b": "norm1.bias", "n2_w": "norm2.weight", "n2_b": "norm2.bias",
    "n3_w": "norm3.weight", "n3_b": "norm3.bias",
}


class _Packed:
    """Keeps the ctypes structs and every tensor they point at alive together."""

    def __init__(self):
        self.keep: list[Tensor] = []
        self.layers = None
        self.struct = None

    def dev(self, t: Tensor, device) -> Tensor:
        t = t.detach()
        if t.device != device or t.dtype != torch.float32 or not t.is_contiguous():
            t = t.to(device=device, dtype=torch.float32).contiguous()
        self.keep.append(t)
        return t

    def fill_layers(self, sd: Mapping[str, Tensor], stem: str, n_layers: int, device, decoder: bool):
        arr = (LayerWeights * n_layers)()
        for l in range(n_layers):
            for field, key in _DEC_KEYS.items():
                full = f"{stem}{l}.{key}"
                if full in sd:
                    setattr(arr[l], field, self.dev(sd[full], device).data_ptr())
                elif decoder or not (field.startswith("ca_") or field.startswith("n3_")):
                    raise KeyError(f"missing weight {full}")
        self.layers = arr


def _count_layers(sd: Mapping[str, Tensor], stem: str) -> int:
    n = 0
    while f"{stem}{n}.norm1.weight" in sd:
        n += 1
    return n


def pack_denoiser(sd: Mapping[str, Tensor], device, prefix: str = "diffusion_action_generator.",
                  heads: int = 4, max_len: Optional[int] = None) -> _Packed:
    """Builds the ``sd_denoiser_weights`` descriptor from checkpoint-keyed tensors
    (zero-copy for tensors already on ``device``)."""
    device = torch.device(device)
    p = _Packed()
    emb_w = p.dev(sd[prefix + "embedding.weight"], device)
    d, J = emb_w.shape
    stem = prefix + "transformer_decoder.layers."
    L = _count_layers(sd, stem)
    p.fill_layers(sd, stem, L, device, decoder=True)
    T_max = int(max_len) if max_len is not None else 512
    pe = p.dev(positional_table(d, T_max), device)
    w = DenoiserWeights()
    w.d, w.J, w.L, w.heads = d, J, L, heads
    w.emb_w = emb_w.data_ptr()
    w.emb_b = p.dev(sd[prefix + "embedding.bias"], device).data_ptr()
    w.out_w = p.dev(sd[prefix + "fc_out.weight"], device).data_ptr()
    w.out_b = p.dev(sd[prefix + "fc_out.bias"], device).data_ptr()
    w.pe = pe.data_ptr()
    w.T_max = T_max
    w.layers = C.cast(p.layers, C.POINTER(LayerWeights))
    p.struct = w
    p.d, p.J, p.L, p.heads, p.T_max = d, J, L, heads, T_max
    return p


def pack_encoder(sd: Mapping[str, Tensor], device, prefix: str, heads: int = 4, max_len: Optional[int] = None) -> _Packed:
    """Builds the ``sd_encoder_weights`` descriptor for a BaseEncoder (``prefix`` ends with '.')."""
    device = torch.device(device)
    p = _Packed()
    emb_w = p.dev(sd[prefix + "embedding.weight"], device)
    d, Cin, patch = emb_w.shape
    stem = prefix + "transformer_encoder.layers."
    L = _count_layers(sd, stem)
    p.fill_layers(sd, stem, L, device, decoder=False)
    S_max = int(max_len) if max_len is not None else 512
    pe = p.dev(positional_table(d, S_max), device)
    w = EncoderWeights()
    w.d, w.C, w.p, w.L, w.heads, w.S_max = d, Cin, patch, L, heads, S_max
    w.emb_w = emb_w.data_ptr()
    w.emb_b = p.dev(sd[prefix + "embedding.bias"], device).data_ptr()
    w.pe = pe.data_ptr()
    w.layers = C.cast(p.layers, C.POINTER(LayerWeights))
    p.struct = w
    p.d, p.C, p.p, p.L, p.heads, p.S_max = d, Cin, patch, L, heads, S_max
    return p


_ws_cache: dict = {}
_ws_retired: list = []   # buffers outgrown while their stream was capturing: the graph under capture may hold their address


def workspace(n_floats: int, device) -> Tensor:
    """Grow-only scratch buffer per (device, stream).  A buffer that is outgrown DURING a stream capture stays alive: an earlier call of the
    same capture (a context encoder, before the rollout asks for more) has put its address into the graph, and the buffer may live in the
    private pool of an older graph that no longer exists - released here, the next capture's ``empty_cache`` would return it to the driver
    and the graph would replay into unmapped memory."""
    key = (torch.device(device), _stream())
    buf = _ws_cache.get(key)
    if buf is None or buf.numel() < n_floats:
        if buf is not None and torch.cuda.is_current_stream_capturing():
            _ws_retired.append(buf)
        buf = torch.empty(int(n_floats), dtype=torch.float32, device=device)
        _ws_cache[key] = buf
    return buf


# --------------------------------------------------------------------------------------
# calls
# --------------------------------------------------------------------------------------
def denoiser_forward(packed: _Packed, x: Tensor, memory: Tensor) -> Tensor:
    """DiffusionActionGenerator.forward (reference ml/model/decoder.py:38-54)."""
    lib = _lib.load()
    _req(x, "x"); _req(memory, "memory")
    B, T, J = x.shape
    Bm, M, d = memory.shape
    if Bm != B or d != packed.d or J != packed.J:
        raise ValueError(f"shape mismatch: x {tuple(x.shape)}, memory {tuple(memory.shape)}, model d={packed.d} J={packed.J}")
    out = torch.empty_like(x)
    ws = workspace(lib.sd_workspace_floats(B, T, M, d, packed.L, 0), x.device)
    check(lib.sd_denoiser_forward(C.byref(packed.struct), x.data_ptr(), memory.data_ptr(), out.data_ptr(),
                                  ws.data_ptr(), B, T, M, _stream()), "sd_denoiser_forward")
    return out


def encoder_forward(packed: _Packed, x: Tensor) -> Tensor:
    """BaseEncoder.forward (reference ml/model/encoder/base.py:41-53)."""
    lib = _lib.load()
    _req(x, "x")
    B, S, Cin = x.shape
    if Cin != packed.C:
        raise ValueError(f"encoder expects {packed.C} input features, got {Cin}")
    n = S // packed.p
    out = torch.empty(B, n, packed.d, dtype=torch.float32, device=x.device)
    ws = workspace(lib.sd_workspace_floats(B, n, 1, packed.d, 1, 0), x.device)
    check(lib.sd_encoder_forward(C.byref(packed.struct), x.data_ptr(), out.data_ptr(), ws.data_ptr(), B, S, _stream()),
          "sd_encoder_forward")
    return out


def step_token(steps: Tensor, freq: Tensor, token: Tensor, out: Optional[Tensor] = None, row_stride: Optional[int] = None) -> Tensor:
    """StepToken.forward (reference ml/model/misc.py:25-35) -> (B, 1, d)."""
    lib = _lib.load()
    if steps.dtype not in (torch.int64, torch.float32):
        steps = steps.to(torch.int64 if not steps.is_floating_point() else torch.float32)
    _req(steps, "steps", steps.dtype); _req(freq, "freq"); _req(token, "token")
    B = steps.shape[0]
    d = token.numel() * 2
    if out is None:
        out = torch.empty(B, 1, d, dtype=torch.float32, device=steps.device)
        row_stride = d
    check(lib.sd_step_token(steps.data_ptr(), int(steps.dtype == torch.int64), freq.data_ptr(), token.data_ptr(),
                            out.data_ptr(), int(row_stride), B, d, _stream()), "sd_step_token")
    return out


def game_state_embed(idx: Tensor, table: Tensor) -> Tensor:
    """GameStateEncoder.forward (reference ml/model/encoder/game_state.py:19-27) -> (B, 1, d)."""
    lib = _lib.load()
    _req(idx, "game_state", torch.int64); _req(table, "embedding.weight")
    B = idx.shape[0]
    n, d = table.shape
    out = torch.empty(B, 1, d, dtype=torch.float32, device=idx.device)
    check(lib.sd_game_state_embed(idx.data_ptr(), table.data_ptr(), out.data_ptr(), d, B, d, n, _stream()),
          "sd_game_state_embed")
    return out


def normalize(x: Tensor, mean: Tensor, std: Tensor, inverse: bool = False) -> Tensor:
    """Normalizer.normalize / denormalize (reference dataset/pytorch.py:410-414), last dim = joints."""
    lib = _lib.load()
    _req(x, "x"); _req(mean, "mean"); _req(std, "std")
    out = torch.empty_like(x)
    check(lib.sd_normalize(x.data_ptr(), mean.data_ptr(), std.data_ptr(), out.data_ptr(), x.numel(), x.shape[-1],
                           int(inverse), _stream()), "sd_normalize")
    return out


def ddim_add_noise(x0: Tensor, noise: Tensor, t: Tensor, acp: Tensor) -> Tensor:
    """scheduler.add_noise (reference call site ml/training/train.py:218)."""
    lib = _lib.load()
    _req(x0, "x0"); _req(noise, "noise"); _req(t, "timesteps", torch.int64); _req(acp, "alphas_cumprod")
    out = torch.empty_like(x0)
    B = x0.shape[0]
    check(lib.sd_ddim_add_noise(x0.data_ptr(), noise.data_ptr(), t.data_ptr(), acp.data_ptr(), out.data_ptr(), B,
                                x0.numel() // B, _stream()), "sd_ddim_add_noise")
    return out


def ddim_step(eps: Tensor, x: Tensor, coef4) -> Tensor:
    """scheduler.step(...).prev_sample (reference call site ml/inference/plot.py:131)."""
    lib = _lib.load()
    _req(eps, "eps"); _req(x, "x")
    out = torch.empty_like(x)
    c = [float(v) for v in coef4]
    check(lib.sd_ddim_step(eps.data_ptr(), x.data_ptr(), out.data_ptr(), c[0], c[1], c[2], c[3], x.numel(), _stream()),
          "sd_ddim_step")
    return out


STATUS_NONFINITE = 1  # SD_STATUS_NONFINITE
STATUS_SHARP_LOGITS = 2  # SD_STATUS_SHARP_LOGITS (sampler mode 4: a self-attention logit beyond the validated range)


def pin_rows(rows, B: int, T: int, device) -> Tensor:
    """The pinned-row counts of ``ddim_sample(pin=(known, rows))`` as the (B,) int32 device tensor the kernels read: an int (the same
    count for every trajectory), or B of them as a sequence or a tensor.  Counts outside [0, T] raise ValueError where they can be seen
    without a read-back - an int, a sequence, a host tensor; a device tensor is converted as it is (an int32 one is used in place)."""
    if isinstance(rows, Tensor) and rows.is_cuda:
        if tuple(rows.shape) != (B,) or rows.dtype.is_floating_point or rows.dtype == torch.bool:
            raise ValueError(f"pin rows: expected ({B},) integers, got {tuple(rows.shape)} {rows.dtype}")
        return rows.to(device=device, dtype=torch.int32).contiguous()
    if isinstance(rows, bool) or (isinstance(rows, Tensor) and (rows.dtype.is_floating_point or rows.dtype == torch.bool)):
        raise ValueError(f"pin rows: expected an int or ({B},) integers, got {rows!r}")
    try:
        host = torch.full((B,), operator.index(rows), dtype=torch.int64)
    except TypeError:
        try:
            host = torch.as_tensor(rows).to(torch.int64)
        except (TypeError, ValueError, RuntimeError):
            raise ValueError(f"pin rows: expected an int or ({B},) integers, got {rows!r}") from None
    if tuple(host.shape) != (B,):
        raise ValueError(f"pin rows: expected an int or ({B},) integers, got shape {tuple(host.shape)}")
    if B and (int(host.min()) < 0 or int(host.max()) > T):
        raise ValueError(f"pin rows: every count must lie in [0, {T}] (the horizon), got {host.tolist()}")
    return host.to(torch.int32).to(device)


def _pin_req(pin, B: int, T: int, J: int, device) -> tuple:
    """(known, rows) of a pinned call, validated: known (B, T, J) fp32 on the device, rows through ``pin_rows``."""
    try:
        known, rows = pin
    except (TypeError, ValueError):
        raise ValueError("pin: expected (known, rows)") from None
    rows = pin_rows(rows, B, T, device)
    if not isinstance(known, Tensor) or tuple(known.shape) != (B, T, J):
        raise ValueError(f"pin known: expected a ({B}, {T}, {J}) tensor, got {tuple(getattr(known, 'shape', ()))}")
    _req(known, "pin known")
    if known.device != device:
        raise ValueError(f"pin known: expected a tensor on {device}, got {known.device}")
    return known, rows


def hold_mask(mask, B: int, T: int, J: int, device, rows=None) -> Tensor:
    """The element mask of ``ddim_sample(hold=(known, mask))`` as the (B, T) int32 words the kernels read: bit j of word (b, t) set =
    element (b, t, j) is held.  ``mask``: a bool tensor (B, T, J), (T, J) or (J,) - the latter two broadcast over the leading dimensions -
    or a (B, T) int32 tensor of words, which is used as it is (on ``device``).  ``rows`` (an int or (B,) counts, as ``pin_rows``): the
    leading rows[b] full rows are held as well - the composition of a pin with a hold.  ValueError for J > 32 (one word per row) or a
    wrong shape.  Bit 31 (J = 32) comes out as the sign bit of the int32 word."""
    if isinstance(J, bool) or not 1 <= int(J) <= 32:
        raise ValueError(f"hold mask: one 32-bit word per (trajectory, row) describes at most 32 joints, got J = {J}")
    B, T, J = int(B), int(T), int(J)
    if not isinstance(mask, Tensor):
        raise ValueError(f"hold mask: expected a bool tensor ({B}, {T}, {J}), ({T}, {J}) or ({J},), or ({B}, {T}) int32 words, got {type(mask).__name__}")
    if mask.dtype == torch.int32 and tuple(mask.shape) == (B, T):
        words = mask.to(device).contiguous()
    elif mask.dtype == torch.bool and tuple(mask.shape) in ((B, T, J), (T, J), (J,)):
        weights = torch.ones(J, dtype=torch.int64, device=mask.device) << torch.arange(J, dtype=torch.int64, device=mask.device)
        w64 = (mask.expand(B, T, J).to(torch.int64) * weights).sum(-1)                  # 0 .. 2^32 - 1
        words = torch.where(w64 >= 2 ** 31, w64 - 2 ** 32, w64).to(torch.int32).to(device).contiguous()   # the same 32 bits, signed
    else:
        raise ValueError(f"hold mask: expected a bool tensor ({B}, {T}, {J}), ({T}, {J}) or ({J},), or ({B}, {T}) int32 words, "
                         f"got {tuple(mask.shape)} {mask.dtype}")
    if rows is not None:
        counts = pin_rows(rows, B, T, device)
        full = -1 if J == 32 else (1 << J) - 1
        lead = torch.arange(T, device=words.device).unsqueeze(0) < counts.unsqueeze(1)
        words = torch.where(lead, words | full, words).to(torch.int32)
    return words


def _hold_req(hold, B: int, T: int, J: int, device) -> tuple:
    """(known, mask words) of a call with held elements, validated: known (B, T, J) fp32 on the device, the mask through ``hold_mask``."""
    try:
        known, mask = hold
    except (TypeError, ValueError):
        raise ValueError("hold: expected (known, mask)") from None
    words = hold_mask(mask, B, T, J, device)
    if not isinstance(known, Tensor) or tuple(known.shape) != (B, T, J):
        raise ValueError(f"hold known: expected a ({B}, {T}, {J}) tensor, got {tuple(getattr(known, 'shape', ()))}")
    _req(known, "hold known")
    if known.device != device:
        raise ValueError(f"hold known: expected a tensor on {device}, got {known.device}")
    return known, words


def _draws_req(draws, B: int, n_ctx: Optional[int]) -> int:
    """``draws`` of a sampler call, validated before any launch: an int >= 1 with ``n_ctx * draws == B`` (n_ctx None: no context rows -
    the draws then only have to divide B)."""
    if isinstance(draws, bool) or not isinstance(draws, int):
        raise ValueError(f"draws: expected an int >= 1, got {draws!r}")
    if draws < 1:
        raise ValueError(f"draws: expected an int >= 1, got {draws}")
    if B % draws:
        raise ValueError(f"draws: {B} trajectories are not a multiple of draws = {draws}")
    if n_ctx is not None and n_ctx * draws != B:
        raise ValueError(f"context shape mismatch: {n_ctx} contexts x {draws} draws != {B} trajectories")
    return draws


def _ddim_sample_native(packed: "_Packed", ctx: Optional[Tensor], step_tokens: Tensor, coef: np.ndarray, x: Tensor, tr: Optional[Tensor],
                        et: Optional[Tensor], ws: Tensor, status: Optional[Tensor], max_mode: int, pin, draws: int, hold=None, multistep=None,
                        limits=None, slew=None, accel=None):
    """The native rollout of ``ddim_sample`` and ``GraphedSampler`` on validated operands, x updated in place: always
    ``sd_ddim_sample_draws`` - with ``draws`` = 1 and NULL pin pointers it is ``sd_ddim_sample_eps``, with ``pin = (known, noise, rows)``
    ``sd_ddim_sample_pin``, launch for launch; ``hold = (known, noise, mask words)``: ``sd_ddim_sample_hold`` (never beside a pin).
    ``multistep = (w (n_steps,) fp32 on the host, history (B, T, J) on the device)``: ``sd_ddim_sample_multistep``, with ``hold`` or
    without (never beside a pin: the callers fold it into a mask).
    ``limits = (lo, hi, reproject)`` (the (32,) device arrays of ``joint_limits``): ``sd_ddim_sample_limits``, with ``multistep`` and
    ``hold`` or without either (never beside a pin).
    ``slew = (v, start or None)`` (needs ``limits``, which may all be infinite): ``sd_ddim_sample_slew``.
    ``accel = (a, start2 or None)`` (needs ``slew``, whose ``v`` may all be infinite): ``sd_ddim_sample_accel``.
    Returns x, or (x, trace?, eps_trace?) where those buffers were given."""
    B, T, _ = x.shape
    if accel is not None:
        msw, hist = multistep if multistep is not None else (None, None)
        check(_lib.load().sd_ddim_sample_accel(C.byref(packed.struct), _ptr(ctx), step_tokens.data_ptr(), coef.ctypes.data_as(_lib.c_float_p),
                                               x.data_ptr(), _ptr(tr), _ptr(et), ws.data_ptr(), B, T, 0 if ctx is None else ctx.shape[1],
                                               len(coef), _ptr(status), int(max_mode), *[_ptr(t) for t in (hold or (None, None, None))], draws,
                                               None if msw is None else msw.ctypes.data_as(_lib.c_float_p), _ptr(hist),
                                               limits[0].data_ptr(), limits[1].data_ptr(), int(bool(limits[2])), slew[0].data_ptr(), _ptr(slew[1]),
                                               accel[0].data_ptr(), _ptr(accel[1]), _stream()),
              "sd_ddim_sample_accel")
        out = (x,) + tuple(t for t in (tr, et) if t is not None)
        return out if len(out) > 1 else x
    if slew is not None:
        msw, hist = multistep if multistep is not None else (None, None)
        check(_lib.load().sd_ddim_sample_slew(C.byref(packed.struct), _ptr(ctx), step_tokens.data_ptr(), coef.ctypes.data_as(_lib.c_float_p),
                                              x.data_ptr(), _ptr(tr), _ptr(et), ws.data_ptr(), B, T, 0 if ctx is None else ctx.shape[1],
                                              len(coef), _ptr(status), int(max_mode), *[_ptr(t) for t in (hold or (None, None, None))], draws,
                                              None if msw is None else msw.ctypes.data_as(_lib.c_float_p), _ptr(hist),
                                              limits[0].data_ptr(), limits[1].data_ptr(), int(bool(limits[2])), slew[0].data_ptr(), _ptr(slew[1]),
                                              _stream()),
              "sd_ddim_sample_slew")
        out = (x,) + tuple(t for t in (tr, et) if t is not None)
        return out if len(out) > 1 else x
    if limits is not None:
        msw, hist = multistep if multistep is not None else (None, None)
        check(_lib.load().sd_ddim_sample_limits(C.byref(packed.struct), _ptr(ctx), step_tokens.data_ptr(), coef.ctypes.data_as(_lib.c_float_p),
                                                x.data_ptr(), _ptr(tr), _ptr(et), ws.data_ptr(), B, T, 0 if ctx is None else ctx.shape[1],
                                                len(coef), _ptr(status), int(max_mode), *[_ptr(t) for t in (hold or (None, None, None))], draws,
                                                None if msw is None else msw.ctypes.data_as(_lib.c_float_p), _ptr(hist),
                                                limits[0].data_ptr(), limits[1].data_ptr(), int(bool(limits[2])), _stream()),
              "sd_ddim_sample_limits")
        out = (x,) + tuple(t for t in (tr, et) if t is not None)
        return out if len(out) > 1 else x
    if multistep is not None:
        msw, hist = multistep
        check(_lib.load().sd_ddim_sample_multistep(C.byref(packed.struct), _ptr(ctx), step_tokens.data_ptr(), coef.ctypes.data_as(_lib.c_float_p),
                                                   x.data_ptr(), _ptr(tr), _ptr(et), ws.data_ptr(), B, T, 0 if ctx is None else ctx.shape[1],
                                                   len(coef), _ptr(status), int(max_mode), *[_ptr(t) for t in (hold or (None, None, None))], draws,
                                                   msw.ctypes.data_as(_lib.c_float_p), hist.data_ptr(), _stream()),
              "sd_ddim_sample_multistep")
        out = (x,) + tuple(t for t in (tr, et) if t is not None)
        return out if len(out) > 1 else x
    if hold is not None:
        check(_lib.load().sd_ddim_sample_hold(C.byref(packed.struct), _ptr(ctx), step_tokens.data_ptr(), coef.ctypes.data_as(_lib.c_float_p),
                                              x.data_ptr(), _ptr(tr), _ptr(et), ws.data_ptr(), B, T, 0 if ctx is None else ctx.shape[1], len(coef),
                                              _ptr(status), int(max_mode), *[_ptr(t) for t in hold], draws, _stream()),
              "sd_ddim_sample_hold")
        out = (x,) + tuple(t for t in (tr, et) if t is not None)
        return out if len(out) > 1 else x
    check(_lib.load().sd_ddim_sample_draws(C.byref(packed.struct), _ptr(ctx), step_tokens.data_ptr(), coef.ctypes.data_as(_lib.c_float_p),
                                           x.data_ptr(), _ptr(tr), _ptr(et), ws.data_ptr(), B, T, 0 if ctx is None else ctx.shape[1], len(coef),
                                           _ptr(status), int(max_mode), *[_ptr(t) for t in (pin or (None, None, None))], draws, _stream()),
          "sd_ddim_sample_draws")
    out = (x,) + tuple(t for t in (tr, et) if t is not None)
    return out if len(out) > 1 else x


class GraphedSampler:
    """The whole rollout (n_steps x (L x 2 + 3) kernel launches of ``sd_ddim_sample``) captured
    once into a hipGraph and replayed: removes the per-launch host cost, which dominates at
    small batch (the robot's B = 1, 30-step rollout).  Static shapes; the inputs are copied
    into the captured buffers before every replay.  ``status`` (one int32 on the device) is
    the range-guard word of ``sd_ddim_sample_ex``, rewritten by every replay.  ``pin=True`` captures the pinned call on static
    pin buffers (known rows, start noise, row counts): a replay copies the call's ``pin=(known, rows)`` into them, so one graph
    serves every pinning, none (rows = 0) included.  ``draws`` > 1: the context buffer holds B / draws contexts, trajectory b reads
    context b // draws.  ``hold=True`` captures the call with held elements (``sd_ddim_sample_hold``) on static known, noise and mask
    buffers: a replay copies the call's ``hold=(known, mask)`` into them, so one graph serves every mask, the empty one included; not
    together with ``pin`` (compose them through ``hold_mask(rows=...)``).  ``multistep=w`` (``multistep_weights``) captures the
    second-order multistep rollout (``sd_ddim_sample_multistep``) on a static history buffer, which no replay needs cleared: its first
    step does not read it.  With ``pin=True`` the pin is folded into a mask (J <= 32): the graph is captured on hold buffers and a replay's
    ``pin=(known, rows)`` becomes ``hold_mask(rows=rows)``.  ``limits=True`` captures the call under per-joint limits
    (``sd_ddim_sample_limits``, ``reproject`` fixed at capture) on two static (32,) arrays, ``self.limits``, which the kernels read on the
    device at every step: they start unlimited, ``set_limits`` rewrites them in place and the captured rollout stays captured; a pin is
    folded into a mask as under ``multistep``.  ``slew=True`` captures the call under per-joint slew limits (``sd_ddim_sample_slew``) on a
    static (32,) array ``self.slew_v`` (all +inf at first) and a static (B, 32) array ``self.slew_start`` (all NaN at first), read on the
    device at every step: ``set_slew`` rewrites them in place.  It implies the limit arrays, which stay infinite unless ``set_limits`` is
    called.  ``accel=True`` captures the call under per-joint acceleration limits (``sd_ddim_sample_accel``) on a static (32,) array
    ``self.accel_a`` (all +inf at first) and a static (B, 32) array ``self.accel_start2`` (all NaN at first): ``set_accel`` rewrites them
    in place and keeps the capture.  It implies the slew and limit arrays.  (One native call for all of them: ``_ddim_sample_native``.)"""

    def __init__(self, packed: _Packed, B: int, T: int, Mc: int, step_tokens: Tensor, coef: np.ndarray, max_mode: int = -1, pin: bool = False,
                 draws: int = 1, hold: bool = False, multistep=None, limits: bool = False, reproject: bool = False, slew: bool = False,
                 accel: bool = False):
        dev = step_tokens.device
        slew = bool(slew) or bool(accel)
        limits = bool(limits) or bool(slew)
        if pin and hold:
            raise ValueError("GraphedSampler: pin and hold exclude each other - compose them through ops.hold_mask(rows=...)")
        self.multistep = None if multistep is None else _multistep_req(multistep, len(coef))
        self.limits, self.reproject = (joint_limits({}, J=packed.J, device=dev) if limits else None), bool(reproject)
        self.slew_v = joint_slew({}, J=packed.J, device=dev) if slew else None
        self.slew_start = torch.full((B, 32), float("nan"), dtype=torch.float32, device=dev) if slew else None
        self.accel_a = joint_accel({}, J=packed.J, device=dev) if accel else None
        self.accel_start2 = torch.full((B, 32), float("nan"), dtype=torch.float32, device=dev) if accel else None
        self.pin_as_hold = bool(pin) and (self.multistep is not None or self.limits is not None)
        if self.pin_as_hold:
            pin, hold = False, True
        self.draws = _draws_req(draws, B, None)
        self.packed, self.coef = packed, np.ascontiguousarray(coef, dtype=np.float32)
        self.tokens = step_tokens.contiguous()
        self.max_mode = int(max_mode)
        self.x = torch.zeros(B, T, packed.J, dtype=torch.float32, device=dev)
        self.ctx = torch.zeros(B // self.draws, Mc, packed.d, dtype=torch.float32, device=dev) if Mc > 0 else None
        self.status = torch.zeros(1, dtype=torch.int32, device=dev)
        self.pin = None
        if pin:   # (known, noise, rows)
            self.pin = (torch.zeros_like(self.x), torch.zeros_like(self.x), torch.zeros(B, dtype=torch.int32, device=dev))
        self.hold = None
        if hold:   # (known, noise, mask words)
            if packed.J > 32:
                raise ValueError(f"hold: one 32-bit mask word per row describes at most 32 joints, got J = {packed.J}")
            self.hold = (torch.zeros_like(self.x), torch.zeros_like(self.x), torch.zeros(B, T, dtype=torch.int32, device=dev))
        self.hist = torch.empty_like(self.x) if self.multistep is not None else None
        lib = _lib.load()
        self.ws = torch.empty(lib.sd_workspace_floats(B, T, max(Mc, 1), packed.d, packed.L, len(self.coef)),
                              dtype=torch.float32, device=dev)
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            self._run()  # warm-up outside capture: lazy module load and LDS attributes happen here
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self._run()

    def _run(self):
        _ddim_sample_native(self.packed, self.ctx, self.tokens, self.coef, self.x, None, None, self.ws, self.status, self.max_mode, self.pin, self.draws,
                            self.hold, None if self.multistep is None else (self.multistep, self.hist),
                            None if self.limits is None else (self.limits.lo, self.limits.hi, self.reproject),
                            None if self.slew_v is None else (self.slew_v, self.slew_start),
                            None if self.accel_a is None else (self.accel_a, self.accel_start2))

    def set_accel(self, accel) -> None:
        """Rewrites the captured acceleration arrays in place (``accel`` as ``ddim_sample`` takes it: ``a`` or ``(a, start2)``; without
        ``start2`` the second anchors go back to NaN): every later replay runs under them."""
        if self.accel_a is None:
            raise ValueError("GraphedSampler: set_accel needs a graph captured with accel=True")
        a, start2 = _accel_req(accel, self.x.shape[0], self.packed.J, self.x.device)
        self.accel_a.copy_(a)
        if start2 is None:
            self.accel_start2.fill_(float("nan"))
        else:
            self.accel_start2.copy_(start2)

    def set_slew(self, slew) -> None:
        """Rewrites the captured slew arrays in place (``slew`` as ``ddim_sample`` takes it: ``v`` or ``(v, start)``; without ``start``
        the anchors go back to NaN): every later replay runs under them."""
        if self.slew_v is None:
            raise ValueError("GraphedSampler: set_slew needs a graph captured with slew=True")
        v, start = _slew_req(slew, self.x.shape[0], self.packed.J, self.x.device)
        self.slew_v.copy_(v)
        if start is None:
            self.slew_start.fill_(float("nan"))
        else:
            self.slew_start.copy_(start)

    def set_limits(self, limits) -> None:
        """Rewrites the captured limit arrays in place (``limits`` as ``ddim_sample`` takes it): every later replay runs under them."""
        if self.limits is None:
            raise ValueError("GraphedSampler: set_limits needs a graph captured with limits=True")
        new = _limits_req(limits, self.packed.J, self.x.device)
        self.limits.lo.copy_(new.lo)
        self.limits.hi.copy_(new.hi)

    def replay_into(self, ctx: Optional[Tensor], x_T: Tensor, pin=None, hold=None) -> Tensor:
        """Copies the inputs into the captured buffers, replays, and returns the captured x buffer itself
        (overwritten by the next replay)."""
        if self.pin_as_hold:   # a multistep or limits graph captured with pin=True: the pin as a mask
            if pin is None or hold is not None:
                raise ValueError("GraphedSampler: a graph captured with pin=True takes pin=(known, rows) at every call, one without takes none")
            known, rows = _pin_req(pin, *self.x.shape, self.x.device)
            B, T, J = self.x.shape
            pin, hold = None, (known, hold_mask(torch.zeros(J, dtype=torch.bool, device=self.x.device), B, T, J, self.x.device, rows=rows))
        if (pin is None) != (self.pin is None):
            raise ValueError("GraphedSampler: a graph captured with pin=True takes pin=(known, rows) at every call, one without takes none")
        if (hold is None) != (self.hold is None):
            raise ValueError("GraphedSampler: a graph captured with hold=True takes hold=(known, mask) at every call, one without takes none")
        if self.ctx is not None and tuple(ctx.shape) != tuple(self.ctx.shape):
            raise ValueError(f"context shape mismatch: expected {tuple(self.ctx.shape)} ({self.draws} draws per context), got {tuple(ctx.shape)}")
        self.x.copy_(x_T)
        if self.ctx is not None:
            self.ctx.copy_(ctx)
        if pin is not None:
            known, rows = _pin_req(pin, *self.x.shape, self.x.device)
            self.pin[0].copy_(known)
            self.pin[1].copy_(x_T)
            self.pin[2].copy_(rows)
        if hold is not None:
            known, words = _hold_req(hold, *self.x.shape, self.x.device)
            self.hold[0].copy_(known)
            self.hold[1].copy_(x_T)
            self.hold[2].copy_(words)
        self.graph.replay()
        return self.x

    def __call__(self, ctx: Optional[Tensor], x_T: Tensor, pin=None, hold=None) -> Tensor:
        return self.replay_into(ctx, x_T, pin, hold).clone()


def ddim_sample(packed: _Packed, ctx: Optional[Tensor], step_tokens: Tensor, coef: np.ndarray, x_T: Tensor,
                trace: bool = False, inplace: bool = False, status: Optional[Tensor] = None, max_mode: int = -1,
                eps_trace: bool = False, pin=None, draws: int = 1, hold=None, multistep=None, limits=None, reproject: bool = False,
                slew=None, accel=None):
    """The reference's sampling loop (ml/inference/plot.py:122-131, ml/training/distill.py:179-189)
    as ONE native call.  Returns the sample, or (sample, per-step trace) when ``trace``; with ``eps_trace`` the
    noise prediction of every step (n_steps, B, T, J) - the value of ``forward_with_context`` inside the loop - is
    appended to the returned tuple.
    ``status`` (int32 tensor of one element on the device) receives the range-guard word of
    ``sd_ddim_sample_ex`` - not read here, so the call stays asynchronous; ``max_mode`` caps the kernel selection
    (see ``ddim_sample_guarded``).
    ``pin = (known, rows)``: conditioning by inpainting (``sd_ddim_sample_pin``).  ``known`` (B, T, J) in normalised space; ``rows`` an
    int or (B,) counts (``pin_rows``): row t of trajectory b is held to ``known`` iff t < rows[b] - on entry c0[0] known + c1[0] x_T,
    after step i c2[i] known + c3[i] x_T in place of the DDIM update, so the returned rows equal ``known`` exactly; every other row is
    sampled to fit, reading the pinned ones through self-attention.  The noise of the pinned rows is ``x_T`` itself (with ``inplace``
    a private copy of it is taken first).  ``max_mode`` 4 runs the mode-3 kernels.  ``pin=None`` is the call without any of this.
    ``draws`` = G > 1: several draws per observation (``sd_ddim_sample_draws``).  ``ctx`` is (B / G, Mc, d) and trajectory b reads context
    b // G: the context is projected and folded once per context and the G draws share its planes - bit for bit the result of the call with
    ``ctx.repeat_interleave(G, 0)``, without the G copies.  Everything else (``x_T``, the traces, ``pin``, ``status``) stays per trajectory.
    ``hold = (known, mask)``: the element form of the pin (``sd_ddim_sample_hold``) - ``mask`` as ``hold_mask`` takes it: element (b, t, j)
    is held to ``known`` iff its bit is set, with the pin's coefficients and the pin's exactness at the last step; every other element is
    sampled to fit.  J <= 32.  ``pin`` and ``hold`` together raise ValueError: ``hold_mask(mask, ..., rows=rows)`` composes them.  The
    trajectory routes run one hold kernel per step for any ``draws``.
    ``multistep = w`` (``multistep_weights``: (n_steps,) fp32, w[0] == 0): the second-order multistep solver (``sd_ddim_sample_multistep``) -
    after the DDIM update of step i, ``x += w[i] * (x0[i - 1] - x0[i])``; no extra denoiser evaluation, and all zeros is DDIM.  It composes
    with everything above; a ``pin`` is folded into ``hold_mask(rows=rows)`` for this call (J <= 32).  The trajectory routes run one
    multistep kernel per step (no fused rollout form).
    ``limits = (lo, hi)``, a range r, ``{joint: (lo, hi)}`` or ``joint_limits(...)``: per-joint limits in normalised space
    (``sd_ddim_sample_limits``; diffusers' ``clip_sample``, per joint) - at every step the predicted clean trajectory x0 is clamped to
    [lo[j], hi[j]] before the update is formed from it, in the lane that holds it, so the last step returns every free element bitwise
    inside the limits; a NaN stays NaN.  ``reproject`` (diffusers' ``use_clipped_model_output``): a clamped element's eps is recomputed
    from the clamped x0.  Held elements keep the hold's value whatever the limits say; ``eps_trace`` stays the network's prediction.  It
    composes with everything above (a ``pin`` is folded into a mask: J <= 32); infinite limits are the multistep call bit for bit.  One
    limits kernel per step on the trajectory routes (no fused rollout form).
    ``slew = v`` or ``(v, start)`` (``joint_slew``'s forms; ``start`` (B, J) or (B, 32), NaN: none): per-joint slew limits in normalised
    space (``sd_ddim_sample_slew``) - at every step, consecutive rows of the predicted clean trajectory are kept within ``v[j]`` of each
    other by a scan over the rows t = 0 .. T - 1 (row 0 against ``start``), then clamped to ``limits`` (optional beside it; the box always
    wins), before the update is formed.  A held element enters the scan as the hold's value: a jump into it is the caller's business.
    Every free element of the result lies bitwise within ``fl(p +- v)`` of a predecessor p inside the box.  It composes with everything
    above; infinite ``v`` without ``start`` is the ``limits=`` call bit for bit.  One slew kernel per step on the trajectory routes (the
    limits twins around the scan, x0 exchanged through LDS; no fused rollout form); behind the row-panel routes one scan kernel, a thread
    per trajectory and joint.
    ``accel = a`` or ``(a, start2)`` (``joint_accel``'s forms; ``start2`` (B, J) or (B, 32), NaN: none): per-joint acceleration limits in
    normalised space (``sd_ddim_sample_accel``) - the scan carries the two rows before (row -1 is ``slew``'s ``start``, row -2 is
    ``start2``) and keeps row t within ``a[j]`` of their constant-velocity continuation ``fl(y1 + fl(y1 - y2))``, then applies the slew
    interval, the box and the hold as above: the box wins over the slew limit, which wins over the acceleration limit.  A missing or NaN
    predecessor limits nothing.  ``slew`` and ``limits`` are optional beside it.  There is no braking ahead of the box - where the box or
    the slew interval wins, the second difference at that row can exceed ``a`` - and without a box or a slew limit the velocity can
    accumulate and the scan can run away from the prediction.  Infinite ``a`` without ``start2`` is the ``slew=`` call bit for bit.  One
    acceleration kernel per step on the trajectory routes (the slew twins with two rows of state); ``max_mode`` 4 runs the mode-3 kernels."""
    draws = _draws_req(draws, x_T.shape[0], None if ctx is None else ctx.shape[0])   # (shapes only: before anything touches a device)
    if pin is not None and hold is not None:
        raise ValueError("pin and hold exclude each other: compose them through ops.hold_mask(mask, B, T, J, device, rows=rows)")
    if multistep is not None:   # (likewise)
        multistep = _multistep_req(multistep, step_tokens.shape[0])
    lib = _lib.load()
    _req(x_T, "x_T"); _req(step_tokens, "step_tokens")
    B, T, J = x_T.shape
    n_steps = step_tokens.shape[0]
    Mc = 0
    if ctx is not None:
        _req(ctx, "context")
        Mc = ctx.shape[1]
        if ctx.shape[0] * draws != B or ctx.shape[2] != packed.d:
            raise ValueError("context shape mismatch")
    coef = np.ascontiguousarray(coef, dtype=np.float32)
    if coef.shape != (n_steps, 4):
        raise ValueError("coef must be (n_steps, 4)")
    if status is not None:
        _req(status, "status", torch.int32)
    if pin is not None:
        pin = _pin_req(pin, B, T, J, x_T.device)
        if multistep is not None or limits is not None or slew is not None or accel is not None:   # these kernels take a mask: the pin as its leading full rows
            hold, pin = (pin[0], hold_mask(torch.zeros(J, dtype=torch.bool, device=x_T.device), B, T, J, x_T.device, rows=pin[1])), None
    if hold is not None:
        hold = _hold_req(hold, B, T, J, x_T.device)
    if accel is not None:
        accel = _accel_req(accel, B, J, x_T.device)
        slew = {} if slew is None else slew
    if slew is not None:
        slew = _slew_req(slew, B, J, x_T.device)
        limits = {} if limits is None else limits
    if limits is not None:
        limits = _limits_req(limits, J, x_T.device)
        limits = (limits.lo, limits.hi, bool(reproject))
    x = x_T if inplace else x_T.clone()
    tr = torch.empty(n_steps, B, T, J, dtype=torch.float32, device=x.device) if trace else None
    et = torch.empty(n_steps, B, T, J, dtype=torch.float32, device=x.device) if eps_trace else None
    ws = workspace(lib.sd_workspace_floats(B, T, max(Mc, 1), packed.d, packed.L, n_steps), x.device)
    if pin is not None:   # (known, noise, rows); the noise never x itself: the first step overwrites x
        pin = (pin[0], x_T.clone() if inplace else x_T, pin[1])
    if hold is not None:   # (known, noise, mask words), the noise as the pin's
        hold = (hold[0], x_T.clone() if inplace else x_T, hold[1])
    if multistep is not None:   # (weights, history): the history is written before it is read - no clearing
        multistep = (multistep, torch.empty_like(x))
    return _ddim_sample_native(packed, ctx, step_tokens, coef, x, tr, et, ws, status, max_mode, pin, draws, hold, multistep, limits, slew, accel)


def default_sampler_cap() -> int:
    """The highest sampler mode a call runs unless told otherwise: 3 - three fp16 products at every site, valid for any weights.
    Mode 4 (two products at the Q | K | V projection, guarded by SD_STATUS_SHARP_LOGITS) is opt-in: ``max_mode=4`` at the call
    (``End2EndDiffusionTransformer.sample(..., max_mode=4)``) or ``SD_SAMPLER_MODE=4`` in the environment."""
    import os

    try:
        cap = int(os.environ.get("SD_SAMPLER_MODE", "3"))
    except ValueError:
        cap = 3
    return cap if 0 <= cap <= 4 else 3


def sampler_cap(packed: _Packed, max_mode: Optional[int] = None) -> int:
    """``max_mode`` of a call: the caller's (or the default), lowered to 3 once these weights tripped mode 4's guard."""
    cap = default_sampler_cap() if max_mode is None else int(max_mode)
    return min(cap, getattr(packed, "sampler_cap", 4))


def ddim_sample_guarded(packed: _Packed, ctx: Optional[Tensor], step_tokens: Tensor, coef: np.ndarray, x_T: Tensor,
                        trace: bool = False, max_mode: Optional[int] = None, pin=None, draws: int = 1, hold=None, multistep=None,
                        limits=None, reproject: bool = False, slew=None, accel=None):
    """``ddim_sample`` with the range guard read back (one host synchronisation): when the split-fp16 kernels of
    sampler modes 2 .. 4 were driven out of their operand range (|8 v| >= 65520 for a LayerNorm / attention / GELU output -
    e.g. a checkpoint with LayerNorm weights in the thousands), the rollout is repeated on the exact-fp32 MFMA kernels
    (``max_mode`` 1), which have no such limit.  Raises if that result is not finite either (non-finite inputs).
    ``max_mode``: None = ``default_sampler_cap()`` (3).  With 4, mode 4's own guard (SD_STATUS_SHARP_LOGITS: a self-attention logit
    beyond the range its two-product Q | K | V site is validated on) repeats the rollout on mode 3 and pins ``packed.sampler_cap`` there.
    ``pin``, ``hold``, ``draws``, ``multistep``, ``limits``, ``reproject``, ``slew`` and ``accel``: as in ``ddim_sample``; every repeat carries them (the rerun at ``max_mode`` 1 expands the context
    rows: correct, not shared; a repeat restarts from ``x_T``, so the multistep history needs nothing more)."""
    import warnings

    draws = _draws_req(draws, x_T.shape[0], None if ctx is None else ctx.shape[0])
    if pin is not None and hold is not None:
        raise ValueError("pin and hold exclude each other: compose them through ops.hold_mask(mask, B, T, J, device, rows=rows)")
    if pin is not None:   # validated and uploaded once for all repeats
        pin = _pin_req(pin, *x_T.shape, x_T.device)
    if hold is not None:
        hold = _hold_req(hold, *x_T.shape, x_T.device)
    if multistep is not None:
        multistep = _multistep_req(multistep, step_tokens.shape[0])
    if limits is not None:
        limits = _limits_req(limits, x_T.shape[2], x_T.device)
    if slew is not None:
        slew = _slew_req(slew, x_T.shape[0], x_T.shape[2], x_T.device)
    if accel is not None:
        accel = _accel_req(accel, x_T.shape[0], x_T.shape[2], x_T.device)
    status = torch.zeros(1, dtype=torch.int32, device=x_T.device)
    cap = sampler_cap(packed, max_mode)
    out = ddim_sample(packed, ctx, step_tokens, coef, x_T, trace=trace, status=status, max_mode=cap, pin=pin, draws=draws, hold=hold, multistep=multistep,
                      limits=limits, reproject=reproject, slew=slew, accel=accel)
    word = int(status.item())
    if word == 0:
        return out
    if word & STATUS_SHARP_LOGITS:
        # sampler mode 4 met a self-attention logit beyond the range its two-product Q | K | V projection is validated on
        # (SD_SHARP_LOGIT_LIMIT): the same rollout with three fp16 products at every site (mode 3).  Sharpness is a property
        # of the checkpoint, so later calls with these weights start there.
        packed.sampler_cap = 3
        if not word & STATUS_NONFINITE:
            out = ddim_sample(packed, ctx, step_tokens, coef, x_T, trace=trace, status=status, max_mode=3, pin=pin, draws=draws, hold=hold, multistep=multistep,
                              limits=limits, reproject=reproject, slew=slew, accel=accel)
            if int(status.item()) == 0:
                return out
    mode = _lib.load().sd_sampler_mode(packed.d, packed.heads, x_T.shape[1], 0 if ctx is None else ctx.shape[1], packed.J)
    if mode < 2 and _chain16_possible(packed):
        mode = 2   # the unfused row chains run on the split-fp16 pipe as well
    if mode >= 2:
        warnings.warn("sd_ddim_sample: the split-fp16 kernels left their operand range (non-finite sample); "
                      "repeating the rollout on the fp32-MFMA kernels", RuntimeWarning, stacklevel=2)
        out = ddim_sample(packed, ctx, step_tokens, coef, x_T, trace=trace, status=status, max_mode=1, pin=pin, draws=draws, hold=hold, multistep=multistep,
                          limits=limits, reproject=reproject, slew=slew, accel=accel)
        if int(status.item()) == 0:
            return out
    raise FloatingPointError("sd_ddim_sample produced non-finite values on the fp32 kernels too: the inputs or the weights are not finite")


_NO_LIMITS: dict = {}


def _no_limits(J: int, device) -> Limits:
    """The infinite limit arrays of a direct call without ``limits`` (the kernels always read a box), uploaded once per (J, device): a
    captured tick must not upload anything."""
    key = (int(J), torch.device(device))
    if key not in _NO_LIMITS:
        _NO_LIMITS[key] = joint_limits({}, J=J, device=device)
    return _NO_LIMITS[key]


def _direct_req(x_shape, device, hold, limits, slew) -> tuple:
    """(known, mask words, lo, hi, v, start) of a direct call, validated: ``hold``, ``limits`` and ``slew`` in ``ddim_sample``'s forms."""
    B, T, J = x_shape
    known, words = (None, None) if hold is None else _hold_req(hold, B, T, J, device)
    v, start = (None, None) if slew is None else _slew_req(slew, B, J, device)
    lim = _no_limits(J, device) if limits is None else _limits_req(limits, J, device)
    return known, words, lim.lo, lim.hi, v, start


def direct_sample(packed: _Packed, ctx: Optional[Tensor], token: Tensor, x_T: Tensor, hold=None, limits=None, slew=None, draws: int = 1,
                  raw: bool = False, status: Optional[Tensor] = None, max_mode: int = 3, accel=None):
    """A distilled one-step decoder under the guarantees of ``ddim_sample`` (``sd_direct_sample``): the network's output at the ONE step
    token ``token`` ((d,) or (1, d): the token of t = 0, ros.py:293-298) is the clean trajectory x0 itself, so the result is that
    prediction projected - ``hold = (known, mask)``, then the slew scan ``slew = v`` or ``(v, start)`` over the rows, then the box
    ``limits``, each as ``ddim_sample`` takes and defines it for the predicted x0 of a rollout (whose last step returns the clamped x0
    itself; a one-step model is that last step alone).  ``x_T`` (B, T, J), the start noise, is only read.  ``draws`` = G: ``ctx`` holds
    B / G contexts, prepared once each; G noises give G different trajectories.  Returns the projected sample, or ``(sample, raw)`` with
    ``raw=True``: ``raw`` is the unprojected prediction - ``forward_with_context(ctx, x_T, zeros)`` bit for bit.  With nothing set the
    sample is ``raw`` bit for bit, -0 included; a NaN prediction stays NaN and limits nothing after it; every free element lies bitwise
    inside ``limits`` and within ``fl(p +- v)`` of its predecessor p.  On the trajectory routes this is ONE launch of a direct twin of
    the step kernels; on the others (``max_mode`` < 3, or a shape without trajectory kernels) the eps launches and one projection
    launch.  ``status`` as in ``ddim_sample`` (not read here).  There is no ``pin``, no ``multistep`` and no ``reproject``: one step has
    no free rows that could adapt to pinned ones, no history and no eps to recompute.
    ``accel = a`` or ``(a, start2)``: acceleration limits as ``ddim_sample`` defines them.  The call is then TWO launches on every route:
    the plain direct launch with nothing set, which returns ``raw``, then ``direct_project(raw, ..., accel=)`` (there is no fused
    direct twin: the fused launch measured no faster than launch + projection at the robot's T = 10, profiles/direct_bench.jsonl), in one
    native call (``sd_direct_sample_accel``).  The status word tells of the projected sample."""
    draws = _draws_req(draws, x_T.shape[0], None if ctx is None else ctx.shape[0])
    lib = _lib.load()
    _req(x_T, "x_T"); _req(token, "token")
    if x_T.dim() != 3:
        raise ValueError("x_T: expected (B, T, J)")
    B, T, J = x_T.shape
    if token.numel() != packed.d:
        raise ValueError(f"token: expected ONE step token of {packed.d} floats, got {tuple(token.shape)}")
    Mc = 0
    if ctx is not None:
        _req(ctx, "context")
        Mc = ctx.shape[1]
        if ctx.shape[0] * draws != B or ctx.shape[2] != packed.d:
            raise ValueError("context shape mismatch")
    if status is not None:
        _req(status, "status", torch.int32)
    known, words, lo, hi, v, start = _direct_req((B, T, J), x_T.device, hold, limits, slew)
    if accel is not None:   # sd_direct_sample_accel: the plain launch, which returns raw, then the projection
        a, start2 = _accel_req(accel, B, J, x_T.device)
        out, pred = torch.empty_like(x_T), torch.empty_like(x_T)
        ws = workspace(lib.sd_workspace_floats(B, T, max(Mc, 1), packed.d, packed.L, 1), x_T.device)
        check(lib.sd_direct_sample_accel(C.byref(packed.struct), _ptr(ctx), token.data_ptr(), x_T.data_ptr(), out.data_ptr(), pred.data_ptr(), ws.data_ptr(),
                                         B, T, Mc, _ptr(status), int(max_mode), _ptr(known), _ptr(words), draws, lo.data_ptr(), hi.data_ptr(), _ptr(v),
                                         _ptr(start), a.data_ptr(), _ptr(start2), _stream()), "sd_direct_sample_accel")
        return (out, pred) if raw else out
    out = torch.empty_like(x_T)
    pred = torch.empty_like(x_T) if raw else None
    ws = workspace(lib.sd_workspace_floats(B, T, max(Mc, 1), packed.d, packed.L, 1), x_T.device)
    check(lib.sd_direct_sample(C.byref(packed.struct), _ptr(ctx), token.data_ptr(), x_T.data_ptr(), out.data_ptr(), _ptr(pred), ws.data_ptr(), B, T, Mc,
                               _ptr(status), int(max_mode), _ptr(known), _ptr(words), draws, lo.data_ptr(), hi.data_ptr(), _ptr(v), _ptr(start),
                               _stream()), "sd_direct_sample")
    return (out, pred) if raw else out


def direct_sample_guarded(packed: _Packed, ctx: Optional[Tensor], token: Tensor, x_T: Tensor, hold=None, limits=None, slew=None, draws: int = 1,
                          raw: bool = False, max_mode: Optional[int] = None, accel=None):
    """``direct_sample`` with the range guard read back (one host synchronisation), as ``ddim_sample_guarded``: a non-finite result on
    the split-fp16 kernels is repeated on the exact-fp32 MFMA kernels (``max_mode`` 1: the eps launches, then the projection launch),
    with the same ``hold``, ``limits``, ``slew`` and ``draws``; FloatingPointError if that is not finite either.  ``max_mode`` None: the
    default cap (mode 4 has no direct twin and runs as 3)."""
    import warnings

    draws = _draws_req(draws, x_T.shape[0], None if ctx is None else ctx.shape[0])
    B, T, J = x_T.shape
    if hold is not None:   # validated and uploaded once for both runs
        hold = _hold_req(hold, B, T, J, x_T.device)
    if limits is not None:
        limits = _limits_req(limits, J, x_T.device)
    if slew is not None:
        slew = _slew_req(slew, B, J, x_T.device)
    if accel is not None:
        accel = _accel_req(accel, B, J, x_T.device)
    status = torch.zeros(1, dtype=torch.int32, device=x_T.device)
    cap = min(sampler_cap(packed, max_mode), 3)
    out = direct_sample(packed, ctx, token, x_T, hold=hold, limits=limits, slew=slew, draws=draws, raw=raw, status=status, max_mode=cap, accel=accel)
    if int(status.item()) == 0:
        return out
    if cap >= 2:
        warnings.warn("sd_direct_sample: the split-fp16 kernels left their operand range (non-finite sample); "
                      "repeating the call on the fp32-MFMA kernels", RuntimeWarning, stacklevel=2)
        out = direct_sample(packed, ctx, token, x_T, hold=hold, limits=limits, slew=slew, draws=draws, raw=raw, status=status, max_mode=1, accel=accel)
        if int(status.item()) == 0:
            return out
    raise FloatingPointError("sd_direct_sample produced non-finite values on the fp32 kernels too: the inputs or the weights are not finite")


def direct_project(raw: Tensor, hold=None, limits=None, slew=None, accel=None) -> Tensor:
    """The projection of ``direct_sample`` on its own (``sd_direct_project``): ``raw`` (B, T, J) - a predicted clean trajectory from
    anywhere - under ``hold = (known, mask)``, the slew scan ``slew = v`` or ``(v, start)`` and the box ``limits``, in ``ddim_sample``'s
    forms; a new tensor.  Compares and selects, one fp32 add and one subtract per row: -0 stays -0, a NaN stays NaN and limits nothing
    after it, an infinite prediction comes out as its limit.  ``accel = a`` or ``(a, start2)``: the acceleration scan of
    ``ddim_sample(accel=...)`` ahead of the slew interval (``sd_direct_project_accel``)."""
    lib = _lib.load()
    _req(raw, "raw")
    if raw.dim() != 3:
        raise ValueError("direct_project: raw must be a whole (B, T, J) sample")
    B, T, J = raw.shape
    known, words, lo, hi, v, start = _direct_req((B, T, J), raw.device, hold, limits, slew)
    out = torch.empty_like(raw)
    if accel is not None:
        a, start2 = _accel_req(accel, B, J, raw.device)
        check(lib.sd_direct_project_accel(raw.data_ptr(), out.data_ptr(), _ptr(known), _ptr(words), lo.data_ptr(), hi.data_ptr(), _ptr(v), _ptr(start),
                                          a.data_ptr(), _ptr(start2), B, T, J, _stream()), "sd_direct_project_accel")
        return out
    check(lib.sd_direct_project(raw.data_ptr(), out.data_ptr(), _ptr(known), _ptr(words), lo.data_ptr(), hi.data_ptr(), _ptr(v), _ptr(start), B, T, J,
                                _stream()), "sd_direct_project")
    return out


def select_medoid(x: Tensor, draws: int, gather: bool = True, index: Optional[Tensor] = None, out: Optional[Tensor] = None):
    """The representative of each context's draws (``sd_select_medoid``): ``x`` (C * draws, T, J) - the draws of a context contiguous, as
    ``ddim_sample(draws=...)`` returns them - or (C, draws, T, J).  Returns ``(index, chosen)``: index (C,) int32 with
    index[c] = argmin_i sum_k |x[c, i] - x[c, k]|^2 (ties to the lowest index), and chosen (C, T, J) = x[c, index[c]] bit for bit, or None
    without ``gather``.  One launch, no read-back.  ``index`` / ``out``: buffers to write into (a session's static ones)."""
    if isinstance(draws, bool) or not isinstance(draws, int) or not 1 <= draws <= 64:
        raise ValueError(f"select_medoid: draws must be an int in [1, 64], got {draws!r}")
    _req(x, "x")
    if x.dim() == 4:
        if x.shape[1] != draws:
            raise ValueError(f"select_medoid: x {tuple(x.shape)} does not hold {draws} draws per context")
        Cn, _, T, J = x.shape
    elif x.dim() == 3 and x.shape[0] % draws == 0 and x.shape[0] > 0:
        Cn, T, J = x.shape[0] // draws, x.shape[1], x.shape[2]
    else:
        raise ValueError(f"select_medoid: expected (C * {draws}, T, J) or (C, {draws}, T, J), got {tuple(x.shape)}")
    if index is None:
        index = torch.empty(Cn, dtype=torch.int32, device=x.device)
    if gather and out is None:
        out = torch.empty(Cn, T, J, dtype=torch.float32, device=x.device)
    check(_lib.load().sd_select_medoid(x.data_ptr(), index.data_ptr(), out.data_ptr() if gather else None, Cn, draws, T, J, _stream()),
          "sd_select_medoid")
    return index, (out if gather else None)


def coherence_weights_host(T: int, decay: float = 0.5) -> np.ndarray:
    """The row weights of ``select_coherent`` on the host: (T,) fp32, w[tau] = decay ** tau computed in float64 and rounded once.
    ValueError unless 0 < decay <= 1.  (decay = 0.5 is the value of the Bidirectional Decoding paper; it has not been measured on this
    policy.)"""
    T = int(T)
    if T < 1:
        raise ValueError(f"select_coherent: T must be positive, got {T}")
    if isinstance(decay, bool) or not isinstance(decay, (int, float)) or not 0.0 < float(decay) <= 1.0:
        raise ValueError(f"select_coherent: decay must be a number in (0, 1], got {decay!r}")
    return np.array([float(decay) ** tau for tau in range(T)], dtype=np.float64).astype(np.float32)


@functools.lru_cache(maxsize=64)
def _coherence_weights(T: int, decay: float, device: str) -> Tensor:
    return torch.from_numpy(coherence_weights_host(T, decay)).to(device)


def coherence_weights(T: int, decay: float = 0.5, device="cuda") -> Tensor:
    """``coherence_weights_host`` in device memory, cached per (T, decay, device): read only."""
    coherence_weights_host(T, decay)   # (the argument errors, every time)
    return _coherence_weights(int(T), float(decay), str(torch.device(device)))


def coherence_lambda(contrast: float, w, shift: int, G: int, T: int, J: int) -> float:
    """``lam`` of ``sd_select_coherent`` for a per-element ``contrast``: the coherence of a draw sums J * sum(w[:R]) weighted squares
    (R = T - shift), its medoid score (G - 1) * T * J squares, so lam = contrast * (J * sum(w[:R])) / ((G - 1) * T * J) weighs the two
    means per element ``contrast`` to 1.  float64 on the host from the fp32 weights as the kernel reads them, rounded once to fp32 (the
    value returned is that fp32 number).  G = 1: 0 (one draw has no other to be close to)."""
    if isinstance(contrast, bool) or not isinstance(contrast, (int, float)) or not float(contrast) >= 0.0 or math.isinf(float(contrast)):
        raise ValueError(f"select_coherent: contrast must be a finite number >= 0, got {contrast!r}")
    if G == 1 or contrast == 0:
        return 0.0
    R = T - shift
    total = np.asarray(w, dtype=np.float32)[:R].astype(np.float64).sum()
    return float(np.float32(np.float64(contrast) * (J * total) / np.float64((G - 1) * T * J)))


@functools.lru_cache(maxsize=256)
def _coherence_lambda_decay(contrast: float, decay: float, shift: int, G: int, T: int, J: int) -> float:
    return coherence_lambda(contrast, coherence_weights_host(T, decay), shift, G, T, J)


def select_coherent(x: Tensor, draws: int, prev: Tensor, shift: int, row_weights: Optional[Tensor] = None, decay: float = 0.5,
                    contrast: float = 0.0, robots=None, gather: bool = True, index: Optional[Tensor] = None, out: Optional[Tensor] = None,
                    cost=None):
    """The draw of each context that continues the context's previous plan (``sd_select_coherent``; the backward-coherence criterion of
    Bidirectional Decoding, Liu et al. 2024).  ``x`` (C * draws, T, J) or (C, draws, T, J) as ``select_medoid`` takes it; ``prev``
    (Cp, T, J): the last committed plan per context in the same normalised space, NaN where there is none; ``shift`` = S in [0, T): the
    rows that passed since, so rows [0, T - S) of a draw and rows [S, T) of the plan describe the same instants.
    cost[c, g] = sum over those rows and the joints of w[tau] * (x - prev)^2 + lam * (the medoid score of draw g); a NaN of ``prev``
    and a zero weight leave their elements out; a context whose plan leaves every element out falls back to the medoid
    (``select_medoid``'s index bit for bit).  The lowest index among the smallest costs wins.
    ``row_weights``: (T,) fp32 weights >= 0 (a device tensor is used as it is; a CPU tensor is checked and uploaded); default
    w[tau] = ``decay`` ** tau (``coherence_weights``).  ``contrast`` >= 0, per element: ``coherence_lambda``; 0 costs G distance sums
    and no medoid.  (With ``row_weights`` on the device and contrast > 0 the weights are read back once to compute lam.)
    ``robots`` (see ``robot_index``; a device tensor is the int32 upload of it): context c reads ``prev[robots[c]]``; default: Cp = C
    and context c reads ``prev[c]``.
    Returns ``(index, chosen, cost)``: index (C,) int32; chosen (C, T, J) = x[c, index[c]] bit for bit, or None without ``gather``; cost
    (C, G) fp32 where ``cost`` is True (a new tensor) or a buffer to write into, else None.  ``index`` / ``out``: buffers to write into.
    One launch, no read-back."""
    if isinstance(draws, bool) or not isinstance(draws, int) or not 1 <= draws <= 64:
        raise ValueError(f"select_coherent: draws must be an int in [1, 64], got {draws!r}")
    if x.dim() == 4:
        if x.shape[1] != draws:
            raise ValueError(f"select_coherent: x {tuple(x.shape)} does not hold {draws} draws per context")
        Cn, _, T, J = x.shape
    elif x.dim() == 3 and x.shape[0] % draws == 0 and x.shape[0] > 0:
        Cn, T, J = x.shape[0] // draws, x.shape[1], x.shape[2]
    else:
        raise ValueError(f"select_coherent: expected (C * {draws}, T, J) or (C, {draws}, T, J), got {tuple(x.shape)}")
    if not isinstance(prev, Tensor) or prev.dim() != 3 or tuple(prev.shape[1:]) != (T, J) or prev.shape[0] < 1:
        raise ValueError(f"select_coherent: prev is (Cp, {T}, {J}), got {tuple(getattr(prev, 'shape', ()))}")
    if isinstance(shift, bool) or not isinstance(shift, int) or not 0 <= shift < T:
        raise ValueError(f"select_coherent: shift must be an int in [0, {T}), got {shift!r}")
    Cp = prev.shape[0]
    if robots is None and Cp != Cn:
        raise ValueError(f"select_coherent: prev holds {Cp} plans for {Cn} contexts and no robots= says which")
    given = row_weights is not None
    if given:
        if not isinstance(row_weights, Tensor) or tuple(row_weights.shape) != (T,) or row_weights.dtype != torch.float32:
            raise ValueError(f"select_coherent: row_weights is a ({T},) fp32 tensor, got {getattr(row_weights, 'shape', row_weights)!r}")
        if not row_weights.is_cuda and not bool((row_weights >= 0).all() and torch.isfinite(row_weights).all()):
            raise ValueError("select_coherent: row_weights are finite numbers >= 0")
        lam = coherence_lambda(contrast, None, shift, 1, T, J)   # (the argument errors before anything is read back)
        if draws > 1 and contrast != 0:
            lam = coherence_lambda(contrast, row_weights.detach().cpu().numpy(), shift, draws, T, J)
    else:
        coherence_weights_host(T, decay)
        coherence_lambda(contrast, None, shift, 1, T, J)
        lam = _coherence_lambda_decay(float(contrast), float(decay), shift, draws, T, J)
    r = None if robots is None else _robots_on(robots, Cp, x.device)
    if r is not None and r.numel() != Cn:
        raise ValueError(f"select_coherent: robots names {r.numel()} plans for {Cn} contexts")
    _req(x, "x"); _req(prev, "prev")
    if prev.device != x.device:
        raise ValueError(f"select_coherent: prev is on {prev.device}, x on {x.device}")
    w = row_weights.to(x.device).contiguous() if given else coherence_weights(T, decay, x.device)
    if index is None:
        index = torch.empty(Cn, dtype=torch.int32, device=x.device)
    if gather and out is None:
        out = torch.empty(Cn, T, J, dtype=torch.float32, device=x.device)
    if cost is True:
        cost = torch.empty(Cn, draws, dtype=torch.float32, device=x.device)
    elif cost is False:
        cost = None
    check(_lib.load().sd_select_coherent(x.data_ptr(), prev.data_ptr(), _ptr(r), w.data_ptr(), index.data_ptr(), out.data_ptr() if gather else None,
                                         _ptr(cost), Cn, draws, T, J, shift, lam, _stream()), "sd_select_coherent")
    return index, (out if gather else None), cost


PREPARE_WEIGHTS, PREPARE_CONTEXT = 1, 2   # SD_PREPARE_*
E_UNSUPPORTED = -4   # SD_E_UNSUPPORTED


class LoopSampler:
    """``forward_with_context`` inside the reference's own denoising loop (soccer_diffusion/ml/inference/plot.py:122-131,
    ml/training/distill.py:179-189, ml/inference/ros.py:301-310) on the trajectory kernels of sampler mode 3: one launch of
    ``traj_step_kernel`` per call (plus the step tokens' K / V and fold).  What does not depend on x or the step - the split
    weight planes, the context's K / V folded with Wq / Woc - is prepared into a workspace this object owns and reused until the
    weights (``weights_key``) or the context tensors (identity and version counters; held here so that their addresses cannot be
    recycled under the cache) change; a context without version counters (inference tensors) is prepared on every call.  ``supported``
    is False where the shape does not take these kernels.
    ``draws`` = G > 1: the context tensors hold C = B / G rows and trajectory b reads context b // G (``sd_sampler_prepare_draws`` /
    ``sd_sampler_eps_draws``): folded once per context, bit for bit the result on ``ctx.repeat_interleave(G, 0)``.  With ``n_tok`` = B
    every trajectory still reads its own step token - the denoiser at G timesteps of the same window."""

    def __init__(self, packed: _Packed, B: int, T: int, Mc: int, n_tok: int, device, max_mode: int = 3, draws: int = 1):
        lib = _lib.load()
        self.draws = _draws_req(draws, B, None)
        self.shape = (B, T, Mc, n_tok)
        self.max_mode = int(max_mode)
        self.supported = _lib.sampler_route_draws(packed.d, packed.heads, T, Mc, packed.J, packed.L, B, self.draws if Mc > 0 else 1,
                                                  self.max_mode).startswith("TRAJ_")
        self.ws = (torch.empty(lib.sd_workspace_floats(B, T, max(Mc, 1), packed.d, packed.L, n_tok), dtype=torch.float32, device=device)
                   if self.supported else None)
        self.status = torch.zeros(1, dtype=torch.int32, device=device) if self.supported and self.max_mode == 4 else None
        self.weights_key = None
        self.context: list = []
        self.versions = None
        self.prepares = 0   # (tests: how many times the context was folded)

    def _context_hit(self, context) -> bool:
        return (len(context) == len(self.context) and all(a is b for a, b in zip(context, self.context))
                and current(self.versions, version_key(*context)))

    def eps(self, packed: _Packed, context, tokens: Tensor, x: Tensor, weights_key) -> Optional[Tensor]:
        """Noise prediction (B, T, J) or None when the library declines the shape (the caller falls back)."""
        lib = _lib.load()
        B, T, Mc, n_tok = self.shape
        _req(x, "x"); _req(tokens, "step tokens")
        what = 0
        if not current(self.weights_key, weights_key):
            what = PREPARE_WEIGHTS | PREPARE_CONTEXT   # the fold multiplies the context's K / V with Wq / Woc
        elif not self._context_hit(context):
            what = PREPARE_CONTEXT
        if what:
            ctx = None
            if Mc > 0:
                ctx = (context[0] if len(context) == 1 else torch.cat(list(context), dim=1)).contiguous()
                _req(ctx, "context")
                if ctx.shape[0] * self.draws != B:
                    raise ValueError(f"context shape mismatch: {ctx.shape[0]} contexts x {self.draws} draws != {B} trajectories")
            rc = lib.sd_sampler_prepare_draws(C.byref(packed.struct), _ptr(ctx), self.ws.data_ptr(), B, T, Mc, n_tok, what, self.max_mode, self.draws,
                                              _stream())
            if rc == E_UNSUPPORTED:
                self.supported = False
                return None
            check(rc, "sd_sampler_prepare_draws")
            self.weights_key, self.context, self.versions = weights_key, list(context), version_key(*context)
            self.prepares += 1
        eps = torch.empty_like(x)
        rc = lib.sd_sampler_eps_draws(C.byref(packed.struct), tokens.data_ptr(), x.data_ptr(), eps.data_ptr(), self.ws.data_ptr(), B, T, Mc, n_tok,
                                      _ptr(self.status), self.max_mode, self.draws, _stream())
        if rc == E_UNSUPPORTED:
            self.supported = False
            return None
        check(rc, "sd_sampler_eps_draws")
        return eps


def sqerr_rows(a: Tensor, b: Tensor) -> Tensor:
    """(rows,) = mean over everything behind the first dimension of (a - b)^2 (``sd_eval_sqerr_rows``: fp32, fixed summation order)."""
    _req(a, "a"); _req(b, "b")
    if a.shape != b.shape or a.dim() < 1 or a.numel() == 0 or a.device != b.device:
        raise ValueError(f"sqerr_rows: expected two equal non-empty shapes on one device, got {tuple(a.shape)} and {tuple(b.shape)}")
    rows = a.shape[0]
    out = torch.empty(rows, dtype=torch.float32, device=a.device)
    check(_lib.load().sd_eval_sqerr_rows(a.data_ptr(), b.data_ptr(), out.data_ptr(), rows, a.numel() // rows, _stream()), "sd_eval_sqerr_rows")
    return out


def trajectory_errors(x: Tensor, target: Tensor, mean: Tensor, std: Tensor, draws: int = 1, angular: bool = True):
    """Errors of sampled trajectories against the recorded ones (``sd_eval_trajectory_errors``, one launch).  ``x`` (C * draws, T, J) or
    (C, draws, T, J) in the sampler's normalised space, ``target`` (C, T, J) the joint commands as the data source delivers them (radians in
    [0, 2 pi)).  d = (x std + mean) - target, with ``angular`` reduced modulo 2 pi into [-pi, pi].  Returns ``(err, row_err, joint_err, best)``:
    the mean of d^2 over (T, J) as (C, draws), over J as (C, draws, T), over T as (C, draws, J), and best (C,) int32 = argmin over the draws
    of err (ties to the lowest index)."""
    if isinstance(draws, bool) or not isinstance(draws, int) or not 1 <= draws <= 64:
        raise ValueError(f"trajectory_errors: draws must be an int in [1, 64], got {draws!r}")
    _req(x, "x"); _req(target, "target"); _req(mean, "mean"); _req(std, "std")
    if target.dim() != 3 or target.shape[0] == 0:
        raise ValueError(f"trajectory_errors: target must be (C, T, J), got {tuple(target.shape)}")
    Cn, T, J = target.shape
    if tuple(x.shape) not in ((Cn * draws, T, J), (Cn, draws, T, J)):
        raise ValueError(f"trajectory_errors: expected x ({Cn} * {draws}, {T}, {J}), got {tuple(x.shape)}")
    if tuple(mean.shape) != (J,) or tuple(std.shape) != (J,) or not 1 <= J <= 32:
        raise ValueError(f"trajectory_errors: mean and std must be ({J},) with J <= 32, got {tuple(mean.shape)} and {tuple(std.shape)}")
    dev = x.device
    if any(t.device != dev for t in (target, mean, std)):
        raise ValueError("trajectory_errors: x, target, mean and std must be on one device")
    err = torch.empty(Cn, draws, dtype=torch.float32, device=dev)
    row_err = torch.empty(Cn, draws, T, dtype=torch.float32, device=dev)
    joint_err = torch.empty(Cn, draws, J, dtype=torch.float32, device=dev)
    best = torch.empty(Cn, dtype=torch.int32, device=dev)
    check(_lib.load().sd_eval_trajectory_errors(x.data_ptr(), target.data_ptr(), mean.data_ptr(), std.data_ptr(), err.data_ptr(), row_err.data_ptr(),
                                                joint_err.data_ptr(), best.data_ptr(), Cn, draws, T, J, int(bool(angular)), _stream()),
          "sd_eval_trajectory_errors")
    return err, row_err, joint_err, best


def max_step(x: Tensor, mean: Tensor, std: Tensor) -> Tensor:
    """The largest step between consecutive rows of sampled trajectories, per joint (``sd_eval_max_step``, one launch): ``x`` (N, T, J) in
    the sampler's normalised space -> (N, J) with [n, j] = max over t of |r[t + 1] - r[t]|, r = x std + mean (fp32).  The number from
    which a slew limit is chosen, and the one that shows it held."""
    _req(x, "x"); _req(mean, "mean"); _req(std, "std")
    if x.dim() != 3 or x.shape[0] == 0:
        raise ValueError(f"max_step: x must be (N, T, J), got {tuple(x.shape)}")
    N, T, J = x.shape
    if tuple(mean.shape) != (J,) or tuple(std.shape) != (J,) or not 1 <= J <= 32 or mean.device != x.device or std.device != x.device:
        raise ValueError(f"max_step: mean and std must be ({J},) with J <= 32 on x's device")
    out = torch.empty(N, J, dtype=torch.float32, device=x.device)
    check(_lib.load().sd_eval_max_step(x.data_ptr(), mean.data_ptr(), std.data_ptr(), out.data_ptr(), N, T, J, _stream()), "sd_eval_max_step")
    return out


def max_accel(x: Tensor, mean: Tensor, std: Tensor) -> Tensor:
    """The largest second difference of sampled trajectories, per joint (``sd_max_accel``, one launch): ``x`` (N, T, J) in the sampler's
    normalised space -> (N, J) with [n, j] = max over t of |(r[t + 1] - r[t]) - (r[t] - r[t - 1])|, r = x std + mean (fp32, one rounding per
    operation).  The number from which an acceleration limit is chosen.  T <= 2: 0."""
    _req(x, "x"); _req(mean, "mean"); _req(std, "std")
    if x.dim() != 3 or x.shape[0] == 0:
        raise ValueError(f"max_accel: x must be (N, T, J), got {tuple(x.shape)}")
    N, T, J = x.shape
    if tuple(mean.shape) != (J,) or tuple(std.shape) != (J,) or not 1 <= J <= 32 or mean.device != x.device or std.device != x.device:
        raise ValueError(f"max_accel: mean and std must be ({J},) with J <= 32 on x's device")
    out = torch.empty(N, J, dtype=torch.float32, device=x.device)
    check(_lib.load().sd_max_accel(x.data_ptr(), mean.data_ptr(), std.data_ptr(), out.data_ptr(), N, T, J, _stream()), "sd_max_accel")
    return out


def noise_loss_grid(model, ctx_list, x0n: Tensor, noise: Tensor, timesteps: Tensor, acp: Optional[Tensor] = None, return_eps: bool = False):
    """The training loss of C held-out windows at K timesteps each: (C, K) with [c, k] = mean over (T, J) of
    (eps(x_t, t_k | context c) - noise[c K + k])^2, x_t = ``ddim_add_noise(x0n[c], noise[c K + k], t_k)``.  ``model``: an
    ``End2EndDiffusionTransformer`` in ``eval()``; ``ctx_list``: its context tensors for the C windows (``encode_input_data``);
    ``x0n`` (C, T, J) normalised; ``noise`` (C K, T, J); ``timesteps`` (K,) int64 on the device.  One denoiser evaluation of C K trajectories
    through ``model.forward_with_context(..., draws=K)``: the context is folded once per window and each trajectory reads its own step token
    (K distinct ones are folded); where the library declines the shape the context rows are expanded and the existing path runs - the same
    result, only not shared.  ``return_eps``: also the prediction (C K, T, J)."""
    _req(x0n, "x0n"); _req(noise, "noise"); _req(timesteps, "timesteps", torch.int64)
    if x0n.dim() != 3 or timesteps.dim() != 1 or timesteps.numel() == 0:
        raise ValueError("noise_loss_grid: x0n must be (C, T, J) and timesteps (K,)")
    Cn, T, J = x0n.shape
    K = timesteps.shape[0]
    if tuple(noise.shape) != (Cn * K, T, J):
        raise ValueError(f"noise_loss_grid: noise must be ({Cn * K}, {T}, {J}), got {tuple(noise.shape)}")
    acp = alphas_cumprod().to(x0n.device) if acp is None else acp
    t_all = timesteps.repeat(Cn)                                   # trajectory c K + k is window c at timestep k
    x_t = ddim_add_noise(x0n.repeat_interleave(K, 0).contiguous(), noise, t_all, acp)
    with torch.no_grad():
        eps = model.forward_with_context(list(ctx_list), x_t, t_all, draws=K)
    loss = sqerr_rows(eps.contiguous(), noise).view(Cn, K)
    return (loss, eps) if return_eps else loss


def _chain16_possible(packed: _Packed) -> bool:
    return packed.d in (128, 256, 512) and packed.J % 4 == 0


# ---- single ops (unit parity tests) ----------------------------------------------------
def linear(A: Tensor, W: Tensor, bias: Optional[Tensor] = None, ln: Optional[tuple] = None, act: str = "none",
           res: Optional[Tensor] = None, out: Optional[Tensor] = None) -> Tensor:
    lib = _lib.load()
    _req(A, "A"); _req(W, "W")
    R, d = A.shape
    N = W.shape[0]
    if out is None:
        out = torch.empty(R, N, dtype=torch.float32, device=A.device)
    check(lib.sd_op_linear(A.data_ptr(), W.data_ptr(), _ptr(bias), _ptr(ln[0]) if ln else None,
                           _ptr(ln[1]) if ln else None, _ptr(res), out.data_ptr(), R, N, d,
                           {"none": 0, "gelu": 1}[act], _stream()), "sd_op_linear")
    return out


def attention(q: Tensor, k: Tensor, v: Tensor, heads: int, extra: Optional[tuple] = None) -> Tensor:
    """q (B,Tq,d), k/v (B,S,d) contiguous; extra = (k_row (d,), v_row (d,)) shared by the batch."""
    lib = _lib.load()
    _req(q, "q"); _req(k, "k"); _req(v, "v")
    B, Tq, d = q.shape
    S = k.shape[1]
    out = torch.empty_like(q)
    check(lib.sd_op_attention(q.data_ptr(), d, k.data_ptr(), v.data_ptr(), d, _ptr(extra[0]) if extra else None,
                              _ptr(extra[1]) if extra else None, out.data_ptr(), d, B, Tq, S, d, heads, _stream()),
          "sd_op_attention")
    return out


def patch_embed(x: Tensor, w: Tensor, b: Tensor, pe: Tensor) -> Tensor:
    lib = _lib.load()
    _req(x, "x"); _req(w, "w"); _req(b, "b"); _req(pe, "pe")
    B, S, Cin = x.shape
    if w.dim() == 2:
        d, p = w.shape[0], 1
    else:
        d, _, p = w.shape
    out = torch.empty(B, S // p, d, dtype=torch.float32, device=x.device)
    check(lib.sd_op_patch_embed(x.data_ptr(), w.data_ptr(), b.data_ptr(), pe.data_ptr(), out.data_ptr(), B, S, Cin, p, d,
                                _stream()), "sd_op_patch_embed")
    return out


def fc_out(h: Tensor, W: Tensor, b: Tensor, x_io: Optional[Tensor] = None, coef4=None, want_eps: bool = True):
    lib = _lib.load()
    _req(h, "h"); _req(W, "W"); _req(b, "b")
    R, d = h.shape
    J = W.shape[0]
    eps = torch.empty(R, J, dtype=torch.float32, device=h.device) if want_eps else None
    cbuf = None
    if coef4 is not None:
        cbuf = (C.c_float * 4)(*[float(v) for v in coef4])
    check(lib.sd_op_fc_out(h.data_ptr(), W.data_ptr(), b.data_ptr(), _ptr(eps), _ptr(x_io),
                           C.cast(cbuf, _lib.c_float_p) if cbuf is not None else None, R, d, J, _stream()), "sd_op_fc_out")
    return eps


# ---- training ops (backward of the blocks, loss, optimizer) ------------------------------
def _rows(t: Tensor, name: str):
    """(data_ptr, row stride) of a tensor viewed as rows of its last dim; the last dim must
    be contiguous and all leading dims must collapse to one uniform row stride (true for
    column slices of a packed [.., 3d] buffer)."""
    if not t.is_cuda or t.dtype != torch.float32:
        raise RuntimeError(f"{name}: expected a float32 tensor on the MI355X; soccerdiffusion_amd has no CPU path")
    if t.stride(-1) != 1:
        raise ValueError(f"{name}: last dimension must be contiguous")
    ld = t.stride(-2) if t.dim() >= 2 else t.shape[-1]
    for i in range(t.dim() - 2):
        if t.shape[i] != 1 and t.stride(i) != t.stride(i + 1) * t.shape[i + 1]:
            raise ValueError(f"{name}: rows are not uniformly strided")
    return t.data_ptr(), int(ld)


def linear_strided(A: Tensor, W: Tensor, bias: Optional[Tensor] = None, res: Optional[Tensor] = None,
                   out: Optional[Tensor] = None) -> Tensor:
    """out[R,N] = A W^T + bias (+res) where A may be a column slice (row stride > d)."""
    lib = _lib.load()
    ap, lda = _rows(A, "A")
    _req(W, "W")
    R = A.numel() // A.shape[-1]
    d = A.shape[-1]
    N = W.shape[0]
    if out is None:
        out = torch.empty(R, N, dtype=torch.float32, device=A.device)
    check(lib.sd_op_linear_strided(ap, lda, W.data_ptr(), _ptr(bias), None, None, _ptr(res), out.data_ptr(), R, N, d, 0,
                                   _stream()), "sd_op_linear_strided")
    return out


def pack_weight_blocks(src: Tensor, src_off: Tensor, n_blocks: int, d: int, dst: Tensor, transposed: bool = False) -> None:
    """Split ``n_blocks`` d x d fp32 blocks (block b at ``src`` + ``src_off[b]`` floats; device int64 offsets) - or their
    transposes - into the fp16 hi | lo fragment planes of ``linear_packed`` (2 d^2 halfs per block, consecutive in ``dst``),
    one launch."""
    lib = _lib.load()
    _req(src, "src")
    if src_off.dtype != torch.int64 or not src_off.is_cuda or dst.dtype != torch.float16 or dst.numel() < 2 * d * d * n_blocks:
        raise ValueError("pack_weight_blocks: src_off must be a device int64 tensor and dst a float16 tensor of 2 d^2 n_blocks")
    check(lib.sd_pack_weight_blocks(src.data_ptr(), src_off.data_ptr(), n_blocks, dst.data_ptr(), d, int(bool(transposed)), _stream()),
          "sd_pack_weight_blocks")


def linear_packed(A: Tensor, wpk: int, N: int, bias: Optional[Tensor] = None, ln: Optional[tuple] = None,
                  res: Optional[Tensor] = None, drop=None, out: Optional[Tensor] = None) -> Tensor:
    """out[R,N] = [res +] [dropout](LN?(A) W^T + bias) with ``wpk`` = the ADDRESS of the split planes of W's N / d blocks
    (pack_weight_blocks); A may be a column slice."""
    lib = _lib.load()
    ap, lda = _rows(A, "A")
    d = A.shape[-1]
    R = A.numel() // d
    if out is None:
        out = torch.empty(R, N, dtype=torch.float32, device=A.device)
    p, seed, site = _drop(drop)
    check(lib.sd_op_linear_packed(ap, lda, wpk, _ptr(bias), _ptr(ln[0]) if ln else None, _ptr(ln[1]) if ln else None, _ptr(res),
                                  out.data_ptr(), R, N, d, p, seed, site, _stream()), "sd_op_linear_packed")
    return out


def _addr(t) -> Optional[int]:
    """Address of a tensor / an int address / None, for the pointer fields of the chain argument structs."""
    if t is None:
        return None
    if isinstance(t, int):
        return t
    if not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous():
        raise RuntimeError("chain operands must be contiguous float32 tensors on the MI355X; soccerdiffusion_amd has no CPU path")
    return t.data_ptr()


def train_fwd_chain(R: int, d: int, h_in: Tensor, *, a=None, wo=None, bo=None, h_out=None, ln=None, n_out=None, w1=None, b1=None,
                    pre=None, u=None, w2=None, b2=None, h2_out=None, nln=None, nn_out=None, wn=None, bn=None, y_out=None,
                    n_next: int = 0, p: float = 0.0, seed: int = 0, sites=(0, 0, 0), amax=(None, None, None, None)) -> None:
    """One launch of sd_train_fwd_chain (include/soccerdiffusion_hip.h).  Weights (wo, w1, w2, wn) are ADDRESSES of split
    planes; ``ln`` / ``nln`` are (weight, bias) pairs; ``sites`` = (out-projection, GELU, FFN output) dropout sites;
    ``amax`` = addresses of the abs-max words of (a, n_out, u, nn_out) or None."""
    lib = _lib.load()
    args = _lib.TrainFwdChainArgs(
        R=R, d=d, n_next=n_next, a=_addr(a), wo=wo, bo=_addr(bo), h_in=_addr(h_in), h_out=_addr(h_out),
        ln_w=_addr(ln[0]) if ln else None, ln_b=_addr(ln[1]) if ln else None, n_out=_addr(n_out), w1=w1, b1=_addr(b1), pre=_addr(pre),
        u=_addr(u), w2=w2, b2=_addr(b2), h2_out=_addr(h2_out), nln_w=_addr(nln[0]) if nln else None,
        nln_b=_addr(nln[1]) if nln else None, nn_out=_addr(nn_out), wn=wn, bn=_addr(bn), y_out=_addr(y_out), p=float(p),
        seed=int(seed) & 0xFFFFFFFFFFFFFFFF, site_out=int(sites[0]), site_act=int(sites[1]), site_ffn=int(sites[2]),
        amax_a=amax[0], amax_n=amax[1], amax_u=amax[2], amax_nn=amax[3], amax_h2=amax[4] if len(amax) > 4 else None)
    check(lib.sd_train_fwd_chain(C.byref(args), _stream()), "sd_train_fwd_chain")


def pack_weight_traj(W: Tensor, out: Optional[Tensor] = None) -> Tensor:
    """(N, 256) weight rows -> the split fp16 planes sd_train_layer_fwd streams (16 x 16 x 32 fragment order of csrc/sd_traj.h, scale 2^8)."""
    lib = _lib.load()
    _req(W, "W")
    N, K = W.shape
    if out is None:
        out = torch.empty(lib.sd_pack_weight_traj_halfs(N, K), dtype=torch.float16, device=W.device)
    check(lib.sd_pack_weight_traj(W.data_ptr(), N, K, out.data_ptr(), _stream()), "sd_pack_weight_traj")
    return out


def pack_weight_traj_multi(base: Tensor, src: Tensor, rows: Tensor, dst: Tensor, max_rows: int, planes: Tensor) -> None:
    """All registered weight slices of a flat parameter buffer -> their trajectory-kernel planes, one launch (device index arrays)."""
    check(_lib.load().sd_pack_weight_traj_multi(base.data_ptr(), src.data_ptr(), rows.data_ptr(), dst.data_ptr(), src.numel(), int(max_rows),
                                                planes.data_ptr(), _stream()), "sd_pack_weight_traj_multi")


def train_head_fwd(x: Tensor, w_emb: int, b_emb: Tensor, pe: Tensor, ln, w_qkv: int, b_qkv: Tensor, amax_n1: Optional[int]):
    """One launch of sd_train_head_fwd: (h0, n1, qkv) of the decoder stack's entry; w_emb / w_qkv are ADDRESSES of planes."""
    _req(x, "x")
    B, T, J = x.shape
    h0 = torch.empty(B, T, 256, dtype=torch.float32, device=x.device)
    n1 = torch.empty(B * T, 256, dtype=torch.float32, device=x.device)
    qkv = torch.empty(B, T, 768, dtype=torch.float32, device=x.device)
    check(_lib.load().sd_train_head_fwd(x.data_ptr(), w_emb, _addr(b_emb), _addr(pe), h0.data_ptr(), _addr(ln[0]), _addr(ln[1]), n1.data_ptr(), w_qkv,
                                        _addr(b_qkv), qkv.data_ptr(), amax_n1, B, T, J, _stream()), "sd_train_head_fwd")
    return h0, n1, qkv


def train_layer_fwd_ok(d: int, heads: int, T: int, M: int) -> bool:
    return bool(_lib.load().sd_train_layer_fwd_ok(d, heads, T, M))


def train_layer_fwd(B: int, T: int, M: int, heads: int, *, tensors: dict, weights: dict, p: float = 0.0, seed: int = 0, sites=(0,) * 6,
                    amax=(None,) * 7) -> None:
    """One launch of sd_train_layer_fwd: ``tensors`` / ``weights`` map the field names of sd_train_layer_fwd_args to tensors (weights
    w_*: ADDRESSES of planes from pack_weight_traj); ``sites`` = dropout sites (self-attention probabilities, its out-projection, cross-
    attention probabilities, its out-projection, GELU, FFN output); ``amax`` = addresses of the abs-max words of (a_sa, n2, a_ca, nf, u,
    nn1, h3) or None."""
    lib = _lib.load()
    kw = {k: (_addr(v) if isinstance(v, Tensor) else v) for k, v in {**tensors, **weights}.items()}
    args = _lib.TrainLayerFwdArgs(B=B, T=T, M=M, d=256, heads=heads, p=float(p), seed=int(seed) & 0xFFFFFFFFFFFFFFFF,
                                  site_sa_probs=int(sites[0]), site_sa_out=int(sites[1]), site_ca_probs=int(sites[2]), site_ca_out=int(sites[3]),
                                  site_act=int(sites[4]), site_ffn=int(sites[5]), amax_a_sa=amax[0], amax_n2=amax[1], amax_a_ca=amax[2],
                                  amax_nf=amax[3], amax_u=amax[4], amax_nn=amax[5], amax_out=amax[6], **kw)
    check(lib.sd_train_layer_fwd(C.byref(args), _stream()), "sd_train_layer_fwd")


def train_bwd_chain(R: int, d: int, dy: Tensor, wt: int, dx: Tensor, *, passes: int = 1, dym=None, pre=None, dpre=None, wt1=None,
                    x=None, ln_w=None, dres=None, dg=None, db=None, p: float = 0.0, seed: int = 0, sites=(0, 0),
                    amax=(None, None)) -> None:
    """One launch of sd_train_bwd_chain.  ``dy`` (R, passes * d) may be a row-strided view; ``wt`` / ``wt1`` are ADDRESSES of
    the split planes of the transposed blocks; ``sites`` = (mask of dy, mask after the GELU); ``amax`` = addresses of the
    abs-max words of (masked dy, dpre) or None."""
    lib = _lib.load()
    dyp, ldy = _rows(dy, "dy")
    args = _lib.TrainBwdChainArgs(
        R=R, d=d, passes=passes, ldy=ldy, dy=dyp, dym=_addr(dym), wt=wt, pre=_addr(pre), dpre=_addr(dpre), wt1=wt1, x=_addr(x),
        ln_w=_addr(ln_w), dres=_addr(dres), dg=_addr(dg), db=_addr(db), dx=_addr(dx), p=float(p), seed=int(seed) & 0xFFFFFFFFFFFFFFFF,
        site_in=int(sites[0]), site_act=int(sites[1]), amax_dy=amax[0], amax_dpre=amax[1], amax_dx=amax[2] if len(amax) > 2 else None)
    check(lib.sd_train_bwd_chain(C.byref(args), _stream()), "sd_train_bwd_chain")


def absmax(x: Tensor, amax: int) -> None:
    """Max the bits of max |x| into the SD_AMAX_WORDS words at address ``amax`` (zeroed by the caller); x may be row-strided."""
    lib = _lib.load()
    xp, ld = _rows(x, "x")
    width = x.shape[-1]
    check(lib.sd_op_absmax(xp, x.numel() // width, width, ld, amax, _stream()), "sd_op_absmax")


def gemm_tn_grouped(problems) -> None:
    """dW += dY^T X (db += column sums of dY) for every (dY, X, dW, db, amax_dy, amax_x) in ``problems`` in one launch per 8.
    dY / X may be row-strided views; ``amax_*`` are ADDRESSES of device words with the bits of max |dY| / max |X|."""
    lib = _lib.load()
    arr = (_lib.GemmTnProblem * len(problems))()
    for q, (dY, X, dW, db, ay, ax) in zip(arr, problems):
        yp, ldy = _rows(dY, "dY"); xp, ldx = _rows(X, "X")
        _req(dW, "dW")
        q.dY, q.X, q.dW, q.db, q.amax_dy, q.amax_x = yp, xp, dW.data_ptr(), _ptr(db), ay, ax
        q.R, q.N, q.K = dY.numel() // dY.shape[-1], dY.shape[-1], X.shape[-1]
        q.ldy, q.ldx, q.ldw = ldy, ldx, dW.stride(0)
    check(lib.sd_gemm_tn_grouped(arr, len(problems), _stream()), "sd_gemm_tn_grouped")


# ---- dropout (training; one Philox mask function shared by every kernel, include/soccerdiffusion_hip.h) ----------------
def _drop(drop) -> tuple:
    """(p, seed, site) -> ctypes-ready triple; None = no dropout."""
    if drop is None:
        return 0.0, 0, 0
    p, seed, site = drop
    return float(p), int(seed) & 0xFFFFFFFFFFFFFFFF, int(site) & 0xFFFFFFFFFFFFFFFF


def dropout(x: Tensor, drop, out: Optional[Tensor] = None) -> Tensor:
    """x o mask over the last dim as the mask width (rows = everything else)."""
    lib = _lib.load()
    _req(x, "x")
    width = x.shape[-1]
    if out is None:
        out = torch.empty_like(x)
    p, seed, site = _drop(drop)
    check(lib.sd_op_dropout(x.data_ptr(), out.data_ptr(), x.numel() // width, width, p, seed, site, _stream()), "sd_op_dropout")
    return out


def dropout_mask(rows: int, width: int, drop, device) -> Tensor:
    """The (rows, width) multiplier tensor (0 or 1/(1-p)) the kernels apply for this (p, seed, site)."""
    lib = _lib.load()
    mask = torch.empty(rows, width, dtype=torch.float32, device=device)
    p, seed, site = _drop(drop)
    check(lib.sd_op_dropout_mask(mask.data_ptr(), rows, width, p, seed, site, _stream()), "sd_op_dropout_mask")
    return mask


def gelu_dropout_fwd(pre: Tensor, drop) -> Tensor:
    lib = _lib.load()
    _req(pre, "pre")
    out = torch.empty_like(pre)
    width = pre.shape[-1]
    p, seed, site = _drop(drop)
    check(lib.sd_op_gelu_dropout_fwd(pre.data_ptr(), out.data_ptr(), pre.numel() // width, width, p, seed, site, _stream()),
          "sd_op_gelu_dropout_fwd")
    return out


def gelu_dropout_bwd(dy: Tensor, pre: Tensor, drop) -> Tensor:
    lib = _lib.load()
    _req(dy, "dy"); _req(pre, "pre")
    out = torch.empty_like(pre)
    width = pre.shape[-1]
    p, seed, site = _drop(drop)
    check(lib.sd_op_gelu_dropout_bwd(dy.data_ptr(), pre.data_ptr(), out.data_ptr(), pre.numel() // width, width, p, seed, site,
                                     _stream()), "sd_op_gelu_dropout_bwd")
    return out


def linear_dropout(A: Tensor, W: Tensor, bias: Optional[Tensor], res: Tensor, drop, out: Optional[Tensor] = None) -> Tensor:
    """out = res + dropout(A W^T + bias): the fused epilogue of the split-fp16 panel GEMM."""
    lib = _lib.load()
    _req(A, "A"); _req(W, "W"); _req(res, "res")
    R, d = A.shape
    N = W.shape[0]
    if out is None:
        out = torch.empty(R, N, dtype=torch.float32, device=A.device)
    p, seed, site = _drop(drop)
    check(lib.sd_op_linear_dropout(A.data_ptr(), d, W.data_ptr(), _ptr(bias), res.data_ptr(), out.data_ptr(), R, N, d, p, seed, site,
                                   _stream()), "sd_op_linear_dropout")
    return out


def attention_lse(q: Tensor, k: Tensor, v: Tensor, heads: int, drop=None):
    """Forward attention that also returns lse2 (B, heads, Tq).  q (B,Tq,d), k/v (B,S,d) may be
    column-slice views of packed buffers.  ``drop`` = (p, seed, site): dropout on the probabilities."""
    lib = _lib.load()
    qp, ldq = _rows(q, "q"); kp, ldk = _rows(k, "k"); vp, ldv = _rows(v, "v")
    if ldk != ldv:
        raise ValueError("k and v must share a row stride")
    B, Tq, d = q.shape
    S = k.shape[1]
    out = torch.empty(B, Tq, d, dtype=torch.float32, device=q.device)
    lse = torch.empty(B, heads, Tq, dtype=torch.float32, device=q.device)
    p, seed, site = _drop(drop)
    check(lib.sd_op_attention_lse_dropout(qp, ldq, kp, vp, ldk, out.data_ptr(), d, lse.data_ptr(), B, Tq, S, d, heads, p, seed, site,
                                          _stream()), "sd_op_attention_lse")
    return out, lse


def attention_bwd(q: Tensor, k: Tensor, v: Tensor, o: Tensor, dO: Tensor, lse: Tensor, dq: Tensor, dk: Tensor, dv: Tensor,
                  heads: int, drop=None) -> None:
    lib = _lib.load()
    qp, ldq = _rows(q, "q"); kp, ldk = _rows(k, "k"); vp, ldv = _rows(v, "v")
    op, ldo = _rows(o, "o"); dop, lddo = _rows(dO, "dO")
    dqp, lddq = _rows(dq, "dq"); dkp, lddk = _rows(dk, "dk"); dvp, lddv = _rows(dv, "dv")
    if ldk != ldv or lddk != lddv:
        raise ValueError("k/v (and dk/dv) must share a row stride")
    B, Tq, d = q.shape
    S = k.shape[1]
    p, seed, site = _drop(drop)
    check(lib.sd_op_attention_bwd_dropout(qp, ldq, kp, vp, ldk, op, ldo, dop, lddo, lse.data_ptr(), dqp, lddq, dkp, dvp, lddk,
                                          B, Tq, S, d, heads, p, seed, site, _stream()), "sd_op_attention_bwd")


def train_xattn_shared_ok(d: int, heads: int, T: int, Mc: int) -> bool:
    """The shared cross-attention kernels take this shape (head dim 16 / 32 / 64, 1 <= T <= 100, Mc >= 1)."""
    return bool(_lib.load().sd_train_xattn_shared_ok(int(d), int(heads), int(T), int(Mc)))


def _xattn_shared_shapes(q: Tensor, kv_ctx: Tensor, kv_tok: Tensor, draws: int):
    for t, name in ((q, "q"), (kv_ctx, "kv_ctx"), (kv_tok, "kv_tok")):
        _req(t, name)
    B, T, d = q.shape
    C_, Mc = kv_ctx.shape[0], kv_ctx.shape[1]
    _draws_req(draws, B, C_)
    if tuple(kv_ctx.shape) != (C_, Mc, 2 * d) or tuple(kv_tok.shape) != (B, 1, 2 * d):
        raise ValueError(f"shared cross-attention: expected kv_ctx (C, Mc, {2 * d}) and kv_tok ({B}, 1, {2 * d}), got {tuple(kv_ctx.shape)} and "
                         f"{tuple(kv_tok.shape)}")
    return C_, T, Mc, d


def train_xattn_shared_fwd(q: Tensor, kv_ctx: Tensor, kv_tok: Tensor, heads: int, draws: int, drop=None):
    """Cross-attention of C * draws trajectories over C shared contexts: q (C * draws, T, d), kv_ctx (C, Mc, 2d), kv_tok (C * draws, 1, 2d);
    trajectory b's keys are context b // draws's rows, then its own token row.  Returns (out, lse2) as ``attention_lse`` on the expanded
    K | V does - the same dropout mask under the same ``drop``.  A shape the kernels decline raises ``Unsupported``-coded RuntimeError."""
    lib = _lib.load()
    C_, T, Mc, d = _xattn_shared_shapes(q, kv_ctx, kv_tok, draws)
    out = torch.empty_like(q)
    lse = torch.empty(q.shape[0], heads, T, dtype=torch.float32, device=q.device)
    p, seed, site = _drop(drop)
    check(lib.sd_train_xattn_shared_fwd(q.data_ptr(), kv_ctx.data_ptr(), kv_tok.data_ptr(), out.data_ptr(), lse.data_ptr(), C_, draws, T, Mc, d,
                                        heads, p, seed, site, _stream()), "sd_train_xattn_shared_fwd")
    return out, lse


def train_xattn_shared_bwd(q: Tensor, kv_ctx: Tensor, kv_tok: Tensor, o: Tensor, dO: Tensor, lse: Tensor, heads: int, draws: int, drop=None):
    """(dq, dkv_ctx, dkv_tok) of ``train_xattn_shared_fwd``; dkv_ctx is summed over the draws in a fixed order (bitwise repeatable)."""
    lib = _lib.load()
    C_, T, Mc, d = _xattn_shared_shapes(q, kv_ctx, kv_tok, draws)
    _req(o, "o"); _req(dO, "dO"); _req(lse, "lse")
    if o.shape != q.shape or dO.shape != q.shape or tuple(lse.shape) != (q.shape[0], heads, T):
        raise ValueError("shared cross-attention backward: o / dO / lse do not match q")
    dq, dkv_ctx, dkv_tok = torch.empty_like(q), torch.empty_like(kv_ctx), torch.empty_like(kv_tok)
    p, seed, site = _drop(drop)
    check(lib.sd_train_xattn_shared_bwd(q.data_ptr(), kv_ctx.data_ptr(), kv_tok.data_ptr(), o.data_ptr(), dO.data_ptr(), lse.data_ptr(),
                                        dq.data_ptr(), dkv_ctx.data_ptr(), dkv_tok.data_ptr(), C_, draws, T, Mc, d, heads, p, seed, site,
                                        _stream()), "sd_train_xattn_shared_bwd")
    return dq, dkv_ctx, dkv_tok


def expand_rows(x: Tensor, draws: int) -> Tensor:
    """x (C, ...) -> (C * draws, ...), row b = x[b // draws] (``repeat_interleave(draws, 0)``)."""
    _req(x, "x")
    _draws_req(draws, 0, None)
    C_ = x.shape[0]
    row = x.numel() // C_
    out = torch.empty(C_ * draws, *x.shape[1:], dtype=torch.float32, device=x.device)
    check(_lib.load().sd_train_expand_rows(x.data_ptr(), out.data_ptr(), C_, draws, row, _stream()), "sd_train_expand_rows")
    return out


def expand_rows_bwd(dout: Tensor, draws: int) -> Tensor:
    """The gradient of ``expand_rows``: the sum over each group of ``draws`` rows, in draw order."""
    _req(dout, "dout")
    _draws_req(draws, dout.shape[0], None)
    C_ = dout.shape[0] // draws
    row = dout.numel() // dout.shape[0]
    din = torch.empty(C_, *dout.shape[1:], dtype=torch.float32, device=dout.device)
    check(_lib.load().sd_train_expand_rows_bwd(dout.data_ptr(), din.data_ptr(), C_, draws, row, _stream()), "sd_train_expand_rows_bwd")
    return din


def gemm_tn(dY: Tensor, X: Tensor, dW: Tensor, db: Optional[Tensor] = None) -> None:
    """dW[N,K] += dY[R,N]^T X[R,K]; db[N] += colsum(dY).  dY / X may be column slices."""
    lib = _lib.load()
    yp, ldy = _rows(dY, "dY"); xp, ldx = _rows(X, "X")
    _req(dW, "dW")
    N, K = dY.shape[-1], X.shape[-1]
    R = dY.numel() // N
    if X.numel() // K != R or tuple(dW.shape) != (N, K):
        raise ValueError("gemm_tn: shape mismatch")
    check(lib.sd_op_gemm_tn(yp, ldy, xp, ldx, dW.data_ptr(), K, _ptr(db), R, N, K, _stream()), "sd_op_gemm_tn")


def layernorm_fwd(x: Tensor, g: Tensor, b: Tensor, want_stats: bool = True):
    lib = _lib.load()
    _req(x, "x")
    d = x.shape[-1]
    R = x.numel() // d
    y = torch.empty_like(x)
    mean = torch.empty(R, dtype=torch.float32, device=x.device) if want_stats else None
    rstd = torch.empty(R, dtype=torch.float32, device=x.device) if want_stats else None
    check(lib.sd_op_layernorm_fwd(x.data_ptr(), g.data_ptr(), b.data_ptr(), y.data_ptr(), _ptr(mean), _ptr(rstd), R, d,
                                  _stream()), "sd_op_layernorm_fwd")
    return y, mean, rstd


def layernorm_bwd(dy: Tensor, x: Tensor, mean: Tensor, rstd: Tensor, g: Tensor, dres: Optional[Tensor] = None):
    lib = _lib.load()
    _req(dy, "dy"); _req(x, "x")
    d = x.shape[-1]
    R = x.numel() // d
    dx = torch.empty_like(x)
    dg = torch.zeros(d, dtype=torch.float32, device=x.device)
    db = torch.zeros(d, dtype=torch.float32, device=x.device)
    check(lib.sd_op_layernorm_bwd(dy.data_ptr(), x.data_ptr(), mean.data_ptr(), rstd.data_ptr(), g.data_ptr(), _ptr(dres),
                                  dx.data_ptr(), dg.data_ptr(), db.data_ptr(), R, d, _stream()), "sd_op_layernorm_bwd")
    return dx, dg, db


def layernorm_bwd_into(dy: Tensor, x: Tensor, mean: Tensor, rstd: Tensor, g: Tensor, dg: Tensor, db: Tensor,
                       dres: Optional[Tensor] = None) -> Tensor:
    """LayerNorm backward that ACCUMULATES the affine gradients into existing dg / db buffers; ``dres`` (same shape as x)
    is added to dx inside the kernel (the residual branch's gradient)."""
    lib = _lib.load()
    _req(dy, "dy"); _req(x, "x")
    if dres is not None:
        _req(dres, "dres")
    d = x.shape[-1]
    R = x.numel() // d
    dx = torch.empty_like(x)
    check(lib.sd_op_layernorm_bwd(dy.data_ptr(), x.data_ptr(), mean.data_ptr(), rstd.data_ptr(), g.data_ptr(), _ptr(dres),
                                  dx.data_ptr(), dg.data_ptr(), db.data_ptr(), R, d, _stream()), "sd_op_layernorm_bwd")
    return dx


def gelu_fwd(pre: Tensor) -> Tensor:
    lib = _lib.load()
    _req(pre, "pre")
    out = torch.empty_like(pre)
    check(lib.sd_op_gelu_fwd(pre.data_ptr(), out.data_ptr(), pre.numel(), _stream()), "sd_op_gelu_fwd")
    return out


def gelu_bwd(dy: Tensor, pre: Tensor) -> Tensor:
    lib = _lib.load()
    _req(dy, "dy"); _req(pre, "pre")
    out = torch.empty_like(pre)
    check(lib.sd_op_gelu_bwd(dy.data_ptr(), pre.data_ptr(), out.data_ptr(), pre.numel(), _stream()), "sd_op_gelu_bwd")
    return out


def colsum(src: Tensor, out: Tensor) -> None:
    """out[c] += sum_r src[r, c] for a (possibly column-sliced) 2-D / 3-D src."""
    lib = _lib.load()
    sp, ld = _rows(src, "src")
    width = src.shape[-1]
    check(lib.sd_op_colsum(sp, ld, src.numel() // width, width, out.data_ptr(), _stream()), "sd_op_colsum")


def small_k_matmul(A: Tensor, Bm: Tensor) -> Tensor:
    lib = _lib.load()
    _req(A, "A"); _req(Bm, "B")
    K, N = Bm.shape
    R = A.numel() // K
    out = torch.empty(R, N, dtype=torch.float32, device=A.device)
    check(lib.sd_op_small_k_matmul(A.data_ptr(), Bm.data_ptr(), out.data_ptr(), R, K, N, _stream()), "sd_op_small_k_matmul")
    return out


def mse_loss(pred: Tensor, target: Tensor, want_grad: bool = True):
    """(loss (1,), grad or None): F.mse_loss mean reduction and 2 (pred - target) / n."""
    lib = _lib.load()
    _req(pred, "pred"); _req(target, "target")
    loss = torch.empty(1, dtype=torch.float32, device=pred.device)
    grad = torch.empty_like(pred) if want_grad else None
    scratch = torch.empty(256, dtype=torch.float64, device=pred.device)
    check(lib.sd_mse_loss(pred.data_ptr(), target.data_ptr(), loss.data_ptr(), _ptr(grad), scratch.data_ptr(), pred.numel(),
                          _stream()), "sd_mse_loss")
    return loss, grad


def adamw_step_dev(p: Tensor, g: Tensor, m: Tensor, v: Tensor, hyper7: Tensor) -> None:
    """AdamW update with its seven scalars in device memory (graph-capturable; see adamw_hyper)."""
    lib = _lib.load()
    for t, n in ((p, "p"), (g, "g"), (m, "m"), (v, "v"), (hyper7, "hyper7")):
        _req(t, n)
    if hyper7.numel() < 7:
        raise ValueError("hyper7 needs 7 floats")
    check(lib.sd_adamw_step_dev(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), hyper7.data_ptr(), _stream()),
          "sd_adamw_step_dev")


def adamw_hyper(lr: float, beta1: float, beta2: float, eps: float, weight_decay: float, step: int, out: Tensor) -> None:
    """Fills ``out[:7]`` (a CPU float32 tensor, e.g. pinned) with the scalars sd_adamw_step derives for update ``step``."""
    if out.is_cuda or out.dtype != torch.float32 or out.numel() < 7 or not out.is_contiguous():
        raise ValueError("out must be a contiguous CPU float32 tensor with >= 7 elements")
    check(_lib.load().sd_adamw_hyper(lr, beta1, beta2, eps, weight_decay, step, C.cast(out.data_ptr(), _lib.c_float_p)), "sd_adamw_hyper")


def set_dropout_epoch(word: Optional[Tensor]) -> None:
    """Process-wide: the uint32 device word every dropout kernel adds to its Philox key at run time (None = off)."""
    if word is not None and (not word.is_cuda or word.element_size() != 4 or word.numel() < 1):
        raise ValueError("the epoch word must be a 4-byte element on the device")
    check(_lib.load().sd_set_dropout_epoch(None if word is None else word.data_ptr()), "sd_set_dropout_epoch")


def adamw_step(p: Tensor, g: Tensor, m: Tensor, v: Tensor, lr: float, beta1: float, beta2: float, eps: float,
               weight_decay: float, step: int) -> None:
    lib = _lib.load()
    for t, n in ((p, "p"), (g, "g"), (m, "m"), (v, "v")):
        _req(t, n)
    check(lib.sd_adamw_step(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), lr, beta1, beta2, eps,
                            weight_decay, step, _stream()), "sd_adamw_step")


def adamw_ema_step(p: Tensor, g: Tensor, m: Tensor, v: Tensor, ema: Tensor, lr: float, beta1: float, beta2: float, eps: float,
                   weight_decay: float, step: int, ema_weight: float) -> None:
    """``adamw_step`` and ``ema += ema_weight (p_new - ema)`` in the same launch."""
    lib = _lib.load()
    for t, n in ((p, "p"), (g, "g"), (m, "m"), (v, "v"), (ema, "ema")):
        _req(t, n)
    if ema.numel() != p.numel():
        raise ValueError("ema must have as many elements as p")
    check(lib.sd_adamw_ema_step(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), ema.data_ptr(), p.numel(), lr, beta1, beta2, eps,
                                weight_decay, step, ema_weight, _stream()), "sd_adamw_ema_step")


def adamw_ema_step_dev(p: Tensor, g: Tensor, m: Tensor, v: Tensor, ema: Tensor, hyper7: Tensor, ema_weight: Tensor) -> None:
    """``adamw_step_dev`` and the EMA in the same launch, this update's weight read from the device float ``ema_weight``."""
    lib = _lib.load()
    for t, n in ((p, "p"), (g, "g"), (m, "m"), (v, "v"), (ema, "ema"), (hyper7, "hyper7"), (ema_weight, "ema_weight")):
        _req(t, n)
    if hyper7.numel() < 7 or ema_weight.numel() < 1 or ema.numel() != p.numel():
        raise ValueError("hyper7 needs 7 floats, ema_weight one, ema as many elements as p")
    check(lib.sd_adamw_ema_step_dev(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), ema.data_ptr(), p.numel(), hyper7.data_ptr(),
                                    ema_weight.data_ptr(), _stream()), "sd_adamw_ema_step_dev")


def grad_norm_workspace_doubles() -> int:
    """Doubles of device scratch ``grad_norm`` needs (a constant of the library: its fixed grid)."""
    return int(_lib.load().sd_grad_norm_workspace_doubles())


def grad_norm(g: Tensor, partials: Tensor, clip: Tensor, skipped: Tensor, max_norm: float) -> None:
    """Global 2-norm of the flat gradient ``g`` in one deterministic fp64 summation -> ``clip[0]``; the clipping coefficient
    ``min(1, max_norm / (norm + 1e-6))`` (fp32, torch's clip_grad_norm_) -> ``clip[1]``, or 0 where the norm is not finite - then the
    int32 ``skipped[0]`` goes up by one.  Two launches, no host read: graph-capturable.  ``partials``: ``grad_norm_workspace_doubles()``
    float64 of scratch."""
    lib = _lib.load()
    max_norm = float(max_norm)
    if not max_norm >= 0.0:   # (NaN fails the comparison)
        raise ValueError(f"max_norm must be >= 0 (inf = norm and guard only), got {max_norm!r}")
    _req(g, "g"); _req(partials, "partials", torch.float64); _req(clip, "clip"); _req(skipped, "skipped", torch.int32)
    if g.numel() < 1 or partials.numel() < grad_norm_workspace_doubles() or clip.numel() < 2 or skipped.numel() < 1:
        raise ValueError("g needs >= 1 element, partials grad_norm_workspace_doubles() doubles, clip 2 floats, skipped one int32")
    check(lib.sd_grad_norm(g.data_ptr(), g.numel(), partials.data_ptr(), clip.data_ptr(), skipped.data_ptr(), max_norm, _stream()),
          "sd_grad_norm")


def adamw_clip_step(p: Tensor, g: Tensor, m: Tensor, v: Tensor, ema: Optional[Tensor], clip: Tensor, lr: float, beta1: float, beta2: float,
                    eps: float, weight_decay: float, step: int, ema_weight: float = 0.0) -> None:
    """``adamw_step`` (``ema`` None) or ``adamw_ema_step`` on ``g * clip[1]``, skipped entirely where ``clip[0]`` is not finite
    (``clip``: what ``grad_norm`` wrote); ``g`` is not modified."""
    lib = _lib.load()
    for t, n in ((p, "p"), (g, "g"), (m, "m"), (v, "v"), (clip, "clip")) + (() if ema is None else ((ema, "ema"),)):
        _req(t, n)
    if clip.numel() < 2 or (ema is not None and ema.numel() != p.numel()):
        raise ValueError("clip needs 2 floats, ema as many elements as p")
    check(lib.sd_adamw_clip_step(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), _ptr(ema), p.numel(), lr, beta1, beta2, eps,
                                 weight_decay, step, ema_weight, clip.data_ptr(), _stream()), "sd_adamw_clip_step")


def adamw_clip_step_dev(p: Tensor, g: Tensor, m: Tensor, v: Tensor, ema: Optional[Tensor], clip: Tensor, hyper7: Tensor,
                        ema_weight: Optional[Tensor] = None) -> None:
    """``adamw_step_dev`` (``ema`` None) or ``adamw_ema_step_dev`` on ``g * clip[1]``, skipped where ``clip[0]`` is not finite."""
    lib = _lib.load()
    if ema is not None and ema_weight is None:
        raise ValueError("with ema the update needs the device float ema_weight")
    for t, n in ((p, "p"), (g, "g"), (m, "m"), (v, "v"), (clip, "clip"), (hyper7, "hyper7")) + (
            () if ema is None else ((ema, "ema"), (ema_weight, "ema_weight"))):
        _req(t, n)
    if hyper7.numel() < 7 or clip.numel() < 2 or (ema is not None and (ema_weight.numel() < 1 or ema.numel() != p.numel())):
        raise ValueError("hyper7 needs 7 floats, clip 2, ema_weight one, ema as many elements as p")
    check(lib.sd_adamw_clip_step_dev(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), _ptr(ema), p.numel(), hyper7.data_ptr(),
                                     None if ema is None else ema_weight.data_ptr(), clip.data_ptr(), _stream()), "sd_adamw_clip_step_dev")


# ---- image path: ResNet basic-block convolution (csrc/sd_conv.hip) -------------------------------------
class PackedConv3x3:
    """A 3 x 3 (or 1 x 1) convolution weight (Cout, Cin, k, k) in the fragment order of ``sd_conv3x3_bn_act`` / ``sd_conv_s2_bn_act`` plus
    the power-of-two scale the fp16 planes carry; ``refresh`` repacks in place (when: derived.py)."""

    def __init__(self, weight: Tensor):
        lib = _lib.load()
        _req(weight, "weight")
        Cout, Cin, kh, kw = weight.shape
        if kh != kw or kh not in (1, 3) or Cout % 64 or Cin % 64:
            raise ValueError("3 x 3 or 1 x 1 kernels with channel counts that are multiples of 64")
        self.Cout, self.Cin, self.ksize = Cout, Cin, kh
        self.planes = torch.empty(lib.sd_conv_packed_halfs(Cout, Cin, kh), dtype=torch.float16, device=weight.device)
        self.scale = torch.empty(1, dtype=torch.float32, device=weight.device)
        self._word = torch.zeros(1, dtype=torch.int32, device=weight.device)
        self.refresh(weight)

    def refresh(self, weight: Tensor) -> "PackedConv3x3":
        w = weight.detach().contiguous()
        check(_lib.load().sd_conv_pack(w.data_ptr(), self.Cout, self.Cin, self.ksize, self.planes.data_ptr(), self.scale.data_ptr(),
                                       self._word.data_ptr(), _stream()), "sd_conv_pack")
        return self


def absmax_word(x: Tensor, word: Optional[Tensor] = None, zero: bool = True) -> Tensor:
    """The bits of max |x| in one int32 device word (the activation scale ``conv3x3_bn_act`` derives for its fp16 planes)."""
    _req(x, "x")
    if word is None:
        word = torch.zeros(1, dtype=torch.int32, device=x.device)
    elif zero:
        word.zero_()
    check(_lib.load().sd_absmax_word(x.data_ptr(), x.numel(), word.data_ptr(), _stream()), "sd_absmax_word")
    return word


def conv3x3_bn_act(x: Tensor, x_amax: Tensor, w: PackedConv3x3, bn_scale: Tensor, bn_shift: Tensor, res: Optional[Tensor] = None,
                   relu: bool = True, y_amax: Optional[Tensor] = None, zero_amax: bool = True) -> Tensor:
    """relu(conv(x) * bn_scale + bn_shift (+ res)) on NHWC fp32 tensors, stride 1: 3 x 3 / padding 1 or 1 x 1 (``w.ksize``) - torchvision
    BasicBlock's / Bottleneck's conv / bn / relu in inference mode (reference: soccer_diffusion/ml/model/encoder/image.py:55-83).  ``x_amax``: word from
    ``absmax_word`` or the ``y_amax`` of the launch that produced x; ``y_amax`` (zeroed here unless ``zero_amax`` is False: the caller
    zeroed it, e.g. all words of a forward in one fill) receives max |y|."""
    _req(x, "x"); _req(bn_scale, "bn_scale"); _req(bn_shift, "bn_shift")
    N, H, W, Cin = x.shape
    if Cin != w.Cin:
        raise ValueError("channel mismatch")
    y = torch.empty(N, H, W, w.Cout, dtype=torch.float32, device=x.device)
    if res is not None:
        _req(res, "res")
        if res.shape != y.shape:
            raise ValueError("residual shape mismatch")
    if y_amax is not None and zero_amax:
        y_amax.zero_()
    fn = _lib.load().sd_conv3x3_bn_act if w.ksize == 3 else _lib.load().sd_conv1x1_bn_act   # (a 1 x 1 weight: Bottleneck projections)
    check(fn(x.data_ptr(), w.planes.data_ptr(), w.scale.data_ptr(), x_amax.data_ptr(), bn_scale.data_ptr(),
             bn_shift.data_ptr(), _ptr(res), y.data_ptr(), _ptr(y_amax), N, H, W, Cin, w.Cout, int(relu), _stream()),
          "sd_conv3x3_bn_act" if w.ksize == 3 else "sd_conv1x1_bn_act")
    return y


def conv_s2_bn_act(x: Tensor, x_amax: Tensor, w: PackedConv3x3, bn_scale: Tensor, bn_shift: Tensor, relu: bool = True,
                   y_amax: Optional[Tensor] = None, zero_amax: bool = True) -> Tensor:
    """act(conv(x; stride 2) * bn_scale + bn_shift) on NHWC fp32 tensors: the 3 x 3 / padding 1 convolution that opens ResNet layers 2 - 4 or
    their 1 x 1 shortcut (``w.ksize``), inference BatchNorm folded (reference: torchvision BasicBlock via
    soccer_diffusion/ml/model/encoder/image.py:55-83).  Same conventions as ``conv3x3_bn_act``."""
    _req(x, "x"); _req(bn_scale, "bn_scale"); _req(bn_shift, "bn_shift")
    N, H, W, Cin = x.shape
    if Cin != w.Cin:
        raise ValueError("channel mismatch")
    y = torch.empty(N, (H + 1) // 2, (W + 1) // 2, w.Cout, dtype=torch.float32, device=x.device)
    if y_amax is not None and zero_amax:
        y_amax.zero_()
    check(_lib.load().sd_conv_s2_bn_act(x.data_ptr(), w.planes.data_ptr(), w.scale.data_ptr(), x_amax.data_ptr(), bn_scale.data_ptr(),
                                        bn_shift.data_ptr(), y.data_ptr(), _ptr(y_amax), N, H, W, Cin, w.Cout, w.ksize, int(relu), _stream()),
          "sd_conv_s2_bn_act")
    return y


class PackedStem:
    """ResNet's first convolution (64, 3, 7, 7) in the fragment order of ``sd_stem_conv_bn_relu_pool``; ``refresh`` repacks in place."""

    def __init__(self, weight: Tensor):
        lib = _lib.load()
        _req(weight, "weight")
        if tuple(weight.shape) != (64, 3, 7, 7):
            raise ValueError("the ResNet stem convolution is (64, 3, 7, 7)")
        self.planes = torch.empty(lib.sd_stem_packed_halfs(), dtype=torch.float16, device=weight.device)
        self.scale = torch.empty(1, dtype=torch.float32, device=weight.device)
        self._word = torch.zeros(1, dtype=torch.int32, device=weight.device)
        self.refresh(weight)

    def refresh(self, weight: Tensor) -> "PackedStem":
        w = weight.detach().contiguous()
        check(_lib.load().sd_stem_pack(w.data_ptr(), self.planes.data_ptr(), self.scale.data_ptr(), self._word.data_ptr(), _stream()),
              "sd_stem_pack")
        return self


def stem_conv_bn_relu_pool(x: Tensor, x_amax: Tensor, w: PackedStem, bn_scale: Tensor, bn_shift: Tensor,
                           y_amax: Optional[Tensor] = None, zero_amax: bool = True) -> Tensor:
    """maxpool3x3/s2/p1(relu(conv7x7/s2/p3(x) * bn_scale + bn_shift)): NCHW frames (N, 3, H, W) -> NHWC map (N, Hp, Wp, 64) in one
    launch - torchvision ResNet's conv1 / bn1 / relu / maxpool in inference mode (reference: soccer_diffusion/ml/model/encoder/image.py:55-83)."""
    _req(x, "x"); _req(bn_scale, "bn_scale"); _req(bn_shift, "bn_shift")
    N, C3, H, W = x.shape
    if C3 != 3:
        raise ValueError("the stem takes 3-channel frames")
    Hc, Wc = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    y = torch.empty(N, (Hc - 1) // 2 + 1, (Wc - 1) // 2 + 1, 64, dtype=torch.float32, device=x.device)
    if y_amax is not None and zero_amax:
        y_amax.zero_()
    check(_lib.load().sd_stem_conv_bn_relu_pool(x.data_ptr(), w.planes.data_ptr(), w.scale.data_ptr(), x_amax.data_ptr(), bn_scale.data_ptr(),
                                                bn_shift.data_ptr(), y.data_ptr(), _ptr(y_amax), N, H, W, _stream()),
          "sd_stem_conv_bn_relu_pool")
    return y


# ---- image path: Swin-T / Swin-S inference (csrc/sd_swin.hip) -------------------------------------------
def swin_window_plan(H: int, W: int, window: int, shift: int) -> tuple:
    """(pH, pW, sh, sw, nWy, nWx) of torchvision's shifted-window attention on an H x W map (ml/model/encoder/image.py,
    _ShiftedWindowAttention.forward): the map padded at the bottom / right to whole windows, the shift per dimension (0 where one window covers
    the padded map) and the window counts.  The same rule as the C host code of sd_swin_window_attention (sd_swin_window_plan)."""
    if H <= 0 or W <= 0 or window <= 0 or shift < 0:
        raise ValueError("positive map and window, non-negative shift")
    pH, pW = H + (window - H % window) % window, W + (window - W % window) % window
    return pH, pW, 0 if window >= pH else shift, 0 if window >= pW else shift, pH // window, pW // window


def _swin_req(t: Tensor, name: str, device=None, dtype=torch.float32, aligned: bool = False) -> Tensor:
    """Argument check of the Swin entry points: ValueError (never a launch) for a CPU tensor, another dtype or device, a strided view; ``aligned``:
    a 16-byte aligned start (the activation operands the kernels read 16 bytes at a time - parameters are read element-wise: an optimizer's flat
    buffer places them anywhere)."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise ValueError(f"{name}: expected a tensor on the MI355X (cuda) device")
    if t.dtype != dtype:
        raise ValueError(f"{name}: expected {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name}: expected a contiguous tensor")
    if device is not None and t.device != device:
        raise ValueError(f"{name}: on {t.device}, expected {device}")
    if aligned and t.data_ptr() % 16:
        raise ValueError(f"{name}: expected a 16-byte aligned tensor")
    return t


def _swin_ln(ln, K: int, device, name: str):
    if ln is None:
        return None, None, 1e-5
    g, b, eps = ln
    for t, n in ((g, f"{name} weight"), (b, f"{name} bias")):
        _swin_req(t, n, device)
        if t.numel() != K:
            raise ValueError(f"{n}: {t.numel()} values, expected {K}")
    return g.data_ptr(), b.data_ptr(), float(eps)


class PackedTokenLinear:
    """An nn.Linear weight (N, K), K a multiple of 32, in the fragment order of ``sd_token_linear`` (split fp16 planes) plus the inverse
    power-of-two scale of each row; ``refresh`` repacks in place."""

    def __init__(self, weight: Tensor):
        lib = _lib.load()
        w = weight.detach()
        _swin_req(w, "weight")
        if w.dim() != 2 or w.shape[1] % 32 or w.shape[0] <= 0:
            raise ValueError(f"weight (N, K) with K a multiple of 32, got {tuple(w.shape)}")
        self.N, self.K = int(w.shape[0]), int(w.shape[1])
        self.device = w.device
        self.planes = torch.empty(lib.sd_token_packed_halfs(self.N, self.K), dtype=torch.float16, device=w.device)
        self.w_inv = torch.empty(lib.sd_token_pad_cols(self.N), dtype=torch.float32, device=w.device)
        self.refresh(weight)

    def refresh(self, weight: Tensor) -> "PackedTokenLinear":
        w = weight.detach()
        _swin_req(w, "weight", self.device)
        if tuple(w.shape) != (self.N, self.K):
            raise ValueError("weight shape changed")
        check(_lib.load().sd_token_pack(w.data_ptr(), self.N, self.K, self.planes.data_ptr(), self.w_inv.data_ptr(), _stream()),
              "sd_token_pack")
        return self


def token_linear(A: Tensor, w: PackedTokenLinear, bias: Optional[Tensor] = None, ln: Optional[tuple] = None, gelu: bool = False,
                 res: Optional[Tensor] = None, out: Optional[Tensor] = None) -> Tensor:
    """out (..., N) = [+ res] [gelu] (LayerNorm?(A) W^T + bias) for token rows A (..., K): the Swin block's qkv (``ln`` = (norm1.weight,
    norm1.bias, eps)), proj (+ residual), fc1 (norm2, ``gelu``: erf-GELU), fc2 (+ residual) and the head, one launch.  ``res`` may be ``out``
    itself (the residual add in place)."""
    dev = w.device
    _swin_req(A, "A", dev, aligned=True)
    if A.dim() < 1 or A.shape[-1] != w.K:
        raise ValueError(f"A: last dimension {A.shape[-1] if A.dim() else None}, expected K = {w.K}")
    R = A.numel() // w.K
    if R <= 0:
        raise ValueError("A: no rows")
    if ln is not None and w.K > 1536:
        raise ValueError("the LayerNorm prologue takes K <= 1536")
    shape = (*A.shape[:-1], w.N)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=dev)
    elif tuple(_swin_req(out, "out", dev).shape) != shape:
        raise ValueError(f"out: shape {tuple(out.shape)}, expected {shape}")
    if bias is not None and _swin_req(bias, "bias", dev).numel() != w.N:
        raise ValueError(f"bias: {bias.numel()} values, expected {w.N}")
    if res is not None:
        if tuple(_swin_req(res, "res", dev).shape) != shape:
            raise ValueError(f"res: shape {tuple(res.shape)}, expected {shape}")
        if res.data_ptr() != out.data_ptr() and res.data_ptr() < out.data_ptr() + out.numel() * 4 and out.data_ptr() < res.data_ptr() + res.numel() * 4:
            raise ValueError("res overlaps out without being out")
    if A.data_ptr() < out.data_ptr() + out.numel() * 4 and out.data_ptr() < A.data_ptr() + A.numel() * 4:
        raise ValueError("A overlaps out")
    g, b, eps = _swin_ln(ln, w.K, dev, "ln")
    check(_lib.load().sd_token_linear(A.data_ptr(), w.planes.data_ptr(), w.w_inv.data_ptr(), _ptr(bias), g, b, eps, _ptr(res), out.data_ptr(),
                                      R, w.N, w.K, int(bool(gelu)), _stream()), "sd_token_linear")
    return out


def token_merge_linear(x: Tensor, w: PackedTokenLinear, ln: tuple) -> Tensor:
    """torchvision PatchMerging on NHWC tokens: x (N, H, W, C) -> reduction(norm(cat(x[0::2, 0::2], x[1::2, 0::2], x[0::2, 1::2],
    x[1::2, 1::2]))) (N, ceil(H/2), ceil(W/2), w.N), the 2 x 2 gather (zero padding for an odd H / W) inside the GEMM's operand load."""
    dev = w.device
    _swin_req(x, "x", dev, aligned=True)
    if x.dim() != 4 or 4 * x.shape[3] != w.K or x.shape[3] % 32:
        raise ValueError(f"x (N, H, W, C) with 4 C = {w.K}, C a multiple of 32; got {tuple(x.shape)}")
    if w.K > 1536:
        raise ValueError("the LayerNorm prologue takes 4 C <= 1536")
    N, H, W, Cc = x.shape
    g, b, eps = _swin_ln(ln, w.K, dev, "ln")
    out = torch.empty(N, (H + 1) // 2, (W + 1) // 2, w.N, dtype=torch.float32, device=dev)
    check(_lib.load().sd_token_merge_linear(x.data_ptr(), N, H, W, Cc, w.planes.data_ptr(), w.w_inv.data_ptr(), g, b, eps, out.data_ptr(), w.N,
                                            _stream()), "sd_token_merge_linear")
    return out


def swin_window_attention(qkv: Tensor, heads: int, window: int, shift: int, qkv_bias: Tensor, table: Tensor, index: Tensor) -> Tensor:
    """torchvision's shifted-window attention before proj, with no rolled or padded tensor: qkv (N, H, W, 3 C) - the qkv Linear of the
    un-padded map - -> (N, H, W, C); head dimension 32 (C = 32 heads), window <= 8.  ``table`` / ``index``: the module's
    relative_position_bias_table ((2 window - 1)^2, heads) and relative_position_index (window^4,) int64."""
    dev = qkv.device
    _swin_req(qkv, "qkv", aligned=True)
    if qkv.dim() != 4 or qkv.shape[3] % 3:
        raise ValueError(f"qkv (N, H, W, 3 C), got {tuple(qkv.shape)}")
    N, H, W, C3 = qkv.shape
    C = C3 // 3
    if C != 32 * heads:
        raise ValueError(f"head dimension 32: C = {C} for {heads} heads")
    if not 1 <= window <= 8 or not 0 <= shift < window:
        raise ValueError("window 1 .. 8, 0 <= shift < window")
    if _swin_req(qkv_bias, "qkv_bias", dev).numel() != C3:
        raise ValueError("qkv_bias: 3 C values")
    if tuple(_swin_req(table, "table", dev).shape) != ((2 * window - 1) ** 2, heads):
        raise ValueError(f"table: shape {tuple(table.shape)}, expected {((2 * window - 1) ** 2, heads)}")
    if _swin_req(index, "index", dev, torch.int64).numel() != window ** 4:
        raise ValueError("index: window^4 entries")
    out = torch.empty(N, H, W, C, dtype=torch.float32, device=dev)
    check(_lib.load().sd_swin_window_attention(qkv.data_ptr(), qkv_bias.data_ptr(), table.data_ptr(), index.data_ptr(), out.data_ptr(), N, H, W, C,
                                               heads, window, shift, _stream()), "sd_swin_window_attention")
    return out


def swin_patch_embed(x: Tensor, weight: Tensor, bias: Tensor, ln: tuple) -> Tensor:
    """Swin's stem: LayerNorm(conv4x4/s4(x) + bias) from NCHW frames x (N, 3, H, W) to NHWC tokens (N, H // 4, W // 4, 96), one launch."""
    dev = x.device
    _swin_req(x, "x")   # (element-wise loads: any view of the frames)
    if x.dim() != 4 or x.shape[1] != 3 or x.shape[2] < 4 or x.shape[3] < 4:
        raise ValueError(f"x (N, 3, H, W) with H, W >= 4, got {tuple(x.shape)}")
    if tuple(_swin_req(weight, "weight", dev).shape) != (96, 3, 4, 4) or _swin_req(bias, "bias", dev).numel() != 96:
        raise ValueError("the patch embedding is Conv2d(3, 96, 4, stride 4) with bias")
    g, b, eps = _swin_ln(ln, 96, dev, "ln")
    N, _, H, W = x.shape
    out = torch.empty(N, H // 4, W // 4, 96, dtype=torch.float32, device=dev)
    check(_lib.load().sd_swin_patch_embed(x.data_ptr(), weight.data_ptr(), bias.data_ptr(), g, b, eps, out.data_ptr(), N, H, W, _stream()),
          "sd_swin_patch_embed")
    return out


def swin_head(x: Tensor, ln: tuple, w: PackedTokenLinear, bias: Optional[Tensor]) -> Tensor:
    """Swin's head on NHWC tokens x (N, H, W, C): head(mean over H W of norm(x)) -> (N, w.N); two launches (LayerNorm + mean, the Linear)."""
    dev = w.device
    _swin_req(x, "x", dev)
    if x.dim() != 4 or x.shape[3] != w.K or x.shape[3] % 64 or x.shape[3] > 1024:
        raise ValueError(f"x (N, H, W, C) with C = {w.K} a multiple of 64 up to 1024, got {tuple(x.shape)}")
    N, H, W, Cc = x.shape
    g, b, eps = _swin_ln(ln, Cc, dev, "ln")
    pooled = torch.empty(N, Cc, dtype=torch.float32, device=dev)
    check(_lib.load().sd_swin_head_pool(x.data_ptr(), g, b, eps, pooled.data_ptr(), N, H * W, Cc, _stream()), "sd_swin_head_pool")
    return token_linear(pooled, w, bias)


# ---- image feed: OpenCV INTER_AREA down-scaling of the stored frames + the reference's normalisation (csrc/sd_frames.hip) ----------------
FRAME_SIZE = 480   # the recordings store 480 x 480 rgb8 frames (dataset/models.py:111-113)


def area_is_integer(R: int, src: int = FRAME_SIZE) -> bool:
    """cv::resize's choice of resizeAreaFast for src -> R (imgproc/src/resize.cpp): scale = 1 / (R / src) within DBL_EPSILON of an integer
    (saturate_cast<int> rounds half to even, as Python's round)."""
    scale = 1.0 / (R / src)
    return abs(scale - round(scale)) < sys.float_info.epsilon


def area_taps(R: int, src: int = FRAME_SIZE) -> tuple:
    """computeResizeAreaTab (imgproc/src/resize.cpp) of one axis src -> R, in Python doubles (no contraction), each weight rounded to fp32
    once: (first, count, woff) int32 (R,) - output index d reads source indices first[d] .. first[d] + count[d] - 1 with the weights
    weights[woff[d] ...] in that order (the left partial tap, the full ones, the right partial one) - and weights float32."""
    if not 1 <= R <= src:
        raise ValueError(f"1 <= R <= {src}, got {R}")
    scale = 1.0 / (R / src)
    first, count, woff, w = [], [], [], []
    for d in range(R):
        fsx1 = d * scale
        fsx2 = fsx1 + scale
        cell = min(scale, src - fsx1)
        sx1, sx2 = math.ceil(fsx1), math.floor(fsx2)
        sx2 = min(sx2, src - 1)
        sx1 = min(sx1, sx2)
        taps = []
        if sx1 - fsx1 > 1e-3:
            taps.append((sx1 - 1, (sx1 - fsx1) / cell))
        taps += [(sx, 1.0 / cell) for sx in range(sx1, sx2)]
        if fsx2 - sx2 > 1e-3:
            taps.append((sx2, min(min(fsx2 - sx2, 1.0), cell) / cell))
        first.append(taps[0][0])
        count.append(len(taps))
        woff.append(len(w))
        w += [t[1] for t in taps]
        # the kernel's row streaming relies on it: consecutive outputs share at most their boundary source index
        if d and first[d] < first[d - 1] + count[d - 1] - 1:
            raise AssertionError(f"area taps of {src} -> {R}: outputs {d - 1} and {d} overlap by more than one source index")
    return (np.asarray(first, np.int32), np.asarray(count, np.int32), np.asarray(woff, np.int32), np.asarray(w, np.float64).astype(np.float32))


_area_tables: dict = {}


def _area_table(R: int, device) -> tuple:
    key = (R, str(device))
    if key not in _area_tables:
        first, count, woff, w = area_taps(R)
        _area_tables[key] = (torch.from_numpy(np.concatenate([first, count, woff])).to(device), torch.from_numpy(w).to(device))
    return _area_tables[key]


def frames_area(store: Tensor, index: Tensor, R: int, out: Optional[Tensor] = None) -> Tensor:
    """The reference's frame preprocessing (dataset/pytorch.py:209-211 + its transforms) on gathered frames, one launch:
    cv2.resize(frame, (R, R), interpolation=cv2.INTER_AREA) of store[index] - OpenCV's integer-factor path or its generic area path, bit
    for bit as restated in DESIGN.md section 2 - then x / 255, (x - ImageNet mean) / std, channels first.  store (N, 480, 480, 3) uint8 on
    the device, index (...) int64 into it, -1 (or any index outside [0, N)) = a zero frame -> (..., 3, R, R) float32, 1 <= R <= 480."""
    _swin_req(store, "store", dtype=torch.uint8, aligned=True)
    if store.dim() != 4 or tuple(store.shape[1:]) != (FRAME_SIZE, FRAME_SIZE, 3):
        raise ValueError(f"store: (N, {FRAME_SIZE}, {FRAME_SIZE}, 3) rgb8 frames, got {tuple(store.shape)}")
    dev = store.device
    _swin_req(index, "index", dev, torch.int64)
    if isinstance(R, bool) or not isinstance(R, (int, np.integer)) or not 1 <= R <= FRAME_SIZE:
        raise ValueError(f"R: an int in 1 .. {FRAME_SIZE} (down-scaling only), got {R!r}")
    R = int(R)
    shape = (*index.shape, 3, R, R)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=dev)
    elif tuple(_swin_req(out, "out", dev).shape) != shape:
        raise ValueError(f"out: shape {tuple(out.shape)}, expected {shape}")
    tab = w = None
    if not area_is_integer(R):
        tab, w = _area_table(R, dev)
    check(_lib.load().sd_frames_area(store.data_ptr(), store.shape[0], index.data_ptr(), index.numel(), R, _ptr(tab), _ptr(w),
                                     0 if w is None else w.numel(), out.data_ptr(), _stream()), "sd_frames_area")
    return out


# ---- camera intake: OpenCV INTER_LINEAR of raw camera frames + the reference's normalisation (csrc/sd_frames.hip) ------------------------
CAMERA_MAX = 4096   # sd_camera_intake: 1 <= H, W, R <= 4096
LINEAR_BITS = 11    # INTER_RESIZE_COEF_BITS: the coefficient pair of a tap sums to 1 << 11


def linear_taps(src: int, dst: int) -> tuple:
    """cv::resize's INTER_LINEAR table of one axis src -> dst for 8-bit images (imgproc/src/resize.cpp, restated in DESIGN.md section 2):
    (index int32 (dst,), coef int16 (dst, 2)).  Output d reads source index[d] with coef[d, 0] and min(index[d] + 1, src - 1) with
    coef[d, 1].  scale = 1 / (dst / src) in doubles; f = float32((d + 0.5) scale - 0.5), s = floor(f), f -= s in fp32; s < 0 -> (0, 0),
    s >= src - 1 -> (src - 1, 0); coef = cvRound((1 - f) 2048), cvRound(f 2048) from fp32 products, round half to even."""
    for name, v in (("src", src), ("dst", dst)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1:
            raise ValueError(f"{name}: an int >= 1, got {v!r}")
    scale = 1.0 / (dst / src)
    one, unit = np.float32(1.0), np.float32(1 << LINEAR_BITS)
    index, coef = np.empty(dst, np.int32), np.empty((dst, 2), np.int16)
    for d in range(dst):
        f = np.float32((d + 0.5) * scale - 0.5)
        s = math.floor(f)
        f = np.float32(f - np.float32(s))
        if s < 0:
            s, f = 0, np.float32(0.0)
        if s >= src - 1:
            s, f = src - 1, np.float32(0.0)
        index[d] = s
        coef[d] = (int(np.rint(np.float32(one - f) * unit)), int(np.rint(f * unit)))
    return index, coef


def camera_route(H: int, W: int, R: int) -> str:
    """The route cv2.resize(frame, (R, R)) with INTER_LINEAR takes for an (H, W) frame: "copy" at the same size, "area2" at an exact
    factor 2 on both axes (cv::resize turns INTER_LINEAR into INTER_AREA there), "linear" for everything else."""
    if H == R and W == R:
        return "copy"
    if H == 2 * R and W == 2 * R:
        return "area2"
    return "linear"


_linear_tables: dict = {}


def _linear_table(src: int, R: int, device) -> tuple:
    key = (src, R, str(device))
    if key not in _linear_tables:
        index, coef = linear_taps(src, R)
        _linear_tables[key] = (torch.from_numpy(index).to(device), torch.from_numpy(coef).to(device))
    return _linear_tables[key]


def camera_intake(frames: Tensor, R: int, order: str = "rgb", out: Optional[Tensor] = None) -> Tensor:
    """The robot node's frame preprocessing (ros.py:186-200) in one launch: cv2.resize(frame, (R, R)) with the default INTER_LINEAR - bit for
    bit as restated in DESIGN.md section 2 - then x / 255, (x - ImageNet mean) / std, channels first.  frames (..., H, W, 3) uint8 on the
    device, at any address (a slice of a larger buffer is read in place); ``order``: "rgb", or "bgr" for frames whose channels arrive in
    OpenCV's order -> (..., 3, R, R) float32 with the channels in the model's order.  1 <= H, W, R <= 4096."""
    if not isinstance(frames, Tensor) or frames.dtype != torch.uint8:
        raise ValueError(f"frames: expected a uint8 tensor, got {getattr(frames, 'dtype', type(frames))}")
    if frames.dim() < 3 or frames.shape[-1] != 3:
        raise ValueError(f"frames: expected (..., H, W, 3), got {tuple(frames.shape)}")
    H, W = int(frames.shape[-3]), int(frames.shape[-2])
    if not (1 <= H <= CAMERA_MAX and 1 <= W <= CAMERA_MAX):
        raise ValueError(f"frames: 1 <= H, W <= {CAMERA_MAX}, got {H} x {W}")
    if order not in ("rgb", "bgr"):
        raise ValueError(f"order: 'rgb' or 'bgr', got {order!r}")
    if isinstance(R, bool) or not isinstance(R, (int, np.integer)) or not 1 <= R <= CAMERA_MAX:
        raise ValueError(f"R: an int in 1 .. {CAMERA_MAX}, got {R!r}")
    R = int(R)
    _swin_req(frames, "frames", dtype=torch.uint8)
    dev = frames.device
    shape = (*frames.shape[:-3], 3, R, R)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=dev)
    elif tuple(_swin_req(out, "out", dev).shape) != shape:
        raise ValueError(f"out: shape {tuple(out.shape)}, expected {shape}")
    xi = xc = yi = yc = None
    if camera_route(H, W, R) == "linear":
        (xi, xc), (yi, yc) = _linear_table(W, R, dev), _linear_table(H, R, dev)
    n = frames.numel() // (H * W * 3)
    check(_lib.load().sd_camera_intake(frames.data_ptr(), n, H, W, int(order == "bgr"), R, _ptr(xi), _ptr(xc), _ptr(yi), _ptr(yc), out.data_ptr(),
                                       _stream()), "sd_camera_intake")
    return out


# ---- the ResNet encoder heads (csrc/sd_head.hip): avgpool -> fc, or Conv2d(C, 32, 1) + bias flattened NCHW -> fc ------------------------
def _operand(t: Tensor, row=(0, 0, 0), col=(0, 0, 0)):
    """sd_strided_operand: element (i, j) at ((i / d) s1 + (i % d) s0) + ((j / d') s1' + (j % d') s0') floats from t's start (d = 0: i s0)."""
    return _lib.StridedOperand(t.data_ptr(), *row, *col)


_ones: dict = {}


def _one(device) -> Tensor:
    key = str(device)
    if key not in _ones:
        _ones[key] = torch.ones(1, dtype=torch.float32, device=device)
    return _ones[key]


def head_gemm(M: int, N: int, K: int, A, B, Cop, bias: Optional[Tensor] = None, accumulate: bool = False, device=None) -> None:
    """C (M x N) [+]= A (M x K) B (K x N) [+ bias], operands given as ``_operand`` descriptors (sd_head_gemm): deterministic split
    reductions through a scratch buffer, fp32 FMA."""
    lib = _lib.load()
    n_scr = lib.sd_head_gemm_scratch_floats(M, N, K)
    scratch = torch.empty(n_scr, dtype=torch.float32, device=device) if n_scr else None
    args = _lib.HeadGemmArgs(M, N, K, A, B, Cop, _ptr(bias), _ptr(scratch), int(bool(accumulate)), 0)
    check(lib.sd_head_gemm(C.byref(args), _stream()), "sd_head_gemm")


def _head_check(x: Tensor, conv_w: Optional[Tensor], conv_b: Optional[Tensor], fc_w: Tensor, fc_b: Tensor) -> tuple:
    dev = x.device
    _swin_req(x, "x")
    if x.dim() != 4:
        raise ValueError(f"x: the NHWC map (N, H, W, C), got {tuple(x.shape)}")
    N, H, W, Cc = x.shape
    if conv_w is not None:
        if tuple(_swin_req(conv_w, "conv_w", dev).shape) not in ((32, Cc, 1, 1), (32, Cc)) or _swin_req(conv_b, "conv_b", dev).numel() != 32:
            raise ValueError(f"the no-avgpool head is Conv2d({Cc}, 32, 1) with bias")
    J = 32 * H * W if conv_w is not None else Cc
    if _swin_req(fc_w, "fc_w", dev).dim() != 2 or fc_w.shape[1] != J or _swin_req(fc_b, "fc_b", dev).numel() != fc_w.shape[0]:
        raise ValueError(f"fc: Linear({J}, d) with bias expected, got weight {tuple(fc_w.shape)}")
    return N, H * W, Cc, J, fc_w.shape[0]


def resnet_head(x: Tensor, conv_w: Optional[Tensor], conv_b: Optional[Tensor], fc_w: Tensor, fc_b: Tensor) -> tuple:
    """The ResNet encoder head on the last block's NHWC map x (N, H, W, C): ``conv_w is None`` -> fc(mean over H W) (AdaptiveAvgPool2d((1, 1))),
    else fc(flatten_NCHW(Conv2d(C, 32, 1)(x))).  Returns (y (N, d), the fc input (N, J)) - the latter is what the backward needs."""
    N, HW, Cc, J, d = _head_check(x, conv_w, conv_b, fc_w, fc_b)
    dev = x.device
    feat = torch.empty(N, J, dtype=torch.float32, device=dev)
    if conv_w is None:
        check(_lib.load().sd_head_pool(x.data_ptr(), feat.data_ptr(), N, HW, Cc, _stream()), "sd_head_pool")
    else:   # feat[n, o HW + p] = cb[o] + sum_c x[n, p, c] cw[o, c]: rows m = n HW + p
        head_gemm(N * HW, 32, Cc, _operand(x, (0, 0, Cc), (0, 0, 1)), _operand(conv_w, (0, 0, 1), (0, 0, Cc)),
                  _operand(feat, (HW, 32 * HW, 1), (0, 0, HW)), bias=conv_b, device=dev)
    y = torch.empty(N, d, dtype=torch.float32, device=dev)
    head_gemm(N, d, J, _operand(feat, (0, 0, J), (0, 0, 1)), _operand(fc_w, (0, 0, 1), (0, 0, J)), _operand(y, (0, 0, d), (0, 0, 1)),
              bias=fc_b, device=dev)
    return y, feat


def resnet_head_backward(dy: Tensor, x: Tensor, feat: Tensor, conv_w: Optional[Tensor], fc_w: Tensor, grads: tuple, want_dx: bool = True):
    """The head's backward for dy (N, d): accumulates into grads = (d conv_w, d conv_b, d fc_w, d fc_b) (None for the avgpool head's conv
    pair; the buffers are added to, as the optimizer's flat gradient is) and returns the NHWC gradient of x (or None)."""
    dev = x.device
    N, H, W, Cc = x.shape
    HW, d = H * W, fc_w.shape[0]
    J = feat.shape[1]
    _swin_req(dy, "dy", dev)
    if tuple(dy.shape) != (N, d) or tuple(feat.shape) != (N, J):
        raise ValueError("dy (N, d) and the saved fc input (N, J) expected")
    dcw, dcb, dfw, dfb = grads
    one = _one(dev)
    # fc: d fc_w += dy^T feat, d fc_b += 1^T dy
    head_gemm(d, J, N, _operand(dy, (0, 0, 1), (0, 0, d)), _operand(feat, (0, 0, J), (0, 0, 1)), _operand(dfw, (0, 0, J), (0, 0, 1)),
              accumulate=True, device=dev)
    head_gemm(1, d, N, _operand(one), _operand(dy, (0, 0, d), (0, 0, 1)), _operand(dfb, (0, 0, 0), (0, 0, 1)), accumulate=True, device=dev)
    if conv_w is None and not want_dx:
        return None
    dfeat = torch.empty(N, J, dtype=torch.float32, device=dev)          # dy fc_w
    head_gemm(N, J, d, _operand(dy, (0, 0, d), (0, 0, 1)), _operand(fc_w, (0, 0, J), (0, 0, 1)), _operand(dfeat, (0, 0, J), (0, 0, 1)), device=dev)
    if conv_w is None:
        dx = torch.empty_like(x)
        check(_lib.load().sd_head_pool_bwd(dfeat.data_ptr(), dx.data_ptr(), N, HW, Cc, _stream()), "sd_head_pool_bwd")
        return dx
    # dz[n][p][o] = dfeat[n, o HW + p]; reduction index k = n HW + p
    dz_k = (HW, 32 * HW, 1)
    head_gemm(32, Cc, N * HW, _operand(dfeat, (0, 0, HW), dz_k), _operand(x, (0, 0, Cc), (0, 0, 1)), _operand(dcw, (0, 0, Cc), (0, 0, 1)),
              accumulate=True, device=dev)
    head_gemm(1, 32, N * HW, _operand(one), _operand(dfeat, dz_k, (0, 0, HW)), _operand(dcb, (0, 0, 0), (0, 0, 1)), accumulate=True, device=dev)
    if not want_dx:
        return None
    dx = torch.empty_like(x)                                              # dz conv_w
    head_gemm(N * HW, Cc, 32, _operand(dfeat, dz_k, (0, 0, HW)), _operand(conv_w, (0, 0, Cc), (0, 0, 1)), _operand(dx, (0, 0, Cc), (0, 0, 1)),
              device=dev)
    return dx


# --------------------------------------------------------------------------------------
# closed-loop policy session: device-side sensor rings (csrc/sd_session.hip; the stateful layer is session.py)
# --------------------------------------------------------------------------------------
def _ring_req(ring: Tensor, head: Tensor) -> tuple:
    _req(ring, "ring"); _req(head, "head", torch.int32)
    if ring.dim() != 3 or head.dim() != 1 or head.shape[0] != ring.shape[0] or head.device != ring.device:
        raise ValueError(f"a ring is (B, L, C) fp32 with an int32 head word per robot, got {tuple(ring.shape)} and {tuple(head.shape)}")
    return tuple(ring.shape)


def robot_index(robots, B: int) -> Tensor:
    """A subset of the robots of a batch as the int32 CPU tensor (S) the ``*_at`` entry points read once it is uploaded: a sequence of ints
    or a 1-D integer CPU tensor, every index in [0, B), no index twice (two workgroups of one launch would own the same ring).  This is
    the only validation there is - the device checks nothing but the range - and it needs no GPU."""
    if isinstance(robots, Tensor):
        if robots.is_cuda:
            raise ValueError("robots: indices are validated on the host - pass a list or a CPU tensor (a device tensor would have to be read back)")
        if robots.dim() != 1 or robots.dtype in (torch.bool, torch.float16, torch.bfloat16, torch.float32, torch.float64):
            raise ValueError(f"robots: expected a 1-D integer tensor of robot indices, got {tuple(robots.shape)} {robots.dtype}")
        idx = [int(v) for v in robots.tolist()]
    else:
        try:
            robots = idx = list(robots)
        except TypeError:
            raise ValueError(f"robots: expected a sequence of robot indices, got {robots!r}") from None
        try:
            idx = [operator.index(v) for v in idx if not isinstance(v, bool)]
        except TypeError:
            idx = None
        if idx is None or len(idx) != len(robots):
            raise ValueError(f"robots: expected a flat sequence of ints, got {robots!r}")
    bad = [v for v in idx if not 0 <= v < B]
    if bad:
        raise ValueError(f"robots: index {bad[0]} is outside [0, {B})")
    if len(set(idx)) != len(idx):
        raise ValueError(f"robots: an index occurs twice in {idx}; one launch gives every named robot one workgroup")
    return torch.tensor(idx, dtype=torch.int32)


def _robots_on(robots, B: int, device) -> Tensor:
    """``robots`` in device memory: an int32 device tensor is taken as it is (it came from ``robot_index``: PolicySession validates once per
    call and hands the upload to several launches), anything else goes through ``robot_index`` first."""
    if isinstance(robots, Tensor) and robots.is_cuda:
        if robots.dtype != torch.int32 or robots.dim() != 1 or not robots.is_contiguous() or robots.device != device:
            raise ValueError(f"robots: a device tensor must be the contiguous int32 upload of ops.robot_index on {device}")
        return robots
    return robot_index(robots, B).to(device)


def ring_push(ring: Tensor, head: Tensor, rows: Tensor, sub: Optional[Tensor] = None, robots=None) -> None:
    """Appends rows (B, n, C), oldest first, to the ring (B, L, C) and advances its heads; ``sub`` (C) is subtracted from every row.
    ``robots`` (see ``robot_index``): rows is (S, n, C) and block s goes to robot robots[s]; no other robot's ring or head is touched."""
    B, L, Cc = _ring_req(ring, head)
    _req(rows, "rows")
    r = None if robots is None else _robots_on(robots, B, ring.device)
    S = B if r is None else r.numel()
    if rows.dim() != 3 or rows.shape[0] != S or rows.shape[2] != Cc or rows.device != ring.device:
        raise ValueError(f"rows: expected ({S}, n, {Cc}) on {ring.device}, got {tuple(rows.shape)} on {rows.device}")
    if sub is not None and (_req(sub, "sub").numel() != Cc or sub.device != ring.device):
        raise ValueError(f"sub: expected {Cc} values on {ring.device}")
    if r is None:
        check(_lib.load().sd_ring_push(ring.data_ptr(), head.data_ptr(), rows.data_ptr(), _ptr(sub), B, L, Cc, rows.shape[1], _stream()), "sd_ring_push")
    else:
        check(_lib.load().sd_ring_push_at(ring.data_ptr(), head.data_ptr(), rows.data_ptr(), _ptr(sub), r.data_ptr(), S, B, L, Cc, rows.shape[1],
                                          _stream()), "sd_ring_push_at")


def ring_push_quat(ring: Tensor, head: Tensor, quats: Tensor, robots=None) -> None:
    """Appends orientation samples quats (B, n, 4), xyzw and oldest first, to the rotation ring (B, L, 4 | 5) and advances its heads.  The
    ring's width says what is stored: 4 columns the quaternions as they are, 5 columns ``dataset.quats_to_5d``'s rows (axis, sin angle,
    cos angle), computed on the device in fp64 and rounded to fp32 once.  ``robots``: as in ``ring_push``."""
    B, L, Cc = _ring_req(ring, head)
    if Cc not in (4, 5):
        raise ValueError(f"a rotation ring has 4 (quaternion) or 5 (five_dim) columns, got {Cc}")
    _req(quats, "quats")
    r = None if robots is None else _robots_on(robots, B, ring.device)
    S = B if r is None else r.numel()
    if quats.dim() != 3 or quats.shape[0] != S or quats.shape[2] != 4 or quats.device != ring.device:
        raise ValueError(f"quats: expected ({S}, n, 4) on {ring.device}, got {tuple(quats.shape)} on {quats.device}")
    check(_lib.load().sd_ring_push_quat(ring.data_ptr(), head.data_ptr(), quats.data_ptr(), _ptr(r), S, B, L, Cc, quats.shape[1], _stream()),
          "sd_ring_push_quat")


def ring_window(ring: Tensor, head: Tensor, out: Optional[Tensor] = None, robots=None) -> Tensor:
    """The chronological window (B, L, C) of a ring; with ``robots`` the compact (S, L, C) windows of those robots, in their order."""
    B, L, Cc = _ring_req(ring, head)
    r = None if robots is None else _robots_on(robots, B, ring.device)
    shape = (B if r is None else r.numel(), L, Cc)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=ring.device)
    elif tuple(_req(out, "out").shape) != shape or out.device != ring.device:
        raise ValueError(f"out: expected {shape} on {ring.device}")
    if r is None:
        check(_lib.load().sd_ring_window(ring.data_ptr(), head.data_ptr(), out.data_ptr(), *shape, _stream()), "sd_ring_window")
    else:
        check(_lib.load().sd_ring_window_at(ring.data_ptr(), head.data_ptr(), out.data_ptr(), r.data_ptr(), shape[0], B, L, Cc, _stream()),
              "sd_ring_window_at")
    return out


class SessionWindows:
    """The argument block of ``sd_session_windows`` for up to three (ring, head, out, wrap) views of one batch: built once, launched at every
    tick with the same arguments (the heads are device words)."""

    def __init__(self, views: Sequence[tuple]):
        if not 1 <= len(views) <= 3:
            raise ValueError("one to three rings per launch")
        self.tensors = []
        self.array = (_lib.RingView * len(views))()
        for i, (ring, head, out, wrap) in enumerate(views):
            shape = _ring_req(ring, head)
            if tuple(_req(out, "out").shape) != shape or out.device != ring.device or (i and shape[0] != self.B):
                raise ValueError(f"view {i}: out {tuple(out.shape)} does not match its ring {shape}, or the batch differs")
            self.B = shape[0]
            self.tensors.append((ring, head, out))   # the block holds raw pointers: keep their owners alive
            v = self.array[i]
            v.ring, v.head, v.out, v.L, v.C, v.wrap = ring.data_ptr(), head.data_ptr(), out.data_ptr(), shape[1], shape[2], int(bool(wrap))

    def launch(self, robots=None) -> None:
        """``robots`` (S of them, see ``robot_index``): the same block and the same out buffers, of which the leading S row blocks
        ``out[:S]`` then hold the compact windows of those robots (S <= B, so they fit; the rest of out is left as it was)."""
        if robots is None:
            check(_lib.load().sd_session_windows(self.array, len(self.array), self.B, _stream()), "sd_session_windows")
            return
        r = _robots_on(robots, self.B, self.tensors[0][0].device)
        if r.numel() > self.B:
            raise ValueError(f"robots: {r.numel()} robots do not fit the window buffers of a batch of {self.B}")
        check(_lib.load().sd_session_windows_at(self.array, len(self.array), r.data_ptr(), r.numel(), self.B, _stream()), "sd_session_windows_at")


def session_commit(x: Tensor, mean: Tensor, std: Tensor, ring: Tensor, head: Tensor, robots=None) -> Tensor:
    """The published trajectory x * std + mean - pi (B, T, J) of a sampled normalised one, also pushed into the action-history ring.
    ``robots`` (see ``robot_index``): x is (S, T, J) and its rows go into the action rings of those robots only."""
    B, L, J = _ring_req(ring, head)
    _req(x, "x"); _req(mean, "mean"); _req(std, "std")
    r = None if robots is None else _robots_on(robots, B, ring.device)
    S = B if r is None else r.numel()
    if x.dim() != 3 or x.shape[0] != S or x.shape[2] != J or mean.numel() != J or std.numel() != J or x.device != ring.device:
        raise ValueError(f"x: expected ({S}, T, {J}) with {J} means and stds, got {tuple(x.shape)}")
    out = torch.empty_like(x)
    if r is None:
        check(_lib.load().sd_session_commit(x.data_ptr(), mean.data_ptr(), std.data_ptr(), out.data_ptr(), ring.data_ptr(), head.data_ptr(),
                                            B, x.shape[1], J, L, _stream()), "sd_session_commit")
    else:
        check(_lib.load().sd_session_commit_at(x.data_ptr(), mean.data_ptr(), std.data_ptr(), out.data_ptr(), ring.data_ptr(), head.data_ptr(),
                                               r.data_ptr(), S, B, x.shape[1], J, L, _stream()), "sd_session_commit_at")
    return out


def session_commit_carry(x: Tensor, mean: Tensor, std: Tensor, ring: Tensor, head: Tensor, advance: int, carry: int, pin_x0: Tensor,
                         pin_rows: Tensor, robots=None) -> Tensor:
    """``session_commit`` that also prepares the next tick, in the same one launch (``sd_session_commit_carry``): all T rows are
    published, the first ``advance`` of them - the commands executed before the next tick - go into the action ring, rows
    [advance, advance + carry) of x, as sampled, become rows [0, carry) of ``pin_x0[robot]`` (B, T, J) and ``pin_rows[robot]`` (B) int32
    becomes ``carry``.  ``robots``: x is (S, T, J); only those robots' rings, pin rows and counts move."""
    B, L, J = _ring_req(ring, head)
    _req(x, "x"); _req(mean, "mean"); _req(std, "std"); _req(pin_x0, "pin_x0"); _req(pin_rows, "pin_rows", torch.int32)
    r = None if robots is None else _robots_on(robots, B, ring.device)
    S = B if r is None else r.numel()
    if x.dim() != 3 or x.shape[0] != S or x.shape[2] != J or mean.numel() != J or std.numel() != J or x.device != ring.device:
        raise ValueError(f"x: expected ({S}, T, {J}) with {J} means and stds, got {tuple(x.shape)}")
    T = x.shape[1]
    if tuple(pin_x0.shape) != (B, T, J) or tuple(pin_rows.shape) != (B,) or pin_x0.device != ring.device or pin_rows.device != ring.device:
        raise ValueError(f"pin_x0 / pin_rows: expected ({B}, {T}, {J}) fp32 and ({B},) int32 on {ring.device}")
    advance, carry = int(advance), int(carry)
    if advance < 0 or carry < 0 or advance + carry > T:
        raise ValueError(f"advance, carry >= 0 and advance + carry <= {T}, got {advance} and {carry}")
    out = torch.empty_like(x)
    if r is None:
        check(_lib.load().sd_session_commit_carry(x.data_ptr(), mean.data_ptr(), std.data_ptr(), out.data_ptr(), ring.data_ptr(), head.data_ptr(),
                                                  B, T, J, L, advance, carry, pin_x0.data_ptr(), pin_rows.data_ptr(), _stream()),
              "sd_session_commit_carry")
    else:
        check(_lib.load().sd_session_commit_carry_at(x.data_ptr(), mean.data_ptr(), std.data_ptr(), out.data_ptr(), ring.data_ptr(),
                                                     head.data_ptr(), r.data_ptr(), S, B, T, J, L, advance, carry, pin_x0.data_ptr(),
                                                     pin_rows.data_ptr(), _stream()), "sd_session_commit_carry_at")
    return out


def hold_joints(joints, J: int) -> list:
    """The joint indices of a hold / release, validated on the host (no device needed): a non-empty sequence of distinct ints in [0, J),
    J <= 32."""
    if isinstance(J, bool) or not 1 <= int(J) <= 32:
        raise ValueError(f"hold: one 32-bit word per robot describes at most 32 joints, got J = {J}")
    try:
        idx = [operator.index(v) for v in joints if not isinstance(v, bool)]
        n = len(joints)
    except TypeError:
        raise ValueError(f"joints: expected a sequence of joint indices, got {joints!r}") from None
    if not idx or len(idx) != n:
        raise ValueError(f"joints: expected a non-empty flat sequence of ints, got {joints!r}")
    bad = [v for v in idx if not 0 <= v < J]
    if bad:
        raise ValueError(f"joints: index {bad[0]} is outside [0, {J})")
    if len(set(idx)) != len(idx):
        raise ValueError(f"joints: an index occurs twice in {idx}")
    return idx


def session_hold(pin_x0: Tensor, held: Tensor, joints, values: Optional[Tensor], mean: Optional[Tensor], std: Optional[Tensor],
                 robots=None) -> None:
    """One launch (``sd_session_hold``): ``values`` - radians as published, (n,), (S, n) or (S, T, n) fp32 on the device - of the joints
    ``joints`` are normalised with mean and std and written into ``pin_x0[b, :, j]`` (B, T, J) for the selected robots, whose bits in
    ``held`` (B) int32 are set; ``values`` None: the bits are cleared (a release).  ``robots`` as ``robot_index``; None: all, S = B."""
    _req(pin_x0, "pin_x0"); _req(held, "held", torch.int32)
    if pin_x0.dim() != 3 or tuple(held.shape) != (pin_x0.shape[0],) or held.device != pin_x0.device:
        raise ValueError(f"pin_x0 / held: expected (B, T, J) fp32 and (B,) int32 on one device, got {tuple(pin_x0.shape)} and {tuple(held.shape)}")
    B, T, J = pin_x0.shape
    idx = hold_joints(joints, J)
    n = len(idx)
    r = None if robots is None else _robots_on(robots, B, pin_x0.device)
    S = B if r is None else r.numel()
    strides = (0, 0)
    if values is not None:
        _req(values, "values"); _req(mean, "mean"); _req(std, "std")
        if values.device != pin_x0.device or mean.numel() != J or std.numel() != J:
            raise ValueError(f"values: expected fp32 values on {pin_x0.device} with {J} means and stds")
        if tuple(values.shape) == (n,):
            strides = (0, 0)
        elif tuple(values.shape) == (S, n):
            strides = (n, 0)
        elif tuple(values.shape) == (S, T, n):
            strides = (T * n, n)
        else:
            raise ValueError(f"values: expected ({n},), ({S}, {n}) or ({S}, {T}, {n}), got {tuple(values.shape)}")
    array = (C.c_int32 * n)(*idx)
    check(_lib.load().sd_session_hold(pin_x0.data_ptr(), held.data_ptr(), _ptr(values), strides[0], strides[1], array, n, _ptr(mean), _ptr(std),
                                      _ptr(r), S, B, T, J, 0 if values is None else 1, _stream()), "sd_session_hold")


def session_hold_mask(mask: Tensor, held: Tensor, pin_rows: Optional[Tensor], J: int, draws: int = 1, robots=None) -> Tensor:
    """One launch (``sd_session_hold_mask``) composes a tick's mask into ``mask`` (S * draws, T) int32: word (s * draws + g, t) =
    held[b] | (t < pin_rows[b] ? all J bits : 0) for robot b of row s.  ``pin_rows`` None: no carried rows.  ``robots``: a (S,) int32
    device tensor of robot indices (a session's validated subset), or None: all, S = B.  Reads device buffers only."""
    _req(mask, "mask", torch.int32); _req(held, "held", torch.int32)
    B = held.shape[0]
    S = B if robots is None else robots.numel()
    if mask.dim() != 2 or mask.shape[0] != S * draws or mask.device != held.device:
        raise ValueError(f"mask: expected ({S * draws}, T) int32 on {held.device}, got {tuple(mask.shape)}")
    if pin_rows is not None and (tuple(_req(pin_rows, "pin_rows", torch.int32).shape) != (B,) or pin_rows.device != held.device):
        raise ValueError(f"pin_rows: expected ({B},) int32 on {held.device}")
    if robots is not None:
        _req(robots, "robots", torch.int32)
    check(_lib.load().sd_session_hold_mask(mask.data_ptr(), held.data_ptr(), _ptr(pin_rows), _ptr(robots), S, B, mask.shape[1], int(J), int(draws),
                                           _stream()), "sd_session_hold_mask")
    return mask


def session_limits(limits: Limits, lo_rad, hi_rad, mean: Tensor, std: Tensor, J: int) -> Limits:
    """One launch (``sd_session_limits``) writes ``limits`` - the two (32,) device arrays a session's rollout reads - from limits in
    radians as published (``lo_rad``, ``hi_rad``: host arrays of at least J fp32, e.g. ``PolicySession.check_limits``'s): the inverse of
    the commit's expression, each bound moved inward until the commit's expression gives a value inside the radians."""
    lo_rad, hi_rad = np.ascontiguousarray(lo_rad, dtype=np.float32), np.ascontiguousarray(hi_rad, dtype=np.float32)
    if lo_rad.ndim != 1 or hi_rad.ndim != 1 or lo_rad.shape[0] < J or hi_rad.shape[0] < J:
        raise ValueError(f"session_limits: lo_rad and hi_rad must hold at least {J} floats")
    limits = _limits_req(limits, J, mean.device)
    _req(mean, "mean"); _req(std, "std")
    check(_lib.load().sd_session_limits(limits.lo.data_ptr(), limits.hi.data_ptr(), lo_rad.ctypes.data_as(_lib.c_float_p),
                                        hi_rad.ctypes.data_as(_lib.c_float_p), mean.data_ptr(), std.data_ptr(), int(J), _stream()),
          "sd_session_limits")
    return limits


SLEW_U = 2.0 ** -24   # the unit roundoff of fp32


def _half_ulp(z) -> np.ndarray:
    """Half an ulp of the fp32 binade of z (1 + 2^-20), in fp64: the most one rounding to nearest adds to a result of magnitude <= z."""
    z = np.asarray(z, dtype=np.float64) * (1.0 + 2.0 ** -20)
    return np.where(z > 0, np.ldexp(1.0, np.frexp(np.where(z > 0, z, 1.0))[1] - 1 - 24), 0.0)


def session_slew_margin(bound_rad, mean, std) -> np.ndarray:
    """The margin of ``sd_session_slew`` in radians, fp64, per joint: std hu(XS / std) + 2 hu(XS) + 2 hu(pi + R) + 2 hu(R) with
    XS = R + |pi - mean| and hu half an fp32 ulp - what the rounding of y +- v in the scan and both roundings of the commit's expression
    can add to the difference of two published values."""
    R, s = np.asarray(bound_rad, dtype=np.float64), np.asarray(std, dtype=np.float64)
    XS = R + np.abs(math.pi - np.asarray(mean, dtype=np.float64))
    return s * _half_ulp(XS / s) + 2.0 * _half_ulp(XS) + 2.0 * _half_ulp(math.pi + R) + 2.0 * _half_ulp(R)


def denormalised_slew_margin(bound, mean, std) -> np.ndarray:
    """``session_slew_margin`` for trajectories that are denormalised and nothing else, r = x * std + mean (``ops.normalize(inverse=True)``,
    ``ops.max_step``, ``ops.trajectory_errors``): std hu(XS / std) + 2 hu(XS) + 2 hu(Q) with Q = ``bound`` >= |r| and XS = Q + |mean|
    >= |x std| - the scan's rounding and the product's and the sum's of either value (the fma form has one less)."""
    Q, s = np.asarray(bound, dtype=np.float64), np.asarray(std, dtype=np.float64)
    XS = Q + np.abs(np.asarray(mean, dtype=np.float64))
    return s * _half_ulp(XS / s) + 2.0 * _half_ulp(XS) + 2.0 * _half_ulp(Q)


def session_slew_host(v_rad, bound_rad, mean, std) -> np.ndarray:
    """The host model of ``sd_session_slew``'s arithmetic, for J joints: fp32 v_n from fp32 v_rad, bound, mean and std."""
    v = (np.asarray(v_rad, dtype=np.float32).astype(np.float64) - session_slew_margin(bound_rad, np.asarray(mean, dtype=np.float32), np.asarray(std, dtype=np.float32))) / np.asarray(std, dtype=np.float32).astype(np.float64)
    v = np.maximum(v, 0.0)
    out = v.astype(np.float32)
    over = out.astype(np.float64) > v
    out[over] = np.nextafter(out[over], np.float32(0))
    return out


def session_slew(v_n: Tensor, v_rad, bound_rad, mean: Tensor, std: Tensor, J: int) -> Tensor:
    """One launch (``sd_session_slew``) writes ``v_n`` - the (32,) device array a session's rollout reads - from ``v_rad``, radians per
    row as published, and ``bound_rad``, a finite bound on the magnitude of the published values per joint (host arrays of at least J
    fp32)."""
    v_rad, bound_rad = np.ascontiguousarray(v_rad, dtype=np.float32), np.ascontiguousarray(bound_rad, dtype=np.float32)
    if v_rad.ndim != 1 or bound_rad.ndim != 1 or v_rad.shape[0] < J or bound_rad.shape[0] < J:
        raise ValueError(f"session_slew: v_rad and bound_rad must hold at least {J} floats")
    if not _is_dev32(v_n, mean.device):
        raise ValueError(f"session_slew: v_n is the (32,) fp32 array of ops.joint_slew on {mean.device}")
    _req(mean, "mean"); _req(std, "std")
    check(_lib.load().sd_session_slew(v_n.data_ptr(), v_rad.ctypes.data_as(_lib.c_float_p), bound_rad.ctypes.data_as(_lib.c_float_p),
                                      mean.data_ptr(), std.data_ptr(), int(J), _stream()), "sd_session_slew")
    return v_n


def session_anchor(anchor: Tensor, x: Tensor, row: int, draws: int = 1, robots=None) -> Tensor:
    """One launch (``sd_session_anchor``): row ``row`` of ``x`` (S, T, J; normalised space) becomes the anchor of the robots' next tick -
    rows (b * draws + g) of ``anchor`` (B * draws, 32) for robot b = ``robots[s]`` (None: s) and every draw g."""
    _req(x, "x")
    S, T, J = x.shape
    B = anchor.shape[0] // draws
    if not _is_dev32(anchor, x.device, B * draws):
        raise ValueError("session_anchor: anchor is a contiguous (B * draws, 32) fp32 tensor on x's device")
    r = None if robots is None else _robots_on(robots, B, x.device)
    if (S != B) if r is None else (r.numel() != S):
        raise ValueError(f"session_anchor: x holds {S} robots")
    check(_lib.load().sd_session_anchor(anchor.data_ptr(), x.data_ptr(), _ptr(r), S, B, T, J, int(row), int(draws), _stream()), "sd_session_anchor")
    return anchor


def session_accel_margin(bound_rad, mean, std) -> np.ndarray:
    """The margin of ``sd_session_accel`` in radians, fp64, per joint: 4 std hu(3 XS / std) + 4 hu(XS) + 4 hu(pi + R) + 4 hu(R) with
    XS = R + |pi - mean| and hu half an fp32 ulp - what the four roundings of the scan's row function (d, p, p - a, p + a, at magnitudes
    up to 3 XS / std) and the roundings of the commit's expression at three published values with weights 1, 2 and 1 can add to a
    published second difference."""
    R, s = np.asarray(bound_rad, dtype=np.float64), np.asarray(std, dtype=np.float64)
    XS = R + np.abs(math.pi - np.asarray(mean, dtype=np.float64))
    return 4.0 * s * _half_ulp(3.0 * XS / s) + 4.0 * _half_ulp(XS) + 4.0 * _half_ulp(math.pi + R) + 4.0 * _half_ulp(R)


def denormalised_accel_margin(bound, mean, std) -> np.ndarray:
    """``session_accel_margin`` for trajectories that are denormalised and nothing else, r = x * std + mean (``ops.max_accel``):
    4 std hu(3 XS / std) + 4 hu(XS) + 4 hu(Q) with Q = ``bound`` >= |r| and XS = Q + |mean| >= |x std| - the scan's four roundings and the
    product's and the sum's of three values with weights 1, 2 and 1."""
    Q, s = np.asarray(bound, dtype=np.float64), np.asarray(std, dtype=np.float64)
    XS = Q + np.abs(np.asarray(mean, dtype=np.float64))
    return 4.0 * s * _half_ulp(3.0 * XS / s) + 4.0 * _half_ulp(XS) + 4.0 * _half_ulp(Q)


def session_accel_host(a_rad, bound_rad, mean, std) -> np.ndarray:
    """The host model of ``sd_session_accel``'s arithmetic, for J joints: fp32 a_n from fp32 a_rad, bound, mean and std."""
    s32 = np.asarray(std, dtype=np.float32)
    a = (np.asarray(a_rad, dtype=np.float32).astype(np.float64) - session_accel_margin(bound_rad, np.asarray(mean, dtype=np.float32), s32)) / s32.astype(np.float64)
    a = np.maximum(a, 0.0)
    out = a.astype(np.float32)
    over = out.astype(np.float64) > a
    out[over] = np.nextafter(out[over], np.float32(0))
    return out


def session_accel(a_n: Tensor, a_rad, bound_rad, mean: Tensor, std: Tensor, J: int) -> Tensor:
    """One launch (``sd_session_accel``) writes ``a_n`` - the (32,) device array a rollout under ``accel=`` reads - from ``a_rad``, radians
    per row^2 as published, and ``bound_rad``, a finite bound on the magnitude of the published values per joint (host arrays of at least
    J fp32).  ValueError for an ``a_rad`` that is not above its margin (``session_accel_margin``)."""
    a_rad, bound_rad = np.ascontiguousarray(a_rad, dtype=np.float32), np.ascontiguousarray(bound_rad, dtype=np.float32)
    if a_rad.ndim != 1 or bound_rad.ndim != 1 or a_rad.shape[0] < J or bound_rad.shape[0] < J:
        raise ValueError(f"session_accel: a_rad and bound_rad must hold at least {J} floats")
    if not _is_dev32(a_n, mean.device):
        raise ValueError(f"session_accel: a_n is the (32,) fp32 array of ops.joint_accel on {mean.device}")
    _req(mean, "mean"); _req(std, "std")
    margin = session_accel_margin(bound_rad[:J], mean.detach().cpu().numpy(), std.detach().cpu().numpy())
    finite = np.isfinite(a_rad[:J])
    if (a_rad[:J][finite].astype(np.float64) <= margin[finite]).any():
        j = int(np.argmax(finite & (a_rad[:J].astype(np.float64) <= margin)))
        raise ValueError(f"session_accel: a_rad[{j}] = {a_rad[j]} is not above its margin {margin[j]:.3g}")
    check(_lib.load().sd_session_accel(a_n.data_ptr(), a_rad.ctypes.data_as(_lib.c_float_p), bound_rad.ctypes.data_as(_lib.c_float_p),
                                       mean.data_ptr(), std.data_ptr(), int(J), _stream()), "sd_session_accel")
    return a_n


def session_anchor2(anchor: Tensor, anchor2: Tensor, x: Tensor, row: int, draws: int = 1, robots=None) -> None:
    """One launch (``sd_session_anchor2``): ``session_anchor`` with a second destination, for a scan whose state is two rows -
    ``anchor2`` <- row ``row - 1`` of ``x`` (``row`` == 0: the old ``anchor``), ``anchor`` <- row ``row`` of ``x``."""
    _req(x, "x")
    S, T, J = x.shape
    B = anchor.shape[0] // draws
    if not _is_dev32(anchor, x.device, B * draws) or not _is_dev32(anchor2, x.device, B * draws) or anchor.data_ptr() == anchor2.data_ptr():
        raise ValueError("session_anchor2: anchor and anchor2 are two contiguous (B * draws, 32) fp32 tensors on x's device")
    r = None if robots is None else _robots_on(robots, B, x.device)
    if (S != B) if r is None else (r.numel() != S):
        raise ValueError(f"session_anchor2: x holds {S} robots")
    check(_lib.load().sd_session_anchor2(anchor.data_ptr(), anchor2.data_ptr(), x.data_ptr(), _ptr(r), S, B, T, J, int(row), int(draws), _stream()),
          "sd_session_anchor2")


def session_reset(rings: Sequence[tuple], mask: Optional[Tensor] = None, game_state: Optional[Tensor] = None, game_state_value: int = 0,
                  pin_rows: Optional[Tensor] = None) -> None:
    """The start state of an episode for the robots a mask selects, in one launch (``sd_session_reset``): ``rings`` is up to five
    (ring, head, fill) with ``fill`` a device row of C floats or None for zeros; ``mask`` (B) bool or uint8 on the device (None: every
    robot) is read by the kernel only - nothing comes back to the host, so a simulator's ``done`` tensor can be passed as it is;
    ``game_state`` (B) int64 receives ``game_state_value`` for the selected robots.  ``pin_rows`` (B) int32: the carried-row counts of a
    session with overlapping ticks, zeroed for the selected robots in the same launch (``sd_session_reset_carry``)."""
    if not 1 <= len(rings) <= 5:
        raise ValueError("one to five rings per launch")
    array = (_lib.RingReset * len(rings))()
    B, dev = rings[0][0].shape[0], rings[0][0].device
    for i, (ring, head, fill) in enumerate(rings):
        shape = _ring_req(ring, head)
        if shape[0] != B or ring.device != dev:
            raise ValueError(f"ring {i}: {shape} on {ring.device} does not share the batch {B} on {dev}")
        if fill is not None and (_req(fill, "fill").numel() != shape[2] or fill.device != dev):
            raise ValueError(f"ring {i}: fill: expected {shape[2]} values on {dev}")
        v = array[i]
        v.ring, v.head, v.fill, v.L, v.C = ring.data_ptr(), head.data_ptr(), _ptr(fill), shape[1], shape[2]
    if mask is not None:
        if mask.dtype not in (torch.bool, torch.uint8):
            raise TypeError(f"mask: expected torch.bool or torch.uint8, got {mask.dtype}")
        _req(mask, "mask", mask.dtype)
        if tuple(mask.shape) != (B,) or mask.device != dev:
            raise ValueError(f"mask: expected ({B},) on {dev}, got {tuple(mask.shape)} on {mask.device}")
    if game_state is not None and (tuple(_req(game_state, "game_state", torch.int64).shape) != (B,) or game_state.device != dev):
        raise ValueError(f"game_state: expected ({B},) int64 on {dev}")
    if pin_rows is not None:
        if tuple(_req(pin_rows, "pin_rows", torch.int32).shape) != (B,) or pin_rows.device != dev:
            raise ValueError(f"pin_rows: expected ({B},) int32 on {dev}")
        check(_lib.load().sd_session_reset_carry(array, len(rings), _ptr(mask), _ptr(game_state), int(game_state_value), pin_rows.data_ptr(), B,
                                                 _stream()), "sd_session_reset_carry")
        return
    check(_lib.load().sd_session_reset(array, len(rings), _ptr(mask), _ptr(game_state), int(game_state_value), B, _stream()), "sd_session_reset")
