"""Row-by-row parity metrics for (B, T, J) trajectories against an fp64 reference (a plain helper module, not a conftest).

conftest.rel_err is ONE L2 norm over the whole tensor: a bad row of small magnitude, one trajectory of a batch or a lost cross term of a
split product disappears in it.  errors() adds a per-trajectory and a per-row figure, and assert_fp32_grade() holds all three to a
multiple of the error the fp32 CPU oracle itself makes against fp64 on the same inputs - the yardstick is never the kernel's own number."""

from __future__ import annotations

from typing import NamedTuple

import torch

FACTOR = 4.0   # tests/test_gpu_denoiser.py::test_fp16x3_sampler_is_fp32_grade: e < 4 * e_cpu32 + 1e-7
FLOOR = 1e-7
TINY = 1e-300


class Errors(NamedTuple):
    glob: float   # ||got - want|| / ||want|| over the whole tensor (conftest.rel_err)
    traj: float   # max over b of ||got[b] - want[b]||_F / ||want[b]||_F
    row: float    # max over (b, t) of ||got[b, t] - want[b, t]||_2 / s_b,  s_b = sqrt(mean_t ||want[b, t]||_2^2)


def _fail_on_nan(v: torch.Tensor) -> torch.Tensor:
    """NaN orders below everything in max() and passes every `<`: count it (and inf) as an infinite error."""
    return torch.where(torch.isfinite(v), v, torch.full_like(v, float("inf")))


def _measure(got: torch.Tensor, want64: torch.Tensor):
    got = got.detach().to("cpu", torch.float64)
    want = want64.detach().to("cpu", torch.float64)
    if got.shape != want.shape or got.dim() != 3:
        raise ValueError(f"errors() takes two (B, T, J) tensors, got {tuple(got.shape)} and {tuple(want.shape)}")
    if not torch.isfinite(want).all():
        raise ValueError("the fp64 reference itself is not finite")
    d2 = _fail_on_nan(((got - want) ** 2).sum(-1))           # (B, T) squared row errors
    w2 = (want ** 2).sum(-1)                                  # (B, T) squared row norms
    glob = float((d2.sum() / w2.sum().clamp_min(TINY)).sqrt())
    per_traj = (d2.sum(1) / w2.sum(1).clamp_min(TINY)).sqrt()                    # (B,)
    per_row = (d2 / w2.mean(1, keepdim=True).clamp_min(TINY)).sqrt()             # (B, T)
    b_traj = int(per_traj.argmax())
    flat = int(per_row.argmax())
    return Errors(glob, float(per_traj[b_traj]), float(per_row.flatten()[flat])), b_traj, divmod(flat, per_row.shape[1])


def errors(got: torch.Tensor, want64: torch.Tensor) -> Errors:
    """The three figures of `got` against the fp64 reference, computed in float64 on the CPU.  A non-finite value in `got` makes the
    figures it enters infinite."""
    return _measure(got, want64)[0]


def report(label: str, e: Errors, e32: Errors) -> str:
    """One line per gated tensor: kernel and fp32-oracle figures and their ratios (profiles/shipped_shapes_parity.txt)."""
    ratio = [a / max(b, TINY) for a, b in zip(e, e32)]
    return (f"{label:58s} kernel {e.glob:8.2e} {e.traj:8.2e} {e.row:8.2e}  fp32 {e32.glob:8.2e} {e32.traj:8.2e} {e32.row:8.2e}"
            f"  ratio {ratio[0]:5.2f} {ratio[1]:5.2f} {ratio[2]:5.2f}")


def assert_fp32_grade(got: torch.Tensor, want64: torch.Tensor, want32: torch.Tensor, factor: float = FACTOR, floor: float = FLOOR,
                      label: str = "") -> Errors:
    """Each of the three figures of `got` is at most factor * (the same figure of the fp32 CPU oracle `want32`) + floor."""
    e, b_traj, (b_row, t_row) = _measure(got, want64)
    e32 = errors(want32, want64)
    print(report(label, e, e32))
    for name, a, b in zip(Errors._fields, e, e32):
        if not a <= factor * b + floor:
            raise AssertionError(
                f"{label}: '{name}' error {a:.3e} above {factor:g} * {b:.3e} + {floor:g}; kernel (global, traj, row) = "
                f"({e.glob:.3e}, {e.traj:.3e}, {e.row:.3e}), fp32 oracle = ({e32.glob:.3e}, {e32.traj:.3e}, {e32.row:.3e}); "
                f"worst trajectory b = {b_traj}, worst row (b, t) = ({b_row}, {t_row})")
    return e
