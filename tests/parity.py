"""Row-by-row parity metrics against an fp64 reference, for (B, T, J) trajectories and - further down - for the parameter gradients of a
training step (a plain helper module, not a conftest).

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


# ------------------------------------------------------------------------------------------------------------------------------------
# parameter gradients of a training step
# ------------------------------------------------------------------------------------------------------------------------------------
# One L2 norm per parameter (tests/test_gpu_training.py::_check_grads: 1e-4 against the fp32 oracle, floored at 1e-3 of the largest
# gradient) is 150 - 300 x above what fp32 itself does on these gradients, and it cannot see the K block of an in_proj_weight beside its
# V block, one bad output row of a weight gradient or the quiet rows of a tensor.  The three figures of a parameter gradient G against
# the fp64 oracle's W - rows are output features (dimension 0), the rows of a 1-D parameter its elements:
#   glob   ||G - W|| / ||W|| over the parameter
#   block  the same per named block, maximum over blocks: q | k | v of every in_proj_weight / in_proj_bias, any other parameter is one
#   row    max_r ||G_r - W_r|| / s,  s = sqrt(mean_r ||W_r||^2) over ALL rows of the parameter
# each held to factor * (the fp32 CPU oracle's own figure for that parameter) + floor.
#
# Blocks that are zero by construction have no relative error: the key-bias block of every attention (softmax is shift invariant) and,
# with a one-row memory, the cross-attention's query and key blocks and norm2 (the only probability is 1; likewise the self-attention's
# query and key blocks at a horizon of one token).  They stay out of `block`, are gated inside `row` where their parameter has a non-zero
# block (s is then the scale of the live rows beside them) and absolutely, ||G|| <= factor * ||fp32 oracle's|| + floor * (largest
# gradient norm of their layer), where the whole parameter is zero.
# zero_blocks() derives the set from the fp64 oracle; named_zero_blocks() is the list it has to equal - nothing else leaves the
# relative gate.
class GradErrors(NamedTuple):
    glob: float
    block: float
    row: float


ZERO_BLOCK = 1e-6    # a block below this fraction of its parameter's fp64 norm ...
ZERO_PARAM = 1e-12   # ... or a parameter below this fraction of the largest fp64 gradient norm is zero by construction


def _rows(g: torch.Tensor) -> torch.Tensor:
    g = g.detach().to("cpu", torch.float64)
    return g.reshape(g.shape[0], -1) if g.dim() > 1 else g.reshape(-1, 1)


def grad_blocks(name: str, rows: int):
    """[(label, row slice)] of a parameter with `rows` output features."""
    if name.endswith(("in_proj_weight", "in_proj_bias")):
        d = rows // 3
        return [(lab, slice(i * d, (i + 1) * d)) for i, lab in enumerate("qkv")]
    return [("", slice(0, rows))]


def grad_group(name: str) -> str:
    """The layer a parameter belongs to ('...layers.3'), or its module outside the layer stacks ('imu_encoder', 'step_encoding')."""
    parts = name.split(".")
    if "layers" in parts:
        return ".".join(parts[: parts.index("layers") + 2])
    return parts[0]


def zero_blocks(want64) -> set:
    """{(parameter, block label)} whose fp64 gradient is zero by the rule above."""
    norms = {k: float(_rows(g).norm()) for k, g in want64.items()}
    top = max(norms.values())
    out = set()
    for k, g in want64.items():
        W = _rows(g)
        for lab, sl in grad_blocks(k, W.shape[0]):
            if norms[k] < ZERO_PARAM * top or float(W[sl].norm()) < ZERO_BLOCK * norms[k]:
                out.add((k, lab))
    return out


def named_zero_blocks(names, one_row_memory: bool = False, one_token: bool = False) -> set:
    """The blocks that are zero by construction: the key bias of every attention; with a memory of one row also the cross-attention's
    query and key blocks (weight and bias) and the LayerNorm in front of its query projection; with a horizon of one token the decoder
    self-attention's query and key blocks for the same reason (norm1 stays live through the values)."""
    out = set()
    for k in names:
        if k.endswith("in_proj_bias"):
            out.add((k, "k"))
        if one_row_memory and ".multihead_attn.in_proj_" in k:
            out.update({(k, "q"), (k, "k")})
        if one_token and "transformer_decoder" in k and ".self_attn.in_proj_" in k:
            out.update({(k, "q"), (k, "k")})
        if one_row_memory and "transformer_decoder" in k and ".norm2." in k:
            out.add((k, ""))
    return out


class _Param(NamedTuple):
    e: object          # GradErrors, or None for a parameter that is zero as a whole
    norm: float        # ||G||, non-finite counted as inf (the absolute gate's figure)
    block: str         # label of the worst live block
    row: int           # worst row
    row_block: str     # the block it lies in


def _grad_measure(name: str, got: torch.Tensor, want64: torch.Tensor, zero: set) -> _Param:
    G, W = _rows(got), _rows(want64)
    if tuple(got.shape) != tuple(want64.shape):
        raise ValueError(f"{name}: gradient of shape {tuple(got.shape)} against a reference of {tuple(want64.shape)}")
    if not torch.isfinite(W).all():
        raise ValueError(f"{name}: the fp64 reference itself is not finite")
    norm = float(_fail_on_nan((G ** 2).sum()).sqrt())
    blocks = grad_blocks(name, W.shape[0])
    live = [(lab, sl) for lab, sl in blocks if (name, lab) not in zero]
    if not live:
        return _Param(None, norm, "", 0, "")
    d2 = _fail_on_nan(((G - W) ** 2).sum(1))
    w2 = (W ** 2).sum(1)
    per_block = [float((d2[sl].sum() / w2[sl].sum().clamp_min(TINY)).sqrt()) for _, sl in live]
    worst = max(range(len(live)), key=lambda i: per_block[i])
    per_row = (d2 / w2.mean().clamp_min(TINY)).sqrt()
    r = int(per_row.argmax())
    row_block = next(lab for lab, sl in blocks if sl.start <= r < sl.stop)
    e = GradErrors(float((d2.sum() / w2.sum().clamp_min(TINY)).sqrt()), per_block[worst], float(per_row[r]))
    return _Param(e, norm, live[worst][0], r, row_block)


def grad_errors(got, want64, zero=None) -> dict:
    """{parameter: GradErrors} of a dictionary of gradients against the fp64 oracle's (None for a parameter that is zero as a whole).
    `zero` defaults to zero_blocks(want64)."""
    zero = zero_blocks(want64) if zero is None else zero
    return {k: _grad_measure(k, got[k], want64[k], zero).e for k in want64}


def grad_report(label: str, e: GradErrors, e32: GradErrors) -> str:
    """One line per gated parameter group: for each figure the parameter of the group that comes closest to its bound."""
    ratio = [a / max(b, TINY) for a, b in zip(e, e32)]
    return (f"{label:66s} kernel {e.glob:8.2e} {e.block:8.2e} {e.row:8.2e}  fp32 {e32.glob:8.2e} {e32.block:8.2e} {e32.row:8.2e}"
            f"  ratio {ratio[0]:5.2f} {ratio[1]:5.2f} {ratio[2]:5.2f}")


def assert_grads_fp32_grade(got, want64, want32, zero=None, factor: float = FACTOR, floor: float = FLOOR, label: str = "",
                            row_factor=None) -> dict:
    """Every parameter gradient of `got` within factor * (the fp32 CPU oracle's figure) + floor on glob, block and row (`row_factor`, where
    given, replaces the factor of the row figure alone), the blocks in `zero` (default: zero_blocks(want64)) treated as described above.
    Prints one line per parameter group, then raises with every parameter that misses.  Returns {parameter: GradErrors}."""
    if not set(got) == set(want64) == set(want32):
        raise AssertionError(f"{label}: gradient key sets differ: missing {sorted(set(want64) - set(got))}, "
                             f"unexpected {sorted(set(got) - set(want64))}, fp32 oracle {sorted(set(want32) ^ set(want64))}")
    zero = zero_blocks(want64) if zero is None else zero
    groups: dict = {}
    for k in want64:
        groups.setdefault(grad_group(k), []).append(k)
    out, failures = {}, []
    for grp, names in groups.items():
        top = max(float(_rows(want64[k]).norm()) for k in names)
        shown = [None, None, None]   # per figure: (tightness, kernel, fp32)
        for k in names:
            m, m32 = _grad_measure(k, got[k], want64[k], zero), _grad_measure(k, want32[k], want64[k], zero)
            out[k] = m.e
            if m.e is None:
                bound = factor * m32.norm + floor * top
                print(f"{label + ' ' + k:100s} zero by construction: ||G|| {m.norm:8.2e}  fp32 {m32.norm:8.2e}  bound {bound:8.2e}")
                if not m.norm <= bound:
                    failures.append(f"{label}: {k} is zero by construction in the fp64 oracle: ||G|| = {m.norm:.3e} above {factor:g} * "
                                    f"{m32.norm:.3e} + {floor:g} * {top:.3e} (the largest gradient norm of {grp})")
                continue
            for i, (fig, a, b) in enumerate(zip(GradErrors._fields, m.e, m32.e)):
                f = row_factor if fig == "row" and row_factor is not None else factor
                bound = f * b + floor
                if shown[i] is None or a / bound > shown[i][0]:
                    shown[i] = (a / bound, a, b)
                if not a <= bound:
                    where = {"glob": "the whole parameter", "block": f"block '{m.block}'", "row": f"row {m.row} (block '{m.row_block}')"}[fig]
                    failures.append(f"{label}: {k}, {where}: '{fig}' error {a:.3e} above {f:g} * {b:.3e} + {floor:g}; kernel (glob, "
                                    f"block, row) = ({m.e.glob:.3e}, {m.e.block:.3e}, {m.e.row:.3e}), fp32 oracle = ({m32.e.glob:.3e}, "
                                    f"{m32.e.block:.3e}, {m32.e.row:.3e}); worst block '{m.block}', worst row {m.row} (block '{m.row_block}')")
        if all(s is not None for s in shown):
            print(grad_report(f"{label} {grp}", GradErrors(*(s[1] for s in shown)), GradErrors(*(s[2] for s in shown))))
    if failures:
        raise AssertionError("\n".join(failures))
    return out


def assert_loss_fp32_grade(loss, loss64, loss32, factor: float = FACTOR, floor: float = FLOOR, label: str = "") -> float:
    """|loss - loss64| / |loss64| within factor * (the fp32 oracle's) + floor; NaN fails."""
    want = float(loss64)
    e, e32 = abs(float(loss) - want) / abs(want), abs(float(loss32) - want) / abs(want)
    print(f"{label:66s} loss   {e:8.2e}  fp32 {e32:8.2e}  ratio {e / max(e32, TINY):5.2f}")
    if not e <= factor * e32 + floor:
        raise AssertionError(f"{label}: loss {float(loss)!r} against {want!r}: relative error {e:.3e} above {factor:g} * {e32:.3e} + {floor:g}")
    return e
