"""FusedAdamW - torch.optim.AdamW semantics on ONE flat fp32 buffer per quantity - and WeightPlanes, the one store of every copy the
training kernels read instead of the flat parameter buffer itself: split fp16 planes of the d x d blocks and of their transposes, the fp32
transposed gather that stands in for them, and the trajectory kernels' planes.  The optimizer owns its store and refreshes it where every
rewrite of the buffer ends; lookups go from a tensor's address to the live store whose buffer contains it."""

from __future__ import annotations

import contextlib
import os
import weakref
from typing import Iterable, Optional

import torch

from . import derived, ops

Tensor = torch.Tensor

_STORES: list = []   # weak references to the stores that answer lookups; dead ones answer nothing and leave when the next store is built


def planes_of(W: Tensor):
    """The live store whose flat parameter buffer contains W's address (W: a parameter, a row slice such as W[d:], or detached - autograd
    hands the nodes views, so the lookup is by address), else None."""
    a = W.data_ptr()
    for ref in _STORES:
        s = ref()
        if s is not None and s.lo <= a < s.hi:
            return s
    return None


class WeightPlanes:
    """The derived copies of one flat parameter buffer, refreshed by ONE gather / two pack launches per block width after every step (the
    weights are final until the next one) instead of one strided copy or one in-register split per GEMM and workgroup:
      * ``flat_wpk``: [planes of the blocks | planes of the transposed blocks], 2 d^2 halfs each - the fp16 hi | lo fragment planes the
        panel kernel multiplies with (ops.pack_weight_blocks), so the ~45 GEMMs of a step stream 1-KiB fragments;
      * ``flat_wt``: without planes (no GPU, SD_TRAIN_PACKED=0) an fp32 copy of every transposed block, same order, for the dX GEMMs;
      * ``traj``: planes of whole matrices in the 16 x 16 x 32 fragment order of the trajectory kernels (csrc/sd_traj.h), for the slices
        the stacks asked for (``traj_planes``); repacked by one launch.
    ``blocks`` maps a block's address to (float offset of its transpose in flat_wt's order, d, parameter index).  A parameter's copies are
    current while ``derived.versions`` of it is what the last refresh saw (load_state_dict, p.mul_(), ... move it; a write through
    ``p.data`` does not - call ``optimizer.refresh_transposes()`` after one)."""

    def __init__(self, flat_param: Tensor, params):
        self.flat_param, dev = flat_param, flat_param.device
        self.lo = flat_param.data_ptr()
        self.hi = self.lo + 4 * flat_param.numel()
        # gather index of every d x d block of the (N = k d, d) matrices, transposed
        idx, blocks, self.params, at, out_at = [], [], [], 0, 0
        for p in params:
            k = p.numel()
            if p.dim() == 2 and p.shape[1] in (64, 128, 256, 512) and p.shape[0] % p.shape[1] == 0:
                N, d = p.shape
                idx.append(at + torch.arange(k, dtype=torch.int64).view(N // d, d, d).transpose(1, 2).reshape(-1))
                blocks += [(at + blk * d * d, out_at + blk * d * d, d, len(self.params)) for blk in range(N // d)]
                self.params.append(p)
                out_at += k
            at += k
        self.blocks = {self.lo + 4 * src: (off, d, pi) for src, off, d, pi in blocks}
        self.total = out_at
        self.seen = [None] * len(self.params)   # per parameter, the version key of the last refresh (None: never current)
        # per block width, (source offsets, first block) of the pack launches
        self.flat_wpk, self.launches = None, []
        if idx and dev.type == "cuda" and os.environ.get("SD_TRAIN_PACKED", "1") != "0":
            self.flat_wpk = torch.empty(4 * out_at, dtype=torch.float16, device=dev)
            for d in sorted({b[2] for b in blocks}):
                run = [b for b in blocks if b[2] == d]
                # blocks of one width are contiguous in flat_wt only if no other width interleaves: pack run by run
                runs, cur = [], [run[0]]
                for b in run[1:]:
                    if b[1] == cur[-1][1] + d * d:
                        cur.append(b)
                    else:
                        runs.append(cur); cur = [b]
                runs.append(cur)
                for r in runs:
                    self.launches.append((d, len(r), torch.tensor([b[0] for b in r], dtype=torch.int64, device=dev), 2 * r[0][1]))
        self.wt_index = torch.cat(idx).to(dev) if idx and self.flat_wpk is None else None
        self.flat_wt = torch.empty(out_at, dtype=torch.float32, device=dev) if idx and self.flat_wpk is None else None
        self.traj, self.traj_at, self.traj_dev = None, {}, None   # planes, {(source float offset, rows): half offset}, device index arrays
        if self.blocks and flat_param.is_cuda:
            _STORES[:] = [r for r in _STORES if r() is not None] + [weakref.ref(self)]

    def refresh(self) -> None:
        if not self.blocks or not self.flat_param.is_cuda:
            return
        if self.flat_wt is not None:
            torch.index_select(self.flat_param, 0, self.wt_index, out=self.flat_wt)
        for d, n, src, half_off in self.launches:   # the transposition happens inside the pack kernel
            ops.pack_weight_blocks(self.flat_param, src, n, d, self.flat_wpk[half_off:])
            ops.pack_weight_blocks(self.flat_param, src, n, d, self.flat_wpk[2 * self.total + half_off:], transposed=True)
        self.seen = [derived.versions(p) for p in self.params]
        self._repack_traj()

    def block(self, W: Tensor, p: int, d: int):
        """Float offset of the transpose of block p of W in flat_wt's order while W's copies are current, else None."""
        ent = self.blocks.get(W.data_ptr() + 4 * p * d * d)
        if ent is not None and ent[1] == d and W.shape[1] == d and derived.current(self.seen[ent[2]], derived.versions(self.params[ent[2]])):
            return ent[0]
        return None

    def traj_planes(self, slices) -> list:
        """Addresses of the trajectory-kernel planes (ops.pack_weight_traj layout) of rows [row0, row0 + rows) of W for every (W, row0, rows)
        of ``slices`` - a stack asks for all of its slices at once.  New ones register first (lazily: in the eager warm-up steps of a
        graphed loop), then the buffer grows ONCE and every registered slice is repacked, so all the addresses returned hold together;
        addresses handed out before a growth do not."""
        at, n = [], len(self.traj_at)
        for W, row0, rows in slices:
            src = (W.data_ptr() - self.lo) // 4 + row0 * 256
            if W.shape[1] != 256 or W.stride() != (256, 1) or rows % 16 or src + rows * 256 > self.flat_param.numel() or self.block(W, 0, 256) is None:
                raise ValueError("trajectory-order planes are kept for current (N, 256) row-major matrices of this optimizer, 16 rows at a time")
            at.append(self.traj_at.setdefault((src, rows), sum(2 * 256 * r for _, r in self.traj_at)))
        if len(self.traj_at) > n:
            dev = self.flat_param.device
            self.traj = torch.empty(sum(2 * 256 * r for _, r in self.traj_at), dtype=torch.float16, device=dev)
            self.traj_dev = (torch.tensor([s for s, _ in self.traj_at], dtype=torch.int64, device=dev),
                             torch.tensor([r for _, r in self.traj_at], dtype=torch.int32, device=dev),
                             torch.tensor(list(self.traj_at.values()), dtype=torch.int64, device=dev))
            self._repack_traj()
        return [self.traj.data_ptr() + 2 * a for a in at]

    def _repack_traj(self) -> None:
        if self.traj is not None:
            ops.pack_weight_traj_multi(self.flat_param, *self.traj_dev, max(r for _, r in self.traj_at), self.traj)


def _transposed_block(W: Tensor, p: int, d: int) -> Tensor:
    s = planes_of(W)
    off = s.block(W, p, d) if s is not None and s.flat_wt is not None else None
    if off is not None:
        return s.flat_wt[off : off + d * d].view(d, d)
    return W[p * d : (p + 1) * d].t().contiguous()


def _packed_weight(W: Tensor, p: int = 0, transposed: bool = False):
    """Address of the planes of block p of W (and of the blocks behind it), or None when W has no current planes."""
    d = W.shape[1]
    s = planes_of(W)
    if s is None or s.flat_wpk is None or W.stride() != (d, 1):
        return None
    off = s.block(W, p, d)
    return None if off is None else s.flat_wpk.data_ptr() + 2 * (2 * off + (2 * s.total if transposed else 0))


class FusedAdamW(torch.optim.Optimizer):
    """AdamW(lr) with torch's defaults (betas 0.9/0.999, eps 1e-8, weight_decay 1e-2) as the
    reference constructs it (train.py:162).  Parameters, gradients and both moments live in
    four flat buffers (parameters are re-pointed to views), so a step is one kernel launch
    and the data-parallel gradient exchange is one all-reduce.  ``state_dict()`` has torch
    AdamW's layout (``state[i] = {step, exp_avg, exp_avg_sq}``), so checkpoints interchange.
    Being a torch Optimizer, ``OneCycleLR`` drives ``lr`` and ``betas[0]`` as in the reference.

    ``ema_decay`` (None = off: nothing allocated, the plain kernels run): an exponential moving average of the parameters in a
    fifth flat buffer ``flat_ema``, initialised to them and updated by the SAME launch as the AdamW step, eager or replayed
    (``ema += w_t (p_new - ema)``).  The weight of the update that follows t completed ones is
    ``w_t = 1 - min(ema_decay, (1 + t) / (10 + t))`` with ``ema_warmup`` (0.9, 0.818.., .. down to ``1 - ema_decay``: a young average
    forgets its initial weights quickly) and ``1 - ema_decay`` without.  This rule is this package's OWN definition: the reference's
    lineage took its EMA from ``ema_pytorch`` (``EMA(model, beta=0.9999)``), and neither that nor ``diffusers``' EMAModel is
    installed here to pin the warmup against - only the fixed point, ``1 - ema_decay``, is common to all of them.  ``state_dict()``
    stays torch AdamW's; the average travels as a model state dict (``ema_state_dict`` / ``load_ema_state_dict``) beside
    ``ema_state()``.  Sampling from it in mid-training: ``with optimizer.ema_weights(): ...``.

    ``max_grad_norm`` (None = off: nothing allocated, today's launches): ``torch.nn.utils.clip_grad_norm_`` (norm type 2, over the
    whole flat gradient) and a non-finite guard in front of the update, all on the device - eager step, graph replay and the
    data-parallel step (after the all-reduce, so every rank computes the same coefficient) alike.  Two small launches take the norm
    in ONE deterministic fp64 summation (``ops.grad_norm``); the update then runs on ``g * coef`` with
    ``coef = min(1, max_grad_norm / (norm + 1e-6))``, and where the norm is inf or NaN it does not run at all: parameters, moments
    and EMA keep their bits and a device counter goes up.  ``inf`` = guard and norm only (``coef`` = 1: bit for bit the unclipped
    step).  A skipped step still USES UP its step number: the host is not told, so ``_step``, the bias corrections, OneCycleLR and
    ``ema_updates`` advance as after any other step.  ``grad_stats()`` reads norm, coefficient and the count of skipped steps."""

    def __init__(self, params: Iterable[Tensor], lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 1e-2, ema_decay: Optional[float] = None, ema_warmup: bool = True,
                 max_grad_norm: Optional[float] = None):
        params = [p for p in params if p.requires_grad]
        if not params:
            raise ValueError("no trainable parameters")
        if max_grad_norm is not None and not float(max_grad_norm) >= 0.0:   # (NaN fails the comparison)
            raise ValueError(f"max_grad_norm must be >= 0 (inf = guard and norm only) or None, got {max_grad_norm!r}")
        if ema_decay is not None and not 0.0 < ema_decay < 1.0:
            raise ValueError(f"ema_decay must lie in (0, 1) or be None, got {ema_decay!r}")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        dev = params[0].device
        n = sum(p.numel() for p in params)
        self.flat_param = torch.empty(n, dtype=torch.float32, device=dev)
        self.flat_grad = torch.zeros(n, dtype=torch.float32, device=dev)
        self.flat_m = torch.zeros(n, dtype=torch.float32, device=dev)
        self.flat_v = torch.zeros(n, dtype=torch.float32, device=dev)
        self._step = 0
        at = 0
        for p in params:
            k = p.numel()
            self.flat_param[at : at + k].copy_(p.detach().reshape(-1))
            p.data = self.flat_param[at : at + k].view(p.shape)
            p.grad = self.flat_grad[at : at + k].view(p.shape)
            self.state[p] = {"step": torch.tensor(0.0), "exp_avg": self.flat_m[at : at + k].view(p.shape),
                             "exp_avg_sq": self.flat_v[at : at + k].view(p.shape)}
            at += k
        self.ema_decay, self.ema_warmup = (None if ema_decay is None else float(ema_decay)), bool(ema_warmup)
        self.ema_updates = 0   # completed EMA updates (its own count: an average may start in the middle of a run)
        self.flat_ema = self.flat_param.clone() if ema_decay is not None else None
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self._gn_partials = self._clip = self._skipped = None
        if self.max_grad_norm is not None:   # allocated once: their addresses sit in a captured graph
            self._gn_partials = torch.zeros(ops.grad_norm_workspace_doubles(), dtype=torch.float64, device=dev)
            self._clip = torch.tensor([0.0, 1.0], dtype=torch.float32, device=dev)   # [norm, coef] of the last step
            self._skipped = torch.zeros(1, dtype=torch.int32, device=dev)
        self.planes = WeightPlanes(self.flat_param, params)
        self.refresh_transposes()

    flat_wpk = property(lambda self: self.planes.flat_wpk)
    flat_wt = property(lambda self: self.planes.flat_wt)

    def refresh_transposes(self) -> None:
        """The per-step refresh of the derived copies of the weights (WeightPlanes)."""
        ops.bump_weights_generation()   # every path that rewrites flat_param ends here (step, step_from_device_hyper, broadcast)
        self.planes.refresh()

    def zero_grad(self, set_to_none: bool = False):
        self.flat_grad.zero_()
        at = 0
        for p in self.param_groups[0]["params"]:  # keep .grad aliased to the flat buffer
            k = p.numel()
            if p.grad is None or p.grad.data_ptr() != self.flat_grad.data_ptr() + 4 * at:
                p.grad = self.flat_grad[at : at + k].view(p.shape)
            at += k

    @torch.no_grad()
    def step(self, closure=None):
        g = self.param_groups[0]
        self._step += 1
        if self.max_grad_norm is not None:
            ops.grad_norm(self.flat_grad, self._gn_partials, self._clip, self._skipped, self.max_grad_norm)
            ops.adamw_clip_step(self.flat_param, self.flat_grad, self.flat_m, self.flat_v, self.flat_ema, self._clip, g["lr"], g["betas"][0],
                                g["betas"][1], g["eps"], g["weight_decay"], self._step,
                                0.0 if self.flat_ema is None else self.ema_weight_for_step(self.ema_updates))
            self.ema_updates += int(self.flat_ema is not None)
        elif self.flat_ema is None:
            ops.adamw_step(self.flat_param, self.flat_grad, self.flat_m, self.flat_v, g["lr"], g["betas"][0], g["betas"][1],
                           g["eps"], g["weight_decay"], self._step)
        else:
            ops.adamw_ema_step(self.flat_param, self.flat_grad, self.flat_m, self.flat_v, self.flat_ema, g["lr"], g["betas"][0],
                               g["betas"][1], g["eps"], g["weight_decay"], self._step, self.ema_weight_for_step(self.ema_updates))
            self.ema_updates += 1
        self.refresh_transposes()

    @torch.no_grad()
    def step_from_device_hyper(self, hyper7: Tensor, ema_weight: Optional[Tensor] = None) -> None:
        """The update with its scalars read from device memory (``hyper_for_step``): what a captured graph replays.
        Does NOT advance ``_step`` (nor ``ema_updates``) - the caller that fills ``hyper7`` does.  With an EMA, ``ema_weight`` is the
        device float that holds ``ema_weight_for_step(ema_updates)`` when the update runs.  With ``max_grad_norm`` the norm's two
        launches come first and ``max_grad_norm`` is one of their (frozen) arguments."""
        if self.flat_ema is not None and ema_weight is None:
            raise ValueError("this optimizer keeps an EMA: the update needs the device word with its weight")
        if self.max_grad_norm is not None:
            ops.grad_norm(self.flat_grad, self._gn_partials, self._clip, self._skipped, self.max_grad_norm)
            ops.adamw_clip_step_dev(self.flat_param, self.flat_grad, self.flat_m, self.flat_v, self.flat_ema, self._clip, hyper7, ema_weight)
        elif self.flat_ema is None:
            ops.adamw_step_dev(self.flat_param, self.flat_grad, self.flat_m, self.flat_v, hyper7)
        else:
            ops.adamw_ema_step_dev(self.flat_param, self.flat_grad, self.flat_m, self.flat_v, self.flat_ema, hyper7, ema_weight)
        self.refresh_transposes()

    # ---- gradient clipping ---------------------------------------------------------------
    def grad_stats(self) -> dict:
        """``{"norm", "coef", "skipped_steps"}``: the gradient norm and clipping coefficient of the last step (norm 0 / coef 1 before the
        first; coef 0 where that step was skipped) and the number of skipped steps so far.  ONE device read of three words - it waits
        for the stream, so call it where a sync is affordable (``cli train`` does beside the printed loss), not every step."""
        if self.max_grad_norm is None:
            raise RuntimeError("this optimizer does not clip (max_grad_norm=None)")
        w = torch.cat([self._clip, self._skipped.view(torch.float32)]).cpu()
        return {"norm": float(w[0]), "coef": float(w[1]), "skipped_steps": int(w[2:3].view(torch.int32)[0])}

    def set_skipped_steps(self, count: int) -> None:
        """Resume: the count of skipped steps a checkpoint carried."""
        if self.max_grad_norm is None:
            raise RuntimeError("this optimizer does not clip (max_grad_norm=None)")
        self._skipped.fill_(int(count))

    # ---- weight EMA ---------------------------------------------------------------------
    def ema_weight_for_step(self, t: int) -> float:
        """w_t of the class comment: the weight of the EMA update that follows ``t`` completed ones."""
        if self.ema_decay is None:
            raise RuntimeError("this optimizer keeps no EMA (ema_decay=None)")
        if t < 0:
            raise ValueError("t counts completed updates: >= 0")
        return 1.0 - (min(self.ema_decay, (1 + t) / (10 + t)) if self.ema_warmup else self.ema_decay)

    def ema_state(self) -> dict:
        """What a checkpoint keeps beside ``ema_state_dict``: plain types."""
        return {"decay": self.ema_decay, "warmup": self.ema_warmup, "num_updates": self.ema_updates}

    def _ema_view(self, t: Tensor):
        """The slice of flat_ema that stands for ``t`` if ``t`` is one of this optimizer's parameters (by address), else None."""
        off = t.data_ptr() - self.flat_param.data_ptr()
        if self.flat_ema is None or t.numel() == 0 or not 0 <= off < 4 * self.flat_param.numel():
            return None
        return self.flat_ema[off // 4 : off // 4 + t.numel()].view(t.shape)

    def ema_state_dict(self, model) -> dict:
        """``model.state_dict()`` with every tensor this optimizer owns replaced by its EMA view; everything else - buffers such as
        ``mean`` / ``std`` and BatchNorm statistics, frozen parameters, parameters left to no optimizer - is the live model's."""
        if self.flat_ema is None:
            raise RuntimeError("this optimizer keeps no EMA (ema_decay=None)")
        out = model.state_dict()
        for k, t in out.items():
            e = self._ema_view(t)
            if e is not None:
                out[k] = e
        return out

    @torch.no_grad()
    def load_ema_state_dict(self, model, ema_model_state_dict: dict, num_updates: int) -> None:
        """Resume: flat_ema from a dict written by ``ema_state_dict`` (the entries of the tensors this optimizer owns in ``model``)."""
        for k, t in model.state_dict().items():
            e = self._ema_view(t)
            if e is not None:
                e.copy_(ema_model_state_dict[k])
        self.ema_updates = int(num_updates)

    @contextlib.contextmanager
    def ema_weights(self):
        """Inside, the model runs on its EMA weights: the contents of flat_param and flat_ema are exchanged on entry and exchanged back
        on exit (also after an exception), and the derived copies are refreshed both times, so every kernel - training stacks, samplers,
        their packed planes - follows.  Take no optimizer step inside."""
        if self.flat_ema is None:
            raise RuntimeError("this optimizer keeps no EMA (ema_decay=None)")

        def exchange():
            with torch.no_grad():
                held = self.flat_param.clone()
                self.flat_param.copy_(self.flat_ema)
                self.flat_ema.copy_(held)
            self.refresh_transposes()

        exchange()
        try:
            yield self
        finally:
            exchange()

    def hyper_for_step(self, step: int, out) -> None:
        """The seven scalars of update number ``step`` at the CURRENT lr / betas of the param group -> ``out`` (7 floats)."""
        g = self.param_groups[0]
        ops.adamw_hyper(g["lr"], g["betas"][0], g["betas"][1], g["eps"], g["weight_decay"], step, out)

    def state_dict(self):
        for p in self.param_groups[0]["params"]:   # torch AdamW's per-parameter step counters, all equal here
            self.state[p]["step"] = torch.tensor(float(self._step))
        return super().state_dict()

    def load_state_dict(self, state_dict):
        views = {id(p): (self.state[p]["exp_avg"], self.state[p]["exp_avg_sq"]) for p in self.param_groups[0]["params"]}
        super().load_state_dict(state_dict)
        steps = []
        for p in self.param_groups[0]["params"]:
            st = self.state[p]
            m, v = views[id(p)]
            m.copy_(st["exp_avg"]); v.copy_(st["exp_avg_sq"])
            st["exp_avg"], st["exp_avg_sq"] = m, v
            steps.append(int(float(st["step"])))
        self._step = max(steps) if steps else 0
