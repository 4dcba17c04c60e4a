"""End2EndDiffusionTransformer — the boundary class of the hot path
(reference: soccer_diffusion/ml/model/model.py:16-179).

Same keyword constructor, same three methods, same buffers (``mean``, ``std``) and the
same ``state_dict`` keys, so reference checkpoints load unchanged.  Extra (not in the
reference class): ``sample`` runs the whole DDIM loop natively."""

from __future__ import annotations

from typing import Optional, Sequence

import torch
from torch import nn

from ... import derived, ops
from ...derived import cache as _model_cache   # (per-model caches: the loop samplers, the captured graphs)
from .decoder import DiffusionActionGenerator
from .encoder.encoders import GameStateEncoder, IMUEncoder, JointEncoder
from .encoder.image import ImageEncoderType, SequenceEncoderType, image_sequence_encoder_factory
from .misc import StepToken

NUM_HEADS = 4  # fixed by the reference (model.py:57,71,85,115)


class End2EndDiffusionTransformer(nn.Module):
    def __init__(
        self,
        num_joints: int,
        hidden_dim: int,
        use_action_history: bool,
        num_action_history_encoder_layers: int,
        max_action_context_length: int,
        encoder_patch_size: int,
        use_imu: bool,
        imu_orientation_embedding_method,
        num_imu_encoder_layers: int,
        imu_context_length: int,
        use_joint_states: bool,
        joint_state_encoder_layers: int,
        joint_state_context_length: int,
        use_images: bool,
        image_encoder_type: ImageEncoderType,
        image_sequence_encoder_type: SequenceEncoderType,
        num_image_sequence_encoder_layers: int,
        image_context_length: int,
        image_use_final_avgpool: bool,
        image_resolution: int,
        use_gamestate: bool,
        num_decoder_layers: int,
        trajectory_prediction_length: int,
    ):
        super().__init__()
        d = hidden_dim
        self.hidden_dim, self.num_joints = d, num_joints
        self.trajectory_prediction_length = trajectory_prediction_length
        self.step_encoding = StepToken(d)

        def seq(kind, enabled, *args):
            return kind(*args) if enabled else None

        self.action_history_encoder = seq(JointEncoder, use_action_history, num_joints, encoder_patch_size, d,
                                          num_action_history_encoder_layers, NUM_HEADS, max_action_context_length)
        self.imu_encoder = seq(IMUEncoder, use_imu, imu_orientation_embedding_method, encoder_patch_size, d,
                               num_imu_encoder_layers, NUM_HEADS, imu_context_length)
        self.joint_states_encoder = seq(JointEncoder, use_joint_states, num_joints, encoder_patch_size, d,
                                        joint_state_encoder_layers, NUM_HEADS, joint_state_context_length)
        self.image_sequence_encoder = (
            image_sequence_encoder_factory(
                encoder_type=image_sequence_encoder_type, image_encoder_type=image_encoder_type, hidden_dim=d,
                num_layers=num_image_sequence_encoder_layers, max_seq_len=image_context_length,
                use_final_avgpool=image_use_final_avgpool, resolution=image_resolution)
            if use_images else None
        )
        self.game_state_encoder = GameStateEncoder(d) if use_gamestate else None
        self.diffusion_action_generator = DiffusionActionGenerator(
            num_joints=num_joints, hidden_dim=d, num_layers=num_decoder_layers, num_heads=NUM_HEADS,
            max_seq_len=trajectory_prediction_length)
        self.register_buffer("mean", torch.zeros(num_joints))
        self.register_buffer("std", torch.ones(num_joints))

    # ---- reference API -----------------------------------------------------------------
    def encode_input_data(self, input_data: dict[str, torch.Tensor]) -> list[torch.Tensor]:
        """Context tokens per enabled modality, in the reference's fixed order
        [action history, IMU, joint state, images, game state] (model.py:135-144)."""
        pairs = ((self.action_history_encoder, "joint_command_history"), (self.imu_encoder, "rotation"),
                 (self.joint_states_encoder, "joint_state"), (self.image_sequence_encoder, "image_data"),
                 (self.game_state_encoder, "game_state"))
        return [enc(input_data[key]) for enc, key in pairs if enc is not None]

    def forward(self, input_data: dict[str, torch.Tensor], noisy_action_predictions: torch.Tensor,
                step: torch.Tensor, draws: int = 1) -> torch.Tensor:
        """``draws`` = K > 1 (not in the reference): ``input_data`` holds C windows, encoded once; ``noisy_action_predictions`` C K
        trajectories, trajectory b of window b // K (``forward_with_context``)."""
        if draws != 1:   # (validated before any encoder runs)
            ops._draws_req(draws, noisy_action_predictions.shape[0], None)
        return self.forward_with_context(self.encode_input_data(input_data), noisy_action_predictions, step, draws)

    def forward_with_context(self, context: Sequence[torch.Tensor], noisy_action_predictions: torch.Tensor,
                             step: torch.Tensor, draws: int = 1) -> torch.Tensor:
        """Predicted noise for x_t given precomputed context tokens; the step token is the
        LAST memory row (model.py:176).  ``step`` is int64 or float, shape (B,) (or (1,) at B=1).
        ``draws`` = G > 1 (not in the reference): the context tensors hold C rows, ``x`` C * G trajectories, trajectory b reads context
        b // G.  On the trajectory kernels the context is folded once per row (``ops.LoopSampler(draws=G)``); elsewhere the rows are
        expanded and the call is the one with ``draws`` = 1 - the same result, only not shared.  With a tape (training) the context is
        projected to K | V once per row and layer where ``training.denoiser_forward_autograd`` takes the shared route, and its gradient
        is the sum over the G draws in a fixed order."""
        x = noisy_action_predictions
        B = x.shape[0]
        if draws != 1:
            ops._draws_req(draws, B, context[0].shape[0] if len(context) else None)
        if step.dim() == 0:
            step = step.reshape(1)
        if step.shape[0] != B and step.shape[0] != 1:
            raise RuntimeError(f"step has {step.shape[0]} entries for a batch of {B}")  # torch.cat would fail too
        step = step.to(x.device)
        eps = self._loop_form_eps(context, x, step, draws)
        if eps is not None:
            return eps
        if draws != 1:
            dag = self.diffusion_action_generator
            tape = torch.is_grad_enabled() and (any(c.requires_grad for c in context) or any(p.requires_grad for p in dag.parameters())
                                                or self.step_encoding.token.requires_grad)
            if len(context) and (tape or (self.training and dag.dropout.p > 0.0)):
                # training (train_step(draws=)): the context stays C rows - projected once per context where the shared
                # cross-attention applies, expanded by a node with a fixed-order backward where it does not
                from ...training import denoiser_forward_autograd, step_token_autograd

                tokens = step_token_autograd(self.step_encoding, step if step.shape[0] == B else step.expand(B), fixed_order=True)
                ctx = context[0] if len(context) == 1 else torch.cat(list(context), dim=1)
                return denoiser_forward_autograd(dag, x, ctx, draws=draws, tokens=tokens)
            return self.forward_with_context([c.repeat_interleave(draws, 0) for c in context], x, step)
        if step.shape[0] != B:
            step = step.expand(B)
        memory = self._assemble_memory(context, step, B, x.device)
        return self.diffusion_action_generator(x, memory)

    def _loop_form_eps(self, context, x: torch.Tensor, step: torch.Tensor, draws: int = 1) -> Optional[torch.Tensor]:
        """Inference calls (no tape, no live dropout) on shapes the trajectory kernels take run ``ops.LoopSampler``: the reference's
        loops call this method once per DDIM step with the same context (plot.py:122-131, distill.py:179-189, ros.py:301-310), so the
        weights' split planes and the context's folded K / V are prepared on the first call and reused by the following ones.
        Returns None where that route does not apply (training, a differentiable input, CPU tensors, other shapes)."""
        import os

        dag = self.diffusion_action_generator
        if (not x.is_cuda or x.dtype != torch.float32 or x.dim() != 3 or (self.training and dag.dropout.p > 0.0)
                or os.environ.get("SD_LOOP_FORM", "1") == "0"):
            return None
        if torch.is_grad_enabled() and (x.requires_grad or any(c.requires_grad for c in context)
                                        or any(p.requires_grad for p in dag.parameters()) or self.step_encoding.token.requires_grad):
            return None
        if any((not c.is_cuda) or c.dtype != torch.float32 or c.dim() != 3 or c.shape[0] * draws != x.shape[0] for c in context):
            return None
        B, T, _ = x.shape
        Mc = sum(int(c.shape[1]) for c in context)
        n_tok = 1 if step.shape[0] == 1 else B
        packed = dag.packed()
        cap = min(ops.sampler_cap(packed), 3)   # (mode 4 needs its status word read back: a host synchronisation per call)
        key = (B, T, Mc, n_tok, x.device, cap) if draws == 1 else (B, T, Mc, n_tok, x.device, cap, draws)
        cache = _model_cache(self, "loop")
        ls = cache.get(key)
        if ls is None:
            if len(cache) >= 4:
                cache.clear()   # a prepared workspace is pinned memory: a handful of shapes at a time
            ls = cache[key] = ops.LoopSampler(packed, B, T, Mc, n_tok, x.device, max_mode=cap, draws=draws)
        if not ls.supported:
            return None
        if step.dtype not in (torch.int64, torch.float32):
            step = step.to(torch.float32 if step.is_floating_point() else torch.int64)
        tokens = ops.step_token(step.contiguous(), self.step_encoding._freq, self.step_encoding.token.detach()).view(n_tok, self.hidden_dim)
        # (dag.packed() rebuilds its descriptor when a parameter's storage moved: its identity stands for the pointers)
        versions = derived.version_key(*dag.parameters())
        wkey = None if versions is None else (id(packed), versions)
        return ls.eps(packed, list(context), tokens, x.contiguous(), wkey)

    # ---- extras ------------------------------------------------------------------------
    def dropout_stacks(self):
        """The transformer stacks that carry dropout (decoder + every enabled context encoder), in a fixed order."""
        from .encoder.encoders import BaseEncoder

        stacks = [self.diffusion_action_generator]
        for m in self.modules():
            if isinstance(m, BaseEncoder):
                stacks.append(m)
        return stacks

    def set_dropout(self, p: float, seed: Optional[int] = None) -> "End2EndDiffusionTransformer":
        """Dropout probability of every transformer layer (live in ``train()`` mode only).  The reference never sets it,
        i.e. trains with torch's default 0.1 - also the default here; 0 selects the parity path (golden gradients).
        ``seed`` keys the Philox masks (default: ``torch.initial_seed()`` at first use; give every data-parallel rank
        its own).  The ResNet / Swin image backbones (torch.nn modules) are not affected."""
        if not 0.0 <= p < 1.0:
            raise ValueError("dropout probability must be in [0, 1)")
        for i, m in enumerate(self.dropout_stacks()):
            m.dropout.p = float(p)
            m.dropout.salt = i
            if seed is not None:
                m.dropout.seed = int(seed)
        return self

    def _assemble_memory(self, context, step, B, device) -> torch.Tensor:
        grad_path = torch.is_grad_enabled() and any(c.requires_grad for c in context)
        if grad_path or (torch.is_grad_enabled() and self.step_encoding.token.requires_grad):
            from ...training import step_token_autograd

            return torch.cat(list(context) + [step_token_autograd(self.step_encoding, step)], dim=1)
        d = self.hidden_dim
        M = sum(int(c.shape[1]) for c in context) + 1
        memory = torch.empty(B, M, d, dtype=torch.float32, device=device)
        at = 0
        for c in context:
            n = c.shape[1]
            memory[:, at : at + n].copy_(c)
            at += n
        step = step.contiguous()
        if step.dtype not in (torch.int64, torch.float32):
            step = step.to(torch.float32 if step.is_floating_point() else torch.int64)
        # the kernel writes sample b's token straight into row M-1 of its memory block
        ops.step_token(step, self.step_encoding._freq, self.step_encoding.token.detach(),
                       out=memory.view(-1)[(M - 1) * d :], row_stride=M * d)
        return memory

    @torch.no_grad()
    def sample(self, context: Sequence[torch.Tensor], x_T: torch.Tensor, num_inference_steps: int,
               return_trace: bool = False, alphas_cumprod: Optional[torch.Tensor] = None, use_graph: bool = False,
               with_dropout: bool = False, max_mode: Optional[int] = None, pin=None, draws: int = 1, hold=None, solver: str = "ddim",
               limits=None, reproject: bool = False, slew=None, accel=None):
        """The reference's denoising loop (plot.py:122-131 / distill.py:179-189 / ros.py:301-310)
        as one native call: n x (denoiser forward + DDIM update) with the context K/V cached.
        ``use_graph`` replays the rollout from a hipGraph captured for this (B, T, M, n) shape.
        ``max_mode``: the highest sampler mode (``sd_sampler_mode``) the call may run; None = ``ops.default_sampler_cap()`` = 3 (three fp16
        products at every site: valid for any weights); 4 opts in to the guarded two-product Q | K | V site (falls back to 3 by itself).
        The native rollout has no dropout (inference).  ``with_dropout=True`` on a model in ``train()`` mode instead
        steps through ``forward_with_context`` + the scheduler update like the reference's loop does, dropout live in
        every call - what distill.py's teacher, which is never put into eval mode, actually computes (distill.py:127-189).
        ``pin = (known, rows)``: the leading ``rows[b]`` rows of trajectory b are held to ``known`` (normalised space) at every
        denoising step and the rest is sampled to fit (``ops.ddim_sample``); a captured graph serves every ``rows`` and ``known``.
        Not with ``with_dropout``.
        ``draws`` = G > 1: G draws per observation - the context tensors hold B / G observations, ``x_T`` B trajectories, trajectory b reads
        observation b // G and the G draws share its folded context (``ops.ddim_sample``).  Not with ``with_dropout``.
        ``hold = (known, mask)``: the element form of ``pin`` - element (b, t, j) is held to ``known`` where ``mask`` (a bool tensor
        (B, T, J), (T, J) or (J,), or the (B, T) int32 words of ``ops.hold_mask``) is set: joints another module owns, keyframes.  A captured
        graph serves every mask and ``known``.  Not together with ``pin`` (``ops.hold_mask(rows=...)`` composes them), not with
        ``with_dropout``.
        ``solver``: "ddim" (default: every call is the call without this argument) or "multistep" - the second-order multistep solver
        (DPM-Solver++ 2M in its x0 form, ``ops.multistep_weights``) on the same timesteps: no extra denoiser evaluation, one history term
        per element inside the step launch; meant for fewer steps.  It composes with ``pin``, ``hold``, ``draws``, ``use_graph`` and
        ``return_trace``.  Not with ``with_dropout``.
        ``limits`` (``(lo, hi)`` of (J,) floats, one range r, ``{joint: (lo, hi)}`` or ``ops.joint_limits(...)``; normalised space): the
        predicted clean trajectory is clamped to the joints' limits at every step inside the step launch (``ops.ddim_sample``; diffusers'
        ``clip_sample``, per joint), so the returned free elements lie inside them bit for bit; ``reproject``: diffusers'
        ``use_clipped_model_output``.  It composes with ``pin``, ``hold``, ``draws``, ``solver``, ``use_graph`` (the graph reads the limits
        on the device: one capture serves every value) and ``return_trace``.  Not with ``with_dropout``; J <= 32.
        ``slew`` (``v`` or ``(v, start)``, ``ops.joint_slew``'s forms; normalised space): consecutive rows of the predicted clean
        trajectory are kept within ``v[j]`` of each other at every step (row 0 against ``start`` (B, J)), then clamped to ``limits``
        (``ops.ddim_sample(slew=...)``).  It composes with what ``limits`` composes with.
        ``accel`` (``a`` or ``(a, start2)``, ``ops.joint_accel``'s forms; normalised space): the second difference of consecutive rows of
        the predicted clean trajectory is kept within ``a[j]`` at every step (rows -1 and -2: ``slew``'s ``start`` and ``start2``), ahead
        of the slew interval and the box (``ops.ddim_sample(accel=...)``, which states what this is not: no braking ahead of the box).  It
        composes with what ``slew`` composes with."""
        if accel is not None and with_dropout:
            raise ValueError("sample: accel is a feature of the native rollout; with_dropout steps through forward_with_context")
        if slew is not None and with_dropout:
            raise ValueError("sample: slew is a feature of the native rollout; with_dropout steps through forward_with_context")
        if limits is not None and with_dropout:
            raise ValueError("sample: limits is a feature of the native rollout; with_dropout steps through forward_with_context")
        if solver not in ("ddim", "multistep"):
            raise ValueError(f"sample: solver must be 'ddim' or 'multistep', got {solver!r}")
        if solver != "ddim" and with_dropout:
            raise ValueError("sample: solver is a feature of the native rollout; with_dropout steps through forward_with_context")
        if hold is not None and with_dropout:
            raise ValueError("sample: hold is a feature of the native rollout; with_dropout steps through forward_with_context")
        if hold is not None and pin is not None:
            raise ValueError("sample: pin and hold exclude each other - compose them through ops.hold_mask(mask, B, T, J, device, rows=rows)")
        if pin is not None and with_dropout:
            raise ValueError("sample: pin is a feature of the native rollout; with_dropout steps through forward_with_context")
        if draws != 1 and with_dropout:
            raise ValueError("sample: draws is a feature of the native rollout; with_dropout steps through forward_with_context")
        if with_dropout and self.training and self.diffusion_action_generator.dropout.p > 0.0:
            from ...scheduler import DDIMScheduler

            sch = DDIMScheduler(beta_schedule="squaredcos_cap_v2", clip_sample=False)
            sch.set_timesteps(num_inference_steps)
            x, trace = x_T, []
            for t in sch.timesteps.tolist():
                eps = self.forward_with_context(context, x, torch.full((x.shape[0],), t, dtype=torch.int64, device=x.device))
                x = sch.step(eps, t, x).prev_sample
                if return_trace:
                    trace.append(x)
            return (x, torch.stack(trace)) if return_trace else x
        ts = ops.ddim_timesteps(num_inference_steps)
        acp = ops.alphas_cumprod() if alphas_cumprod is None else alphas_cumprod
        coef = ops.ddim_coefficients(ts, acp, num_inference_steps)
        msw = ops.multistep_weights(ts, acp, num_inference_steps) if solver == "multistep" else None
        ctx = torch.cat(list(context), dim=1).contiguous() if len(context) else None
        packed = self.diffusion_action_generator.packed()
        if use_graph and not return_trace:
            B, T, _ = x_T.shape
            Mc = 0 if ctx is None else ctx.shape[1]
            cap = ops.sampler_cap(packed, max_mode)   # as ops.ddim_sample_guarded
            # the weights are read through pointers at replay (their addresses are the key); the step-token table is captured by value
            token = derived.source_key(self.step_encoding.token)
            key = (B, T, Mc, num_inference_steps, x_T.device, self.diffusion_action_generator._signature(), token, cap, pin is not None, draws, hold is not None, solver,
                   limits is not None, bool(reproject), slew is not None, accel is not None)
            cache = _model_cache(self, "graphs")
            if token is None or key not in cache:
                cache.clear()  # one shape at a time: a graph pins its workspace
                cache[key] = ops.GraphedSampler(packed, B, T, Mc, self.step_encoding.table(ts, x_T.device), coef, max_mode=cap,
                                                pin=pin is not None, draws=draws, hold=hold is not None, multistep=msw, limits=limits is not None,
                                                reproject=reproject, slew=slew is not None, accel=accel is not None)
            if limits is not None:
                cache[key].set_limits(limits)
            elif slew is not None or accel is not None:
                cache[key].set_limits({})
            if slew is not None:
                cache[key].set_slew(slew)
            elif accel is not None:
                cache[key].set_slew({})
            if accel is not None:
                cache[key].set_accel(accel)
            out = cache[key](ctx, x_T, pin, hold)
            word = int(cache[key].status.item())
            if word == 0:
                return out
            if word & ops.STATUS_SHARP_LOGITS:
                packed.sampler_cap = 3   # pinned before the eager rerun: it starts on mode 3, not on mode 4 again
            # range guard tripped (ops.ddim_sample_guarded): fall through to the guarded eager path
        tokens = self.step_encoding.table(ts, x_T.device)
        return ops.ddim_sample_guarded(packed, ctx, tokens, coef, x_T.contiguous(), trace=return_trace, max_mode=max_mode, pin=pin, draws=draws, hold=hold, multistep=msw,
                                       limits=limits, reproject=reproject, slew=slew, accel=accel)

    @torch.no_grad()
    def sample_direct(self, context: Sequence[torch.Tensor], x_T: torch.Tensor, hold=None, limits=None, slew=None, draws: int = 1,
                      raw: bool = False, max_mode: Optional[int] = None, accel=None):
        """A distilled one-step decoder's tick (ros.py:293-298) under ``sample``'s guarantees: ``forward_with_context(context, x_T,
        zeros)`` - whose output is the clean trajectory, not a noise prediction - plus the projection of ``sample``'s ``hold``, ``slew``
        and ``limits`` (same forms, normalised space), in ONE launch on the trajectory kernels (``ops.direct_sample``).  ``draws`` = G:
        the context tensors hold B / G observations; G start noises give G different trajectories.  ``raw=True`` also returns the
        unprojected prediction, which is ``forward_with_context``'s value bit for bit.  With nothing set the result is that value.
        There is no ``pin``, no ``solver`` and no ``reproject``: one step has no rows that could adapt to pinned ones, no history and
        no eps to recompute.  The range guard is read back as in ``sample`` (``ops.direct_sample_guarded``).  ``accel``: ``sample``'s
        acceleration limits - then two launches, the plain direct launch and the projection (``ops.direct_sample``)."""
        ctx = torch.cat(list(context), dim=1).contiguous() if len(context) else None
        packed = self.diffusion_action_generator.packed()
        t0 = torch.zeros(1, dtype=torch.int64, device=x_T.device)
        token = ops.step_token(t0, self.step_encoding._freq, self.step_encoding.token.detach()).view(1, self.hidden_dim)
        return ops.direct_sample_guarded(packed, ctx, token, x_T.contiguous(), hold=hold, limits=limits, slew=slew, draws=draws, raw=raw,
                                         max_mode=max_mode, accel=accel)
