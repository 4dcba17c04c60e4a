"""DDIMScheduler: the subset of ``diffusers.DDIMScheduler`` (0.31.0) the reference uses,
restated natively (reference call sites: ml/training/train.py:185-186,218;
ml/inference/plot.py:71-73,124-131; ml/training/distill.py:151-152,179-189).

Constructed exactly like the reference does — ``DDIMScheduler(beta_schedule=
"squaredcos_cap_v2", clip_sample=False)`` — everything else is the diffusers default
(1000 train steps, epsilon prediction, leading spacing, eta = 0, final alpha 1).
``clip_sample=True`` (diffusers' default, which the reference switches off) is accepted as well: ``step`` clamps the predicted clean
sample to +- ``clip_sample_range`` - or to the per-joint ``limits`` of the constructor, which diffusers has not - before it forms the
update (``sd_ddim_limit_step``); ``step(..., use_clipped_model_output=True)`` recomputes a clamped element's model output from it.
``slew=v`` or ``(v, start)`` (``ops.joint_slew``'s forms; diffusers has nothing like it): ``step`` also keeps consecutive rows of the
predicted clean sample within ``v[j]`` of each other (``sd_ddim_slew_step``, the scan of ``ops.ddim_sample(slew=...)``); the samples are
then whole (B, T, J) trajectories, since the scan walks a trajectory's rows in order.
``accel=a`` or ``(a, start2)`` (``ops.joint_accel``'s forms): ``step`` also keeps the second difference of consecutive rows within
``a[j]`` (``sd_ddim_accel_step``, the scan of ``ops.ddim_sample(accel=...)``), ahead of the slew interval and the box.
diffusers itself is not available offline: scheduler parity is UNPINNED."""

from __future__ import annotations

from types import SimpleNamespace

import torch

from . import ops


class DDIMScheduler:
    def __init__(self, num_train_timesteps: int = 1000, beta_schedule: str = "squaredcos_cap_v2",
                 clip_sample: bool = False, prediction_type: str = "epsilon", clip_sample_range: float = 1.0, limits=None, slew=None,
                 accel=None):
        if beta_schedule != "squaredcos_cap_v2" or prediction_type != "epsilon":
            raise NotImplementedError("only the configuration the reference uses is implemented: "
                                      "beta_schedule='squaredcos_cap_v2', epsilon prediction")
        if not float(clip_sample_range) >= 0:
            raise ValueError(f"clip_sample_range must be >= 0, got {clip_sample_range}")
        self.config = {"num_train_timesteps": num_train_timesteps, "beta_schedule": beta_schedule,
                       "clip_sample": bool(clip_sample), "prediction_type": prediction_type, "clip_sample_range": float(clip_sample_range)}
        # what step clamps the predicted clean sample to: per-joint limits (ops.joint_limits' forms), else +- clip_sample_range, else nothing
        self._limits_spec = limits if limits is not None else (float(clip_sample_range) if clip_sample else None)
        self._limits_dev: dict = {}
        self._slew_spec = slew   # v or (v, start): step runs the slew scan over the rows of every (B, T, J) sample
        self._slew_dev: dict = {}
        self._accel_spec = accel   # a or (a, start2): the scan's state is two rows
        self._accel_dev: dict = {}
        if accel is not None and slew is None:
            self._slew_spec = {}   # an acceleration step always carries the slew arrays: no limit, no anchor
        self._table_len = num_train_timesteps
        self.alphas_cumprod = ops.alphas_cumprod(num_train_timesteps)  # CPU fp32, like diffusers
        self._acp_dev: dict = {}
        self.num_inference_steps = None
        self.timesteps = torch.arange(num_train_timesteps - 1, -1, -1, dtype=torch.int64)

    def _check_config(self):
        # the reference overwrites config["num_train_timesteps"] after construction (train.py:186);
        # every shipped YAML uses 1000 = the table length.  Any other value is undefined there.
        if self.config["num_train_timesteps"] != self._table_len:
            raise ValueError("train_denoising_timesteps must equal the scheduler table length (1000)")

    def _acp(self, device) -> torch.Tensor:
        key = torch.device(device)
        if key not in self._acp_dev:
            self._acp_dev[key] = self.alphas_cumprod.to(key)
        return self._acp_dev[key]

    def add_noise(self, original_samples: torch.Tensor, noise: torch.Tensor, timesteps: torch.Tensor) -> torch.Tensor:
        self._check_config()
        return ops.ddim_add_noise(original_samples.contiguous(), noise.contiguous(),
                                  timesteps.to(device=original_samples.device, dtype=torch.int64).contiguous(),
                                  self._acp(original_samples.device))

    def set_timesteps(self, num_inference_steps: int, device=None) -> None:
        self._check_config()
        if num_inference_steps > self._table_len:
            raise ValueError("num_inference_steps exceeds num_train_timesteps")
        self.num_inference_steps = num_inference_steps
        self.timesteps = torch.tensor(ops.ddim_timesteps(num_inference_steps, self._table_len), dtype=torch.int64,
                                      device=device)

    def _limits(self, sample: torch.Tensor):
        """The limits as the kernel reads them, on the sample's device for its last dimension (the joints), or None: no clipping."""
        if self._limits_spec is None:
            return None
        key = (sample.device, sample.shape[-1])
        if key not in self._limits_dev:
            self._limits_dev[key] = ops._limits_req(self._limits_spec, sample.shape[-1], sample.device)
        return self._limits_dev[key]

    def _slew(self, sample: torch.Tensor):
        """(v, start) as the kernel reads them, on the sample's device for its (B, T, J) shape, or None: no slew limits."""
        if self._slew_spec is None:
            return None
        if sample.dim() != 3:
            raise ValueError(f"slew: the scan walks the rows of whole (B, T, J) samples, got {tuple(sample.shape)}")
        key = (sample.device, sample.shape[0], sample.shape[-1])
        if key not in self._slew_dev:
            self._slew_dev[key] = ops._slew_req(self._slew_spec, sample.shape[0], sample.shape[-1], sample.device)
        return self._slew_dev[key]

    def _accel(self, sample: torch.Tensor):
        """(a, start2) as the kernel reads them, on the sample's device for its (B, T, J) shape, or None: no acceleration limits."""
        if self._accel_spec is None:
            return None
        if sample.dim() != 3:
            raise ValueError(f"accel: the scan walks the rows of whole (B, T, J) samples, got {tuple(sample.shape)}")
        key = (sample.device, sample.shape[0], sample.shape[-1])
        if key not in self._accel_dev:
            self._accel_dev[key] = ops._accel_req(self._accel_spec, sample.shape[0], sample.shape[-1], sample.device)
        return self._accel_dev[key]

    def step(self, model_output: torch.Tensor, timestep, sample: torch.Tensor, use_clipped_model_output: bool = False):
        if self.num_inference_steps is None:
            raise ValueError("call set_timesteps before step")
        t = int(timestep)
        coef = ops.ddim_coefficients([t], self.alphas_cumprod, self.num_inference_steps, self._table_len)[0]
        limits = self._limits(sample)
        accel = self._accel(sample)
        slew = self._slew(sample)
        if accel is not None:
            return SimpleNamespace(prev_sample=ops.accel_step(model_output.contiguous(), sample.contiguous(), coef, accel, slew=slew, limits=limits,
                                                              reproject=use_clipped_model_output))
        if slew is not None:
            return SimpleNamespace(prev_sample=ops.slew_step(model_output.contiguous(), sample.contiguous(), coef, slew, limits=limits,
                                                             reproject=use_clipped_model_output))
        if limits is not None:
            return SimpleNamespace(prev_sample=ops.limit_step(model_output.contiguous(), sample.contiguous(), coef, limits,
                                                              reproject=use_clipped_model_output))
        return SimpleNamespace(prev_sample=ops.ddim_step(model_output.contiguous(), sample.contiguous(), coef))


class MultistepScheduler(DDIMScheduler):
    """The second-order multistep solver (DPM-Solver++ 2M in its x0 form) for the reference's loop form: the constructor,
    ``set_timesteps``, ``timesteps`` and ``add_noise`` of ``DDIMScheduler``; ``step(model_output, t, sample).prev_sample`` is the DDIM
    update plus ``w * (x0 of the step before - x0 of this step)`` (``ops.multistep_weights``, ``sd_multistep_step``: one launch).  The
    previous x0 stays on the device, in a buffer of the sample's shape; ``set_timesteps`` clears the history, so every rollout starts
    first order, and the steps must then be taken in the order of ``timesteps``.  ``clip_sample`` / ``clip_sample_range`` / ``limits`` as
    ``DDIMScheduler`` takes them, ``slew`` and ``accel`` too: the history then holds the clamped x0.

    It runs on THIS project's leading grid (``ops.ddim_timesteps``: t - ratio, the last step to alpha = 1), not on a grid of its own, so
    that its step counts compare with ``DDIMScheduler``'s: n steps here evaluate the denoiser at the same n timesteps.  Parity with
    diffusers' ``DPMSolverMultistepScheduler`` is UNPINNED for the reason ``DDIMScheduler``'s is - diffusers is not available offline
     - and that class spaces its timesteps differently by default."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self._weights, self._hist, self._next = None, None, 0

    def set_timesteps(self, num_inference_steps: int, device=None) -> None:
        super().set_timesteps(num_inference_steps, device)
        self._grid = ops.ddim_timesteps(num_inference_steps, self._table_len)
        self._weights = ops.multistep_weights(self._grid, self.alphas_cumprod, num_inference_steps, self._table_len)
        self._hist, self._next = None, 0

    def step(self, model_output: torch.Tensor, timestep, sample: torch.Tensor, use_clipped_model_output: bool = False):
        if self.num_inference_steps is None:
            raise ValueError("call set_timesteps before step")
        t = int(timestep)
        i = self._next
        if i >= len(self._grid) or self._grid[i] != t:
            if t != self._grid[0]:
                raise ValueError(f"MultistepScheduler.step: the history term needs the steps in the order of timesteps; expected "
                                 f"t = {self._grid[i] if i < len(self._grid) else self._grid[0]}, got {t}")
            i = 0   # a new rollout on the same grid: no history yet
        coef = ops.ddim_coefficients([t], self.alphas_cumprod, self.num_inference_steps, self._table_len)[0]
        if self._hist is None or self._hist.shape != sample.shape or self._hist.device != sample.device:
            self._hist = torch.empty_like(sample, memory_format=torch.contiguous_format)
        limits = self._limits(sample)
        accel = self._accel(sample)
        slew = self._slew(sample)
        if accel is not None:   # the history holds the x0 the acceleration scan returned
            out = ops.accel_step(model_output.contiguous(), sample.contiguous(), coef, accel, slew=slew, limits=limits, hist=self._hist,
                                 w=float(self._weights[i]), reproject=use_clipped_model_output)
        elif slew is not None:   # the history holds the slewed and clamped x0
            out = ops.slew_step(model_output.contiguous(), sample.contiguous(), coef, slew, limits=limits, hist=self._hist,
                                w=float(self._weights[i]), reproject=use_clipped_model_output)
        elif limits is not None:   # clip_sample / limits: the history holds the clamped x0
            out = ops.limit_step(model_output.contiguous(), sample.contiguous(), coef, limits, hist=self._hist, w=float(self._weights[i]),
                                 reproject=use_clipped_model_output)
        else:
            out = ops.multistep_step(model_output.contiguous(), sample.contiguous(), self._hist, coef, float(self._weights[i]))
        self._next = i + 1
        return SimpleNamespace(prev_sample=out)
