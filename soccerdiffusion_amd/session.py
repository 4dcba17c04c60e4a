"""Closed-loop policy session: the receding-horizon tick of the reference's robot node (soccer_diffusion/ml/inference/ros.py:165-335) with
the sensor buffers on the device.

ros.py keeps every stream as a Python list of CPU tensors, stacks and uploads all of them at every tick and runs the image backbone on
the whole frame window again, although only the frames that arrived since the last tick are new (its own TODO, ros.py:180-183).  A
``PolicySession`` owns one ring per enabled modality in device memory (csrc/sd_session.hip): ``push_*`` appends rows, ``push_image``
encodes the new frames only and stores their tokens, and ``step`` is windows -> context encoders -> rollout -> commit.  In eval mode a
frame's token depends on that frame alone (BatchNorm on running statistics, no dropout), so caching it changes nothing but the batch the
backbone kernels see.

    s = PolicySession(model, num_inference_steps=30, batch=1, hyperparams=checkpoint["hyperparams"])
    s.push_joint_state(q); s.push_rotation(r); s.push_image(frame)     # the callbacks / timers of ros.py:165-257
    s.push_orientation(quat); s.push_camera(frame_u8)                 # the same from raw sensor data: xyzw quaternions, uint8 (H, W, 3) frames
    traj = s.step()                                                   # (B, T, J): what ros.py:321-335 publishes

Every entry point takes ``robots=`` for a subset of the batch (robots that tick at their own times, episodes that end robot by robot):

    s.push_image(frame, robots=[2]); traj = s.step(robots=[0, 2])      # (2, T, J); robot 1's rings are neither read nor written
    s.reset(robots=done)                                               # a (B,) bool mask, on the device as it is, or an index list

Overlapping ticks (``carry=K``): a tick commits the first ``advance`` rows of its trajectory to the action history and carries the
next K rows into the following tick, whose first K rows are pinned to them at every denoising step (``ops.ddim_sample(pin=...)``) - the
new trajectory continues the one the robot is still executing instead of being an unrelated draw:

    s = PolicySession(model, batch=1, carry=4, advance=5, hyperparams=hp)   # T = 10: tick every 5 points, 4 points held across the seam
    traj = s.step()                                                         # traj[:, :4] == the previous tick's traj[:, 5:9], bit for bit

Several draws per tick (``draws=G``): the context is encoded once per robot, G trajectories are sampled from it on the shared folded
context (``ops.ddim_sample(draws=G)``), and the medoid of the G - the draw with the smallest summed squared distance to the others - is
chosen on the device, committed and returned instead of a single, possibly outlying, sample:

    s = PolicySession(model, batch=2, draws=4, hyperparams=hp)
    traj, all_draws, index = s.step(return_draws=True)                      # (2, T, J), (2, 4, T, J), (2,): traj[b] == all_draws[b, index[b]]

With overlapping ticks the draw can instead be the one that continues the previous plan (``select="coherent"``: the backward-coherence
criterion of Bidirectional Decoding, ``ops.select_coherent``) - successive ticks of a multimodal policy then stay on one mode:

    s = PolicySession(model, batch=2, draws=8, advance=5, select="coherent", hyperparams=hp)   # T = 10: five rows of overlap
    traj = s.step(); s.selection()                                          # {"index": (2,), "cost": (2, 8)} of that tick

Held joints (``holds=True``): joints that another module owns - the head follows the ball tracker, a motor is switched off - are held at
given angles INSIDE the rollout (``ops.ddim_sample(hold=...)``), so the free joints are sampled to fit what the robot will really do:

    s = PolicySession(model, batch=3, holds=True, hyperparams=hp)
    s.hold([0, 1], [0.3, -0.7], robots=[0, 2])                              # radians as published; until release(), through reset() too
    traj = s.step()                                                         # traj[[0, 2]][:, :, [0, 1]] are those angles in every row

A distilled decoder (``cli distill``'s student, the checkpoint ros.py:47 loads: one forward at t = 0 whose output is the clean trajectory)
takes the same ``limits``, ``slew``, ``holds``, ``draws`` / ``select`` and ``use_graph`` with ``direct=True`` - its output is the x0 they are defined on, projected
inside the one launch (``model.sample_direct``); it refuses ``carry``, ``solver="multistep"`` and ``reproject``:

    s = PolicySession.from_checkpoint("student.pth", batch=1, direct=True, limits=(lo, hi), slew=0.16, draws=8, advance=5, select="coherent", use_graph=True)

There is no CPU path and no fallback: the model must be on the GPU and in eval mode."""

from __future__ import annotations

import gc
import math
import weakref
from typing import Optional

import numpy as np
import torch

from . import ops
from .derived import current, version_key

KEYS = ("joint_command_history", "rotation", "joint_state")   # the ring modalities, in encode_input_data's order
WRAPPED = {"joint_command_history": True, "rotation": False, "joint_state": True}   # (x + 3 pi) % (2 pi): ros.py:266-273
DEFAULT_GAME_STATE = 2   # ros.py:274
SELECTORS = ("medoid", "coherent")   # PolicySession(select=...): which of a tick's draws is committed
# what a distilled session without direct=True says when it refuses limits, slew, holds, draws or use_graph
_DIRECT_HINT = "pass direct=True: its output is x0, which is then projected inside the one launch (model.sample_direct)"


class _GraphedTick:
    """Windows, context encoders and rollout of one session's tick as one captured hipGraph (linear; the warm-up and capture recipe of
    ``ops.GraphedSampler``).  The graph changes no ring - the commit stays outside - so warming it up and capturing it leave the
    session's state alone.  A call copies the noise into the captured buffer, replays, reads the range-guard word back as the eager
    route does (``ops.ddim_sample_guarded``) and returns the captured sample buffer, which the next call overwrites.  A session with
    carry captures the pinned rollout on the session's own pin buffers, which the commit outside the graph rewrites: the same graph
    serves a first tick (no rows pinned), every later one and the ticks after a partial reset.  For a distilled decoder the captured
    tick is windows, context encoders, the ONE direct launch (``ops.direct_sample``: the forward at t = 0 and the projection of its output)
    and the selection; its step token is computed inside the tick from the session's device zeros."""

    def __init__(self, session: "PolicySession", x_T: torch.Tensor):
        m, dev = session.model, session.device
        # a weak reference: the session owns its tick, and with a strong one back the pair would be a cycle that only Python's collector
        # frees - at an arbitrary allocation, possibly inside a LATER capture, where destroying a graph is not permitted and aborts
        self.session = weakref.proxy(session)
        ts = ops.ddim_timesteps(session.n_steps)
        self.packed = m.diffusion_action_generator.packed()
        if not session.distilled:   # (a distilled decoder has no schedule: its one step token is computed inside the tick)
            self.tokens = m.step_encoding.table(ts, dev)
            self.coef = ops.ddim_coefficients(ts, ops.alphas_cumprod(), session.n_steps)
        self.msw = ops.multistep_weights(ts, ops.alphas_cumprod(), session.n_steps) if session.solver == "multistep" else None
        # (limits: the session's own device arrays, which set_limits rewrites in place - the capture stays)
        self.lim = session._direct_lim() if session.distilled else session._lim()
        self.cap = ops.sampler_cap(self.packed, 3)
        self.noise = x_T.clone()
        self.status = torch.zeros(1, dtype=torch.int32, device=dev)
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            self._run()   # outside capture: lazy module loads, the workspaces of this stream
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        self.graph = torch.cuda.CUDAGraph()
        collecting = gc.isenabled()
        gc.disable()   # no collection inside the capture: a dead graph of another owner that it found would be destroyed mid-capture
        try:
            with torch.cuda.graph(self.graph):
                self._run()
        finally:
            if collecting:
                gc.enable()

    def _run(self) -> None:
        s = self.session
        if s.distilled:   # windows, context encoders, ONE direct launch (ops.direct_sample) and the selection
            cond = s._direct_cond()
            self.ctx = s._context()
            ctx = torch.cat(self.ctx, dim=1).contiguous() if self.ctx else None
            m = s.model
            token = ops.step_token(s._t0[:1], m.step_encoding._freq, m.step_encoding.token.detach()).view(1, m.hidden_dim)
            self.all = ops.direct_sample(self.packed, ctx, token, self.noise, status=self.status, max_mode=self.cap, draws=s.draws, **cond, **self.lim)
            if s.draws == 1:
                self.x = self.all
            else:
                self.index, self.x, self.cost = s._select(self.all)
            return
        cond = s._cond()   # (holds: the mask's compose launch is part of the captured tick; it reads the session's static buffers only)
        self.ctx = s._context()
        ctx = torch.cat(self.ctx, dim=1).contiguous() if self.ctx else None
        if s.draws == 1:
            self.x = ops.ddim_sample(self.packed, ctx, self.tokens, self.coef, self.noise, status=self.status, max_mode=self.cap, **cond,
                                     multistep=self.msw, **self.lim)
            return
        # G draws per robot on the shared context, and the selected one: the selection is part of the captured tick (select="coherent"
        # reads the session's plan, which the commit outside the graph rewrites in place)
        self.all = ops.ddim_sample(self.packed, ctx, self.tokens, self.coef, self.noise, status=self.status, max_mode=self.cap, **cond,
                                   draws=s.draws, multistep=self.msw, **self.lim)
        self.index, self.x, self.cost = s._select(self.all)

    def __call__(self, x_T: torch.Tensor):
        """The sample (B, T, J); with draws > 1: (the selected sample, all draws (B * G, T, J), index (B,), cost (B, G) or None)."""
        self.noise.copy_(x_T)
        self.graph.replay()
        s = self.session
        if int(self.status.item()) == 0:
            return self.x if s.draws == 1 else (self.x, self.all, self.index, self.cost)
        # the range guard tripped: model.sample's guarded eager route on the context the replay has just encoded
        if s.distilled:
            x = s.model.sample_direct(self.ctx, x_T, draws=s.draws, max_mode=3, **s._direct_cond(), **s._direct_lim()).contiguous()
        else:
            x = s.model.sample(self.ctx, x_T, s.n_steps, max_mode=3, **s._cond(), draws=s.draws, solver=s.solver, **s._lim()).contiguous()
        if s.draws == 1:
            return x
        index, chosen, cost = s._select(x)
        return chosen, x, index, cost


class PolicySession:
    def __init__(self, model, num_inference_steps: int = 30, batch: int = 1, distilled: Optional[bool] = None, seed: int = 0,
                 hyperparams: Optional[dict] = None, use_graph: bool = False, carry: int = 0, advance: Optional[int] = None, draws: int = 1,
                 select: str = "medoid", holds: bool = False, solver: str = "ddim", limits=None, reproject: bool = False, slew=None,
                 coherence_decay: float = 0.5, contrast: float = 0.0, direct: bool = False, accel=None):
        """``model``: an End2EndDiffusionTransformer in eval mode on a GPU.  ``hyperparams``: the checkpoint's dictionary (default: the
        model's ``hyperparams`` attribute where it has one).  REQUIRED for a model with images: the model does not keep its
        ``image_resolution`` (the size of the all-zero start frames), nor ``image_context_length`` where it has no sequence encoder;
        also read for ``distilled_decoder`` unless ``distilled`` says it.  ``use_graph``: windows, context encoders and rollout of
        ``step`` are replayed from one captured hipGraph (a distilled decoder: windows, encoders, the one direct launch and the selection).
        ``direct=True`` (a DISTILLED decoder only - one forward at t = 0 whose output is the clean trajectory: ros.py:293-298): the session
        takes ``limits``, ``slew``, ``holds``, ``draws`` / ``select`` and ``use_graph`` through ``model.sample_direct``: the network's
        output is x0, on which all of them are defined - a one-step model is the last step of a limited rollout alone.  Without the flag
        a distilled session refuses these options as it always did (nothing that ran before runs differently), and the message names it.  G start noises give G different trajectories,
        so the selectors mean what they mean for the rollout.  It refuses ``carry`` (one step cannot adapt its free rows to pinned ones:
        ``select="coherent"`` plus ``slew`` from the last committed row is its continuity), ``solver="multistep"`` (no history) and
        ``reproject`` (no eps to recompute), with or without the flag.  Built with none of the options it makes the calls it always made:
        ``forward_with_context``.
        ``carry`` / ``advance`` (overlapping ticks): a tick pushes the first ``advance`` rows of its trajectory into the action history
        (default: T - carry) and pins the first ``carry`` rows of the next tick to its rows [advance, advance + carry), in normalised
        space as sampled, at every denoising step.  ``advance`` is the number of trajectory points between two ticks.  carry = 0 with
        the default advance is the session without any of this, launch for launch.  Not for a distilled decoder (no rollout to pin).
        ``draws`` = G / ``select``: a tick samples G trajectories per robot from the once-encoded context and commits and returns the
        one ``select`` names - "medoid": the draw closest to all others (``ops.select_medoid``, on the device).  With ``carry`` all G
        draws share the seam and the carried rows come from the selected draw.  draws = 1 is the session without any of this, launch
        for launch (no selection launch).
        ``select="coherent"`` / ``coherence_decay`` / ``contrast`` (overlapping ticks only: ``advance`` < T): the draw that continues the
        robot's previous plan (``ops.select_coherent``; the backward-coherence criterion of Bidirectional Decoding, Liu et al. 2024).  Rows
        [advance, T) of the last committed trajectory and rows [0, T - advance) of the new draws describe the same instants; the draw with
        the smallest weighted squared distance over them is committed, row tau weighted ``coherence_decay`` ** tau (0.5 is the paper's
        value and has NOT been measured on this policy), plus ``contrast`` (per element, >= 0) times the medoid score.  The session keeps
        the last committed trajectory per robot in normalised space on the device, NaN until the robot's first tick and after its
        ``reset``: such a robot's tick commits the medoid.  The plan is written beside the commit, outside a captured tick.  The rows
        pinned by ``carry`` equal the plan's and contribute exactly 0.  ``selection()`` returns the last tick's indices and costs.  It
        composes with ``carry``, ``holds``, ``limits``, ``slew``, ``solver``, ``robots=`` and ``use_graph``; ``select="medoid"`` is the
        session without any of this, launch for launch.
        ``holds=True``: the session can hold chosen joints of chosen robots at given angles inside the rollout (``hold`` / ``release``:
        joints another module owns, a motor that is switched off) - the free joints are sampled to fit them.  It allocates the known-value
        buffer, a word of held joints per robot and the tick's mask; every tick then composes the mask in one launch and runs the
        rollout with ``ops.ddim_sample(hold=...)``, the carried rows of ``carry`` included.  Without the flag every launch is the one
        of the session without any of this.  J <= 32.
        ``solver``: "ddim" (default: the session without this argument, launch for launch) or "multistep" - every tick's rollout runs the
        second-order multistep solver (``model.sample(solver="multistep")``) on the same ``num_inference_steps`` timesteps; meant for fewer
        steps per tick.  It composes with ``carry`` (the carried rows become the mask's leading rows: the seam stays bit-exact; J <= 32),
        ``holds``, ``draws``, ``robots=`` and ``use_graph``.  Not for a distilled decoder.
        ``limits = (lo, hi)`` ((J,) floats, one range r, or ``{joint: (lo, hi)}``) / ``reproject``: joint limits in radians AS PUBLISHED
        (after ``- pi``), as real numbers without modular arithmetic; -inf / +inf: no limit.  One launch converts them to normalised space
        on the device, each bound moved inward until the commit's expression gives a value inside the radians (``sd_session_limits``), and
        every tick's rollout clamps the predicted clean trajectory to them at every step (``ops.ddim_sample(limits=...)``): the published
        trajectory of every tick lies inside the given radians bit for bit, with no clamp in the commit and no extra launch per tick.
        ``set_limits`` rewrites the same device arrays, safe under ``use_graph``.  It composes with ``carry`` (the carried rows travel as
        mask bits, as under ``holds``: the seam stays exact, and they were published under the limits; J <= 32), ``holds`` (a held joint
        keeps its value whatever the limits say), ``draws``, ``robots=``, ``solver`` and ``use_graph``.  Without the argument every launch
        is the one of the session without any of this.
        ``slew`` ((J,) floats, one number, or ``{joint: v}``): slew limits in radians PER ROW as published - ``v = max velocity / row
        rate``, e.g. 8 rad/s at 50 Hz rows: 0.16; +inf: none.  One launch converts them to normalised space, ``v / std[j]`` moved inward by
        a margin that covers the rounding of the scan and of the commit (``sd_session_slew``), and every tick's rollout keeps consecutive
        rows of the predicted clean trajectory within them at every step (``ops.ddim_sample(slew=...)``): consecutive published rows of a
        tick differ by at most ``v``, evaluated exactly, and so does a tick's first row from the robot's last committed row (row
        ``advance - 1`` of its previous tick, kept on the device in normalised space; none after ``reset`` for the robots reset).  The
        margin assumes published values inside ``limits`` where both sides are given, else inside [-pi, pi].  ``set_slew`` rewrites the
        same device array, safe under ``use_graph``.  With ``carry`` row 0 is pinned: the scan starts from the carried rows (the seam
        stays exact) and no anchor is used.  A jump into a held joint's value is not limited.  It composes with ``limits``, ``holds``,
        ``draws``, ``robots=``, ``solver`` and ``use_graph``.  A ``v`` not above its margin raises.
        ``accel`` ((J,) floats, one number, or ``{joint: a}``): acceleration limits in radians PER ROW^2 as published - ``a = max
        acceleration / row rate^2``; +inf: none.  One launch converts them to normalised space, ``a / std[j]`` moved inward by a derived
        margin (``sd_session_accel``, ``ops.session_accel_margin``: the four roundings of the scan's row function and the commit's
        roundings at three published values), and every tick's rollout limits the second difference of consecutive rows of the predicted
        clean trajectory at every step (``ops.ddim_sample(accel=...)``), a tick's first two rows against the robot's last two committed
        rows (rows ``advance - 2`` and ``advance - 1`` of its previous tick, kept on the device; none after ``reset`` for the robots
        reset).  Every published triple then has a second difference of at most ``a``, evaluated exactly, unless the box or the slew
        limit won at its last row: there is NO braking ahead of the box.  It REQUIRES ``limits`` that are finite on both sides for every
        joint with a finite ``a`` (ValueError otherwise): without a bound the velocity can accumulate and the scan can run away from the
        prediction, and the margin is derived from that bound.  ``set_accel`` rewrites the same device array, safe under ``use_graph``.
        With ``carry`` no anchor is used, as for ``slew``: the pinned rows are the state, and ``carry >= 2`` is what gives continuity of
        acceleration across the seam.  It composes with ``limits``, ``slew``, ``holds``, ``draws``, ``select``, ``robots=``, ``solver``,
        ``use_graph`` and ``direct=True``.  An ``a`` not above its margin raises."""
        hp = dict(hyperparams if hyperparams is not None else (getattr(model, "hyperparams", None) or {}))
        self.distilled = bool(hp.get("distilled_decoder", False)) if distilled is None else bool(distilled)
        self.direct = self.check_direct(direct, self.distilled)                                                            # (needs no device)
        self.carry, self.advance = self.check_carry(model.trajectory_prediction_length, carry, advance, self.distilled)   # (likewise)
        self.draws, self.select = self.check_draws(draws, select, self.distilled, self.direct)                             # (likewise)
        self.coherence_decay, self.contrast = self.check_select(self.select, model.trajectory_prediction_length, self.advance, self.draws,
                                                                coherence_decay, contrast)                                # (likewise)
        self.holds = self.check_hold(holds, model.num_joints, self.distilled, self.direct)                                            # (likewise)
        self.solver = self.check_solver(solver, model.num_joints, self.carry, self.distilled)                              # (likewise)
        limits = self.check_limits(limits, model.num_joints, self.carry, self.distilled, self.direct)                                 # (likewise)
        self.reproject = self.check_reproject(reproject, self.distilled)
        slew = self.check_slew(slew, model.num_joints, self.carry, self.distilled, self.direct)                                       # (likewise)
        accel = self.check_accel(accel, model.num_joints, self.carry, self.distilled, self.direct, limits)                            # (likewise)
        params = [p for p in model.parameters()]
        if model.training:
            raise RuntimeError("PolicySession: the model is in train() mode; cached image tokens are exact in eval mode only - call model.eval()")
        if not params or not all(p.is_cuda for p in params):
            raise RuntimeError("PolicySession: the model is on the CPU; soccerdiffusion_amd has no CPU path - move it to the GPU (model.cuda())")
        if batch < 1 or num_inference_steps < 1:
            raise ValueError("batch and num_inference_steps must be positive")
        self.model, self.B, self.n_steps = model, int(batch), int(num_inference_steps)
        self.device = params[0].device
        self.hyperparams = hp
        self.T, self.J = model.trajectory_prediction_length, model.num_joints
        self._seed, self._watched = int(seed), None
        self.use_graph = bool(use_graph)
        if self.use_graph and self.distilled and not self.direct:
            raise ValueError("PolicySession: use_graph replays the rollout; a distilled decoder has none - " + _DIRECT_HINT)
        # a distilled session with any of the options runs the direct launch (model.sample_direct); with none, forward_with_context as ever
        self._direct = self.direct and (self.use_graph or self.draws > 1 or self.holds or limits is not None or slew is not None
                                        or accel is not None)
        encoders = {"joint_command_history": model.action_history_encoder, "rotation": model.imu_encoder,
                    "joint_state": model.joint_states_encoder}
        self._encoders = {k: e for k, e in encoders.items() if e is not None}
        self._shapes = {k: (e.max_seq_len, e.input_dim) for k, e in self._encoders.items()}
        self._images = model.image_sequence_encoder
        if self._images is not None:
            seq = getattr(self._images, "transformer_encoder", None)   # SequenceEncoderType.NONE: the image encoder itself
            self._image_encoder = self._images.image_encoder if seq is not None else self._images
            self._sequence = seq
            S = seq.max_seq_len if seq is not None else hp.get("image_context_length")
            R = hp.get("image_resolution")
            if S is None or R is None:
                raise ValueError("PolicySession: a model with images needs hyperparams with image_resolution (and image_context_length "
                                 "where it has no sequence encoder)")
            self.S, self.R = int(S), int(R)
        self._limits = None   # the normalised limits the rollout reads (two (32,) device arrays): they survive reset()
        if limits is not None:
            self._limits = ops.joint_limits({}, J=self.J, device=self.device)
            ops.session_limits(self._limits, *limits, model.mean, model.std, self.J)
        self._slew_v = self._anchor = None   # the normalised slew limits (32,) and the scan's anchors (B * draws, 32): device arrays
        self._accel_a = self._anchor2 = None   # the normalised acceleration limits (32,) and the rows before the anchors (B * draws, 32)
        self._limits_rad = limits
        # select="coherent": the last committed trajectory per robot (normalised space; NaN: none), and the last tick's (index, cost)
        self._plan = (torch.full((self.B, self.T, self.J), float("nan"), dtype=torch.float32, device=self.device)
                      if self.select == "coherent" and self.draws > 1 else None)
        self._selected = None
        if slew is not None:
            if self._limits is None:   # the slew call reads a box: an infinite one
                self._limits = ops.joint_limits({}, J=self.J, device=self.device)
            self._slew_v = ops.joint_slew({}, J=self.J, device=self.device)
            self._anchor = torch.full((self.B * self.draws, 32), float("nan"), dtype=torch.float32, device=self.device)
            self._mean_host = model.mean.detach().reshape(-1).cpu().numpy().astype(np.float32)
            self._std_host = model.std.detach().reshape(-1).cpu().numpy().astype(np.float32)
            self._write_slew(slew)
        if accel is not None:   # (limits are given: check_accel; the acceleration call reads the slew arrays: infinite ones without slew)
            if self._slew_v is None:
                self._slew_v = ops.joint_slew({}, J=self.J, device=self.device)
                self._anchor = torch.full((self.B * self.draws, 32), float("nan"), dtype=torch.float32, device=self.device)
                self._mean_host = model.mean.detach().reshape(-1).cpu().numpy().astype(np.float32)
                self._std_host = model.std.detach().reshape(-1).cpu().numpy().astype(np.float32)
                self._slew_rad = None
            self._accel_a = ops.joint_accel({}, J=self.J, device=self.device)
            self._anchor2 = torch.full((self.B * self.draws, 32), float("nan"), dtype=torch.float32, device=self.device)
            self._write_accel(accel)
        self.reset()

    @staticmethod
    def check_carry(T: int, carry: int = 0, advance: Optional[int] = None, distilled: bool = False) -> tuple:
        """(carry, advance) of a session with horizon T, validated (no device needed): advance defaults to T - carry; ValueError if
        carry < 0, advance < 1, advance + carry > T, or carry > 0 with a distilled decoder."""
        carry = int(carry)
        if carry < 0:
            raise ValueError(f"carry: the number of rows held across two ticks cannot be negative, got {carry}")
        advance = int(T) - carry if advance is None else int(advance)
        if advance < 1:
            raise ValueError(f"advance: a tick must commit at least one row (T = {T}, carry = {carry}), got {advance}")
        if advance + carry > T:
            raise ValueError(f"advance + carry = {advance} + {carry} exceeds the horizon T = {T}")
        if carry > 0 and distilled:
            raise ValueError("carry: a distilled decoder is one forward at t = 0 - there is no rollout whose rows could be pinned")
        return carry, advance

    @staticmethod
    def check_draws(draws: int = 1, select: str = "medoid", distilled: bool = False, direct: bool = False) -> tuple:
        """(draws, select) of a session, validated (no device needed): ValueError unless draws is an int in [1, 64] and select a known
        selector, or if draws > 1 with a distilled decoder without ``direct`` (with it, G start noises are G draws of the one-step map)."""
        if isinstance(draws, bool) or not isinstance(draws, int) or not 1 <= draws <= 64:
            raise ValueError(f"draws: the number of trajectories sampled per robot and tick is an int in [1, 64], got {draws!r}")
        if select not in SELECTORS:
            raise ValueError(f"select: one of {SELECTORS}, got {select!r}")
        if draws > 1 and distilled and not direct:
            raise ValueError("draws: a distilled decoder is one forward at t = 0 - " + _DIRECT_HINT)
        return draws, select

    @staticmethod
    def check_select(select: str = "medoid", T: int = 1, advance: Optional[int] = None, draws: int = 1, decay: float = 0.5,
                     contrast: float = 0.0) -> tuple:
        """(decay, contrast) of a session with horizon T that commits ``advance`` rows per tick, validated (no device needed): ValueError
        for an unknown selector, a ``decay`` outside (0, 1], a ``contrast`` < 0 (or NaN), or ``select="coherent"`` with advance == T -
        ticks that do not overlap have nothing to compare."""
        if select not in SELECTORS:
            raise ValueError(f"select: one of {SELECTORS}, got {select!r}")
        if isinstance(decay, bool) or not isinstance(decay, (int, float)) or not 0.0 < float(decay) <= 1.0:
            raise ValueError(f"coherence_decay: a number in (0, 1], got {decay!r}")
        if isinstance(contrast, bool) or not isinstance(contrast, (int, float)) or not float(contrast) >= 0.0 or math.isinf(float(contrast)):
            raise ValueError(f"contrast: a finite number >= 0, got {contrast!r}")
        advance = int(T) if advance is None else int(advance)
        if select == "coherent" and advance >= int(T):
            raise ValueError(f"select: 'coherent' compares a tick's draws with the rows of the previous plan they overlap - advance = {advance} "
                             f"of T = {T} rows leaves no overlap (give advance < T, with or without carry)")
        return float(decay), float(contrast)

    @staticmethod
    def check_hold(holds: bool = False, J: int = 1, distilled: bool = False, direct: bool = False) -> bool:
        """``holds`` of a session with J joints, validated (no device needed): ValueError if it is set with a distilled decoder without
        ``direct`` (with it, an element is held in the decoder's output, which is x0) or with more than 32 joints (one mask word per row)."""
        holds = bool(holds)
        if holds and distilled and not direct:
            raise ValueError("holds: a distilled decoder is one forward at t = 0 - " + _DIRECT_HINT)
        if holds and not 1 <= int(J) <= 32:
            raise ValueError(f"holds: one 32-bit mask word per row describes at most 32 joints, got J = {J}")
        return holds

    @staticmethod
    def check_solver(solver: str = "ddim", J: int = 1, carry: int = 0, distilled: bool = False) -> str:
        """``solver`` of a session, validated (no device needed): ValueError unless it is "ddim" or "multistep"; for "multistep" with a
        distilled decoder (no rollout), or with ``carry`` and J > 32 (the carried rows travel as a 32-bit mask word per row)."""
        if solver not in ("ddim", "multistep"):
            raise ValueError(f"solver: expected 'ddim' or 'multistep', got {solver!r}")
        if solver == "multistep" and distilled:
            raise ValueError("solver: a distilled decoder is one forward at t = 0 - there is no rollout for a multistep solver")
        if solver == "multistep" and carry > 0 and not 1 <= int(J) <= 32:
            raise ValueError(f"solver: with carry the multistep rollout pins rows through a 32-bit mask word per row, got J = {J}")
        return solver

    @staticmethod
    def check_limits(limits=None, J: int = 1, carry: int = 0, distilled: bool = False, direct: bool = False):
        """``limits`` of a session with J joints, validated (no device needed): None, or the two (32,) fp32 host arrays in radians, padded
        with -inf / +inf (``(lo, hi)`` of (J,) floats, one range r, or ``{joint: (lo, hi)}``, as ``ops.joint_limits`` takes them).
        ValueError for a wrong shape, a NaN or lo > hi, with a distilled decoder without ``direct`` (with it, the decoder's output is the
        x0 that is limited), or with ``carry`` and J > 32 (the carried rows travel as a 32-bit mask word per row)."""
        if limits is None:
            return None
        if distilled and not direct:
            raise ValueError("limits: a distilled decoder is one forward at t = 0 - " + _DIRECT_HINT)
        if carry > 0 and not 1 <= int(J) <= 32:
            raise ValueError(f"limits: with carry the limited rollout pins rows through a 32-bit mask word per row, got J = {J}")
        return ops._limits_host(limits, J)

    @staticmethod
    def check_direct(direct: bool = False, distilled: bool = False) -> bool:
        """``direct`` of a session, validated (no device needed): ValueError if it is set without a distilled decoder - a model that
        predicts noise has a rollout, and its output is not x0."""
        if direct and not distilled:
            raise ValueError("direct: the projection of a one-step output is a distilled decoder's route - this model predicts noise and has a rollout")
        return bool(direct)

    @staticmethod
    def check_reproject(reproject: bool = False, distilled: bool = False) -> bool:
        """``reproject`` of a session, validated (no device needed): ValueError if it is set with a distilled decoder - its output is x0,
        there is no eps that could be recomputed from a clamped one."""
        if reproject and distilled:
            raise ValueError("reproject: a distilled decoder predicts x0 itself - there is no eps to recompute from the clamped x0")
        return bool(reproject)

    def set_limits(self, lo, hi=None) -> None:
        """New joint limits in radians as published (``lo``, ``hi`` as the constructor's ``limits=(lo, hi)``; ``set_limits(r)`` or
        ``set_limits({joint: (lo, hi)})`` as there): ONE small launch rewrites the session's device arrays in place, so a captured tick
        stays captured and the next tick runs under the new limits."""
        if self._limits is None:
            raise RuntimeError("PolicySession.set_limits: the session was built without limits")
        host = self.check_limits(lo if hi is None else (lo, hi), self.J, self.carry, self.distilled, self.direct)
        if self._accel_a is not None:   # (before anything is written: the new box must still bound every joint with a finite a)
            self._accel_box(self._accel_rad, self.J, host)
        ops.session_limits(self._limits, *host, self.model.mean, self.model.std, self.J)
        self._limits_rad = host
        if self._slew_v is not None and self._slew_rad is not None:   # the slew margin depends on the bound the limits give: one more launch
            self._write_slew(self._slew_rad)
        if self._accel_a is not None:   # likewise
            self._write_accel(self._accel_rad)

    @staticmethod
    def check_slew(slew=None, J: int = 1, carry: int = 0, distilled: bool = False, direct: bool = False):
        """``slew`` of a session with J joints, validated (no device needed): None, or the (32,) fp32 host array in radians per row,
        padded with +inf ((J,) floats, one number, or ``{joint: v}``, as ``ops.joint_slew`` takes them).  ValueError for a wrong shape, a
        NaN or a negative value, J > 32, or with a distilled decoder without ``direct`` (with it, the scan runs on the decoder's output)."""
        if slew is None:
            return None
        if distilled and not direct:
            raise ValueError("slew: a distilled decoder is one forward at t = 0 - " + _DIRECT_HINT)
        return ops._slew_host(slew, J)

    def _write_slew(self, v_rad) -> None:
        """ONE launch: the session's (32,) device array from ``v_rad`` (``check_slew``'s array) under the current ``limits``."""
        J = self.J
        bound = np.full(J, math.pi, dtype=np.float32)   # |published| <= pi unless limits on both sides say otherwise
        if self._limits_rad is not None:
            lo, hi = (np.abs(a[:J]) for a in self._limits_rad)
            both = np.isfinite(lo) & np.isfinite(hi)
            one = np.where(np.isfinite(lo), lo, np.where(np.isfinite(hi), hi, 0.0))
            bound = np.where(both, np.maximum(lo, hi), np.maximum(bound, one)).astype(np.float32)
        margin = ops.session_slew_margin(bound, self._mean_host[:J], self._std_host[:J])
        small = np.isfinite(v_rad[:J]) & ~(v_rad[:J].astype(np.float64) > margin)
        if small.any():
            j = int(np.argmax(small))
            raise ValueError(f"slew: v[{j}] = {v_rad[j]} rad per row is not above the margin {margin[j]:.3e} of the fp32 arithmetic")
        ops.session_slew(self._slew_v, v_rad, bound, self.model.mean, self.model.std, J)
        self._slew_rad = v_rad

    def set_slew(self, slew) -> None:
        """New slew limits in radians per row as published (as the constructor's ``slew``): ONE small launch rewrites the session's device
        array in place, so a captured tick stays captured and the next tick runs under the new limits."""
        if self._slew_v is None:
            raise RuntimeError("PolicySession.set_slew: the session was built without slew")
        self._write_slew(self.check_slew(slew, self.J, self.carry, self.distilled, self.direct))

    @staticmethod
    def check_accel(accel=None, J: int = 1, carry: int = 0, distilled: bool = False, direct: bool = False, limits=None):
        """``accel`` of a session with J joints, validated (no device needed): None, or the (32,) fp32 host array in radians per row^2,
        padded with +inf ((J,) floats, one number, or ``{joint: a}``, as ``ops.joint_accel`` takes them).  ``limits``: the session's, as
        ``check_limits`` returns them.  ValueError for a wrong shape, a NaN or a negative value, J > 32, with a distilled decoder without
        ``direct``, or for a joint with a finite ``a`` whose limits are not finite on both sides - without a bound the scan can run away
        from the prediction, and the margin of the conversion is derived from that bound."""
        if accel is None:
            return None
        if distilled and not direct:
            raise ValueError("accel: a distilled decoder is one forward at t = 0 - " + _DIRECT_HINT)
        return PolicySession._accel_box(ops._accel_host(accel, J), J, limits)

    @staticmethod
    def _accel_box(a, J: int, limits):
        """``a`` (``check_accel``'s array) if ``limits`` (``check_limits``' arrays, or None) are finite on both sides for every joint with
        a finite ``a[j]``; ValueError otherwise."""
        lo, hi = (np.full(32, -np.inf), np.full(32, np.inf)) if limits is None else limits
        open_ = np.isfinite(a[:J]) & ~(np.isfinite(lo[:J]) & np.isfinite(hi[:J]))
        if open_.any():
            j = int(np.argmax(open_))
            raise ValueError(f"accel: joint {j} has a finite acceleration limit but no finite box - give limits that are finite on both sides "
                             f"for every such joint (without a bound the scan can run away from the prediction)")
        return a

    def _write_accel(self, a_rad) -> None:
        """ONE launch: the session's (32,) device array from ``a_rad`` (``check_accel``'s array) under the current ``limits``."""
        J = self.J
        lo, hi = (np.abs(b[:J]) for b in self._limits_rad)
        bound = np.where(np.isfinite(a_rad[:J]), np.maximum(lo, hi), math.pi).astype(np.float32)   # (an unlimited joint's bound is not read)
        bound = np.where(np.isfinite(bound), bound, math.pi).astype(np.float32)
        margin = ops.session_accel_margin(bound, self._mean_host[:J], self._std_host[:J])
        small = np.isfinite(a_rad[:J]) & ~(a_rad[:J].astype(np.float64) > margin)
        if small.any():
            j = int(np.argmax(small))
            raise ValueError(f"accel: a[{j}] = {a_rad[j]} rad per row^2 is not above the margin {margin[j]:.3e} of the fp32 arithmetic")
        ops.session_accel(self._accel_a, a_rad, bound, self.model.mean, self.model.std, J)
        self._accel_rad = a_rad

    def set_accel(self, accel) -> None:
        """New acceleration limits in radians per row^2 as published (as the constructor's ``accel``): ONE small launch rewrites the
        session's device array in place, so a captured tick stays captured and the next tick runs under the new limits."""
        if self._accel_a is None:
            raise RuntimeError("PolicySession.set_accel: the session was built without accel")
        self._write_accel(self.check_accel(accel, self.J, self.carry, self.distilled, self.direct, self._limits_rad))

    def _lim(self, dev_idx=None) -> dict:
        """The limit arguments of the tick's rollout (of the robots ``dev_idx``): none in a session without limits or slew."""
        if self._limits is None:
            return {}
        out = {"limits": self._limits, "reproject": self.reproject}
        if self._slew_v is not None:
            start = None   # with carry row 0 is pinned: the scan starts from the carried rows
            if self.carry == 0:
                G = self.draws
                start = self._anchor if dev_idx is None else self._anchor.view(self.B, G * 32)[dev_idx.long()].reshape(-1, 32).contiguous()
            out["slew"] = (self._slew_v, start)
            if self._accel_a is not None:
                start2 = None   # (with carry the pinned rows are the state)
                if self.carry == 0:
                    G = self.draws
                    start2 = self._anchor2 if dev_idx is None else self._anchor2.view(self.B, G * 32)[dev_idx.long()].reshape(-1, 32).contiguous()
                out["accel"] = (self._accel_a, start2)
        return out

    def _direct_lim(self, dev_idx=None) -> dict:
        """``_lim`` for the direct launch of a distilled decoder: the same device arrays and anchors, without ``reproject``."""
        out = self._lim(dev_idx)
        out.pop("reproject", None)
        return out

    def _direct_cond(self, dev_idx=None) -> dict:
        """The conditioning of a distilled tick: ``hold=`` in a session with ``holds`` (the mask's compose launch), else nothing."""
        return {"hold": self._hold(dev_idx)} if self.holds else {}

    @property
    def _carrying(self) -> bool:
        """The commit is the carrying one: anything but carry = 0 with the whole trajectory pushed."""
        return self.carry > 0 or self.advance != self.T

    def _pin(self, dev_idx=None):
        """``pin`` of the tick's rollout: the session's pin buffers (of the robots ``dev_idx``), or None for a session without carry."""
        if self.carry == 0:
            return None
        if dev_idx is None:
            known, rows = self._pin_x0, self._pin_rows
        else:
            i = dev_idx.long()
            known, rows = self._pin_x0[i], self._pin_rows[i]
        if self.draws > 1:   # every draw of a robot is pinned to the robot's carried rows: all draws share the seam
            S, G = rows.shape[0], self.draws
            known = known.unsqueeze(1).expand(S, G, self.T, self.J).reshape(S * G, self.T, self.J).contiguous()
            rows = rows.unsqueeze(1).expand(S, G).reshape(S * G).contiguous()
        return known, rows

    def _hold(self, dev_idx=None):
        """``hold`` of the tick's rollout in a session with ``holds``: ONE launch composes the mask - the robots' held joints in every row,
        all joints in the carried rows - into the session's mask buffer (of the robots ``dev_idx``: its leading rows), and the known values
        are the session's pin buffer: the carried rows and the held joints' values live side by side in it."""
        G = self.draws
        if dev_idx is None:
            known, mask = self._pin_x0, self._mask
        else:
            known, mask = self._pin_x0[dev_idx.long()], self._mask[:dev_idx.numel() * G]
        ops.session_hold_mask(mask, self._held, self._pin_rows if self.carry > 0 else None, self.J, G, robots=dev_idx)
        if G > 1:   # every draw of a robot holds the robot's values
            S = known.shape[0]
            known = known.unsqueeze(1).expand(S, G, self.T, self.J).reshape(S * G, self.T, self.J).contiguous()
        return known, mask

    def _cond(self, dev_idx=None) -> dict:
        """The conditioning arguments of the tick's rollout: ``hold=`` in a session with ``holds``, else the parent's ``pin=``."""
        return {"hold": self._hold(dev_idx)} if self.holds else {"pin": self._pin(dev_idx)}

    def hold(self, joints, values, robots=None) -> None:
        """Holds the joints ``joints`` (indices) at ``values`` - radians as ``step`` publishes them; (n,), (S, n) or (S, T, n): the same
        for every robot and row, per robot, or per robot and row of the horizon - for all robots or for ``robots`` (an index list).  One
        launch normalises the values with the model's mean and std on the device, writes them into the session's known-value buffer
        and sets the joints' bits in the robots' held words; from the next tick on the rollout holds these elements at every step and
        returns them exactly.  A hold stays until ``release`` - through ``reset()`` too: a switched-off motor stays off.  With ``carry``
        the values are constant over the horizon ((n,) or (S, n)): the carried rows share the buffer, and a joint that is newly held
        between two ticks takes its new value in the carried rows as well (the seam stays exact on every other element)."""
        if not self.holds:
            raise RuntimeError("PolicySession.hold: the session was built without holds=True")
        idx = ops.hold_joints(joints, self.J)
        S, dev_idx = (self.B, None) if robots is None else self._subset(robots)[::2]
        v = torch.as_tensor(values, dtype=torch.float32)
        n = len(idx)
        if tuple(v.shape) not in ((n,), (S, n), (S, self.T, n)):
            raise ValueError(f"values: expected ({n},), ({S}, {n}) or ({S}, {self.T}, {n}) radians, got {tuple(v.shape)}")
        if v.dim() == 3 and self.carry > 0:
            raise ValueError("hold: with carry the held values are constant over the horizon - the carried rows overwrite the leading rows "
                             "of the same buffer; pass (n,) or (S, n) values")
        m = self.model
        ops.session_hold(self._pin_x0, self._held, idx, v.to(self.device).contiguous(), m.mean, m.std, robots=dev_idx)

    def release(self, joints=None, robots=None) -> None:
        """Ends the hold of ``joints`` (None: all joints) for all robots or for ``robots``: one launch clears the bits."""
        if not self.holds:
            raise RuntimeError("PolicySession.release: the session was built without holds=True")
        idx = list(range(self.J)) if joints is None else ops.hold_joints(joints, self.J)
        dev_idx = None if robots is None else self._subset(robots)[2]
        ops.session_hold(self._pin_x0, self._held, idx, None, None, None, robots=dev_idx)

    # ---- the plan: shapes from hyperparameters alone ---------------------------------------
    @staticmethod
    def plan(hyperparams: dict) -> dict:
        """Ring shapes (rows, columns) per robot and the decoder's memory rows for a hyperparameter dictionary (a shipped YAML):
        context tokens per modality = context length // encoder_patch_size, one per image, one for the game state; + the step token."""
        hp, p = hyperparams, hyperparams["encoder_patch_size"]
        J = hp["num_joints"]
        rings, tokens = {}, 0
        if hp["use_action_history"]:
            rings["joint_command_history"] = (hp["action_context_length"], J)
        if hp["use_imu"]:
            rings["rotation"] = (hp["imu_context_length"], 5 if hp["imu_orientation_embedding_method"] == "five_dim" else 4)
        if hp["use_joint_states"]:
            rings["joint_state"] = (hp["joint_state_context_length"], J)
        tokens = sum(L // p for L, _ in rings.values())
        if hp["use_images"]:
            rings["image_tokens"] = (hp["image_context_length"], hp["hidden_dim"])
            tokens += hp["image_context_length"]
        if hp["use_gamestate"]:
            tokens += 1
        return {"rings": rings, "context_rows": tokens, "memory_rows": tokens + 1, "trajectory": (hp["trajectory_prediction_length"], J)}

    # ---- state -----------------------------------------------------------------------------
    def _weights_key(self):
        """derived.version_key of every parameter and persistent buffer (BatchNorm statistics, mean, std)."""
        if self._watched is None:   # (rebuilt by reset())
            self._watched = list(self.model.parameters()) + [b for mod in self.model.modules() for n, b in mod._buffers.items()
                                                             if b is not None and n not in mod._non_persistent_buffers_set]
        return version_key(*self._watched)

    def _check_weights(self, what: str) -> None:
        if not current(self._key, self._weights_key()):
            raise RuntimeError(f"PolicySession.{what}: the model's weights changed since the session was built; its cached image tokens "
                               "belong to the old weights - call reset()")

    def _subset(self, robots) -> tuple:
        """(S, the indices on the host, the indices on the device) of ``ops.robot_index``: validated once per call."""
        idx = ops.robot_index(robots, self.B)
        return idx.numel(), idx, idx.to(self.device)

    def _reset_some(self, robots) -> None:
        if self.model.training:
            raise RuntimeError("PolicySession.reset: the model is in train() mode - call model.eval()")
        self._check_weights("reset")   # a part of the batch cannot adopt new weights: the other robots' tokens belong to the old ones
        if isinstance(robots, torch.Tensor) and robots.dtype == torch.bool:
            if tuple(robots.shape) != (self.B,) or (robots.is_cuda and robots.device != self.device):
                raise ValueError(f"reset: a mask is ({self.B},) bool on the CPU or on {self.device}, got {tuple(robots.shape)} on {robots.device}")
            mask = robots.to(self.device).contiguous()   # (a device mask stays where it is: nothing is read back)
        else:
            mask = torch.zeros(self.B, dtype=torch.bool)
            mask[ops.robot_index(robots, self.B).long()] = True
            mask = mask.to(self.device)
        ops.session_reset(self._resettable, mask, self._game_state, DEFAULT_GAME_STATE, pin_rows=self._pin_rows if self._carrying else None)
        if self._anchor is not None:   # no last command: the robots' next first row is free
            self._anchor.view(self.B, -1).masked_fill_(mask.view(self.B, 1), float("nan"))
        if self._anchor2 is not None:   # ... and its next two rows are free of the acceleration limit
            self._anchor2.view(self.B, -1).masked_fill_(mask.view(self.B, 1), float("nan"))
        if self._plan is not None:     # no plan: the robots' next tick commits the medoid of its draws
            self._plan.masked_fill_(mask.view(self.B, 1, 1), float("nan"))

    def reset(self, robots=None) -> None:
        """Rings back to ``context_length`` rows of zeros (ros.py:87-106), the image ring to the token of an all-zero frame
        (ros.py:88-92), the game state to 2, the noise generator to the seed; the current weights become the session's.
        ``robots`` (an index list as ``ops.robot_index`` takes it, or a (B,) bool mask on the CPU or on the session's device, which is
        used without a synchronisation): the end of those robots' episodes only.  Their rings, head words and game state go back to the
        start state in one launch, the image-token ring to the zero-frame token of the last whole reset (the backbone does not run).
        Nothing is allocated, a captured tick stays valid, the noise generator and the session's weights stay; weights that moved since
        the last whole reset raise as in ``step``.  With ``carry`` the robots' carried-row counts are zeroed in the same launch: their
        next tick is unpinned, a first tick."""
        if robots is not None:
            return self._reset_some(robots)
        if self.model.training:
            raise RuntimeError("PolicySession.reset: the model is in train() mode - call model.eval()")
        dev, B = self.device, self.B
        new = lambda L, C: (torch.zeros(B, L, C, dtype=torch.float32, device=dev), torch.zeros(B, dtype=torch.int32, device=dev))
        self._rings = {k: new(L, C) for k, (L, C) in self._shapes.items()}
        self._wins = {k: torch.empty_like(r) for k, (r, _) in self._rings.items()}
        # the commit always has a ring to push into: without an action-history encoder a private one of T rows that nothing reads
        self._action = self._rings.get("joint_command_history") or new(self.T, self.J)
        self._launch = (ops.SessionWindows([(*self._rings[k], self._wins[k], WRAPPED[k]) for k in KEYS if k in self._rings])
                        if self._rings else None)
        self._game_state = torch.full((B,), DEFAULT_GAME_STATE, dtype=torch.int64, device=dev)
        self._gen = torch.Generator(device=dev).manual_seed(self._seed)
        self._t0 = torch.zeros(B, dtype=torch.int64, device=dev)
        if self._anchor is not None:   # (in place: the array is the session's for its lifetime)
            self._anchor.fill_(float("nan"))
        if self._anchor2 is not None:
            self._anchor2.fill_(float("nan"))
        if self._plan is not None:
            self._plan.fill_(float("nan"))
        self._selected = None
        if self._carrying:   # the rows carried into the next tick (normalised space) and how many per robot: 0 until a tick has committed
            self._pin_rows = torch.zeros(B, dtype=torch.int32, device=dev)
        if self.holds and getattr(self, "_held", None) is not None:
            pass   # a hold survives reset(): the held words and the known values stay; the carried-row counts above are new
        elif self._carrying or self.holds:
            self._pin_x0 = torch.zeros(B, self.T, self.J, dtype=torch.float32, device=dev)
            if self.holds:   # the held joints of every robot, and the tick's mask (one word per (trajectory, row))
                self._held = torch.zeros(B, dtype=torch.int32, device=dev)
                self._mask = torch.zeros(B * self.draws, self.T, dtype=torch.int32, device=dev)
        self._watched, self._graph = None, None
        self._key = self._weights_key()
        self._resettable = [(*r, None) for r in {id(r[0]): r for r in (*self._rings.values(), self._action)}.values()]
        if self._images is not None:
            d = self.model.hidden_dim
            self._tokens = new(self.S, d)
            self._token_win = torch.empty_like(self._tokens[0])
            with torch.no_grad():
                zero = self._image_encoder(torch.zeros(1, 1, 3, self.R, self.R, dtype=torch.float32, device=dev))   # (1, 1, d)
            ops.ring_push(*self._tokens, zero.expand(B, self.S, d).contiguous())
            self._resettable.append((*self._tokens, zero.reshape(d).clone()))   # kept: a partial reset writes this token again

    # ---- pushes ----------------------------------------------------------------------------
    def _rows(self, x: torch.Tensor, tail: tuple, name: str, S: Optional[int] = None) -> torch.Tensor:
        """(B, *tail) or (B, n, *tail) -> a contiguous fp32 device tensor (B, n, *tail); the caller's tensor is only read.  ``S``: the
        leading dimension where the call names a subset of the robots."""
        S = self.B if S is None else S
        if not isinstance(x, torch.Tensor):
            x = torch.as_tensor(x)
        if x.dim() == len(tail) + 1:
            x = x.unsqueeze(1)
        if x.dim() != len(tail) + 2 or x.shape[0] != S or tuple(x.shape[2:]) != tail:
            raise ValueError(f"{name}: expected ({S}, {', '.join(map(str, tail))}) or ({S}, n, {', '.join(map(str, tail))}), "
                             f"got {tuple(x.shape)}")
        return x.to(device=self.device, dtype=torch.float32).contiguous()

    def _push(self, key: str, x: torch.Tensor, name: str, robots) -> None:
        if key not in self._rings:
            raise RuntimeError(f"PolicySession.{name}: the model has this modality switched off - there is no ring to push into")
        if robots is None:
            return ops.ring_push(*self._rings[key], self._rows(x, (self._shapes[key][1],), name))
        S, _, dev_idx = self._subset(robots)
        ops.ring_push(*self._rings[key], self._rows(x, (self._shapes[key][1],), name, S), robots=dev_idx)

    def push_joint_state(self, q: torch.Tensor, robots=None) -> None:
        """Raw joint angles (B, J) or (B, n, J), oldest first, as ros.py:205-214 stores them (the wrap happens in ``step``).
        ``robots``: the leading dimension is ``len(robots)`` and only those robots' rings move."""
        self._push("joint_state", q, "push_joint_state", robots)

    def push_rotation(self, r: torch.Tensor, robots=None) -> None:
        """Orientation rows (B, 4 | 5) or (B, n, 4 | 5) (quaternion or the five-dimensional form: ros.py:216-253); ``robots`` as in
        ``push_joint_state``."""
        self._push("rotation", r, "push_rotation", robots)

    def push_orientation(self, q: torch.Tensor, robots=None) -> None:
        """Orientation samples as the IMU delivers them: xyzw quaternions (B, 4) or (B, n, 4), oldest first (ros.py:216-253).  The
        rotation ring's own width decides what is stored: the quaternions as they are, or, for ``imu_orientation_embedding_method:
        five_dim``, ``dataset.quats_to_5d``'s rows, computed on the device (``ops.ring_push_quat``); ``robots`` as in ``push_joint_state``."""
        if "rotation" not in self._rings:
            raise RuntimeError("PolicySession.push_orientation: the model has this modality switched off - there is no ring to push into")
        S, dev_idx = (None, None) if robots is None else self._subset(robots)[::2]
        ops.ring_push_quat(*self._rings["rotation"], self._rows(q, (4,), "push_orientation", S), robots=dev_idx)

    def _image_gate(self, name: str) -> None:
        if self._images is None:
            raise RuntimeError(f"PolicySession.{name}: the model has images switched off - there is no ring to push into")
        self._check_weights(name)
        if self.model.training:
            raise RuntimeError(f"PolicySession.{name}: the model is in train() mode - call model.eval()")

    def _push_frames(self, x: torch.Tensor, dev_idx) -> None:
        """Preprocessed fp32 frames (S, n, 3, R, R) on the device -> their tokens into the token rings of the batch or of ``dev_idx``."""
        if x.shape[0] == 0:
            return
        with torch.no_grad():
            tokens = self._image_encoder(x)
        ops.ring_push(*self._tokens, tokens.contiguous(), robots=dev_idx)

    def push_image(self, frames: torch.Tensor, robots=None) -> None:
        """Frames (B, 3, R, R) or (B, n, 3, R, R), preprocessed as ros.py:191-200 and already at ``image_resolution``: encoded now by
        the model's image encoder, on these frames only; the tokens go into the ring and no frame is kept.  ``robots``: the leading
        dimension is ``len(robots)``, the encoder sees ``len(robots) * n`` frames and only those robots' token rings move."""
        self._image_gate("push_image")
        S, dev_idx = (None, None) if robots is None else self._subset(robots)[::2]
        self._push_frames(self._rows(frames, (3, self.R, self.R), "push_image", S), dev_idx)

    def push_camera(self, frames: torch.Tensor, robots=None, interpolation: str = "linear", order: str = "rgb") -> None:
        """Raw camera frames, uint8 (B, H, W, 3) or (B, n, H, W, 3) of any size: preprocessed on the device, then handled as
        ``push_image`` handles its frames.  A CPU tensor is uploaded as uint8 (``non_blocking``), a device tensor is read in place.
        ``interpolation``: "linear" is the robot node's preprocessing (ros.py:186-200: cv2.resize's default INTER_LINEAR, [0, 1] scaling,
        ImageNet mean / std: ``ops.camera_intake``); "area" is the training set's (dataset/pytorch.py:209-211: INTER_AREA of 480 x 480
        frames: ``ops.frames_area``).  ``order``: "rgb", or "bgr" where the channels arrive in OpenCV's order; ``robots`` as in
        ``push_image``."""
        self._image_gate("push_camera")
        S, dev_idx = (None, None) if robots is None else self._subset(robots)[::2]
        S = self.B if S is None else S
        if not isinstance(frames, torch.Tensor) or frames.dtype != torch.uint8:
            raise ValueError(f"push_camera: expected a uint8 tensor, got {getattr(frames, 'dtype', type(frames))}")
        if frames.dim() == 4:
            frames = frames.unsqueeze(1)
        if frames.dim() != 5 or frames.shape[0] != S or frames.shape[-1] != 3:
            raise ValueError(f"push_camera: expected ({S}, H, W, 3) or ({S}, n, H, W, 3), got {tuple(frames.shape)}")
        if interpolation not in ("linear", "area"):
            raise ValueError(f"interpolation: 'linear' or 'area', got {interpolation!r}")
        if order not in ("rgb", "bgr"):
            raise ValueError(f"order: 'rgb' or 'bgr', got {order!r}")
        if interpolation == "area" and tuple(frames.shape[2:4]) != (ops.FRAME_SIZE, ops.FRAME_SIZE):
            raise ValueError(f"push_camera: interpolation='area' is the preprocessing of the recordings' {ops.FRAME_SIZE} x {ops.FRAME_SIZE} "
                             f"frames, got {frames.shape[2]} x {frames.shape[3]}")
        frames = frames.to(self.device, non_blocking=True).contiguous()
        if interpolation == "linear":
            x = ops.camera_intake(frames, self.R, order=order)
        else:
            if order == "bgr":
                frames = frames.flip(-1)
            index = torch.arange(S * frames.shape[1], device=self.device).view(S, frames.shape[1])
            x = ops.frames_area(frames.view(-1, ops.FRAME_SIZE, ops.FRAME_SIZE, 3), index, self.R)
        self._push_frames(x, dev_idx)

    def set_game_state(self, idx, robots=None) -> None:
        """Game state index per robot (an int for all of them, or B of them); ros.py:274 feeds the constant 2.  ``robots``: for those
        robots only (an int for all of them, or ``len(robots)`` of them)."""
        if robots is not None:
            S, _, dev_idx = self._subset(robots)
            value = idx if isinstance(idx, int) else torch.as_tensor(idx).reshape(S).to(self.device)
            self._game_state[dev_idx.long()] = value
        elif isinstance(idx, int):
            self._game_state.fill_(idx)
        else:
            self._game_state.copy_(torch.as_tensor(idx).reshape(self.B))

    # ---- the tick --------------------------------------------------------------------------
    def _context(self, subset: Optional[tuple] = None) -> list:
        """The context tokens of the batch, or of a ``_subset``: its compact windows are the leading S row blocks of the window buffers."""
        m = self.model
        S, _, dev_idx = subset if subset is not None else (self.B, None, None)
        if self._launch is not None:
            self._launch.launch(dev_idx)
        ctx = [self._encoders[k](self._wins[k][:S]) for k in KEYS if k in self._encoders]
        if self._images is not None:
            win = ops.ring_window(*self._tokens, out=self._token_win[:S], robots=dev_idx)
            ctx.append(self._sequence(win) if self._sequence is not None else win)
        if m.game_state_encoder is not None:
            ctx.append(m.game_state_encoder(self._game_state if dev_idx is None else self._game_state[dev_idx.long()]))
        return ctx

    def windows(self, robots=None) -> dict:
        """Copies of the contiguous windows the next ``step`` would encode, keyed as ``encode_input_data``'s input (``image_tokens``:
        the per-frame tokens, what the image sequence encoder reads).  ``robots``: the compact windows (S, ...) of those robots."""
        S, _, dev_idx = (self.B, None, None) if robots is None else self._subset(robots)
        if self._launch is not None:
            self._launch.launch(dev_idx)
        out = {k: w[:S].clone() for k, w in self._wins.items()}
        if self._images is not None:
            out["image_tokens"] = ops.ring_window(*self._tokens, robots=dev_idx)
        if self.model.game_state_encoder is not None:
            out["game_state"] = self._game_state.clone() if dev_idx is None else self._game_state[dev_idx.long()]
        return out

    def step(self, x_T: Optional[torch.Tensor] = None, robots=None, return_draws: bool = False):
        """One tick (ros.py:259-335): the published trajectory (B, T, J) = denormalised sample - pi, also appended to the action
        history (its first ``advance`` rows in a session with overlapping ticks, whose first ``carry`` rows equal rows
        [advance, advance + carry) of the robot's previous tick).  ``x_T``: the start noise (B, T, J) (only read); default: drawn from the session's device generator.
        ``robots``: the tick of those S robots alone - their windows, the context encoders and the rollout at batch S, the commit into
        their action rings only; x_T and the result are (S, T, J).  A subset tick runs eagerly, on the same rings, also where
        ``use_graph`` is set: the captured graph serves the whole batch.
        A session with ``draws`` = G > 1 samples G trajectories per robot - ``x_T`` is (B * G, T, J), robot b's draws contiguous - and
        commits and returns the selected one; ``return_draws=True`` returns ``(trajectory, draws (B, G, T, J), index (B,) int32)``, the
        draws denormalised like the trajectory (``trajectory[b]`` is ``draws[b, index[b]]`` bit for bit).  With draws = 1 the draws
        are the trajectory itself and the index is 0."""
        m = self.model
        self._check_weights("step")
        if m.training:
            raise RuntimeError("PolicySession.step: the model is in train() mode - call model.eval()")
        subset = None if robots is None else self._subset(robots)
        G = self.draws
        S = self.B if subset is None else subset[0]
        shape = (S * G, self.T, self.J)
        if x_T is None:
            x_T = torch.randn(shape, dtype=torch.float32, device=self.device, generator=self._gen)
        elif tuple(x_T.shape) != shape or not x_T.is_cuda or x_T.dtype != torch.float32:
            raise ValueError(f"x_T: expected an fp32 tensor {shape} on {self.device}, got {tuple(x_T.shape)} {x_T.dtype} on {x_T.device}")
        if S == 0:
            empty = torch.empty((0, self.T, self.J), dtype=torch.float32, device=self.device)
            if not return_draws:
                return empty
            return empty, empty.view(0, G, self.T, self.J), torch.empty(0, dtype=torch.int32, device=self.device)
        with torch.no_grad():
            dev_idx = None if subset is None else subset[2]
            if self.use_graph and subset is None:
                if self._graph is None:   # first tick after construction / reset(): the rings are new
                    self._graph = _GraphedTick(self, x_T)
                x = self._graph(x_T)
            else:
                cond = self._direct_cond(dev_idx) if self.distilled else self._cond(dev_idx)   # (holds: the mask's compose launch opens the tick)
                ctx = self._context(subset)
                if self.distilled and not self._direct:   # one forward at t = 0 (ros.py:293-298)
                    x = m.forward_with_context(ctx, x_T.contiguous(), self._t0[:S])
                elif self.distilled:   # the same forward and the projection of its output - hold, slew, limits - in one launch
                    every = m.sample_direct(ctx, x_T, draws=G, max_mode=3, **cond, **self._direct_lim(dev_idx)).contiguous()
                    if G == 1:
                        x = every
                    else:
                        index, chosen, cost = self._select(every, dev_idx)
                        x = (chosen, every, index, cost)
                elif G == 1:
                    x = m.sample(ctx, x_T, self.n_steps, max_mode=3, **cond, solver=self.solver, **self._lim(dev_idx))
                else:   # the context was encoded once per robot; its G draws share the folded planes
                    every = m.sample(ctx, x_T, self.n_steps, max_mode=3, **cond, draws=G, solver=self.solver, **self._lim(dev_idx)).contiguous()
                    index, chosen, cost = self._select(every, dev_idx)
                    x = (chosen, every, index, cost)
            if G == 1:
                out = self._commit(x.contiguous(), dev_idx)
                if not return_draws:
                    return out
                return out, out.unsqueeze(1), torch.zeros(S, dtype=torch.int32, device=self.device)
            chosen, every, index, cost = x
            out = self._commit(chosen, dev_idx)
            if self._plan is not None:
                # beside the commit and outside a captured tick, like the anchor: a replay whose range guard trips is repeated eagerly and
                # must still see the OLD plan.  Only the ticked robots' plans move.
                if dev_idx is None:
                    self._plan.copy_(chosen)
                else:
                    self._plan.index_copy_(0, dev_idx.long(), chosen)
                self._selected = (index, cost)
            if not return_draws:
                return out
            # the commit's expression, one rounding per operation (sd_session.hip: contraction off): (x * std + mean) - pi
            every = (every.view(S, G, self.T, self.J) * m.std + m.mean) - math.pi
            return out, every, index.clone()

    def _select(self, every: torch.Tensor, dev_idx=None) -> tuple:
        """(index (S,), chosen (S, T, J), cost (S, G) or None) of a tick's draws ``every`` (S * G, T, J): the session's selection launch."""
        if self._plan is None:
            return (*ops.select_medoid(every, self.draws), None)
        return ops.select_coherent(every, self.draws, self._plan, self.advance, decay=self.coherence_decay, contrast=self.contrast,
                                   robots=dev_idx, cost=True)

    def selection(self) -> dict:
        """The last tick's selection in a ``select="coherent"`` session: clones of ``{"index": (S,) int32, "cost": (S, G) fp32}`` - the
        costs ``ops.select_coherent`` compared (for a robot without a plan: its draws' medoid scores)."""
        if self._plan is None:
            raise RuntimeError("PolicySession.selection: the session was built without select='coherent' (and draws > 1)")
        if self._selected is None:
            raise RuntimeError("PolicySession.selection: no tick has run since the session was built or reset")
        index, cost = self._selected
        return {"index": index.clone(), "cost": cost.clone()}

    def _commit(self, x: torch.Tensor, dev_idx) -> torch.Tensor:
        m = self.model
        if self._anchor is not None and self.carry == 0:
            # the next tick's scan starts from the last row this one commits (normalised space, as sampled).  One launch beside the commit,
            # outside a captured tick like the commit itself: a replay whose range guard trips is repeated eagerly under the OLD anchor.
            if self._anchor2 is not None:   # both rows of the acceleration scan's state, in the same one launch
                ops.session_anchor2(self._anchor, self._anchor2, x, self.advance - 1, self.draws, robots=dev_idx)
            else:
                ops.session_anchor(self._anchor, x, self.advance - 1, self.draws, robots=dev_idx)
        if not self._carrying:
            return ops.session_commit(x, m.mean, m.std, *self._action, robots=dev_idx)
        return ops.session_commit_carry(x, m.mean, m.std, *self._action, self.advance, self.carry, self._pin_x0, self._pin_rows, robots=dev_idx)

    @classmethod
    def from_checkpoint(cls, path: str, device=None, ema: bool = False, **kwargs) -> "PolicySession":
        """A session on the model of a checkpoint written by ``cli train`` / ``cli distill`` (or by the reference).  ``ema=True``: on the
        checkpoint's ``ema_model_state_dict`` (``cli train --ema-decay``) instead of the last iterate; ValueError if it holds none.
        ``direct=None``: as the checkpoint says - True for a distilled one (``cli rollout``)."""
        from .cli import build_model

        ckpt = torch.load(path, map_location="cpu", weights_only=True)
        key = "ema_model_state_dict" if ema else "model_state_dict"
        if key not in ckpt:
            raise ValueError(f"checkpoint {path} has no '{key}' (ema=True needs one trained with --ema-decay)")
        model = build_model(ckpt["hyperparams"]).to(device if device is not None else torch.device("cuda", torch.cuda.current_device()))
        model.load_state_dict(ckpt[key])
        if "direct" in kwargs and kwargs["direct"] is None:
            kwargs["direct"] = bool(ckpt["hyperparams"].get("distilled_decoder", False))
        return cls(model.eval(), hyperparams=ckpt["hyperparams"], **kwargs)
