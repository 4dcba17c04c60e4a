#!/usr/bin/env python3
"""Tick latency of the closed control loop (soccer_diffusion/ml/inference/ros.py:259-335: budget 0.2 s per tick), PolicySession against
the same tick written on the public API that exists without it - what ros.py does: Python lists of CPU tensors as sensor buffers, per
tick append + trim, torch.stack(...).to(device) of every modality (the whole frame window included), the wrap on the device,
encode_input_data on the full windows (the backbone on all ten frames), model.sample, ops.normalize(inverse) - pi, and the published rows
back into the host-side action list.  Both ticks start from new sensor rows in host memory and end with the trajectory in host memory.

Shapes: default.yaml and sim_scratch.yaml with their images (10 frames of 224 x 224, ResNet-18 without the final avgpool), per tick
trajectory_prediction_length joint-state / rotation samples and two new frames (ros.py:155-163), 30 DDIM steps, B = 1, 16, 64 robots.
Three variants run in one process, in alternating blocks of ticks - the list tick, the session, and the session with use_graph=True
(windows, encoders and rollout replayed from one hipGraph) -; one JSON line per case with the median and the extremes of the blocks per
variant and the spread (the largest range of a variant's blocks).  The list tick's sensor lists are ordinary pageable host tensors, as
ros.py's are.  The first tick of the variants is compared as well (same sensor rows, same noise), and the host time of the session's
stale-weights check (a scan of every parameter's version counter, twice per tick with images) is timed on its own.
Exit status 1 when a session variant is slower than the list tick beyond the spread in any case, or a first tick differs by more than 1e-4.

--reset measures the end of an episode instead (B = 16 and 64): reset(robots=[one robot]), reset(robots=<device mask of half the robots>)
and the whole reset() as the baseline, each followed by its first step(), with use_graph off and on, plus the ordinary tick without a
reset.  One repetition is: two new frames and the other sensor rows pushed (untimed), synchronise, the reset, synchronise (= device plus
host time of the reset), the step, synchronise.  A block is the mean of --ticks repetitions; the variants run in alternating blocks and
every figure is the median over the blocks, with the extremes and the spread as above.  Exit status 1 when a partial reset plus its tick is
slower than the whole reset plus its tick beyond the spread, or, with use_graph, when the tick after a partial reset is slower than an
ordinary replayed tick beyond the spread.

--raw HxW measures the session's two sensor intakes against each other: per tick two uint8 camera frames (H, W, 3) and xyzw quaternions in
host memory through push_camera / push_orientation, against two fp32 frames that are already (3, R, R) and rotation rows that are already in
the model's form through push_image / push_rotation - the second one leaves out the host's cv2.resize, scaling, normalisation and
quats_to_5d, which this tool does not time (cv2 is not a dependency, and another resize would not be the node's).  Two eager sessions on one
model, alternating blocks, medians, extremes and spread as above; no exit status depends on it.

--carry K measures what overlapping ticks cost: PolicySession(carry=K) - the first K rows of every tick pinned to the previous tick's,
the rollout on the pinned instantiations of the step kernels plus one entry launch, the carrying commit - against the session without
carry, eager and with use_graph, four sessions on one model fed the same sensor rows in alternating blocks; medians, extremes and spread
as above, the cost of the pin stated as the difference of the medians.  No exit status depends on it.

--hold measures what held joints cost: PolicySession(holds=True) with two joints of every robot held - one more launch per tick that
composes the mask, the rollout on the hold instantiations of the step kernels plus one entry launch - against the session without holds
(the yardstick: launch for launch the tick as it was), eager and with use_graph, four sessions on one model fed the same sensor rows in
alternating blocks; medians, extremes and spread as above, the cost stated as the difference of the medians.  No exit status depends on it.
usage: python tools/bench_session.py [--quick] [--blocks 7] [--ticks 10] [--reset [--out profiles/session_partial_reset.jsonl]]
                                     [--raw 480x640 [--out profiles/session_raw_tick.jsonl]]
                                     [--carry 4 [--out profiles/session_carry.jsonl]]
                                     [--hold [--out profiles/session_hold.jsonl]]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from soccerdiffusion_amd import cli, ops  # noqa: E402
from soccerdiffusion_amd.session import PolicySession  # noqa: E402

BASE = dict(action_context_length=100, trajectory_prediction_length=10, epochs=1, batch_size=1, lr=1e-4, train_denoising_timesteps=1000,
            image_context_length=10, imu_context_length=100, joint_state_context_length=100, num_normalization_samples=10, num_joints=20,
            use_images=True, image_sequence_encoder_type="transformer", image_encoder_type="resnet18", image_resolution=224,
            image_use_final_avgpool=False, num_image_sequence_encoder_layers=1, distill_teacher_inference_steps=30)
CONFIGS = {   # the values of the reference's YAML of the same name
    "default": dict(hidden_dim=128, use_action_history=True, num_action_history_encoder_layers=2, use_imu=True,
                    imu_orientation_embedding_method="quaternion", num_imu_encoder_layers=2, use_joint_states=True,
                    joint_state_encoder_layers=2, num_decoder_layers=4, use_gamestate=True, encoder_patch_size=1),
    "sim_scratch": dict(hidden_dim=256, use_action_history=True, num_action_history_encoder_layers=4, use_imu=True,
                        imu_orientation_embedding_method="five_dim", num_imu_encoder_layers=2, use_joint_states=False,
                        joint_state_encoder_layers=4, num_decoder_layers=6, use_gamestate=False, encoder_patch_size=5),
}
N_STEPS, NEW_FRAMES = 30, 2


class ListNode:
    """The tick as ros.py writes it, for B robots in lockstep (every list entry is (B, ...))."""

    def __init__(self, model, params, B):
        self.m, self.p, self.B, self.dev = model, params, B, torch.device("cuda")
        J, R = params["num_joints"], params["image_resolution"]
        rot = 5 if params["imu_orientation_embedding_method"] == "five_dim" else 4
        self.len = {"joint_command_history": params["action_context_length"], "rotation": params["imu_context_length"],
                    "joint_state": params["joint_state_context_length"], "image_data": params["image_context_length"]}
        tail = {"joint_command_history": (J,), "rotation": (rot,), "joint_state": (J,), "image_data": (3, R, R)}
        on = {"joint_command_history": params["use_action_history"], "rotation": params["use_imu"], "joint_state": params["use_joint_states"],
              "image_data": params["use_images"]}
        self.lists = {k: [torch.zeros(B, *tail[k])] * self.len[k] for k in tail if on[k]}     # ros.py:87-106

    def append(self, key, rows):
        if key in self.lists:
            for i in range(rows.shape[1]):
                self.lists[key].append(rows[:, i])
            self.lists[key] = self.lists[key][-self.len[key]:]

    def tick(self, new, x_T):
        for key, rows in new.items():
            self.append(key, rows)
        batch = {}
        for key, lst in self.lists.items():                                                     # ros.py:265-275
            x = torch.stack(list(lst), dim=1).to(self.dev)
            batch[key] = (x + 3 * np.pi) % (2 * np.pi) if key in ("joint_state", "joint_command_history") else x
        if self.p["use_gamestate"]:
            batch["game_state"] = torch.zeros(self.B, dtype=torch.long).to(self.dev) + 2
        with torch.no_grad():
            x = self.m.sample(self.m.encode_input_data(batch), x_T, N_STEPS)
            traj = (ops.normalize(x.contiguous(), self.m.mean, self.m.std, inverse=True) - np.pi).cpu()   # ros.py:313-327
        self.append("joint_command_history", traj)
        return traj


def session_tick(s, new, x_T):
    if "joint_state" in new:
        s.push_joint_state(new["joint_state"])
    if "rotation" in new:
        s.push_rotation(new["rotation"])
    s.push_image(new["image_data"])
    return s.step(x_T).cpu()


def sensor_rows(params, B, g):
    J, T, R = params["num_joints"], params["trajectory_prediction_length"], params["image_resolution"]
    new = {"image_data": torch.rand(B, NEW_FRAMES, 3, R, R, generator=g)}
    if params["use_joint_states"]:
        new["joint_state"] = (torch.rand(B, T, J, generator=g) - 0.5) * 2 * np.pi
    if params["use_imu"]:
        new["rotation"] = torch.randn(B, T, 5 if params["imu_orientation_embedding_method"] == "five_dim" else 4, generator=g)
    return new


def block_ms(tick, news, x_T):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for new in news:
        tick(new, x_T)          # (ends in a device-to-host copy of the trajectory: every tick is synchronised)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / len(news) * 1e3


def reset_block_ms(s, kind, news, x_T, mask):
    """(reset ms, first step ms), each the mean over one block of repetitions."""
    t_reset = t_step = 0.0
    for new in news:
        if "joint_state" in new:
            s.push_joint_state(new["joint_state"])
        if "rotation" in new:
            s.push_rotation(new["rotation"])
        s.push_image(new["image_data"])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if kind == "whole":
            s.reset()
        elif kind == "one":
            s.reset(robots=[s.B // 2])
        elif kind == "half_mask":
            s.reset(robots=mask)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        s.step(x_T)
        torch.cuda.synchronize()
        t_reset, t_step = t_reset + (t1 - t0), t_step + (time.perf_counter() - t1)
    return t_reset / len(news) * 1e3, t_step / len(news) * 1e3


def reset_leg(args):
    """Partial reset against whole reset, each with the tick that follows it (--reset)."""
    blocks = 3 if args.quick else args.blocks
    kinds = ("none", "one", "half_mask", "whole")
    failed, lines = False, []
    for name, over in CONFIGS.items():
        params = {**BASE, **over}
        torch.manual_seed(0)
        model = cli.build_model(params).cuda().eval()
        T, J = params["trajectory_prediction_length"], params["num_joints"]
        for B in ((16,) if args.quick else (16, 64)):
            g = torch.Generator().manual_seed(7)
            sessions = {False: PolicySession(model, num_inference_steps=N_STEPS, batch=B, hyperparams=params),
                        True: PolicySession(model, num_inference_steps=N_STEPS, batch=B, hyperparams=params, use_graph=True)}
            x_T = torch.randn(B, T, J, device="cuda", generator=torch.Generator(device="cuda").manual_seed(8))
            mask = (torch.arange(B, device="cuda") % 2 == 0)                 # a simulator's done flags: already on the device
            news = [{k: v.cuda() for k, v in sensor_rows(params, B, g).items()} for _ in range(args.ticks)]
            variants = [(graph, kind) for graph in (False, True) for kind in kinds]
            for graph, kind in variants:                                      # warm-up: one untimed block of every variant
                reset_block_ms(sessions[graph], kind, news, x_T, mask)
            times = {v: [] for v in variants}
            for _ in range(blocks):                                           # alternating blocks: drift of the box hits all of them
                for v in variants:
                    times[v].append(reset_block_ms(sessions[v[0]], v[1], news, x_T, mask))
            rec = {"config": name, "B": B, "steps": N_STEPS, "new_frames_per_tick": NEW_FRAMES, "frame_size": [params["image_resolution"]] * 2,
                   "blocks": blocks, "repetitions_per_block": args.ticks, "one_robot": B // 2, "mask_robots": int(mask.sum())}
            ok = True
            for graph in (False, True):
                cols = {}
                for kind in kinds:
                    r, st = [t[0] for t in times[(graph, kind)]], [t[1] for t in times[(graph, kind)]]
                    both = [a + b for a, b in zip(r, st)]
                    cols[kind] = {"reset_ms": {"median": round(statistics.median(r), 3), "min": round(min(r), 3), "max": round(max(r), 3)},
                                  "first_step_ms": {"median": round(statistics.median(st), 3), "min": round(min(st), 3), "max": round(max(st), 3)},
                                  "reset_plus_step_ms": {"median": round(statistics.median(both), 3), "min": round(min(both), 3),
                                                         "max": round(max(both), 3)}}
                spread = max(c[f]["max"] - c[f]["min"] for c in cols.values() for f in ("reset_plus_step_ms", "first_step_ms"))
                total = lambda kind: cols[kind]["reset_plus_step_ms"]["median"]
                tick = lambda kind: cols[kind]["first_step_ms"]["median"]
                not_slower = bool(total("one") <= total("whole") + spread and total("half_mask") <= total("whole") + spread)
                cols.update(spread_ms=round(spread, 3), partial_not_slower_than_whole_beyond_spread=not_slower)
                ok = ok and not_slower
                if graph:
                    replayed = bool(tick("one") <= tick("none") + spread and tick("half_mask") <= tick("none") + spread)
                    cols["tick_after_partial_reset_costs_a_replayed_tick"] = replayed
                    ok = ok and replayed
                rec["use_graph" if graph else "eager"] = cols
            failed = failed or not ok
            lines.append(json.dumps(rec))
            print(lines[-1], flush=True)
            del sessions
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    if failed:
        raise SystemExit(1)


def raw_tick(s, new, x_T):
    if "joint_state" in new:
        s.push_joint_state(new["joint_state"])
    if "orientation" in new:
        s.push_orientation(new["orientation"])
    s.push_camera(new["camera"])
    return s.step(x_T).cpu()


def raw_leg(args):
    """Raw sensor data through push_camera / push_orientation against preprocessed data through push_image / push_rotation (--raw HxW)."""
    H, W = cli._camera_size(args.raw)
    blocks = 3 if args.quick else args.blocks
    lines = []
    for name, over in CONFIGS.items():
        params = {**BASE, **over}
        torch.manual_seed(0)
        model = cli.build_model(params).cuda().eval()
        T, J = params["trajectory_prediction_length"], params["num_joints"]
        for B in ((1, 16) if args.quick else (1, 16, 64)):
            g = torch.Generator().manual_seed(7)
            s_pre, s_raw = (PolicySession(model, num_inference_steps=N_STEPS, batch=B, hyperparams=params) for _ in range(2))
            x_T = torch.randn(B, T, J, device="cuda", generator=torch.Generator(device="cuda").manual_seed(8))
            pre = [sensor_rows(params, B, g) for _ in range(args.ticks)]
            raw = []
            for new in pre:
                r = {"camera": torch.randint(0, 256, (B, NEW_FRAMES, H, W, 3), dtype=torch.uint8, generator=g)}
                if "joint_state" in new:
                    r["joint_state"] = new["joint_state"]
                if "rotation" in new:
                    r["orientation"] = torch.randn(B, T, 4, generator=g)
                raw.append(r)
            variants = ((lambda new, x: session_tick(s_pre, new, x), pre), (lambda new, x: raw_tick(s_raw, new, x), raw))
            for tick, news in variants:                                    # warm-up: one untimed block of both
                block_ms(tick, news, x_T)
            t_pre, t_raw = [], []
            for _ in range(blocks):                                        # alternating blocks: drift of the box hits both
                for (tick, news), into in zip(variants, (t_pre, t_raw)):
                    into.append(block_ms(tick, news, x_T))
            mp, mr = statistics.median(t_pre), statistics.median(t_raw)
            spread = max(max(v) - min(v) for v in (t_pre, t_raw))
            R = params["image_resolution"]
            rec = {"config": name, "B": B, "steps": N_STEPS, "new_frames_per_tick": NEW_FRAMES, "camera": [H, W], "frame_size": [R, R],
                   "blocks": blocks, "ticks_per_block": args.ticks,
                   "host_bytes_per_tick": {"preprocessed_fp32": B * NEW_FRAMES * 12 * R * R, "raw_uint8": B * NEW_FRAMES * 3 * H * W},
                   "preprocessed_tick_ms": {"median": round(mp, 3), "min": round(min(t_pre), 3), "max": round(max(t_pre), 3)},
                   "raw_tick_ms": {"median": round(mr, 3), "min": round(min(t_raw), 3), "max": round(max(t_raw), 3)},
                   "spread_ms": round(spread, 3), "raw_minus_preprocessed_ms": round(mr - mp, 3),
                   "difference_beyond_spread": bool(abs(mr - mp) > spread),
                   "host_preprocessing": "not timed: the preprocessed variant's frames and rotation rows are made outside the timed blocks"}
            lines.append(json.dumps(rec))
            print(lines[-1], flush=True)
            del s_pre, s_raw
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


def carry_leg(args):
    """The session with carry against the session without, eager and replayed from a graph (--carry K)."""
    blocks = 3 if args.quick else args.blocks
    lines = []
    for name, over in CONFIGS.items():
        params = {**BASE, **over}
        torch.manual_seed(0)
        model = cli.build_model(params).cuda().eval()
        T, J = params["trajectory_prediction_length"], params["num_joints"]
        for B in ((1, 16) if args.quick else (1, 16, 64)):
            g = torch.Generator().manual_seed(7)
            keys = [(graph, carry) for graph in (False, True) for carry in (0, args.carry)]
            sessions = {k: PolicySession(model, num_inference_steps=N_STEPS, batch=B, hyperparams=params, use_graph=k[0], carry=k[1]) for k in keys}
            x_T = torch.randn(B, T, J, device="cuda", generator=torch.Generator(device="cuda").manual_seed(8))
            news = [sensor_rows(params, B, g) for _ in range(args.ticks)]
            for k in keys:                                                 # warm-up: one untimed block of every variant (and the capture)
                block_ms(lambda new, x: session_tick(sessions[k], new, x), news, x_T)
            times = {k: [] for k in keys}
            for _ in range(blocks):                                        # alternating blocks: drift of the box hits all of them
                for k in keys:
                    times[k].append(block_ms(lambda new, x: session_tick(sessions[k], new, x), news, x_T))
            col = lambda v: {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}
            spread = max(max(v) - min(v) for v in times.values())
            med = {k: statistics.median(v) for k, v in times.items()}
            rec = {"config": name, "B": B, "steps": N_STEPS, "new_frames_per_tick": NEW_FRAMES, "frame_size": [params["image_resolution"]] * 2,
                   "memory_rows": PolicySession.plan(params)["memory_rows"], "blocks": blocks, "ticks_per_block": args.ticks,
                   "carry": args.carry, "advance": sessions[(False, args.carry)].advance,
                   "eager": {"carry_0_tick_ms": col(times[(False, 0)]), "carry_tick_ms": col(times[(False, args.carry)]),
                             "pin_cost_ms": round(med[(False, args.carry)] - med[(False, 0)], 3)},
                   "use_graph": {"carry_0_tick_ms": col(times[(True, 0)]), "carry_tick_ms": col(times[(True, args.carry)]),
                                 "pin_cost_ms": round(med[(True, args.carry)] - med[(True, 0)], 3)},
                   "spread_ms": round(spread, 3)}
            rec["pin_cost_beyond_spread"] = bool(max(abs(rec["eager"]["pin_cost_ms"]), abs(rec["use_graph"]["pin_cost_ms"])) > spread)
            lines.append(json.dumps(rec))
            print(lines[-1], flush=True)
            del sessions
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


HELD = ([0, 1], [0.3, -0.7])   # --hold: the head's two joints, say, at fixed angles


def hold_leg(args):
    """The session with two held joints against the session without holds, eager and replayed from a graph (--hold)."""
    blocks = 3 if args.quick else args.blocks
    lines = []
    for name, over in CONFIGS.items():
        params = {**BASE, **over}
        torch.manual_seed(0)
        model = cli.build_model(params).cuda().eval()
        T, J = params["trajectory_prediction_length"], params["num_joints"]
        for B in ((1, 16) if args.quick else (1, 16, 64)):
            g = torch.Generator().manual_seed(7)
            keys = [(graph, holds) for graph in (False, True) for holds in (False, True)]
            sessions = {k: PolicySession(model, num_inference_steps=N_STEPS, batch=B, hyperparams=params, use_graph=k[0], holds=k[1]) for k in keys}
            for k in keys:
                if k[1]:
                    sessions[k].hold(*HELD)
            x_T = torch.randn(B, T, J, device="cuda", generator=torch.Generator(device="cuda").manual_seed(8))
            news = [sensor_rows(params, B, g) for _ in range(args.ticks)]
            for k in keys:                                                 # warm-up: one untimed block of every variant (and the capture)
                block_ms(lambda new, x: session_tick(sessions[k], new, x), news, x_T)
            times = {k: [] for k in keys}
            for _ in range(blocks):                                        # alternating blocks: drift of the box hits all of them
                for k in keys:
                    times[k].append(block_ms(lambda new, x: session_tick(sessions[k], new, x), news, x_T))
            col = lambda v: {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}
            spread = max(max(v) - min(v) for v in times.values())
            med = {k: statistics.median(v) for k, v in times.items()}
            rec = {"config": name, "B": B, "steps": N_STEPS, "new_frames_per_tick": NEW_FRAMES, "frame_size": [params["image_resolution"]] * 2,
                   "memory_rows": PolicySession.plan(params)["memory_rows"], "blocks": blocks, "ticks_per_block": args.ticks,
                   "held_joints": HELD[0],
                   "eager": {"holds_off_tick_ms": col(times[(False, False)]), "holds_on_tick_ms": col(times[(False, True)]),
                             "hold_cost_ms": round(med[(False, True)] - med[(False, False)], 3)},
                   "use_graph": {"holds_off_tick_ms": col(times[(True, False)]), "holds_on_tick_ms": col(times[(True, True)]),
                                 "hold_cost_ms": round(med[(True, True)] - med[(True, False)], 3)},
                   "spread_ms": round(spread, 3)}
            rec["hold_cost_beyond_spread"] = bool(max(abs(rec["eager"]["hold_cost_ms"]), abs(rec["use_graph"]["hold_cost_ms"])) > spread)
            lines.append(json.dumps(rec))
            print(lines[-1], flush=True)
            del sessions
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="B = 1 and 16 only, fewer blocks")
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--ticks", type=int, default=10, help="ticks per block")
    ap.add_argument("--reset", action="store_true", help="measure partial and whole resets with the tick that follows them")
    ap.add_argument("--raw", type=str, default=None, metavar="HxW", help="measure raw uint8 camera frames of this size and quaternions through "
                    "push_camera / push_orientation against preprocessed ones through push_image / push_rotation")
    ap.add_argument("--carry", type=int, default=None, metavar="K", help="measure PolicySession(carry=K) against the session without carry, "
                    "eager and with use_graph")
    ap.add_argument("--hold", action="store_true", help="measure PolicySession(holds=True) with two held joints against the session without "
                    "holds, eager and with use_graph")
    ap.add_argument("--out", type=str, default=None, help="--reset, --raw, --carry, --hold: also write the JSON lines to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_session.py measures on the GPU: no device found")
    if args.reset:
        return reset_leg(args)
    if args.raw:
        return raw_leg(args)
    if args.carry is not None:
        return carry_leg(args)
    if args.hold:
        return hold_leg(args)
    blocks = 3 if args.quick else args.blocks
    failed = False
    for name, over in CONFIGS.items():
        params = {**BASE, **over}
        torch.manual_seed(0)
        model = cli.build_model(params).cuda().eval()
        T, J = params["trajectory_prediction_length"], params["num_joints"]
        for B in ((1, 16) if args.quick else (1, 16, 64)):
            g = torch.Generator().manual_seed(7)
            node, s = ListNode(model, params, B), PolicySession(model, num_inference_steps=N_STEPS, batch=B, hyperparams=params)
            sg = PolicySession(model, num_inference_steps=N_STEPS, batch=B, hyperparams=params, use_graph=True)
            x_T = torch.randn(B, T, J, device="cuda", generator=torch.Generator(device="cuda").manual_seed(8))
            first = sensor_rows(params, B, g)
            a, b, c = node.tick(first, x_T), session_tick(s, first, x_T), session_tick(sg, first, x_T)   # same state, rows, noise
            err = float((b.double() - a.double()).norm() / a.double().norm())
            err_graph = float((c.double() - b.double()).norm() / b.double().norm())
            news = [sensor_rows(params, B, g) for _ in range(args.ticks)]
            variants = (node.tick, lambda new, x: session_tick(s, new, x), lambda new, x: session_tick(sg, new, x))
            for tick in variants:                                          # warm-up: one untimed block of every variant at this shape
                block_ms(tick, news, x_T)
            base, sess, graph = [], [], []
            for _ in range(blocks):                                        # alternating blocks: drift of the box hits all of them
                for tick, into in zip(variants, (base, sess, graph)):
                    into.append(block_ms(tick, news, x_T))
            mb, ms, mg = statistics.median(base), statistics.median(sess), statistics.median(graph)
            spread = max(max(v) - min(v) for v in (base, sess, graph))
            t0 = time.perf_counter()
            for _ in range(200):
                s._check_weights("bench")
            check_us = (time.perf_counter() - t0) / 200 * 1e6
            ok = bool(ms <= mb + spread and mg <= mb + spread and err < 1e-4 and err_graph < 1e-4)
            failed = failed or not ok
            rec = {"config": name, "B": B, "steps": N_STEPS, "frames_in_window": params["image_context_length"], "new_frames_per_tick": NEW_FRAMES,
                   "frame_size": [params["image_resolution"]] * 2, "memory_rows": PolicySession.plan(params)["memory_rows"],
                   "blocks": blocks, "ticks_per_block": args.ticks,
                   "list_tick_ms": {"median": round(mb, 3), "min": round(min(base), 3), "max": round(max(base), 3)},
                   "list_buffers": "pageable host memory",
                   "session_tick_ms": {"median": round(ms, 3), "min": round(min(sess), 3), "max": round(max(sess), 3)},
                   "session_graph_tick_ms": {"median": round(mg, 3), "min": round(min(graph), 3), "max": round(max(graph), 3)},
                   "spread_ms": round(spread, 3), "gain": round(mb / ms, 3), "gain_graph": round(mb / mg, 3),
                   "graph_minus_eager_ms": round(mg - ms, 3), "weights_check_us": round(check_us, 1),
                   "session_not_slower_beyond_spread": ok, "first_tick_rel_err": float(f"{err:.3e}"),
                   "first_tick_graph_vs_eager_rel_err": float(f"{err_graph:.3e}")}
            print(json.dumps(rec), flush=True)
            del node, s, sg
    if failed:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
