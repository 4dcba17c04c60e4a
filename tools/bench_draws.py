#!/usr/bin/env python3
"""What several draws per observation cost, on the public API, in one process (the style of tools/bench_session.py: the arms run in
alternating blocks, a figure is the median over the blocks, the spread is the largest range of an arm's blocks).

sampler  C contexts x G draws (default 512 x 8 = 4096 trajectories, 50 steps, T = 100, J = 20, d = 256, L = 4, Mc = 10) through
         ops.ddim_sample: "shared" = draws=G on the C contexts (sd_ddim_sample_draws: the context prepared once per context, the shared
         instantiations of the step kernels) against "repeated" = today's call on ctx.repeat_interleave(G, 0), which runs the parent's
         kernels (profiles/draws_isa.txt).  Wall time per call; in a second pass with the library's profiler on, the time of the step-kernel
         class (the rollout) - preparation = wall - rollout.
session  default.yaml and sim_scratch.yaml ticks through PolicySession, B robots, 30 steps, eager and use_graph: the session without the
         argument, draws=1, and draws=G for every G asked for, fed the same sensor rows.

One JSON line per case.  No exit status depends on a ratio: nothing here has been measured before.
usage: python tools/bench_draws.py [--quick] [--blocks 5] [--reps 3] [--ticks 5] [--out profiles/draws_bench.jsonl] [--only sampler|session]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_session import BASE, CONFIGS, N_STEPS, sensor_rows  # noqa: E402
from soccerdiffusion_amd import _lib, cli, ops  # noqa: E402
from soccerdiffusion_amd.session import PolicySession  # noqa: E402


def summary(blocks):
    return {"median": statistics.median(blocks), "min": min(blocks), "max": max(blocks)}


def spread(arms):
    return max(max(b) - min(b) for b in arms.values())


def wall_ms(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def step_class_ms(fn):
    """ms of the step-kernel class (and its launches) of one call, from the library's profiler."""
    lib = _lib.load()
    n = len(_lib.KERNEL_CLASSES)
    torch.cuda.synchronize()
    lib.sd_profile_enable(1)
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        lib.sd_profile_enable(0)
    ms, cnt = (C.c_double * n)(), (C.c_long * n)()
    _lib.check(lib.sd_profile_collect(ms, cnt, n), "sd_profile_collect")
    i = _lib.KERNEL_CLASSES.index("traj_step_kernel")
    return ms[i], int(cnt[i])


def bench_sampler(Cn, G, steps, blocks, reps):
    d, L, T, J, Mc = 256, 4, 100, 20, 10
    params = {**BASE, "hidden_dim": d, "num_decoder_layers": L, "trajectory_prediction_length": T, "num_joints": J, "use_images": False,
              "use_action_history": False, "use_imu": False, "use_joint_states": False, "use_gamestate": False, "encoder_patch_size": 5,
              "num_action_history_encoder_layers": 1, "num_imu_encoder_layers": 1, "joint_state_encoder_layers": 1,
              "imu_orientation_embedding_method": "quaternion"}
    torch.manual_seed(0)
    model = cli.build_model(params).cuda().eval()
    packed = model.diffusion_action_generator.packed()
    ts = ops.ddim_timesteps(steps)
    toks = model.step_encoding.table(ts, torch.device("cuda"))
    coef = ops.ddim_coefficients(ts, ops.alphas_cumprod(), steps)
    g = torch.Generator(device="cuda").manual_seed(1)
    ctx = torch.randn(Cn, Mc, d, device="cuda", generator=g)
    rep = ctx.repeat_interleave(G, 0).contiguous()
    x_T = torch.randn(Cn * G, T, J, device="cuda", generator=g)
    arms = {"shared": lambda: ops.ddim_sample(packed, ctx, toks, coef, x_T, draws=G),
            "repeated": lambda: ops.ddim_sample(packed, rep, toks, coef, x_T)}
    same = torch.equal(arms["shared"](), arms["repeated"]())    # (also the warm-up)
    wall = {k: [] for k in arms}
    roll = {k: [] for k in arms}
    launches = {}
    for _ in range(blocks):
        for k, fn in arms.items():
            wall[k].append(wall_ms(fn, reps))
        for k, fn in arms.items():
            ms, launches[k] = step_class_ms(fn)
            roll[k].append(ms)
    out = {"case": "sampler", "contexts": Cn, "draws": G, "trajectories": Cn * G, "steps": steps, "T": T, "J": J, "d": d, "L": L, "Mc": Mc,
           "route": _lib.sampler_route_draws(d, 4, T, Mc, J, L, Cn * G, G), "bitwise_equal": same, "blocks": blocks, "reps": reps,
           "step_launches": launches}
    for k in arms:
        out[k] = {"wall_ms": summary(wall[k]), "rollout_ms": summary(roll[k]),
                  "prepare_ms": statistics.median(wall[k]) - statistics.median(roll[k]),
                  "trajectories_per_s": Cn * G / statistics.median(wall[k]) * 1e3}
    out["spread_ms"] = {"wall": spread(wall), "rollout": spread(roll)}
    out["shared_over_repeated"] = {"wall": out["shared"]["wall_ms"]["median"] / out["repeated"]["wall_ms"]["median"],
                                   "rollout": out["shared"]["rollout_ms"]["median"] / out["repeated"]["rollout_ms"]["median"]}
    return out


def bench_session(name, B, Gs, use_graph, blocks, ticks):
    params = {**BASE, **CONFIGS[name]}
    torch.manual_seed(0)
    model = cli.build_model(params).cuda().eval()
    sessions = {"plain": PolicySession(model, num_inference_steps=N_STEPS, batch=B, hyperparams=params, use_graph=use_graph)}
    for G in Gs:
        sessions[f"draws{G}"] = PolicySession(model, num_inference_steps=N_STEPS, batch=B, hyperparams=params, use_graph=use_graph, draws=G)
    g = torch.Generator().manual_seed(2)
    T, J = params["trajectory_prediction_length"], params["num_joints"]
    noise = {k: torch.randn(B * s.draws, T, J, generator=g).cuda() for k, s in sessions.items()}

    def tick(s, new, x_T):
        if "joint_state" in new:
            s.push_joint_state(new["joint_state"])
        if "rotation" in new:
            s.push_rotation(new["rotation"])
        s.push_image(new["image_data"])
        return s.step(x_T).cpu()

    times = {k: [] for k in sessions}
    for b in range(blocks + 1):     # block 0: warm-up (module loads, the graph capture), not counted
        news = [sensor_rows(params, B, g) for _ in range(ticks)]
        for k, s in sessions.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for new in news:
                tick(s, new, noise[k])
            torch.cuda.synchronize()
            if b:
                times[k].append((time.perf_counter() - t0) / ticks * 1e3)
    out = {"case": "session", "config": name, "B": B, "steps": N_STEPS, "use_graph": use_graph, "blocks": blocks, "ticks": ticks,
           "tick_ms": {k: summary(v) for k, v in times.items()}, "spread_ms": spread(times)}
    med = {k: statistics.median(v) for k, v in times.items()}
    out["draws1_minus_plain_ms"] = med["draws1"] - med["plain"] if "draws1" in med else None
    out["cost_over_one_draw"] = {k: med[k] / med["plain"] for k in med if k != "plain"}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="64 x 8 trajectories, 10 steps, B = 1 only, two blocks")
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--ticks", type=int, default=5)
    ap.add_argument("--only", choices=("sampler", "session"), default=None)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    blocks = 2 if args.quick else args.blocks
    lines = []
    if args.only in (None, "sampler"):
        lines.append(bench_sampler(64 if args.quick else 512, 8, 10 if args.quick else 50, blocks, args.reps))
        print(json.dumps(lines[-1]), flush=True)
    if args.only in (None, "session"):
        for name in ("default", "sim_scratch"):
            for B in ((1,) if args.quick else (1, 16)):
                for use_graph in (False, True):
                    lines.append(bench_session(name, B, (1, 4, 8), use_graph, blocks, args.ticks))
                    print(json.dumps(lines[-1]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
