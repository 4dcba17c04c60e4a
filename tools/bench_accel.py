#!/usr/bin/env python3
"""What per-joint acceleration limits cost in time, on the public API (tools/bench_slew.py's protocol: the arms of a comparison run in
alternating blocks in ONE process, a figure is the median over the blocks, the spread is the largest range of an arm's blocks).  The
comparison is acceleration limits on against slew limits only in the same process; no exit status depends on a figure.  The denoiser
shapes are default.yaml's and sim_scratch.yaml's (tools/bench_session.py), the context rows those of a PolicySession's first tick, and
bench.py's shape (hidden_dim 256, 4 layers, horizon 100, 10 context rows), B = 1, 16 and 64 trajectories.

(a) rollout  an n-step rollout with limits (+- 1 on every joint), slew limits (0.25 per row, anchored) and acceleration limits (0.125 per
             row^2 on every joint, both anchors: they bind) against the same rollout with limits and slew alone, for DDIM and for the
             multistep solver.  Both are one launch per step on the trajectory routes: the slew twin of the step kernel against its
             acceleration twin, whose scan carries two rows (four more dependent operations per row) and whose embedding takes one pass
             over x for the rows' scales (x_token_scale: one more barrier).
(b) tick     a PolicySession tick with limits, slew (0.1 rad per row as published) and accel (0.05 rad per row^2) against the session
             with limits and slew alone, eager and replayed from its graph.

One JSON line per (comparison, config, B).
usage: python tools/bench_accel.py [--quick] [--blocks 5] [--reps 5] [--ticks 4] [--out profiles/accel_bench.jsonl]"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_multistep import compare   # noqa: E402


def rollouts(args, batches, lines):
    import torch

    from bench_session import BASE, CONFIGS
    from soccerdiffusion_amd import _lib, cli, ops
    from soccerdiffusion_amd.session import PolicySession

    acp = ops.alphas_cumprod()
    bench_shape = dict(CONFIGS["sim_scratch"], hidden_dim=256, num_decoder_layers=4, trajectory_prediction_length=100, use_images=False)
    for name in ("default", "sim_scratch", "bench"):
        params = {**BASE, **(bench_shape if name == "bench" else CONFIGS[name])}
        torch.manual_seed(0)
        model = cli.build_model(params).cuda().eval()
        packed = model.diffusion_action_generator.packed()
        d, L, T, J = params["hidden_dim"], params["num_decoder_layers"], params["trajectory_prediction_length"], params["num_joints"]
        if name == "bench":
            Mc = 10
        else:
            with torch.no_grad():
                Mc = sum(int(c.shape[1]) for c in PolicySession(model, batch=1, hyperparams=params)._context())
        g = torch.Generator(device="cuda").manual_seed(1)
        ts = ops.ddim_timesteps(args.steps)
        toks, coef, w = model.step_encoding.table(ts, torch.device("cuda")), ops.ddim_coefficients(ts, acp, args.steps), ops.multistep_weights(ts, acp, args.steps)
        lim = ops.joint_limits(1.0, J=J, device="cuda")
        v = ops.joint_slew(0.25, J=J, device="cuda")
        acc = ops.joint_accel(0.125, J=J, device="cuda")
        for B in batches:
            ctx = torch.randn(B, Mc, d, device="cuda", generator=g)
            x_T = torch.randn(B, T, J, device="cuda", generator=g)
            start = torch.full((B, 32), float("nan"), device="cuda")
            start[:, :J] = 0.5 * torch.randn(B, J, device="cuda", generator=g)
            start2 = torch.full((B, 32), float("nan"), device="cuda")
            start2[:, :J] = start[:, :J] + 0.25 * torch.randn(B, J, device="cuda", generator=g)
            arms = {"ddim_slew": lambda: ops.ddim_sample(packed, ctx, toks, coef, x_T, limits=lim, slew=(v, start)),
                    "ddim_accel": lambda: ops.ddim_sample(packed, ctx, toks, coef, x_T, limits=lim, slew=(v, start), accel=(acc, start2)),
                    "multistep_slew": lambda: ops.ddim_sample(packed, ctx, toks, coef, x_T, multistep=w, limits=lim, slew=(v, start)),
                    "multistep_accel": lambda: ops.ddim_sample(packed, ctx, toks, coef, x_T, multistep=w, limits=lim, slew=(v, start),
                                                               accel=(acc, start2))}
            res = compare(arms, args.blocks, args.reps)
            med = {k: res[k]["median"] for k in arms}
            line = {"case": "rollout", "steps": args.steps, "config": name, "B": B, "d": d, "L": L, "T": T, "J": J, "Mc": Mc,
                    "route": _lib.sampler_route(d, 4, T, Mc, J, L, B, 3), "blocks": args.blocks, "reps": args.reps, "rollout_ms": res,
                    "ddim_accel_minus_slew_ms": med["ddim_accel"] - med["ddim_slew"],
                    "multistep_accel_minus_slew_ms": med["multistep_accel"] - med["multistep_slew"]}
            line["beyond_spread"] = bool(max(abs(line["ddim_accel_minus_slew_ms"]), abs(line["multistep_accel_minus_slew_ms"])) > res["spread_ms"])
            lines.append(json.dumps(line))
            print(lines[-1], flush=True)
        del model, packed


def ticks(args, batches, lines):
    import torch

    from bench_session import BASE, CONFIGS, N_STEPS, block_ms, sensor_rows, session_tick
    from soccerdiffusion_amd import cli
    from soccerdiffusion_amd.session import PolicySession

    for name, over in CONFIGS.items():
        params = {**BASE, **over}
        torch.manual_seed(0)
        model = cli.build_model(params).cuda().eval()
        T, J = params["trajectory_prediction_length"], params["num_joints"]
        for B in batches:
            g = torch.Generator().manual_seed(7)
            keys = [(graph, accel) for graph in (False, True) for accel in (False, True)]
            sessions = {k: PolicySession(model, num_inference_steps=N_STEPS, batch=B, hyperparams=params, use_graph=k[0], limits=1.0,
                                         slew=0.1, accel=0.05 if k[1] else None) for k in keys}
            x_T = torch.randn(B, T, J, device="cuda", generator=torch.Generator(device="cuda").manual_seed(8))
            news = [sensor_rows(params, B, g) for _ in range(args.ticks)]
            for k in keys:                                                 # warm-up: one untimed block of every variant (and the capture)
                block_ms(lambda new, x: session_tick(sessions[k], new, x), news, x_T)
            times = {k: [] for k in keys}
            for _ in range(args.blocks):                                   # alternating blocks: drift of the box hits all of them
                for k in keys:
                    times[k].append(block_ms(lambda new, x: session_tick(sessions[k], new, x), news, x_T))
            col = lambda u: {"median": round(statistics.median(u), 3), "min": round(min(u), 3), "max": round(max(u), 3)}
            spread = max(max(u) - min(u) for u in times.values())
            med = {k: statistics.median(u) for k, u in times.items()}
            rec = {"case": "tick", "config": name, "B": B, "steps": N_STEPS, "memory_rows": PolicySession.plan(params)["memory_rows"],
                   "blocks": args.blocks, "ticks_per_block": args.ticks,
                   "eager": {"slew_tick_ms": col(times[(False, False)]), "accel_tick_ms": col(times[(False, True)]),
                             "accel_cost_ms": round(med[(False, True)] - med[(False, False)], 3)},
                   "use_graph": {"slew_tick_ms": col(times[(True, False)]), "accel_tick_ms": col(times[(True, True)]),
                                 "accel_cost_ms": round(med[(True, True)] - med[(True, False)], 3)},
                   "spread_ms": round(spread, 3)}
            rec["beyond_spread"] = bool(max(abs(rec["eager"]["accel_cost_ms"]), abs(rec["use_graph"]["accel_cost_ms"])) > spread)
            lines.append(json.dumps(rec))
            print(lines[-1], flush=True)
            del sessions
        del model


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="2 blocks of 2 calls, B = 1 and 16")
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10, help="n of the rollouts")
    ap.add_argument("--ticks", type=int, default=4, help="ticks per block of the session comparison")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.quick:
        args.blocks, args.reps = 2, 2
    batches = (1, 16) if args.quick else (1, 16, 64)
    lines = []
    rollouts(args, batches, lines)
    ticks(args, batches, lines)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
