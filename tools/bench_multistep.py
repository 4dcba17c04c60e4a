#!/usr/bin/env python3
"""What the second-order multistep solver costs and buys in time, on the public API (the style of tools/bench_draws.py: the arms of a
comparison run in alternating blocks in ONE process, a figure is the median over the blocks, the spread is the largest range of an
arm's blocks).  The denoiser shapes are default.yaml's and sim_scratch.yaml's (tools/bench_session.py), the context rows those of a
PolicySession's first tick, B = 1, 16 and 64 trajectories.  Neither shipped shape is one the plan fuses (the generic family, and more than
16 memory rows), so a third shape, "bench" - bench.py's: hidden_dim 256, 4 layers, horizon 100, 10 context rows - gives comparison (b) a
case where DDIM does run the fused rollout kernel.

(a) term     an n-step multistep rollout against an n-step DDIM rollout forced to one launch per step (SD_TRAJ_ROLLOUT=steps): what the
             extra term costs.  The switch is read once per process, so this comparison runs in a child process of its own with the
             switch set; both of its arms run there.
(b) fused    the same against the default DDIM rollout (the fused rollout kernel where the plan has one): what not having a fused twin
             costs.  `ddim_rollout` says which form the plan gives this shape in this process (FUSED or PER_STEP).
(c) headline 10 multistep steps against 30 DDIM steps, eager (ops.ddim_sample) and replayed (ops.GraphedSampler).

One JSON line per (comparison, config, B).  No exit status depends on a ratio: nothing here has been measured before.
usage: python tools/bench_multistep.py [--quick] [--blocks 5] [--reps 5] [--out profiles/multistep_bench.jsonl]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def summary(blocks):
    return {"median": statistics.median(blocks), "min": min(blocks), "max": max(blocks)}


def compare(arms, blocks, reps):
    """{arm: summary of ms per call}, the spread, for callables run in alternating blocks."""
    import torch

    def wall_ms(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / reps * 1e3

    for fn in arms.values():   # warm-up: module loads, LDS attributes, workspaces
        fn()
    times = {k: [] for k in arms}
    for _ in range(blocks):
        for k, fn in arms.items():
            times[k].append(wall_ms(fn))
    out = {k: summary(v) for k, v in times.items()}
    out["spread_ms"] = max(max(v) - min(v) for v in times.values())
    return out


def child(which, n, blocks, reps, batches):
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

        def plan(steps):
            ts = ops.ddim_timesteps(steps)
            return (model.step_encoding.table(ts, torch.device("cuda")), ops.ddim_coefficients(ts, acp, steps), ops.multistep_weights(ts, acp, steps))

        for B in batches:
            ctx = torch.randn(B, Mc, d, device="cuda", generator=g)
            x_T = torch.randn(B, T, J, device="cuda", generator=g)
            base = {"config": name, "B": B, "d": d, "L": L, "T": T, "J": J, "Mc": Mc, "route": _lib.sampler_route(d, 4, T, Mc, J, L, B, 3),
                    "blocks": blocks, "reps": reps}
            if which in ("term", "fused"):
                toks, coef, w = plan(n)
                arms = {"multistep": lambda: ops.ddim_sample(packed, ctx, toks, coef, x_T, multistep=w),
                        "ddim": lambda: ops.ddim_sample(packed, ctx, toks, coef, x_T)}
                res = compare(arms, blocks, reps)
                line = {"case": which, "steps": n, **base, "ddim_rollout": _lib.sampler_rollout(d, 4, T, Mc, J, L, B, 3),
                        "rollout_ms": res, "multistep_minus_ddim_ms": res["multistep"]["median"] - res["ddim"]["median"]}
                print(json.dumps(line), flush=True)
                continue
            t10, c10, w10 = plan(10)
            t30, c30, _ = plan(30)
            for graphed in (False, True):
                if graphed:
                    g10 = ops.GraphedSampler(packed, B, T, Mc, t10, c10, multistep=w10)
                    g30 = ops.GraphedSampler(packed, B, T, Mc, t30, c30)
                    arms = {"multistep10": lambda: g10.replay_into(ctx, x_T), "ddim30": lambda: g30.replay_into(ctx, x_T)}
                else:
                    arms = {"multistep10": lambda: ops.ddim_sample(packed, ctx, t10, c10, x_T, multistep=w10),
                            "ddim30": lambda: ops.ddim_sample(packed, ctx, t30, c30, x_T),
                            "ddim10": lambda: ops.ddim_sample(packed, ctx, t10, c10, x_T)}
                res = compare(arms, blocks, reps)
                line = {"case": "headline", "graphed": graphed, **base, "rollout_ms": res,
                        "ddim30_over_multistep10": res["ddim30"]["median"] / res["multistep10"]["median"]}
                print(json.dumps(line), flush=True)
                if graphed:
                    del g10, g30


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="2 blocks of 2 calls, B = 1 and 16")
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10, help="n of comparisons (a) and (b)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", choices=("term", "fused", "headline"), default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.quick:
        args.blocks, args.reps = 2, 2
    batches = (1, 16) if args.quick else (1, 16, 64)
    if args.child:
        child(args.child, args.steps, args.blocks, args.reps, batches)
        return 0
    lines = []
    for which in ("term", "fused", "headline"):   # one fresh process each; the first with the per-step switch set
        env = dict(os.environ, PYTHONPATH=REPO)
        env.pop("SD_TRAJ_ROLLOUT", None)
        if which == "term":
            env["SD_TRAJ_ROLLOUT"] = "steps"
        cmd = [sys.executable, os.path.abspath(__file__), "--child", which, "--blocks", str(args.blocks), "--reps", str(args.reps), "--steps",
               str(args.steps)] + (["--quick"] if args.quick else [])
        r = subprocess.run(cmd, env=env, capture_output=True, text=True)
        sys.stderr.write(r.stderr[-2000:])
        if r.returncode != 0:
            return r.returncode
        for line in r.stdout.splitlines():
            if line.startswith("{"):
                print(line, flush=True)
                lines.append(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
