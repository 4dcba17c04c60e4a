#!/usr/bin/env python3
"""What the fused direct launch of a distilled one-step decoder buys over two launches, on the public API (the style of
tools/bench_slew.py: the arms of a comparison run in alternating blocks in ONE process, a figure is the median over the blocks, the spread
is the largest range of an arm's blocks; no exit status depends on a figure).  The denoiser shapes are default.yaml's and
sim_scratch.yaml's (tools/bench_session.py), the context rows those of a PolicySession's first tick, and bench.py's shape (hidden_dim 256,
4 layers, horizon 100, 10 context rows), B = 1, 16 and 64 trajectories.

(a) call   ops.direct_sample with limits (the 25 % / 75 % quantiles of the prediction), slew limits (the median |row difference|,
           anchored) and two held joints - ONE launch of the direct twin of the step kernel behind the preparation - against the same
           prediction without any of them followed by ops.direct_project: the plain direct launch (the eps launch's work plus one store)
           and the projection kernel as a second launch.  Both arms pay the same preparation of weights, context and step token.
(b) tick   a PolicySession tick on the distilled decoder with limits, slew and two held joints, eager against replayed from its graph.

One JSON line per (comparison, config, B).
usage: python tools/bench_direct.py [--quick] [--blocks 5] [--reps 5] [--ticks 4] [--out profiles/direct_bench.jsonl]"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_multistep import compare   # noqa: E402


def calls(args, batches, lines):
    import torch

    from bench_session import BASE, CONFIGS
    from soccerdiffusion_amd import _lib, cli, ops
    from soccerdiffusion_amd.session import PolicySession

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
        token = ops.step_token(torch.zeros(1, dtype=torch.int64, device="cuda"), model.step_encoding._freq, model.step_encoding.token.detach())
        for B in batches:
            ctx = torch.randn(B, Mc, d, device="cuda", generator=g)
            x_T = torch.randn(B, T, J, device="cuda", generator=g)
            raw = ops.direct_sample(packed, ctx, token, x_T)
            flat = raw.reshape(-1, J)
            lim = ops.joint_limits(flat.quantile(0.25, dim=0), flat.quantile(0.75, dim=0), J=J, device="cuda")
            v = ops.joint_slew((raw[:, 1:] - raw[:, :-1]).abs().reshape(-1, J).median(dim=0).values, J=J, device="cuda")
            start = torch.full((B, 32), float("nan"), device="cuda")
            start[:, :J] = raw[:, T // 2]
            mask = torch.zeros(J, dtype=torch.bool, device="cuda")
            mask[:2] = True
            hold = (torch.zeros_like(raw), ops.hold_mask(mask, B, T, J, "cuda"))
            kw = dict(hold=hold, limits=lim, slew=(v, start))
            fused = ops.direct_sample(packed, ctx, token, x_T, **kw)
            assert torch.equal(fused.view(torch.int32), ops.direct_project(raw, **kw).view(torch.int32))     # the two arms compute the same bits
            moved = float((fused != raw).float().mean())
            arms = {"fused": lambda: ops.direct_sample(packed, ctx, token, x_T, **kw),
                    "two_launches": lambda: ops.direct_project(ops.direct_sample(packed, ctx, token, x_T), **kw),
                    "plain": lambda: ops.direct_sample(packed, ctx, token, x_T)}
            res = compare(arms, args.blocks, args.reps)
            med = {k: res[k]["median"] for k in arms}
            line = {"case": "call", "config": name, "B": B, "d": d, "L": L, "T": T, "J": J, "Mc": Mc,
                    "route": _lib.sampler_route(d, 4, T, Mc, J, L, B, 3), "blocks": args.blocks, "reps": args.reps, "moved": round(moved, 3),
                    "call_ms": res, "fused_minus_two_launches_ms": med["fused"] - med["two_launches"],
                    "fused_minus_plain_ms": med["fused"] - med["plain"]}
            line["beyond_spread"] = bool(abs(line["fused_minus_two_launches_ms"]) > res["spread_ms"])
            lines.append(json.dumps(line))
            print(lines[-1], flush=True)
        del model, packed


def ticks(args, batches, lines):
    import torch

    from bench_session import BASE, CONFIGS, block_ms, sensor_rows, session_tick
    from soccerdiffusion_amd import cli
    from soccerdiffusion_amd.session import PolicySession

    for name, over in CONFIGS.items():
        params = {**BASE, **over, "distilled_decoder": True}
        torch.manual_seed(0)
        model = cli.build_model(params).cuda().eval()
        T, J = params["trajectory_prediction_length"], params["num_joints"]
        for B in batches:
            g = torch.Generator().manual_seed(7)
            sessions = {graph: PolicySession(model, batch=B, hyperparams=params, direct=True, use_graph=graph, limits=1.0, slew=0.1,
                                         holds=True) for graph in (False, True)}
            for s in sessions.values():
                s.hold([0, 1], [0.3, -0.7])
            x_T = torch.randn(B, T, J, device="cuda", generator=torch.Generator(device="cuda").manual_seed(8))
            news = [sensor_rows(params, B, g) for _ in range(args.ticks)]
            for k in sessions:                                             # warm-up: one untimed block of either variant (and the capture)
                block_ms(lambda new, x: session_tick(sessions[k], new, x), news, x_T)
            times = {k: [] for k in sessions}
            for _ in range(args.blocks):                                   # alternating blocks: drift of the box hits both
                for k in sessions:
                    times[k].append(block_ms(lambda new, x: session_tick(sessions[k], new, x), news, x_T))
            col = lambda u: {"median": round(statistics.median(u), 3), "min": round(min(u), 3), "max": round(max(u), 3)}
            spread = max(max(u) - min(u) for u in times.values())
            rec = {"case": "tick", "config": name, "B": B, "memory_rows": PolicySession.plan(params)["memory_rows"], "blocks": args.blocks,
                   "ticks_per_block": args.ticks, "eager_tick_ms": col(times[False]), "use_graph_tick_ms": col(times[True]),
                   "graph_minus_eager_ms": round(statistics.median(times[True]) - statistics.median(times[False]), 3), "spread_ms": round(spread, 3)}
            rec["beyond_spread"] = bool(abs(rec["graph_minus_eager_ms"]) > spread)
            lines.append(json.dumps(rec))
            print(lines[-1], flush=True)
            del sessions
        del model


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="2 blocks of 2 calls, B = 1 and 16")
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ticks", type=int, default=4, help="ticks per block of the session comparison")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.quick:
        args.blocks, args.reps = 2, 2
    lines = []
    calls(args, (1, 16) if args.quick else (1, 16, 64), lines)
    ticks(args, (1, 16), lines)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
