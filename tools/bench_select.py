#!/usr/bin/env python3
"""What choosing the draw that continues the previous plan costs against choosing the medoid, on the public API, in one process (the
style of tools/bench_draws.py: the arms run in alternating blocks, a figure is the median over the blocks, the spread is the largest
range of an arm's blocks).

launch   the selection launch alone at B contexts x G draws of a (T, J) horizon: ops.select_medoid against ops.select_coherent with
         contrast 0 (G distance sums) and contrast 1 (those plus the medoid's G (G - 1) / 2), microseconds per call, --reps calls
         between two synchronisations.
tick     default.yaml's and sim_scratch.yaml's denoisers without images through PolicySession(draws=G, advance=T // 2), B robots, 30
         steps, eager and use_graph: select="medoid" against select="coherent" with contrast 0 and 1, fed the same sensor rows and noise.

One JSON line per case, the blocks' spread beside every figure.  Exit status 1 when a tick with select="coherent", contrast=0 is slower
than the select="medoid" tick of the same process by more than that case's spread; the contrast=1 figures are reported, not gated.
usage: python tools/bench_select.py [--quick] [--blocks 5] [--reps 200] [--ticks 5] [--draws 8] [--out profiles/select_bench.jsonl]
                                    [--only launch|tick]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_session import BASE, CONFIGS, N_STEPS, sensor_rows  # noqa: E402
from soccerdiffusion_amd import cli, ops  # noqa: E402
from soccerdiffusion_amd.session import PolicySession  # noqa: E402

ARMS = {"medoid": dict(select="medoid"), "coherent0": dict(select="coherent", contrast=0.0), "coherent1": dict(select="coherent", contrast=1.0)}


def summary(blocks):
    return {"median": statistics.median(blocks), "min": min(blocks), "max": max(blocks)}


def spread(arms):
    return max(max(b) - min(b) for b in arms.values())


def bench_launch(B, G, T, J, blocks, reps):
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.randn(B * G, T, J, device="cuda", generator=g)
    prev = torch.randn(B, T, J, device="cuda", generator=g)
    S = T // 2
    index, out = torch.empty(B, dtype=torch.int32, device="cuda"), torch.empty(B, T, J, device="cuda")
    arms = {"medoid": lambda: ops.select_medoid(x, G, index=index, out=out),
            "coherent0": lambda: ops.select_coherent(x, G, prev, S, contrast=0.0, index=index, out=out),
            "coherent1": lambda: ops.select_coherent(x, G, prev, S, contrast=1.0, index=index, out=out)}
    times = {k: [] for k in arms}
    for b in range(blocks + 1):      # block 0: warm-up, not counted
        for k, fn in arms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                fn()
            torch.cuda.synchronize()
            if b:
                times[k].append((time.perf_counter() - t0) / reps * 1e6)
    return {"case": "launch", "B": B, "draws": G, "T": T, "J": J, "shift": S, "blocks": blocks, "reps": reps,
            "call_us": {k: summary(v) for k, v in times.items()}, "spread_us": spread(times)}


def bench_tick(name, B, G, use_graph, blocks, ticks):
    params = {**BASE, **CONFIGS[name], "use_images": False}
    torch.manual_seed(0)
    model = cli.build_model(params).cuda().eval()
    T, J = params["trajectory_prediction_length"], params["num_joints"]
    sessions = {k: PolicySession(model, num_inference_steps=N_STEPS, batch=B, hyperparams=params, use_graph=use_graph, draws=G, advance=T // 2, **kw)
                for k, kw in ARMS.items()}
    g = torch.Generator().manual_seed(2)
    x_T = torch.randn(B * G, T, J, generator=g).cuda()

    def tick(s, new):
        if "joint_state" in new:
            s.push_joint_state(new["joint_state"][:, :T // 2])
        if "rotation" in new:
            s.push_rotation(new["rotation"][:, :T // 2])
        return s.step(x_T).cpu()      # (ends in a device-to-host copy of the trajectory: every tick is synchronised)

    times = {k: [] for k in sessions}
    for b in range(blocks + 1):      # block 0: warm-up (module loads, the graph capture, the first tick without a plan), not counted
        news = [sensor_rows({**params, "image_resolution": 1}, B, g) for _ in range(ticks)]
        for k, s in sessions.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for new in news:
                tick(s, new)
            torch.cuda.synchronize()
            if b:
                times[k].append((time.perf_counter() - t0) / ticks * 1e3)
    med = {k: statistics.median(v) for k, v in times.items()}
    sp = spread(times)
    return {"case": "tick", "config": name, "B": B, "draws": G, "steps": N_STEPS, "T": T, "advance": T // 2, "use_graph": use_graph, "blocks": blocks,
            "ticks": ticks, "tick_ms": {k: summary(v) for k, v in times.items()}, "spread_ms": sp,
            "coherent0_minus_medoid_ms": med["coherent0"] - med["medoid"], "coherent1_minus_medoid_ms": med["coherent1"] - med["medoid"],
            "coherent0_within_spread": med["coherent0"] - med["medoid"] <= sp}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="B = 1 only, two blocks")
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--ticks", type=int, default=5)
    ap.add_argument("--draws", type=int, default=8)
    ap.add_argument("--only", choices=("launch", "tick"), default=None)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    blocks = 2 if args.quick else args.blocks
    sizes = (1,) if args.quick else (1, 16, 64)
    lines, ok = [], True

    def emit(line):
        lines.append(line)
        print(json.dumps(line), flush=True)
        if args.out:      # (rewritten after every case: a run that is cut short keeps what it measured)
            with open(args.out, "w") as f:
                for done in lines:
                    f.write(json.dumps(done) + "\n")

    if args.only in (None, "launch"):
        for B in sizes:
            emit(bench_launch(B, args.draws, BASE["trajectory_prediction_length"], BASE["num_joints"], blocks, args.reps))
        if not args.quick:
            emit(bench_launch(16, 64, 100, 20, blocks, args.reps))      # the largest G at the longest shipped horizon
    if args.only in (None, "tick"):
        for name in ("default", "sim_scratch"):
            for B in sizes:
                for use_graph in (False, True):
                    emit(bench_tick(name, B, args.draws, use_graph, blocks, args.ticks))
                    ok = ok and lines[-1]["coherent0_within_spread"]
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
