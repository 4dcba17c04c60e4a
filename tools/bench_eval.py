#!/usr/bin/env python3
"""What sharing the folded context buys a validation loss grid, in one process (the style of tools/bench_draws.py: the arms run in
alternating blocks, a figure is the median over the blocks, the spread is the largest range of an arm's blocks).

A grid is the denoiser at K timesteps of each of C windows: C K trajectories, K per context, each with its own step token.
  shared    sd_sampler_prepare_draws / sd_sampler_eps_draws with draws = K on the C contexts: C contexts projected, folded and packed
  repeated  today's loop form on ctx.repeat_interleave(K, 0): C K contexts folded, K copies of each (the expansion is timed on its own)
Per arm, separately: the context preparation (SD_PREPARE_CONTEXT alone; the weights are prepared once, outside) and the evaluation (the
step tokens' fold and the step launch), wall time around a synchronised call, and the step-kernel class from the library's profiler.
Shapes: decoder_only.yaml as train.py feeds it (T = 10, ten context rows) and the benchmark's T = 100; d = 256, L = 4, J = 20.

One JSON line per shape.  No exit status depends on a ratio: nothing here has been measured before.
usage: python tools/bench_eval.py [--quick] [--blocks 5] [--reps 20] [--out profiles/eval_bench.jsonl]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_draws import spread, step_class_ms, summary, wall_ms  # noqa: E402
from bench_session import BASE  # noqa: E402
from soccerdiffusion_amd import _lib, cli, evaluation, ops  # noqa: E402


def bench_grid(name, Cn, K, T, blocks, reps):
    d, L, J, Mc = 256, 4, 20, 10
    params = {**BASE, "hidden_dim": d, "num_decoder_layers": L, "trajectory_prediction_length": T, "num_joints": J, "use_images": False,
              "use_action_history": False, "use_imu": False, "use_joint_states": False, "use_gamestate": False, "encoder_patch_size": 5,
              "num_action_history_encoder_layers": 1, "num_imu_encoder_layers": 1, "joint_state_encoder_layers": 1,
              "imu_orientation_embedding_method": "quaternion"}
    torch.manual_seed(0)
    model = cli.build_model(params).cuda().eval()
    packed = model.diffusion_action_generator.packed()
    lib = _lib.load()
    B = Cn * K
    g = torch.Generator(device="cuda").manual_seed(1)
    ctx = torch.randn(Cn, Mc, d, device="cuda", generator=g)
    x = torch.randn(B, T, J, device="cuda", generator=g)
    steps = torch.tensor(evaluation.default_timesteps(K), device="cuda").repeat(Cn)
    tokens = ops.step_token(steps, model.step_encoding._freq, model.step_encoding.token.detach()).view(B, d).contiguous()
    w, st = C.byref(packed.struct), torch.cuda.current_stream().cuda_stream
    ws = {k: torch.empty(lib.sd_workspace_floats(B, T, Mc, d, L, B), dtype=torch.float32, device="cuda") for k in ("shared", "repeated")}
    eps = {k: torch.empty_like(x) for k in ws}
    draws = {"shared": K, "repeated": 1}
    rep = [None]

    def expand():
        rep[0] = ctx.repeat_interleave(K, 0).contiguous()

    def prepare(k, what=ops.PREPARE_CONTEXT):
        c = ctx if k == "shared" else rep[0]
        _lib.check(lib.sd_sampler_prepare_draws(w, c.data_ptr(), ws[k].data_ptr(), B, T, Mc, B, what, 3, draws[k], st), "sd_sampler_prepare_draws")

    def evaluate(k):
        _lib.check(lib.sd_sampler_eps_draws(w, tokens.data_ptr(), x.data_ptr(), eps[k].data_ptr(), ws[k].data_ptr(), B, T, Mc, B, None, 3, draws[k], st),
                   "sd_sampler_eps_draws")

    expand()
    for k in ws:   # (also the warm-up)
        prepare(k, ops.PREPARE_WEIGHTS | ops.PREPARE_CONTEXT)
        evaluate(k)
    torch.cuda.synchronize()
    same = torch.equal(eps["shared"], eps["repeated"])
    prep = {k: [] for k in ws}
    ev = {k: [] for k in ws}
    kern = {k: [] for k in ws}
    exp, launches = [], {}
    for _ in range(blocks):
        exp.append(wall_ms(expand, reps))
        for k in ws:
            prep[k].append(wall_ms(lambda: prepare(k), reps))
        for k in ws:
            ev[k].append(wall_ms(lambda: evaluate(k), reps))
        for k in ws:
            ms, launches[k] = step_class_ms(lambda: evaluate(k))
            kern[k].append(ms)
    out = {"case": "loss_grid", "shape": name, "windows": Cn, "K": K, "trajectories": B, "T": T, "J": J, "d": d, "L": L, "Mc": Mc,
           "route": _lib.sampler_route_draws(d, 4, T, Mc, J, L, B, K), "bitwise_equal": same, "blocks": blocks, "reps": reps,
           "step_launches": launches, "expand_ms": summary(exp)}
    for k in ws:
        out[k] = {"prepare_context_ms": summary(prep[k]), "eps_ms": summary(ev[k]), "step_kernel_ms": summary(kern[k])}
    out["repeated"]["total_ms"] = statistics.median(exp) + statistics.median(prep["repeated"]) + statistics.median(ev["repeated"])
    out["shared"]["total_ms"] = statistics.median(prep["shared"]) + statistics.median(ev["shared"])
    out["spread_ms"] = {"prepare_context": spread(prep), "eps": spread(ev), "step_kernel": spread(kern), "expand": max(exp) - min(exp)}
    out["shared_over_repeated"] = {"prepare_context": statistics.median(prep["shared"]) / statistics.median(prep["repeated"]),
                                   "eps": statistics.median(ev["shared"]) / statistics.median(ev["repeated"]),
                                   "step_kernel": statistics.median(kern["shared"]) / statistics.median(kern["repeated"]),
                                   "total": out["shared"]["total_ms"] / out["repeated"]["total_ms"]}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="64 windows, two blocks")
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    blocks = 2 if args.quick else args.blocks
    lines = []
    for name, T in (("decoder_only.yaml", 10), ("benchmark", 100)):
        lines.append(bench_grid(name, 64 if args.quick else 512, 8, T, blocks, args.reps))
        print(json.dumps(lines[-1]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
