"""The rollout kernel (csrc/sd_traj.h, `traj_step_rollout_kernel<NTT, PRECISE>`: every DDIM step of a trajectory in one launch) against
the per-step kernels it loops over.  The arithmetic of a step is the same code, so the two rollout forms must agree bit for bit: any
difference is a bug (a stale x between steps, a step block or a coefficient of the wrong step, a chunk boundary).

The switch that forces the per-step form (SD_TRAJ_ROLLOUT=steps) is read once per process, so the per-step side of every case is computed
by ONE child process that runs this file; the launches of each call are counted with the library's profiler (sd_profile_*), which shows
that the form the plan announces is the form that ran.  d = 256, 4 heads, L = 2, J = 20, synthetic weights, seeded inputs."""

import ctypes as C
import os
import subprocess
import sys
import tempfile

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D, HEADS, L, J = 256, 4, 2, 20
CAP = 64   # steps per launch (TRAJ_ROLLOUT_MAX_STEPS, csrc/sd_traj_host.h)

# name -> (T, B, Mc, n_steps, max_mode, kind); kind: plain | trace | eps | pin
CASES = {}
for T in (1, 16, 17, 100):          # one token; a full tile; a tile and one token; seven tiles, the last with four tokens
    for Mc in (10, 0):
        for mode in (3, 4):
            CASES[f"T{T}-Mc{Mc}-m{mode}"] = (T, 3, Mc, 3, mode, "plain")
CASES["chunk"] = (16, 2, 10, CAP + 1, 3, "plain")     # two launches: CAP steps and one
CASES["B1"] = (17, 1, 10, 3, 3, "plain")
CASES["B5"] = (17, 5, 10, 3, 3, "plain")
CASES["trace"] = (17, 3, 10, 3, 3, "trace")
CASES["eps"] = (17, 3, 10, 3, 3, "eps")
CASES["pin"] = (17, 3, 10, 3, 3, "pin")
PLAIN = [k for k, v in CASES.items() if v[5] == "plain"]


def _inputs(name):
    T, B, Mc, n_steps, mode, kind = CASES[name]
    g = torch.Generator().manual_seed(9100 + sorted(CASES).index(name))
    return torch.randn(B, T, J, generator=g), torch.randn(B, Mc, D, generator=g), torch.randn(B, T, J, generator=g)


def run_cases(names):
    """name -> {x0, status, launches (of the traj_step_kernel class), out (the per-step trace where the kind has one)} on the current device,
    in the rollout form this process's environment selects."""
    from oracle import ddim_ref
    from oracle import denoiser_ref as ref
    from soccerdiffusion_amd import _lib, ops

    lib = _lib.load()
    sd = ref.synthetic_state_dict(D, J, L, seed=33)
    packed = ops.pack_denoiser(sd, "cuda", heads=HEADS, max_len=100)
    acp = ddim_ref.alphas_cumprod()
    ncls = len(_lib.KERNEL_CLASSES)
    res = {}
    for name in names:
        T, B, Mc, n_steps, mode, kind = CASES[name]
        x_T, ctx, known = _inputs(name)
        ts = ddim_ref.timesteps(n_steps).tolist()
        toks = ops.step_token(torch.tensor(ts).cuda(), ops.step_frequencies(D).cuda(), sd["step_encoding.token"].cuda()).reshape(n_steps, D)
        coef = ops.ddim_coefficients(ts, acp, n_steps)
        status = torch.zeros(1, dtype=torch.int32, device="cuda")
        kw = {"trace": {"trace": True}, "eps": {"eps_trace": True}, "pin": {"pin": (known.cuda(), torch.tensor([0, 5, T], dtype=torch.int32))}}.get(kind, {})
        torch.cuda.synchronize()
        lib.sd_profile_enable(1)
        try:
            out = ops.ddim_sample(packed, ctx.cuda(), toks, coef, x_T.cuda(), status=status, max_mode=mode, **kw)
            torch.cuda.synchronize()
        finally:
            lib.sd_profile_enable(0)
        ms, cnt = (C.c_double * ncls)(), (C.c_long * ncls)()
        _lib.check(lib.sd_profile_collect(ms, cnt, ncls), "sd_profile_collect")
        x0, extra = (out[0], out[1]) if isinstance(out, tuple) else (out, None)
        res[name] = {"x0": x0.cpu(), "status": int(status.item()), "launches": int(cnt[_lib.KERNEL_CLASSES.index("traj_step_kernel")]),
                     "out": None if extra is None else torch.stack([t.cpu() for t in extra])}
    return res


if __name__ == "__main__":   # the child: every case in the form its environment selects -> argv[1]
    sys.path.insert(0, REPO)
    torch.save(run_cases(list(CASES)), sys.argv[1])
    sys.exit(0)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fused():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    assert "SD_TRAJ_ROLLOUT" not in os.environ
    return run_cases(list(CASES))


@pytest.fixture(scope="module")
def per_step():
    env = {k: v for k, v in os.environ.items() if not k.startswith("SD_")}
    env.update(SD_TRAJ_ROLLOUT="steps", PYTHONPATH=REPO)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "per_step.pt")
        subprocess.run([sys.executable, os.path.abspath(__file__), path], env=env, check=True, cwd=REPO)
        return torch.load(path, map_location="cpu", weights_only=True)


def _same(a, b):
    return torch.equal(a["x0"], b["x0"]) and a["status"] == b["status"] and bool(torch.isfinite(a["x0"]).all())


def test_the_announced_form_is_the_form_that_ran(fused, per_step):
    from soccerdiffusion_amd import _lib

    for name, (T, B, Mc, n_steps, mode, kind) in CASES.items():
        form = _lib.sampler_rollout(D, HEADS, T, Mc, J, L, B, mode, trace=kind in ("trace", "eps"), pin=kind == "pin")
        assert form == ("FUSED" if kind == "plain" else "PER_STEP"), name
        assert fused[name]["launches"] == ((n_steps + CAP - 1) // CAP if kind == "plain" else n_steps), name
        assert per_step[name]["launches"] == n_steps, name


@pytest.mark.parametrize("name", [k for k in PLAIN if k.startswith("T")])
def test_fused_equals_per_step_bit_for_bit(fused, per_step, name):
    assert _same(fused[name], per_step[name])


def test_chunk_boundary(fused, per_step):
    assert CASES["chunk"][3] == CAP + 1 and fused["chunk"]["launches"] == 2
    assert _same(fused["chunk"], per_step["chunk"])


@pytest.mark.parametrize("name", ["B1", "B5"])
def test_one_trajectory_and_five(fused, per_step, name):
    assert _same(fused[name], per_step[name])


def test_fused_rollout_is_repeatable(fused):
    again = run_cases(["T100-Mc10-m3", "T17-Mc0-m4"])
    for name, r in again.items():
        assert r["launches"] == 1 and _same(r, fused[name]), name


def test_fused_rollout_against_the_fp64_oracle_loop():
    """The bar of tests/test_gpu_mode3_bitwise.py on the sample a fused rollout returns: T = 100, B = 2, 3 steps."""
    from oracle import ddim_ref
    from oracle import denoiser_ref as ref
    from soccerdiffusion_amd import _lib, ops

    T, B, Mc, n_steps = 100, 2, 10, 3
    assert _lib.sampler_rollout(D, HEADS, T, Mc, J, L, B, 3) == "FUSED"
    sd = ref.synthetic_state_dict(D, J, L, seed=33)
    g = torch.Generator().manual_seed(9099)
    x_T, ctx = torch.randn(B, T, J, generator=g), torch.randn(B, Mc, D, generator=g)
    acp = ddim_ref.alphas_cumprod()
    ts = ddim_ref.timesteps(n_steps).tolist()

    def denoise(dtype):
        return lambda x, t: ref.forward_with_context(sd, [ctx], x, torch.full((B,), t, dtype=torch.int64), dtype=dtype)

    packed = ops.pack_denoiser(sd, "cuda", heads=HEADS, max_len=T)
    toks = ops.step_token(torch.tensor(ts).cuda(), ops.step_frequencies(D).cuda(), sd["step_encoding.token"].cuda()).reshape(n_steps, D)
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    x0 = ops.ddim_sample(packed, ctx.cuda(), toks, ops.ddim_coefficients(ts, acp, n_steps), x_T.cuda(), status=status, max_mode=3).cpu()
    assert int(status.item()) == 0
    want64 = ddim_ref.sample(denoise(torch.float64), x_T.double(), n_steps, acp)[-1]
    want32 = ddim_ref.sample(denoise(torch.float32), x_T, n_steps, acp)[-1]
    e = float((x0.double() - want64).norm() / want64.norm())
    e_cpu32 = float((want32.double() - want64).norm() / want64.norm())
    print(f"fused rollout: e {e:.3e} e_cpu32 {e_cpu32:.3e}")
    assert e < 4 * e_cpu32 + 1e-7, (e, e_cpu32)


@pytest.mark.parametrize("name", ["trace", "eps", "pin"])
def test_calls_that_stay_per_step(fused, per_step, name):
    """A call that returns something per step, or pins rows, runs the per-step kernels whatever the switch says: the same launches, the
    same bytes."""
    a, b = fused[name], per_step[name]
    assert a["launches"] == b["launches"] == CASES[name][3]
    assert _same(a, b)
    if a["out"] is not None:
        assert torch.equal(a["out"], b["out"])
    if name == "trace":   # ... and the sample of the fused form of the same inputs is the last row of the trace
        assert torch.equal(a["out"][-1], a["x0"])
