"""Gradient-norm clipping and the non-finite guard of the fused optimizer step, on the GPU: the two norm launches and the clip variants of
the AdamW (+ EMA) kernels by themselves on flat buffers, then the optimizer, the replayed graph, two virtual ranks and the command.

Sizes.  The norm's grid is fixed: W workgroups of 256 threads, a thread walks quads (four floats) with stride 256 W, so one full sweep is
1024 W floats.  n = 1, 3 (tail only), 4 (one quad), 255 (63 quads and a tail, one workgroup busy), 1024 W - 1 / 1024 W / 1024 W + 5 (one
short of a sweep, a sweep, a sweep and a quad and a tail) and 3 * 1024 W + 7 (several strides).

Bounds.  The reference (tests/clip_ref.py) and the kernel sum the same exact fp64 products in different orders: n 2^-53 relative apart at
most, 2e-10 at the largest n here, so the two fp32 norms are equal unless a rounding boundary lies between the sums - one fp32 ulp is
allowed, equality expected and the outcome printed.  Everything else is bit for bit: the coefficient against torch's expression evaluated
in fp32 from the kernel's OWN norm, two launches against each other, and the update against the existing kernels run on ``g * coef``."""

import functools
import math

import pytest
import torch

import clip_ref
from conftest import rel_err

pytestmark = pytest.mark.gpu
HYPER = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=1e-2)
SIZES = [(0, 1), (0, 3), (0, 4), (0, 255), (1, -1), (1, 0), (1, 5), (3, 7)]   # n = sweeps * 1024 W + extra


def _n(sweeps, extra):
    from soccerdiffusion_amd import ops

    return sweeps * 1024 * ops.grad_norm_workspace_doubles() + extra


@functools.lru_cache(maxsize=None)
def _gradient(n, mult=1.0):
    """(the gradient on the device, the reference's norm of it): ``randn * 1e-3``, times ``mult``; computed once per size and ``mult``,
    shared, never written."""
    g = torch.randn(n, generator=torch.Generator().manual_seed(n % 9973)) * 1e-3
    if mult != 1.0:
        g = g * mult
    return g.cuda(), clip_ref.norm_coef(g, math.inf)[0]


def _norm_buffers():
    from soccerdiffusion_amd import ops

    return (torch.zeros(ops.grad_norm_workspace_doubles(), dtype=torch.float64, device="cuda"), torch.full((2,), -7.0, device="cuda"),
            torch.zeros(1, dtype=torch.int32, device="cuda"))


def _half(norm) -> float:
    """Half a norm: exact in fp32, so the C float the library receives is this very number."""
    return float(norm) * 0.5


# ---- 1. the norm, the coefficient, determinism -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sweeps,extra,mult", [(s, e, 1.0) for s, e in SIZES] + [(1, 5, 1e20), (1, 5, 1e-25)])
def test_norm_and_coefficient(sweeps, extra, mult):
    """mult 1e20 / 1e-25: the sum of squares leaves fp32's range at the top / every square underflows it - an fp32 accumulator gives
    inf / 0, the fp64 one the norm (7e19 / 7e-26: ordinary fp32 numbers)."""
    from soccerdiffusion_amd import ops

    n = _n(sweeps, extra)
    g, want = _gradient(n, mult)
    assert math.isfinite(float(want)) and float(want) > 0.0
    if mult != 1.0:
        sq = float((g * g).sum())
        assert math.isinf(sq) if mult > 1 else sq == 0.0   # what an fp32 sum of fp32 squares makes of this gradient
    max_norm = _half(want)
    ws, clip, skipped = _norm_buffers()
    ops.grad_norm(g, ws, clip, skipped, max_norm)
    got = clip.cpu()
    ulp = float(torch.nextafter(want, torch.tensor(math.inf)) - want)
    print(f"n {n} x {mult:g}: norm {float(got[0]):.9g}, reference {float(want):.9g}, {'equal' if got[0] == want else 'ONE ULP APART'}; "
          f"coef {float(got[1]):.9g}")
    assert abs(float(got[0]) - float(want)) <= ulp
    assert got[1] == clip_ref.coef_from_norm(got[0], max_norm) and float(got[1]) < 1.0
    assert int(skipped) == 0
    # a second launch, other buffers: the same bits, partial by partial
    ws2, clip2, skipped2 = _norm_buffers()
    ops.grad_norm(g, ws2, clip2, skipped2, max_norm)
    assert torch.equal(clip2, clip) and torch.equal(ws2, ws) and int(skipped2) == 0
    # a bound that does not bind: coef = 1 exactly (a norm near torch's 1e-6 or below it is scaled by that 1e-6 whatever the bound)
    ops.grad_norm(g, ws2, clip2, skipped2, 2.0 * float(want))
    assert clip2[1].cpu() == clip_ref.coef_from_norm(got[0], 2.0 * float(want)) and clip2[0] == clip[0]
    assert float(clip2[1]) == 1.0 or float(want) < 1e-5
    ops.grad_norm(g, ws2, clip2, skipped2, math.inf)
    assert float(clip2[1]) == 1.0 and clip2[0] == clip[0] and int(skipped2) == 0


@pytest.mark.parametrize("sweeps,extra", [(0, 255), (1, 5)])
def test_norm_does_not_depend_on_alignment(sweeps, extra):
    """The same values 4 bytes off a 16-byte boundary take dword loads: the same elements in the same order, the same partials."""
    from soccerdiffusion_amd import ops

    n = _n(sweeps, extra)
    g, want = _gradient(n)
    shifted = torch.zeros(n + 4, device="cuda")[1:n + 1]
    shifted.copy_(g)
    assert g.data_ptr() % 16 == 0 and shifted.data_ptr() % 16 == 4
    (ws, clip, skipped), (ws2, clip2, skipped2) = _norm_buffers(), _norm_buffers()
    ops.grad_norm(g, ws, clip, skipped, _half(want))
    ops.grad_norm(shifted, ws2, clip2, skipped2, _half(want))
    assert torch.equal(ws, ws2) and torch.equal(clip, clip2)


def test_all_zero_gradient():
    from soccerdiffusion_amd import ops

    ws, clip, skipped = _norm_buffers()
    ops.grad_norm(torch.zeros(1029, device="cuda"), ws, clip, skipped, 1.0)
    assert clip.tolist() == [0.0, 1.0] and int(skipped) == 0


# ---- 2. the update -------------------------------------------------------------------------------------------------------------------------
def _state(n, seed):
    g = torch.Generator().manual_seed(seed)
    p = torch.randn(n, generator=g).cuda()
    return {"p": p, "m": (torch.randn(n, generator=g) * 1e-3).cuda(), "v": (torch.rand(n, generator=g) * 1e-6).cuda(),
            "ema": (p * (0.5 + torch.rand(n, generator=g).cuda()))}


def _clone(st):
    return {k: t.clone() for k, t in st.items()}


def _same(a, b, keys="pmv"):
    names = {"p": "p", "m": "m", "v": "v", "e": "ema"}
    return all(torch.equal(a[names[k]], b[names[k]]) for k in keys)


def _existing_step(st, grad, ema, dev_form, step, w):
    """The kernels that were there before, on ``grad``."""
    from soccerdiffusion_amd import ops

    hyper = torch.zeros(7).pin_memory()
    ops.adamw_hyper(*HYPER.values(), step, hyper)
    if dev_form and ema:
        ops.adamw_ema_step_dev(st["p"], grad, st["m"], st["v"], st["ema"], hyper.cuda(), torch.tensor([w], dtype=torch.float32).cuda())
    elif dev_form:
        ops.adamw_step_dev(st["p"], grad, st["m"], st["v"], hyper.cuda())
    elif ema:
        ops.adamw_ema_step(st["p"], grad, st["m"], st["v"], st["ema"], *HYPER.values(), step, w)
    else:
        ops.adamw_step(st["p"], grad, st["m"], st["v"], *HYPER.values(), step)


def _clip_step(st, grad, clip, ema, dev_form, step, w):
    from soccerdiffusion_amd import ops

    e = st["ema"] if ema else None
    if dev_form:
        hyper = torch.zeros(7).pin_memory()
        ops.adamw_hyper(*HYPER.values(), step, hyper)
        ops.adamw_clip_step_dev(st["p"], grad, st["m"], st["v"], e, clip, hyper.cuda(), torch.tensor([w], dtype=torch.float32).cuda() if ema else None)
    else:
        ops.adamw_clip_step(st["p"], grad, st["m"], st["v"], e, clip, *HYPER.values(), step, w if ema else 0.0)


@pytest.mark.parametrize("sweeps,extra", [(0, 3), (0, 255), (1, 5)])
@pytest.mark.parametrize("ema", [False, True])
@pytest.mark.parametrize("dev_form", [False, True])
def test_update_equals_the_existing_kernels_on_the_clipped_gradient(sweeps, extra, ema, dev_form):
    from soccerdiffusion_amd import ops

    n = _n(sweeps, extra)
    g, want = _gradient(n)
    held = g.clone()
    st = _state(n, seed=n + 1)
    twin = _clone(st)
    ws, clip, skipped = _norm_buffers()
    for step, w in ((1, 0.9), (2, 0.37)):
        ops.grad_norm(g, ws, clip, skipped, _half(want))
        coef = float(clip[1])            # read back; the product below rounds once, on the device
        assert coef < 1.0
        _clip_step(st, g, clip, ema, dev_form, step, w)
        _existing_step(twin, g * coef, ema, dev_form, step, w)
        assert _same(st, twin, "pmve" if ema else "pmv"), step
        assert torch.equal(g, held) and (ema or torch.equal(st["ema"], twin["ema"]))   # the gradient is read only; no EMA, no write
    assert int(skipped) == 0


@pytest.mark.parametrize("ema", [False, True])
@pytest.mark.parametrize("dev_form", [False, True])
def test_max_norm_inf_is_the_existing_step(ema, dev_form):
    from soccerdiffusion_amd import ops

    n = _n(1, 5)
    g, _ = _gradient(n)
    st = _state(n, seed=3)
    twin = _clone(st)
    ws, clip, skipped = _norm_buffers()
    ops.grad_norm(g, ws, clip, skipped, math.inf)
    assert float(clip[1]) == 1.0
    _clip_step(st, g, clip, ema, dev_form, 1, 0.25)
    _existing_step(twin, g, ema, dev_form, 1, 0.25)
    assert _same(st, twin, "pmve")


def test_update_against_the_reference_adamw():
    """The CPU definition (clip_ref.clipped_adamw: torch's single-tensor AdamW on g * coef) within the bound tests/test_gpu_train_ops.py holds
    the unclipped kernel to against torch.optim.AdamW."""
    from soccerdiffusion_amd import ops

    n = _n(0, 255)
    g, want = _gradient(n)
    st = _state(n, seed=11)
    ref = {k: t.cpu() for k, t in st.items()}
    ws, clip, skipped = _norm_buffers()
    for step in (1, 2, 3):
        ops.grad_norm(g, ws, clip, skipped, _half(want))
        _clip_step(st, g, clip, False, False, step, 0.0)
        _, coef, ok = clip_ref.clipped_adamw(ref["p"], g, ref["m"], ref["v"], _half(want), step=step, **HYPER)
        assert ok and float(coef) < 1.0
    assert rel_err(st["p"], ref["p"]) < 1e-6 and rel_err(st["m"], ref["m"]) < 1e-6 and rel_err(st["v"], ref["v"]) < 1e-6


# ---- 3. the guard --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where,value", [("first", math.nan), ("last", math.inf)])
@pytest.mark.parametrize("ema,dev_form", [(True, False), (False, True), (True, True)])
def test_a_gradient_that_is_not_finite_skips_the_step(where, value, ema, dev_form):
    """NaN in element 0 (the first quad of thread 0); +inf in element n - 1, which belongs to the tail thread."""
    from soccerdiffusion_amd import ops

    n = _n(1, 5)
    assert n % 4 != 0
    good, want = _gradient(n)
    bad = good.clone()
    bad[0 if where == "first" else n - 1] = value
    st = _state(n, seed=5)
    before, twin = _clone(st), _clone(st)
    ws, clip, skipped = _norm_buffers()
    ops.grad_norm(bad, ws, clip, skipped, _half(want))
    _clip_step(st, bad, clip, ema, dev_form, 1, 0.9)
    assert not math.isfinite(float(clip[0])) and float(clip[1]) == 0.0 and int(skipped) == 1
    assert _same(st, before, "pmve")
    # the next, finite, step updates as ever (its number is 2: the skipped step used up number 1)
    ops.grad_norm(good, ws, clip, skipped, _half(want))
    _clip_step(st, good, clip, ema, dev_form, 2, 0.37)
    _existing_step(twin, good * float(clip[1]), ema, dev_form, 2, 0.37)
    assert int(skipped) == 1 and 0.0 < float(clip[1]) < 1.0
    assert _same(st, twin, "pmve" if ema else "pmv") and not torch.equal(st["p"], before["p"])


# ---- 4. the optimizer, the replayed graph ----------------------------------------------------------------------------------------------------
def _setup(max_grad_norm, ema_decay=0.9):
    """tests/test_gpu_ema.py's tiny decoder-pretraining set-up.  One forward and backward without an update first: they change no weight
    and no optimizer state (every step zeroes the gradient buffer first), and a capture that follows finds nothing left to initialise."""
    from soccerdiffusion_amd import training
    from test_gpu_ema import _fixed_draws, _train_setup

    m, opt, ns, x0, ctx = _train_setup(ema_decay=ema_decay, max_grad_norm=max_grad_norm)
    noise, t = _fixed_draws(0)
    training.mse_loss(m.forward_with_context(ctx, ns.add_noise(x0, noise, t), t), noise).backward()
    torch.cuda.synchronize()
    sch = torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=1e-3, total_steps=20)
    return m, opt, sch, ns, x0, ctx, torch.Generator(device="cuda").manual_seed(11)


@functools.lru_cache(maxsize=None)
def _first_step_norm() -> float:
    """The unclipped gradient norm of step one of the tiny decoder-pretraining set-up (guard only: max_grad_norm = inf)."""
    from soccerdiffusion_amd import training

    m, opt, sch, ns, x0, ctx, gen = _setup(math.inf)
    training.train_step(m, opt, sch, ns, x0, context=ctx, generator=gen)
    st = opt.grad_stats()
    assert st["coef"] == 1.0 and st["skipped_steps"] == 0 and math.isfinite(st["norm"]) and st["norm"] > 0.0
    return st["norm"]


def _buffers(opt):
    return {"p": opt.flat_param.clone(), "m": opt.flat_m.clone(), "v": opt.flat_v.clone(), "ema": opt.flat_ema.clone()}


def test_optimizer_without_max_grad_norm_allocates_nothing():
    m, opt, *_ = _setup(None)
    assert opt.max_grad_norm is None and opt._clip is None and opt._skipped is None and opt._gn_partials is None
    with pytest.raises(RuntimeError, match="max_grad_norm"):
        opt.grad_stats()


def test_eager_steps_clip_and_the_graph_replays_them_bit_for_bit():
    from soccerdiffusion_amd import training

    max_norm = 0.5 * _first_step_norm()
    m, opt, sch, ns, x0, ctx, gen = _setup(max_norm)
    stats = []
    for _ in range(3):
        training.train_step(m, opt, sch, ns, x0, context=ctx, generator=gen)
        stats.append(opt.grad_stats())
    print("eager:", stats)
    assert stats[0]["norm"] == _first_step_norm() and stats[0]["coef"] < 1.0
    assert stats[0]["coef"] == float(clip_ref.coef_from_norm(torch.tensor(stats[0]["norm"], dtype=torch.float32), max_norm))
    assert all(s["skipped_steps"] == 0 for s in stats) and opt._step == 3 and opt.ema_updates == 3
    eager = _buffers(opt)

    # unclipped, the same three steps end elsewhere: the coefficient did something
    mu, optu, schu, *_ , genu = _setup(None)
    for _ in range(3):
        training.train_step(mu, optu, schu, ns, x0, context=ctx, generator=genu)
    assert not torch.equal(optu.flat_param, eager["p"])

    m2, opt2, sch2, _, _, _, gen2 = _setup(max_norm)
    gs = training.GraphedTrainStep(m2, opt2, sch2, ns, generator=gen2, eager_steps=0)
    try:
        replayed = []
        for _ in range(3):
            gs(x0, context=ctx)
            assert gs.graph is not None
            replayed.append(opt2.grad_stats())
    finally:
        gs.close()
    print("replayed:", replayed)
    assert replayed == stats
    assert _same(_buffers(opt2), eager, "pmve") and opt2._step == 3 and opt2.ema_updates == 3


@pytest.mark.parametrize("graphed", [False, True])
def test_one_inf_in_the_targets_skips_the_step(graphed):
    from soccerdiffusion_amd import training

    m, opt, sch, ns, x0, ctx, gen = _setup(0.5 * _first_step_norm())
    gs = training.GraphedTrainStep(m, opt, sch, ns, generator=gen, eager_steps=0) if graphed else None

    def step(targets):
        if graphed:
            return gs(targets, context=ctx)
        return training.train_step(m, opt, sch, ns, targets, context=ctx, generator=gen)

    try:
        step(x0)
        assert gs is None or gs.graph is not None   # graphed: captured by the first call, every step below is a replay
        before = _buffers(opt)
        bad = x0.clone()
        bad[1, 3, 2] = math.inf
        step(bad)
        st = opt.grad_stats()
        assert st["skipped_steps"] == 1 and st["coef"] == 0.0 and not math.isfinite(st["norm"])
        assert _same(_buffers(opt), before, "pmve")
        assert opt._step == 2 and opt.ema_updates == 2   # the host is not told: the skipped step used up its number
        step(x0)
        st = opt.grad_stats()
        assert st["skipped_steps"] == 1 and math.isfinite(st["norm"]) and 0.0 < st["coef"] <= 1.0
        after = _buffers(opt)
        assert all(torch.isfinite(t).all() for t in after.values()) and not torch.equal(after["p"], before["p"])
    finally:
        if gs is not None:
            gs.close()


# ---- 5. data parallel ------------------------------------------------------------------------------------------------------------------------
def test_two_virtual_ranks_equal_one_full_batch_clipped_step():
    """tests/test_gpu_dp.py's recipe and tolerances with a clip that binds: the norm is taken on the averaged gradient, inside step()."""
    from soccerdiffusion_amd import training
    from soccerdiffusion_amd.scheduler import DDIMScheduler
    from test_gpu_dp import _model

    B, T, J, d = 16, 100, 20, 256
    g = torch.Generator(device="cuda").manual_seed(3)
    x0 = torch.randn(B, T, J, device="cuda", generator=g)
    ctx = torch.randn(B, 10, d, device="cuda", generator=g)
    noise = torch.randn(B, T, J, device="cuda", generator=g)
    t = torch.randint(0, 1000, (B,), device="cuda", generator=g)
    ns = DDIMScheduler(beta_schedule="squaredcos_cap_v2", clip_sample=False)

    probe = _model()
    opt_p = training.FusedAdamW(probe.parameters(), lr=1e-3, max_grad_norm=math.inf)
    training.train_step(probe, opt_p, None, ns, x0, context=[ctx], noise=noise, timesteps=t)
    max_norm = 0.5 * opt_p.grad_stats()["norm"]

    full = _model()
    opt_f = training.FusedAdamW(full.parameters(), lr=1e-3, max_grad_norm=max_norm)
    training.train_step(full, opt_f, None, ns, x0, context=[ctx], noise=noise, timesteps=t)
    grad_f = opt_f.flat_grad.clone()

    dp = _model()
    opt_d = training.FusedAdamW(dp.parameters(), lr=1e-3, max_grad_norm=max_norm)
    halves = []
    for r in range(2):   # what rank r computes before the all-reduce
        sl = slice(r * B // 2, (r + 1) * B // 2)
        opt_d.zero_grad()
        noisy = ns.add_noise(x0[sl], noise[sl], t[sl])
        training.mse_loss(dp.forward_with_context([ctx[sl]], noisy, t[sl]), noise[sl]).backward()
        halves.append(opt_d.flat_grad.clone())
    opt_d.flat_grad.copy_((halves[0] + halves[1]) * 0.5)   # all-reduce(SUM) then 1 / world
    opt_d.step()

    sf, sd = opt_f.grad_stats(), opt_d.grad_stats()
    print("full batch:", sf, "two ranks:", sd)
    assert sf["coef"] < 1.0 and sd["coef"] < 1.0 and sf["skipped_steps"] == sd["skipped_steps"] == 0
    assert abs(sd["norm"] - sf["norm"]) < 2e-5 * sf["norm"]
    rel = float((opt_d.flat_grad - grad_f).norm() / grad_f.norm())
    assert rel < 2e-5, rel
    relp = float((opt_d.flat_param - opt_f.flat_param).norm() / opt_f.flat_param.norm())
    assert relp < 1e-6, relp
    assert not torch.equal(opt_f.flat_param, opt_p.flat_param)


# ---- 6. the command ------------------------------------------------------------------------------------------------------------------------
def _train(*argv) -> str:
    """``cli train`` in this process (the command's own code from the parser on, without a second interpreter start): what it printed."""
    import contextlib
    import io

    from soccerdiffusion_amd import cli

    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        assert cli.main(["train", *argv]) == 0
    return out.getvalue()


@pytest.fixture(scope="module")
def clipped_run(tmp_path_factory):
    """One short epoch (three steps) of ``train --synthetic 96 --clip-grad-norm 0.5``, shared by the tests below."""
    import yaml
    from test_gpu_ema import CFG

    d = tmp_path_factory.mktemp("clip_cli")
    cfg = d / "cfg.yaml"
    cfg.write_text(yaml.safe_dump(CFG))
    ckpt = d / "clip.pth"
    printed = _train("-c", str(cfg), "-o", str(ckpt), "--synthetic", "96", "--clip-grad-norm", "0.5")
    return d, str(cfg), str(ckpt), printed


def test_cli_train_prints_and_saves_the_clip_state(clipped_run):
    from test_gpu_ema import OLD_KEYS

    _, _, ckpt, printed = clipped_run
    line = next(ln for ln in printed.splitlines() if ln.startswith("Epoch 0, it 0"))
    assert "GradNorm: " in line and line.endswith("Skipped: 0"), line
    assert math.isfinite(float(line.split("GradNorm: ")[1].split(",")[0]))
    back = torch.load(ckpt, weights_only=True)
    assert set(back) == OLD_KEYS | {"grad_clip"} and back["grad_clip"] == {"max_norm": 0.5, "skipped_steps": 0}


def test_cli_train_without_the_flag_is_unchanged(clipped_run):
    from test_gpu_ema import OLD_KEYS

    d, cfg, _, _ = clipped_run
    printed = _train("-c", cfg, "-o", str(d / "plain.pth"), "--synthetic", "96")
    assert "Epoch 0, it 0, Loss: " in printed and "GradNorm" not in printed and "Skipped" not in printed
    assert set(torch.load(d / "plain.pth", weights_only=True)) == OLD_KEYS


def test_cli_resume_carries_the_norm_and_the_count_on(clipped_run):
    d, cfg, ckpt, _ = clipped_run
    back = torch.load(ckpt, weights_only=True)
    back["grad_clip"]["skipped_steps"] = 4   # as if four steps had been skipped
    torch.save(back, d / "four.pth")
    printed = _train("-c", cfg, "-p", str(d / "four.pth"), "-o", str(d / "resumed.pth"), "--synthetic", "96")   # no flag: the checkpoint's
    assert "Skipped: 4" in printed
    assert torch.load(d / "resumed.pth", weights_only=True)["grad_clip"] == {"max_norm": 0.5, "skipped_steps": 4}
