"""Weight EMA inside the fused AdamW step, layer by layer on the GPU: the kernel against its definition, the optimizer, the replayed graph,
``ema_weights()``, resume, the commands and the data-parallel helpers.

The bound on the average.  One update computes ``fma(w, p - e, e)``: the subtraction rounds once, the fma once, each by at most half an
ulp of a number no larger than 2 max(|p|, |e|) weighted by w <= 1, respectively than max(|p|, |e|) - about 2^-23 max(|p|, |e|) together -
and an earlier error is carried on with the factor 1 - w <= 1.  After K updates: ``|ema - ref| <= K 2^-23 max(|p|, |ema|)``, where ref is
the fp64 recurrence over the kernel's OWN fp32 parameters and fp32 weights, and the magnitude is the largest either took on the way."""

import ctypes
import functools
import os
import socket
import subprocess
import sys

import pytest
import torch
import yaml

from conftest import REPO
from test_gpu_loop_form import _model

pytestmark = pytest.mark.gpu
ULP = 2.0 ** -23
HYPER = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=1e-2)


class Recurrence:
    """ema_ref (fp64) and the largest magnitude seen, driven by recorded fp32 parameters."""

    def __init__(self, ema0, p0=None):
        self.ref = ema0.double().clone()
        self.mag = self.ref.abs() if p0 is None else torch.maximum(self.ref.abs(), p0.double().abs())
        self.k = 0

    def update(self, p, w):
        w32 = float(torch.tensor(w, dtype=torch.float32))   # what the kernel multiplies with
        self.ref += w32 * (p.double() - self.ref)
        self.mag = torch.maximum(self.mag, torch.maximum(p.double().abs(), self.ref.abs()))
        self.k += 1

    def check(self, ema):
        err = (ema.double() - self.ref).abs()
        bound = self.k * ULP * torch.maximum(self.mag, ema.double().abs())
        worst = float((err - bound).max())
        print(f"ema after {self.k} updates: max err {float(err.max()):.3e}, max err/bound {float((err / bound.clamp_min(1e-300)).max()):.3f}")
        assert worst <= 0.0, worst


# ---- 1. the kernel against its definition ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,offset", [(4099, 0), (64, 0), (4099, 1)])
@pytest.mark.parametrize("dev_form", [False, True])
def test_kernel_against_its_definition(n, offset, dev_form):
    """n = 4099: the 16-byte body plus a 3-element tail over several workgroups; 64: less than one workgroup; offset 1: every buffer but
    the EMA starts 16-byte aligned and the EMA 4 bytes behind, which takes the element-by-element path."""
    from soccerdiffusion_amd import ops

    g = torch.Generator().manual_seed(n + offset)
    p = torch.randn(n, generator=g).cuda()
    m, v = torch.zeros(n).cuda(), torch.zeros(n).cuda()
    ema = torch.zeros(n + 4).cuda()[offset:offset + n]
    ema.copy_(p * (0.5 + torch.rand(n, generator=g).cuda()))
    assert (ema.data_ptr() % 16 == 0) == (offset == 0) and p.data_ptr() % 16 == 0
    p2, m2, v2 = p.clone(), m.clone(), v.clone()
    rec = Recurrence(ema, p)
    hyper, word = torch.zeros(7).pin_memory(), torch.zeros(1).cuda()
    for step, w in enumerate((0.9, 0.37, 1e-4, 0.6180339, 0.05), start=1):
        grad = torch.randn(n, generator=g).cuda()
        if dev_form:
            ops.adamw_hyper(HYPER["lr"], HYPER["beta1"], HYPER["beta2"], HYPER["eps"], HYPER["weight_decay"], step, hyper)
            h = hyper.cuda()
            word.fill_(w)
            ops.adamw_ema_step_dev(p, grad, m, v, ema, h, word)
            ops.adamw_step_dev(p2, grad, m2, v2, h)
        else:
            ops.adamw_ema_step(p, grad, m, v, ema, HYPER["lr"], HYPER["beta1"], HYPER["beta2"], HYPER["eps"], HYPER["weight_decay"], step, w)
            ops.adamw_step(p2, grad, m2, v2, HYPER["lr"], HYPER["beta1"], HYPER["beta2"], HYPER["eps"], HYPER["weight_decay"], step)
        assert torch.equal(p, p2) and torch.equal(m, m2) and torch.equal(v, v2), step   # the update itself did not change
        rec.update(p, w)
        rec.check(ema)


# ---- shared small training set-up ----------------------------------------------------------------------------------------------------
D, L, T, J, MC, B = 128, 1, 10, 4, 3, 2


def _train_setup(d=D, T=T, J=J, mc=MC, ema_decay=0.9, seed=5, **kw):
    from soccerdiffusion_amd import training
    from soccerdiffusion_amd.scheduler import DDIMScheduler

    m, _ = _model(d, J, L, T, seed=seed)
    m.train().set_dropout(0.0)
    opt = training.FusedAdamW(m.parameters(), lr=1e-3, ema_decay=ema_decay, **kw)
    g = torch.Generator().manual_seed(17)
    x0 = torch.randn(B, T, J, generator=g).cuda()
    ctx = [torch.randn(B, mc, d, generator=g).cuda()]
    ns = DDIMScheduler(beta_schedule="squaredcos_cap_v2", clip_sample=False)
    return m, opt, ns, x0, ctx


def _fixed_draws(k):
    g = torch.Generator().manual_seed(100 + k)
    return torch.randn(B, T, J, generator=g).cuda(), torch.randint(0, 1000, (B,), generator=g).cuda()


def _steps(m, opt, ns, x0, ctx, first, count, rec=None):
    from soccerdiffusion_amd import training

    for k in range(first, first + count):
        noise, t = _fixed_draws(k)
        w = opt.ema_weight_for_step(opt.ema_updates) if opt.flat_ema is not None else None
        training.train_step(m, opt, None, ns, x0, context=ctx, noise=noise, timesteps=t)
        if rec is not None:
            rec.update(opt.flat_param, w)


# ---- 2. the optimizer ----------------------------------------------------------------------------------------------------------------
def test_optimizer_keeps_the_average_and_leaves_the_update_alone():
    m, opt, ns, x0, ctx = _train_setup()
    assert torch.equal(opt.flat_ema, opt.flat_param)
    rec = Recurrence(opt.flat_ema, opt.flat_param)
    _steps(m, opt, ns, x0, ctx, 0, 6, rec)
    assert opt.ema_updates == 6 and opt._step == 6
    rec.check(opt.flat_ema)
    assert not torch.equal(opt.flat_ema, opt.flat_param)

    twin, topt, *_ = _train_setup(ema_decay=None)
    assert topt.flat_ema is None
    _steps(twin, topt, ns, x0, ctx, 0, 6)
    # same seeds, same draws, the same update expressions: the twin without an average holds the same bits
    assert torch.equal(opt.flat_param, topt.flat_param) and torch.equal(opt.flat_m, topt.flat_m) and torch.equal(opt.flat_v, topt.flat_v)

    m.mean.fill_(3.0)
    sd = opt.ema_state_dict(m)
    assert set(sd) == set(m.state_dict())
    at = 0
    named = dict(m.named_parameters())
    for p in opt.param_groups[0]["params"]:
        name = next(k for k, q in named.items() if q is p)
        assert torch.equal(sd[name], opt.flat_ema[at:at + p.numel()].view(p.shape)), name
        at += p.numel()
    assert at == opt.flat_ema.numel()
    assert sd["mean"].data_ptr() == m.mean.data_ptr() and sd["std"].data_ptr() == m.std.data_ptr() and float(sd["mean"][0]) == 3.0
    assert opt.state_dict()["state"][0].keys() == {"step", "exp_avg", "exp_avg_sq"}


# ---- 3. the replayed graph -----------------------------------------------------------------------------------------------------------
def _graph_nodes(graph) -> int:
    hip = ctypes.CDLL("libamdhip64.so.7")
    hip.hipGraphGetNodes.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_size_t)]
    hip.hipGraphGetNodes.restype = ctypes.c_int
    n = ctypes.c_size_t(0)
    assert hip.hipGraphGetNodes(ctypes.c_void_p(graph.raw_cuda_graph()), None, ctypes.byref(n)) == 0
    return n.value


def _graphed_run(ema_decay, monkeypatch, rec_wanted):
    from soccerdiffusion_amd import training

    m, opt, ns, x0, ctx = _train_setup(ema_decay=ema_decay)
    sch = torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=1e-3, total_steps=20)
    gen = torch.Generator(device="cuda").manual_seed(11)
    monkeypatch.setattr(torch.cuda, "CUDAGraph", functools.partial(torch.cuda.CUDAGraph, keep_graph=True))   # the graph stays queryable
    gs = training.GraphedTrainStep(m, opt, sch, ns, generator=gen, eager_steps=2)
    rec = Recurrence(opt.flat_ema, opt.flat_param) if rec_wanted else None
    weights = []
    try:
        for k in range(6):
            w = opt.ema_weight_for_step(opt.ema_updates) if rec_wanted else None
            loss = gs(x0, context=ctx)
            assert torch.isfinite(loss).all()
            assert (gs.graph is not None) == (k >= 2)
            if rec_wanted:
                weights.append(w)
                rec.update(opt.flat_param, w)
                rec.check(opt.flat_ema)   # after the eager steps and after EVERY replay: the ninth word arrives and changes per step
                assert opt.ema_updates == k + 1
        nodes = _graph_nodes(gs.graph)
    finally:
        gs.close()
    return nodes, weights, opt


def test_graph_replays_the_average_without_a_launch_more(monkeypatch):
    nodes_ema, weights, opt = _graphed_run(0.9, monkeypatch, True)
    assert len(set(weights)) == 6 and weights[0] == pytest.approx(0.9) and weights[5] == pytest.approx(1 - 6 / 15)
    assert not torch.equal(opt.flat_ema, opt.flat_param)
    nodes_plain, _, _ = _graphed_run(None, monkeypatch, False)
    print(f"captured graph nodes: {nodes_ema} with the EMA, {nodes_plain} without")
    assert nodes_plain > 10 and nodes_ema <= nodes_plain


# ---- 4. ema_weights() ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,T_,J_,mc", [(128, 10, 4, 3), (256, 16, 20, 5)])
def test_ema_weights_context_carries_every_derived_copy(d, T_, J_, mc):
    """d = 128 runs the generic trajectory kernels, d = 256 with 5 + 1 memory rows the tuned step kernel; both cache split weight planes."""
    from soccerdiffusion_amd import training

    m, opt, ns, _, _ = _train_setup(d=d, T=T_, J=J_, mc=mc)
    g = torch.Generator().manual_seed(23)
    x0, ctx = torch.randn(B, T_, J_, generator=g).cuda(), [torch.randn(B, mc, d, generator=g).cuda()]
    x_T = torch.randn(B, T_, J_, generator=g).cuda()
    step = torch.full((B,), 300).cuda()
    for k in range(3):
        noise, t = torch.randn(B, T_, J_, generator=g).cuda(), torch.randint(0, 1000, (B,), generator=g).cuda()
        training.train_step(m, opt, None, ns, x0, context=ctx, noise=noise, timesteps=t)
    m.eval()
    twin, _ = _model(d, J_, L, T_, seed=9)
    twin.load_state_dict({k: v.clone() for k, v in opt.ema_state_dict(m).items()})
    with torch.no_grad():
        want_sample, want_eps = twin.sample(ctx, x_T, 3), twin.forward_with_context(ctx, x_T, step)
        before_sample, before_eps = m.sample(ctx, x_T, 3), m.forward_with_context(ctx, x_T, step)
    assert not torch.equal(want_sample, before_sample)
    p0, e0 = opt.flat_param.clone(), opt.flat_ema.clone()
    with opt.ema_weights():
        assert torch.equal(opt.flat_param, e0) and torch.equal(opt.flat_ema, p0)
        with torch.no_grad():
            assert torch.equal(m.sample(ctx, x_T, 3), want_sample)
            inside_eps = m.forward_with_context(ctx, x_T, step)
            assert not torch.equal(inside_eps, before_eps) and float((inside_eps - want_eps).abs().max()) < 1e-4 * float(want_eps.abs().max())
    assert torch.equal(opt.flat_param, p0) and torch.equal(opt.flat_ema, e0)
    with torch.no_grad():
        assert torch.equal(m.sample(ctx, x_T, 3), before_sample)
        assert torch.equal(m.forward_with_context(ctx, x_T, step), before_eps)
    with pytest.raises(ZeroDivisionError):
        with opt.ema_weights():
            1 / 0
    assert torch.equal(opt.flat_param, p0) and torch.equal(opt.flat_ema, e0)
    with torch.no_grad():
        assert torch.equal(m.sample(ctx, x_T, 3), before_sample)


# ---- 5. resume -----------------------------------------------------------------------------------------------------------------------
def test_resume_continues_the_average_bitwise(tmp_path):
    m, opt, ns, x0, ctx = _train_setup()
    _steps(m, opt, ns, x0, ctx, 0, 6)

    a, aopt, *_ = _train_setup()
    _steps(a, aopt, ns, x0, ctx, 0, 3)
    path = tmp_path / "ckpt.pth"
    torch.save({"model_state_dict": a.state_dict(), "optimizer_state_dict": aopt.state_dict(),
                "ema_model_state_dict": aopt.ema_state_dict(a), "ema": aopt.ema_state()}, path)
    back = torch.load(path, map_location="cpu", weights_only=True)   # plain types only
    assert back["ema"] == {"decay": 0.9, "warmup": True, "num_updates": 3}
    b, _ = _model(D, J, L, T, seed=77)   # other weights: everything has to come from the file
    b.train().set_dropout(0.0)
    b.load_state_dict(back["model_state_dict"])
    from soccerdiffusion_amd import training

    bopt = training.FusedAdamW(b.parameters(), lr=1e-3, ema_decay=back["ema"]["decay"], ema_warmup=back["ema"]["warmup"])
    bopt.load_state_dict(back["optimizer_state_dict"])
    bopt.load_ema_state_dict(b, back["ema_model_state_dict"], back["ema"]["num_updates"])
    assert torch.equal(bopt.flat_ema, aopt.flat_ema) and torch.equal(bopt.flat_param, aopt.flat_param) and bopt.ema_updates == 3
    _steps(b, bopt, ns, x0, ctx, 3, 3)
    assert torch.equal(bopt.flat_param, opt.flat_param) and torch.equal(bopt.flat_ema, opt.flat_ema)
    assert bopt.ema_updates == 6 and bopt._step == 6


# ---- 6. the commands -----------------------------------------------------------------------------------------------------------------
CFG = dict(hidden_dim=64, action_context_length=20, trajectory_prediction_length=16, epochs=1, batch_size=32, lr=1e-3,
           train_denoising_timesteps=1000, image_context_length=0, imu_context_length=20, num_imu_encoder_layers=1,
           joint_state_context_length=20, num_normalization_samples=50, num_joints=20, use_action_history=False,
           num_action_history_encoder_layers=1, use_imu=True, imu_orientation_embedding_method="quaternion",
           use_joint_states=True, joint_state_encoder_layers=1, use_images=False, image_sequence_encoder_type="transformer",
           image_encoder_type="resnet18", num_image_sequence_encoder_layers=1, num_decoder_layers=1,
           distill_teacher_inference_steps=30, use_gamestate=False, encoder_patch_size=5)
OLD_KEYS = {"model_state_dict", "optimizer_state_dict", "lr_scheduler_state_dict", "hyperparams", "current_epoch"}


def _cli(*argv):
    env = dict(os.environ, PYTHONPATH=REPO)
    r = subprocess.run([sys.executable, "-m", "soccerdiffusion_amd.cli", *argv], cwd=REPO, env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return r


@pytest.fixture(scope="module")
def trained(tmp_path_factory):
    """One run of ``train --ema-decay 0.9`` and one without the flag, shared by the tests below."""
    d = tmp_path_factory.mktemp("ema_cli")
    cfg = d / "cfg.yaml"
    cfg.write_text(yaml.safe_dump(CFG))
    ckpt, plain = d / "ema.pth", d / "plain.pth"
    _cli("train", "-c", str(cfg), "-o", str(ckpt), "--synthetic", "96", "--ema-decay", "0.9")
    _cli("train", "-c", str(cfg), "-o", str(plain), "--synthetic", "96")
    return d, str(ckpt), str(plain)


def _manual_ema_model(ckpt):
    from soccerdiffusion_amd import cli

    manual = cli.build_model(CFG).cuda()
    manual.load_state_dict(torch.load(ckpt, weights_only=True)["ema_model_state_dict"])
    return manual.eval()


def test_cli_checkpoint_keys(trained):
    _, ckpt, plain = trained
    assert set(torch.load(plain, weights_only=True)) == OLD_KEYS
    back = torch.load(ckpt, weights_only=True)
    assert set(back) == OLD_KEYS | {"ema_model_state_dict", "ema"}
    assert back["ema"] == {"decay": 0.9, "warmup": True, "num_updates": 3}
    msd, esd = back["model_state_dict"], back["ema_model_state_dict"]
    assert set(msd) == set(esd) and torch.equal(msd["mean"], esd["mean"]) and torch.equal(msd["std"], esd["std"])
    assert not torch.equal(msd["diffusion_action_generator.fc_out.weight"], esd["diffusion_action_generator.fc_out.weight"])


def test_cli_sample_from_the_average(trained):
    from soccerdiffusion_amd import cli, ops

    d, ckpt, _ = trained
    out_e, out_p = d / "s_ema.pt", d / "s_plain.pt"
    _cli("sample", ckpt, "--steps", "5", "--num_samples", "4", "-o", str(out_e), "--synthetic", "16", "--ema")
    _cli("sample", ckpt, "--steps", "5", "--num_samples", "4", "-o", str(out_p), "--synthetic", "16")
    got_e, got_p = torch.load(out_e, weights_only=True), torch.load(out_p, weights_only=True)
    assert torch.equal(got_e["noise"], got_p["noise"]) and not torch.equal(got_e["trajectories"], got_p["trajectories"])
    manual = _manual_ema_model(ckpt)
    data = {k: v.cuda() for k, v in cli.synthetic_dataset(16, CFG, seed=0).items()}
    with torch.no_grad():
        ctx = manual.encode_input_data({k: data[k][:4].contiguous() for k in cli.CONTEXT_KEYS if k in data})
        traj = ops.normalize(manual.sample(ctx, got_e["noise"].cuda(), 5).contiguous(), manual.mean, manual.std, inverse=True)
    assert torch.equal(traj.cpu(), got_e["trajectories"])


def test_session_from_the_average(trained):
    from soccerdiffusion_amd import cli
    from soccerdiffusion_amd.session import PolicySession

    _, ckpt, plain = trained
    x_T = torch.randn(2, CFG["trajectory_prediction_length"], CFG["num_joints"], generator=torch.Generator().manual_seed(4)).cuda()
    stream = cli.synthetic_sensor_stream(2, CFG, 1, seed=0)

    def tick(session):
        session.push_joint_state(stream["joint_state"].cuda())
        session.push_rotation(stream["rotation"].cuda())
        return session.step(x_T).clone()

    kw = dict(num_inference_steps=5, batch=2, seed=0)
    s_ema = tick(PolicySession.from_checkpoint(ckpt, ema=True, **kw))
    s_last = tick(PolicySession.from_checkpoint(ckpt, ema=False, **kw))
    s_manual = tick(PolicySession(_manual_ema_model(ckpt), hyperparams=CFG, **kw))
    assert torch.isfinite(s_ema).all() and not torch.equal(s_ema, s_last) and torch.equal(s_ema, s_manual)
    with pytest.raises(ValueError, match="ema_model_state_dict"):
        PolicySession.from_checkpoint(plain, ema=True, **kw)


# ---- 7. data parallel ------------------------------------------------------------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _dp_worker(rank, world, port, out):
    import torch.distributed as dist

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)   # both ranks on the one GPU, as bench.py's rehearsal
    try:
        from soccerdiffusion_amd import training

        m, opt, ns, x0, ctx = _train_setup(seed=5 + rank)
        opt.flat_ema.add_(float(rank + 1))
        opt.ema_updates = 4 * rank
        mine = opt.flat_ema.clone()
        training.broadcast_parameters(opt, m)
        both = [torch.empty_like(mine).cpu() for _ in range(world)]
        dist.all_gather(both, mine.cpu())
        res = {"bcast": bool(torch.equal(opt.flat_ema.cpu(), both[0])) and not torch.equal(both[0], both[1]) and opt.ema_updates == 0}
        g = torch.Generator().manual_seed(50 + rank)   # every rank its own data
        for _ in range(3):
            noise, t = torch.randn(B, T, J, generator=g).cuda(), torch.randint(0, 1000, (B,), generator=g).cuda()
            training.train_step(m, opt, None, ns, x0 + rank, context=ctx, noise=noise, timesteps=t, world_size=world)
        training.assert_replicas_equal(opt)
        res["moved"] = not torch.equal(opt.flat_ema, opt.flat_param) and opt.ema_updates == 3
        if rank == 1:
            opt.flat_ema[7] += 1.0
        try:
            training.assert_replicas_equal(opt)
            res["raised"] = False
        except RuntimeError as e:
            res["raised"] = "EMA" in str(e)
        out[rank] = res
    finally:
        dist.destroy_process_group()


def test_data_parallel_broadcasts_and_checks_the_average():
    import torch.multiprocessing as mp

    port = _free_port()
    with mp.Manager() as mgr:
        out = mgr.dict()
        mp.spawn(_dp_worker, args=(2, port, out), nprocs=2, join=True)
        want = {"bcast": True, "moved": True, "raised": True}
        assert dict(out) == {0: want, 1: want}
