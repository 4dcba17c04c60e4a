"""Several noise draws per window, the parts that need no GPU: the fp64 restatement of the two-segment attention (tests/shared_attn_ref.py)
pinned against torch autograd on the expanded memory, the validation of ``draws``, ``cli train --noise-draws`` and the checkpoint key."""

import pytest
import torch

import shared_attn_ref as ref

HEADS = 4


@pytest.mark.parametrize("d,C,K,T,Mc", [(64, 2, 3, 5, 7), (128, 1, 4, 10, 1), (256, 3, 1, 1, 40), (64, 2, 2, 33, 65)])
@pytest.mark.parametrize("dropout", [False, True])
def test_reference_equals_autograd_on_the_expanded_memory(d, C, K, T, Mc, dropout):
    q, kc, kt, dO = ref.case(d, HEADS, C, K, T, Mc)
    mask = None
    if dropout:
        g = torch.Generator().manual_seed(5)
        mask = (torch.rand(C * K, HEADS, T, Mc + 1, generator=g) >= 0.1).double() / 0.9
    ql, kcl, ktl = (t.clone().requires_grad_() for t in (q, kc, kt))
    out = ref.expanded(ql, ref.expand_kv(kcl, ktl, K), HEADS, mask)
    out.backward(dO)
    got_out, lse2 = ref.forward(q, kc, kt, HEADS, K, mask)
    dq, dkc, dkt = ref.backward(q, kc, kt, dO, HEADS, K, mask)
    for name, a, b in (("out", got_out, out.detach()), ("dq", dq, ql.grad), ("dkv_ctx", dkc, kcl.grad), ("dkv_tok", dkt, ktl.grad)):
        assert a.shape == b.shape and float((a - b).norm() / b.norm()) < 1e-13, name
    # lse2: the log2-domain log-sum-exp of the scaled scores over both segments
    kv = ref.expand_kv(kc, kt, K)
    s = ref._heads(q, HEADS) @ ref._heads(kv[..., :d], HEADS).transpose(-1, -2) / (d // HEADS) ** 0.5
    assert torch.allclose(lse2, torch.logsumexp(s, -1) / torch.log(torch.tensor(2.0, dtype=torch.float64)), rtol=0, atol=1e-12)
    # the context's gradient is the sum over the draws of what each expanded copy receives
    kvl = kv.clone().requires_grad_()
    ref.expanded(q, kvl, HEADS, mask).backward(dO)
    assert float((kvl.grad[:, :Mc].view(C, K, Mc, 2 * d).sum(1) - dkc).norm() / dkc.norm()) < 1e-13


def test_reference_runs_in_fp32_close_to_fp64():
    q, kc, kt, dO = ref.case(128, HEADS, 2, 3, 10, 40)
    want = ref.forward(q, kc, kt, HEADS, 3) + ref.backward(q, kc, kt, dO, HEADS, 3)
    got = ref.forward(q.float(), kc.float(), kt.float(), HEADS, 3) + ref.backward(q.float(), kc.float(), kt.float(), dO.float(), HEADS, 3)
    for a, b in zip(got, want):
        assert a.dtype == torch.float32 and 0.0 < float((a.double() - b).norm() / b.norm()) < 1e-5


def test_draws_validation():
    from soccerdiffusion_amd import training

    assert training.noise_draws(1) == 1 and training.noise_draws(8) == 8
    for bad in (0, -3, 1.0, True, None, "4"):
        with pytest.raises(ValueError, match="draws"):
            training.noise_draws(bad)
    with pytest.raises(ValueError, match="draws"):
        training.GraphedTrainStep.__init__(object.__new__(training.GraphedTrainStep), None, None, None, None, draws=0)


def test_train_route_and_its_slots_are_unchanged():
    """The shared route is additive: the pinned route table does not move, and the two abs-max slots it uses were the free ones."""
    from soccerdiffusion_amd import training

    assert training._AX_SLOTS == 20 and (training._AX_TOK, training._AX_DKT) == (18, 19)
    r = training.train_route(decoder=True, d=256, heads=4, T=10, M=11, J=20, ffn_is_d=True, params_ok=True, block_planes=True, traj_planes=True,
                             x_differentiable=False, layer_fwd_ok=lambda d, h, T, M: M <= 16)
    assert r == ("chains", True, True)


def test_cli_noise_draws_flag_and_checkpoint_key():
    from soccerdiffusion_amd import cli

    ap = cli.build_parser()
    assert ap.parse_args(["train", "-c", "x.yaml"]).noise_draws is None
    assert ap.parse_args(["train", "-c", "x.yaml", "--noise-draws", "4"]).noise_draws == 4
    for bad in ("0", "-1", "65", "two", "1.5"):
        with pytest.raises(SystemExit):
            ap.parse_args(["train", "-c", "x.yaml", "--noise-draws", bad])
    with pytest.raises(SystemExit):   # out of scope for distillation: the flag does not exist there
        ap.parse_args(["distill", "x.yaml", "x.pth", "--noise-draws", "4"])
    # the flag wins; else the resumed checkpoint's value; else 1
    assert cli.noise_draws_of(None, None) == 1
    assert cli.noise_draws_of(None, {"hyperparams": {}}) == 1
    assert cli.noise_draws_of(None, {"noise_draws": 4}) == 4
    assert cli.noise_draws_of(2, {"noise_draws": 4}) == 2
