"""The shared cross-attention kernels of training with several noise draws per window (csrc/sd_train_shared.hip), alone.

Yardstick: tests/shared_attn_ref.py in fp64, beside the same restatement in fp32 on the CPU; gate: tests/parity.py's (4 x the fp32
run's own error + 1e-7 on the global, per-trajectory and per-row figures).  The kernels' figures are never measured against the
kernels' own numbers.  Tile widths of the kernels: 32-key tiles in 64-key LDS chunks (keys = Mc + 1), 32 queries per wave, T <= 100."""

import pytest
import torch

import parity
import shared_attn_ref as ref

pytestmark = pytest.mark.gpu

HEADS = 4
C = 2


def _ops():
    from soccerdiffusion_amd import ops

    return ops


_CASES: dict = {}


def _case(d, K, T, Mc):
    """Inputs and both CPU references of a case, computed once and shared (never modified)."""
    key = (d, K, T, Mc)
    if key not in _CASES:
        q, kc, kt, dO = ref.case(d, HEADS, C, K, T, Mc)
        want = ref.forward(q, kc, kt, HEADS, K) + ref.backward(q, kc, kt, dO, HEADS, K)
        f = [t.float() for t in (q, kc, kt, dO)]
        want32 = ref.forward(f[0], f[1], f[2], HEADS, K) + ref.backward(*f, HEADS, K)
        _CASES[key] = (f, want, want32)
    return _CASES[key]


NAMES = ("out", "lse2", "dq", "dkv_ctx", "dkv_tok")


def _run(f, K, drop=None):
    ops = _ops()
    q, kc, kt, dO = (t.cuda() for t in f)
    out, lse = ops.train_xattn_shared_fwd(q, kc, kt, HEADS, K, drop)
    dq, dkc, dkt = ops.train_xattn_shared_bwd(q, kc, kt, out, dO, lse, HEADS, K, drop)
    torch.cuda.synchronize()
    return out, lse, dq, dkc, dkt


def _gate(got, want, want32, label):
    for name, g, w, w32 in zip(NAMES, got, want, want32):
        parity.assert_fp32_grade(g, w, w32, label=f"{label} {name}")


# the issue's grid, then one below / at / one above the key tile (32), the key chunk (64) and the query tile (32) widths, and T's ends
GRID = [(d, K, T, Mc) for d in (64, 128, 256) for K in (1, 3, 4) for T in (1, 10) for Mc in (1, 40, 311)]
EDGES = ([(128, 3, 10, Mc) for Mc in (30, 31, 32, 62, 63, 64, 65, 127, 128)] + [(256, 2, T, 40) for T in (31, 32, 33, 64, 65, 99, 100)]
         + [(64, 3, 33, 63), (128, 4, 100, 311)])


@pytest.mark.parametrize("d,K,T,Mc", GRID + EDGES)
def test_shared_xattn_is_fp32_grade(d, K, T, Mc):
    f, want, want32 = _case(d, K, T, Mc)
    _gate(_run(f, K), want, want32, f"d{d} K{K} T{T} Mc{Mc}")


@pytest.mark.parametrize("d,K,T,Mc", [(64, 3, 10, 40), (128, 4, 10, 311), (256, 3, 10, 40), (256, 4, 33, 63), (128, 1, 1, 1)])
def test_dropout_mask_is_the_expanded_calls(d, K, T, Mc):
    """p = 0.1: the shared call and the existing attention on the expanded K | V, under the same (p, seed, site), both meet the gate
    against the fp64 reference with the library's mask for (b, head, t, key), width Mc + 1 - a differing mask is an O(1) error."""
    ops = _ops()
    f, _, _ = _case(d, K, T, Mc)
    drop = (0.1, 1234567, (3 << 24) | (1 << 4) | 2)
    B = C * K
    mask = ops.dropout_mask(B * HEADS * T, Mc + 1, drop, "cuda").cpu().view(B, HEADS, T, Mc + 1)
    assert 0.02 < float((mask == 0).double().mean()) < 0.25 or mask.numel() < 200
    q, kc, kt, dO = (t.double() for t in f)
    want = ref.forward(q, kc, kt, HEADS, K, mask.double()) + ref.backward(q, kc, kt, dO, HEADS, K, mask.double())
    want32 = ref.forward(*f[:3], HEADS, K, mask) + ref.backward(*f, HEADS, K, mask)
    _gate(_run(f, K, drop), want, want32, f"dropout shared d{d} K{K} T{T} Mc{Mc}")
    # the existing kernels on the expanded memory
    qg, dOg = f[0].cuda(), f[3].cuda()
    kv = ref.expand_kv(f[1], f[2], K).cuda().contiguous()
    out, lse = ops.attention_lse(qg, kv[..., :d], kv[..., d:], HEADS, drop)
    dq, dkv = torch.empty_like(qg), torch.empty_like(kv)
    ops.attention_bwd(qg, kv[..., :d], kv[..., d:], out, dOg, lse, dq, dkv[..., :d], dkv[..., d:], HEADS, drop)
    dkc = dkv[:, :Mc].double().view(C, K, Mc, 2 * d).sum(1)
    _gate((out, lse, dq, dkc, dkv[:, Mc:]), want, want32, f"dropout expanded d{d} K{K} T{T} Mc{Mc}")


@pytest.mark.parametrize("d,K,T,Mc,p", [(256, 4, 10, 311, 0.0), (128, 3, 33, 40, 0.1)])
def test_dkv_ctx_is_bitwise_repeatable(d, K, T, Mc, p):
    f, _, _ = _case(d, K, T, Mc)
    drop = (p, 99, 5) if p else None
    a, b = _run(f, K, drop), _run(f, K, drop)
    for name, x, y in zip(NAMES, a, b):
        assert torch.equal(x, y), name


def test_dkv_tok_depends_on_its_own_trajectory_only():
    d, K, T, Mc = 128, 4, 10, 40
    f, _, _ = _case(d, K, T, Mc)
    base = _run(f, K)
    g = [t.clone() for t in f]
    b = 5   # context 1, draw 1: every other trajectory changes, two of them in b's own group
    others = [i for i in range(C * K) if i != b]
    gen = torch.Generator().manual_seed(3)
    for i in (0, 2, 3):
        g[i][others] = torch.randn(g[i][others].shape, generator=gen)
    moved = _run(g, K)
    assert torch.equal(base[4][b], moved[4][b])
    assert torch.equal(base[0][b], moved[0][b]) and torch.equal(base[2][b], moved[2][b])
    assert not torch.equal(base[4][others], moved[4][others])


def test_unsupported_shapes_decline():
    ops = _ops()
    assert ops.train_xattn_shared_ok(256, 4, 100, 311) and ops.train_xattn_shared_ok(64, 4, 1, 1)
    assert not ops.train_xattn_shared_ok(512, 4, 10, 40) and not ops.train_xattn_shared_ok(256, 4, 101, 40)
    assert not ops.train_xattn_shared_ok(256, 4, 10, 0)
    q, kc, kt = torch.zeros(2, 10, 512, device="cuda"), torch.zeros(1, 4, 1024, device="cuda"), torch.zeros(2, 1, 1024, device="cuda")
    with pytest.raises(RuntimeError, match="-4"):
        ops.train_xattn_shared_fwd(q, kc, kt, HEADS, 2)
    with pytest.raises(ValueError, match="draws"):
        ops.train_xattn_shared_fwd(q[:, :, :256].contiguous(), kc[..., :512].contiguous(), kt[..., :512].contiguous(), HEADS, 3)


def test_expand_rows_and_its_fixed_order_sum():
    ops = _ops()
    x = torch.randn(3, 5, 8, device="cuda")
    e = ops.expand_rows(x, 4)
    assert torch.equal(e, x.repeat_interleave(4, 0))
    g = torch.randn(12, 5, 8, device="cuda")
    want = g.view(3, 4, 5, 8)
    acc = want[:, 0].clone()
    for k in range(1, 4):
        acc = acc + want[:, k]
    assert torch.equal(ops.expand_rows_bwd(g, 4), acc)
    for bad in (5, 0, -1, 2.0):   # 12 rows are no multiple of 5: no trailing rows dropped in silence
        with pytest.raises(ValueError, match="draws"):
            ops.expand_rows_bwd(g, bad)
    with pytest.raises(ValueError, match="draws"):
        ops.expand_rows(x, 0)
