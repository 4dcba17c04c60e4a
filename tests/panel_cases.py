"""Cases, expected routes, inputs and fp64 / fp32 CPU oracles for the row-panel decoder routes (panel_plan() of csrc/sd_sampler_plan.h:
CHAINS_F32, CHAINS_F16, FUSED, FUSED_FOLD, FUSED_FOLD_F16 - what a sampler call capped at mode 0 .. 2 runs, what every guarded call
repeats after SD_STATUS_NONFINITE, what sd_denoiser_forward runs and what serves every shape the trajectory families decline) - a plain
helper module, not a conftest.  tests/test_cpu_panel_grade.py pins the route of every (case, cap) against the library and the coverage of
the list itself; tests/test_gpu_panel_grade.py holds the kernels to parity.assert_fp32_grade on the same cases.

The rollout helpers and the power-of-two rescaling construction are shared with tests/test_gpu_shipped_shapes_grade.py (mode 3)."""

from __future__ import annotations

import functools

import torch

from oracle import ddim_ref
from oracle import denoiser_ref as ref

LAYER = "diffusion_action_generator.transformer_decoder.layers.{}."
N_SCHEDULE = 50   # the first steps of the 50-step schedule: t = 980, 960, 940, 920 (|x| stays at its t ~ T level, as in a rollout's start)
N_STEPS = 4
HEADS = 4

F32, F16, FUSED, FOLD, FOLD16 = "CHAINS_F32", "CHAINS_F16", "FUSED", "FUSED_FOLD", "FUSED_FOLD_F16"
PANEL_ROUTES = (F32, F16, FUSED, FOLD, FOLD16)
CAPS = (0, 1, 2)


# ------------------------------------------------------------------------------------------------------------------------------------
# rollout helpers (shared with the mode-3 suite)
# ------------------------------------------------------------------------------------------------------------------------------------
def schedule():
    acp = ddim_ref.alphas_cumprod()
    ts = ddim_ref.timesteps(N_SCHEDULE).tolist()
    return acp, ts


def oracle_rollout(sd, ctx, x_T, dtype, n_steps):
    """The reference's loop (ddim_ref.sample's body) over the first n_steps of the 50-step schedule: x after every step and every noise
    prediction, in `dtype`."""
    acp, ts = schedule()
    B = x_T.shape[0]
    x = x_T.to(dtype)
    xs, eps = [], []
    for t in ts[:n_steps]:
        e = ref.forward_with_context(sd, [ctx] if ctx is not None else [], x, torch.full((B,), t, dtype=torch.int64), dtype=dtype)
        x = ddim_ref.step(e, t, x, N_SCHEDULE, acp)
        assert x.dtype == dtype
        eps.append(e)
        xs.append(x)
    return xs, eps


def gpu_tokens(ops, sd, d, n_steps):
    acp, ts = schedule()
    toks = ops.step_token(torch.tensor(ts[:n_steps]).cuda(), ops.step_frequencies(d).cuda(), sd["step_encoding.token"].cuda())
    return toks.reshape(n_steps, d), ops.ddim_coefficients(ts, acp, N_SCHEDULE)[:n_steps]


def case_id(v):
    return "-".join(str(i) for i in v) if isinstance(v, tuple) else None


# ------------------------------------------------------------------------------------------------------------------------------------
# function-preserving rescaling by powers of two (shared with the mode-3 suite)
# ------------------------------------------------------------------------------------------------------------------------------------
RESCALE_SHAPES = [(256, 100, 10, 20, 2, 2), (128, 10, 40, 20, 2, 2)]   # mode 3: tuned (folded) and generic; cap 1: FUSED_FOLD and CHAINS_F32
PAIRS = ["norm1", "norm2", "norm3", "self_v", "cross_v", "memory"]


@functools.lru_cache(maxsize=None)
def rescale_base(shape):
    """Unscaled weights, inputs, the memory (context rows and the oracle's own step token at t = 980) and both oracles' outputs."""
    d, T, Mc, J, L, B = shape
    sd = ref.synthetic_state_dict(d, J, L, seed=53 + d)
    g = torch.Generator().manual_seed(d + T)
    x = torch.randn(B, T, J, generator=g)
    ctx = torch.randn(B, Mc, d, generator=g)
    tok = ref.step_token(torch.tensor([980]), sd["step_encoding.token"].float(), d)           # (1, 1, d)
    mem = torch.cat([ctx, tok.expand(B, 1, d)], 1)
    want64 = ref.denoiser_forward(sd, x, mem, dtype=torch.float64)
    want32 = ref.denoiser_forward(sd, x, mem)
    return sd, x, ctx, tok, want64, want32


def rescaled(shape, pairs, k):
    """Producer x 2^-k, consumer x 2^k for every pair named: the same function, bit for bit in fp32, on operands 2^k away from where
    the kernels' fixed activation scales expect them.  'memory' scales every memory row - the context and the step token handed to the
    sampler - against the K | V rows of the cross-attention's in_proj_weight."""
    sd0, x, ctx, tok, _, _ = rescale_base(shape)
    d, L = shape[0], shape[4]
    sd = {key: v.clone() for key, v in sd0.items()}
    down, up = 2.0 ** -k, 2.0 ** k
    for l in range(L):
        pre = LAYER.format(l)
        for p in pairs:
            if p in ("norm1", "norm2", "norm3"):
                sd[pre + p + ".weight"] *= down
                sd[pre + p + ".bias"] *= down
                if p == "norm1":
                    sd[pre + "self_attn.in_proj_weight"] *= up
                elif p == "norm2":
                    sd[pre + "multihead_attn.in_proj_weight"][:d] *= up
                else:
                    sd[pre + "linear1.weight"] *= up
            elif p in ("self_v", "cross_v"):
                att = "self_attn" if p == "self_v" else "multihead_attn"
                sd[pre + att + ".in_proj_weight"][2 * d:] *= down
                sd[pre + att + ".in_proj_bias"][2 * d:] *= down
                sd[pre + att + ".out_proj.weight"] *= up
            elif p == "memory":
                sd[pre + "multihead_attn.in_proj_weight"][d:] *= up
            else:
                raise KeyError(p)
    if "memory" in pairs:
        ctx, tok = ctx * down, tok * down
    return sd, x, ctx, tok


# ------------------------------------------------------------------------------------------------------------------------------------
# the cases: (d, T, Mc, J, L, B) with 4 heads -> the route at caps 0, 1, 2
# ------------------------------------------------------------------------------------------------------------------------------------
_CHAINS = (F32, F32, F16)      # the fp16 row chains need J % 4 == 0
_CHAINS32 = (F32, F32, F32)
_FUSED = (FUSED, FUSED, FUSED)
_FOLD = (FUSED, FOLD, FOLD)    # no fp16 layer kernel: hidden_dim != 256 or J % 4 != 0
_FOLD16 = (FUSED, FOLD, FOLD16)

# the rerun path of the shipped configs, and their modes 0 - 2
SHIPPED = {
    (128, 10, 311, 20, 4, 3): _CHAINS,      # default.yaml
    (128, 10, 311, 22, 4, 1): _CHAINS32,    # 22 joints: patch_embed + linear in front of the chains
    (512, 10, 311, 20, 8, 2): _CHAINS,      # larger_model.yaml
    (512, 10, 311, 22, 8, 1): _CHAINS32,
    (256, 10, 50, 20, 6, 2): _CHAINS,       # sim_scratch.yaml
    (256, 10, 50, 22, 6, 1): _CHAINS32,
    (256, 10, 10, 20, 4, 2): _CHAINS,       # decoder_only.yaml
    (256, 10, 0, 20, 4, 2): _FUSED,         # eight trajectories per panel, one key each
    (256, 100, 10, 20, 4, 3): _FOLD16,      # the benchmark's shape
}
# shapes the trajectory families decline: cap 3 lands on the cap-2 route
PANEL_ONLY = {
    (64, 16, 10, 20, 2, 3): _CHAINS32,      # hidden_dim 64
    (256, 100, 10, 33, 2, 2): _FOLD,        # J > 32: two fc_out tiles, J % 4 != 0
    (256, 100, 10, 64, 2, 2): _FOLD16,
    (128, 10, 40, 33, 2, 3): _CHAINS32,
    (256, 128, 3, 20, 1, 2): _FOLD16,       # the last horizon of the fp16 self-attention ...
    (256, 129, 3, 20, 1, 2): _FOLD16,       # ... and the first past it
    (256, 130, 5, 20, 2, 2): _FOLD16,       # T > 100
    (256, 10, 10, 20, 9, 1): _CHAINS,       # nine layers
    (512, 49, 10, 20, 2, 2): _FUSED,        # hidden_dim 512 past 48 tokens, below the fold's 64
    (512, 100, 10, 20, 2, 2): _FOLD,
}
TILE_EDGES = {
    (128, 1, 0, 4, 1, 1): _FUSED,           # one row
    (128, 9, 20, 20, 1, 7): _CHAINS,        # 63 / 64 / 65 rows on both chain routes
    (128, 16, 20, 20, 1, 4): _CHAINS,
    (128, 13, 20, 20, 1, 5): _CHAINS,
    (128, 1, 0, 4, 1, 65): _FUSED,          # 64 trajectories x 1 key fill both key tiles of a panel; a second panel of one row
    (256, 100, 31, 20, 2, 2): _FUSED,       # 64 keys in the two-trajectory panels, 32 in the one-trajectory panel
    (256, 100, 32, 20, 2, 2): _CHAINS,      # 66 keys: off the fused kernel
    (128, 40, 10, 20, 2, 4): _FUSED,        # three trajectories per panel
    (256, 7, 2, 20, 2, 30): _FUSED,         # ten trajectories per panel
    (128, 64, 15, 20, 2, 3): _FOLD,         # the first folded horizon with all 16 key slots
    (256, 64, 15, 20, 2, 3): _FOLD16,
    (512, 64, 15, 20, 2, 3): _FOLD,
    (256, 63, 15, 20, 2, 3): _FUSED,        # one short of the fold on each condition
    (256, 64, 16, 20, 2, 3): _FUSED,
    (256, 97, 0, 4, 1, 2): _FOLD16,         # the step row alone, ragged last panel
    (256, 100, 15, 32, 2, 2): _FOLD16,
    (512, 100, 4, 22, 2, 2): _FOLD,         # a fused layer behind the unfused head, panel_fc_out at J = 22
    (256, 100, 10, 22, 2, 2): _FOLD,
}
ROUTES = {**SHIPPED, **PANEL_ONLY, **TILE_EDGES}
CASES = list(ROUTES)
assert len(CASES) == len(SHIPPED) + len(PANEL_ONLY) + len(TILE_EDGES)
CASE_CAPS = [(s, cap) for s in CASES for cap in CAPS]


def cap_id(v):
    return case_id(v) if isinstance(v, tuple) else f"cap{v}"


def rows(shape) -> int:
    return shape[5] * shape[1]


def panels(shape):
    """[(trajectories touched, keys among them)] per 64-row panel of a fused-route shape (decoder_layer_kernel: panel i holds rows
    64 i .. 64 i + 63 of the (B T, d) row stream; Mk = Mc + 1 memory rows per trajectory)."""
    _, T, Mc, _, _, B = shape
    R = B * T
    out = []
    for r0 in range(0, R, 64):
        n = (min(r0 + 64, R) - 1) // T - r0 // T + 1
        out.append((n, n * (Mc + 1)))
    return out


@functools.lru_cache(maxsize=None)
def inputs(shape):
    """(weights, x_T, context or None) of a case."""
    d, T, Mc, J, L, B = shape
    sd = ref.synthetic_state_dict(d, J, L, seed=23 + T + d)
    g = torch.Generator().manual_seed(T * 5 + Mc + d + J + B)
    x_T = torch.randn(B, T, J, generator=g)
    ctx = torch.randn(B, Mc, d, generator=g) if Mc else None
    return sd, x_T, ctx


@functools.lru_cache(maxsize=None)
def oracles(shape):
    """(x64, eps64, x32, eps32): oracle_rollout over N_STEPS in fp64 and fp32 - computed once per shape, shared by its caps and by the
    sd_denoiser_forward case (the noise prediction at t = 980 IS ref.denoiser_forward on memory())."""
    sd, x_T, ctx = inputs(shape)
    x64, eps64 = oracle_rollout(sd, ctx, x_T, torch.float64, N_STEPS)
    x32, eps32 = oracle_rollout(sd, ctx, x_T, torch.float32, N_STEPS)
    return x64, eps64, x32, eps32


def memory(shape):
    """The memory of one evaluation at t = 980: the context rows and the oracle's own step token appended (rescale_base's form)."""
    sd, x_T, ctx = inputs(shape)
    d, B = shape[0], shape[5]
    tok = ref.step_token(torch.tensor([980]), sd["step_encoding.token"].float(), d).expand(B, 1, d)
    return tok.contiguous() if ctx is None else torch.cat([ctx, tok], 1)


# ------------------------------------------------------------------------------------------------------------------------------------
# a CPU model of the suspected site: an out-projection accumulated in the residual registers
# ------------------------------------------------------------------------------------------------------------------------------------
def _mfma_accumulate(acc, a, w):
    """acc += a w^T the way a chain of mfma_f32_32x32x2f32 does it: two terms of K per instruction, each instruction
    D = fma(a_k1, b_k1, fma(a_k0, b_k0, C)) - fp32 fmas in k order, one rounding per product, no wider sum inside - into the fp32
    accumulator it was given (the product of two fp32 numbers is exact in fp64, so fp64 add + one rounding is the fma)."""
    for k in range(0, a.shape[1], 2):            # one MFMA: K = 2
        for kk in (k, k + 1):
            acc = (acc.double() + a[:, kk:kk + 1].double() * w[:, kk].double()).float()
    return acc


def out_projection_model(d: int, layers: int = 2, rows: int = 64, seed: int = 0):
    """`layers` x three sublayers h += LN(h) W^T + b on `rows` rows of a residual stream at the decoder's magnitudes (embedding + positional
    table ~ 1, synthetic weights ~ 1 / sqrt(d)), in three forms: fp64; fp32 with every MFMA product accumulated INTO the residual
    (chain_a_kernel, decoder_layer_kernel); fp32 into a zero accumulator that meets the residual in one addition (chain_b_kernel).
    Returns (want64, want32, residual_form, own_form), each (1, rows, d) for parity.errors; want32 is plain fp32 torch."""
    g = torch.Generator().manual_seed(seed + d)
    h0 = torch.randn(rows, d, generator=g) + ref.positional_table(d, rows)
    ws = [(torch.randn(d, d, generator=g) / d ** 0.5, 0.1 * torch.randn(d, generator=g)) for _ in range(3 * layers)]

    def ln(v):
        mu = v.mean(-1, keepdim=True)
        return (v - mu) / torch.sqrt(((v - mu) ** 2).mean(-1, keepdim=True) + 1e-5)

    h64, h32, h_res, h_own = h0.double(), h0.clone(), h0.clone(), h0.clone()
    for w, b in ws:
        h64 = h64 + ln(h64) @ w.double().T + b.double()
        h32 = h32 + ln(h32) @ w.T + b
        h_res = _mfma_accumulate(h_res, ln(h_res), w) + b
        h_own = h_own + (_mfma_accumulate(torch.zeros_like(h_own), ln(h_own), w) + b)
    return h64[None], h32[None], h_res[None], h_own[None]
