"""Training side of the hot path: forward/backward of the denoiser and the context encoders
as autograd nodes whose every computation is a HIP kernel, the fused AdamW step on flat
buffers, and the data-parallel gradient all-reduce.

Reference semantics: one iteration of soccer_diffusion/ml/training/train.py:204-240
(normalise, t ~ randint, eps ~ randn, add_noise, forward, F.mse_loss, backward,
AdamW(lr).step, OneCycleLR.step).  The reference trains with torch's default dropout 0.1
(decoder.py:26-33 / encoder/base.py:29-40 never set it, train.py never calls .eval()):
``Dropout`` below reproduces it at torch's four kinds of sites with a counter-based Philox
mask that the backward kernels regenerate (nothing is stored); p = 0 is the parity path
(bit-level parity with torch's own mask stream is not defined: a different generator).

torch.autograd is used as the tape only (plumbing): each node below is one reference
block, its forward and backward are calls into libsoccerdiffusion_hip.so.
"""

from __future__ import annotations

import os
import weakref
from typing import NamedTuple, Optional

import torch
from torch.autograd import Function

from . import ops
from .optim import FusedAdamW, _packed_weight, _transposed_block, planes_of  # noqa: F401  (the optimizer's names stay importable from here)

Tensor = torch.Tensor


def _grad_views(*params):
    """Where parameter gradients go.  When the ``.grad`` buffers of all of ``params`` - parameters, or (parameter, row slice) pairs - are
    preallocated (FusedAdamW aliases them to one flat buffer and zeroes it per step), the backward kernels ACCUMULATE straight into them
    (dW += dY^T X with fp32 atomics) and the autograd node returns None for those inputs: no zero-fill, no extra add kernel, no copy.
    Returns those buffers, or None: fresh zeros are then handed back to autograd as usual."""
    views = []
    for item in params:
        p, sl = item if isinstance(item, tuple) else (item, None)
        if p.grad is None or not p.grad.is_cuda:
            return None
        views.append(p.grad if sl is None else p.grad[sl])
    return views


class _GradSink:
    """_grad_views decided when the forward builds the node; the zeros, if any, are made in the backward."""

    __slots__ = ("views",)

    def __init__(self, *params_and_slices):
        self.views = _grad_views(*params_and_slices) if params_and_slices else None

    def target(self, i: int, like: Tensor):
        """(tensor to accumulate into, value to hand back to autograd)."""
        if self.views is not None:
            return self.views[i], None
        z = torch.zeros(like.shape, dtype=torch.float32, device=like.device)
        return z, z


def _grad_targets(*params):
    """(tensors to accumulate into, values to hand back to autograd), decided and made in the backward."""
    views = _grad_views(*params)
    if views is not None:
        return views, [None] * len(params)
    z = [torch.zeros_like(p[0][p[1]] if isinstance(p, tuple) else p) for p in params]
    return z, z


def _linear(A: Tensor, W: Tensor, b, ln=None, res=None, drop=None) -> Tensor:
    """out = [res +] [dropout](LN?(A) W^T + b) on W's split planes when its optimizer keeps them, else on W itself."""
    wpk = _packed_weight(W)
    if wpk is not None:
        return ops.linear_packed(A, wpk, W.shape[0], b, ln=ln, res=res, drop=drop)
    if drop is not None:
        return ops.linear_dropout(A.contiguous(), W, b, res, drop)
    return ops.linear(A, W, b, ln=ln, res=res)


def _dx_through_weight(dy2d: Tensor, W: Tensor) -> Tensor:
    """dX[R,d] = dY[R,N] @ W[N,d]: the forward panel kernel on W^T, one pass per d-wide
    column slice of dY (N = d, 2d or 3d), accumulated through the residual input."""
    N, d = W.shape
    out = None
    for p in range(N // d):
        wpk = _packed_weight(W, p, transposed=True)
        if wpk is not None:
            out = ops.linear_packed(dy2d[:, p * d : (p + 1) * d], wpk, d, None, res=out, out=out)
        else:
            out = ops.linear_strided(dy2d[:, p * d : (p + 1) * d], _transposed_block(W, p, d), res=out, out=out)
    return out


# ---- dropout sites (torch: nn.MultiheadAttention.dropout, TransformerDecoderLayer.dropout1/2/3 and .dropout) ----------
SITE_SA_PROBS, SITE_SA_OUT, SITE_CA_PROBS, SITE_CA_OUT, SITE_FFN_ACT, SITE_FFN_OUT = range(6)


class Dropout:
    """Dropout configuration of one transformer stack (the decoder or one context encoder).

    ``p`` defaults to torch's 0.1, as in the reference, and is live only in ``module.train()`` mode.  ``seed`` keys
    the Philox mask; every forward call of the stack draws a fresh call index, and a site is
    ``(call << 24) | (salt << 12) | (layer << 4) | kind``, so masks never repeat across calls, stacks, layers or
    sites.  ``for_call()`` returns the per-call object the autograd nodes use (``None`` when dropout is off)."""

    def __init__(self, p: float = 0.1, seed: Optional[int] = None, salt: int = 0):
        self.p, self.seed, self.salt, self.calls = float(p), seed, int(salt), 0

    def for_call(self, training: bool):
        if not training or self.p <= 0.0:
            return None
        if self.seed is None:
            self.seed = int(torch.initial_seed())
        self.calls += 1
        return _DropCall(self.p, self.seed, (self.calls << 24) | (self.salt << 12))


class _DropCall:
    __slots__ = ("p", "seed", "base")

    def __init__(self, p, seed, base):
        self.p, self.seed, self.base = p, seed, base

    def site(self, layer: int, kind: int) -> tuple:
        return (self.p, self.seed, self.base | (layer << 4) | kind)


class _LNLinear(Function):
    """y = act(LayerNorm(x) W^T + b) — LN1+QKV, LN2+Q, LN3+FFN1(+GELU [+ dropout])."""

    @staticmethod
    def forward(ctx, x, ln_w, ln_b, W, b, gelu: bool, sink=None, drop=None, link=None):
        ctx.link = link
        x2 = x.reshape(-1, x.shape[-1])
        pre = _linear(x2, W, b, ln=(ln_w, ln_b))
        if gelu:
            y = ops.gelu_dropout_fwd(pre, drop) if drop is not None else ops.gelu_fwd(pre)
        else:
            y = pre
        ctx.save_for_backward(x2, ln_w, ln_b, W, pre if gelu else None)
        ctx.gelu = gelu
        ctx.drop = drop
        ctx.shape = x.shape
        ctx.sink = sink if sink is not None else _GradSink()
        return y.view(*x.shape[:-1], W.shape[0])

    @staticmethod
    def backward(ctx, dy):
        x2, ln_w, ln_b, W, pre = ctx.saved_tensors
        dy2 = dy.contiguous().view(-1, W.shape[0])
        if ctx.gelu:
            dpre = ops.gelu_dropout_bwd(dy2, pre, ctx.drop) if ctx.drop is not None else ops.gelu_bwd(dy2, pre)
        else:
            dpre = dy2
        n, mean, rstd = ops.layernorm_fwd(x2, ln_w, ln_b)  # recomputed, not stored
        (dg, rg), (dbeta, rbeta) = ctx.sink.target(0, ln_w), ctx.sink.target(1, ln_w)
        (dW, rW), (db, rb) = ctx.sink.target(2, W), ctx.sink.target(3, W[:, 0])
        ops.gemm_tn(dpre, n, dW, db)
        dn = _dx_through_weight(dpre, W)
        # the residual branch's gradient of the same h (left by _LinearRes.backward, which ran first) is added inside the
        # LayerNorm backward kernel instead of by an autograd accumulation kernel
        dres = ctx.link.pop("dres", None) if ctx.link is not None else None
        dx = ops.layernorm_bwd_into(dn, x2, mean, rstd, ln_w, dg, dbeta, dres=dres)
        return dx.view(ctx.shape), rg, rbeta, rW, rb, None, None, None, None


class _LinearRes(Function):
    """y = res + dropout(a W^T + b) — attention out-projection and FFN2 with the residual add
    (torch: x + dropout1(sa_block(x)), x + dropout3(ff_block(x)))."""

    @staticmethod
    def forward(ctx, a, W, b, res, sink=None, drop=None, link=None):
        a2 = a.reshape(-1, a.shape[-1])
        ctx.save_for_backward(a2, W)
        ctx.shape = a.shape
        ctx.drop = drop
        ctx.link = link
        ctx.sink = sink if sink is not None else _GradSink()
        res2 = res.reshape(-1, W.shape[0]).contiguous()
        y = _linear(a2, W, b, res=res2, drop=drop)
        return y.view(*a.shape[:-1], W.shape[0])

    @staticmethod
    def backward(ctx, dy):
        a2, W = ctx.saved_tensors
        dy2 = dy.contiguous().view(-1, W.shape[0])
        dym = ops.dropout(dy2, ctx.drop) if ctx.drop is not None else dy2   # gradient of the dropped branch; the residual gets dy
        (dW, rW), (db, rb) = ctx.sink.target(0, W), ctx.sink.target(1, W[:, 0])
        ops.gemm_tn(dym, a2, dW, db)
        da = _dx_through_weight(dym, W)
        if ctx.link is not None:   # h's other consumer is the _LNLinear that shares this link: it adds dy inside its kernel
            ctx.link["dres"] = dy2
            return da.view(ctx.shape), rW, rb, None, None, None, None
        return da.view(ctx.shape), rW, rb, dy, None, None, None


class _Linear(Function):
    """y = a W^T + b (no norm) — K/V projection of the un-normalised memory rows."""

    @staticmethod
    def forward(ctx, a, W, b, sink=None):
        a2 = a.reshape(-1, a.shape[-1]).contiguous()
        ctx.save_for_backward(a2, W)
        ctx.shape = a.shape
        ctx.sink = sink if sink is not None else _GradSink()
        return _linear(a2, W, b).view(*a.shape[:-1], W.shape[0])

    @staticmethod
    def backward(ctx, dy):
        a2, W = ctx.saved_tensors
        dy2 = dy.contiguous().view(-1, W.shape[0])
        (dW, rW), (db, rb) = ctx.sink.target(0, W), ctx.sink.target(1, W[:, 0])
        ops.gemm_tn(dy2, a2, dW, db)
        da = _dx_through_weight(dy2, W) if ctx.needs_input_grad[0] else None
        return (da.view(ctx.shape) if da is not None else None), rW, rb, None


class _SelfAttention(Function):
    """softmax(q k^T / sqrt(hd)) v on a packed (B, T, 3d) q|k|v buffer."""

    @staticmethod
    def forward(ctx, qkv, heads: int, drop=None):
        d = qkv.shape[-1] // 3
        out, lse = ops.attention_lse(qkv[..., :d], qkv[..., d : 2 * d], qkv[..., 2 * d :], heads, drop)
        ctx.save_for_backward(qkv, out, lse)
        ctx.heads = heads
        ctx.drop = drop
        return out

    @staticmethod
    def backward(ctx, dO):
        qkv, out, lse = ctx.saved_tensors
        d = qkv.shape[-1] // 3
        dqkv = torch.empty_like(qkv)
        ops.attention_bwd(qkv[..., :d], qkv[..., d : 2 * d], qkv[..., 2 * d :], out, dO.contiguous(), lse,
                          dqkv[..., :d], dqkv[..., d : 2 * d], dqkv[..., 2 * d :], ctx.heads, ctx.drop)
        return dqkv, None, None


class _CrossAttention(Function):
    """Queries (B, T, d) against packed memory keys|values (B, M, 2d)."""

    @staticmethod
    def forward(ctx, q, kv, heads: int, drop=None):
        d = q.shape[-1]
        out, lse = ops.attention_lse(q, kv[..., :d], kv[..., d:], heads, drop)
        ctx.save_for_backward(q, kv, out, lse)
        ctx.heads = heads
        ctx.drop = drop
        return out

    @staticmethod
    def backward(ctx, dO):
        q, kv, out, lse = ctx.saved_tensors
        d = q.shape[-1]
        dq, dkv = torch.empty_like(q), torch.empty_like(kv)
        ops.attention_bwd(q, kv[..., :d], kv[..., d:], out, dO.contiguous(), lse, dq, dkv[..., :d], dkv[..., d:], ctx.heads, ctx.drop)
        return dq, dkv, None, None


# abs-max words of tensors that cross from a fused stack to the embedding / fc_out nodes around it (the last layer's output, the
# gradient of the first layer's input).  The slot travels WITH the tensor object, as an attribute (weakref to the stack's table,
# address of the tensor's words, address of a free slot of the same table for the node's own small operand): an address-keyed
# registry could hand a reused allocation the stale maximum of a freed tensor.  The consumer reads the attribute
# from the very object it was handed (before any view) and also checks the shape and the tensor's version counter - an in-place
# update after registration (autograd's InputBuffer accumulating into a gradient it holds the last reference to, an in-place hook)
# would leave a stale, too-small maximum behind; anything else takes the block-floating GEMM.  (This pair versions an
# ACTIVATION, for the length of one step: the only read of ``._version`` outside derived.py, whose rule is about weights.)
def _amax_register(t: Tensor, table: Tensor, slot_addr: int, scratch_addr: int) -> None:
    t._sd_amax = (weakref.ref(table), slot_addr, scratch_addr, tuple(t.shape), t._version)


def _amax_lookup(t: Tensor):
    ent = getattr(t, "_sd_amax", None)
    if ent is None or ent[0]() is None or ent[3] != tuple(t.shape) or ent[4] != t._version:
        return None
    return ent[1], ent[2]


def _dw_skinny(dY: Tensor, X: Tensor, dW: Tensor, db, known: Tensor, small: Tensor, ent=None) -> None:
    """dW += dY^T X where one operand (``known``) carries registered abs-max words (``ent``: what _amax_lookup returned for the
    tensor ``known`` is a view of) and the other (``small``) is cheap to scan: the grouped fp16 GEMM with ragged tiles instead
    of the block-floating-point kernel (67 -> ~20 us for the J = 20 gradients)."""
    ok = ent is not None and dY.shape[-1] % 4 == 0 and X.shape[-1] % 4 == 0 and dY.data_ptr() % 16 == 0 and X.data_ptr() % 16 == 0
    if not ok:
        ops.gemm_tn(dY, X, dW, db)
        return
    ops.absmax(small, ent[1])
    ay, ax = (ent[0], ent[1]) if known is dY else (ent[1], ent[0])
    ops.gemm_tn_grouped([(dY, X, dW, db, ay, ax)])


def _embed_dw(x: Tensor, W: Tensor, b: Tensor, dy: Tensor):
    """The embedding's weight and bias gradient from the gradient ``dy`` of its output: (dy as rows, values to hand back to autograd)."""
    d = W.shape[0]
    if W.dim() == 2:
        patches = x.reshape(-1, x.shape[-1])
    else:  # (d, C, p): patch rows in (c, k) order, a layout copy
        _, C, p = W.shape
        B, S, _ = x.shape
        n = S // p
        patches = x[:, : n * p].reshape(B, n, p, C).permute(0, 1, 3, 2).reshape(B * n, C * p).contiguous()
    (dW, db), (rW, rb) = _grad_targets(W, b)
    ent = _amax_lookup(dy) if dy.is_contiguous() else None   # the very tensor the stack's backward produced
    dy2 = dy.contiguous().view(-1, d)
    _dw_skinny(dy2, patches, dW.view(d, patches.shape[1]), db, known=dy2, small=patches, ent=ent)
    return dy2, rW, rb


class _PatchEmbed(Function):
    """Conv1d(kernel = stride = p) (+ bias + positional table); p = 1 is nn.Linear(J -> d).
    The input is data (noisy trajectory / sensor history): no input gradient."""

    @staticmethod
    def forward(ctx, x, W, b, pe):
        ctx.save_for_backward(x, W, b)
        return ops.patch_embed(x.contiguous(), W, b, pe)

    @staticmethod
    def backward(ctx, dy):
        x, W, b = ctx.saved_tensors
        d = W.shape[0]
        dy2, rW, rb = _embed_dw(x, W, b, dy)
        dx = None
        if ctx.needs_input_grad[0]:
            # only the image tokens are a differentiable input (they come from the ResNet): kernel size 1, C = d
            if W.dim() == 3 and W.shape[2] == 1 and W.shape[1] == d:
                dx = _dx_through_weight(dy2, W.view(d, d)).view(x.shape)
            else:
                raise NotImplementedError("input gradient of a patch embedding is only implemented for kernel size 1 with C = hidden_dim")
        return dx, rW, rb, None


class _EmbedHead(Function):
    """The decoder stack's entry as ONE trajectory-owning launch (sd_train_head_fwd): h0 = Linear(J -> 256)(x) + positional rows, and
    - not differentiated here, as in _FusedLayer - n1 = LN1(h0), qkv = n1 Wqkv^T + b of layer 0.  The gradient of h0 goes where
    _PatchEmbed sends it."""

    @staticmethod
    def forward(ctx, x, W, b, pe, n1w, n1b, w_qkv: int, bqkv, amax_n1: int):
        ctx.save_for_backward(x, W, b)
        x = x.contiguous()
        w_emb = ops.pack_weight_traj(W.detach().contiguous())     # (256, J): a 4-us launch per step
        h0, n1, qkv = ops.train_head_fwd(x, w_emb.data_ptr(), b.detach(), pe, (n1w.detach(), n1b.detach()), w_qkv, bqkv.detach(), amax_n1)
        ctx.mark_non_differentiable(n1, qkv)
        return h0, n1, qkv

    @staticmethod
    def backward(ctx, dy, _dn, _dqkv):
        if ctx.needs_input_grad[0]:   # (train_route sends a differentiable x to _PatchEmbed, which raises as well)
            raise NotImplementedError("the denoiser's embedding has no gradient with respect to the noisy trajectory")
        _, rW, rb = _embed_dw(*ctx.saved_tensors, dy)
        return None, rW, rb, None, None, None, None, None, None


class _FcOut(Function):
    """eps = h W^T + b with W (J, d)."""

    @staticmethod
    def forward(ctx, h, W, b):
        h2 = h.reshape(-1, h.shape[-1])
        ctx.save_for_backward(h2, W, b)
        ctx.amax = _amax_lookup(h) if h.is_contiguous() else None   # the stack's output object itself (h2 is then a view of it)
        ctx.shape = h.shape
        return ops.fc_out(h2, W, b).view(*h.shape[:-1], W.shape[0])

    @staticmethod
    def backward(ctx, dy):
        h2, W, b = ctx.saved_tensors
        dy2 = dy.contiguous().view(-1, W.shape[0])
        (dW, db), (rW, rb) = _grad_targets(W, b)
        _dw_skinny(dy2, h2, dW, db, known=h2, small=dy2, ent=ctx.amax)
        dh = ops.small_k_matmul(dy2, W)
        return dh.view(ctx.shape), rW, rb


class _StepTokenFn(Function):
    @staticmethod
    def forward(ctx, steps, freq, token, fixed_order: bool = False):
        ctx.half = token.shape[-1]
        ctx.fixed_order = fixed_order
        ctx.save_for_backward(token)
        return ops.step_token(steps, freq, token)

    @staticmethod
    def backward(ctx, dtok):
        (token,) = ctx.saved_tensors
        (dtoken,), (rtoken,) = _grad_targets(token)
        learned = dtok.contiguous()[:, 0, ctx.half :]   # the learned half is expanded over the batch
        if ctx.fixed_order and ctx.half % 4 == 0:
            # several draws per window: the rows are added in a fixed order first (colsum's atomics take more than two rows in any
            # order) - level by level, groups of up to 32 consecutive rows at a time, so that no thread walks thousands of rows alone;
            # the grouping is a function of the row count only
            learned = learned.contiguous()
            while learned.shape[0] > 1:
                rows = learned.shape[0]
                f = next((f for f in range(min(32, rows), 1, -1) if rows % f == 0), rows)
                learned = ops.expand_rows_bwd(learned, f)
        ops.colsum(learned, dtoken.view(-1))
        return None, None, rtoken, None


class _MSELoss(Function):
    """F.mse_loss(pred, target) with mean reduction (train.py:229)."""

    @staticmethod
    def forward(ctx, pred, target):
        loss, grad = ops.mse_loss(pred.contiguous(), target.contiguous())
        ctx.save_for_backward(grad)
        return loss.view(())

    @staticmethod
    def backward(ctx, gout):
        (grad,) = ctx.saved_tensors
        return grad * gout, None  # gout is the scalar 1.0 of loss.backward()


def mse_loss(pred: Tensor, target: Tensor) -> Tensor:
    return _MSELoss.apply(pred, target)


def step_token_autograd(step_module, steps: Tensor, fixed_order: bool = False) -> Tensor:
    steps = steps.contiguous()
    if steps.dtype not in (torch.int64, torch.float32):
        steps = steps.to(torch.float32 if steps.is_floating_point() else torch.int64)
    return _StepTokenFn.apply(steps, step_module._freq, step_module.token, fixed_order)


def _layer(lp, h, heads, memory=None, ffn_norm=None, dc=None, li: int = 0):
    """One pre-norm layer; ``dc`` (a _DropCall or None) turns on dropout at torch's sites of layer ``li``."""
    def site(kind):
        return dc.site(li, kind) if dc is not None else None

    # In each of the three sub-blocks h has exactly two consumers, the LayerNorm branch and the residual add, and the
    # residual's backward runs first: it hands its gradient to the LayerNorm backward through `link` (fused add).  Only
    # when h itself needs a gradient - otherwise autograd would never run the LayerNorm branch's backward for it.
    def link():
        return {} if h.requires_grad else None

    sa, n1 = lp.self_attn, lp.norm1
    lk = link()
    qkv = _LNLinear.apply(h, n1.weight, n1.bias, sa.in_proj_weight, sa.in_proj_bias, False,
                          _GradSink(n1.weight, n1.bias, sa.in_proj_weight, sa.in_proj_bias), None, lk)
    a = _SelfAttention.apply(qkv, heads, site(SITE_SA_PROBS))
    h = _LinearRes.apply(a, sa.out_proj.weight, sa.out_proj.bias, h, _GradSink(sa.out_proj.weight, sa.out_proj.bias), site(SITE_SA_OUT), lk)
    if memory is not None:
        d = h.shape[-1]
        ca, n2 = lp.multihead_attn, lp.norm2
        w, b = ca.in_proj_weight, ca.in_proj_bias
        lk = link()
        q = _LNLinear.apply(h, n2.weight, n2.bias, w[:d], b[:d], False,
                            _GradSink(n2.weight, n2.bias, (w, slice(0, d)), (b, slice(0, d))), None, lk)
        kv = _Linear.apply(memory, w[d:], b[d:], _GradSink((w, slice(d, 3 * d)), (b, slice(d, 3 * d))))  # memory is NOT layer-normed
        a = _CrossAttention.apply(q, kv, heads, site(SITE_CA_PROBS))
        h = _LinearRes.apply(a, ca.out_proj.weight, ca.out_proj.bias, h, _GradSink(ca.out_proj.weight, ca.out_proj.bias), site(SITE_CA_OUT), lk)
    lk = link()
    u = _LNLinear.apply(h, ffn_norm.weight, ffn_norm.bias, lp.linear1.weight, lp.linear1.bias, True,
                        _GradSink(ffn_norm.weight, ffn_norm.bias, lp.linear1.weight, lp.linear1.bias), site(SITE_FFN_ACT), lk)
    return _LinearRes.apply(u, lp.linear2.weight, lp.linear2.bias, h, _GradSink(lp.linear2.weight, lp.linear2.bias), site(SITE_FFN_OUT), lk)


# ---- fused layers: the row chains of a layer in one launch each (csrc/sd_train_chain.hip) ---------------------------
# Per decoder layer the forward is  attention, chain A (out-projection + residual, LN2 + Q), K/V of the memory, attention,
# chain B (out-projection + residual, LN3 + FFN1 + GELU + FFN2 + residual, the NEXT layer's LN1 + QKV); the backward is
# five chain launches, two attention backward kernels and seven weight-gradient GEMMs.  A layer therefore hands its
# successor (h, LN1(h), qkv); the successor's backward differentiates LN1 / in_proj (they are its parameters).
# Conditions (else the per-operation nodes above run): hidden_dim 64 / 128 / 256, dim_feedforward == hidden_dim, every
# weight owned by a FusedAdamW that keeps its split planes current (train_route).
_DEC_PARAMS = ("norm1.weight", "norm1.bias", "self_attn.in_proj_weight", "self_attn.in_proj_bias", "self_attn.out_proj.weight",
               "self_attn.out_proj.bias", "norm2.weight", "norm2.bias", "multihead_attn.in_proj_weight", "multihead_attn.in_proj_bias",
               "multihead_attn.out_proj.weight", "multihead_attn.out_proj.bias", "norm3.weight", "norm3.bias", "linear1.weight",
               "linear1.bias", "linear2.weight", "linear2.bias")
_ENC_PARAMS = ("norm1.weight", "norm1.bias", "self_attn.in_proj_weight", "self_attn.in_proj_bias", "self_attn.out_proj.weight",
               "self_attn.out_proj.bias", "norm2.weight", "norm2.bias", "linear1.weight", "linear1.bias", "linear2.weight", "linear2.bias")


def _layer_params(lp, decoder: bool) -> list:
    out = []
    for name in (_DEC_PARAMS if decoder else _ENC_PARAMS):
        t = lp
        for part in name.split("."):
            t = getattr(t, part)
        out.append(t)
    return out


def _stack_facts(layers, d: int, decoder: bool):
    """What train_route asks about a stack's weights: (``params_ok``, ``ffn_is_d``, ``block_planes``, the ONE store that keeps planes for all
    of its matrices - the one that can keep their trajectory-order planes too - or None)."""
    P = [t for lp in layers for t in _layer_params(lp, decoder)]
    mats = [t for t in P if t.dim() == 2]
    params_ok = (bool(layers) and all(t.is_cuda and t.dtype == torch.float32 for t in P)
                 and all(t.shape[1] == d and t.shape[0] % d == 0 for t in mats))
    # (the planes of a block and of its transpose are packed and retired together: one lookup answers for both)
    block_planes = params_ok and all(_packed_weight(t) is not None for t in mats)
    stores = {id(s): s for s in map(planes_of, mats)} if block_planes else {}
    return params_ok, all(lp.linear1.weight.shape[0] == d for lp in layers), block_planes, next(iter(stores.values())) if len(stores) == 1 else None


class TrainRoute(NamedTuple):
    stack: str          # "per_op": the per-operation nodes above; "chains": _fused_stack
    embed_head: bool    # the decoder's embedding + LN1 + QKV of layer 0 as one trajectory-owning launch (_EmbedHead)
    traj_layers: bool   # every decoder layer's forward as one trajectory-owning launch (sd_train_layer_fwd)


def train_route(*, decoder: bool, d: int, heads: int, T: int, M: int, J: int, ffn_is_d: bool, params_ok: bool, block_planes: bool,
                traj_planes: bool, x_differentiable: bool, layer_fwd_ok=None) -> TrainRoute:
    """Which kernels run for a layer stack: decided once per forward, here, from plain facts (DESIGN.md has the table).  ``M``: memory rows
    including the step token (0: an encoder); ``params_ok``: at least one layer and every layer parameter CUDA fp32 of the expected shape;
    ``block_planes`` / ``traj_planes``: a FusedAdamW keeps current block planes (and their transposes) for every matrix / can keep
    trajectory-order planes for the matrices the two flags need.  The callers' ``traj_planes`` carries three things this function does not
    see: ONE optimizer owns every matrix of the stack (a stack split over two runs as row chains), x is on the GPU, and the embedding
    weight is 2-D (always, for the decoder's nn.Linear).  The flags are independent: d = 256 with 17 memory rows enters through
    the head launch and runs its layers as row chains.  SD_TRAIN_FUSED=0 / SD_TRAIN_TRAJ=0 (A/B runs) are read here and nowhere else.
    ``layer_fwd_ok`` stands in for ops.train_layer_fwd_ok (d 256, 4 heads, 1 <= T <= 100, 1 <= M <= 16) where the library is not loaded."""
    if not (os.environ.get("SD_TRAIN_FUSED", "1") != "0" and d in (64, 128, 256) and params_ok and ffn_is_d and block_planes):
        return TrainRoute("per_op", False, False)
    traj = decoder and traj_planes and os.environ.get("SD_TRAIN_TRAJ", "1") != "0"
    return TrainRoute("chains",
                      traj and not x_differentiable and d == 256 and J % 4 == 0 and 4 <= J <= 32 and T <= 100 and heads == 4,
                      traj and M > 0 and bool((layer_fwd_ok or ops.train_layer_fwd_ok)(d, heads, T, M)))


def _traj_slices(layers, route: TrainRoute) -> dict:
    """{name: (W, first row, rows)} of every matrix the trajectory launches of a decoder stack read, in launch order - and of no other (each
    registered slice is pack work per step): "head", layer 0's in-projection; per layer li, under (li, field of sd_train_layer_fwd_args),
    Wo, the query rows of Wc, Woc, W1, W2 and the successor's in-projection."""
    d = 256
    out = {"head": (layers[0].self_attn.in_proj_weight, 0, 3 * d)} if route.embed_head else {}
    for li, lp in enumerate(layers if route.traj_layers else ()):
        out.update({(li, "w_o"): (lp.self_attn.out_proj.weight, 0, d), (li, "w_q"): (lp.multihead_attn.in_proj_weight, 0, d),
                    (li, "w_oc"): (lp.multihead_attn.out_proj.weight, 0, d), (li, "w_1"): (lp.linear1.weight, 0, d), (li, "w_2"): (lp.linear2.weight, 0, d)})
        if li + 1 < len(layers):
            out[li, "w_n"] = (layers[li + 1].self_attn.in_proj_weight, 0, 3 * d)
    return out


# abs-max words of a layer (row li of the stack's int32 table; bits of max |x|, atomically max-ed by the chains' row passes):
# the per-tensor scales of the grouped weight-gradient GEMM
AMAX_WORDS = 64   # SD_AMAX_WORDS: the producers spread their atomics over this many words per tensor
(_AX_N1, _AX_ASA, _AX_N2, _AX_ACA, _AX_NF, _AX_U, _AX_DY2, _AX_DPRE, _AX_DYC, _AX_DQ, _AX_DYS, _AX_DQKV, _AX_DKV, _AX_OUT, _AX_SCR,
 _AX_MEM, _AX_DX, _AX_SCR2, _AX_TOK, _AX_DKT) = range(20)   # _AX_OUT / _AX_DX: the layer's output / its input gradient (for fc_out / the
_AX_SLOTS = 20                             # embedding, with a scratch slot each for their small operand); _AX_MEM: the memory (row 0);
                                           # shared draws: _AX_TOK the step tokens (row 0), _AX_DKT the gradient of their K | V


def _ax(amax: Tensor, layer: int, slot: int) -> int:
    """Address of abs-max word ``slot`` of row ``layer`` of a stack's table."""
    return amax.data_ptr() + 4 * AMAX_WORDS * (layer * _AX_SLOTS + slot)


class _FusedCfg:
    __slots__ = ("heads", "dc", "li", "decoder", "next_ln", "next_w", "next_b", "amax", "tw", "draws")

    def __init__(self, heads, dc, li, decoder, nxt, amax, tw=None, draws: int = 1):
        self.heads, self.dc, self.li, self.decoder, self.amax = heads, dc, li, decoder, amax
        self.draws = draws   # > 1: `memory` holds B / draws contexts, the step tokens come beside it (the shared cross-attention)
        self.tw = tw   # the plane addresses of sd_train_layer_fwd (train_route's traj_layers), else None: attention + row chains
        if nxt is not None:
            self.next_ln = (nxt.norm1.weight.detach(), nxt.norm1.bias.detach())
            self.next_w, self.next_b = nxt.self_attn.in_proj_weight.detach(), nxt.self_attn.in_proj_bias.detach()
        else:
            self.next_ln = self.next_w = self.next_b = None

    def site(self, kind: int) -> int:
        return self.dc.site(self.li, kind)[2] if self.dc is not None else 0

    def ax(self, idx: int, layer_offset: int = 0) -> int:
        """Address of abs-max word ``idx`` of this layer (or of the next one)."""
        return _ax(self.amax, self.li + layer_offset, idx)

    def drop(self, kind: int):
        return self.dc.site(self.li, kind) if self.dc is not None else None

    @property
    def p(self) -> float:
        return self.dc.p if self.dc is not None else 0.0

    @property
    def seed(self) -> int:
        return self.dc.seed if self.dc is not None else 0


def _new(*shape, like: Tensor) -> Tensor:
    return torch.empty(*shape, dtype=torch.float32, device=like.device)


# The memory side of a decoder layer - K/V projection of 11 rows per trajectory, its dX, the abs-max of dkv - is 44 panels per
# launch: 12 launches of ~17 us per step that leave five CUs in six idle.  They run on a second stream (a parallel branch of the
# captured graph) beside the 400-panel chains of the trajectory rows and are joined where their results are needed.
_MEM_SIDE: dict = {}


def _mem_side(device):
    s = _MEM_SIDE.get(device)
    if s is None:
        s = _MEM_SIDE[device] = torch.cuda.Stream(device=device)
    return s


TRAJ_LAYERS = [0]   # decoder layers whose forward ran as ONE trajectory-owning launch (tests assert which path ran)


class _FusedLayer(Function):
    """One pre-norm transformer layer (nn.TransformerDecoderLayer with memory, nn.TransformerEncoderLayer without) given
    (h, LN1(h), qkv = LN1(h) Wqkv^T + b); returns (h', LN1'(h'), qkv') for the next layer (empty tensors after the last)."""

    @staticmethod
    def forward(ctx, h, n1, qkv, memory, tok, cfg: _FusedCfg, *P):
        B, T, d = h.shape
        R = B * T
        dec, last = cfg.decoder, cfg.next_w is None
        heads, p, seed = cfg.heads, cfg.p, cfg.seed
        if dec:
            (n1w, n1b, Wqkv, bqkv, Wo, bo, n2w, n2b, Wc, bc, Woc, boc, nfw, nfb, W1, b1, W2, b2) = P
        else:
            (n1w, n1b, Wqkv, bqkv, Wo, bo, nfw, nfb, W1, b1, W2, b2) = P
        h = h.contiguous()
        if dec:   # the memory's K/V projection beside the self-attention and chain A
            M = memory.shape[1]
            Bm = memory.shape[0]   # B, or the B / draws contexts the draws share (tok: their step tokens (B, 1, d); M then counts context rows)
            kv = _new(Bm, M, 2 * d, like=h)
            kvt = _new(B, 1, 2 * d, like=h) if tok is not None else None
            side = _mem_side(h.device)
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                ops.linear_packed(memory.reshape(Bm * M, d), _packed_weight(Wc, 1), 2 * d, bc[d:], out=kv.view(Bm * M, 2 * d))
                if tok is not None:
                    ops.linear_packed(tok.reshape(B, d), _packed_weight(Wc, 1), 2 * d, bc[d:], out=kvt.view(B, 2 * d))
            h1, n2, q = _new(B, T, d, like=h), _new(R, d, like=h), _new(B, T, d, like=h)
        h2, nf, pre, u, h3 = _new(B, T, d, like=h), _new(R, d, like=h), _new(R, d, like=h), _new(R, d, like=h), _new(B, T, d, like=h)
        nn1, qkv2 = (_new(0, like=h), _new(0, like=h)) if last else (_new(R, d, like=h), _new(B, T, 3 * d, like=h))
        ax_out = cfg.ax(_AX_OUT) if last else None   # the stack's output feeds fc_out (decoder): its weight gradient needs this abs-max
        if cfg.tw is not None:
            # ---- ONE launch for the whole layer forward: a workgroup per trajectory (csrc/sd_train_traj.hip) ----
            a_sa, a_ca, lse_sa, lse_ca = _new(B, T, d, like=h), _new(B, T, d, like=h), _new(B, heads, T, like=h), _new(B, heads, T, like=h)
            torch.cuda.current_stream().wait_stream(side)
            TRAJ_LAYERS[0] += 1
            ops.train_layer_fwd(
                B, T, M, heads,
                tensors=dict(h=h, qkv=qkv, a_sa=a_sa, lse_sa=lse_sa, h1=h1, n2=n2, q=q, kv=kv, a_ca=a_ca, lse_ca=lse_ca, h2=h2, nf=nf, pre=pre, u=u,
                             h3=h3, nn1=None if last else nn1, qkv2=None if last else qkv2,
                             b_o=bo, b_q=bc, b_oc=boc, b_1=b1, b_2=b2, b_n=cfg.next_b, n2_w=n2w, n2_b=n2b, n3_w=nfw, n3_b=nfb,
                             nn_w=None if last else cfg.next_ln[0], nn_b=None if last else cfg.next_ln[1]),
                weights=cfg.tw, p=p, seed=seed, sites=tuple(cfg.site(k) for k in range(6)),   # SITE_* in their own order
                amax=(cfg.ax(_AX_ASA), cfg.ax(_AX_N2), cfg.ax(_AX_ACA), cfg.ax(_AX_NF), cfg.ax(_AX_U), None if last else cfg.ax(_AX_N1, 1), ax_out))
        else:
            a_sa, lse_sa = ops.attention_lse(qkv[..., :d], qkv[..., d : 2 * d], qkv[..., 2 * d :], heads, cfg.drop(SITE_SA_PROBS))
            if dec:
                ops.train_fwd_chain(R, d, h, a=a_sa, wo=_packed_weight(Wo), bo=bo, h_out=h1, nln=(n2w, n2b), nn_out=n2,
                                    wn=_packed_weight(Wc), bn=bc, y_out=q, n_next=1, p=p, seed=seed, sites=(cfg.site(SITE_SA_OUT), 0, 0),
                                    amax=(cfg.ax(_AX_ASA), None, None, cfg.ax(_AX_N2)))
                torch.cuda.current_stream().wait_stream(side)
                if tok is not None:
                    a_ca, lse_ca = ops.train_xattn_shared_fwd(q, kv, kvt, heads, cfg.draws, cfg.drop(SITE_CA_PROBS))
                else:
                    a_ca, lse_ca = ops.attention_lse(q, kv[..., :d], kv[..., d:], heads, cfg.drop(SITE_CA_PROBS))
                a_in, w_in, b_in, h_res, site_out, ax_a = a_ca, Woc, boc, h1, cfg.site(SITE_CA_OUT), _AX_ACA
            else:
                a_in, w_in, b_in, h_res, site_out, ax_a = a_sa, Wo, bo, h, cfg.site(SITE_SA_OUT), _AX_ASA
            nxt = {} if last else dict(nln=cfg.next_ln, nn_out=nn1, wn=_packed_weight(cfg.next_w), bn=cfg.next_b, y_out=qkv2, n_next=3)
            ops.train_fwd_chain(R, d, h_res, a=a_in, wo=_packed_weight(w_in), bo=b_in, h_out=h2, ln=(nfw, nfb), n_out=nf,
                                w1=_packed_weight(W1), b1=b1, pre=pre, u=u, w2=_packed_weight(W2), b2=b2, h2_out=h3, p=p, seed=seed,
                                sites=(site_out, cfg.site(SITE_FFN_ACT), cfg.site(SITE_FFN_OUT)),
                                amax=(cfg.ax(ax_a), cfg.ax(_AX_NF), cfg.ax(_AX_U), cfg.ax(_AX_N1, 1), ax_out), **nxt)
        if last:
            _amax_register(h3, cfg.amax, ax_out, cfg.ax(_AX_SCR))
        ctx.cfg = cfg
        ctx.set_materialize_grads(False)   # LN1'(h') and qkv' carry no gradient: autograd would hand zeros of their size to backward
        ctx.save_for_backward(h, n1, qkv, memory if dec else None, a_sa, lse_sa, h2, nf, pre, u, *((h1, n2, q, kv, a_ca, lse_ca, tok, kvt) if dec else ()), *P)
        ctx.mark_non_differentiable(nn1, qkv2)
        return h3, nn1, qkv2

    @staticmethod
    def backward(ctx, dh3, _dn, _dqkv):
        cfg = ctx.cfg
        dec, heads, p, seed = cfg.decoder, cfg.heads, cfg.p, cfg.seed
        sv = ctx.saved_tensors
        h, n1, qkv, memory, a_sa, lse_sa, h2, nf, pre, u = sv[:10]
        n_c = 8 if dec else 0   # the cross-attention's tensors
        saved_c, P = sv[10 : 10 + n_c], sv[10 + n_c :]
        B, T, d = h.shape
        R = B * T
        if dec:
            (n1w, n1b, Wqkv, bqkv, Wo, bo, n2w, n2b, Wc, bc, Woc, boc, nfw, nfb, W1, b1, W2, b2) = P
            h1, n2, q, kv, a_ca, lse_ca, tok, kvt = saved_c
        else:
            (n1w, n1b, Wqkv, bqkv, Wo, bo, nfw, nfb, W1, b1, W2, b2) = P
        G, back = _grad_targets(*P)
        g = dict(zip(_DEC_PARAMS if dec else _ENC_PARAMS, G))
        nf_name = "norm3" if dec else "norm2"
        wT = lambda W, blk=0: _packed_weight(W, blk, transposed=True)   # noqa: E731
        if dh3 is None:   # (gradients are not materialised: an unused layer output)
            dh3 = torch.zeros_like(h)
        dh3 = dh3.contiguous()
        dh3_2 = dh3.view(R, d)

        # feed-forward block: dy -> mask -> W2^T -> gelu' o mask -> W1^T -> LayerNorm backward (+ dy)
        dym, dpre, dh2 = (_new(R, d, like=h) if p > 0 else dh3_2), _new(R, d, like=h), _new(B, T, d, like=h)
        ops.train_bwd_chain(R, d, dh3_2, wT(W2), dh2, dym=dym if p > 0 else None, pre=pre, dpre=dpre, wt1=wT(W1), x=h2, ln_w=nfw,
                            dres=dh3, dg=g[nf_name + ".weight"], db=g[nf_name + ".bias"], p=p, seed=seed,
                            sites=(cfg.site(SITE_FFN_OUT), cfg.site(SITE_FFN_ACT)), amax=(cfg.ax(_AX_DY2), cfg.ax(_AX_DPRE)))
        # the weight gradients of the layer: one grouped launch at the end (hidden_dim a multiple of 128), else one each
        grouped = d % 128 == 0
        dws = [(dym, u, g["linear2.weight"], g["linear2.bias"], cfg.ax(_AX_DY2), cfg.ax(_AX_U)),
               (dpre, nf, g["linear1.weight"], g["linear1.bias"], cfg.ax(_AX_DPRE), cfg.ax(_AX_NF))]

        dmem = dtok = None
        if dec:
            # cross-attention block
            dym, da = (_new(R, d, like=h) if p > 0 else dh2.view(R, d)), _new(B, T, d, like=h)
            ops.train_bwd_chain(R, d, dh2.view(R, d), wT(Woc), da, dym=dym if p > 0 else None, p=p, seed=seed, sites=(cfg.site(SITE_CA_OUT), 0),
                                amax=(cfg.ax(_AX_DYC), None))
            dws.append((dym, a_ca.view(R, d), g["multihead_attn.out_proj.weight"], g["multihead_attn.out_proj.bias"], cfg.ax(_AX_DYC),
                        cfg.ax(_AX_ACA)))
            if tok is not None:   # dkv: summed over the draws of a context, in draw order
                dq, dkv, dkvt = ops.train_xattn_shared_bwd(q, kv, kvt, a_ca, da, lse_ca, heads, cfg.draws, cfg.drop(SITE_CA_PROBS))
            else:
                dq, dkv = torch.empty_like(q), torch.empty_like(kv)
                ops.attention_bwd(q, kv[..., :d], kv[..., d:], a_ca, da, lse_ca, dq, dkv[..., :d], dkv[..., d:], heads, cfg.drop(SITE_CA_PROBS))
            M, Bm = memory.shape[1], memory.shape[0]
            gWc, gbc = g["multihead_attn.in_proj_weight"], g["multihead_attn.in_proj_bias"]
            if ctx.needs_input_grad[3]:   # (the learned half of the step token sits in the memory)
                dmem = _new(*memory.shape, like=h)
            mside = _mem_side(h.device)
            mside.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(mside):
                if grouped:
                    ops.absmax(dkv.view(Bm * M, 2 * d), cfg.ax(_AX_DKV))
                    dws.append((dkv.view(Bm * M, 2 * d), memory.reshape(Bm * M, d), gWc[d:], gbc[d:], cfg.ax(_AX_DKV), _ax(cfg.amax, 0, _AX_MEM)))
                else:
                    ops.gemm_tn(dkv.view(Bm * M, 2 * d), memory.reshape(Bm * M, d), gWc[d:], gbc[d:])
                if dmem is not None:   # both column passes in one launch
                    ops.train_bwd_chain(Bm * M, d, dkv.view(Bm * M, 2 * d), wT(Wc, 1), dmem.view(Bm * M, d), passes=2)
                if tok is not None:   # the second key segment: the same weight block's gradient from the B token rows
                    if grouped:
                        ops.absmax(dkvt.view(B, 2 * d), cfg.ax(_AX_DKT))
                        dws.append((dkvt.view(B, 2 * d), tok.reshape(B, d), gWc[d:], gbc[d:], cfg.ax(_AX_DKT), _ax(cfg.amax, 0, _AX_TOK)))
                    else:
                        ops.gemm_tn(dkvt.view(B, 2 * d), tok.reshape(B, d), gWc[d:], gbc[d:])
                    if ctx.needs_input_grad[4]:
                        dtok = _new(B, 1, d, like=h)
                        ops.train_bwd_chain(B, d, dkvt.view(B, 2 * d), wT(Wc, 1), dtok.view(B, d), passes=2)
            dh1 = _new(B, T, d, like=h)
            ops.train_bwd_chain(R, d, dq.view(R, d), wT(Wc), dh1, x=h1, ln_w=n2w, dres=dh2, dg=g["norm2.weight"], db=g["norm2.bias"],
                                amax=(cfg.ax(_AX_DQ), None))
            dws.append((dq.view(R, d), n2, gWc[:d], gbc[:d], cfg.ax(_AX_DQ), cfg.ax(_AX_N2)))
            dres = dh1
        else:
            dres = dh2

        # self-attention block
        dym, da = (_new(R, d, like=h) if p > 0 else dres.view(R, d)), _new(B, T, d, like=h)
        ops.train_bwd_chain(R, d, dres.view(R, d), wT(Wo), da, dym=dym if p > 0 else None, p=p, seed=seed, sites=(cfg.site(SITE_SA_OUT), 0),
                            amax=(cfg.ax(_AX_DYS), None))
        dws.append((dym, a_sa.view(R, d), g["self_attn.out_proj.weight"], g["self_attn.out_proj.bias"], cfg.ax(_AX_DYS), cfg.ax(_AX_ASA)))
        dqkv = torch.empty_like(qkv)
        ops.attention_bwd(qkv[..., :d], qkv[..., d : 2 * d], qkv[..., 2 * d :], a_sa, da, lse_sa, dqkv[..., :d], dqkv[..., d : 2 * d],
                          dqkv[..., 2 * d :], heads, cfg.drop(SITE_SA_PROBS))
        dh = _new(B, T, d, like=h)
        ops.train_bwd_chain(R, d, dqkv.view(R, 3 * d), wT(Wqkv), dh, passes=3, x=h, ln_w=n1w, dres=dres, dg=g["norm1.weight"],
                            db=g["norm1.bias"], amax=(cfg.ax(_AX_DQKV), None, cfg.ax(_AX_DX) if cfg.li == 0 else None))
        if cfg.li == 0:   # the gradient of the stack's input feeds the embedding's weight gradient
            _amax_register(dh, cfg.amax, cfg.ax(_AX_DX), cfg.ax(_AX_SCR2))
        dws.append((dqkv.view(R, 3 * d), n1, g["self_attn.in_proj_weight"], g["self_attn.in_proj_bias"], cfg.ax(_AX_DQKV), cfg.ax(_AX_N1)))
        if dec:
            torch.cuda.current_stream().wait_stream(mside)   # dmem and the abs-max of dkv
        if grouped:
            ops.gemm_tn_grouped(dws)
        else:
            for dY, X, dW, db, _, _ in dws:
                ops.gemm_tn(dY, X, dW, db)
        return (dh, None, None, dmem, dtok, None) + tuple(back)


FUSED_STACKS = [0]   # how many layer stacks went through the fused path (tests assert that it is the path that ran)


def _fused_stack(layers, h, heads: int, memory, dc, decoder: bool, hooks: bool, route: TrainRoute, store=None, embed=None, tokens=None,
                 draws: int = 1) -> Tensor:
    """``embed`` = (x, gen) with route.embed_head: the stack starts from the raw trajectory - embedding, LayerNorm 1 and the Q | K | V
    projection of layer 0 in one trajectory-owning launch (_EmbedHead) - instead of from an embedded ``h``.
    ``tokens`` (B, 1, d) with ``draws`` > 1: ``memory`` holds the B / draws contexts WITHOUT the step tokens; every layer projects both
    segments and runs the shared cross-attention (csrc/sd_train_shared.hip)."""
    FUSED_STACKS[0] += 1
    lp0, L = layers[0], len(layers)
    dev = embed[0].device if embed is not None else h.device
    d = lp0.norm1.weight.shape[0]
    amax = torch.zeros(L + 1, _AX_SLOTS, AMAX_WORDS, dtype=torch.int32, device=dev)
    if memory is not None and d % 128 == 0:
        ops.absmax(memory.reshape(-1, d), _ax(amax, 0, _AX_MEM))
        if tokens is not None:
            ops.absmax(tokens.reshape(-1, d), _ax(amax, 0, _AX_TOK))
    # the trajectory launches' planes: every slice of the stack in one request, so no address is resolved before a later registration grows the buffer
    slices = _traj_slices(layers, route)
    tw = dict(zip(slices, store.traj_planes(slices.values()))) if slices else {}
    if embed is not None:
        x, gen = embed
        pe = gen.positional_encoding.pe[0, : x.shape[1]].contiguous()
        h, n1, qkv = _EmbedHead.apply(x, gen.embedding.weight, gen.embedding.bias, pe, lp0.norm1.weight, lp0.norm1.bias, tw["head"], lp0.self_attn.in_proj_bias,
                                      _ax(amax, 0, _AX_N1))
        B, T, d = h.shape
    else:
        B, T, d = h.shape
        h = h.contiguous()
        with torch.no_grad():
            n1, qkv = _new(B * T, d, like=h), _new(B, T, 3 * d, like=h)
            ops.train_fwd_chain(B * T, d, h.detach(), nln=(lp0.norm1.weight, lp0.norm1.bias), nn_out=n1,
                                wn=_packed_weight(lp0.self_attn.in_proj_weight), bn=lp0.self_attn.in_proj_bias, y_out=qkv, n_next=3,
                                amax=(None, None, None, _ax(amax, 0, _AX_N1)))
    for li, lp in enumerate(layers):
        if hooks:
            _layer_input_hook(h, li)
        # traj_layers is a property of the stack: every layer passes the same shape test, and "chains" already required planes for every layer
        lw = {k: tw.get((li, k)) for k in ("w_o", "w_q", "w_oc", "w_1", "w_2", "w_n")} if route.traj_layers else None
        cfg = _FusedCfg(heads, dc, li, decoder, layers[li + 1] if li + 1 < L else None, amax, lw, draws)
        h, n1, qkv = _FusedLayer.apply(h, n1, qkv, memory, tokens, cfg, *_layer_params(lp, decoder))
    return h


class _ExpandRows(Function):
    """c (C, ...) -> (C K, ...), row b = c[b // K]; the backward sums each group of K rows in draw order (one small kernel each way)."""

    @staticmethod
    def forward(ctx, c, draws: int):
        ctx.draws = draws
        return ops.expand_rows(c.contiguous(), draws)

    @staticmethod
    def backward(ctx, dy):
        return ops.expand_rows_bwd(dy.contiguous(), ctx.draws), None


def expand_context(c: Tensor, draws: int) -> Tensor:
    return _ExpandRows.apply(c, draws)


SHARED_STACKS = [0]       # decoder stacks (draws > 1) whose draws shared the projected context: the shared cross-attention kernels ran
EXPANDED_CONTEXTS = [0]   # decoder stacks (draws > 1) whose context was expanded to one copy per draw: the existing path ran


def denoiser_forward_autograd(gen, x: Tensor, memory: Tensor, draws: int = 1, tokens: Optional[Tensor] = None) -> Tensor:
    """Differentiable DiffusionActionGenerator.forward (reference ml/model/decoder.py:38-54).
    ``draws`` = K > 1 (training with several noise draws per window): ``x`` holds C K trajectories, ``memory`` the C contexts (C, Mc, d)
    without their step tokens and ``tokens`` (C K, 1, d) those; trajectory b reads context b // K and token b.  Where the stack runs as
    row chains and the shared cross-attention takes the shape, K | V of the context are projected once per context (SHARED_STACKS);
    anywhere else the context is expanded by ``expand_context`` and the call is the one with ``draws`` = 1 (EXPANDED_CONTEXTS)."""
    T = x.shape[1]
    pe = gen.positional_encoding.pe[0, :T].contiguous()
    memory = memory.contiguous()
    dc = gen.dropout.for_call(gen.training)
    layers = list(gen.transformer_decoder.layers)
    W = gen.embedding.weight
    params_ok, ffn_is_d, block_planes, store = _stack_facts(layers, W.shape[0], decoder=True)
    M = memory.shape[1] + (1 if draws > 1 else 0)
    route = train_route(decoder=True, d=W.shape[0], heads=gen.num_heads, T=T, M=M, J=x.shape[-1], ffn_is_d=ffn_is_d, params_ok=params_ok,
                        block_planes=block_planes, traj_planes=store is not None and x.is_cuda and W.dim() == 2, x_differentiable=x.requires_grad)
    if draws > 1:
        tokens = tokens.contiguous()
        # (SD_TRAIN_SHARED=0, A/B runs: the expanding route everywhere - read here and nowhere else)
        if (route.stack == "chains" and os.environ.get("SD_TRAIN_SHARED", "1") != "0"
                and ops.train_xattn_shared_ok(W.shape[0], gen.num_heads, T, memory.shape[1])):
            SHARED_STACKS[0] += 1
            route = route._replace(traj_layers=False)   # (a layer launch owns one trajectory AND its memory)
        else:
            EXPANDED_CONTEXTS[0] += 1
            memory, tokens, draws = torch.cat([expand_context(memory, draws), tokens], dim=1), None, 1
    h = None if route.embed_head else _PatchEmbed.apply(x, W, gen.embedding.bias, pe)
    if route.stack == "chains":
        h = _fused_stack(layers, h, gen.num_heads, memory, dc, decoder=True, hooks=True, route=route, store=store,
                         embed=(x, gen) if route.embed_head else None, tokens=tokens, draws=draws)
    else:
        for li, lp in enumerate(layers):
            _layer_input_hook(h, li)
            h = _layer(lp, h, gen.num_heads, memory=memory, ffn_norm=lp.norm3, dc=dc, li=li)
    return _FcOut.apply(h, gen.fc_out.weight, gen.fc_out.bias)


def encoder_forward_autograd(enc, x: Tensor) -> Tensor:
    """Differentiable BaseEncoder.forward (reference ml/model/encoder/base.py:41-53)."""
    n = x.shape[1] // enc.patch_size
    pe = enc.positional_encoding.pe[0, :n].contiguous()
    h = _PatchEmbed.apply(x, enc.embedding.weight, enc.embedding.bias, pe)
    dc = enc.dropout.for_call(enc.training)
    layers = list(enc.transformer_encoder.layers)
    params_ok, ffn_is_d, block_planes, _ = _stack_facts(layers, h.shape[-1], decoder=False)
    route = train_route(decoder=False, d=h.shape[-1], heads=enc.num_heads, T=n, M=0, J=x.shape[-1], ffn_is_d=ffn_is_d, params_ok=params_ok,
                        block_planes=block_planes, traj_planes=False, x_differentiable=x.requires_grad)
    if route.stack == "chains":
        return _fused_stack(layers, h, enc.num_heads, None, dc, decoder=False, hooks=False, route=route)
    for li, lp in enumerate(layers):
        h = _layer(lp, h, enc.num_heads, memory=None, ffn_norm=lp.norm2, dc=dc, li=li)
    return h


def broadcast_parameters(optimizer: FusedAdamW, model=None, src: int = 0, group=None) -> None:
    """Data-parallel start: every rank takes rank ``src``'s replica - the optimizer's flat parameter buffer and both
    moment buffers (three broadcasts), plus every tensor of ``model`` the optimizer does not own (buffers such as
    ``mean`` / ``std`` and BatchNorm statistics, frozen parameters).  Without it replicas that were initialised from
    different RNG states would apply the averaged gradient to different weights and drift apart silently."""
    import torch.distributed as dist

    if not dist.is_initialized() or dist.get_world_size(group) <= 1:
        return
    ema = getattr(optimizer, "flat_ema", None)   # afterwards a deterministic function of identical parameters: no exchange of its own
    for buf in (optimizer.flat_param, optimizer.flat_m, optimizer.flat_v) + (() if ema is None else (ema,)):
        dist.broadcast(buf, src=src, group=group)
    step = torch.tensor([optimizer._step, getattr(optimizer, "ema_updates", 0)], dtype=torch.int64, device=optimizer.flat_param.device)
    dist.broadcast(step, src=src, group=group)
    optimizer._step = int(step[0].item())
    if ema is not None:
        optimizer.ema_updates = int(step[1].item())
    if model is not None:
        lo = optimizer.flat_param.data_ptr()
        hi = lo + 4 * optimizer.flat_param.numel()
        for t in list(model.parameters()) + list(model.buffers()):
            if t.numel() == 0 or lo <= t.data_ptr() < hi:
                continue
            if t.dtype == torch.int64 and t.dim() == 0:   # BatchNorm's num_batches_tracked
                tmp = t.detach().reshape(1).clone()
                dist.broadcast(tmp, src=src, group=group)
                t.data.copy_(tmp.reshape(()))
            else:
                dist.broadcast(t.detach(), src=src, group=group)
    optimizer.refresh_transposes()


def assert_replicas_equal(optimizer: FusedAdamW, group=None) -> None:
    """Data-parallel invariant: every rank holds bit-identical parameters (same start by broadcast, same averaged gradient,
    same deterministic update).  Two scalars per rank (sum and sum of squares of the flat parameter buffer, in fp64) are
    MIN- and MAX-reduced; a difference means the replicas have drifted apart - raise instead of training on silently."""
    import torch.distributed as dist

    if not dist.is_initialized() or dist.get_world_size(group) <= 1:
        return
    p = optimizer.flat_param.double()
    sig = [p.sum(), (p * p).sum()]
    if getattr(optimizer, "flat_ema", None) is not None:
        e = optimizer.flat_ema.double()
        sig += [e.sum(), (e * e).sum()]
    sig = torch.stack(sig)
    lo, hi = sig.clone(), sig.clone()
    dist.all_reduce(lo, op=dist.ReduceOp.MIN, group=group)
    dist.all_reduce(hi, op=dist.ReduceOp.MAX, group=group)
    if not torch.equal(lo, hi):
        raise RuntimeError(f"data-parallel replicas diverged: parameter{' / EMA' if sig.numel() > 2 else ''} checksums differ across ranks "
                           f"({lo.tolist()} .. {hi.tolist()})")


def allreduce_gradients(optimizer: FusedAdamW, world_size: int, group=None) -> None:
    """Data-parallel gradient exchange: ONE sum all-reduce of the flat fp32 gradient buffer
    over RCCL/xGMI (gloo on CPU tests), then the mean.  The reference is single-device."""
    import torch.distributed as dist

    if world_size <= 1:
        return
    dist.all_reduce(optimizer.flat_grad, op=dist.ReduceOp.SUM, group=group)
    optimizer.flat_grad.mul_(1.0 / world_size)


class BucketedAllReduce:
    """Gradient exchange overlapped with the backward: the flat gradient buffer is cut into
    one bucket per decoder layer (fc_out rides with the last layer, whose gradients are complete first) plus one for
    everything else (embedding, step token, context encoders).  ``ready(l)`` - called from a tensor hook when the
    gradient with respect to layer l's INPUT exists, i.e. when every gradient kernel of layer l has been enqueued -
    starts that bucket's asynchronous sum all-reduce (RCCL runs it on its own stream behind the work enqueued so far,
    while the backward of layers l-1 .. 0 keeps the compute stream busy); ``finish()`` reduces the rest, waits for all
    of them and applies the 1 / world mean.  The buckets partition the buffer, so the result equals
    ``allreduce_gradients`` exactly (same sum order per element: one all-reduce each)."""

    def __init__(self, optimizer: FusedAdamW, decoder, world_size: int, group=None):
        self.opt, self.world, self.group = optimizer, world_size, group
        base = optimizer.flat_param.data_ptr()
        layers = list(decoder.transformer_decoder.layers)
        self.ranges = []
        for i, lp in enumerate(layers):
            ps = list(lp.parameters()) + (list(decoder.fc_out.parameters()) if i == len(layers) - 1 else [])
            offs = sorted(((p.data_ptr() - base) // 4, p.numel()) for p in ps)
            lo, hi = offs[0][0], offs[-1][0] + offs[-1][1]
            if hi - lo != sum(n for _, n in offs) or lo < 0 or hi > optimizer.flat_param.numel():
                raise RuntimeError("layer parameters are not one contiguous range of the flat buffer")
            self.ranges.append((lo, hi))
        self.ranges.sort()
        for (a, b), (c, d) in zip(self.ranges, self.ranges[1:]):
            if b != c:
                raise RuntimeError("decoder layers are not adjacent in the flat buffer")
        self.handles, self.done = [], set()

    def ready(self, layer: int) -> None:
        import torch.distributed as dist

        if self.world <= 1 or layer in self.done:
            return
        self.done.add(layer)
        lo, hi = self.ranges[layer]
        self.handles.append(dist.all_reduce(self.opt.flat_grad[lo:hi], op=dist.ReduceOp.SUM, group=self.group, async_op=True))

    def finish(self) -> None:
        import torch.distributed as dist

        if self.world <= 1:
            return
        for l in range(len(self.ranges)):
            self.ready(l)          # a layer whose hook never fired (no gradient path) is reduced here
        n = self.opt.flat_grad.numel()
        lo, hi = self.ranges[0][0], self.ranges[-1][1]
        for a, b in ((0, lo), (hi, n)):
            if b > a:
                self.handles.append(dist.all_reduce(self.opt.flat_grad[a:b], op=dist.ReduceOp.SUM, group=self.group, async_op=True))
        for h in self.handles:
            h.wait()
        self.handles, self.done = [], set()
        self.opt.flat_grad.mul_(1.0 / self.world)


_BUCKETS: Optional[BucketedAllReduce] = None   # the exchange in progress (set by train_step around loss.backward())


def _layer_input_hook(h: Tensor, layer: int) -> None:
    """Fires when the gradient of decoder layer ``layer``'s input exists: its bucket is complete."""
    if _BUCKETS is not None and h.requires_grad:
        h.register_hook(lambda g, l=layer: (_BUCKETS.ready(l) if _BUCKETS is not None else None, None)[1])


def noise_draws(draws) -> int:
    """``draws`` of a training call, validated as the samplers validate theirs (``ops._draws_req``): an int >= 1."""
    return ops._draws_req(draws, 0, None)


def train_step(model, optimizer: FusedAdamW, lr_scheduler, scheduler, joint_targets: Tensor, context=None,
               input_data=None, noise: Optional[Tensor] = None, timesteps: Optional[Tensor] = None,
               world_size: int = 1, generator: Optional[torch.Generator] = None, bucketed: bool = True, draws: int = 1) -> Tensor:
    """One iteration of the reference loop body (train.py:204-240) on already-normalised
    targets.  ``context`` given = the --decoder-pretraining path (train.py:221-224).
    ``draws`` = K > 1 (not in the reference): K (timestep, noise) pairs per window on ONE encoded observation - ``joint_targets`` (C, T, J)
    and the context / ``input_data`` hold C windows, ``noise`` (C K, T, J) and ``timesteps`` (C K,) (drawn from ``generator`` when not
    given) one entry per trajectory, trajectory b belongs to window b // K; the loss is the MSE over all C K trajectories.  Every
    context encoder runs once per window; the result is the step on the K times repeated context.  ``draws`` = 1 is the call without it.
    Data parallel (``world_size`` > 1): the gradient all-reduce runs per decoder layer, overlapped with the rest of the
    backward (``BucketedAllReduce``); ``bucketed=False`` = one all-reduce after it.  Gradient clipping and the non-finite guard
    (``FusedAdamW(max_grad_norm=...)``) live in ``optimizer.step()``, behind the exchange: the norm is that of the reduced gradient,
    every rank computes the same coefficient and takes or skips the step together - no collective of their own."""
    global _BUCKETS
    draws = noise_draws(draws)
    B = joint_targets.shape[0] * draws
    dev = joint_targets.device
    if draws > 1 and timesteps is not None and tuple(timesteps.shape) != (B,):
        raise ValueError(f"timesteps: expected ({B},) = windows x draws entries, got {tuple(timesteps.shape)}")
    if draws > 1 and noise is not None and tuple(noise.shape) != (B,) + tuple(joint_targets.shape[1:]):
        raise ValueError(f"noise: expected {(B,) + tuple(joint_targets.shape[1:])} = (windows x draws, T, J), got {tuple(noise.shape)}")
    optimizer.zero_grad()
    if timesteps is None:
        timesteps = torch.randint(0, scheduler.config["num_train_timesteps"], (B,), device=dev, generator=generator).long()
    if noise is None:
        noise = torch.randn(joint_targets.shape if draws == 1 else (B,) + tuple(joint_targets.shape[1:]), device=dev, generator=generator)
    noisy = scheduler.add_noise(joint_targets if draws == 1 else joint_targets.repeat_interleave(draws, 0), noise, timesteps)
    kw = {} if draws == 1 else {"draws": draws}
    buckets = None
    if world_size > 1 and bucketed:
        buckets = getattr(optimizer, "_buckets", None)
        if buckets is None or buckets.world != world_size:
            buckets = optimizer._buckets = BucketedAllReduce(optimizer, model.diffusion_action_generator, world_size)
    _BUCKETS = buckets            # the forward registers one hook per decoder layer while this is set
    try:
        if context is not None:
            pred = model.forward_with_context(context, noisy, timesteps, **kw)
        else:
            pred = model(input_data, noisy, timesteps, **kw)
        loss = mse_loss(pred, noise)
        loss.backward()
        if buckets is not None:
            buckets.finish()
        else:
            allreduce_gradients(optimizer, world_size)
    finally:
        _BUCKETS = None
    optimizer.step()
    if lr_scheduler is not None:
        lr_scheduler.step()
    return loss.detach()


class GraphedTrainStep:
    """``train_step`` captured into a hipGraph and replayed (decoder-pretraining path or full model, static shapes).

    The B = 256 step is ~120 kernel launches issued from Python through autograd; rocprofv3 shows the GPU idle for
    ~18 % of the step waiting for them.  A replay has no host work beyond one 32-byte upload (36 with a weight EMA).  What changes from step to
    step cannot sit in kernel arguments, which a graph freezes, so it comes from device memory instead:
      * AdamW's scalars (OneCycleLR's lr and cycled beta1, the bias corrections) - ``sd_adamw_step_dev``;
      * with ``FusedAdamW(ema_decay=...)`` the weight of the coming EMA update, a ninth word - ``sd_adamw_ema_step_dev``, same launch;
      * with ``FusedAdamW(max_grad_norm=...)`` the gradient norm, the clipping coefficient and the non-finite guard: the two
        ``sd_grad_norm`` launches write them to device words and ``sd_adamw_clip_step_dev`` reads them there, all three inside the
        captured update (``max_grad_norm`` itself is a frozen argument: constant for a run).  A replay equals the eager step bit for
        bit, and a step with a non-finite gradient leaves the weights as they were without the host being told
        (``optimizer.grad_stats()`` reads the count);
      * the per-step part of the dropout key - ``sd_set_dropout_epoch`` (process-wide; reset by ``close()``);
      * timesteps and noise come from ``generator`` (registered with the graph: torch advances its Philox offset per replay).
    The first ``eager_steps`` calls run the ordinary ``train_step`` (they are real training steps and warm every lazy
    initialisation up); the next call captures, and from then on every call replays.
    Data parallel (``world_size`` > 1): EVERY call is the eager ``train_step`` with its per-layer ``BucketedAllReduce`` - the one
    data-parallel step of this package (``cli train`` runs the same).  Overlapping the exchange with the backward needs the host
    to issue layer l's all-reduce while the GPU still runs the backward of layers l-1 .. 0; a single captured graph cannot
    signal the host or a side stream in mid-replay on this stack (torch refuses external event-record nodes on ROCm,
    tools/exp/graph_event.py), and since the fused row chains (~60 launches per step) the eager step is within 1 % of the
    replay (1 000-step soak: 3.67 vs 3.65 ms).  ``split_update=True`` keeps the round-2 form (graph up to the end of the
    backward, then ONE flat all-reduce and the update) for A/B runs and its parity test."""

    def __init__(self, model, optimizer: FusedAdamW, lr_scheduler, scheduler, world_size: int = 1,
                 generator: Optional[torch.Generator] = None, eager_steps: int = 2, split_update: Optional[bool] = None, draws: int = 1):
        self.model, self.opt, self.lr_sched, self.sched = model, optimizer, lr_scheduler, scheduler
        self.draws = noise_draws(draws)   # (timestep, noise) pairs per window (train_step): the captured shapes are (windows x draws, T, J)
        self.world, self.gen, self.eager_left = world_size, generator, eager_steps
        # data parallel: the eager bucketed step (see the class comment) unless split_update is forced
        self.split = False if split_update is None else bool(split_update)
        self.eager_dp = world_size > 1 and not self.split
        self.graph = None
        dev = optimizer.flat_param.device
        # 7 AdamW scalars + the dropout epoch word (+ with an EMA the weight of the coming EMA update): ONE pinned upload per step
        self.ema = optimizer.flat_ema is not None
        words = 9 if self.ema else 8
        self.hyper = torch.zeros(words, dtype=torch.float32, device=dev)
        self._ring = [torch.zeros(words, dtype=torch.float32).pin_memory() for _ in range(8)]
        self._events = [None] * 8
        self._n = 0
        self._epoch = 0
        self._static = None

    # ---- inputs -------------------------------------------------------------------------
    def _stage(self, targets, context, input_data):
        if self._static is None:
            self._static = {"targets": targets.clone(),
                            "context": None if context is None else [c.clone() for c in context],
                            "input": None if input_data is None else {k: v.clone() for k, v in input_data.items()}}
            return
        st = self._static
        st["targets"].copy_(targets)
        if context is not None:
            for dst, src in zip(st["context"], context):
                dst.copy_(src)
        if input_data is not None:
            for k, v in input_data.items():
                st["input"][k].copy_(v)

    def _upload_hyper(self):
        slot = self._n % len(self._ring)
        if self._events[slot] is not None:
            self._events[slot].synchronize()     # the upload that last used this pinned buffer has run
        host = self._ring[slot]
        self.opt.hyper_for_step(self.opt._step + 1, host)
        self._epoch = (self._epoch + 1) & 0x7FFFFFFF
        host[7:8].view(torch.int32)[0] = self._epoch
        if self.ema:
            host[8] = self.opt.ema_weight_for_step(self.opt.ema_updates)
        self.hyper.copy_(host, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self._events[slot] = ev
        self._n += 1

    def _body(self):
        st = self._static
        K = self.draws
        B = st["targets"].shape[0] * K
        dev = st["targets"].device
        self.opt.zero_grad()
        t = torch.randint(0, self.sched.config["num_train_timesteps"], (B,), device=dev, generator=self.gen).long()
        noise = torch.randn((B,) + tuple(st["targets"].shape[1:]), device=dev, generator=self.gen)
        noisy = self.sched.add_noise(st["targets"] if K == 1 else st["targets"].repeat_interleave(K, 0), noise, t)
        kw = {} if K == 1 else {"draws": K}
        if st["context"] is not None:
            pred = self.model.forward_with_context(st["context"], noisy, t, **kw)
        else:
            pred = self.model(st["input"], noisy, t, **kw)
        loss = mse_loss(pred, noise)
        loss.backward()
        if not self.split:
            self._update()
        return loss.detach()

    def _update(self):
        self.opt.step_from_device_hyper(self.hyper[:7], self.hyper[8:9] if self.ema else None)

    def __call__(self, joint_targets: Tensor, context=None, input_data=None) -> Tensor:
        if self.eager_left > 0 or self.eager_dp:
            self.eager_left = max(self.eager_left - 1, 0)
            return train_step(self.model, self.opt, self.lr_sched, self.sched, joint_targets, context=context,
                              input_data=input_data, world_size=self.world, generator=self.gen, draws=self.draws)
        self._stage(joint_targets, context, input_data)
        if self.graph is None:
            ops.set_dropout_epoch(self.hyper[7:8])
            torch.cuda.synchronize()
            self.graph = torch.cuda.CUDAGraph()
            if self.gen is not None:
                self.graph.register_generator_state(self.gen)
            with torch.cuda.graph(self.graph):
                self._loss = self._body()
        self._upload_hyper()
        self.graph.replay()
        ops.bump_weights_generation()   # the replayed update rewrote the flat parameter buffer without any Python-side hook
        if self.split:
            allreduce_gradients(self.opt, self.world)
            self._update()
        self.opt._step += 1
        self.opt.ema_updates += int(self.ema)
        if self.lr_sched is not None:
            self.lr_sched.step()
        return self._loss

    def close(self) -> None:
        """Detaches the process-wide dropout epoch word (it lives in this object's ``hyper`` buffer)."""
        if self.graph is not None:
            torch.cuda.synchronize()
            ops.set_dropout_epoch(None)
            self.graph = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001 - interpreter shutdown
            pass
