"""Autograd wrappers of the transformer kernels (csrc/kernels/transformer.hip).

On ROCm bf16 tensors they run the hand-written gfx950 kernels; anything else falls back
to the plain PyTorch definition (CPU tests, fp32 tiny models).
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from .._native import kernels
from . import reference as _ref


def _hip_bf16(*ts) -> bool:
    return all(t.is_cuda and t.dtype == torch.bfloat16 for t in ts)


@dataclass(frozen=True)
class Drop:
    """One dropout site of a GPT-2 call (csrc/kernels/dropout_hash.h; twin: ops/reference.py). The mask is a function
    of these values and the coordinates inside the sample, so it does not depend on how a batch is cut into calls."""
    T: int                     # threshold round(256 p), 1..255
    seed: int                  # the run's dropout seed (< 2^63)
    ctr: Optional[torch.Tensor]  # int64 [1] step counter on the compute device (None: 0)
    site: int                  # reference.DROP_SITE_*
    layer: int                 # global layer index h.{i} (0 for the embedding)
    sample0: int = 0           # dataset index of the call's first sample
    head0: int = 0             # global index of the call's first head (attention)

    def kw(self) -> dict:
        """The kernels' keyword arguments."""
        return dict(drop_t=self.T, drop_seed=self.seed, drop_ctr=self.ctr,
                    drop_site_layer=(self.site << 16) | self.layer, sample0=self.sample0)

    def keep(self, B: int, S: int, C: int, device) -> torch.Tensor:
        """[B, S, C] keep mask of an element-wise site, from the torch twin."""
        return _ref.gpt2_site_keep(self.seed, self.ctr, self.site, self.layer, self.sample0, B, S, C, self.T, device)

    @property
    def scale(self) -> float:
        return _ref.dropout_scale(self.T)


def _drop_mul(h, drop: Drop):
    """drop(h) = h * M * 256 / (256 - T) on [B, S, C], plain torch (the fallback path: CPU, fp32)."""
    B, S, C = h.shape
    m = drop.keep(B, S, C, h.device)
    return h * (m.to(torch.float32) * drop.scale).to(h.dtype)


class _LayerNormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b, eps):
        xc = x.contiguous()
        y, mean, rstd = kernels().layernorm_fwd_bf16(xc, w, b, eps)
        ctx.save_for_backward(xc, w, mean, rstd)
        ctx.params = (w, b)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, w, mean, rstd = ctx.saved_tensors
        wp, bp = ctx.params
        if wp.grad is not None and bp.grad is not None and wp.grad.is_contiguous() and bp.grad.is_contiguous():
            # flat-buffer gradients: dw/db are added in place by the reduction kernel
            dx = kernels().layernorm_bwd_bf16_accum(x, w, gy.contiguous(), mean, rstd, wp.grad, bp.grad)
            return dx, None, None, None
        dx, dw, db = kernels().layernorm_bwd_bf16(x, w, gy.contiguous(), mean, rstd)
        return dx, dw.to(w.dtype), db.to(w.dtype), None


def layer_norm(x, w, b, eps: float = 1e-5):
    if _hip_bf16(x, w, b) and x.shape[-1] % 8 == 0 and x.shape[-1] <= 4096:
        return _LayerNormFn.apply(x, w, b, eps)
    return F.layer_norm(x, (x.shape[-1],), w, b, eps)


class _LayerNormPassFn(torch.autograd.Function):
    """(x, LayerNorm(x)) for an x that also feeds a residual path: the backward adds the residual-path gradient inside
    the LayerNorm backward kernel (fp32, rounded once) instead of autograd summing the two bf16 gradients with a
    separate add kernel (GPT-2: each stage's first block)."""

    @staticmethod
    def forward(ctx, x, w, b, eps):
        xc = x.contiguous()
        y, mean, rstd = kernels().layernorm_fwd_bf16(xc, w, b, eps)
        ctx.save_for_backward(xc, w, mean, rstd)
        ctx.params = (w, b)
        return xc.view_as(xc), y

    @staticmethod
    def backward(ctx, g_x, g_y):
        x, w, mean, rstd = ctx.saved_tensors
        wp, bp = ctx.params
        g_x = None if g_x is None else g_x.contiguous()
        if g_y is None:
            return g_x, None, None, None
        if wp.grad is not None and bp.grad is not None and wp.grad.is_contiguous() and bp.grad.is_contiguous():
            d = kernels().layernorm_bwd_bf16_accum(x, w, g_y.contiguous(), mean, rstd, wp.grad, bp.grad, g_x)
            return d, None, None, None
        d, dw, db = kernels().layernorm_bwd_bf16(x, w, g_y.contiguous(), mean, rstd)
        if g_x is not None:
            d = d + g_x
        return d, dw.to(w.dtype), db.to(w.dtype), None


def layer_norm_pass(x, ln: nn.LayerNorm):
    """(x, ln(x)), both differentiable; on ROCm bf16 the two gradients of x meet inside the LayerNorm backward."""
    w, b = ln.weight, ln.bias
    if _hip_bf16(x, w, b) and x.shape[-1] % 8 == 0 and x.shape[-1] <= 4096:
        return _LayerNormPassFn.apply(x, w, b, ln.eps)
    return x, ln(x)


class _AddLayerNormFn(torch.autograd.Function):
    """xs = x + h; y = LayerNorm(xs) in one pass. Backward: dxs = g_xs + LN_bwd(g_y), added inside
    the LayerNorm backward kernel; both addends of the residual get dxs."""

    @staticmethod
    def forward(ctx, x, h, w, b, eps):
        xs, y, mean, rstd = kernels().add_layernorm_fwd_bf16(x.contiguous(), h.contiguous(), w, b, eps)
        ctx.save_for_backward(xs, w, mean, rstd)
        ctx.params = (w, b)
        return xs, y

    @staticmethod
    def backward(ctx, g_xs, g_y):
        xs, w, mean, rstd = ctx.saved_tensors
        wp, bp = ctx.params
        g_xs = None if g_xs is None else g_xs.contiguous()
        if wp.grad is not None and bp.grad is not None and wp.grad.is_contiguous() and bp.grad.is_contiguous():
            d = kernels().layernorm_bwd_bf16_accum(xs, w, g_y.contiguous(), mean, rstd, wp.grad, bp.grad, g_xs)
            return d, d, None, None, None
        d, dw, db = kernels().layernorm_bwd_bf16(xs, w, g_y.contiguous(), mean, rstd)
        if g_xs is not None:
            d = d + g_xs
        return d, d, dw.to(w.dtype), db.to(w.dtype), None


class _AddLayerNormDropFn(torch.autograd.Function):
    """xs = x + drop(h); y = LayerNorm(xs) in one pass (residual dropout, one rounding of the sum). Backward: x gets
    d = g_xs + LN_bwd(g_y); h gets bf16(d * M * scale), rounded from the fp32 d in the same kernel pass. The mask is
    regenerated from the hash, nothing beyond the plain fused add + LayerNorm is saved."""

    @staticmethod
    def forward(ctx, x, h, w, b, eps, drop: Drop):
        xs, y, mean, rstd = kernels().add_layernorm_drop_fwd_bf16(x.contiguous(), h.contiguous(), w, b, eps,
                                                                  **drop.kw())
        ctx.save_for_backward(xs, w, mean, rstd)
        ctx.params, ctx.drop = (w, b), drop
        return xs, y

    @staticmethod
    def backward(ctx, g_xs, g_y):
        xs, w, mean, rstd = ctx.saved_tensors
        wp, bp = ctx.params
        g_xs = None if g_xs is None else g_xs.contiguous()
        if g_y is None:  # (a stage that ends in this sum would use dropout_add instead)
            g_y = torch.zeros_like(xs)
        direct = wp.grad is not None and bp.grad is not None and wp.grad.is_contiguous() and bp.grad.is_contiguous()
        gw = wp.grad if direct else torch.zeros_like(w)
        gb = bp.grad if direct else torch.zeros_like(w)
        d, dh = kernels().layernorm_bwd_bf16_accum_drop(xs, w, g_y.contiguous(), mean, rstd, gw, gb, g_xs,
                                                        **ctx.drop.kw())
        if direct:
            return d, dh, None, None, None, None
        return d, dh, gw, gb, None, None


def add_layer_norm(x, h, ln: nn.LayerNorm, drop: Optional[Drop] = None):
    """(x + h, ln(x + h)): the residual add fused into the LayerNorm pass on ROCm bf16. ``drop``: residual dropout on
    h, (x + drop(h), ln(x + drop(h))), in the same pass."""
    w, b = ln.weight, ln.bias
    if _hip_bf16(x, h, w, b) and x.shape[-1] % 8 == 0 and x.shape[-1] <= 4096 and x.shape == h.shape:
        if drop is not None:
            return _AddLayerNormDropFn.apply(x, h, w, b, ln.eps, drop)
        return _AddLayerNormFn.apply(x, h, w, b, ln.eps)
    xs = x + (h if drop is None else _drop_mul(h, drop))
    return xs, ln(xs)


class _DropoutAddFn(torch.autograd.Function):
    """x + drop(h) where no LayerNorm follows on this stage (HIP, bf16); backward: (g, bf16(g * M * scale))."""

    @staticmethod
    def forward(ctx, x, h, drop: Drop):
        ctx.drop = drop
        return kernels().dropout_add_bf16(x.contiguous(), h.contiguous(), **drop.kw())

    @staticmethod
    def backward(ctx, g):
        g = g.contiguous()
        return g, kernels().dropout_add_bf16(None, g, **ctx.drop.kw()), None


def dropout_add(x, h, drop: Drop):
    """x + drop(h) for [B, S, C] tensors."""
    if _hip_bf16(x, h) and x.shape[-1] % 4 == 0 and x.shape == h.shape:
        return _DropoutAddFn.apply(x, h, drop)
    return x + _drop_mul(h, drop)


class LayerNorm(nn.LayerNorm):
    """nn.LayerNorm (same parameter names) backed by the HIP kernel for bf16 on ROCm."""

    def forward(self, x):
        return layer_norm(x, self.weight, self.bias, self.eps)


def cross_entropy_sum(logits, target, scale: float, need_grad: bool, ignore_index: int | None = -100):
    """Summed token cross-entropy on [rows, V] logits.

    Returns (loss_sum, correct, count, dlogits): dlogits = scale * d(loss_sum)/dlogits in the
    logits dtype (None unless ``need_grad``). bf16 on ROCm uses the fused single-row kernel
    (never materialises fp32 logits).

    ``count`` is the number of rows whose target is not ``ignore_index``; counting them reads the device
    (a host sync). ``ignore_index=None`` promises that no target is ignored: count is then the number of
    rows and nothing is read back, which keeps a training step graph-capturable."""
    no_ignore = ignore_index is None
    if no_ignore:
        ignore_index = -100
    if _hip_bf16(logits):
        if not (logits.stride(-1) == 1 and (logits.shape[0] <= 1 or logits.stride(0) >= logits.shape[1])):
            logits = logits.contiguous()  # (rows may be padded: the lm_head's [T, 50304]-strided logits stay in place)
        loss, ok, g = kernels().cross_entropy_bf16(logits, target.contiguous(), float(scale),
                                                   ignore_index, need_grad)
        valid = target.numel() if no_ignore else int((target != ignore_index).sum())
        return loss.sum(), ok.sum(), valid, g
    z = logits.float().detach().requires_grad_(need_grad)
    with torch.enable_grad():
        loss = F.cross_entropy(z, target, reduction="sum", ignore_index=ignore_index)
    g = None
    if need_grad:
        (g,) = torch.autograd.grad(loss * scale, z)
        g = g.to(logits.dtype)
    valid = target != ignore_index
    correct = ((z.detach().argmax(1) == target) & valid).sum()
    count = target.numel() if no_ignore else int(valid.sum())
    return loss.detach(), correct, count, g


class _FlashAttnFn(torch.autograd.Function):
    """Causal attention on a fused qkv projection [B, S, 3C] (HIP kernels, bf16, d = 64)."""

    @staticmethod
    def forward(ctx, qkv, n_head: int, scale: float, drop: Optional[Drop] = None):
        B, S, C3 = qkv.shape
        C = C3 // 3
        D = C // n_head
        qkv = qkv.contiguous()
        q, k, v = (qkv[..., i * C:(i + 1) * C].view(B, S, n_head, D) for i in range(3))
        # dropout on the probabilities inside the kernels: the backward regenerates the mask from these same values
        ctx.dkw = {} if drop is None else dict(drop.kw(), head0=drop.head0)
        out, lse = kernels().attention_fwd(q, k, v, scale, True, **ctx.dkw)
        ctx.save_for_backward(qkv, out, lse)
        ctx.n_head, ctx.scale = n_head, scale
        return out.view(B, S, C)

    @staticmethod
    def backward(ctx, gout):
        qkv, out, lse = ctx.saved_tensors
        B, S, C3 = qkv.shape
        C, H = C3 // 3, ctx.n_head
        D = C // H
        dqkv = torch.empty_like(qkv)
        q, k, v = (qkv[..., i * C:(i + 1) * C].view(B, S, H, D) for i in range(3))
        dq, dk, dv = (dqkv[..., i * C:(i + 1) * C].view(B, S, H, D) for i in range(3))
        kernels().attention_bwd(q, k, v, out, gout.contiguous().view(B, S, H, D), lse, dq, dk, dv, ctx.scale, True,
                                **ctx.dkw)
        return dqkv, None, None, None


def causal_attention(qkv, n_head: int, drop: Optional[Drop] = None):
    """softmax(q k^T / sqrt(d), causal) v from a fused [B, S, 3C] projection -> [B, S, C]. ``drop``: dropout on the
    probabilities (inside the flash kernels on ROCm bf16 d = 64; elsewhere an explicit masked softmax . matmul with the
    same mask from the torch twin)."""
    B, S, C3 = qkv.shape
    C = C3 // 3
    D = C // n_head
    if _hip_bf16(qkv) and D == 64:
        if drop is not None:
            return _FlashAttnFn.apply(qkv, n_head, 1.0 / math.sqrt(D), drop)
        return _FlashAttnFn.apply(qkv, n_head, 1.0 / math.sqrt(D))
    q, k, v = qkv.split(C, dim=2)
    q = q.view(B, S, n_head, D).transpose(1, 2)
    k = k.view(B, S, n_head, D).transpose(1, 2)
    v = v.view(B, S, n_head, D).transpose(1, 2)
    if drop is not None:
        att = (q @ k.transpose(-2, -1)) * (1.0 / math.sqrt(D))
        causal = torch.ones(S, S, dtype=torch.bool, device=qkv.device).tril()
        att = F.softmax(att.masked_fill(~causal, float("-inf")), dim=-1)
        keep = _ref.gpt2_attn_keep(drop.seed, drop.ctr, drop.layer, drop.sample0, B, drop.head0, n_head, S, drop.T,
                                   qkv.device)
        y = (att * (keep.to(torch.float32) * drop.scale).to(att.dtype)) @ v
    else:
        y = F.scaled_dot_product_attention(q, k, v, is_causal=True)
    return y.transpose(1, 2).contiguous().view(B, S, C)


class _GeluFn(torch.autograd.Function):
    """tanh-GELU on the HIP kernels (gpt2_ops.hip); the backward multiplies in place."""

    @staticmethod
    def forward(ctx, x):
        xc = x.contiguous()
        ctx.save_for_backward(xc)
        return kernels().gelu_fwd_bf16(xc)

    @staticmethod
    def backward(ctx, gy):
        (x,) = ctx.saved_tensors
        return kernels().gelu_bwd_bf16(gy.contiguous(), x, False)


def gelu(x):
    """GELU with the tanh approximation (GPT-2's activation)."""
    if _hip_bf16(x) and x.numel() % 8 == 0:
        return _GeluFn.apply(x)
    return F.gelu(x, approximate="tanh")


class _EmbeddingFn(torch.autograd.Function):
    """wte[tok] + wpe[:S] (HIP gather). The backward adds into wte.grad / wpe.grad in place (flat
    gradient buffer) with a deterministic segmented sum over the stably sorted tokens."""

    @staticmethod
    def forward(ctx, tok, wte, wpe, drop: Optional[Drop] = None):
        tok = tok.contiguous()
        if drop is None:
            out = kernels().embedding_fwd_bf16(tok, wte, wpe)
        else:  # embedding dropout on the sum, one rounding
            out = kernels().embedding_drop_fwd_bf16(tok, wte, wpe, **drop.kw())
        ctx.tok = tok
        ctx.params = (wte, wpe)
        ctx.drop = drop
        return out

    @staticmethod
    def backward(ctx, g):
        wte, wpe = ctx.params
        g = g.contiguous()
        if ctx.drop is not None:  # mask and scale g, then the deterministic segmented sums as without dropout
            g = kernels().dropout_add_bf16(None, g, **ctx.drop.kw())
        sorted_tok, perm = torch.sort(ctx.tok.reshape(-1), stable=True)
        direct = all(p.grad is not None and p.grad.is_contiguous() and p.grad.dtype == torch.bfloat16
                     for p in (wte, wpe))
        if direct:
            kernels().embedding_bwd_bf16(g, sorted_tok, perm, wte.grad, wpe.grad)
            return None, None, None, None
        gwte, gwpe = torch.zeros_like(wte), torch.zeros_like(wpe)
        kernels().embedding_bwd_bf16(g, sorted_tok, perm, gwte, gwpe)
        return None, gwte, gwpe, None


def embedding(tok, wte, wpe, drop: Optional[Drop] = None):
    """GPT-2 input embedding: wte[tok] + wpe[position] for tok [B, S]; ``drop``: embedding dropout on the sum."""
    if _hip_bf16(wte, wpe) and tok.is_cuda and wte.shape[1] % 4 == 0:
        if drop is not None:
            return _EmbeddingFn.apply(tok, wte, wpe, drop)
        return _EmbeddingFn.apply(tok, wte, wpe)
    S = tok.shape[1]
    e = F.embedding(tok, wte) + F.embedding(torch.arange(S, device=tok.device), wpe)[None]
    return e if drop is None else _drop_mul(e, drop)
