"""GPT-2 (small: 12 layers, d=768, 12 heads, ctx 1024, vocab 50257) split into pipeline
stages, bf16 (BASELINE config 5: "2-stage GPT-2-small transformer split bf16").

Stage 0 owns the token/position embeddings, the last stage owns ``ln_f`` + ``lm_head``;
the 12 blocks are divided evenly. Boundary tensor: [mb, S, 768] bf16 (1.5 MiB per sample
at S=1024) — the large-activation send that RCCL p2p overlaps with compute.

The output projection is untied from ``wte`` because the two live on different ranks
(documented deviation from the 124M tied checkpoint; +38.6M parameters on the last stage).
Linear layers (ops/linear.py) and LayerNorms accumulate their weight/bias gradients straight
into the flat gradient buffer (GEMM beta = 1, in-place bf16 reductions) instead of
materialise-then-add. Parameter names follow the common GPT-2 layout (wte, wpe, h.{i}.ln_1, h.{i}.attn.c_attn,
h.{i}.attn.c_proj, h.{i}.ln_2, h.{i}.mlp.c_fc, h.{i}.mlp.c_proj, ln_f, lm_head).

Dropout (GPT-2's recipe: embedding, attention probabilities, both residual branches) draws its masks from a counter
hash (csrc/kernels/dropout_hash.h, twin in ops/reference.py) keyed by the run's seed, the engine's step counter, the
site, the global layer, the dataset index of the sample, the global head and the coordinates inside the sample: the
masks do not depend on the micro-batch split, the pipeline placement or the tensor-parallel rank. Probabilities are
quantised to T / 256 (``GPT2Config.effective_pdrop``).
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from .base import ModelSpec, PipelineStage
from ..ops.decode import (ATTENTION_APPEND_MAX_T, ATTENTION_FORK_MAX_N, LINEAR_DECODE_MAX_M, attention_append,
                          attention_decode, attention_extend, attention_fork, embedding_at, linear_decode)
from ..ops.linear import Linear, _w_padded, linear, lm_head, mlp_gelu
from ..ops.reference import (DROP_SITE_ATTN, DROP_SITE_EMBD, DROP_SITE_RESID_ATTN, DROP_SITE_RESID_MLP,
                             dropout_threshold)
from ..ops.transformer import (Drop, LayerNorm, add_layer_norm, causal_attention, cross_entropy_sum, dropout_add,
                               embedding, gelu, layer_norm_pass)
from ..parallel.tp import TPContext, column_slice, copy_to_tp, reduce_from_tp, shard_parameter


@dataclass
class GPT2Config:
    n_layer: int = 12
    n_head: int = 12
    n_embd: int = 768
    vocab_size: int = 50257
    block_size: int = 1024
    dropout: float = 0.0  # sets the three probabilities below where they are not given
    embd_pdrop: Optional[float] = None   # on wte[tok] + wpe[pos]
    attn_pdrop: Optional[float] = None   # on the attention probabilities
    resid_pdrop: Optional[float] = None  # on each block's attention and MLP output before the residual add

    def __post_init__(self):
        for f in ("embd_pdrop", "attn_pdrop", "resid_pdrop"):
            if getattr(self, f) is None:
                setattr(self, f, float(self.dropout))
            dropout_threshold(getattr(self, f))  # range check

    def thresholds(self) -> dict:
        """site -> T = round(256 p) (0: off)."""
        return {f: dropout_threshold(getattr(self, f)) for f in ("embd_pdrop", "attn_pdrop", "resid_pdrop")}

    def effective_pdrop(self) -> dict:
        """The probabilities the kernels apply: T / 256."""
        return {f: t / 256.0 for f, t in self.thresholds().items()}


def dropout_seed(seed: int) -> int:
    """The run's dropout seed (63 bits) from the run seed: the same on every rank."""
    return ((int(seed) + 1) * 0x9E3779B97F4A7C15 ^ 0xD1B54A32D192ED03) & ((1 << 63) - 1)


class CausalSelfAttention(nn.Module):
    def __init__(self, cfg: GPT2Config):
        super().__init__()
        self.c_attn = Linear(cfg.n_embd, 3 * cfg.n_embd)
        self.c_proj = Linear(cfg.n_embd, cfg.n_embd)
        self.n_head = cfg.n_head
        self.head0 = 0  # global index of this rank's first head
        self.tp: TPContext = None

    def shard_tp(self, tp: TPContext):
        """Keep this rank's heads: the q/k/v columns of c_attn (column-parallel) and the matching
        input features of c_proj (row-parallel; its bias stays whole, added after the reduce)."""
        C = self.c_proj.weight.shape[0]
        cols = column_slice(C, tp)
        idx = torch.cat([torch.arange(cols.start, cols.stop) + i * C for i in range(3)])
        shard_parameter(self.c_attn, "weight", 0, idx)
        shard_parameter(self.c_attn, "bias", 0, idx)
        shard_parameter(self.c_proj, "weight", 1, cols)
        self.n_head //= tp.size
        self.head0 = tp.rank * self.n_head
        self.tp = tp

    def forward(self, x, drop: Optional[Drop] = None):
        # HIP flash attention (bf16, head_dim 64) on ROCm; PyTorch SDPA elsewhere. drop: attention dropout of this
        # layer and call; the mask is keyed by the global head index
        if drop is not None:
            drop = Drop(drop.T, drop.seed, drop.ctr, drop.site, drop.layer, drop.sample0, self.head0)
        if self.tp is None:
            return self.c_proj(causal_attention(self.c_attn(x), self.n_head, drop))
        a = causal_attention(self.c_attn(copy_to_tp(x, self.tp)), self.n_head, drop)
        return reduce_from_tp(linear(a, self.c_proj.weight), self.tp) + self.c_proj.bias


class MLP(nn.Module):
    def __init__(self, cfg: GPT2Config):
        super().__init__()
        self.c_fc = Linear(cfg.n_embd, 4 * cfg.n_embd)
        self.c_proj = Linear(4 * cfg.n_embd, cfg.n_embd)
        self.tp: TPContext = None

    def shard_tp(self, tp: TPContext):
        cols = column_slice(self.c_fc.weight.shape[0], tp)
        shard_parameter(self.c_fc, "weight", 0, cols)
        shard_parameter(self.c_fc, "bias", 0, cols)
        shard_parameter(self.c_proj, "weight", 1, cols)
        self.tp = tp

    def forward(self, x):
        if self.tp is None:  # GELU fused into the c_fc forward / c_proj input-gradient GEMM epilogues
            return mlp_gelu(x, self.c_fc.weight, self.c_fc.bias, self.c_proj.weight, self.c_proj.bias)
        h = gelu(self.c_fc(copy_to_tp(x, self.tp)))
        return reduce_from_tp(linear(h, self.c_proj.weight), self.tp) + self.c_proj.bias


class Block(nn.Module):
    def __init__(self, cfg: GPT2Config):
        super().__init__()
        self.ln_1 = LayerNorm(cfg.n_embd)
        self.attn = CausalSelfAttention(cfg)
        self.ln_2 = LayerNorm(cfg.n_embd)
        self.mlp = MLP(cfg)

    def forward(self, x):
        x = x + self.attn(self.ln_1(x))
        return x + self.mlp(self.ln_2(x))


class GPT2Stage(PipelineStage):
    """One pipeline stage of GPT-2.

    Dropout: the engine's hooks ``fwd`` / ``head_fwd`` hand the call's dataset offset (``ctx["sample0"]``) and train flag
    to ``forward`` through the attributes ``_sample0`` / ``_drop_call``, set for the duration of the call and reset after
    it (the engine calls a stage from one thread). A direct ``stage(x)`` outside those hooks, with the module in
    training mode and some probability > 0, draws the masks of samples 0, 1, ... (``sample0 = 0``): call it through
    ``fwd`` with ``ctx["sample0"]`` set when the rows are other samples."""

    def __init__(self, cfg: GPT2Config, stage_id: int, num_stages: int):
        super().__init__()
        if cfg.n_layer % num_stages:
            raise ValueError("n_layer must be divisible by num_stages")
        self.cfg = cfg
        self.stage_id, self.num_stages = stage_id, num_stages
        self.loss_kind = "ce"
        per = cfg.n_layer // num_stages
        if stage_id == 0:
            self.wte = nn.Embedding(cfg.vocab_size, cfg.n_embd)
            self.wpe = nn.Embedding(cfg.block_size, cfg.n_embd)
        self.h = nn.ModuleDict({str(i): Block(cfg) for i in range(stage_id * per, (stage_id + 1) * per)})
        if stage_id == num_stages - 1:
            self.ln_f = LayerNorm(cfg.n_embd)
            self.lm_head = Linear(cfg.n_embd, cfg.vocab_size, bias=False)
            # the vocabulary padded to a multiple of 64 rows in the flat storage (zero rows, zero gradient): the
            # lm_head's three GEMMs run on the hand-written kernels as 50304-wide GEMMs (ops/linear.py lm_head)
            self.flat_row_multiple = {"lm_head.weight": 64}
        # dropout: the engine hands over its device step counter (rng_step) and each call's dataset offset
        # (ctx["sample0"]) only when some probability is on; with all three at 0 nothing below runs
        self._drop_t = cfg.thresholds()
        self.uses_rng_step = self.uses_sample0 = any(self._drop_t.values())
        self.drop_seed = dropout_seed(0)
        self._sample0, self._drop_call = 0, True
        self._init()

    def set_run_seed(self, seed: int):
        """The engine's run seed: every rank derives the same dropout seed from it."""
        self.drop_seed = dropout_seed(seed)

    def _drop(self, which: str, site: int, layer: int) -> Optional[Drop]:
        t = self._drop_t[which]
        if not t or not (self.training and self._drop_call):
            return None
        return Drop(t, self.drop_seed, getattr(self, "rng_step", None), site, layer, self._sample0)

    def _with_call(self, ctx, train, fn):
        """Run a stage hook with the call's dataset offset and train flag visible to forward()."""
        self._sample0, self._drop_call = int(ctx.get("sample0", 0)), bool(train)
        try:
            return fn()
        finally:
            self._sample0, self._drop_call = 0, True

    def fwd(self, x, ctx, train):
        if not self.uses_sample0:
            return super().fwd(x, ctx, train)
        return self._with_call(ctx, train, lambda: PipelineStage.fwd(self, x, ctx, train))

    supports_tp = True

    def shard_tp(self, tp: TPContext):
        """Tensor-parallel split of every block (parallel/tp.py); embeddings, LayerNorms and the
        vocabulary head stay replicated."""
        if self.cfg.n_head % tp.size:
            raise ValueError(f"n_head={self.cfg.n_head} is not divisible by tp={tp.size}")
        for blk in self.h.values():
            blk.attn.shard_tp(tp)
            blk.mlp.shard_tp(tp)
        self.tp = tp

    def _init(self):
        for name, p in self.named_parameters():
            if name.endswith("c_proj.weight"):
                nn.init.normal_(p, 0.0, 0.02 / math.sqrt(2 * self.cfg.n_layer))
            elif p.dim() >= 2:
                nn.init.normal_(p, 0.0, 0.02)
            elif name.endswith("bias"):
                nn.init.zeros_(p)

    # ---- last stage: fused vocab cross-entropy (no fp32 copy of the [tokens, 50257] logits) --
    def head_fwd(self, x, target, ctx, train, loss_scale, stats=None):
        if not self.uses_sample0:
            return self._head_fwd(x, target, ctx, train, loss_scale)
        return self._with_call(ctx, train, lambda: self._head_fwd(x, target, ctx, train, loss_scale))

    def _head_fwd(self, x, target, ctx, train, loss_scale):
        if not train:
            with torch.no_grad():
                logits = self(x)
                l, c, n, _ = cross_entropy_sum(logits.reshape(-1, logits.shape[-1]), target.reshape(-1), 1.0, False,
                                               ignore_index=None)
            return l, c, n
        if not self.is_first:
            x = x.detach().requires_grad_(True)
        with torch.enable_grad():
            logits = self(x)
        l, c, n, g = cross_entropy_sum(logits.detach().reshape(-1, logits.shape[-1]), target.reshape(-1),
                                       loss_scale, True, ignore_index=None)  # token targets: none ignored, no sync
        ctx["x"], ctx["logits"], ctx["glogits"] = x, logits, g.view_as(logits)
        return l, c, n

    def head_bwd(self, ctx):
        x, logits, g = ctx.pop("x"), ctx.pop("logits"), ctx.pop("glogits")
        torch.autograd.backward(logits, g)
        return None if self.is_first else x.grad

    def forward(self, x):
        if self.stage_id == 0:  # token + position embedding (HIP gather, deterministic backward)
            x = embedding(x, self.wte.weight, self.wpe.weight, self._drop("embd_pdrop", DROP_SITE_EMBD, 0))
        last = self.stage_id == self.num_stages - 1
        blocks = list(self.h.values())
        if not blocks:
            return lm_head(self.ln_f(x), self.lm_head.weight) if last else x
        # each residual add is fused into the LayerNorm that reads its sum (ln_2 of the same block,
        # ln_1 of the next, ln_f at the end); the block maths is exactly Block.forward
        x, y = layer_norm_pass(x, blocks[0].ln_1)  # (x feeds ln_1 and the residual: one backward node for both)
        layers = [int(k) for k in self.h.keys()]  # global layer indices h.{i}
        for i, blk in enumerate(blocks):
            li = layers[i]
            a = blk.attn(y, self._drop("attn_pdrop", DROP_SITE_ATTN, li))
            x, y = add_layer_norm(x, a, blk.ln_2, self._drop("resid_pdrop", DROP_SITE_RESID_ATTN, li))
            m = blk.mlp(y)
            nxt = blocks[i + 1].ln_1 if i + 1 < len(blocks) else (self.ln_f if last else None)
            dm = self._drop("resid_pdrop", DROP_SITE_RESID_MLP, li)
            if nxt is None:
                x = x + m if dm is None else dropout_add(x, m, dm)
            else:
                x, y = add_layer_norm(x, m, nxt, dm)
        return lm_head(y, self.lm_head.weight) if last else x

    # ---- generation: KV cache, prefill, one decode step (ops/decode.py; parallel/generate.py drives them) ----------
    def new_cache(self, B: int, Smax: int, fused: bool = False) -> "KVCache":
        """An empty cache for B samples and up to Smax positions: K and V [B, Smax, H, D] per local layer, one
        device-side length. ``fused``: also the arrival counters of ``decode_step(fused=True)``, one zeroed int32
        buffer with a slice of its own per call site (four projections and the attention of every local layer; the
        lm_head is not split over K and needs none)."""
        if Smax > self.cfg.block_size:
            raise ValueError(f"a cache of {Smax} positions exceeds block_size={self.cfg.block_size}")
        if getattr(self, "tp", None) is not None:
            raise ValueError("generation does not run tensor-parallel stages (tp > 1)")
        p = next(self.parameters())
        H, D = self.cfg.n_head, self.cfg.n_embd // self.cfg.n_head
        mk = lambda: torch.empty((B, Smax, H, D), dtype=p.dtype, device=p.device)  # noqa: E731
        n = len(self.h)
        tickets = None
        if fused:
            tickets = torch.zeros(n * sum(self._ticket_sizes(B)), dtype=torch.int32, device=p.device)
        return KVCache([mk() for _ in range(n)], [mk() for _ in range(n)],
                       torch.zeros(B, dtype=torch.int32, device=p.device), 0, Smax, tickets)

    def _ticket_sizes(self, B: int):
        """Counters per call site of one layer (DECODE_SITES order): a projection has one per 16 output columns, the
        attention one per (sample, head). Each slice is padded to 16 bytes, so the buffer, zeroed as a whole from its
        allocation's start, stays a multiple of 16 bytes."""
        C = self.cfg.n_embd
        inner = next(iter(self.h.values())).mlp.c_fc.weight.shape[0] if len(self.h) else 4 * C
        raw = (3 * C // 16, B * self.cfg.n_head, C // 16, inner // 16, C // 16)
        return tuple((v + 3) // 4 * 4 for v in raw)

    def _ticket_views(self, cache: "KVCache"):
        """Per local layer, {site: its slice of cache.tickets}; built once per cache."""
        views = getattr(cache, "_views", None)
        if views is None:
            sizes = self._ticket_sizes(cache.lens.shape[0])
            if cache.tickets is None or cache.tickets.numel() < len(self.h) * sum(sizes):
                raise ValueError("decode_step(fused=True) needs a cache from new_cache(..., fused=True)")
            views, o = [], 0
            for _ in range(len(self.h)):
                d = {}
                for site, n in zip(DECODE_SITES, sizes):
                    d[site] = cache.tickets[o:o + n]
                    o += n
                views.append(d)
            cache._views = views
        return views

    def _head_logits(self, y):
        """[B, ld] logits of rows y [B, C]: ld is the padded vocabulary where the weight sits in row-padded storage
        (pad columns exact zeros), else the vocabulary."""
        w = self.lm_head.weight
        wp = _w_padded(w) if (w.is_cuda and w.dtype == torch.bfloat16) else None
        return linear_decode(y, w if wp is None else wp)

    def _layers(self, x, attn, mlp):
        """The blocks of this stage over x, without dropout: the one layer loop of the generation methods. Each residual
        add is fused into the LayerNorm that reads its sum, as in ``forward``. ``attn(i, blk, y)`` is local block i's
        attention branch through its ``c_proj``, ``mlp(i, blk, y)`` its MLP branch. Returns (x, y): the residual
        stream, and what the next LayerNorm made of it (``ln_f`` on the last stage; None on a stage without blocks)."""
        blocks = list(self.h.values())
        y = None
        if blocks:
            x, y = layer_norm_pass(x, blocks[0].ln_1)
        for i, blk in enumerate(blocks):
            x, y = add_layer_norm(x, attn(i, blk, y), blk.ln_2)
            m = mlp(i, blk, y)
            nxt = blocks[i + 1].ln_1 if i + 1 < len(blocks) else (self.ln_f if self.is_last else None)
            if nxt is None:
                x = x + m
            else:
                x, y = add_layer_norm(x, m, nxt)
        return x, y

    def _normed(self, x, y):
        """The last stage's ``ln_f`` rows after ``_layers``: its y, or ``ln_f(x)`` where the stage has no blocks."""
        return self.ln_f(x) if y is None else y

    @staticmethod
    def _decode_lines(attention, tickets=None):
        """The (attn, mlp) pair of ``_layers`` on ``linear_decode``, shared by the decode methods:
        ``attention(i, qkv)`` is the method's own attention call on block i's fused projection; ``tickets[i]``
        {site: counters or None} selects the one-launch forms of block i's projections."""
        def tk(i, site):
            return None if tickets is None else tickets[i][site]

        def attn(i, blk, y):
            at = blk.attn
            qkv = linear_decode(y, at.c_attn.weight, at.c_attn.bias, tickets=tk(i, "c_attn"))
            return linear_decode(attention(i, qkv), at.c_proj.weight, at.c_proj.bias, tickets=tk(i, "attn_proj"))

        def mlp(i, blk, y):
            fc, pr = blk.mlp.c_fc, blk.mlp.c_proj
            m = linear_decode(y, fc.weight, fc.bias, gelu=True, tickets=tk(i, "c_fc"))
            return linear_decode(m, pr.weight, pr.bias, tickets=tk(i, "mlp_proj"))

        return attn, mlp

    @torch.no_grad()
    def prefill(self, x, cache: "KVCache", lens=None, head_rows: int = 1):
        """The prompt through this stage: today's forward (flash attention at the prompt length, no dropout) plus the
        copies of every layer's k / v into the cache. x: tokens [B, S0] on stage 0, else [B, S0, C]. Returns the
        boundary [B, S0, C], or on the last stage the logits [B, ld] of the last position only.

        ``lens`` (int32 [B] on the device, 1 <= lens[b] <= S0, checked by the caller on the host): ragged prompts,
        right-padded to S0. Causal attention keeps every position < lens[b] independent of the padding, and the cache
        rows >= lens[b] are never read by the decode attention (each is overwritten before its turn). The cache
        lengths become ``lens``, ``cache.n`` = S0 bounds the longest row, and the last stage returns the logits of
        position lens[b] - 1 of each sample (a gather on the device).

        ``head_rows`` = n > 1 (``generate(num_samples=n)``): the last stage returns [B n, ld], sample b's logits in
        rows b n .. b n + n - 1. The sample's last hidden row is repeated ahead of the lm_head, not the logits after
        it, so the head runs over B n rows through the entry point that the prefill of the n-fold repeated prompts
        takes (``linear_decode`` up to 64 rows, the GEMM beyond) and the rows carry that call's bits."""
        if self.stage_id == 0:
            x = embedding(x, self.wte.weight, self.wpe.weight)
        B, S, C = x.shape
        if cache.n != 0 or S > cache.smax or B != cache.lens.shape[0]:
            raise ValueError(f"prefill of {B} x {S} tokens into a cache of {cache.lens.shape[0]} x {cache.smax} "
                             f"holding {cache.n}")
        H = self.cfg.n_head

        def attn(i, blk, y):
            qkv = blk.attn.c_attn(y)
            cache.k[i][:, :S].copy_(qkv[..., C:2 * C].view(B, S, H, C // H))
            cache.v[i][:, :S].copy_(qkv[..., 2 * C:].view(B, S, H, C // H))
            return blk.attn.c_proj(causal_attention(qkv, H))

        x, y = self._layers(x, attn, lambda i, blk, y: blk.mlp(y))
        if lens is None:
            cache.lens.fill_(S)
        else:
            cache.lens.copy_(lens)
        cache.n = S
        if not self.is_last:
            return x
        y = self._normed(x, y)
        if lens is None and head_rows == 1:
            return self._head_logits(y[:, -1].contiguous())
        rows = torch.arange(B, device=y.device) * S + (cache.lens.to(torch.int64) - 1)
        if head_rows > 1:
            rows = rows.repeat_interleave(int(head_rows))
        return self._head_logits(y.reshape(B * S, C).index_select(0, rows))

    @torch.no_grad()
    def extend(self, x, cache: "KVCache", nq=None):
        """T new positions per sample into a cache that may already hold some: chunked prefill and the catch-up of a
        generation session (parallel/session.py). x: tokens [B, T] on stage 0, else [B, T, C], right-padded, any T
        with cache.n + T <= cache.smax; ``nq`` int32 [B] on the device: the sample's live positions, 0..T (None: all
        T). Position t of sample b is lens[b] + t (clamped to block_size - 1 for the ``wpe`` lookup of a dead one).

        The layer lines are ``prefill``'s, the modules' own GEMM calls, so a prompt position runs through the same
        entry points whichever chunk carries it; ``attention_extend`` stands where ``prefill`` has
        ``causal_attention`` plus the two cache copies. Afterwards ``cache.lens += nq`` and ``cache.n`` =
        min(n + T, smax). Returns [B, T, C], or on the last stage the logits [B, ld] of each sample's last live
        position (row nq[b] - 1, gathered on the device before the lm_head); the row of a sample with nq[b] == 0
        holds unspecified values."""
        if x.dim() < 2 or x.shape[1] < 1:
            raise ValueError(f"extend: x must be [B, T(, C)] with T >= 1, got {tuple(x.shape)}")
        B, T = x.shape[0], x.shape[1]
        if B != cache.lens.shape[0] or cache.n + T > cache.smax:
            raise ValueError(f"extend of {B} x {T} positions into a cache of {cache.lens.shape[0]} x {cache.smax} "
                             f"holding {cache.n}")
        dev = cache.lens.device
        if nq is None:
            nq = torch.full((B,), T, dtype=torch.int32, device=dev)
        n_keys = cache.n + T
        if self.stage_id == 0:
            pos = cache.lens[:, None] + torch.arange(T, dtype=torch.int32, device=dev)[None, :]
            pos = pos.clamp_(max=self.cfg.block_size - 1).reshape(B * T)
            x = embedding_at(x.reshape(B * T), pos, self.wte.weight, self.wpe.weight).view(B, T, -1)
        C = x.shape[-1]
        H = self.cfg.n_head

        def attn(i, blk, y):
            qkv = blk.attn.c_attn(y)
            return blk.attn.c_proj(attention_extend(qkv, cache.k[i], cache.v[i], cache.lens, nq, H, n_keys))

        x, y = self._layers(x, attn, lambda i, blk, y: blk.mlp(y))
        cache.lens.add_(nq)
        cache.n = n_keys
        if not self.is_last:
            return x
        y = self._normed(x, y)
        rows = torch.arange(B, device=dev) * T + (nq.to(torch.int64) - 1).clamp_(min=0)
        return self._head_logits(y.reshape(B * T, C).index_select(0, rows))

    @torch.no_grad()
    def decode_step(self, x, cache: "KVCache", fused: bool = False):
        """One new token per sample. x: tokens [B] on stage 0, else [B, C]. Appends the token's k / v to the cache,
        advances the device-side length, returns [B, C] or on the last stage the logits [B, ld]. No host
        synchronisation: positions come from ``cache.lens``.

        ``fused`` (a cache from ``new_cache(fused=True)``): the one-launch forms (ops/decode.py ``tickets``) at the
        call sites of DECODE_FUSED_SITES, the four projections, and the attention over ``n_keys = smax`` so that no
        launch depends on the step's index. The same bits as ``fused=False``, 8 launches per block for 12; this is
        the step that parallel/decode_graph.py captures. The counters are zeroed once at the start of the
        step, so a step that died midway cannot poison the next."""
        if cache.n + 1 > cache.smax:
            raise ValueError(f"the cache is full ({cache.n} of {cache.smax} positions)")
        if fused:
            return self._decode_step_fused(x, cache)
        if self.stage_id == 0:
            x = embedding_at(x, cache.lens, self.wte.weight, self.wpe.weight)
        H = self.cfg.n_head
        x, y = self._layers(x, *self._decode_lines(
            lambda i, qkv: attention_decode(qkv, cache.k[i], cache.v[i], cache.lens, H, cache.n + 1)))
        cache.lens.add_(1)
        cache.n += 1
        return self._head_logits(self._normed(x, y)) if self.is_last else x

    def fork_cache(self, cache: "KVCache", n_samples: int, nmax: int) -> "ForkedKVCache":
        """n_samples continuations of every prompt of a prefilled ``cache``: the cache itself becomes the shared
        prefix (its ``lens`` are the prompt lengths; it is only read from here on), and every row b n + j, sibling j
        of prompt b, gets ``nmax`` suffix positions of its own per local layer. ``cache.n + nmax`` may not exceed
        block_size."""
        if isinstance(n_samples, bool) or not isinstance(n_samples, int) or not 1 <= n_samples <= ATTENTION_FORK_MAX_N:
            raise ValueError(f"fork_cache: n_samples must be an integer in 1..{ATTENTION_FORK_MAX_N}, got {n_samples!r}")
        if cache.n < 1:
            raise ValueError("fork_cache: the cache holds no prompt; prefill it first")
        if nmax < 1 or cache.n + nmax > self.cfg.block_size:
            raise ValueError(f"fork_cache: {cache.n} prompt positions + nmax = {nmax} must lie in {cache.n + 1}.."
                             f"block_size={self.cfg.block_size}")
        R = cache.lens.shape[0] * n_samples
        mk = lambda t: torch.empty((R, nmax) + t.shape[2:], dtype=t.dtype, device=t.device)  # noqa: E731
        return ForkedKVCache(cache, [mk(t) for t in cache.k], [mk(t) for t in cache.v],
                             cache.lens.repeat_interleave(n_samples), n_samples, cache.n, int(nmax))

    @torch.no_grad()
    def decode_step_forked(self, x, fc: "ForkedKVCache"):
        """``decode_step`` over the B n rows of a forked cache: one new token per row, x tokens [B n] on stage 0, else
        [B n, C]. The lines are ``decode_step``'s with ``attention_fork`` at the attention site, which reads a
        prompt's keys once for its n siblings; every other kernel of the step computes a row from that row alone, so
        a row's bits are those of ``decode_step`` on the n-fold repeated batch (docs/NUMERICS.md). Appends the
        token's k / v to the row's suffix, advances ``fc.lens`` and ``fc.n``; returns [B n, C] or on the last stage
        the logits [B n, ld]."""
        if fc.n + 1 - fc.prefix.n > fc.nmax:
            raise ValueError(f"the forked cache is full ({fc.n - fc.prefix.n} of {fc.nmax} suffix positions)")
        if self.stage_id == 0:
            x = embedding_at(x, fc.lens, self.wte.weight, self.wpe.weight)
        H = self.cfg.n_head
        pre = fc.prefix
        x, y = self._layers(x, *self._decode_lines(
            lambda i, qkv: attention_fork(qkv, pre.k[i], pre.v[i], pre.lens, fc.ks[i], fc.vs[i], fc.lens,
                                          fc.n_samples, H, fc.n + 1)))
        fc.lens.add_(1)
        fc.n += 1
        return self._head_logits(self._normed(x, y)) if self.is_last else x

    @torch.no_grad()
    def decode_block(self, x, cache: "KVCache", nq):
        """T = 1..8 new tokens per sample in one pass: the verify step of prompt-lookup speculation
        (parallel/generate.py lookup=K). x: tokens [B, T] on stage 0, else [B, T, C]; ``nq`` int32 [B] on the device:
        the sample's live tokens, 0..T. Token t of sample b sits at position lens[b] + t (clamped to block_size - 1
        for a dead one) and a live one attends to the cache plus tokens 0..t of its sample, whose k / v go to cache
        rows lens[b] + t. ``decode_step``'s kernels run over the B * T rows, with ``attention_append`` for the
        attention; each of them computes a row from that row alone, so a live row's bits are those of the
        ``decode_step`` that would have processed the token (docs/NUMERICS.md). Returns [B, T, C], or on the last
        stage the logits [B * T, ld] of all rows (row b * T + t).

        The device-side length is NOT advanced: the caller's ``lookup_step`` does that by the accepted count, so the
        stages of one rank must share one ``cache.lens`` tensor. ``cache.n`` becomes the host's bound min(n + T,
        smax). On ROCm bf16 B * T <= 64 is required (``linear_decode``'s rows): more rows would take another GEMM
        with other bits, and are refused."""
        if x.dim() < 2 or not 1 <= x.shape[1] <= ATTENTION_APPEND_MAX_T:
            raise ValueError(f"decode_block: x must be [B, T(, C)] with T in 1..{ATTENTION_APPEND_MAX_T}, got "
                             f"{tuple(x.shape)}")
        B, T = x.shape[0], x.shape[1]
        p = next(self.parameters())
        if p.is_cuda and p.dtype == torch.bfloat16 and B * T > LINEAR_DECODE_MAX_M:
            raise ValueError(f"decode_block: {B} samples x {T} tokens = {B * T} rows, but the decode projections take "
                             f"at most {LINEAR_DECODE_MAX_M} rows per step")
        if B != cache.lens.shape[0]:
            raise ValueError(f"decode_block: {B} samples into a cache of {cache.lens.shape[0]}")
        n_keys = min(cache.n + T, cache.smax)
        if self.stage_id == 0:
            pos = cache.lens[:, None] + torch.arange(T, dtype=torch.int32, device=cache.lens.device)[None, :]
            pos = pos.clamp_(max=self.cfg.block_size - 1).reshape(B * T)
            x = embedding_at(x.reshape(B * T), pos, self.wte.weight, self.wpe.weight)
        else:
            x = x.reshape(B * T, x.shape[-1])
        H = self.cfg.n_head
        x, y = self._layers(x, *self._decode_lines(
            lambda i, qkv: attention_append(qkv.view(B, T, -1), cache.k[i], cache.v[i], cache.lens, nq, H,
                                            n_keys).view(B * T, -1)))
        cache.n = n_keys
        return self._head_logits(self._normed(x, y)) if self.is_last else x.view(B, T, -1)

    @torch.no_grad()
    def _decode_step_fused(self, x, cache: "KVCache", _sites=None):
        """decode_step's lines with the counters of the call sites in DECODE_FUSED_SITES passed in and the attention's
        grid over the whole cache. ``_sites`` (tools/bench_generate.py only): other sites, to measure each one's
        share."""
        if cache.n + 1 > cache.smax:
            raise ValueError(f"the cache is full ({cache.n} of {cache.smax} positions)")
        sites = DECODE_FUSED_SITES if _sites is None else frozenset(_sites)
        views = self._ticket_views(cache)
        cache.tickets.zero_()
        if self.stage_id == 0:
            x = embedding_at(x, cache.lens, self.wte.weight, self.wpe.weight)
        H = self.cfg.n_head
        tk = [{s: (v if s in sites else None) for s, v in d.items()} for d in views]
        x, y = self._layers(x, *self._decode_lines(
            lambda i, qkv: attention_decode(qkv, cache.k[i], cache.v[i], cache.lens, H, cache.smax,
                                            tickets=tk[i]["attn"]), tk))
        cache.lens.add_(1)
        cache.n += 1
        return self._head_logits(self._normed(x, y)) if self.is_last else x


# the call sites of one block in decode_step, and those that run their one-launch form under fused=True (a site
# measured slower inside the captured step stays on two launches: docs/TUNING_NOTES.md "Graph-replayed decode")
DECODE_SITES = ("c_attn", "attn", "attn_proj", "c_fc", "mlp_proj")
DECODE_FUSED_SITES = frozenset(DECODE_SITES) - {"attn"}  # (the attention: 2.7 % slower on one launch, kept on two)


@dataclass
class KVCache:
    """A stage's generation state: per local layer K and V [B, Smax, H, D]; ``lens`` int32 [B] on the device (keys
    cached per sample, what the kernels read); ``n`` the host's bound on them (the count itself after an equal-length
    prefill, the longest row's after a ragged one; all samples advance together), so the bounds are checked without
    reading the device."""
    k: list
    v: list
    lens: torch.Tensor
    n: int
    smax: int
    tickets: Optional[torch.Tensor] = None  # new_cache(fused=True): the arrival counters of decode_step(fused=True)


@dataclass
class ForkedKVCache:
    """n_samples continuations of every prompt of a prefilled cache (``GPT2Stage.fork_cache``): ``prefix`` is that
    cache of B rows, read only, its ``lens`` the prompt lengths; ``ks`` / ``vs`` per local layer [B n_samples, nmax,
    H, D] hold each row's own later keys, row b n_samples + j being sibling j of prompt b; ``lens`` int32 [B
    n_samples] on the device = prompt plus suffix keys cached per row; ``n`` the host's bound on them."""
    prefix: KVCache
    ks: list
    vs: list
    lens: torch.Tensor
    n_samples: int
    n: int
    nmax: int


def gpt2_spec(num_stages: int = 2, cfg: GPT2Config = None, seq_len: int = None, dtype=torch.bfloat16,
              name: str = "gpt2") -> ModelSpec:
    cfg = cfg or GPT2Config()
    S = min(seq_len or cfg.block_size, cfg.block_size)

    def build(s):
        return GPT2Stage(cfg, s, num_stages)

    def shape(s, mb):
        return (mb, S, cfg.n_embd)

    return ModelSpec(name=name, num_stages=num_stages, build_stage=build, boundary_shape=shape,
                     boundary_dtype=dtype, input_kind="tokens", param_dtype=dtype, vocab_size=cfg.vocab_size,
                     seq_len=S)
