"""Plain-PyTorch fp32 reference implementations of every fused op.

They define the exact semantics the HIP kernels (csrc/kernels/*.hip) must reproduce and are
what the numerics tests compare against. They also serve the CPU (Gloo) path.
"""
from __future__ import annotations

import math
from typing import Optional, Tuple

import torch
import torch.nn.functional as F


def linear_relu_fwd(x, w, b):
    return torch.relu(x @ w.t() + b)


def linear_relu_bwd(x, y, gy, w, gw: Optional[torch.Tensor], gb: Optional[torch.Tensor], need_dx: bool):
    gz = gy * (y > 0).to(gy.dtype)
    if gw is not None:
        gw += gz.t() @ x
    if gb is not None:
        gb += gz.sum(0)
    return gz @ w if need_dx else None


def linear_fwd(x, w, b):
    return x @ w.t() + (b if b is not None else 0)


def linear_logsoftmax_nll(x, w, b, target, gw, gb, scale: float, need_dx: bool):
    z = x @ w.t() + b
    lp = F.log_softmax(z, dim=1)
    loss = -lp.gather(1, target.view(-1, 1)).sum()
    correct = (lp.argmax(1) == target).sum()
    dx = None
    if gw is not None or need_dx:
        dz = lp.exp()
        dz[torch.arange(z.shape[0]), target] -= 1.0
        dz *= scale
        if gw is not None:
            gw += dz.t() @ x
        if gb is not None:
            gb += dz.sum(0)
        if need_dx:
            dx = dz @ w
    return loss, correct, dx


def linear_logsoftmax_nll_dl(x, w, b, target, gw, gb, scale: float):
    """Training head whose boundary gradient is returned as its factor dl = scale * (softmax - onehot)
    (dx = dl @ w); gw/gb accumulated. Returns (loss_sum, correct, dl)."""
    z = x @ w.t() + b
    lp = F.log_softmax(z, dim=1)
    loss = -lp.gather(1, target.view(-1, 1)).sum()
    correct = (lp.argmax(1) == target).sum()
    dl = lp.exp()
    dl[torch.arange(z.shape[0]), target] -= 1.0
    dl *= scale
    gw += dl.t() @ x
    gb += dl.sum(0)
    return loss, correct, dl


def sgd_momentum_(p, g, buf, lr: float, momentum: float, dampening: float = 0.0, weight_decay: float = 0.0,
                  nesterov: bool = False, first: bool = False):
    """torch.optim.SGD semantics (first step: buf = g, no dampening)."""
    d = g if weight_decay == 0 else g + weight_decay * p
    if momentum != 0:
        if first:
            buf.copy_(d)
        else:
            buf.mul_(momentum).add_(d, alpha=1 - dampening)
        d = d + momentum * buf if nesterov else buf
    p.add_(d, alpha=-lr)


CLIP_EPS = 1e-6  # torch.nn.utils.clip_grad_norm_'s: c = max_norm / (norm + 1e-6), clamped to 1


def lr_at(step: int, lr: float, warmup: int = 0, decay_steps: int = 0, min_lr: float = 0.0,
          kind: str = "constant") -> float:
    """Learning rate of step ``step`` (1-based): linear warmup ``lr * step / warmup`` for ``step <= warmup``; then
    ``lr`` (constant), or cosine decay from ``lr`` at ``warmup`` to ``min_lr`` at ``decay_steps`` and ``min_lr`` from
    there on. A cosine schedule without a horizon (``decay_steps <= warmup``, e.g. 0) has nothing to decay over and
    stays at ``lr``."""
    if kind not in ("constant", "cosine"):
        raise ValueError(f"unknown lr schedule {kind!r} (constant, cosine)")
    t = float(step)
    if step <= warmup:
        return lr * t / float(warmup)
    if kind == "cosine" and decay_steps > warmup:
        prog = min(1.0, (t - float(warmup)) / float(decay_steps - warmup))
        return min_lr + 0.5 * (lr - min_lr) * (1.0 + math.cos(math.pi * prog))
    return lr


def grad_sqnorm(g) -> torch.Tensor:
    """Sum of squares of ``g`` as one float64 scalar tensor."""
    return g.detach().double().pow(2).sum()


def clip_coef(sqnorm, max_norm: float):
    """``clip_grad_norm_``'s coefficient from the squared global norm: min(1, max_norm / (norm + 1e-6));
    1 with clipping off (``max_norm <= 0``). float64 scalar tensor; a non-finite norm propagates."""
    if max_norm <= 0:
        return torch.ones((), dtype=torch.float64)
    norm = torch.as_tensor(sqnorm, dtype=torch.float64).sqrt()
    return torch.clamp(max_norm / (norm + CLIP_EPS), max=1.0)


def adamw_(p, g, m, v, step: int, lr: float, beta1: float = 0.9, beta2: float = 0.999, eps: float = 1e-8,
           weight_decay=0.0, clip: float = 1.0):
    """torch.optim.AdamW's step ``step`` (>= 1) in place on fp32 ``p``, ``m``, ``v``, the gradient scaled by the clip
    coefficient ``clip`` first. ``weight_decay``: a number, or a per-element tensor (``wd`` where the element belongs
    to a decayed parameter, 0 elsewhere). ``lr`` is the step's learning rate (``lr_at``)."""
    g = g.to(p.dtype)
    if clip != 1.0:
        g = g * float(clip)
    one = torch.ones((), dtype=p.dtype)
    lr_t = torch.tensor(lr, dtype=p.dtype)
    if torch.is_tensor(weight_decay):
        p.mul_(one - lr_t * weight_decay.to(p.dtype))
    elif weight_decay != 0:
        p.mul_(one - lr_t * torch.tensor(weight_decay, dtype=p.dtype))
    m.mul_(beta1).add_(g, alpha=1 - beta1)
    v.mul_(beta2).addcmul_(g, g, value=1 - beta2)
    step_size = lr / (1.0 - beta1 ** step)
    rbc2 = 1.0 / math.sqrt(1.0 - beta2 ** step)
    denom = v.sqrt().mul_(rbc2).add_(eps)
    p.addcdiv_(m, denom, value=-step_size)


def cross_entropy_fwd_bwd(logits, target, scale: float, ignore_index: int = -100):
    """Returns (loss_sum, correct, count, dlogits) with dlogits = scale * (softmax - onehot)."""
    z = logits.float()
    lse = torch.logsumexp(z, dim=1, keepdim=True)
    valid = target != ignore_index
    t = target.clamp_min(0)
    loss = (lse.squeeze(1) - z.gather(1, t.view(-1, 1)).squeeze(1))[valid].sum()
    correct = ((z.argmax(1) == target) & valid).sum()
    g = torch.exp(z - lse)
    g[torch.arange(z.shape[0]), t] -= 1.0
    g *= scale
    g[~valid] = 0
    return loss, correct, int(valid.sum()), g.to(logits.dtype)


def layernorm_fwd(x, w, b, eps: float = 1e-5):
    return F.layer_norm(x.float(), (x.shape[-1],), w.float(), b.float(), eps).to(x.dtype)


def gelu_tanh(x):
    return F.gelu(x.float(), approximate="tanh").to(x.dtype)


# ---- reference CNN (ref_cnn.hip) ------------------------------------------------------------
_M64 = (1 << 64) - 1


def dropout_keep_scale(seed: int, sample0: int, n: int, units: int, p: float) -> torch.Tensor:
    """[n, units] float32 dropout multipliers, bit-identical to ref_cnn.hip's counter hash:
    keep iff u(seed, sample0 + i, unit) >= p, kept units scaled by 1/(1-p)."""
    import numpy as np
    if p <= 0.0:
        return torch.ones(n, units)
    a = (np.arange(n, dtype=np.uint64) + np.uint64(sample0) + np.uint64(1))[:, None]
    b = np.arange(units, dtype=np.uint64)[None, :] + np.uint64(7)
    with np.errstate(over="ignore"):
        x = (np.uint64(seed & _M64) ^ (np.uint64(0x9E3779B97F4A7C15) * a) ^ (np.uint64(0xC2B2AE3D27D4EB4F) * b))
        x ^= x >> np.uint64(33)
        x *= np.uint64(0xFF51AFD7ED558CCD)
        x ^= x >> np.uint64(33)
        x *= np.uint64(0xC4CEB9FE1A85EC53)
        x ^= x >> np.uint64(33)
    h = (x & np.uint64(0xFFFFFFFF)) >> np.uint64(8)
    u = h.astype(np.float32) * np.float32(1.0 / 16777216.0)
    keep = u >= np.float32(p)
    sc = np.float32(1.0) / (np.float32(1.0) - np.float32(p))
    return torch.from_numpy(np.where(keep, sc, np.float32(0.0)).astype(np.float32))


def effective_seed(seed: int, ctr=None) -> int:
    """ref_cnn.hip's eff_seed: seed + 0x9E3779B97F4A7C15 * step_counter (mod 2^64)."""
    c = 0 if ctr is None else int(ctr.reshape(-1)[0])
    return (seed + 0x9E3779B97F4A7C15 * c) & _M64


def ref_cnn_stage0(x, w1, b1, w2, b2, seed: int, sample0: int, p: float, drop: bool):
    """Network1 forward with hash-based Dropout2d (autograd-capable)."""
    z1 = F.relu(F.max_pool2d(F.conv2d(x, w1, b1), 2))
    z2 = F.conv2d(z1, w2, b2)
    if drop:
        z2 = z2 * dropout_keep_scale(seed, sample0, x.shape[0], 20, p).to(z2.device)[:, :, None, None]
    return F.relu(F.max_pool2d(z2, 2)).reshape(-1, 320)


def ref_cnn_stage1_logp(x, w1, b1, w2, b2, seed: int, sample0: int, p: float, drop: bool):
    """Network2 forward (log-probabilities) with hash-based dropout (autograd-capable)."""
    h = F.relu(F.linear(x, w1, b1))
    if drop:
        h = h * dropout_keep_scale(seed, sample0, x.shape[0], 50, p).to(h.device)
    return F.log_softmax(F.linear(h, w2, b2), dim=1)


# ---- GPT-2 dropout masks (csrc/kernels/dropout_hash.h) --------------------------------------
# The host twin of the kernels' counter hash, in plain torch int64 ops (two's-complement wrap-around stands for the
# kernels' unsigned arithmetic), so it runs on the CPU and on a device tensor and agrees with the kernels bit for bit.
# A mask bit is a function of (seed, step counter, site, global layer, dataset index of the sample, global head,
# coordinates inside the sample) and nothing else.
DROP_SITE_EMBD, DROP_SITE_ATTN, DROP_SITE_RESID_ATTN, DROP_SITE_RESID_MLP = 1, 2, 3, 4
_M32 = 0xFFFFFFFF
_GOLDEN64 = 0x9E3779B97F4A7C15


def _s64(v: int) -> int:
    """The int64 with the bits of v mod 2^64."""
    v &= _M64
    return v - (1 << 64) if v >= (1 << 63) else v


def _lsr64(x, s: int):
    return (x >> s) & ((1 << (64 - s)) - 1)


def _splitmix64(x):
    x = x + _s64(_GOLDEN64)
    x = (x ^ _lsr64(x, 30)) * _s64(0xBF58476D1CE4E5B9)
    x = (x ^ _lsr64(x, 27)) * _s64(0x94D049BB133111EB)
    return x ^ _lsr64(x, 31)


def _fmix32(h):
    """Murmur3's finaliser on int64 tensors holding 32-bit values."""
    h = h ^ (h >> 16)
    h = (h * 0x85EBCA6B) & _M32
    h = h ^ (h >> 13)
    h = (h * 0xC2B2AE35) & _M32
    return h ^ (h >> 16)


def dropout_threshold(p: float) -> int:
    """T = round(256 p), 1..255 for p > 0: a value is kept iff its mask byte >= T (effective p = T / 256)."""
    if not 0.0 <= p < 1.0:
        raise ValueError(f"dropout probability must be in [0, 1), got {p}")
    if p == 0.0:
        return 0
    return min(255, max(1, int(math.floor(256.0 * p + 0.5))))


def dropout_scale(T: int) -> float:
    """256 / (256 - T) as the kernels compute it (one fp32 division)."""
    return float(torch.tensor(256.0, dtype=torch.float32) / torch.tensor(float(256 - T), dtype=torch.float32))


def gpt2_dropout_row_keys(seed: int, ctr, site: int, layer: int, samples, heads):
    """32-bit row keys (int64 tensor, broadcast of ``samples`` and ``heads``). ``ctr``: the int64 step-counter tensor
    (read on its device, no host sync) or None for counter 0."""
    eff = torch.as_tensor(_s64(seed), dtype=torch.int64, device=samples.device)
    if ctr is not None:
        eff = eff + _s64(_GOLDEN64) * ctr.reshape(-1)[0].to(samples.device)
    skey = _splitmix64(eff ^ ((int(site) << 32) | int(layer)))
    return _lsr64(_splitmix64(skey ^ ((samples << 32) | heads)), 32)


def gpt2_dropout_keep(rkey, na: int, nb: int, T: int):
    """keep[..., a, b] (bool) for row keys ``rkey`` [...]: byte (b & 3) of fmix32(rkey ^ a * 0x9E3779B1 ^
    (b >> 2) * 0x85EBCA77) >= T."""
    dev = rkey.device
    a = (torch.arange(na, dtype=torch.int64, device=dev) * 0x9E3779B1) & _M32
    b = torch.arange(nb, dtype=torch.int64, device=dev)
    b4 = ((b >> 2) * 0x85EBCA77) & _M32
    word = _fmix32(rkey[..., None, None] ^ a[:, None] ^ b4[None, :])
    return ((word >> (8 * (b & 3))) & 255) >= T


def gpt2_attn_keep(seed: int, ctr, layer: int, sample0: int, B: int, head0: int, H: int, S: int, T: int,
                   device=None):
    """[B, H, S, S] keep mask of the attention probabilities (query, key) of samples sample0.. and heads head0.. ."""
    dev = device if device is not None else (ctr.device if ctr is not None else "cpu")
    smp = torch.arange(sample0, sample0 + B, dtype=torch.int64, device=dev)[:, None]
    hd = torch.arange(head0, head0 + H, dtype=torch.int64, device=dev)[None, :]
    return gpt2_dropout_keep(gpt2_dropout_row_keys(seed, ctr, DROP_SITE_ATTN, layer, smp, hd), S, S, T)


def gpt2_site_keep(seed: int, ctr, site: int, layer: int, sample0: int, B: int, S: int, C: int, T: int, device=None):
    """[B, S, C] keep mask of an element-wise site (position, channel)."""
    dev = device if device is not None else (ctr.device if ctr is not None else "cpu")
    smp = torch.arange(sample0, sample0 + B, dtype=torch.int64, device=dev)
    return gpt2_dropout_keep(gpt2_dropout_row_keys(seed, ctr, site, layer, smp, torch.zeros_like(smp)), S, C, T)


# ---- generation: the sampler (csrc/kernels/sample.hip) ----------------------------------------
# The same counter hash, site DROP_SITE_SAMPLE, layer 0, head 0, a = the position of the token being drawn, the
# vocabulary id in the b4 slot (one word per candidate), no step counter: a drawn token is a function of
# (seed, sample, position, logits) and of nothing else.
DROP_SITE_SAMPLE = 5


def sample_uniforms(seed: int, samples, positions, vocab: int):
    """u [B, vocab] float32 for samples [B] and positions [B] (int tensors on one device):
    u = ((word >> 9) + 0.5) * 2^-23, word = fmix32(rkey ^ position * 0x9E3779B1 ^ v * 0x85EBCA77). Every u is exact in
    fp32 and lies in [2^-24, 1 - 2^-24]."""
    samples = samples.to(torch.int64)
    rkey = gpt2_dropout_row_keys(seed, None, DROP_SITE_SAMPLE, 0, samples, torch.zeros_like(samples))
    a = (positions.to(torch.int64).to(samples.device) * 0x9E3779B1) & _M32
    v = (torch.arange(vocab, dtype=torch.int64, device=samples.device) * 0x85EBCA77) & _M32
    word = _fmix32(rkey[:, None] ^ a[:, None] ^ v[None, :])
    return ((word >> 9).to(torch.float32) + 0.5) * (2.0 ** -23)


def gumbel_from_uniform(u):
    """g = -log(-log u) in the dtype of u."""
    return -torch.log(-torch.log(u))


def top_k_candidates(logits, top_k: int):
    """[B, V] bool: the tokens whose logit is >= the k-th largest logit value of their row (ties at the boundary are
    all candidates); top_k <= 0 or >= V: every token. NaN logits are never candidates."""
    z = torch.nan_to_num(logits.float(), nan=-math.inf)
    V = z.shape[1]
    ok = ~torch.isnan(logits)
    if top_k <= 0 or top_k >= V:
        return ok
    kth = torch.topk(z, int(top_k), dim=1).values[:, -1:]
    return ok & (z >= kth)


def top_p_threshold(logits, top_k: int, top_p: float, temperature: float):
    """theta [B] float64 of top_p_candidates (top_p off: -inf, i.e. every top-k candidate passes)."""
    cand = top_k_candidates(logits, top_k)
    z = torch.where(cand, logits.double(), torch.full_like(logits, -math.inf, dtype=torch.float64))
    B = z.shape[0]
    if not 0.0 < top_p < 1.0 or temperature <= 0:
        return torch.full((B,), -math.inf, dtype=torch.float64, device=z.device)
    s = z.sort(1, descending=True).values
    m = s[:, :1]
    w = torch.exp((s - m) / float(temperature))
    w = torch.where(s == m, torch.ones_like(w), w)  # (a maximum of +inf: inf - inf)
    w = torch.where(torch.isnan(w), torch.zeros_like(w), w)  # (a row without candidates)
    cum = w.cumsum(1)
    # the first sorted position whose cumulative mass reaches top_p of the total: its value is theta (inside a run of
    # equal values the run's end reaches it too, and no larger value's run does)
    first = (cum >= float(top_p) * cum[:, -1:]).to(torch.int8).argmax(1)
    return s.gather(1, first[:, None])[:, 0]


def top_p_candidates(logits, top_k: int, top_p: float, temperature: float):
    """[B, V] bool, the nucleus inside the top-k candidates C_k, in float64: with m the largest candidate logit and
    w_v = exp((l_v - m) / T) for v in C_k, theta is the largest logit value x with sum{w_v : l_v >= x} >= top_p *
    sum{w_v}; the candidates are {v in C_k : l_v >= theta}. Ties at theta are all kept and every token with the maximal
    logit is a member. top_p <= 0 or >= 1 (or temperature 0): top_k_candidates."""
    cand = top_k_candidates(logits, top_k)
    if not 0.0 < top_p < 1.0 or temperature <= 0:
        return cand
    theta = top_p_threshold(logits, top_k, top_p, temperature)
    return cand & (torch.nan_to_num(logits.double(), nan=-math.inf) >= theta[:, None])


def _first_argmax(score, cand):
    """Index of the largest score among the candidates, the lowest index on ties (token 0 for a row without any)."""
    s = torch.where(cand, score, torch.full_like(score, -math.inf))
    V = s.shape[1]
    idx = torch.arange(V, device=s.device)[None, :].expand_as(s)
    hit = cand & (s == s.amax(1, keepdim=True))
    tok = torch.where(hit, idx, torch.full_like(idx, V)).amin(1)
    return torch.where(tok == V, torch.zeros_like(tok), tok)


def sample_logits(logits, vocab: int, temperature: float, top_k: int, seed: int, sample0: int, positions,
                  rows_per_sample: int = 1):
    """Tokens [B] int64 from logits [B, ld] (columns < vocab take part). temperature == 0: greedy (argmax, lowest index
    on ties). temperature > 0: Gumbel-max over the top-k candidates, argmax_v(l_v * (1 / T) + g_v) in fp32 with one
    multiply and one add, noise from sample_uniforms for samples sample0 + row // rows_per_sample and the given
    positions [B] (rows_per_sample > 1: several positions of one sample in one call)."""
    if temperature < 0:
        raise ValueError(f"temperature must be >= 0, got {temperature}")
    z = logits[:, :vocab]
    cand = top_k_candidates(z, top_k)
    zf = torch.nan_to_num(z.float(), nan=-math.inf)
    if temperature == 0:
        return _first_argmax(zf, cand)
    B = z.shape[0]
    samples = sample0 + torch.arange(B, dtype=torch.int64, device=z.device) // int(rows_per_sample)
    g = gumbel_from_uniform(sample_uniforms(seed, samples, positions, vocab))
    inv_t = torch.tensor(1.0 / float(temperature), dtype=torch.float32, device=z.device)
    return _first_argmax(zf * inv_t + g, cand)


def sample_step(logits, vocab: int, temperature: float, top_k: int, top_p: float, seed: int, sample0: int, positions,
                out=None, done=None, gen_len=None, eos: int = -1, pad: int = 0, rows_per_sample: int = 1):
    """sample_logits over the nucleus (top_p_candidates) plus one generation step's bookkeeping, in place. Returns the
    step's tokens [B]. Per row, with pos = positions[row]: a row whose ``done`` flag is set emits ``pad`` and changes
    nothing; else the token goes to out[row, pos], gen_len[row] grows by one and done[row] is set when the token is
    ``eos`` (-1: none). A pos outside [0, W) changes none of the three. With top_p off and no bookkeeping tensors the
    tokens are sample_logits'."""
    if temperature < 0:
        raise ValueError(f"temperature must be >= 0, got {temperature}")
    if not 0.0 <= top_p <= 1.0:
        raise ValueError(f"top_p must be in [0, 1], got {top_p}")
    z = logits[:, :vocab]
    cand = top_p_candidates(z, top_k, top_p, temperature)
    zf = torch.nan_to_num(z.float(), nan=-math.inf)
    B = z.shape[0]
    if temperature == 0:
        tok = _first_argmax(zf, cand)
    else:
        samples = sample0 + torch.arange(B, dtype=torch.int64, device=z.device) // int(rows_per_sample)
        g = gumbel_from_uniform(sample_uniforms(seed, samples, positions, vocab))
        inv_t = torch.tensor(1.0 / float(temperature), dtype=torch.float32, device=z.device)
        tok = _first_argmax(zf * inv_t + g, cand)
    live = torch.ones(B, dtype=torch.bool, device=z.device) if done is None else done == 0
    tok = torch.where(live, tok, torch.full_like(tok, pad))
    pos = positions.to(torch.int64)
    W = out.shape[1] if out is not None else None
    write = live if W is None else live & (pos >= 0) & (pos < W)
    if out is not None:
        rows = torch.arange(B, device=z.device)[write]
        out[rows, pos[write]] = tok[write]
    if gen_len is not None:
        gen_len += write.to(gen_len.dtype)
    if done is not None:
        done |= (write & (tok == eos)).to(done.dtype)
    return tok


# ---- generation: prompt-lookup speculation (csrc/kernels/lookup.hip) ---------------------------------------------
def lookup_drafts(hist, ngram: int, k: int, limit: int):
    """(start, drafts) for a row's history ``hist`` (int64 [L + 1]: the tokens up to the newest, at column L): start
    = the largest s <= L - ngram with hist[s : s + ngram] == hist[L - ngram + 1 : L + 1] (-1: none, or fewer than
    ngram + 1 tokens), drafts = hist[s + ngram + i] for i < n = min(k, L - s - ngram + 1, limit - 2 - L): what followed
    the most recent earlier occurrence of the last ``ngram`` tokens, as far as the row's width ``limit`` has room for
    the drafts and the token after them."""
    L = hist.shape[0] - 1
    if L < ngram:
        return -1, hist[:0]
    win = hist.unfold(0, ngram, 1)[:L - ngram + 1]  # starts 0 .. L - ngram
    hits = (win == hist[L - ngram + 1:]).all(1).nonzero()
    if hits.numel() == 0:
        return -1, hist[:0]
    s = int(hits[-1])
    n = max(0, min(k, L - s - ngram + 1, limit - 2 - L))
    return s, hist[s + ngram:s + ngram + n]


def lookup_step(g, tok_in, nq_in, out, lens, limit, done, gen_len, row_steps, k: int, ngram: int, eos: int = -1,
                pad: int = 0):
    """One bookkeeping launch of prompt-lookup speculation, in place; the definition of csrc/kernels/lookup.hip.

    State per row b: ``out`` int64 [B, W] the token matrix; ``lens[b]`` the cache length, which is also the column of
    the row's newest token (not yet in the cache); ``limit[b]`` the row's final width (clamped to W); ``done``,
    ``gen_len``, ``row_steps`` int32 [B]. A row is full when lens[b] + 1 >= limit[b]; a done or full row changes
    nothing.

    Accept (``g`` int64 [B, k + 1] given, with the step's inputs ``tok_in`` [B, k + 1] = newest token + drafts and
    ``nq_in`` [B] = 1 + the number of drafts): a = the number of leading drafts d[i] = tok_in[b, 1 + i] with d[i] ==
    g[b, i]; the row emits g[b, 0..a], cut so that column lens[b] + 1 + i < limit[b] and after the first ``eos``
    (kept). The tokens go to out[b, lens[b] + 1 + i], gen_len[b] and lens[b] grow by the count, done[b] is set on an
    eos, row_steps[b] grows by one. ``g`` None: nothing to accept (the first drafts, after the eagerly sampled token).

    Draft (with the new lens): ``lookup_drafts`` of out[b, 0 .. lens[b]].

    Returns (tok_next int64 [B, k + 1]: the newest token, the drafts, ``pad`` in the unused slots; nq_next int32 [B]:
    1 + the number of drafts; all_done int32 [1]: 1 iff every nq_next is 0). A done or full row has nq_next 0 and
    ``pad`` throughout."""
    B, W = out.shape
    T = k + 1
    tok_next = torch.full((B, T), int(pad), dtype=torch.int64, device=out.device)
    nq_next = torch.zeros(B, dtype=torch.int32, device=out.device)
    for b in range(B):
        L = int(lens[b])
        lim = min(int(limit[b]), W)
        dn = bool(done[b]) or L < 0 or L >= W
        if g is not None and not dn and L + 1 < lim:
            n = max(0, min(int(nq_in[b]) - 1, k))
            a = 0
            while a < n and int(tok_in[b, 1 + a]) == int(g[b, a]):
                a += 1
            cnt = min(a + 1, lim - 1 - L)
            for i in range(cnt):
                if int(g[b, i]) == eos:
                    cnt, dn = i + 1, True
                    break
            out[b, L + 1:L + 1 + cnt] = g[b, :cnt]
            L += cnt
            lens[b] = L
            gen_len[b] += cnt
            row_steps[b] += 1
            if dn:
                done[b] = 1
        if dn or L + 1 >= lim:
            continue
        _, drafts = lookup_drafts(out[b, :L + 1], ngram, k, lim)
        n = drafts.shape[0]
        tok_next[b, 0] = out[b, L]
        tok_next[b, 1:1 + n] = drafts
        nq_next[b] = 1 + n
    all_done = (nq_next.max() == 0).to(torch.int32).reshape(1)
    return tok_next, nq_next, all_done
