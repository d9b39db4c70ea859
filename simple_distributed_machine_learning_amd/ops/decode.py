"""Generation-time ops: the wrappers of the decode kernels (csrc/kernels/attention_decode.hip, attention_append.hip,
attention_extend.hip, attention_fork.hip, linear_decode.hip, sample.hip, lookup.hip) and their torch twins.

Dispatch: ROCm bf16 tensors (head width 64 for the attention) run the hand-written kernels, and a shape the kernels do
not take is an error there, never a library call. CPU tensors, fp32 and other head widths run the twins below, which
define the semantics. Nothing here builds an autograd graph: generation runs under ``torch.no_grad()``.
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

from .._native import kernels
from . import reference as _ref

EPI_STORE, EPI_BIAS, EPI_BIAS_GELU = 0, 1, 5  # csrc/kernels/kernels.h GemmEpi
LINEAR_DECODE_MAX_M = 64  # kLinearDecodeMaxM
ATTENTION_APPEND_MAX_T = 8  # kAttnAppendMaxT
ATTENTION_FORK_MAX_N = 64  # kAttnForkMaxN
LOOKUP_MAX_DRAFTS, LOOKUP_MAX_NGRAM = 7, 8  # kLookupMaxDrafts, kLookupMaxNgram


def _hip_bf16(*ts) -> bool:
    return all(t.is_cuda and t.dtype == torch.bfloat16 for t in ts)


def linear_decode_supported(M: int, N: int, K: int, ldx: int = None, ldw: int = None) -> bool:
    """Shapes the weight-streaming kernel takes: 1 <= M <= 64, K % 64 == 0, N % 16 == 0, row strides % 8 == 0."""
    return bool(kernels().linear_decode_supported(M, N, K, K if ldx is None else ldx, K if ldw is None else ldw))


def linear_decode(x, w, b=None, gelu: bool = False, tickets=None):
    """y [M, N] = x [M, K] w[N, K]^T (+ b) (then tanh-GELU; needs b). ROCm bf16: linear_decode.hip for M <= 64 (W
    streamed once over the whole chip), gemm_bf16.hip above that; anything else: torch.

    ``tickets``: the one-launch form of linear_decode.hip. An int32 tensor on x's device with at least N / 16 entries,
    all zero on entry; the kernel leaves them zero. Where the shape is split over K, the last split to arrive at a
    column tile sums the tile instead of a second launch; the bits are those of the call without tickets. A wrong
    dtype, device or size is a RuntimeError. The torch twins and the M > 64 path ignore it."""
    if gelu and b is None:
        raise ValueError("linear_decode: the GELU epilogue comes with a bias")
    if _hip_bf16(x, w):
        epi = EPI_BIAS_GELU if gelu else (EPI_BIAS if b is not None else EPI_STORE)
        if x.shape[0] <= LINEAR_DECODE_MAX_M:
            if tickets is None:
                return kernels().linear_decode(x, w, b, epi)
            return kernels().linear_decode(x, w, b, epi, tickets)
        return kernels().gemm_bf16(x, w, b, False, epi)[0]
    y = F.linear(x, w, b)
    return F.gelu(y, approximate="tanh") if gelu else y


def attention_decode_ref(qkv, k_cache, v_cache, lens, n_head: int, n_keys: int):
    """The twin: write the new k, v at cache row lens[b]; softmax(q K[0..lens[b]]^T / sqrt(D)) V[0..lens[b]] in fp32.
    Rows past lens[b] are selected away (a cache from torch.empty may hold NaN patterns)."""
    B, C3 = qkv.shape
    C = C3 // 3
    D = C // n_head
    q, k, v = (qkv[:, i * C:(i + 1) * C].view(B, n_head, D) for i in range(3))
    idx = lens.to(torch.int64)
    rows = torch.arange(B, device=qkv.device)
    k_cache[rows, idx] = k
    v_cache[rows, idx] = v
    live = torch.arange(n_keys, device=qkv.device)[None, :] <= idx[:, None]  # [B, n_keys]
    kc = torch.where(live[:, :, None, None], k_cache[:, :n_keys], torch.zeros_like(k_cache[:, :n_keys])).float()
    vc = torch.where(live[:, :, None, None], v_cache[:, :n_keys], torch.zeros_like(v_cache[:, :n_keys])).float()
    s = torch.einsum("bhd,bshd->bhs", q.float(), kc) * (1.0 / math.sqrt(D))
    p = torch.softmax(s.masked_fill(~live[:, None, :], -math.inf), dim=-1)
    return torch.einsum("bhs,bshd->bhd", p, vc).to(qkv.dtype).reshape(B, C)


def attention_decode(qkv, k_cache, v_cache, lens, n_head: int, n_keys: int, tickets=None):
    """One new token per sample against a KV cache. qkv [B, 3C]: the token's fused projection; k_cache / v_cache
    [B, Smax, H, D] (views with any row strides); lens int32 [B] on the device: keys already cached. Writes the new
    k, v to cache row lens[b] and returns the attention output [B, C] over keys 0..lens[b]. ``lens`` is not changed:
    the caller advances it once per step, on the device. ``n_keys`` is the host's bound lens[b] + 1 <= n_keys (the
    caller counts the steps itself, so no length is read back); n_keys <= Smax or a ValueError.

    ``tickets``: the one-launch form of attention_decode.hip. An int32 tensor on qkv's device with at least B * H
    entries, all zero on entry; the kernel leaves them zero. The last live chunk of a (sample, head) to arrive combines
    the chunks instead of a second launch, so the caller may pass ``n_keys = Smax`` (the bound then never changes);
    the bits are those of the call without tickets at any n_keys > max(lens). A wrong dtype, device or size is a
    RuntimeError. The bound n_keys > max(lens) cannot be checked without reading the device: if it is violated, the
    rows concerned are not written and their counters are left non-zero, so zero the tensor before using it again
    (``decode_step`` passes Smax and zeroes its buffer every step). The torch twin ignores it."""
    Smax = k_cache.shape[1]
    if not 1 <= n_keys <= Smax:
        raise ValueError(f"attention_decode: {n_keys} keys with the new one, but the cache has {Smax} rows")
    D = k_cache.shape[-1]
    if _hip_bf16(qkv, k_cache, v_cache) and D == 64:
        if tickets is not None:
            return kernels().attention_decode(qkv, k_cache, v_cache, lens, 1.0 / math.sqrt(D), int(n_keys), tickets)
        return kernels().attention_decode(qkv, k_cache, v_cache, lens, 1.0 / math.sqrt(D), int(n_keys))
    return attention_decode_ref(qkv, k_cache, v_cache, lens, n_head, n_keys)


def _check_lens_nq(who: str, B: int, lens, nq):
    for name, t in (("lens", lens), ("nq", nq)):
        if t.dtype != torch.int32 or t.shape != (B,):
            raise ValueError(f"{who}: {name} must be int32 [B], got {t.dtype} {tuple(t.shape)}")


def attention_append_ref(qkv, k_cache, v_cache, lens, nq, n_head: int, n_keys: int):
    """The twin: query t of sample b is live iff t < nq[b] and lens[b] + t < n_keys. A live query writes its k, v at
    cache row lens[b] + t and returns softmax(q_t K[0..lens[b]+t]^T / sqrt(D)) V[0..lens[b]+t] in fp32, which is
    ``attention_decode_ref`` for that token with lens[b] + t keys cached; a dead query writes nothing and returns
    zeros. Rows past a query's own are selected away (they may hold NaN patterns)."""
    B, T, C3 = qkv.shape
    C = C3 // 3
    D = C // n_head
    Smax = k_cache.shape[1]
    rows = torch.arange(B, device=qkv.device)
    keys = torch.arange(n_keys, device=qkv.device)[None, :]
    out = torch.zeros((B, T, C), dtype=qkv.dtype, device=qkv.device)
    for t in range(T):
        q, k, v = (qkv[:, t, i * C:(i + 1) * C].view(B, n_head, D) for i in range(3))
        at = lens.to(torch.int64) + t
        alive = (nq.to(torch.int64) > t) & (at < n_keys)  # [B]
        idx = at.clamp(0, Smax - 1)
        sel = alive[:, None, None]
        k_cache[rows, idx] = torch.where(sel, k, k_cache[rows, idx])
        v_cache[rows, idx] = torch.where(sel, v, v_cache[rows, idx])
        live = (keys <= idx[:, None]) & alive[:, None]  # [B, n_keys]
        kc = torch.where(live[:, :, None, None], k_cache[:, :n_keys], torch.zeros_like(k_cache[:, :n_keys])).float()
        vc = torch.where(live[:, :, None, None], v_cache[:, :n_keys], torch.zeros_like(v_cache[:, :n_keys])).float()
        s = torch.einsum("bhd,bshd->bhs", q.float(), kc) * (1.0 / math.sqrt(D))
        s = s.masked_fill(~live[:, None, :], -math.inf).masked_fill(~alive[:, None, None], 0.0)
        o = torch.einsum("bhs,bshd->bhd", torch.softmax(s, dim=-1), vc).to(qkv.dtype).reshape(B, C)
        out[:, t] = torch.where(alive[:, None], o, torch.zeros_like(o))
    return out


def attention_append(qkv, k_cache, v_cache, lens, nq, n_head: int, n_keys: int):
    """T = 1..8 new tokens per sample against a KV cache (attention_append.hip). qkv [B, T, 3C]: the tokens' fused
    projections; the caches and ``lens`` as ``attention_decode`` takes them; ``nq`` int32 [B] on the device: the
    sample's live queries, 0..T. Query t is live iff t < nq[b] and lens[b] + t < n_keys (the host's bound on the rows
    in use, 1 <= n_keys <= Smax or a ValueError): it writes its k, v to cache row lens[b] + t and its output row is,
    bit for bit on the kernels, what ``attention_decode`` returns for that token with lens[b] + t keys cached. A dead
    query writes no cache row and returns zeros. Returns [B, T, C]; ``lens`` is not changed."""
    T = qkv.shape[1] if qkv.dim() == 3 else 0
    if not 1 <= T <= ATTENTION_APPEND_MAX_T:
        raise ValueError(f"attention_append: qkv must be [B, T, 3C] with T in 1..{ATTENTION_APPEND_MAX_T}, got "
                         f"{tuple(qkv.shape)}")
    Smax = k_cache.shape[1]
    if not 1 <= n_keys <= Smax:
        raise ValueError(f"attention_append: n_keys = {n_keys}, but the cache has {Smax} rows")
    _check_lens_nq("attention_append", qkv.shape[0], lens, nq)
    D = k_cache.shape[-1]
    if _hip_bf16(qkv, k_cache, v_cache) and D == 64:
        return kernels().attention_append(qkv, k_cache, v_cache, lens, nq, 1.0 / math.sqrt(D), int(n_keys))
    return attention_append_ref(qkv, k_cache, v_cache, lens, nq, n_head, n_keys)


def attention_extend_ref(qkv, k_cache, v_cache, lens, nq, n_head: int, n_keys: int):
    """The twin of ``attention_extend``: ``attention_append_ref``'s semantics at any T, one masked softmax per sample
    in fp32 over keys 0..n_keys-1. The live positions' k, v go to cache rows lens[b] + t first; position t then sees
    keys 0..lens[b]+t. Rows it does not see are selected away (they may hold NaN patterns); a dead position writes
    nothing and returns zeros."""
    B, T, C3 = qkv.shape
    C = C3 // 3
    D = C // n_head
    Smax = k_cache.shape[1]
    q, k, v = (qkv[..., i * C:(i + 1) * C].view(B, T, n_head, D) for i in range(3))
    at = lens.to(torch.int64)[:, None] + torch.arange(T, device=qkv.device)[None, :]  # [B, T]: absolute positions
    alive = (torch.arange(T, device=qkv.device)[None, :] < nq.to(torch.int64)[:, None]) & (at < n_keys) & \
        (lens.to(torch.int64)[:, None] >= 0)
    idx = at.clamp(0, Smax - 1)
    rows = torch.arange(B, device=qkv.device)[:, None].expand(B, T)
    sel = alive[:, :, None, None]
    k_cache[rows[alive], idx[alive]] = k[alive]
    v_cache[rows[alive], idx[alive]] = v[alive]
    keys = torch.arange(n_keys, device=qkv.device)
    live = (keys[None, None, :] <= idx[:, :, None]) & alive[:, :, None]  # [B, T, n_keys]
    used = live.any(dim=1)[:, :, None, None]  # [B, n_keys, 1, 1]: rows some position of the sample sees
    kc = torch.where(used, k_cache[:, :n_keys], torch.zeros_like(k_cache[:, :n_keys])).float()
    vc = torch.where(used, v_cache[:, :n_keys], torch.zeros_like(v_cache[:, :n_keys])).float()
    s = torch.einsum("bthd,bshd->bhts", q.float(), kc) * (1.0 / math.sqrt(D))
    s = s.masked_fill(~live[:, None], -math.inf).masked_fill(~alive[:, None, :, None], 0.0)
    o = torch.einsum("bhts,bshd->bthd", torch.softmax(s, dim=-1), vc).to(qkv.dtype)
    return torch.where(sel, o, torch.zeros_like(o)).reshape(B, T, C)


def attention_extend(qkv, k_cache, v_cache, lens, nq, n_head: int, n_keys: int):
    """Any T >= 1 new positions per sample against a KV cache plus themselves (attention_extend.hip): chunked prefill
    and a session's catch-up. qkv [B, T, 3C]: the chunk's fused projections, right-padded; the caches, ``lens`` and
    ``nq`` as ``attention_append`` takes them. Position t is live iff t < nq[b] and lens[b] + t < n_keys (the host's
    bound on the rows in use, 1 <= n_keys <= Smax or a ValueError): it writes its k, v to cache row lens[b] + t and
    returns the causal attention over keys 0..lens[b]+t, on the kernels with the bits ``causal_attention`` gives that
    position of the full sequence (docs/NUMERICS.md). A dead position writes no cache row and returns zeros. Returns
    [B, T, C]; ``lens`` is not changed."""
    if qkv.dim() != 3 or qkv.shape[1] < 1 or k_cache.dim() != 4 or k_cache.shape != v_cache.shape or \
            qkv.shape[0] != k_cache.shape[0] or qkv.shape[2] != 3 * k_cache.shape[2] * k_cache.shape[3] or \
            k_cache.shape[2] != n_head:
        raise ValueError(f"attention_extend: qkv must be [B, T >= 1, 3C] against caches [B, Smax, H, D] with C = H D, "
                         f"got {tuple(qkv.shape)}, {tuple(k_cache.shape)}, {tuple(v_cache.shape)}, n_head={n_head}")
    if not (qkv.dtype == k_cache.dtype == v_cache.dtype):
        raise ValueError(f"attention_extend: qkv and the caches must share one dtype, got {qkv.dtype}, "
                         f"{k_cache.dtype}, {v_cache.dtype}")
    Smax = k_cache.shape[1]
    if not 1 <= n_keys <= Smax:
        raise ValueError(f"attention_extend: n_keys = {n_keys}, but the cache has {Smax} rows")
    _check_lens_nq("attention_extend", qkv.shape[0], lens, nq)
    D = k_cache.shape[-1]
    if _hip_bf16(qkv, k_cache, v_cache) and D == 64:
        return kernels().attention_extend(qkv, k_cache, v_cache, lens, nq, 1.0 / math.sqrt(D), int(n_keys))
    return attention_extend_ref(qkv, k_cache, v_cache, lens, nq, n_head, n_keys)


def attention_fork_ref(qkv, kp, vp, plens, ks, vs, lens, n: int, n_head: int, n_keys: int):
    """The twin of ``attention_fork``: materialise each row's cache, the group's ``plens[g]`` prompt rows followed by
    the row's ``lens[r] - plens[g]`` suffix rows, run ``attention_decode_ref`` on it with ``lens[r]`` keys cached, and
    write the new k, v to suffix row ``lens[r] - plens[g]``. Rows the token does not see are zeros in the materialised
    cache (the tails of both caches may hold NaN patterns)."""
    R = qkv.shape[0]
    Pmax, Nmax = kp.shape[1], ks.shape[1]
    C = qkv.shape[1] // 3
    rows = torch.arange(R, device=qkv.device)
    grp = rows // int(n)
    pl, ln = plens.to(torch.int64)[grp], lens.to(torch.int64)
    i = torch.arange(Pmax + Nmax, device=qkv.device)[None, :]  # key index
    from_p, from_s = i < pl[:, None], (i >= pl[:, None]) & (i < ln[:, None])
    ip = i.clamp(max=Pmax - 1).expand(R, -1)
    is_ = (i - pl[:, None]).clamp(0, Nmax - 1)
    caches = []
    for pre, suf in ((kp, ks), (vp, vs)):
        both = torch.where(from_p[:, :, None, None], pre[grp[:, None], ip],
                           torch.where(from_s[:, :, None, None], suf[rows[:, None], is_],
                                       torch.zeros((), dtype=suf.dtype, device=suf.device)))
        caches.append(both)
    out = attention_decode_ref(qkv, caches[0], caches[1], lens, n_head, n_keys)
    ks[rows, ln - pl] = qkv[:, C:2 * C].view(R, n_head, -1)
    vs[rows, ln - pl] = qkv[:, 2 * C:].view(R, n_head, -1)
    return out


def attention_fork(qkv, kp, vp, plens, ks, vs, lens, n: int, n_head: int, n_keys: int):
    """One new token for each of R = G n rows, n continuations per prompt (attention_fork.hip). Row g n + j is sibling
    j of group g. qkv [R, 3C]: the tokens' fused projections; ``kp`` / ``vp`` [G, Pmax, H, D] with ``plens`` int32 [G]
    on the device: the groups' prompt keys, stored once and only read; ``ks`` / ``vs`` [R, Nmax, H, D]: every row's own
    later keys; ``lens`` int32 [R] on the device: ``plens[g]`` plus the row's suffix keys. Key i of row r is
    ``kp[g, i]`` for i < plens[g], ``ks[r, i - plens[g]]`` up to lens[r], and the row's own ``qkv`` at i == lens[r],
    which is written to suffix row lens[r] - plens[g]. Returns [R, C], bit for bit on the kernels what
    ``attention_decode`` returns for that token on a cache holding the prompt rows followed by the suffix rows; the
    kernel loads a 64-key chunk of the prompt once for the n siblings. ``n_keys`` is the host's bound lens[r] + 1 <=
    n_keys <= Pmax + Nmax, or a ValueError; ``lens`` and ``plens`` are not changed."""
    if isinstance(n, bool) or not isinstance(n, int) or not 1 <= n <= ATTENTION_FORK_MAX_N:
        raise ValueError(f"attention_fork: n must be an integer in 1..{ATTENTION_FORK_MAX_N} (samples per group), got "
                         f"{n!r}")
    ts = (qkv, kp, vp, ks, vs)
    if _hip_bf16(*ts) and kp.dim() == 4 and kp.shape[-1] == 64 and kp.shape[2] == n_head:
        # the kernel path: the binding checks every argument (the decode loop calls this once per layer and step, so
        # nothing is checked twice); its refusals name the function and leave here as ValueError, like the twin path's
        try:
            return kernels().attention_fork(qkv, kp, vp, plens, ks, vs, lens, n, 1.0 / math.sqrt(64), int(n_keys))
        except RuntimeError as e:
            if not str(e).startswith("attention_fork:"):
                raise
            raise ValueError(str(e).split("\n")[0]) from None
    if qkv.dim() != 2 or kp.dim() != 4 or ks.dim() != 4 or kp.shape != vp.shape or ks.shape != vs.shape or \
            kp.shape[2:] != ks.shape[2:] or kp.shape[2] != n_head or qkv.shape[1] != 3 * kp.shape[2] * kp.shape[3] or \
            qkv.shape[0] != kp.shape[0] * n or ks.shape[0] != qkv.shape[0] or kp.shape[1] < 1 or ks.shape[1] < 1:
        raise ValueError(f"attention_fork: qkv must be [G n, 3C] against prefix caches [G, Pmax, H, D] and suffix "
                         f"caches [G n, Nmax, H, D] with C = H D, got {tuple(qkv.shape)}, {tuple(kp.shape)}, "
                         f"{tuple(vp.shape)}, {tuple(ks.shape)}, {tuple(vs.shape)}, n={n}, n_head={n_head}")
    if any(t.dtype != qkv.dtype for t in ts) or any(t.device != qkv.device for t in ts + (plens, lens)):
        raise ValueError(f"attention_fork: qkv and the caches must share one dtype, and all tensors one device, got "
                         f"{[str(t.dtype) for t in ts]} on {[str(t.device) for t in ts + (plens, lens)]}")
    if kp.stride() != vp.stride() or ks.stride() != vs.stride():
        raise ValueError("attention_fork: kp / vp and ks / vs must each share one layout, got strides "
                         f"{kp.stride()}, {vp.stride()}, {ks.stride()}, {vs.stride()}")
    G, Pmax, Nmax = kp.shape[0], kp.shape[1], ks.shape[1]
    if not 1 <= n_keys <= Pmax + Nmax:
        raise ValueError(f"attention_fork: n_keys = {n_keys}, but the caches have {Pmax} + {Nmax} rows")
    for name, t, want in (("plens", plens, G), ("lens", lens, G * n)):
        if t.dtype != torch.int32 or t.shape != (want,):
            raise ValueError(f"attention_fork: {name} must be int32 [{want}], got {t.dtype} {tuple(t.shape)}")
    return attention_fork_ref(qkv, kp, vp, plens, ks, vs, lens, n, n_head, n_keys)


def lookup_step(g, tok_in, nq_in, out, lens, limit, done, gen_len, row_steps, k: int, ngram: int, eos: int = -1,
                pad: int = 0):
    """Prompt-lookup speculation's bookkeeping, one launch per verify step: accept the step's drafts against the
    sampler's tokens ``g``, then draft the next step's tokens from the row's own history (ops/reference.py lookup_step
    is the definition). Returns (tok_next [B, k + 1], nq_next [B], all_done [1]). Device tensors: lookup.hip, integer
    work with no host synchronisation; CPU tensors: the twin."""
    if not 1 <= int(k) <= LOOKUP_MAX_DRAFTS:
        raise ValueError(f"lookup_step: k must be in 1..{LOOKUP_MAX_DRAFTS}, got {k}")
    if not 1 <= int(ngram) <= LOOKUP_MAX_NGRAM:
        raise ValueError(f"lookup_step: ngram must be in 1..{LOOKUP_MAX_NGRAM}, got {ngram}")
    if out.is_cuda:
        return tuple(kernels().lookup_step(g, tok_in, nq_in, out, lens, limit, done, gen_len, row_steps, int(k),
                                           int(ngram), int(eos), int(pad)))
    return _ref.lookup_step(g, tok_in, nq_in, out, lens, limit, done, gen_len, row_steps, int(k), int(ngram), int(eos),
                            int(pad))


def embedding_at(tok, pos, wte, wpe):
    """wte[tok[b]] + wpe[pos[b]] -> [B, C] for tok int64 [B] and pos int32 [B] on the device."""
    if _hip_bf16(wte, wpe) and tok.is_cuda and wte.shape[1] % 4 == 0:
        return kernels().embedding_at(tok.contiguous(), pos, wte, wpe)
    return F.embedding(tok, wte) + F.embedding(pos.to(torch.int64), wpe)


def sample_logits(logits, vocab: int, temperature: float, top_k: int, seed: int, sample0: int, positions,
                  rows_per_sample: int = 1):
    """Tokens int64 [B] from logits [B, ld]: greedy at temperature 0, else top-k Gumbel-max keyed by
    (seed, sample0 + row // rows_per_sample, positions[row], token) (ops/reference.py sample_logits is the
    definition). ROCm bf16: the on-device sampler, no host synchronisation."""
    if int(rows_per_sample) < 1:
        raise ValueError(f"sample_logits: rows_per_sample must be >= 1, got {rows_per_sample}")
    if _hip_bf16(logits):
        return kernels().sample_logits(logits, int(vocab), float(temperature), int(top_k), int(seed), int(sample0),
                                       positions, int(rows_per_sample))
    return _ref.sample_logits(logits, vocab, temperature, top_k, seed, sample0, positions, int(rows_per_sample))


def sample_step(logits, vocab: int, temperature: float, top_k: int, top_p: float, seed: int, sample0: int, positions,
                out=None, done=None, gen_len=None, eos: int = -1, pad: int = 0, rows_per_sample: int = 1):
    """sample_logits over the top-p nucleus of the top-k candidates, with one generation step's bookkeeping in the
    same launch (ops/reference.py sample_step is the definition): tokens int64 [B]; ``out`` int64 [B, W] gets the token
    at column positions[row], ``gen_len`` int32 [B] grows by one, ``done`` int32 [B] is set on ``eos`` (-1: none); a
    row already done emits ``pad`` and changes nothing. ``rows_per_sample``: row r is sample sample0 + r //
    rows_per_sample (the verify step of prompt-lookup speculation draws several positions of a sample at once). ROCm
    bf16: the on-device sampler, no host synchronisation."""
    if int(rows_per_sample) < 1:
        raise ValueError(f"sample_step: rows_per_sample must be >= 1, got {rows_per_sample}")
    if _hip_bf16(logits):
        return kernels().sample_step(logits, int(vocab), float(temperature), int(top_k), float(top_p), int(seed),
                                     int(sample0), positions, out, done, gen_len, int(eos), int(pad),
                                     int(rows_per_sample))
    return _ref.sample_step(logits, vocab, temperature, top_k, top_p, seed, sample0, positions, out, done, gen_len,
                            eos, pad, int(rows_per_sample))
