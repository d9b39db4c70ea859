"""Shared pieces of the fork tests (n samples per prompt): the cases of the attention_fork tests, a prefix cache and a
suffix cache with NaN tails, the cache that attention_decode would need for the same rows, and the repeated-prompt call
that ``generate(num_samples=n)`` must reproduce."""
from __future__ import annotations

import math

import torch

G, H, PMAX, NMAX = 3, 2, 192, 72
C = H * 64
SCALE = 0.125
NS = (1, 2, 3, 8)
# prompt lengths per group, tests/test_attention_append_gpu.py's LENS: from {1, 57..64, 120..128}, so a group has zero,
# one or two whole 64-key chunks in its prompt
PLENS = [(1, 57, 120), (58, 64, 121), (59, 63, 128), (60, 62, 127), (61, 126, 125), (122, 123, 124), (64, 1, 128)]
# suffix keys per row, rotated over the rows: with the prompt lengths above the new key lands on both sides of the 64-,
# 128- and 192-key edges, and the chunk that holds plens[g] is read from the prefix, the suffix and qkv at once
SUFFIX = (0, 1, 5, 6, 7, 8, 63, 64, 65)


def rnd(*shape, seed=0, amp=1.5, dtype=torch.bfloat16):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.empty(shape).uniform_(-1, 1, generator=g) * amp).to(dtype)


def bits(t):
    """The raw bits (bf16 or fp32): equality that holds for NaN patterns too."""
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def nan_tail(cache, lens):
    c = cache.clone()
    for b, n in enumerate(lens):
        c[b, n:] = math.nan
    return c


def suffix_lens(n, i):
    """Suffix keys of the G n rows of case i."""
    return [SUFFIX[(r + 2 * i + n) % len(SUFFIX)] for r in range(G * n)]


def fork_inputs(n, i, dtype=torch.bfloat16, pmax=PMAX, nmax=NMAX):
    """(qkv [R, 3C], kp, vp [G, pmax, H, 64], plens, ks, vs [R, nmax, H, 64], suffix lengths, lens) of case i at n
    samples per group, on the CPU; rows past the lengths hold NaN in both caches."""
    plens, suf = PLENS[i], suffix_lens(n, i)
    R = G * n
    qkv = rnd(R, 3 * C, seed=1000 * n + i, dtype=dtype)
    kp = nan_tail(rnd(G, pmax, H, 64, seed=2000 * n + i, dtype=dtype), plens)
    vp = nan_tail(rnd(G, pmax, H, 64, seed=3000 * n + i, dtype=dtype), plens)
    ks = nan_tail(rnd(R, nmax, H, 64, seed=4000 * n + i, dtype=dtype), suf)
    vs = nan_tail(rnd(R, nmax, H, 64, seed=5000 * n + i, dtype=dtype), suf)
    lens = [plens[r // n] + suf[r] for r in range(R)]
    return qkv, kp, vp, plens, ks, vs, suf, lens


def materialise(pre, suf_cache, plens, suf, n):
    """[R, Pmax + Nmax, H, 64]: per row the group's prompt rows followed by the row's suffix rows, NaN after."""
    R = suf_cache.shape[0]
    full = torch.full((R, pre.shape[1] + suf_cache.shape[1]) + tuple(pre.shape[2:]), math.nan, dtype=pre.dtype)
    for r in range(R):
        p, s = plens[r // n], suf[r]
        full[r, :p] = pre[r // n, :p]
        full[r, p:p + s] = suf_cache[r, :s]
    return full


def i32(v, device="cpu"):
    return torch.tensor(list(v), dtype=torch.int32, device=device)


def repeated(generate, engine, prompts, new, n, **kw):
    """The call ``generate(num_samples=n)`` must reproduce: every prompt n times in a row, the lengths likewise."""
    kw = dict(kw)
    if kw.get("prompt_lens") is not None:
        kw["prompt_lens"] = torch.as_tensor(kw["prompt_lens"]).repeat_interleave(n)
    return generate(engine, prompts.repeat_interleave(n, 0), new, **kw)


def same(got, want):
    """Tokens, or (tokens, lengths[, stats]): every tensor equal, every count equal."""
    got, want = (got if isinstance(got, tuple) else (got,)), (want if isinstance(want, tuple) else (want,))
    assert len(got) == len(want)
    for a, b in zip(got, want):
        if isinstance(a, dict):
            assert a.keys() == b.keys() and a["steps"] == b["steps"]
            assert all(torch.equal(a[k], b[k]) for k in ("row_steps", "generated"))
        else:
            assert a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b)
