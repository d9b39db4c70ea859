"""Shared pieces of the ragged-generation tests: the float64 nucleus written out plainly (sort and cumsum in numpy,
independent of the torch twin), the bound delta of docs/NUMERICS.md on the kernel's cumulative mass fraction, the
sampler inputs of the GPU tests, rule sequences and the rank body of the multi-process runs."""
from __future__ import annotations

import numpy as np
import torch

from generate_util import RULE_A, RULE_B, VOCAB

T_CASES, K_CASES, P_CASES = (0.7, 1.0), (0, 50), (0.5, 0.9, 0.95)
CASES = [(T, k, p) for T in T_CASES for k in K_CASES for p in P_CASES]
SAMPLER_SETS = {"gpt2": (64, 50257, 50304), "tiny": (5, 97, 128)}  # B, V, ld; the seed is V


def delta(V: int) -> float:
    """docs/NUMERICS.md, top-p: the kernel's cumulative mass fraction is within delta of the exact one."""
    return 0.6 * 2.0 ** -23 + V * 2.0 ** -40


def sampler_logits(B, V, ld, seed):
    """tests/test_decode_kernels_gpu.py's sampler inputs (that module skips without a GPU)."""
    g = torch.Generator().manual_seed(seed)
    z = torch.zeros(B, ld)
    z[:, :V] = torch.randn(B, V, generator=g) * 2.0
    return z.to(torch.bfloat16)


def nucleus64(logits, top_k: int, top_p: float, T: float):
    """(cand bool [B, V], theta float64 [B], margin float64 [B]) by the issue's rule, row by row in numpy float64:
    margin = the distance of top_p to the nearest cumulative mass fraction of the row (inf with top_p off)."""
    z = logits.double().numpy()
    B, V = z.shape
    cand = np.zeros((B, V), dtype=bool)
    theta = np.full(B, -np.inf)
    margin = np.full(B, np.inf)
    for r in range(B):
        l = z[r]
        ok = ~np.isnan(l)
        c = ok.copy()
        if 0 < top_k < V:
            kth = np.sort(np.where(ok, l, -np.inf))[::-1][top_k - 1]
            c = ok & (l >= kth)
        if 0.0 < top_p < 1.0 and c.any():
            vals, counts = np.unique(l[c], return_counts=True)  # ascending distinct values
            vals, counts = vals[::-1], counts[::-1]
            w = np.exp((vals - vals[0]) / T)
            w[vals == vals[0]] = 1.0
            frac = np.cumsum(w * counts)
            frac = frac / frac[-1]  # mass fraction of {l >= vals[j]}
            j = int(np.argmax(frac >= top_p))
            theta[r] = vals[j]
            margin[r] = np.abs(frac - top_p).min()
            c = c & (l >= vals[j])
        cand[r] = c
    return torch.from_numpy(cand), torch.from_numpy(theta), torch.from_numpy(margin)


def rule_seq(start: int, n: int):
    """n tokens of the synthetic data's rule t' = (a t + b) mod 97 from ``start``."""
    out = [int(start)]
    for _ in range(n - 1):
        out.append((out[-1] * RULE_A + RULE_B) % VOCAB)
    return out


def eos_prompts(lens, steps, orbit_start: int = 0):
    """Prompts of the given lengths, cut from one orbit of the rule so that row b draws the token ``eos`` first as its
    steps[b]-th new token (the orbit is a cycle: a prompt may hold the eos already, which ends nothing). Returns
    (prompts as lists, eos)."""
    n = max(l + s for l, s in zip(lens, steps)) + 1
    orbit = rule_seq(orbit_start, n)
    assert max(steps) <= len(set(orbit)), "a row would meet the eos before its step: the cycle is shorter"
    e = n - 1  # index of the eos in the orbit
    return [orbit[e - s - l + 1:e - s + 1] for l, s in zip(lens, steps)], orbit[e]


def ragged_worker(rank, world, model, device, dtype, ckpt_dir, transport, prompts, new, eos, kw):
    """One rank of a pp = world pipeline: load the checkpoint, run one ragged generation with an eos."""
    from generate_util import make_engine
    from simple_distributed_machine_learning_amd.parallel.generate import generate, pad_prompts
    from simple_distributed_machine_learning_amd.utils.checkpoint import load_checkpoint

    eng = make_engine(model, device, dtype, rank, world, pp=world, kind="gpipe", transport=transport, backend="gloo")
    load_checkpoint(eng, ckpt_dir)
    p, lens = pad_prompts(prompts, 0)
    tok, n = generate(eng, p, new, prompt_lens=lens, eos_token=eos, return_lengths=True, **kw)
    return {"tokens": tok.cpu(), "lengths": n.cpu(), "stages": sorted(eng.stages)}
