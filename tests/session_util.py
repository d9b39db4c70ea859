"""Shared pieces of the generation-session tests (CPU twins and GPU kernels): rows that follow the synthetic data's
rule, the top-1 / top-2 logit gap of a finished run, the session's cache invariant, and the run-through-the-stages
helpers of the chunked-prefill checks."""
from __future__ import annotations

import torch

from generate_util import RULE_A, RULE_B, VOCAB, nocache_logits


def rule_next(tok: int, n: int):
    """The n tokens the rule t' = (a t + b) mod 97 brings after ``tok``."""
    row = []
    for _ in range(n):
        tok = (int(tok) * RULE_A + RULE_B) % VOCAB
        row.append(tok)
    return row


def rule_rows(starts, length: int):
    return torch.tensor([[int(t)] + rule_next(t, length - 1) for t in starts], dtype=torch.int64)


def rows_of(tokens, lengths):
    """A session's or generate()'s result as lists, each row up to its own length."""
    return [r[:n] for r, n in zip(tokens.cpu().tolist(), lengths.cpu().tolist())]


def min_gap(engine, tokens, lengths, first):
    """The smallest top-1 / top-2 logit gap over the drawn positions first[b] .. lengths[b] - 1 of a finished run, from
    the training-path forward of each row."""
    gaps = []
    for row, n, f in zip(tokens.cpu(), lengths.cpu().tolist(), list(first)):
        if n <= f:
            continue
        lg = nocache_logits(engine, row[None, :n].to(engine.device))[0, f - 1:n - 1, :VOCAB].float()
        top2 = lg.topk(2, dim=-1).values
        gaps.append(float((top2[:, 0] - top2[:, 1]).min()))
    return min(gaps)


def check_invariant(session):
    """On every stage cache.lens[b] == lengths[b] - 1, and the host's copies agree with the device."""
    lengths = session.lengths.cpu()
    for c in session.caches:
        assert torch.equal(c.lens.cpu(), lengths - 1), (c.lens.tolist(), lengths.tolist())
        assert c.n == int(lengths.max()) - 1
    assert session._len_h == lengths.tolist() and session._done_h == [bool(v) for v in session.done.cpu().tolist()]


@torch.no_grad()
def prefill_logits(engine, prompts, lens=None):
    """One-shot prefill through the engine's stages: the logits [B, ld] of each row's last position."""
    B, S0 = prompts.shape
    x = prompts.to(engine.device)
    for s in range(engine.P):
        m = engine.stages[s]
        c = m.new_cache(B, S0)
        x = m.prefill(x, c) if lens is None else m.prefill(x, c, lens=lens.to(engine.device))
    return x


@torch.no_grad()
def extend_logits(engine, prompts, chunk: int, lens=None, smax=None):
    """The same prompt through ``extend`` in chunks of ``chunk`` positions (ragged: per-row counts per chunk, the logits
    of the chunk that held a row's last token). Returns (logits [B, ld], the stages' caches)."""
    B, S0 = prompts.shape
    dev = engine.device
    u = [S0] * B if lens is None else [int(v) for v in lens.tolist()]
    caches = [engine.stages[s].new_cache(B, smax or S0) for s in range(engine.P)]
    start = [0] * B
    logits = None
    for c0 in range(0, max(u), chunk):
        nq_h = [max(0, min(ub - c0, chunk)) for ub in u]
        T = max(nq_h)
        idx = torch.tensor([[min(st + t, S0 - 1) for t in range(T)] for st in start], dtype=torch.int64)
        x = prompts.gather(1, idx).to(dev)
        nq = torch.tensor(nq_h, dtype=torch.int32, device=dev)
        for s in range(engine.P):
            caches[s].n = max(st + q for st, q in zip(start, nq_h) if q > 0) - T
            x = engine.stages[s].extend(x, caches[s], None if lens is None and T == chunk else nq)
        start = [st + q for st, q in zip(start, nq_h)]
        ends = torch.tensor([0 < ub - c0 <= chunk for ub in u], dtype=torch.bool, device=dev)
        logits = x if logits is None else torch.where(ends[:, None], x, logits)
    return logits, caches
