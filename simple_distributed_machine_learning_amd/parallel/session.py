"""A generation session: the token matrix and one KV cache per stage kept between calls (models/gpt2.py prefill /
extend / decode_step; ops/decode.py).

    s = GenerationSession(engine, prompts, max_len, prompt_lens=None, pad_token=0, seed=None, sample0=0)
    tokens, lengths = s.generate(32, temperature=0.9, top_k=20)   # [B, max_len], [B]
    tokens, lengths = s.generate(32, temperature=0.9, top_k=20)   # the tokens of one generate(64) call, bit for bit
    s.append(more_tokens, lens)                                   # the next turn, a tool result: 0..A tokens per row
    tokens, lengths = s.generate(32, eos_token=9)
    s.close()

State: ``out`` int64 [B, max_len] padded with ``pad_token``; ``lengths`` and ``done`` int32 [B] on the device; one
cache of [B, max_len] positions per stage. The sampler's noise is keyed by (seed, sample0 + row, position), as in
``generate()``, so where a call ends does not change what is drawn.

Invariant between calls: on every stage ``cache.lens[b] == lengths[b] - 1``: a row's newest token is known but not yet
processed. (Before the first ``generate`` the caches are empty and the whole prompt is unprocessed.) ``generate``
restores it for every row, the rows that are done included: a done row rides along in ``decode_step`` as in
``generate()``, and its cache length is taken back by one after each step, so it keeps rewriting the one row past its
history, which its revival overwrites before any read.

``generate`` first catches up on the unprocessed tokens u_b of every row (0 for a done row, else lengths[b] -
cache.lens[b]) and keeps the logits of each row's last token:
  * every cache empty and ``prefill_chunk == 0``: ``prefill``, the lines and bits of ``generate()``;
  * no row with u_b > 1: one ``decode_step``; this is what makes two calls equal one long call bit for bit;
  * otherwise ``extend`` over chunks of P positions, P = ``prefill_chunk`` or max u_b: chunk c carries
    clamp(u_b - c P, 0, P) positions of each row, counted from the row's own cached length, and a row keeps the logits
    of the chunk that held its last token (a select on the device).
Then the loop of ``generate()`` itself (parallel/gen_common.py ``decode_loop``; the session is the sampler's token
state, ``gen_len`` its ``lengths``): ``sample_step`` (token, its place in ``out``, the length, the done flag on the
eos), ``decode_step``, and with an eos the stop check every ``stop_check`` steps.

Host synchronisation: one read of ``lengths`` / ``done`` at the end of a ``generate`` call (plus the stop checks with an
eos), none per step. It makes the host's bounds exact: ``append`` and the next ``generate`` check against ``max_len``
and size their chunks without touching the device.

Refused: pp > 1, tp > 1, dp > 1, ``--schedule rotate`` (sessions across pipeline ranks are a follow-up, as are
sessions inside the captured graph of ``graph=True``), ``max_len > block_size``, ``prefill_chunk < 0``, and an
``append`` or ``generate`` that would pass ``max_len``.
"""
from __future__ import annotations

from typing import Optional

import torch

from .gen_common import Sampling, clean_prompts, decode_loop, eval_stages


def _as_rows(tokens, lens, B: int, what: str):
    """(int64 [B, A] tensor, list of B counts) from a [B, A] tensor with optional counts, or a list of B lists."""
    if not torch.is_tensor(tokens):
        rows = [list(r) for r in tokens]
        if lens is None:
            lens = [len(r) for r in rows]
        width = max([len(r) for r in rows] + [1])
        tokens = torch.tensor([r + [0] * (width - len(r)) for r in rows], dtype=torch.int64).reshape(len(rows), width)
    if tokens.dim() != 2 or tokens.dtype != torch.int64 or tokens.shape[0] != B:
        raise ValueError(f"{what}: tokens must be int64 [B = {B}, A] (or {B} lists), got {tuple(tokens.shape)} "
                         f"{tokens.dtype}")
    A = tokens.shape[1]
    n = [A] * B if lens is None else [int(v) for v in (lens.tolist() if torch.is_tensor(lens) else lens)]
    if len(n) != B or min(n) < 0 or max(n) > A:
        raise ValueError(f"{what}: lens must be {B} counts in 0..{A} (the tokens' width), got {n}")
    return tokens, n


class GenerationSession:
    """See the module docstring. One rank; the engine's stages all live on it."""

    def __init__(self, engine, prompts, max_len: int, prompt_lens=None, pad_token: int = 0,
                 seed: Optional[int] = None, sample0: int = 0):
        from ..models.gpt2 import dropout_seed
        from .generate import _check, _check_step

        mesh = engine.mesh
        if mesh.pp > 1:
            raise ValueError(f"GenerationSession: pp={mesh.pp} is not supported (the caches of a session live on one "
                             "rank); run one rank")
        prompts, cfg = _check(engine, prompts, 0)  # tp, dp, rotate, a decode path, the prompts' form
        max_len = int(max_len)
        if max_len > cfg.block_size:
            raise ValueError(f"GenerationSession: max_len {max_len} exceeds block_size={cfg.block_size}")
        if prompts.shape[1] > max_len:
            raise ValueError(f"GenerationSession: prompts of width {prompts.shape[1]} do not fit max_len={max_len}")
        lens_host = _check_step(cfg, prompts, 1.0, prompt_lens, None, pad_token, 0)
        self.engine, self.cfg = engine, cfg
        self.max_len, self.pad_token, self.sample0 = max_len, int(pad_token), int(sample0)
        self.seed = dropout_seed(0 if seed is None else seed)
        dev = self.device = engine.device
        B, S0 = prompts.shape
        self.B = B
        self._ragged = lens_host is not None
        self._width0 = S0  # the first prefill runs over the prompts' own width, as generate() does
        self._len_h = list(lens_host) if self._ragged else [S0] * B  # the host's copies: exact between calls
        self._cached_h = [0] * B
        self._done_h = [False] * B
        self._fresh = True  # every cache empty
        self.lengths = self.gen_len = torch.tensor(self._len_h, dtype=torch.int32, device=dev)
        self.done = torch.zeros(B, dtype=torch.int32, device=dev)
        self.out = torch.full((B, max_len), self.pad_token, dtype=torch.int64, device=dev)
        self.out[:, :S0] = clean_prompts(prompts.to(dev), self.lengths, self.out[:, :S0])
        self.stages = [engine.stages[s] for s in range(engine.P)]
        self.caches = [m.new_cache(B, max_len) for m in self.stages]
        self.steps = 0  # decode loop steps of the last generate call

    def close(self):
        """Drop the caches and the token matrix; the session takes no further calls."""
        self.caches = self.out = self.lengths = self.gen_len = self.done = None

    def _open(self, what: str):
        if self.caches is None:
            raise ValueError(f"GenerationSession.{what}: the session is closed")

    # ---- append ------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def append(self, tokens, lens=None):
        """Row b's first ``lens[b]`` (0..A; None: all A) of ``tokens`` [B, A] go to out[b, lengths[b]:] and its length
        grows by as many. A row that gets at least one token is no longer done: this is how the turn after an eos
        starts. Nothing is processed here; the next ``generate`` catches up."""
        self._open("append")
        tokens, n = _as_rows(tokens, lens, self.B, "GenerationSession.append")
        V = self.cfg.vocab_size
        for b in range(self.B):
            if self._len_h[b] + n[b] > self.max_len:
                raise ValueError(f"GenerationSession.append: row {b} holds {self._len_h[b]} tokens; {n[b]} more would "
                                 f"pass max_len={self.max_len}")
        if tokens.numel() and (int(tokens.min()) < 0 or int(tokens.max()) >= V):
            raise ValueError(f"GenerationSession.append: token ids must be in [0, {V})")
        if max(n) == 0:
            return
        # the host knows every length exactly: the cells to write, their tokens and the counts go over in one copy
        host = tokens.cpu().tolist()
        cells = [(b, self._len_h[b] + t, host[b][t]) for b in range(self.B) for t in range(n[b])]
        pk = torch.tensor([c[0] for c in cells] + [c[1] for c in cells] + [c[2] for c in cells] + n,
                          dtype=torch.int64).to(self.device)
        N = len(cells)
        self.out.index_put_((pk[:N], pk[N:2 * N]), pk[2 * N:3 * N])
        n_dev = pk[3 * N:].to(torch.int32)
        self.lengths.add_(n_dev)
        self.done.mul_(n_dev == 0)
        for b in range(self.B):
            self._len_h[b] += n[b]
            self._done_h[b] = self._done_h[b] and n[b] == 0

    # ---- generate ----------------------------------------------------------------------------------------------
    def _bound(self, n: int):
        for c in self.caches:
            c.n = n

    def _run(self, fn):
        """x through the stages in order; fn(stage module, its cache, x) -> x."""
        x = None
        for m, c in zip(self.stages, self.caches):
            x = fn(m, c, x)
        return x

    def _catch_up(self, u, prefill_chunk: int, may_be_done: bool):
        """Process the unprocessed tokens (u[b] per row); returns the logits [B, ld] of each live row's last token."""
        dev, B = self.device, self.B
        if self._fresh and prefill_chunk == 0:
            # generate()'s lines: the prompt in one pass (after an append: over the longest row, ragged)
            plain = not self._ragged and self._len_h == [self._width0] * B
            W = self._width0 if max(self._len_h) <= self._width0 else max(self._len_h)
            x0 = self.out[:, :W].contiguous()
            if plain:
                logits = self._run(lambda m, c, x: m.prefill(x0 if x is None else x, c))
            else:
                logits = self._run(lambda m, c, x: m.prefill(x0 if x is None else x, c, lens=self.lengths))
            self._cached_h = list(self._len_h)
            return logits
        if max(u) <= 1:
            # the newest token of every row (a done row rides along), as the loop of generate() runs it
            tok = self.out.gather(1, self.caches[0].lens.to(torch.int64)[:, None])[:, 0]
            return self._decode(tok, may_be_done)
        P = prefill_chunk if prefill_chunk > 0 else max(u)
        # The host knows every length exactly, so each chunk's token columns, counts and "my last token is in this
        # chunk" flags are built here and go to the device in one copy, before the first pass is enqueued (a copy
        # from the host waits for the stream).
        plan, flat = [], []
        for c0 in range(0, max(u), P):
            nq_h = [max(0, min(ub - c0, P)) for ub in u]
            T = max(nq_h)
            cols = [min(ch + c0 + t, self.max_len - 1) for ch in self._cached_h for t in range(T)]
            plan.append((nq_h, T, len(flat)))
            flat += cols + nq_h + [int(0 < ub - c0 <= P) for ub in u]
        pk = torch.tensor(flat, dtype=torch.int64).to(dev)
        logits = None
        for nq_h, T, o in plan:
            x0 = self.out.gather(1, pk[o:o + B * T].view(B, T))
            nq = pk[o + B * T:o + B * T + B].to(torch.int32)
            ends = pk[o + B * T + B:o + B * T + 2 * B] != 0
            # the kernels need n_keys = n + T >= every live row's last new row; rows above it are dead in this chunk
            self._bound(max(ch + q for ch, q in zip(self._cached_h, nq_h) if q > 0) - T)
            lg = self._run(lambda m, c, x: m.extend(x0 if x is None else x, c, nq))
            self._cached_h = [ch + q for ch, q in zip(self._cached_h, nq_h)]
            logits = lg if logits is None else torch.where(ends[:, None], lg, logits)
        return logits

    def _decode(self, tok, may_be_done: bool):
        """One decode_step on every stage under the host's exact bound; a done row's cache length stays put."""
        self._bound(max(self._cached_h))  # (a row that went done during this call counts as advancing: a bound)
        logits = self._run(lambda m, c, x: m.decode_step(tok if x is None else x, c))
        if may_be_done:
            for c in self.caches:
                c.lens.sub_(self.done)
        self._cached_h = [ch + (0 if d else 1) for ch, d in zip(self._cached_h, self._done_h)]
        return logits

    def generate(self, max_new_tokens: int, temperature: float = 0.0, top_k: int = 0, top_p: float = 1.0,
                 eos_token: Optional[int] = None, stop_check: int = 16, prefill_chunk: int = 0):
        """Up to ``max_new_tokens`` more tokens per row that is not done; returns (tokens int64 [B, max_len], lengths
        int64 [B]), copies of the session's state. The sampling arguments are ``generate()``'s. ``prefill_chunk`` = P
        > 0: the catch-up always runs through ``extend``, at most P positions per row and pass."""
        from .generate import _check_step

        self._open("generate")
        new = int(max_new_tokens)
        if int(prefill_chunk) < 0:
            raise ValueError(f"generate: prefill_chunk must be >= 0, got {prefill_chunk}")
        _check_step(self.cfg, self.out, top_p, None, eos_token, self.pad_token, stop_check, temperature)
        if new < 0:
            raise ValueError(f"generate: max_new_tokens must be >= 0, got {new}")
        for b in range(self.B):
            if not self._done_h[b] and self._len_h[b] + new > self.max_len:
                raise ValueError(f"GenerationSession.generate: row {b} holds {self._len_h[b]} tokens; {new} more "
                                 f"would pass max_len={self.max_len}")
        sp = Sampling(self.cfg.vocab_size, temperature, top_k, top_p, self.seed, self.sample0,
                      -1 if eos_token is None else int(eos_token), self.pad_token)
        return self.run(new, sp, int(stop_check) if eos_token is not None else 0, int(prefill_chunk))

    @torch.no_grad()
    def run(self, new: int, sp: Sampling, check: int, prefill_chunk: int):
        """``generate`` on checked arguments (``generate()`` with ``prefill_chunk`` > 0 comes in here)."""
        self.steps = 0
        if new == 0 or all(self._done_h):
            return self.out.clone(), self.lengths.to(torch.int64)
        may_be_done = sp.eos >= 0 or any(self._done_h)
        with eval_stages(self.stages):
            u = [0 if d else n - ch for n, ch, d in zip(self._len_h, self._cached_h, self._done_h)]
            logits = self._catch_up(u, prefill_chunk, may_be_done)
            self._fresh = False
            lens = self.caches[-1].lens  # the position of the token drawn: every live row's length
            self.steps = decode_loop(logits, new, check, lambda logits, t: sp.step(logits, lens, self),
                                     lambda tok, t: self._decode(tok, may_be_done),
                                     lambda: bool(self.done.min().item()))
        # the one read of the call: the host's bounds become exact again
        state = torch.stack([self.lengths, self.done]).tolist()
        self._len_h, self._done_h = [int(v) for v in state[0]], [bool(v) for v in state[1]]
        self._cached_h = [n - 1 for n in self._len_h]
        self._bound(max(self._cached_h))
        return self.out.clone(), self.lengths.to(torch.int64)
