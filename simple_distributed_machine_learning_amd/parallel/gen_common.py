"""The one copy of what the generation drivers share (parallel/generate.py, decode_graph.py, session.py): the eval-mode
bracket, the sampling arguments, the token matrix with its per-row state, the decode loop and the result's form."""
from contextlib import contextmanager
from dataclasses import dataclass

import torch

from ..ops.decode import sample_logits, sample_step


@contextmanager
def eval_stages(modules):
    """The stage modules (a list) in eval mode; on the way out, an exception included, each is back in its own."""
    was_training = [m.training for m in modules]
    for m in modules:
        m.eval()
    try:
        yield
    finally:
        for m, tr in zip(modules, was_training):
            m.train(tr)


@dataclass(frozen=True)
class Sampling:
    """The sampler's arguments of one call, checked: ``seed`` is through ``dropout_seed``, ``eos`` is -1 for none."""
    vocab: int
    temperature: float
    top_k: int
    top_p: float
    seed: int
    sample0: int
    eos: int
    pad: int

    def step(self, logits, positions, state):
        """``sample_step`` with its bookkeeping on ``state`` (anything with ``out``, ``done`` and ``gen_len``)."""
        return sample_step(logits, self.vocab, self.temperature, self.top_k, self.top_p, self.seed, self.sample0,
                           positions, state.out, state.done, state.gen_len, self.eos, self.pad)

    def draw(self, logits, positions, rows_per_sample: int):
        """``sample_step``'s draw alone, ``rows_per_sample`` rows of ``logits`` per sample (``lookup``'s verify)."""
        return sample_step(logits, self.vocab, self.temperature, self.top_k, self.top_p, self.seed, self.sample0,
                           positions, rows_per_sample=rows_per_sample)

    def logits(self, logits, positions):
        return sample_logits(logits, self.vocab, self.temperature, self.top_k, self.seed, self.sample0, positions)


def clean_prompts(prompts, lens, padded):
    """``prompts`` [B, S0] with ``padded``'s pad tokens in every row's padding, whatever the caller left there."""
    return torch.where(torch.arange(prompts.shape[1], device=prompts.device)[None, :] < lens[:, None], prompts, padded)


class TokenState:
    """The token matrix of one call on ``prompts`` [B, S0] (``lens_host``: their lengths, None: S0) and what the step
    sampler keeps per row. The prefill reads ``prompts`` and ``lens_dev`` (int32; None: one length). ``out`` int64
    [R, total] and ``lens0`` int64 [R] hold the R = B ``repeat`` rows, every prompt's ``repeat`` times in a row.
    ``stepped``: ``out`` starts as the pad token and the cleaned prompts, and ``sample_step`` writes it, counts in
    ``gen_len`` and sets ``done`` (int32 [R]); otherwise the host stores a column per step, every row ends at ``total``
    and there are no counters. ``storage`` = (out, done, gen_len): a graph session's static buffers, not new ones."""

    def __init__(self, prompts, lens_host, total: int, pad: int, device, stepped: bool = True, repeat: int = 1,
                 storage=None):
        B, S0 = prompts.shape
        R = B * repeat
        self.stepped, self.total = stepped, total
        self.lens0 = torch.tensor(lens_host if lens_host is not None else [S0] * B, dtype=torch.int64, device=device)
        self.lens_dev = self.lens0.to(torch.int32) if lens_host is not None else None
        self.prompts = prompts.to(device)
        if storage is None:  # (the two counters come from one fill)
            storage = (torch.empty((R, total), dtype=torch.int64, device=device),
                       *(torch.zeros((2, R), dtype=torch.int32, device=device) if stepped else (None, None)))
        self.out, self.done, self.gen_len = storage
        if stepped:
            self.out.fill_(pad)
            self.prompts = clean_prompts(self.prompts, self.lens0, self.out[:B, :S0])
        if repeat > 1:
            self.lens0 = self.lens0.repeat_interleave(repeat)
            self.out[:, :S0] = self.prompts.repeat_interleave(repeat, 0)
        else:
            self.out[:, :S0] = self.prompts

    def lengths(self):
        return self.lens0 + self.gen_len if self.stepped else torch.full_like(self.lens0, self.total)

    def sampler(self, sampling: Sampling, positions):
        """``sample(logits, t)`` of ``decode_loop`` for the token at ``positions`` (a cache's device-side lengths): the
        step sampler, or, un-stepped, ``sample_logits`` and the host's store of column S0 + t."""
        if self.stepped:
            return lambda logits, t: sampling.step(logits, positions, self)
        return lambda logits, t: self._store(sampling.logits(logits, positions), t)

    def _store(self, tok, t: int):
        self.out[:, self.prompts.shape[1] + t] = tok
        return tok


def decode_loop(logits, new: int, check: int, sample, advance, all_done) -> int:
    """The loop of every driver but ``lookup``'s: ``sample(logits, t)`` draws token t, ``advance(tok, t)`` processes it
    and returns the next logits. With ``check`` > 0 the host asks ``all_done()`` after every ``check``-th token but the
    last, and stops on yes: the loop's only read from the device. Returns the number of tokens drawn, 1..``new``."""
    for t in range(new):
        tok = sample(logits, t)
        if t + 1 == new or (check and (t + 1) % check == 0 and all_done()):
            break
        logits = advance(tok, t)
    return t + 1


def result(out, lengths, lens0, return_lengths: bool, return_stats: bool, steps: int, row_steps=None):
    """generate()'s result: tokens, (tokens, lengths), (tokens, stats) or (tokens, lengths, stats). ``row_steps``
    None: a row emits one token in every step it takes part in."""
    res = (out, lengths) if return_lengths else out
    if return_stats:
        generated = lengths - lens0
        stats = {"steps": steps, "row_steps": generated.clone() if row_steps is None else row_steps.to(torch.int64),
                 "generated": generated}
        res = (res if isinstance(res, tuple) else (res,)) + (stats,)
    return res
