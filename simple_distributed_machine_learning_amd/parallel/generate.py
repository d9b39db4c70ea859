"""Autoregressive generation on an engine's GPT-2 stages (models/gpt2.py prefill / decode_step; ops/decode.py).

``generate(engine, prompts, max_new_tokens, ...)`` runs on every rank of the pipeline and returns the same
``[B, S0 + max_new_tokens]`` tokens on each. The stages run where the engine placed them (pipe 0's stage -> rank map):
the prompt goes through ``prefill`` (the training forward at the prompt length plus the cache copies), then every
new token through ``decode_step``. Boundaries, ``[B, S0, C]`` for the prefill and ``[B, C]`` per step, cross ranks through
``engine.transport`` into buffers of ``engine.bufs``. The rank of the last stage samples (ops/decode.py sample_logits)
and sends the ``[B]`` tokens to the rank of stage 0 under a tag no schedule uses; at the end the tokens are
broadcast to all ranks.

Sampling is keyed by (seed, sample, position): ``seed`` = ``dropout_seed(seed)``, sample = ``sample0`` + the
prompt's row, position = the index of the token drawn. The result does not depend on the batch split, the placement
or the rank. A decode step reads nothing back from the device: positions live in the cache's device-side lengths and
the sampled tokens stay on the device until the end.

Ragged prompts, stop tokens and top-p (``prompt_lens``, ``eos_token``, ``top_p`` in (0, 1)) move the step onto
``sample_step``, which draws the token and, in the same launch, writes it to the token matrix at the row's own position
(its cache length), counts it and sets the row's done flag on the eos; a done row emits the pad token and writes
nothing. The result is ``[B, Lmax + max_new_tokens]``: a row's prompt, its generated tokens contiguously from its own
length, the pad token after. Only with an eos, every ``stop_check`` steps, the host reads one flag (are all rows done?),
agreed through the pipeline group where there is one. A call without the three arguments runs the lines it always ran.

``graph=True`` (one rank, ROCm bf16, head width 64) replays one captured decode step per token instead of issuing its
launches from the host: parallel/decode_graph.py. The tokens and lengths are those of ``graph=False`` bit for bit.

``lookup=K`` (1..7, one rank) is prompt-lookup speculation: after the prefill and the first token, every step verifies
K drafted tokens per row next to the row's newest one. The drafts are what followed the most recent earlier occurrence
of the row's last ``lookup_ngram`` tokens in its own history (``lookup_step``, on the device); ``decode_block`` runs
the K + 1 positions in one pass and the sampler draws the token of every position, keyed by (seed, sample, position)
as always; a row keeps the tokens up to and including the first one that differs from its draft. An accepted draft IS
the token the plain loop would have drawn, so tokens and lengths are those of ``lookup=0``, bit for bit on the
kernels (docs/NUMERICS.md), in fewer steps. Every sampling mode runs through the step bookkeeping here, so the result
has the step sampler's layout. Every ``stop_check`` steps the host reads one flag (are all rows done or full?), with or
without an eos: that is what ends the loop early. ``return_stats=True`` appends ``{"steps", "row_steps",
"generated"}``.

``prefill_chunk=P`` (one rank) prefills the prompt through ``extend`` in chunks of P positions (models/gpt2.py; the
extend-attention kernel) and then decodes as always; it runs on a ``GenerationSession`` (parallel/session.py), which is
also how a cache outlives a call: more tokens, the next turn, appended tokens. It is refused with ``graph=True`` and
with ``lookup > 0``.

``num_samples=n`` (2..64, one rank) returns n continuations of every prompt, ``[B n, S0 + max_new_tokens]`` with row
``b n + j`` sibling j of prompt b. The prompts are prefilled once; every stage's cache is forked (models/gpt2.py
``fork_cache``: the prefilled cache stays as the shared prefix, each row gets ``max_new_tokens`` suffix positions) and
the B n rows decode through ``decode_step_forked``, whose attention (attention_fork.hip) reads a prompt's keys once
for its n siblings. Row ``b n + j`` is the sampler's sample ``sample0 + b n + j``, so siblings draw different noise, and
tokens, lengths and stats are those of the call on ``prompts.repeat_interleave(n, 0)`` bit for bit (docs/NUMERICS.md).
It is refused with ``graph=True``, ``lookup > 0``, ``prefill_chunk > 0`` and pp > 1.

``num_beams=K`` (2..8, one rank) is beam search: K hypotheses per prompt, every step keeping the K continuations with
the highest cumulative log-probability (``beam_step``, ops/reference.py: the rule, its tie-breaks included). The
prompts are prefilled once and every stage's cache forked as for ``num_samples`` (models/gpt2.py ``beam_cache``); a
step is the beam step, the re-parenting of every stage's suffix caches by the step's parents (one gather launch per
stage) and ``decode_step_forked`` on the step's tokens. A hypothesis that draws the eos is finished: it keeps its
score, rides along fed with the pad token and competes with the live ones for its place. The loop ends after
``max_new_tokens`` steps, or at a ``stop_check`` step on which every hypothesis of every prompt is finished (the one
flag the host reads); there is no other early-termination heuristic, so a finished hypothesis can still be displaced
by a live one that overtakes it. At the end the tokens are traced back through the parents and a prompt's hypotheses
ranked by ``score / length ** length_penalty`` (length = generated tokens, the eos included; 0.0: the raw score),
lowest beam first on ties. The result is the best hypothesis per prompt, ``[B, S0 + max_new_tokens]``, or with
``return_beams=True`` all ``[B K, ...]`` rows, best first per prompt, followed by their scores (fp32 [B K], the
cumulative log-probabilities). It is refused with sampling (``temperature > 0``, ``top_k > 0``, ``top_p`` in (0, 1)),
``num_samples > 1``, ``graph=True``, ``lookup > 0``, ``prefill_chunk > 0`` and pp > 1; on the kernels B K may not
exceed 64 rows (the decode projections' bound) and the vocabulary 65536.

``kv_dtype="fp8"`` stores every stage's KV cache as e4m3 bytes with one int8 exponent per (sample, key, head) row
(ops/decode.py ``kv_quantize``: 66 bytes per row for 128): the prefill quantises the prompt's k and v in one launch per
layer and every decode step runs ``attention_decode_fp8``, which streams half the bytes. The numerics are those of the
format (docs/NUMERICS.md "fp8 KV cache"), so the tokens may differ from ``"bf16"``'s; a row's tokens still do not
depend on the batch, and ``graph=True`` replays them bit for bit. It serves the plain loop (any pp, ragged prompts,
eos, top-k, top-p) and ``graph=True``; it is refused with ``lookup > 0``, ``num_samples > 1``, ``num_beams > 1``,
``prefill_chunk > 0`` and by ``GenerationSession``. ``"bf16"`` (the default) runs the lines it always ran.

``kv_dtype="fp4"`` is the same path on OCP microscaling e2m1 (ops/decode.py ``kv_quantize_fp4``: 16 bytes of nibbles
and one int8 exponent per block of 32 channels, 34 bytes per row): ``kv_quantize_rows_fp4`` in the prefill,
``attention_decode_fp4`` in every step. It serves and refuses what ``"fp8"`` does; its rounding is much coarser
(docs/NUMERICS.md "fp4 KV cache" has the bound and the measured drift).

``repetition_penalty``, ``no_repeat_ngram_size`` and ``return_logprobs`` move the step onto ``sample_step`` as well,
on its variant that reads the row's own history out[row, :pos] in the same launch (ops/reference.py
``process_logits`` is the rule; csrc/kernels/sample_penalty.hip): a logit whose token occurs in the history is
multiplied by theta where negative and by 1 / theta otherwise and rounded to bf16 again, then every token that would
complete an n-gram the history already holds gets -inf, and temperature, top-k, top-p and the noise work on that row
unchanged. The log-probability is that of the raw logits (no penalty, temperature 1) for the token the row emits:
what the model thought of it, whatever the knobs; ``logprobs.sum(1)`` ranks the rows of ``num_samples``. A step is
still one sampler launch and reads nothing back, so every driver that samples through ``Sampling.step`` serves them:
the plain loop at any pp, ``graph=True``, ``num_samples``, ``prefill_chunk`` and ``GenerationSession``. Refused with
``lookup > 0`` (a verify row's history would have to include the step's own drafts) and ``num_beams > 1``; on the
kernels a penalty or a ban takes a vocabulary of at most 65536.

Limitations: tensor parallelism, data parallelism and ``--schedule rotate`` are refused. With pp ranks one rank works
at a time (a token must leave the last stage before stage 0 can embed it); several sample groups in flight would fill
the bubble and are not implemented. ``graph=True`` is refused with pp > 1: the step's boundaries cross ranks between
kernels, and a transport call cannot be part of a captured graph. ``lookup > 0`` is refused with ``graph=True`` (the
verify step is not captured yet) and with pp > 1 (the other ranks' caches would need the accepted counts); on the
kernels B * (K + 1) may not exceed 64 rows.

``generate()`` itself checks the arguments and hands the call to one driver: ``_generate_pipeline`` (the plain loop),
``_generate_lookup``, ``_generate_forked``, ``_generate_beam``, ``_generate_chunked`` or decode_graph's
``generate_graphed``. The token state, the sampling arguments, the decode loop and the form of the result are one copy,
parallel/gen_common.py.
"""
from __future__ import annotations

from functools import partial
from typing import Optional

import torch

from ..ops.decode import (ATTENTION_FORK_MAX_N, BEAM_MAX_K, BEAM_MAX_ROWS, BEAM_MAX_VOCAB, KV_DTYPES,
                          LINEAR_DECODE_MAX_M, LOOKUP_MAX_DRAFTS, LOOKUP_MAX_NGRAM, beam_backtrack, beam_step,
                          lookup_step)
from ..ops.reference import check_penalty
from .decode_graph import check_graph, generate_graphed
from .gen_common import Sampling, TokenState, decode_loop, eval_stages, result
from .session import GenerationSession

# message tags no schedule produces: message_tag() keeps mb * 4096 + stage in the bits above 2, and a schedule's
# stage index is far below 4095
_TAG_STAGE = 4095
PL_GEN_ACT, PL_GEN_TOK = 0, 1


def _tag(kind: int, stage: int, step: int) -> int:
    from .p2p import message_tag

    return message_tag(kind, stage & 1, _TAG_STAGE, step * 64 + (stage >> 1))


def _check(engine, prompts, max_new_tokens: int):
    mesh = engine.mesh
    if mesh.tp > 1:
        raise ValueError(f"generate: tensor parallelism (tp={mesh.tp}) is not supported")
    if mesh.dp > 1:
        raise ValueError(f"generate: data parallelism (dp={mesh.dp}) is not supported; run one pipeline")
    if engine.kind == "rotate":
        raise ValueError("generate: schedule 'rotate' places every stage on every rank; use gpipe or 1f1b")
    if not all(hasattr(m, "decode_step") for m in engine.stages.values()):
        raise ValueError(f"generate: model {engine.spec.name!r} has no decode path (gpt2 / gpt2_tiny have)")
    if not torch.is_tensor(prompts):
        lens = {len(p) for p in prompts}
        if len(lens) != 1:
            raise ValueError(f"generate: prompts of unequal lengths {sorted(lens)}; one call takes one length")
        prompts = torch.tensor([list(p) for p in prompts], dtype=torch.int64)
    if prompts.dim() != 2 or prompts.dtype != torch.int64 or prompts.shape[0] < 1 or prompts.shape[1] < 1:
        raise ValueError("generate: prompts must be a non-empty int64 [B, S0] tensor")
    cfg = next(iter(engine.stages.values())).cfg
    S0 = prompts.shape[1]
    if max_new_tokens < 0 or S0 + max_new_tokens > cfg.block_size:
        raise ValueError(f"generate: prompt length {S0} + max_new_tokens {max_new_tokens} exceeds block_size="
                         f"{cfg.block_size}")
    return prompts, cfg


def pad_prompts(prompts, pad_token: int = 0):
    """(tokens int64 [B, Lmax] right-padded with ``pad_token``, lengths int32 [B]) from a list of token-id lists of
    any non-zero lengths: the ``prompts`` / ``prompt_lens`` pair of a ragged ``generate`` call."""
    rows = [list(p) for p in prompts]
    if not rows or not all(rows):
        raise ValueError("pad_prompts: every prompt needs at least one token")
    lmax = max(len(r) for r in rows)
    t = torch.tensor([r + [int(pad_token)] * (lmax - len(r)) for r in rows], dtype=torch.int64)
    return t, torch.tensor([len(r) for r in rows], dtype=torch.int32)


def _check_step(cfg, prompts, top_p, prompt_lens, eos_token, pad_token, stop_check, temperature=0.0):
    """The refusals of the sampling arguments; returns the prompt lengths as a list (None: one length)."""
    if temperature < 0:
        raise ValueError(f"generate: temperature must be >= 0, got {temperature}")
    if not 0.0 <= float(top_p) <= 1.0:
        raise ValueError(f"generate: top_p must be in [0, 1], got {top_p}")
    V = cfg.vocab_size
    if eos_token is not None and not 0 <= int(eos_token) < V:
        raise ValueError(f"generate: eos_token {eos_token} is outside the vocabulary [0, {V})")
    if not 0 <= int(pad_token) < V:
        raise ValueError(f"generate: pad_token {pad_token} is outside the vocabulary [0, {V})")
    if int(stop_check) < 0:
        raise ValueError(f"generate: stop_check must be >= 0, got {stop_check}")
    if prompt_lens is None:
        return None
    B, Lmax = prompts.shape
    lens = [int(v) for v in (prompt_lens.tolist() if torch.is_tensor(prompt_lens) else prompt_lens)]
    if len(lens) != B:
        raise ValueError(f"generate: {len(lens)} prompt_lens for {B} prompts")
    if min(lens) < 1 or max(lens) > Lmax:
        raise ValueError(f"generate: prompt_lens must be in 1..{Lmax} (the prompts' width), got {lens}")
    return lens


def _check_lookup(engine, cfg, B: int, lookup, lookup_ngram, graph: bool):
    """The refusals of ``lookup`` / ``lookup_ngram``."""
    if isinstance(lookup, bool) or not isinstance(lookup, int) or not 0 <= lookup <= LOOKUP_MAX_DRAFTS:
        raise ValueError(f"generate: lookup must be an integer in 0..{LOOKUP_MAX_DRAFTS} (drafts per step), got "
                         f"{lookup!r}")
    if isinstance(lookup_ngram, bool) or not isinstance(lookup_ngram, int) or \
            not 1 <= lookup_ngram <= LOOKUP_MAX_NGRAM:
        raise ValueError(f"generate: lookup_ngram must be an integer in 1..{LOOKUP_MAX_NGRAM}, got {lookup_ngram!r}")
    if lookup == 0:
        return
    if graph:
        raise ValueError("generate: lookup > 0 with graph=True is not supported (the verify step is not captured yet)")
    if engine.mesh.pp > 1:
        raise ValueError(f"generate: lookup > 0 with pp={engine.mesh.pp} is not supported (the other ranks' caches "
                         "would need the accepted counts); run one rank")
    on_kernels = engine.device.type == "cuda" and engine.dtype == torch.bfloat16 and cfg.n_embd // cfg.n_head == 64
    if on_kernels and B * (lookup + 1) > LINEAR_DECODE_MAX_M:
        raise ValueError(f"generate: {B} samples x (lookup + 1 = {lookup + 1}) tokens = {B * (lookup + 1)} rows per "
                         f"verify step, but the decode projections take at most {LINEAR_DECODE_MAX_M}")


def _generate_chunked(engine, prompts, lens_host, new: int, sp: Sampling, check: int, prefill_chunk: int):
    """The driver of ``prefill_chunk`` > 0: a session of this call's length (parallel/session.py), run once. ``sp``
    carries this call's seed, so the session needs none of its own."""
    s = GenerationSession(engine, prompts, prompts.shape[1] + new, lens_host, sp.pad, sample0=sp.sample0)
    lens0 = s.lengths.to(torch.int64)
    out, lengths = s.run(new, sp, check, prefill_chunk)
    logp = s.logp
    s.close()
    return (out, lengths, lens0, s.steps), logp


def _check_samples(engine, num_samples, graph: bool, lookup: int, prefill_chunk: int):
    """The refusals of ``num_samples``."""
    if isinstance(num_samples, bool) or not isinstance(num_samples, int) or \
            not 1 <= num_samples <= ATTENTION_FORK_MAX_N:
        raise ValueError(f"generate: num_samples must be an integer in 1..{ATTENTION_FORK_MAX_N}, got {num_samples!r}")
    if num_samples == 1:
        return
    for on, what in ((graph, "graph=True (the forked step is not captured yet)"),
                     (lookup > 0, "lookup > 0 (the verify step does not read a shared prefix yet)"),
                     (prefill_chunk > 0, "prefill_chunk > 0 (a session cannot be forked yet)"),
                     (engine.mesh.pp > 1, f"pp={engine.mesh.pp} (the fork does not cross pipeline ranks yet); run one "
                                          "rank")):
        if on:
            raise ValueError(f"generate: num_samples > 1 is not supported with {what}")


def _generate_forked(engine, st: TokenState, sp: Sampling, new: int, check: int, n: int):
    """The driver of ``num_samples`` = n > 1 (one rank): the B prompts are prefilled once, every stage's cache is forked
    (models/gpt2.py fork_cache) and the B n rows decode through ``decode_step_forked``. Row b n + j is sibling j of
    prompt b and sample ``sample0 + b n + j`` of the sampler: ``st`` holds the rows of the call on
    ``prompts.repeat_interleave(n, 0)``, and the sampler and the loop are that call's, so its bits are too."""
    P = engine.P
    stages = [engine.stages[s] for s in range(P)]
    with eval_stages(stages):
        caches = [m.new_cache(*st.prompts.shape) for m in stages]  # the shared prefixes: the prompt's rows and no more
        x = st.prompts
        for s, m in enumerate(stages):
            x = m.prefill(x, caches[s], lens=st.lens_dev, head_rows=n if s == P - 1 else 1)
        forks = [m.fork_cache(caches[s], n, new) for s, m in enumerate(stages)]

        def advance(x, t):
            for m, fork in zip(stages, forks):
                x = m.decode_step_forked(x, fork)
            return x
        steps = decode_loop(x, new, check, st.sampler(sp, forks[P - 1].lens), advance,
                            lambda: bool(st.done.min().item()))
    return st.out, st.lengths(), st.lens0, steps


def _check_beams(engine, cfg, B: int, num_beams, temperature, top_k, top_p, num_samples, graph: bool,
                 lookup: int, prefill_chunk: int):
    """The refusals of ``num_beams``."""
    if isinstance(num_beams, bool) or not isinstance(num_beams, int) or not 1 <= num_beams <= BEAM_MAX_K:
        raise ValueError(f"generate: num_beams must be an integer in 1..{BEAM_MAX_K}, got {num_beams!r}")
    if num_beams == 1:
        return
    for on, what in ((temperature > 0, "temperature > 0 (beam search does not sample)"),
                     (top_k > 0, "top_k > 0 (beam search does not sample)"),
                     (0.0 < float(top_p) < 1.0, "top_p in (0, 1) (beam search does not sample)"),
                     (num_samples > 1, "num_samples > 1 (the beams are the rows of the fork)"),
                     (graph, "graph=True (the beam step is not captured yet)"),
                     (lookup > 0, "lookup > 0 (the verify step does not read a shared prefix yet)"),
                     (prefill_chunk > 0, "prefill_chunk > 0 (a session cannot be forked yet)"),
                     (engine.mesh.pp > 1, f"pp={engine.mesh.pp} (the fork does not cross pipeline ranks yet); run one "
                                          "rank")):
        if on:
            raise ValueError(f"generate: num_beams > 1 is not supported with {what}")
    if engine.device.type == "cuda" and engine.dtype == torch.bfloat16:
        if B * num_beams > BEAM_MAX_ROWS:
            raise ValueError(f"generate: {B} prompts x num_beams = {num_beams} = {B * num_beams} rows per step, but "
                             f"the beam step and the decode projections take at most {BEAM_MAX_ROWS}")
        if cfg.vocab_size > BEAM_MAX_VOCAB:
            raise ValueError(f"generate: num_beams > 1 takes a vocabulary of at most {BEAM_MAX_VOCAB}, got "
                             f"{cfg.vocab_size}")


def _generate_beam(engine, st: TokenState, sp: Sampling, new: int, check: int, K: int, length_penalty: float):
    """The driver of ``num_beams`` = K > 1 (one rank; module docstring). ``st`` holds the B K rows of the call on
    ``prompts.repeat_interleave(K, 0)``; row b K + j is beam j of prompt b until the final ranking. Returns the rows
    best first per prompt, their lengths and prompt lengths, the steps and the scores."""
    P, dev = engine.P, engine.device
    stages = [engine.stages[s] for s in range(P)]
    B = st.prompts.shape[0]
    R = B * K
    score = torch.full((B, K), -float("inf"), dtype=torch.float32, device=dev)
    score[:, 0] = 0.0  # the K rows of a prompt start identical: only the first may branch
    state = [score.view(R), *torch.zeros((2, R), dtype=torch.int32, device=dev), None]  # score, fin, glen, all_done
    tok_hist = torch.empty((max(new, 1), R), dtype=torch.int64, device=dev)
    par_hist = torch.empty((max(new, 1), R), dtype=torch.int32, device=dev)
    steps = 0
    if new > 0:
        with eval_stages(stages):
            caches = [m.new_cache(*st.prompts.shape) for m in stages]
            x = st.prompts
            for s, m in enumerate(stages):
                x = m.prefill(x, caches[s], lens=st.lens_dev, head_rows=K if s == P - 1 else 1)
            forks = [m.beam_cache(caches[s], K, new) for s, m in enumerate(stages)]

            def sample(logits, t):
                tok, par, *state[:] = beam_step(logits, sp.vocab, K, *state[:3], sp.eos, sp.pad, tok_hist[t],
                                                par_hist[t])
                return tok, par

            def advance(tp, t):
                x, par = tp
                for m, fork in zip(stages, forks):
                    fork.reparent(par)
                    x = m.decode_step_forked(x, fork)
                return x
            steps = decode_loop(x, new, check, sample, advance, lambda: bool(state[3].item()))
    score, _, glen, _ = state
    beam_backtrack(st.out, st.lens0, tok_hist, par_hist, glen, steps, K, sp.pad)
    # the final ranking, once per call: score / length ** length_penalty in fp64, the lowest beam first on ties
    rank = score.double() / glen.clamp(min=1).double().pow(float(length_penalty))
    order = torch.sort(rank.view(B, K), dim=1, descending=True, stable=True).indices
    rows = (torch.arange(B, device=dev)[:, None] * K + order).reshape(R)
    return st.out[rows], (st.lens0 + glen)[rows], st.lens0, steps, score[rows]


def _generate_lookup(engine, st: TokenState, sp: Sampling, new: int, every: int, K: int, ngram: int):
    """The driver of ``lookup`` = K > 0 (one rank): the prefill and the first token as always, then verify steps of
    K + 1 positions per row; every ``every`` steps the host reads one flag (are all rows done or full?)."""
    stages = [engine.stages[s] for s in range(engine.P)]
    B, T, dev = st.prompts.shape[0], K + 1, engine.device
    row_steps = torch.zeros(B, dtype=torch.int32, device=dev)
    steps = 0
    with eval_stages(stages):
        caches = [m.new_cache(B, st.total) for m in stages]
        lens = caches[0].lens
        for c in caches[1:]:  # decode_block leaves the lengths to lookup_step: the stages read one tensor
            c.lens = lens
        x = st.prompts
        for m, c in zip(stages, caches):
            x = m.prefill(x, c, lens=st.lens_dev)
        sp.step(x, lens, st)
        # from here on lens[b] is the column of row b's newest token, which is not in the cache yet
        limit = (st.lens0 + new).to(torch.int32)
        nxt, nq, flag = lookup_step(None, None, None, st.out, lens, limit, st.done, st.gen_len, row_steps, K, ngram,
                                    sp.eos, sp.pad)
        offs = torch.arange(1, T + 1, dtype=torch.int32, device=dev)[None, :]
        for steps in range(1, new):
            x = nxt
            for m, c in zip(stages, caches):
                x = m.decode_block(x, c, nq)
            pos = (lens[:, None] + offs).reshape(B * T)  # the token drawn at row (b, t) sits at lens[b] + t + 1
            g = sp.draw(x, pos, T)
            nxt, nq, flag = lookup_step(g.view(B, T), nxt, nq, st.out, lens, limit, st.done, st.gen_len, row_steps, K,
                                        ngram, sp.eos, sp.pad)
            if every and steps % every == 0 and steps < new - 1 and bool(flag.item()):
                break
    return st.out, st.lengths(), st.lens0, steps, row_steps


def _check_kv_dtype(kv_dtype, lookup: int, num_samples: int, num_beams: int, prefill_chunk: int):
    """The refusals of ``kv_dtype``."""
    if kv_dtype not in KV_DTYPES:
        raise ValueError(f"generate: kv_dtype must be one of {KV_DTYPES}, got {kv_dtype!r}")
    if kv_dtype == "bf16":
        return
    for on, what in ((lookup > 0, "lookup > 0 (the verify step's attention reads a bf16 cache)"),
                     (num_samples > 1, "num_samples > 1 (the fork's attention reads bf16 caches)"),
                     (num_beams > 1, "num_beams > 1 (the beams' caches are bf16 forks)"),
                     (prefill_chunk > 0, "prefill_chunk > 0 (the session's extend attention reads a bf16 cache)")):
        if on:
            raise ValueError(f"generate: kv_dtype={kv_dtype!r} is not supported with {what}")


def _check_grouped(cfg, lookup: int, num_samples: int, num_beams: int, prefill_chunk: int, kv_dtype: str):
    """The refusals of a model with ``n_kv_head != n_head`` (grouped-query attention): the plain loop and
    ``graph=True`` serve its cache."""
    if not getattr(cfg, "grouped", False):
        return
    for on, what in ((lookup > 0, "lookup > 0 (the verify step's attention reads one kv head per query head)"),
                     (num_samples > 1, "num_samples > 1 (the fork's attention reads one kv head per query head)"),
                     (num_beams > 1, "num_beams > 1 (the beams' caches are forks)"),
                     (prefill_chunk > 0, "prefill_chunk > 0 (the extend attention reads one kv head per query head)"),
                     (kv_dtype != "bf16", f"kv_dtype={kv_dtype!r} (the fp8 / fp4 decode kernels read one kv head per "
                                          "query head)")):
        if on:
            raise ValueError(f"generate: n_kv_head={cfg.n_kv_head} != n_head={cfg.n_head} is not supported with {what}")


def _check_penalty(repetition_penalty, no_repeat_ngram_size, return_logprobs, lookup: int = 0, num_beams: int = 1):
    """The refusals of ``repetition_penalty`` / ``no_repeat_ngram_size`` / ``return_logprobs``; returns the three as
    ``Sampling``'s last fields."""
    check_penalty("generate", repetition_penalty, no_repeat_ngram_size)
    sp3 = float(repetition_penalty), int(no_repeat_ngram_size), bool(return_logprobs)
    if sp3 != (1.0, 0, False):
        for on, what in ((lookup > 0, "lookup > 0 (a verify row's history would have to hold the step's own drafts)"),
                         (num_beams > 1, "num_beams > 1 (the beam step ranks by its own scores)")):
            if on:
                raise ValueError("generate: repetition_penalty, no_repeat_ngram_size and return_logprobs are not "
                                 f"supported with {what}")
    return sp3


def _generate_pipeline(engine, cfg, st: TokenState, sp: Sampling, new: int, check: int, kv_dtype: str = "bf16"):
    """The plain driver, on every rank of the pipeline (module docstring)."""
    mesh, dev, P = engine.mesh, engine.device, engine.P
    sched = engine.schedule(1, True)
    owner = [sched.stage_rank(0, s) for s in range(P)]  # pipeline rank of each stage
    me = mesh.pp_rank
    grank = lambda r: mesh.global_rank(mesh.dp_rank, r)  # noqa: E731
    tr = engine.transport
    (B, S0), total = st.prompts.shape, st.total
    mine = [s for s in range(P) if owner[s] == me and s in engine.stages]
    dt, C = engine.dtype, cfg.n_embd
    first, last = owner[0], owner[P - 1]

    def run_stages(x, step: int, prefill: bool):
        """Run this rank's stages in order for one prefill / decode step; x: stage 0's input where this rank holds it.
        Returns the logits where this rank holds the last stage."""
        res = None
        for s in range(P):
            if owner[s] != me:
                continue
            if s > 0 and owner[s - 1] != me:
                shape = (B, S0, C) if prefill else (B, C)
                buf_ = engine.bufs.get(("gen_act", s, prefill), shape, dt)
                tr.irecv(buf_, grank(owner[s - 1]), _tag(PL_GEN_ACT, s, step)).wait()
                x = buf_
            mod = engine.stages[s]
            x = mod.prefill(x, caches[s], lens=st.lens_dev) if prefill else mod.decode_step(x, caches[s])
            if s == P - 1:
                res = x
            elif owner[s + 1] != me:
                tr.isend(x, grank(owner[s + 1]), _tag(PL_GEN_ACT, s + 1, step))
                x = None
        return res

    def exchange_token(tok, step: int):
        """The sampled tokens from the last stage's rank to stage 0's."""
        if first == last:
            return tok
        if (grank(last), grank(first)) not in mesh.p2p_groups:
            # more than two ranks: only pipeline neighbours have a channel, so the tokens go through the pipeline
            # group (a sum in which every other rank adds zeros)
            t_ = tok if me == last else torch.zeros(B, dtype=torch.int64, device=dev)
            tr.all_reduce(t_, channel="fwd", async_op=False)
            return t_
        if me == last:
            tr.isend(tok, grank(first), _tag(PL_GEN_TOK, 0, step))
            return tok
        if me == first:
            buf_ = engine.bufs.get(("gen_tok",), (B,), torch.int64)
            tr.irecv(buf_, grank(last), _tag(PL_GEN_TOK, 0, step)).wait()
            return buf_
        return None

    def all_done() -> bool:
        """The one host read of the stop check: are all rows done? The last stage's rank holds the flags; in a
        pipeline every rank learns the answer through the pipeline group (the others add zeros)."""
        if mesh.pp == 1 or tr is None:
            return bool(st.done.min().item())
        flag = st.done.min().to(torch.int64).reshape(1) if me == last else torch.zeros(1, dtype=torch.int64, device=dev)
        tr.all_reduce(flag, channel="fwd", async_op=False)
        return bool(flag.item())

    def advance(tok, t: int):
        tok = exchange_token(tok, t)
        return run_stages(tok if me == first else None, t + 1, prefill=False)

    with eval_stages([engine.stages[s] for s in mine]):
        caches = {s: engine.stages[s].new_cache(B, total, kv_dtype=kv_dtype) for s in mine}
        # token index S0 + t (ragged: lens[b] + t); only the last stage's rank samples
        sample = st.sampler(sp, caches[P - 1].lens) if me == last else lambda logits, t: None
        logits = run_stages(st.prompts if me == first else None, 0, prefill=True)
        steps = decode_loop(logits, new, check, sample, advance, all_done)
        out, lengths = st.out, st.lengths()
        if tr is not None:
            tr.drain_sends()
            if mesh.pp > 1:  # the last stage's rank holds the tokens and the lengths: everyone gets them, in one sum
                buf = torch.cat([out, lengths[:, None]], 1) if me == last else \
                    torch.zeros((B, total + 1), dtype=torch.int64, device=dev)
                tr.all_reduce(buf, channel="fwd", async_op=False)
                out, lengths = buf[:, :total].contiguous(), buf[:, total].clone()
                if st.logp is not None:  # (zeros on every rank but the last stage's)
                    tr.all_reduce(st.logp, channel="fwd", async_op=False)
    return out, lengths, st.lens0, steps


@torch.no_grad()
def generate(engine, prompts, max_new_tokens: int, temperature: float = 0.0, top_k: int = 0,
             seed: Optional[int] = None, sample0: int = 0, top_p: float = 1.0, prompt_lens=None,
             eos_token: Optional[int] = None, pad_token: int = 0, stop_check: int = 16, return_lengths: bool = False,
             graph: bool = False, lookup: int = 0, lookup_ngram: int = 2, return_stats: bool = False,
             prefill_chunk: int = 0, num_samples: int = 1, num_beams: int = 1, length_penalty: float = 0.0,
             return_beams: bool = False, kv_dtype: str = "bf16", repetition_penalty: float = 1.0,
             no_repeat_ngram_size: int = 0, return_logprobs: bool = False):
    """Tokens [B, S0 + max_new_tokens] (int64, on the engine's device) on every rank; see the module docstring.
    ``seed``: the run seed of the noise (None: 0); ``temperature`` 0 is greedy and draws no noise; ``top_p`` in (0, 1)
    samples inside the nucleus of the top-k candidates. ``prompt_lens`` [B] with right-padded ``prompts`` (see
    ``pad_prompts``): ragged prompts, every row generating up to ``max_new_tokens`` tokens from its own length on.
    ``eos_token``: a row stops after drawing it; what follows is ``pad_token``. ``stop_check``: with an eos, the host
    asks every that many steps whether all rows are done (0: never; the result does not depend on it).
    ``return_lengths``: (tokens, lengths int64 [B]), a row's prompt plus its generated tokens, the eos included.
    ``graph``: replay one captured decode step per token (parallel/decode_graph.py; the same tokens and lengths). The
    session stays on the engine, so the next call of the same shape and sampling arguments captures nothing.
    ``lookup`` = K in 1..7: prompt-lookup speculation with K drafts per row and step, matched on the row's last
    ``lookup_ngram`` tokens (module docstring); the same tokens and lengths in fewer steps. ``stop_check`` then counts
    verify steps and is honoured without an eos too. ``return_stats``: a dict is appended to the result, ``steps`` (the
    host's loop count), ``row_steps`` and ``generated`` (int64 [B] on the device: the steps in which the row emitted a
    token, and its generated tokens). ``prefill_chunk`` = P > 0 (one rank, not with ``graph`` or ``lookup``): the prompt
    goes through ``extend`` in chunks of P positions instead of one ``prefill`` pass, on a ``GenerationSession``
    (parallel/session.py) that lives for this call; 0 runs the lines it always ran. ``num_samples`` = n in 2..64 (one
    rank, not with ``graph``, ``lookup`` or ``prefill_chunk``): n continuations of every prompt from one prefill and
    one copy of the prompt's keys; the result has B n rows, row b n + j sibling j of prompt b, and is that of the call
    on ``prompts.repeat_interleave(n, 0)`` bit for bit (module docstring); 1 runs the lines it always ran.
    ``num_beams`` = K in 2..8 (one rank, greedy arguments only, not with ``num_samples``, ``graph``, ``lookup`` or
    ``prefill_chunk``): beam search (module docstring). The result is each prompt's best hypothesis under
    ``score / length ** length_penalty``; ``return_beams``: all [B K, ...] rows, best first per prompt, and their
    scores fp32 [B K] appended to the result; 1 runs the lines it always ran. ``kv_dtype`` "fp8": an 8-bit KV cache
    (module docstring; the plain loop and ``graph=True`` only); "bf16" runs the lines it always ran.
    ``repetition_penalty`` theta > 0 (1: off), ``no_repeat_ngram_size`` n in 0..8 (0: off): the step sampler draws
    from ``process_logits`` of a row's logits and its own history (module docstring). ``return_logprobs``: fp32
    [R, total] is appended to the result, the model's log-probability of every generated token at its column, 0 at
    prompt and pad columns. Not with ``lookup > 0`` or ``num_beams > 1``; all three off runs the lines it always ran."""
    from ..models.gpt2 import dropout_seed

    new = int(max_new_tokens)
    prompts, cfg = _check(engine, prompts, new)
    lens_host = _check_step(cfg, prompts, top_p, prompt_lens, eos_token, pad_token, stop_check, temperature)
    _check_lookup(engine, cfg, prompts.shape[0], lookup, lookup_ngram, graph)
    if isinstance(prefill_chunk, bool) or not isinstance(prefill_chunk, int) or prefill_chunk < 0:
        raise ValueError(f"generate: prefill_chunk must be an integer >= 0, got {prefill_chunk!r}")
    if prefill_chunk > 0 and (graph or lookup > 0):
        raise ValueError("generate: prefill_chunk > 0 with graph=True or lookup > 0 is not supported (the chunked "
                         "prefill runs on a session, which neither path drives yet)")
    if return_stats and graph:
        raise ValueError("generate: return_stats is not available with graph=True")
    _check_samples(engine, num_samples, graph, lookup, prefill_chunk)
    _check_beams(engine, cfg, prompts.shape[0], num_beams, temperature, top_k, top_p, num_samples,
                 graph, lookup, prefill_chunk)
    _check_kv_dtype(kv_dtype, lookup, num_samples, num_beams, prefill_chunk)
    _check_grouped(cfg, lookup, num_samples, num_beams, prefill_chunk, kv_dtype)
    if graph:
        check_graph(engine, cfg)
    sp = Sampling(cfg.vocab_size, temperature, top_k, top_p, dropout_seed(0 if seed is None else seed), sample0,
                  -1 if eos_token is None else int(eos_token), int(pad_token),
                  *_check_penalty(repetition_penalty, no_repeat_ngram_size, return_logprobs, lookup, num_beams))
    check = int(stop_check) if eos_token is not None else 0
    # the step kernel (sample + bookkeeping in one launch) serves these arguments; without them the host stores a column
    stepped = lens_host is not None or eos_token is not None or 0.0 < float(top_p) < 1.0 or sp.extra
    state = partial(TokenState, prompts, lens_host, prompts.shape[1] + new, sp.pad, engine.device,
                    logprobs=sp.logprobs)
    logp = None
    if num_beams > 1:
        K = num_beams
        *res, scores = _generate_beam(engine, state(repeat=K), sp, new, check, K, float(length_penalty))
        if not return_beams:  # the best hypothesis of every prompt
            res[:3] = [t[::K].contiguous() for t in res[:3]]
        res = result(*res[:3], return_lengths, return_stats, *res[3:])
        if return_beams:
            res = (res if isinstance(res, tuple) else (res,)) + (scores,)
        return res
    if prefill_chunk > 0:
        res, logp = _generate_chunked(engine, prompts, lens_host, new, sp, check, prefill_chunk)
    elif graph and new > 0:
        res = generate_graphed(engine, prompts, lens_host, new, sp, check, kv_dtype)
        logp = engine.decode_session.logp.clone() if sp.logprobs else None
    elif lookup > 0 and new > 0:
        res = _generate_lookup(engine, state(), sp, new, int(stop_check), lookup, lookup_ngram)
    else:
        st = state(stepped=stepped or lookup > 0, repeat=num_samples)
        logp = st.logp
        if new == 0:  # nothing to draw in any of these modes: the prompts come back, cleaned where the mode steps
            res = st.out, st.lengths(), st.lens0, 0
        elif num_samples > 1:
            res = _generate_forked(engine, st, sp, new, check, num_samples)
        else:
            res = _generate_pipeline(engine, cfg, st, sp, new, check, kv_dtype)
    return result(*res[:3], return_lengths, return_stats, *res[3:], logp=logp if sp.logprobs else None)
