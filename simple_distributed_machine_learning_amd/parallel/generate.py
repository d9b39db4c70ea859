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

Limitations: tensor parallelism, data parallelism and ``--schedule rotate`` are refused. With pp ranks one rank works
at a time (a token must leave the last stage before stage 0 can embed it); several sample groups in flight would fill
the bubble and are not implemented. ``graph=True`` is refused with pp > 1: the step's boundaries cross ranks between
kernels, and a transport call cannot be part of a captured graph. ``lookup > 0`` is refused with ``graph=True`` (the
verify step is not captured yet) and with pp > 1 (the other ranks' caches would need the accepted counts); on the
kernels B * (K + 1) may not exceed 64 rows.

``generate()`` itself checks the arguments and hands the call to one driver: ``_generate_pipeline`` (the plain loop),
``_generate_lookup``, ``_generate_forked``, ``_generate_chunked`` or decode_graph's ``generate_graphed``. The token
state, the sampling arguments, the decode loop and the form of the result are one copy, parallel/gen_common.py.
"""
from __future__ import annotations

from functools import partial
from typing import Optional

import torch

from ..ops.decode import ATTENTION_FORK_MAX_N, LINEAR_DECODE_MAX_M, LOOKUP_MAX_DRAFTS, LOOKUP_MAX_NGRAM, lookup_step
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
    s.close()
    return out, lengths, lens0, s.steps


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


def _generate_pipeline(engine, cfg, st: TokenState, sp: Sampling, new: int, check: int):
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
        caches = {s: engine.stages[s].new_cache(B, total) for s in mine}
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
    return out, lengths, st.lens0, steps


@torch.no_grad()
def generate(engine, prompts, max_new_tokens: int, temperature: float = 0.0, top_k: int = 0,
             seed: Optional[int] = None, sample0: int = 0, top_p: float = 1.0, prompt_lens=None,
             eos_token: Optional[int] = None, pad_token: int = 0, stop_check: int = 16, return_lengths: bool = False,
             graph: bool = False, lookup: int = 0, lookup_ngram: int = 2, return_stats: bool = False,
             prefill_chunk: int = 0, num_samples: int = 1):
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
    on ``prompts.repeat_interleave(n, 0)`` bit for bit (module docstring); 1 runs the lines it always ran."""
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
    if graph:
        check_graph(engine, cfg)
    sp = Sampling(cfg.vocab_size, temperature, top_k, top_p, dropout_seed(0 if seed is None else seed), sample0,
                  -1 if eos_token is None else int(eos_token), int(pad_token))
    check = int(stop_check) if eos_token is not None else 0
    # the step kernel (sample + bookkeeping in one launch) serves these arguments; without them the host stores a column
    stepped = lens_host is not None or eos_token is not None or 0.0 < float(top_p) < 1.0
    state = partial(TokenState, prompts, lens_host, prompts.shape[1] + new, sp.pad, engine.device)
    if prefill_chunk > 0:
        res = _generate_chunked(engine, prompts, lens_host, new, sp, check, prefill_chunk)
    elif new == 0:  # nothing to draw in any other mode: the prompts come back, cleaned where the mode steps
        st = state(stepped=stepped or lookup > 0, repeat=num_samples)
        res = st.out, st.lengths(), st.lens0, 0
    elif num_samples > 1:
        res = _generate_forked(engine, state(stepped=stepped, repeat=num_samples), sp, new, check, num_samples)
    elif graph:
        res = generate_graphed(engine, prompts, lens_host, new, sp, check)
    elif lookup > 0:
        res = _generate_lookup(engine, state(), sp, new, int(stop_check), lookup, lookup_ngram)
    else:
        res = _generate_pipeline(engine, cfg, state(stepped=stepped), sp, new, check)
    return result(*res[:3], return_lengths, return_stats, *res[3:])
