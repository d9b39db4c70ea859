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

Limitations: tensor parallelism, data parallelism and ``--schedule rotate`` are refused. With pp ranks one rank works
at a time (a token must leave the last stage before stage 0 can embed it); several sample groups in flight would fill
the bubble and are not implemented.
"""
from __future__ import annotations

from typing import Optional

import torch

from ..ops.decode import sample_logits

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


@torch.no_grad()
def generate(engine, prompts, max_new_tokens: int, temperature: float = 0.0, top_k: int = 0,
             seed: Optional[int] = None, sample0: int = 0) -> torch.Tensor:
    """Tokens [B, S0 + max_new_tokens] (int64, on the engine's device) on every rank; see the module docstring.
    ``seed``: the run seed of the noise (None: 0); ``temperature`` 0 is greedy and draws no noise."""
    from ..models.gpt2 import dropout_seed

    prompts, cfg = _check(engine, prompts, int(max_new_tokens))
    if temperature < 0:
        raise ValueError(f"generate: temperature must be >= 0, got {temperature}")
    mesh, dev, P = engine.mesh, engine.device, engine.P
    sched = engine.schedule(1, True)
    owner = [sched.stage_rank(0, s) for s in range(P)]  # pipeline rank of each stage
    me = mesh.pp_rank
    grank = lambda r: mesh.global_rank(mesh.dp_rank, r)  # noqa: E731
    tr = engine.transport
    B, S0 = prompts.shape
    new = int(max_new_tokens)
    total = S0 + new
    prompts = prompts.to(dev)
    out = torch.empty((B, total), dtype=torch.int64, device=dev)
    out[:, :S0] = prompts
    if new == 0:
        return out
    nseed = dropout_seed(0 if seed is None else seed)
    mine = [s for s in range(P) if owner[s] == me and s in engine.stages]
    was_training = {s: engine.stages[s].training for s in mine}
    for s in mine:
        engine.stages[s].eval()
    caches = {s: engine.stages[s].new_cache(B, total) for s in mine}
    dt = engine.dtype
    C = cfg.n_embd
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
                buf = engine.bufs.get(("gen_act", s, prefill), shape, dt)
                tr.irecv(buf, grank(owner[s - 1]), _tag(PL_GEN_ACT, s, step)).wait()
                x = buf
            mod = engine.stages[s]
            x = mod.prefill(x, caches[s]) if prefill else mod.decode_step(x, caches[s])
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
            buf = engine.bufs.get(("gen_tok",), (B,), torch.int64)
            tr.irecv(buf, grank(last), _tag(PL_GEN_TOK, 0, step)).wait()
            return buf
        return None

    try:
        tok = None
        for t in range(new):  # token index S0 + t
            x = (prompts if t == 0 else tok) if me == first else None
            logits = run_stages(x, t, prefill=(t == 0))
            if me == last:
                cache = caches[P - 1]
                tok = sample_logits(logits, cfg.vocab_size, temperature, top_k, nseed, sample0, cache.lens)
                out[:, S0 + t] = tok
            if t + 1 < new:
                tok = exchange_token(tok, t)
        if tr is not None:
            tr.drain_sends()
            if mesh.pp > 1:  # the last stage's rank holds the tokens: everyone gets them
                mask = out if me == last else out.zero_()
                tr.all_reduce(mask, channel="fwd", async_op=False)
    finally:
        for s in mine:
            engine.stages[s].train(was_training[s])
    return out
