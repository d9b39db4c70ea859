"""The graph-replayed decode loop of ``generate(..., graph=True)`` (parallel/generate.py).

An eager decode step is about 150 launches, and at GPT-2 small the host needs several times longer to issue them than
the device to run them. Here one step is captured once with ``torch.cuda.graph`` and replayed once per token:

  * the prompt's prefill and the first token's sampling run eagerly, as in the eager call;
  * the captured step is this rank's ``decode_step(fused=True)`` over all its stages (models/gpt2.py: the one-launch
    projections, the attention's grid over the whole cache so that nothing depends on the step's index),
    ``sample_step`` (the token, the token matrix, the done flags and the lengths, at device-side positions), and the
    copy of the token into the static buffer that the next replay embeds. One stream, a linear chain of nodes;
  * the stop check stays outside the graph: every ``stop_check`` steps the host reads one flag, as in the eager call.
    The loop here checks before replay t what the eager loop (parallel/gen_common.py) checks after token t - 1.

Every sampling mode goes through ``sample_step`` here (the eager call without ragged prompts, eos or top-p writes
``out[:, S0 + t]`` from the host, a column a graph would freeze); it draws the tokens ``sample_logits`` draws, so the
tokens and lengths are those of the eager call bit for bit.

A session (the static token / out / done / length buffers, the KV caches with their counters, the graph) stays on the
engine as ``engine.decode_session``; at most one. The next call with the same key, (B, total width, temperature,
top_k, top_p, seed, sample0, eos, pad, the parameters' storage addresses), replays it without capturing again; any
other key replaces it. The weights are read in place, so optimizer steps between two calls need no new capture as long
as the storages stay. ``engine.decode_graph_captures`` counts the captures.

Refused: a device that is not ROCm, a dtype or head width that runs the torch twins (there is nothing to capture), and
pp > 1 (a boundary crosses ranks between two kernels of the step, and a transport call cannot sit inside a graph).
"""
from __future__ import annotations

from dataclasses import astuple, replace

import torch

from .gen_common import Sampling, TokenState, eval_stages


def check_graph(engine, cfg) -> None:
    """The refusals of ``graph=True``."""
    dev = engine.device
    if engine.mesh.pp > 1:
        raise ValueError(f"generate: graph=True is not supported with pp={engine.mesh.pp}: the step's boundaries cross "
                         "ranks between kernels; run one rank, or graph=False")
    if dev.type != "cuda" or torch.version.hip is None:
        raise ValueError(f"generate: graph=True replays a captured step on a ROCm device; the engine is on {dev}")
    D = cfg.n_embd // cfg.n_head
    if engine.dtype != torch.bfloat16 or D != 64:
        raise ValueError(f"generate: graph=True captures the decode kernels (bf16, head width 64); dtype "
                         f"{engine.dtype} with head width {D} runs the torch twins; use graph=False")


class DecodeSession:
    """The static state of one captured decode step; see the module docstring."""

    def __init__(self, engine, key, B: int, total: int, _sites=None):
        """``_sites`` (tools/bench_generate.py only): the call sites on one launch, None: models/gpt2.py's."""
        dev = engine.device
        self.key, self.B, self.total, self._sites = key, B, total, _sites
        self.stage_ids = sorted(engine.stages)
        self.caches = {s: engine.stages[s].new_cache(B, total, fused=True) for s in self.stage_ids}
        self.tok = torch.zeros(B, dtype=torch.int64, device=dev)  # the token the next replay embeds
        self.out = torch.zeros((B, total), dtype=torch.int64, device=dev)
        self.done = torch.zeros(B, dtype=torch.int32, device=dev)
        self.gen_len = torch.zeros(B, dtype=torch.int32, device=dev)
        self.graph = None

    def step(self, engine, sampling: Sampling) -> None:
        x = self.tok
        for s in self.stage_ids:
            if self._sites is None:
                x = engine.stages[s].decode_step(x, self.caches[s], fused=True)
            else:
                x = engine.stages[s]._decode_step_fused(x, self.caches[s], _sites=self._sites)
        self.tok.copy_(sampling.step(x, self.caches[self.stage_ids[-1]].lens, self))

    def capture(self, engine, sampling: Sampling) -> None:
        """One eager step on the capture stream (every kernel of the step has run once before the capture; the state
        it touches is the empty caches' row 0 and the buffers, which every call initialises), then the capture."""
        stream = torch.cuda.Stream(device=engine.device)
        stream.wait_stream(torch.cuda.current_stream(engine.device))
        with torch.cuda.stream(stream):
            self.step(engine, sampling)
        torch.cuda.current_stream(engine.device).wait_stream(stream)
        self.reset()
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph, stream=stream):
            self.step(engine, sampling)
        engine.decode_graph_captures += 1

    def reset(self) -> None:
        """Empty caches (the prefill requires it), no token generated."""
        for c in self.caches.values():
            c.n = 0
            c.lens.zero_()
        self.done.zero_()
        self.gen_len.zero_()

    def replay(self) -> None:
        self.graph.replay()
        for c in self.caches.values():  # the host's bound follows the device-side lengths
            c.n = min(c.n + 1, c.smax)


def _param_addresses(engine):
    return tuple(p.untyped_storage().data_ptr() for s in sorted(engine.stages) for p in engine.stages[s].parameters())


@torch.no_grad()
def generate_graphed(engine, prompts, lens_host, new: int, sampling: Sampling, check: int):
    """generate()'s driver for ``graph=True`` on one rank holding every stage; the arguments are already checked.
    Returns (tokens, lengths, prompt lengths, steps)."""
    B, total = prompts.shape[0], prompts.shape[1] + new
    sp = replace(sampling, temperature=float(sampling.temperature), top_k=int(sampling.top_k),
                 top_p=float(sampling.top_p), sample0=int(sampling.sample0))
    key = (B, total) + astuple(sp)[1:] + (_param_addresses(engine),)
    stage_ids = sorted(engine.stages)
    with eval_stages([engine.stages[s] for s in stage_ids]):
        ses = engine.decode_session
        if ses is None or ses.key != key:
            engine.decode_session = None  # (the old session's memory goes before the new one's is taken)
            del ses
            ses = DecodeSession(engine, key, B, total)
            ses.capture(engine, sp)
            engine.decode_session = ses
        ses.reset()
        st = TokenState(prompts, lens_host, total, sp.pad, engine.device, storage=(ses.out, ses.done, ses.gen_len))
        # the prompt and the first token: eager, into the session's caches and buffers
        x = st.prompts
        for s in stage_ids:
            x = engine.stages[s].prefill(x, ses.caches[s], lens=st.lens_dev)
        ses.tok.copy_(sp.step(x, ses.caches[stage_ids[-1]].lens, ses))
        for t in range(1, new):  # token index S0 + t (ragged: lens[b] + t); decode_loop's check after token t - 1
            if check and t % check == 0 and bool(ses.done.min().item()):
                break
            ses.replay()
        return ses.out.clone(), st.lengths(), st.lens0, 0  # (no step count: stats are refused with a graph)
