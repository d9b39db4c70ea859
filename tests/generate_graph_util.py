"""Shared pieces of the graph-replayed generation tests (module-level so spawn can import the rank body)."""
from __future__ import annotations

import torch

from generate_util import VOCAB, make_engine


def refused_worker(rank, world, model, device, dtype):
    """One rank of a pp = world pipeline asking for graph=True: the refusal's message (None: it was not refused). The
    refusal comes before any message is sent, so the ranks need not agree on anything."""
    from simple_distributed_machine_learning_amd.parallel.generate import generate

    eng = make_engine(model, device, dtype, rank, world, pp=world, kind="gpipe", backend="gloo")
    try:
        generate(eng, torch.arange(VOCAB)[:, None], 4, graph=True)
    except ValueError as e:
        return str(e)
    return None
