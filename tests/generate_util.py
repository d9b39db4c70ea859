"""Shared pieces of the generation tests: engines, the synthetic data's rule, the no-cache reference loop and the rank
body of the multi-process runs (module-level so spawn can import it)."""
from __future__ import annotations

import torch

RULE_A, RULE_B, VOCAB = 48271 % 97, 12345 % 97, 97


def rule_holds(tokens, first: int = 0):
    """[B, S - 1 - first] bool: transition t -> t + 1 obeys t' = (a t + b) mod 97, from position ``first`` on."""
    t = tokens.cpu()
    return (t[:, first + 1:] == (t[:, first:-1] * RULE_A + RULE_B) % VOCAB)


def spec_of(model: str, dtype):
    """"gpt2_tiny" (d = 16 heads: the torch twins everywhere) or "gpt2_d64" (the dropout tests' d = 64 config: the
    kernels on ROCm bf16)."""
    from simple_distributed_machine_learning_amd.models import get_model_spec
    from simple_distributed_machine_learning_amd.models.gpt2 import GPT2Config, gpt2_spec

    if model == "gpt2_tiny":
        return get_model_spec("gpt2_tiny", 2, dtype=dtype)
    cfg = GPT2Config(n_layer=2, n_head=2, n_embd=128, vocab_size=VOCAB, block_size=64)
    return gpt2_spec(2, cfg=cfg, seq_len=32, dtype=dtype, name="gpt2_d64")


def make_engine(model, device, dtype, rank=0, world=1, pp=1, kind="1f1b", transport=None, backend=None, seed=1,
                lr=3e-3):
    from simple_distributed_machine_learning_amd.parallel import PipelineEngine, init_mesh

    mesh = init_mesh(pp=pp, schedule_kind=kind, rank=rank, world_size=world, device=torch.device(device),
                     backend=backend, timeout_s=120, transport=transport)
    return PipelineEngine(spec_of(model, dtype), mesh, schedule_kind=kind, num_microbatches=1, lr=lr, seed=seed,
                          optimizer="adamw")


def train_steps(engine, steps: int, batch: int, seq_len: int):
    from simple_distributed_machine_learning_amd.data import SyntheticTokens

    ds = SyntheticTokens(steps * batch, seq_len, VOCAB, seed=1234, device=engine.device)
    engine.train()
    for i in range(steps):
        engine.run(ds, i * batch, batch, train=True)
    engine.eval()
    return engine


@torch.no_grad()
def nocache_logits(engine, tokens):
    """The training-path forward (eval mode) of a one-process engine: logits [B, S, V]."""
    x = tokens
    for s in range(engine.P):
        x = engine.stages[s](x)
    return x


@torch.no_grad()
def nocache_greedy(engine, prompts, new: int):
    """Greedy decoding by re-running the full forward on the growing prefix."""
    seq = prompts.to(engine.device)
    for _ in range(new):
        nxt = nocache_logits(engine, seq)[:, -1].float().argmax(-1, keepdim=True)
        seq = torch.cat([seq, nxt], 1)
    return seq


def generate_worker(rank, world, model, device, dtype, ckpt_dir, transport, new, sampled):
    """One rank of a pp = world pipeline: load the checkpoint, generate greedily (and sampled) from the 97 one-token
    prompts."""
    from simple_distributed_machine_learning_amd.parallel.generate import generate
    from simple_distributed_machine_learning_amd.utils.checkpoint import load_checkpoint

    eng = make_engine(model, device, dtype, rank, world, pp=world, kind="gpipe", transport=transport, backend="gloo")
    load_checkpoint(eng, ckpt_dir)
    prompts = torch.arange(VOCAB)[:, None]
    out = {"greedy": generate(eng, prompts, new).cpu(), "stages": sorted(eng.stages),
           "bytes_sent": eng.transport.bytes_sent if eng.transport else 0}
    if sampled:
        out["sampled"] = generate(eng, prompts, new, temperature=0.9, top_k=20, seed=5).cpu()
    return out
