"""Extend attention and generation sessions on one MI355X: what the kernel costs per layer and what a kept cache gains.

    python tools/bench_extend.py [--rounds 3] [--out profiles/extend_attention.jsonl]

Two parts, each alternated over --rounds rounds in one process, every round written out (one JSON line each):
  (i)  per layer, B = 16, 12 heads of width 64: the prefill lines of models/gpt2.py (causal_attention over S = 1024 plus
       the two strided copies into the cache) against attention_extend at (L 0, T 1024), and attention_extend alone at
       (L 896, T 128) and (L 512, T 32). One device-event window around --reps calls, every call on another copy of
       the cache, the copies totalling more than the last-level cache (tools/bench_generate.py's method). Reported,
       not gated: the default prefill keeps its path.
  (ii) GPT-2 small, B = 16: a session holding 512 tokens per row (511 cached, the newest unprocessed) takes 32 appended
       tokens and generates 32 more, against a fresh generate() on the same 544-token rows for 32 new tokens. Greedy;
       the weights are the initial ones, the tokens are not compared. Timed from the append to the tokens on the
       host. The gate, in every round: the session is not slower than the fresh call (exit status 1 if it is).
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from simple_distributed_machine_learning_amd.models import get_model_spec  # noqa: E402
from simple_distributed_machine_learning_amd.ops.decode import attention_extend  # noqa: E402
from simple_distributed_machine_learning_amd.ops.transformer import causal_attention  # noqa: E402
from simple_distributed_machine_learning_amd.parallel import PipelineEngine, init_mesh  # noqa: E402
from simple_distributed_machine_learning_amd.parallel.generate import generate  # noqa: E402
from simple_distributed_machine_learning_amd.parallel.session import GenerationSession  # noqa: E402

DEV = torch.device("cuda", 0)
BF = torch.bfloat16
LLC_BYTES = 320 << 20


def window(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(reps):
        fn(i)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


# ---- (i) ------------------------------------------------------------------------------------------------------------
@torch.no_grad()
def bench_layer(rounds, reps, emit):
    B, H, D, S = 16, 12, 64, 1024
    C = H * D
    copies = LLC_BYTES // (B * S * C * 2 * 2) + 2
    kc = torch.randn(copies, B, S, H, D, device=DEV, dtype=BF)
    vc = torch.randn(copies, B, S, H, D, device=DEV, dtype=BF)
    qkv = {T: torch.randn(copies, B, T, 3 * C, device=DEV, dtype=BF) for T in (1024, 128, 32)}

    def prefill_lines(i):
        x, k, v = qkv[S][i % copies], kc[i % copies], vc[i % copies]
        k.copy_(x[..., C:2 * C].view(B, S, H, D))
        v.copy_(x[..., 2 * C:].view(B, S, H, D))
        causal_attention(x, H)

    def extend(L, T):
        lens = torch.full((B,), L, dtype=torch.int32, device=DEV)
        nq = torch.full((B,), T, dtype=torch.int32, device=DEV)
        return lambda i: attention_extend(qkv[T][i % copies], kc[i % copies], vc[i % copies], lens, nq, H, L + T)

    fns = {"prefill lines S=1024 (attention_fwd + 2 copies)": prefill_lines,
           "attention_extend L=0 T=1024": extend(0, 1024),
           "attention_extend L=896 T=128": extend(896, 128),
           "attention_extend L=512 T=32": extend(512, 32)}
    for fn in fns.values():
        window(fn, copies)
    us = {k: [] for k in fns}
    for r in range(rounds):
        for name, fn in fns.items():  # alternated
            ms = window(fn, reps)
            us[name].append(round(ms * 1e3, 1))
            emit({"part": "i", "what": name, "B": B, "H": H, "round": r, "us": round(ms * 1e3, 1)})
    names = list(fns)
    emit({"part": "i", "summary": "per layer", "B": B, "H": H, **{n: us[n] for n in names},
          "extend_over_prefill_lines": round(statistics.median(us[names[1]]) / statistics.median(us[names[0]]), 3)})


# ---- (ii) -----------------------------------------------------------------------------------------------------------
def bench_session(rounds, emit):
    mesh = init_mesh(pp=1, schedule_kind="1f1b", rank=0, world_size=1, device=DEV)
    engine = PipelineEngine(get_model_spec("gpt2", 2), mesh, schedule_kind="1f1b", num_microbatches=1)
    engine.eval()
    B, held, add, new = 16, 512, 32, 32
    V = engine.stages[0].cfg.vocab_size
    g = torch.Generator().manual_seed(0)
    prompts = torch.randint(0, V, (B, held - 1), generator=g)
    more = torch.randint(0, V, (B, add), generator=g)

    def session_call():
        s = GenerationSession(engine, prompts, held + add + new)
        s.generate(1)  # 512 tokens per row, 511 of them cached (not timed)
        rows = torch.cat([s.out[:, :held].cpu(), more], 1)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        s.append(more)
        out, _ = s.generate(new)
        out = out.cpu()
        dt = time.perf_counter() - t0
        s.close()
        return dt, rows, out

    def fresh_call(rows):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = generate(engine, rows, new).cpu()
        return time.perf_counter() - t0, out

    _, rows, _ = session_call()  # warm-up of both forms
    fresh_call(rows)
    ms = {"session": [], "fresh": []}
    for r in range(rounds):  # alternated
        dt, rows, _ = session_call()
        ms["session"].append(round(dt * 1e3, 2))
        emit({"part": "ii", "form": "session: append 32, generate 32 on 511 cached", "B": B, "round": r,
              "ms": round(dt * 1e3, 2)})
        dt, _ = fresh_call(rows)
        ms["fresh"].append(round(dt * 1e3, 2))
        emit({"part": "ii", "form": "fresh generate() on 544-token rows, 32 new", "B": B, "round": r,
              "ms": round(dt * 1e3, 2)})
    ok = all(a <= b for a, b in zip(ms["session"], ms["fresh"]))
    emit({"part": "ii", "summary": "session against a fresh call", "session_ms": ms["session"], "fresh_ms": ms["fresh"],
          "session_over_fresh": round(statistics.median(ms["session"]) / statistics.median(ms["fresh"]), 3),
          "gate_session_not_slower_in_any_round": bool(ok)})
    return ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=50, help="calls per kernel timing window of (i)")
    ap.add_argument("--parts", default="i,ii")
    ap.add_argument("--out", default="profiles/extend_attention.jsonl")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_extend.py measures on the GPU; none is visible")
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    parts = set(a.parts.split(","))
    ok = True
    with open(a.out, "w") as f:
        def emit(rec):
            line = json.dumps(rec)
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()

        if "i" in parts:
            bench_layer(a.rounds, a.reps, emit)
            torch.cuda.empty_cache()
        if "ii" in parts:
            ok = bench_session(a.rounds, emit)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
