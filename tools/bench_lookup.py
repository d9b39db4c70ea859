"""Prompt-lookup speculation on one MI355X: what a verify step costs and what generate(lookup=K) gains.

    python tools/bench_lookup.py [--rounds 3] [--out profiles/lookup_generate.jsonl]

Three parts, each alternated over --rounds rounds in one process, every round written out (one JSON line each):
  (i)   attention_append at T = 1, 2, 4, 8 against T calls of attention_decode (the cache length advancing between
        them), B = 8, 12 heads, ctx 128 / 512 / 1024: one device-event window around --reps rounds of calls, every
        round of calls on another copy of the cache, the copies totalling more than the last-level cache
        (tools/bench_generate.py's method).
  (ii)  one verify step of GPT-2 small (decode_block over T positions per row, the sampler over all B * T rows,
        lookup_step) against one plain step (decode_step, sample_logits), from caches holding --ctx keys: B = 8 at
        T = 1, 4, 8 and B = 16 at T = 4. c(T) = verify / plain is the number of tokens per step at which speculation
        breaks even.
  (iii) tokens/s end to end, generate(lookup=3, stop_check=4) against the plain eager loop, on the d = 64 GPT-2 of the
        tests trained here on the synthetic rule (period 6): 8 rule-following prompts of 8 tokens, 56 new tokens, greedy.
        The tokens must be equal. The gate, in every round: lookup tokens/s >= plain tokens/s (exit status 1 if not).
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from simple_distributed_machine_learning_amd import _native  # noqa: E402
from simple_distributed_machine_learning_amd.data import SyntheticTokens  # noqa: E402
from simple_distributed_machine_learning_amd.models import get_model_spec  # noqa: E402
from simple_distributed_machine_learning_amd.models.gpt2 import GPT2Config, gpt2_spec  # noqa: E402
from simple_distributed_machine_learning_amd.ops.decode import lookup_step, sample_logits, sample_step  # noqa: E402
from simple_distributed_machine_learning_amd.parallel import PipelineEngine, init_mesh  # noqa: E402
from simple_distributed_machine_learning_amd.parallel.generate import generate  # noqa: E402

DEV = torch.device("cuda", 0)
BF = torch.bfloat16
LLC_BYTES = 320 << 20
RULE_A, RULE_B, VOCAB = 48271 % 97, 12345 % 97, 97


def window(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(reps):
        fn(i)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


# ---- (i) ------------------------------------------------------------------------------------------------------------
def bench_attention(rounds, reps, emit):
    K = _native.kernels()
    B, H, D = 8, 12, 64
    for ctx in (128, 512, 1024):
        Smax = ctx + 8
        copies = max(2, min(reps, LLC_BYTES // (B * Smax * H * D * 2 * 2) + 1))
        kc = torch.randn(copies, B, Smax, H, D, device=DEV, dtype=BF)
        vc = torch.randn(copies, B, Smax, H, D, device=DEV, dtype=BF)
        for T in (1, 2, 4, 8):
            qkv = torch.randn(B, T, 3 * H * D, device=DEV, dtype=BF)
            lens = [torch.full((B,), ctx + t, dtype=torch.int32, device=DEV) for t in range(T)]
            nq = torch.full((B,), T, dtype=torch.int32, device=DEV)

            def seq(i):
                for t in range(T):
                    K.attention_decode(qkv[:, t], kc[i % copies], vc[i % copies], lens[t], 0.125, ctx + T)

            fns = {"attention_append": lambda i: K.attention_append(qkv, kc[i % copies], vc[i % copies], lens[0], nq,
                                                                    0.125, ctx + T),
                   "T x attention_decode": seq}
            for fn in fns.values():
                window(fn, copies)
            us = {k: [] for k in fns}
            for r in range(rounds):
                for name, fn in fns.items():  # alternated
                    ms = window(fn, reps)
                    us[name].append(round(ms * 1e3, 2))
                    emit({"part": "i", "kernel": name, "B": B, "H": H, "ctx": ctx, "T": T, "round": r,
                          "us": round(ms * 1e3, 2)})
            emit({"part": "i", "summary": "attention", "B": B, "ctx": ctx, "T": T, "append_us": us["attention_append"],
                  "sequential_us": us["T x attention_decode"],
                  "append_over_sequential": round(statistics.median(us["attention_append"]) /
                                                  statistics.median(us["T x attention_decode"]), 3)})
        del kc, vc


# ---- (ii) -----------------------------------------------------------------------------------------------------------
@torch.no_grad()
def run_steps(engine, B, T, ctx, steps):
    """Seconds per step: T = 0 the plain step (decode_step + sample_logits), else the verify step at T positions per
    row (decode_block + sample_step over B * T rows + lookup_step), from caches holding ctx keys."""
    stages = [engine.stages[s] for s in range(engine.P)]
    V = stages[0].cfg.vocab_size
    room = min(steps * max(T, 1) + 8, stages[0].cfg.block_size - ctx)  # (a row that fills up just stops advancing)
    caches = [st.new_cache(B, ctx + room) for st in stages]
    for c in caches:
        for t in c.k + c.v:
            t.normal_()
        c.lens.fill_(ctx)
        c.n = ctx
    if T:
        for c in caches[1:]:
            c.lens = caches[0].lens
    lens = caches[-1].lens
    W = ctx + room
    out = torch.randint(0, V, (B, W), device=DEV)
    limit = torch.full((B,), W, dtype=torch.int32, device=DEV)
    done, gen_len, row_steps = (torch.zeros(B, dtype=torch.int32, device=DEV) for _ in range(3))
    tok = torch.randint(0, V, (B, max(T, 1)), device=DEV)
    nq = torch.full((B,), T, dtype=torch.int32, device=DEV)
    offs = torch.arange(1, T + 1, dtype=torch.int32, device=DEV)[None, :]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        if T == 0:
            x = tok[:, 0]
            for st, c in zip(stages, caches):
                x = st.decode_step(x, c)
            tok = sample_logits(x, V, 0.0, 0, 0, 0, lens)[:, None]
        else:
            x = tok
            for st, c in zip(stages, caches):
                x = st.decode_block(x, c, nq)
            g = sample_step(x, V, 0.0, 0, 1.0, 0, 0, (lens[:, None] + offs).reshape(B * T), rows_per_sample=T)
            if T > 1:
                nxt, nq2, _ = lookup_step(g.view(B, T), tok, nq, out, lens, limit, done, gen_len, row_steps, T - 1, 2)
            tok = g.view(B, T)  # (every position stays live: the cost of a full step, whatever was accepted)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps


def bench_step(engine, ctx, steps, rounds, emit):
    for B, Ts in ((8, (1, 4, 8)), (16, (4,))):
        forms = (0,) + Ts
        for T in forms:
            run_steps(engine, B, T, ctx, 4)
        ms = {T: [] for T in forms}
        for r in range(rounds):
            for T in forms:  # alternated
                s = run_steps(engine, B, T, ctx, steps)
                ms[T].append(round(s * 1e3, 4))
                emit({"part": "ii", "step": "decode_step" if T == 0 else f"verify T={T}", "B": B, "ctx": ctx,
                      "round": r, "ms_per_step": round(s * 1e3, 4)})
        for T in Ts:
            emit({"part": "ii", "summary": "verify step", "B": B, "T": T, "ctx": ctx, "verify_ms": ms[T],
                  "decode_step_ms": ms[0],
                  "c_T_break_even_tokens_per_step": round(statistics.median(ms[T]) / statistics.median(ms[0]), 3)})


# ---- (iii) ----------------------------------------------------------------------------------------------------------
def trained_d64():
    cfg = GPT2Config(n_layer=2, n_head=2, n_embd=128, vocab_size=VOCAB, block_size=64)
    spec = gpt2_spec(2, cfg=cfg, seq_len=32, dtype=BF, name="gpt2_d64")
    mesh = init_mesh(pp=1, schedule_kind="1f1b", rank=0, world_size=1, device=DEV)
    eng = PipelineEngine(spec, mesh, schedule_kind="1f1b", num_microbatches=1, lr=3e-3, seed=1, optimizer="adamw")
    ds = SyntheticTokens(200 * 16, 32, VOCAB, seed=1234, device=DEV)
    eng.train()
    for i in range(200):
        eng.run(ds, i * 16, 16, train=True)
    eng.eval()
    return eng


def bench_end_to_end(rounds, calls, emit):
    eng = trained_d64()
    rows = []
    for t in (1, 2, 5, 17, 40, 63, 77, 96):
        row = [t]
        while len(row) < 8:
            row.append((row[-1] * RULE_A + RULE_B) % VOCAB)
        rows.append(row)
    prompts = torch.tensor(rows, dtype=torch.int64)
    B, new = len(rows), 56
    forms = {"plain": dict(), "lookup=3": dict(lookup=3, stop_check=4)}
    want = generate(eng, prompts, new)
    got, stats = generate(eng, prompts, new, return_stats=True, **forms["lookup=3"])
    equal = bool(torch.equal(got, want))
    seq = want.cpu()
    follows = float((seq[:, 1:] == (seq[:, :-1] * RULE_A + RULE_B) % VOCAB).float().mean())
    emit({"part": "iii", "check": "tokens equal", "equal": equal, "rule_followed": round(follows, 4),
          "steps": stats["steps"], "row_steps": stats["row_steps"].tolist()})
    tps = {k: [] for k in forms}
    for r in range(rounds):
        for name, kw in forms.items():  # alternated
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(calls):
                generate(eng, prompts, new, **kw).cpu()
            s = (time.perf_counter() - t0) / calls
            tps[name].append(round(B * new / s, 1))
            emit({"part": "iii", "loop": name, "B": B, "prompt": 8, "new": new, "round": r,
                  "ms_per_call": round(s * 1e3, 3), "tokens_per_s": round(B * new / s, 1)})
    ok = equal and all(a >= b for a, b in zip(tps["lookup=3"], tps["plain"]))
    emit({"part": "iii", "summary": "end to end", "lookup_tokens_per_s": tps["lookup=3"],
          "plain_tokens_per_s": tps["plain"],
          "lookup_over_plain": round(statistics.median(tps["lookup=3"]) / statistics.median(tps["plain"]), 3),
          "gate_lookup_at_least_plain_every_round": bool(ok)})
    return ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=200, help="calls per kernel timing window of (i)")
    ap.add_argument("--steps", type=int, default=64, help="steps per timing of (ii)")
    ap.add_argument("--ctx", type=int, default=512, help="cached keys of (ii)")
    ap.add_argument("--calls", type=int, default=5, help="generate calls per timing of (iii)")
    ap.add_argument("--parts", default="i,ii,iii")
    ap.add_argument("--out", default="profiles/lookup_generate.jsonl")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_lookup.py measures on the GPU; none is visible")
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
            bench_attention(a.rounds, a.reps, emit)
        if "ii" in parts:
            mesh = init_mesh(pp=1, schedule_kind="1f1b", rank=0, world_size=1, device=DEV)
            engine = PipelineEngine(get_model_spec("gpt2", 2), mesh, schedule_kind="1f1b", num_microbatches=1)
            engine.eval()
            bench_step(engine, a.ctx, a.steps, a.rounds, emit)
            del engine
            torch.cuda.empty_cache()
        if "iii" in parts:
            ok = bench_end_to_end(a.rounds, a.calls, emit)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
