"""Several samples per prompt on one MI355X: what attention_fork costs against duplicated caches, and what
generate(num_samples=n) gains over the call on the n-fold repeated prompts.

    python tools/bench_fork.py [--rounds 3] [--out profiles/fork_attention.jsonl]

Two parts, each alternated over --rounds rounds in one process, every round written out (one JSON line each):
  (i)  per layer: attention_fork over G = 8 groups of n = 1, 2, 4, 8 siblings (12 heads, prompts of 128 / 512 / 960
       keys, 32 suffix keys per row) against attention_decode over the G n rows of a cache that holds every prompt n
       times. One device-event window around --reps back-to-back calls, every call on another copy of the caches, the
       copies totalling more than the last-level cache (tools/bench_generate.py's method).
  (ii) end to end, GPT-2 small (initial weights; the tokens are compared, not judged): B = 4 prompts of 512 tokens,
       n = 4, 32 new tokens, sampled. generate(num_samples=4) against generate on the repeated prompts: seconds per
       call (host clock, ending with the tokens on the host), torch.cuda.max_memory_allocated of each, and the KV-cache
       bytes of both forms from the formula B n (S0 + new) rows against B S0 + B n new. The tokens must be equal. The
       gate, in every round: the forked call is not slower (exit status 1 if it is).
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
from simple_distributed_machine_learning_amd.models import get_model_spec  # noqa: E402
from simple_distributed_machine_learning_amd.parallel import PipelineEngine, init_mesh  # noqa: E402
from simple_distributed_machine_learning_amd.parallel.generate import generate  # noqa: E402

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
def bench_attention(rounds, reps, emit):
    K = _native.kernels()
    G, H, D, suffix, room = 8, 12, 64, 32, 40
    row = H * D * 2 * 2  # bytes of one key's k and v
    for prompt in (128, 512, 960):
        for n in (1, 2, 4, 8):
            R = G * n
            cf = max(2, min(reps, LLC_BYTES // ((G * prompt + R * room) * row) + 1))
            cd = max(2, min(reps, LLC_BYTES // (R * (prompt + room) * row) + 1))
            kp, vp = (torch.randn(cf, G, prompt, H, D, device=DEV, dtype=BF) for _ in range(2))
            ks, vs = (torch.randn(cf, R, room, H, D, device=DEV, dtype=BF) for _ in range(2))
            kd, vd = (torch.randn(cd, R, prompt + room, H, D, device=DEV, dtype=BF) for _ in range(2))
            qkv = torch.randn(R, 3 * H * D, device=DEV, dtype=BF)
            plens = torch.full((G,), prompt, dtype=torch.int32, device=DEV)
            lens = torch.full((R,), prompt + suffix, dtype=torch.int32, device=DEV)
            nk = prompt + suffix + 1
            fns = {"attention_fork": lambda i: K.attention_fork(qkv, kp[i % cf], vp[i % cf], plens, ks[i % cf],
                                                                vs[i % cf], lens, n, 0.125, nk),
                   "attention_decode, duplicated": lambda i: K.attention_decode(qkv, kd[i % cd], vd[i % cd], lens,
                                                                                0.125, nk)}
            for fn in fns.values():
                window(fn, max(cf, cd))
            us = {k: [] for k in fns}
            for r in range(rounds):
                for name, fn in fns.items():  # alternated
                    ms = window(fn, reps)
                    us[name].append(round(ms * 1e3, 2))
                    emit({"part": "i", "kernel": name, "G": G, "H": H, "n": n, "prompt": prompt, "suffix": suffix,
                          "round": r, "us": round(ms * 1e3, 2)})
            emit({"part": "i", "summary": "attention", "G": G, "n": n, "prompt": prompt, "suffix": suffix,
                  "fork_us": us["attention_fork"], "duplicated_us": us["attention_decode, duplicated"],
                  "fork_over_duplicated": round(statistics.median(us["attention_fork"]) /
                                                statistics.median(us["attention_decode, duplicated"]), 3),
                  "kv_bytes_fork": (G * prompt + R * (suffix + 1)) * row,
                  "kv_bytes_duplicated": R * (prompt + suffix + 1) * row})
            del kp, vp, ks, vs, kd, vd
            torch.cuda.empty_cache()


# ---- (ii) -----------------------------------------------------------------------------------------------------------
def bench_end_to_end(rounds, calls, emit):
    mesh = init_mesh(pp=1, schedule_kind="1f1b", rank=0, world_size=1, device=DEV)
    eng = PipelineEngine(get_model_spec("gpt2", 2), mesh, schedule_kind="1f1b", num_microbatches=1)
    eng.eval()
    cfg = eng.stages[0].cfg
    B, n, S0, new = 4, 4, 512, 32
    g = torch.Generator().manual_seed(3)
    prompts = torch.randint(0, cfg.vocab_size, (B, S0), generator=g)
    kw = dict(temperature=1.0, top_k=50, seed=7)
    forms = {"repeated": lambda: generate(eng, prompts.repeat_interleave(n, 0), new, **kw),
             "num_samples": lambda: generate(eng, prompts, new, num_samples=n, **kw)}
    want, got = forms["repeated"]().cpu(), forms["num_samples"]().cpu()
    equal = bool(torch.equal(got, want))
    groups = want.view(B, n, -1)
    differ = sum(int(not torch.equal(groups[b, 0], groups[b, j])) for b in range(B) for j in range(1, n))
    per_key = cfg.n_layer * 2 * cfg.n_embd * 2  # bytes of one position's k and v over all layers
    emit({"part": "ii", "check": "tokens equal", "equal": equal, "siblings_that_differ_from_sibling_0": differ,
          "of": B * (n - 1), "kv_cache_bytes_repeated": B * n * (S0 + new) * per_key,
          "kv_cache_bytes_num_samples": (B * S0 + B * n * new) * per_key,
          "formula": "B n (S0 + new) rows against B S0 + B n new"})
    ms, peak = {k: [] for k in forms}, {k: [] for k in forms}
    for r in range(rounds):
        for name, fn in forms.items():  # alternated
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            t0 = time.perf_counter()
            for _ in range(calls):
                fn().cpu()
            s = (time.perf_counter() - t0) / calls
            ms[name].append(round(s * 1e3, 3))
            peak[name].append(torch.cuda.max_memory_allocated())
            emit({"part": "ii", "form": name, "B": B, "n": n, "prompt": S0, "new": new, "round": r,
                  "ms_per_call": round(s * 1e3, 3), "max_memory_allocated": peak[name][-1],
                  "above_the_model": peak[name][-1] - base})
    ok = equal and all(a <= b for a, b in zip(ms["num_samples"], ms["repeated"]))
    emit({"part": "ii", "summary": "end to end", "num_samples_ms": ms["num_samples"], "repeated_ms": ms["repeated"],
          "num_samples_over_repeated": round(statistics.median(ms["num_samples"]) / statistics.median(ms["repeated"]), 3),
          "max_memory_allocated_num_samples": peak["num_samples"], "max_memory_allocated_repeated": peak["repeated"],
          "gate_num_samples_not_slower_in_any_round": bool(ok)})
    return ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=200, help="calls per kernel timing window of (i)")
    ap.add_argument("--calls", type=int, default=3, help="generate calls per timing of (ii)")
    ap.add_argument("--parts", default="i,ii")
    ap.add_argument("--out", default="profiles/fork_attention.jsonl")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_fork.py measures on the GPU; none is visible")
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
            ok = bench_end_to_end(a.rounds, a.calls, emit)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
