"""GPT-2 small generation on one MI355X: the decode kernels next to the library calls for the same work, and the
whole decode loop, hand-written against library-substituted, alternated in one process over --rounds rounds.

    python tools/bench_generate.py [--B 16] [--ctx 512] [--rounds 3] [--sweep]
        [--out_kernels profiles/generate_kernels.jsonl] [--out_loop profiles/generate_gpt2.jsonl]
    python tools/bench_generate.py --ragged [--out_ragged profiles/ragged_generate.jsonl]
    python tools/bench_generate.py --graph [--sweep] [--out_graph profiles/generate_graph.jsonl]

Per kernel (one JSON line per kernel, shape and round): the time of one call, taken as a device-event window around
--reps back-to-back calls, and the achieved GB/s of the bytes that must move: W for the projections (x and y are
below 1 % of it), K + V for the attention. Every call of a window reads another copy of its operand, the copies
totalling more than the 256 MB last-level cache, as a decode step streams each layer's weights and cache once. A
window is the larger of the device time and the host's enqueue time of its calls: at these sizes (microseconds) the
small shapes sit on the enqueue floor, and the kernels' own durations come from a `rocprofv3 --kernel-trace --stats`
run of this tool (README "Generation").
  * linear_decode / torch.addmm / gemm_bf16 at M = B rows, the four GPT-2 shapes and the lm_head
  * attention_decode / F.scaled_dot_product_attention with a one-row query over the cached keys
Decode loop: --steps steps of the 12-layer model (2 stages in one process) from a cache already holding ctx keys,
greedy sampling on the device, tokens/s = B * steps / seconds (host clock around a device synchronise). "lib" is the
same loop with torch.addmm, index_put + scaled_dot_product_attention, F.embedding and argmax in place of the four
hand kernels (the LayerNorm kernels are the same in both). The gate: hand >= lib at --B 16 --ctx 512.
--sweep adds B in {1, 16, 64} x ctx in {128, 1024}.

--ragged measures only the step sampler (sample_step: top-p and the step's bookkeeping) and writes --out_ragged:
  * the sampler window, --reps back-to-back calls on logits [B, 50257] (ld 50304) at T = 0.8, alternated over --rounds:
    sample_step at top_p = 0.9 with top_k 0 and 50, against (a) sample_logits (top_p off) and (b) top-p in torch (sort,
    softmax, cumsum, Gumbel-max) on the same logits. The gate: sample_step is not slower than (b); the cost over (a) is
    reported only.
  * one decode-loop row: the loop with ragged cache lengths and sample_step doing the bookkeeping (token matrix, done
    flags, lengths, an eos set) against today's loop (sample_logits and the column store out[:, t] = tok).

--graph measures the graph-replayed decode step (parallel/decode_graph.py) and writes --out_graph:
  * per-kernel windows, one-launch (tickets) against two-launch, alternated over --rounds: the four projections at
    M = B and attention_decode at ctx 128 / 512 / 1024;
  * the decode loop in three forms, alternated over --rounds: (a) today's eager loop, (b) the captured step with the
    two-launch kernels, (c) the captured step as decode_step(fused=True) runs it; then (c) with each call site
    flipped (a one-launch site put back on two launches, a two-launch site put on one). The gate: (c) >= (a) in tokens/s in every round at --B 16 --ctx 512. --sweep adds the B x ctx grid.
--graph --replays N only captures form (c) and replays it N times: the run to put under `rocprofv3 --kernel-trace
--stats`, where a kernel's calls / (N + 1) are its launches per step (one eager step precedes the capture).
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from simple_distributed_machine_learning_amd import _native  # noqa: E402
from simple_distributed_machine_learning_amd.models import get_model_spec  # noqa: E402
from simple_distributed_machine_learning_amd.models.gpt2 import DECODE_FUSED_SITES, DECODE_SITES  # noqa: E402
from simple_distributed_machine_learning_amd.ops.decode import sample_logits, sample_step  # noqa: E402
from simple_distributed_machine_learning_amd.ops.transformer import add_layer_norm, layer_norm_pass  # noqa: E402
from simple_distributed_machine_learning_amd.parallel import PipelineEngine, init_mesh  # noqa: E402
from simple_distributed_machine_learning_amd.parallel.decode_graph import DecodeSession  # noqa: E402
from simple_distributed_machine_learning_amd.parallel.gen_common import Sampling  # noqa: E402

DEV = torch.device("cuda", 0)
BF = torch.bfloat16
LLC_BYTES = 320 << 20  # operand copies per window: beyond the 256 MB last-level cache
SHAPES = {"c_attn": (2304, 768), "attn_proj": (768, 768), "c_fc": (3072, 768), "mlp_proj": (768, 3072),
          "lm_head": (50304, 768)}


def window(fn, reps):
    """ms per call of fn(i), i = 0 .. reps - 1, from one device-event window."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(reps):
        fn(i)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def bench_kernels(B, ctxs, rounds, reps, emit):
    K = _native.kernels()
    for name, (N, Kd) in SHAPES.items():
        copies = max(2, min(reps, LLC_BYTES // (N * Kd * 2) + 1))
        w = torch.randn(copies, N, Kd, device=DEV, dtype=BF) * 0.02
        b = torch.randn(N, device=DEV, dtype=BF)
        x = torch.randn(B, Kd, device=DEV, dtype=BF)
        fns = {"linear_decode": lambda i: K.linear_decode(x, w[i % copies], b, 1),
               "torch.addmm": lambda i: torch.addmm(b, x, w[i % copies].t())}
        if name in ("c_attn", "c_fc"):
            fns["gemm_bf16"] = lambda i: K.gemm_bf16(x, w[i % copies], b, False, 1)
        for fn in fns.values():
            window(fn, copies)  # warm-up: every copy touched, code objects loaded, the library's algorithm picked
        for r in range(rounds):
            for kname, fn in fns.items():  # alternated
                ms = window(fn, reps)
                emit({"kernel": kname, "shape": name, "M": B, "N": N, "K": Kd, "round": r, "us": round(ms * 1e3, 2),
                      "GB_per_s": round(N * Kd * 2 / (ms * 1e-3) / 1e9, 1), "bytes": N * Kd * 2, "copies": copies})
        del w
    H, D = 12, 64
    for ctx in ctxs:
        Smax = ctx + 1
        per = B * Smax * H * D * 2 * 2
        copies = max(2, min(reps, LLC_BYTES // per + 1))
        kc = torch.randn(copies, B, Smax, H, D, device=DEV, dtype=BF)
        vc = torch.randn(copies, B, Smax, H, D, device=DEV, dtype=BF)
        qkv = torch.randn(B, 3 * H * D, device=DEV, dtype=BF)
        lens = torch.full((B,), ctx, dtype=torch.int32, device=DEV)
        q4 = qkv[:, :H * D].view(B, H, 1, D)

        def lib(i):
            k, v = kc[i % copies].transpose(1, 2), vc[i % copies].transpose(1, 2)
            return F.scaled_dot_product_attention(q4, k, v)

        fns = {"attention_decode": lambda i: K.attention_decode(qkv, kc[i % copies], vc[i % copies], lens, 0.125, Smax),
               "F.scaled_dot_product_attention": lib}
        for fn in fns.values():
            window(fn, copies)
        nbytes = B * (ctx + 1) * H * D * 2 * 2
        for r in range(rounds):
            for kname, fn in fns.items():
                ms = window(fn, reps)
                emit({"kernel": kname, "B": B, "H": H, "ctx": ctx, "round": r, "us": round(ms * 1e3, 2),
                      "GB_per_s": round(nbytes / (ms * 1e-3) / 1e9, 1), "bytes": nbytes, "copies": copies})
        del kc, vc


# ---- the decode loop ---------------------------------------------------------------------------------------------
def lib_decode_step(stage, x, cache):
    """models/gpt2.py decode_step with library calls in place of the hand kernels."""
    cfg = stage.cfg
    H, C = cfg.n_head, cfg.n_embd
    B = x.shape[0]
    rows = torch.arange(B, device=x.device)
    if stage.stage_id == 0:
        x = F.embedding(x, stage.wte.weight) + F.embedding(cache.lens.long(), stage.wpe.weight)
    last = stage.stage_id == stage.num_stages - 1
    blocks = list(stage.h.values())
    n = cache.n + 1
    x, y = layer_norm_pass(x, blocks[0].ln_1)
    for i, blk in enumerate(blocks):
        at, mlp = blk.attn, blk.mlp
        qkv = torch.addmm(at.c_attn.bias, y, at.c_attn.weight.t())
        q, k, v = (qkv[:, j * C:(j + 1) * C].view(B, H, C // H) for j in range(3))
        idx = cache.lens.long()
        cache.k[i][rows, idx] = k
        cache.v[i][rows, idx] = v
        a = F.scaled_dot_product_attention(q[:, :, None], cache.k[i][:, :n].transpose(1, 2),
                                           cache.v[i][:, :n].transpose(1, 2)).reshape(B, C)
        a = torch.addmm(at.c_proj.bias, a, at.c_proj.weight.t())
        x, y = add_layer_norm(x, a, blk.ln_2)
        hdn = F.gelu(torch.addmm(mlp.c_fc.bias, y, mlp.c_fc.weight.t()), approximate="tanh")
        m = torch.addmm(mlp.c_proj.bias, hdn, mlp.c_proj.weight.t())
        nxt = blocks[i + 1].ln_1 if i + 1 < len(blocks) else (stage.ln_f if last else None)
        if nxt is None:
            x = x + m
        else:
            x, y = add_layer_norm(x, m, nxt)
    cache.lens.add_(1)
    cache.n += 1
    return y @ stage.lm_head.weight.t() if last else x


@torch.no_grad()
def run_loop(engine, B, ctx, steps, hand):
    """Seconds of `steps` decode steps from caches holding ctx keys (random contents; greedy sampling); where ctx +
    steps would pass block_size the loop starts at block_size - steps keys and ends at block_size."""
    stages = [engine.stages[s] for s in range(engine.P)]
    ctx = min(ctx, stages[0].cfg.block_size - steps)
    caches = [st.new_cache(B, ctx + steps) for st in stages]
    for c in caches:
        for t in c.k + c.v:
            t.normal_()
        c.lens.fill_(ctx)
        c.n = ctx
    V = stages[0].cfg.vocab_size
    tok = torch.randint(0, V, (B,), device=DEV)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        x = tok
        for st, c in zip(stages, caches):
            x = st.decode_step(x, c) if hand else lib_decode_step(st, x, c)
        tok = sample_logits(x, V, 0.0, 0, 0, 0, caches[-1].lens) if hand else x[:, :V].argmax(-1)
    torch.cuda.synchronize()
    return time.perf_counter() - t0


# ---- the step sampler (--ragged) -----------------------------------------------------------------------------------
def torch_top_p(z, V, T, top_k, top_p):
    """Top-p sampling in library calls: sort, softmax, cumsum, Gumbel-max over the kept prefix."""
    l = z[:, :V].float() / T
    if top_k:
        l = l.masked_fill(l < l.topk(top_k).values[:, -1:], -float("inf"))
    s, idx = l.sort(descending=True)
    pr = s.softmax(-1)
    s = s.masked_fill(pr.cumsum(-1) - pr >= top_p, -float("inf"))  # drop what follows the token that reaches top_p
    g = -torch.log(-torch.log(torch.rand_like(s).clamp_(1e-7, 1 - 1e-7)))
    return idx.gather(1, (s + g).argmax(-1, keepdim=True))[:, 0]


def bench_sampler(B, rounds, reps, emit):
    V, ld, T, P = 50257, 50304, 0.8, 0.9
    z = torch.zeros(B, ld, device=DEV, dtype=BF)
    z[:, :V] = (torch.randn(B, V, device=DEV) * 2.0).to(BF)
    pos = torch.arange(B, dtype=torch.int32, device=DEV)
    ok = True
    for top_k in (0, 50):
        fns = {"sample_step top_p": lambda i: sample_step(z, V, T, top_k, P, 1, 0, pos),
               "sample_logits": lambda i: sample_logits(z, V, T, top_k, 1, 0, pos),
               "torch top_p": lambda i: torch_top_p(z, V, T, top_k, P)}
        for fn in fns.values():
            window(fn, 10)
        us = {k: [] for k in fns}
        for r in range(rounds):
            for kname, fn in fns.items():  # alternated
                ms = window(fn, reps)
                us[kname].append(ms * 1e3)
                emit({"sampler": kname, "B": B, "V": V, "T": T, "top_k": top_k, "top_p": P if "top_p" in kname else 1.0,
                      "round": r, "us": round(ms * 1e3, 2)})
        med = {k: statistics.median(v) for k, v in us.items()}
        gate = med["sample_step top_p"] <= med["torch top_p"]
        ok = ok and gate
        emit({"summary": "sampler", "top_k": top_k, "sample_step_us": round(med["sample_step top_p"], 2),
              "sample_logits_us": round(med["sample_logits"], 2), "torch_top_p_us": round(med["torch top_p"], 2),
              "step_over_sample_logits": round(med["sample_step top_p"] / med["sample_logits"], 3),
              "gate_step_not_slower_than_torch": bool(gate)})
    return ok


@torch.no_grad()
def run_step_loop(engine, B, ctx, steps, ragged):
    """run_loop with generate()'s sampling lines: today's (sample_logits, then the column store) or, ragged, cache
    lengths ctx - 3 b and sample_step with the token matrix, the done flags, the lengths and an eos in its launch.
    Returns (seconds, rows done at the end)."""
    stages = [engine.stages[s] for s in range(engine.P)]
    ctx = min(ctx, stages[0].cfg.block_size - steps)
    caches = [st.new_cache(B, ctx + steps) for st in stages]
    lens = torch.full((B,), ctx, dtype=torch.int32, device=DEV)
    if ragged:
        lens -= (3 * torch.arange(B, device=DEV, dtype=torch.int32)).clamp_(max=ctx - 1)
    for c in caches:
        for t in c.k + c.v:
            t.normal_()
        c.lens.copy_(lens)
        c.n = ctx
    V = stages[0].cfg.vocab_size
    out = torch.zeros((B, ctx + steps), dtype=torch.int64, device=DEV)
    done = torch.zeros(B, dtype=torch.int32, device=DEV)
    gen_len = torch.zeros(B, dtype=torch.int32, device=DEV)
    tok = torch.randint(0, V, (B,), device=DEV)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for t in range(steps):
        x = tok
        for st, c in zip(stages, caches):
            x = st.decode_step(x, c)
        if ragged:
            tok = sample_step(x, V, 0.0, 0, 1.0, 0, 0, caches[-1].lens, out, done, gen_len, V - 1, 0)
        else:
            tok = sample_logits(x, V, 0.0, 0, 0, 0, caches[-1].lens)
            out[:, ctx + t] = tok
    torch.cuda.synchronize()
    return time.perf_counter() - t0, int(done.sum())


def bench_step_loop(engine, B, ctx, steps, rounds, emit):
    for ragged in (False, True):
        run_step_loop(engine, B, ctx, 8, ragged)
    tps = {False: [], True: []}
    for r in range(rounds):
        for ragged in (False, True):  # alternated
            s, nd = run_step_loop(engine, B, ctx, steps, ragged)
            tps[ragged].append(B * steps / s)
            emit({"loop": "ragged + eos (sample_step)" if ragged else "today (sample_logits + store)", "B": B,
                  "ctx": ctx, "steps": steps, "round": r, "ms_per_step": round(s / steps * 1e3, 4),
                  "tokens_per_s": round(B * steps / s, 1), "rows_done": nd})
    a, b = statistics.median(tps[True]), statistics.median(tps[False])
    emit({"summary": "decode loop, step sampler", "B": B, "ctx": ctx, "ragged_tokens_per_s": round(a, 1),
          "today_tokens_per_s": round(b, 1), "ragged_over_today": round(a / b, 3)})


def bench_loop(engine, B, ctx, steps, rounds, emit, gate):
    for hand in (True, False):
        run_loop(engine, B, ctx, 8, hand)  # warm-up of both paths at this shape
    tps = {True: [], False: []}
    for r in range(rounds):
        for hand in (True, False):  # alternated
            s = run_loop(engine, B, ctx, steps, hand)
            tps[hand].append(B * steps / s)
            emit({"loop": "hand" if hand else "lib", "B": B, "ctx": ctx, "steps": steps, "round": r,
                  "ms_per_step": round(s / steps * 1e3, 4), "tokens_per_s": round(B * steps / s, 1)})
    h, l = statistics.median(tps[True]), statistics.median(tps[False])
    rec = {"summary": "decode loop", "B": B, "ctx": ctx, "hand_tokens_per_s": round(h, 1),
           "lib_tokens_per_s": round(l, 1), "hand_over_lib": round(h / l, 3)}
    if gate:
        rec["gate_hand_at_least_lib"] = bool(h >= l)
    emit(rec)
    return h >= l


# ---- the graph-replayed step (--graph) -----------------------------------------------------------------------------
def bench_fused_kernels(B, ctxs, rounds, reps, emit):
    """One-launch (tickets) against two-launch windows of the decode kernels, operands as in bench_kernels."""
    K = _native.kernels()
    for name, (N, Kd) in SHAPES.items():
        if name == "lm_head":  # not split over K: there is one launch either way
            continue
        copies = max(2, min(reps, LLC_BYTES // (N * Kd * 2) + 1))
        w = torch.randn(copies, N, Kd, device=DEV, dtype=BF) * 0.02
        b = torch.randn(N, device=DEV, dtype=BF)
        x = torch.randn(B, Kd, device=DEV, dtype=BF)
        tk = torch.zeros(N // 16, dtype=torch.int32, device=DEV)
        epi = 5 if name == "c_fc" else 1
        fns = {"two launches": lambda i: K.linear_decode(x, w[i % copies], b, epi),
               "one launch": lambda i: K.linear_decode(x, w[i % copies], b, epi, tk)}
        for fn in fns.values():
            window(fn, copies)
        for r in range(rounds):
            for kname, fn in fns.items():  # alternated
                ms = window(fn, reps)
                emit({"kernel": "linear_decode", "form": kname, "shape": name, "M": B, "N": N, "K": Kd,
                      "KS": K.linear_decode_splits(N, Kd), "round": r, "us": round(ms * 1e3, 2)})
        del w
    H, D = 12, 64
    for ctx in ctxs:
        Smax = ctx + 1
        copies = max(2, min(reps, LLC_BYTES // (B * Smax * H * D * 2 * 2) + 1))
        kc = torch.randn(copies, B, Smax, H, D, device=DEV, dtype=BF)
        vc = torch.randn(copies, B, Smax, H, D, device=DEV, dtype=BF)
        qkv = torch.randn(B, 3 * H * D, device=DEV, dtype=BF)
        lens = torch.full((B,), ctx, dtype=torch.int32, device=DEV)
        tk = torch.zeros(B * H, dtype=torch.int32, device=DEV)
        fns = {"two launches": lambda i: K.attention_decode(qkv, kc[i % copies], vc[i % copies], lens, 0.125, Smax),
               "one launch": lambda i: K.attention_decode(qkv, kc[i % copies], vc[i % copies], lens, 0.125, Smax, tk)}
        for fn in fns.values():
            window(fn, copies)
        for r in range(rounds):
            for kname, fn in fns.items():
                ms = window(fn, reps)
                emit({"kernel": "attention_decode", "form": kname, "B": B, "H": H, "ctx": ctx, "round": r,
                      "us": round(ms * 1e3, 2)})
        del kc, vc


SAMPLING = Sampling(vocab=50257, temperature=0.0, top_k=0, top_p=1.0, seed=0, sample0=0, eos=-1, pad=0)


@torch.no_grad()
def graph_session(engine, B, ctx, steps, sites):
    """A captured step (generate(graph=True)'s session) over caches of ctx + steps rows with random contents."""
    ctx = min(ctx, engine.stages[0].cfg.block_size - steps)
    ses = DecodeSession(engine, None, B, ctx + steps, _sites=sites)
    ses.capture(engine, SAMPLING)
    for c in ses.caches.values():
        for t in c.k + c.v:
            t.normal_()
    return ses, ctx


@torch.no_grad()
def run_graph_loop(ses, ctx, steps):
    """Seconds of `steps` replays from caches holding ctx keys."""
    ses.reset()
    for c in ses.caches.values():
        c.lens.fill_(ctx)
        c.n = ctx
    ses.tok.random_(0, 50257)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        ses.replay()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def bench_graph_loop(engine, B, ctx, steps, rounds, emit, gate, sites):
    forms = {"(a) eager": "eager", "(b) graph, two-launch kernels": (), "(c) graph, one-launch kernels": None}
    if sites:
        for s in DECODE_SITES:  # each site flipped against decode_step's choice
            if s in DECODE_FUSED_SITES:
                forms[f"(c) with {s} on two launches"] = tuple(DECODE_FUSED_SITES - {s})
            else:
                forms[f"(c) with {s} on one launch"] = tuple(DECODE_FUSED_SITES | {s})
    ses = {k: graph_session(engine, B, ctx, steps, f) for k, f in forms.items() if f != "eager"}
    run_loop(engine, B, ctx, 8, True)
    for k, (se, c) in ses.items():
        run_graph_loop(se, c, 8)
    tps = {k: [] for k in forms}
    for r in range(rounds):
        for k in forms:  # alternated
            s = run_loop(engine, B, ctx, steps, True) if forms[k] == "eager" else run_graph_loop(*ses[k], steps)
            tps[k].append(B * steps / s)
            emit({"loop": k, "B": B, "ctx": ctx, "steps": steps, "round": r, "ms_per_step": round(s / steps * 1e3, 4),
                  "tokens_per_s": round(B * steps / s, 1)})
    a, b, c = (tps[k] for k in list(forms)[:3])
    rec = {"summary": "graph-replayed decode loop", "B": B, "ctx": ctx,
           "eager_tokens_per_s": [round(v, 1) for v in a], "graph_two_launch_tokens_per_s": [round(v, 1) for v in b],
           "graph_one_launch_tokens_per_s": [round(v, 1) for v in c],
           "one_launch_over_eager": round(statistics.median(c) / statistics.median(a), 3),
           "one_launch_over_two_launch": round(statistics.median(c) / statistics.median(b), 3)}
    for k in list(forms)[3:]:
        rec[k] = round(statistics.median(tps[k]) / statistics.median(c), 3)  # > 1: the flipped site is faster
    ok = all(x >= y for x, y in zip(c, a))
    if gate:
        rec["gate_graph_at_least_eager_every_round"] = bool(ok)
    emit(rec)
    del ses
    torch.cuda.empty_cache()
    return ok


def main_graph(a):
    os.makedirs(os.path.dirname(a.out_graph) or ".", exist_ok=True)
    mesh = init_mesh(pp=1, schedule_kind="1f1b", rank=0, world_size=1, device=DEV)
    engine = PipelineEngine(get_model_spec("gpt2", 2), mesh, schedule_kind="1f1b", num_microbatches=1)
    engine.eval()
    if a.replays:
        ses, ctx = graph_session(engine, a.B, a.ctx, a.replays, None)
        s = run_graph_loop(ses, ctx, a.replays)
        print(json.dumps({"replays": a.replays, "ms_per_step": round(s / a.replays * 1e3, 4)}), flush=True)
        return 0
    with open(a.out_graph, "w") as f:
        def emit(rec):
            line = json.dumps(rec)
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()

        if not a.no_kernels:
            bench_fused_kernels(a.B, sorted({128, a.ctx, 1024}), a.rounds, a.reps, emit)
        ok = bench_graph_loop(engine, a.B, a.ctx, a.steps, a.rounds, emit, gate=True, sites=True)
        if a.sweep:
            for B in (1, 16, 64):
                for ctx in (128, 1024):
                    bench_graph_loop(engine, B, ctx, a.steps, a.rounds, emit, gate=False, sites=False)
    return 0 if ok else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=16)
    ap.add_argument("--ctx", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=200, help="calls per kernel timing window")
    ap.add_argument("--steps", type=int, default=128, help="decode steps per loop timing")
    ap.add_argument("--sweep", action="store_true", help="also B in {1, 16, 64} x ctx in {128, 1024}")
    ap.add_argument("--no_kernels", action="store_true")
    ap.add_argument("--out_kernels", default="profiles/generate_kernels.jsonl")
    ap.add_argument("--out_loop", default="profiles/generate_gpt2.jsonl")
    ap.add_argument("--ragged", action="store_true", help="only the step sampler's window and its decode-loop row")
    ap.add_argument("--out_ragged", default="profiles/ragged_generate.jsonl")
    ap.add_argument("--graph", action="store_true", help="only the graph-replayed step: kernel windows and the loops")
    ap.add_argument("--out_graph", default="profiles/generate_graph.jsonl")
    ap.add_argument("--replays", type=int, default=0, help="with --graph: capture, replay this often, nothing else")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_generate.py measures on the GPU; none is visible")
    if a.graph:
        return main_graph(a)
    if a.ragged:
        os.makedirs(os.path.dirname(a.out_ragged) or ".", exist_ok=True)
        with open(a.out_ragged, "w") as f:
            def emit(rec):
                line = json.dumps(rec)
                print(line, flush=True)
                f.write(line + "\n")
                f.flush()

            ok = bench_sampler(a.B, a.rounds, a.reps, emit)
            mesh = init_mesh(pp=1, schedule_kind="1f1b", rank=0, world_size=1, device=DEV)
            engine = PipelineEngine(get_model_spec("gpt2", 2), mesh, schedule_kind="1f1b", num_microbatches=1)
            engine.eval()
            bench_step_loop(engine, a.B, a.ctx, a.steps, a.rounds, emit)
        return 0 if ok else 1
    for p in (a.out_kernels, a.out_loop):
        os.makedirs(os.path.dirname(p) or ".", exist_ok=True)
    ok = True
    with open(a.out_kernels, "w") as fk, open(a.out_loop, "w") as fl:
        def emitter(f):
            def emit(rec):
                line = json.dumps(rec)
                print(line, flush=True)
                f.write(line + "\n")
                f.flush()
            return emit

        if not a.no_kernels:
            bench_kernels(a.B, sorted({128, a.ctx, 1024}), a.rounds, a.reps, emitter(fk))
        mesh = init_mesh(pp=1, schedule_kind="1f1b", rank=0, world_size=1, device=DEV)
        engine = PipelineEngine(get_model_spec("gpt2", 2), mesh, schedule_kind="1f1b", num_microbatches=1)
        engine.eval()
        ok = bench_loop(engine, a.B, a.ctx, a.steps, a.rounds, emitter(fl), gate=True)
        if a.sweep:
            for B in (1, 16, 64):
                for ctx in (128, 1024):
                    bench_loop(engine, B, ctx, a.steps, a.rounds, emitter(fl), gate=False)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
