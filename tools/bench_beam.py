"""Beam search's step, cache gather and end-to-end cost on the GPU, hand-written kernels against torch compositions.

    python tools/bench_beam.py [--rounds 3] [--out profiles/beam_step.jsonl]

(i)   beam_step [R, 50257] (ld 50304), (B, K) = (4, 4) and (8, 8): beam.hip's two launches against log_softmax of the
      fp32 logits + scores, topk over [B, K V] and the index arithmetic. Windows of --reps back-to-back calls that end
      in a synchronise, hand and torch alternated over the rounds. Gate: hand is not slower in any round.
(ii)  beam_gather_kv, GPT-2 small's 12 layers, R = 16, u = 32 and 128, against 24 index_selects; GB/s of the bytes it
      reads and writes. Reported, not gated.
(iii) generate(num_beams=4) on GPT-2 small, 4 prompts of 512 tokens, 32 new, ms per call, against num_samples=4 greedy
      on the same prompts (the same rows without the search). Reported, not gated.
Everything runs in one process; all rounds are written."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from simple_distributed_machine_learning_amd.models import get_model_spec  # noqa: E402
from simple_distributed_machine_learning_amd.ops.decode import beam_gather_kv, beam_step  # noqa: E402
from simple_distributed_machine_learning_amd.parallel import PipelineEngine, init_mesh  # noqa: E402
from simple_distributed_machine_learning_amd.parallel.generate import generate  # noqa: E402

DEV = torch.device("cuda", 0)
V, LD = 50257, 50304


def window(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps  # us per call


def torch_beam_step(z, K, score, fin, glen, eos):
    R = z.shape[0]
    B = R // K
    c = torch.log_softmax(z[:, :V].float(), dim=-1) + score[:, None]
    s_new, idx = c.view(B, K * V).topk(K, dim=1)
    par, tok = idx // V, idx % V
    prow = (torch.arange(B, device=z.device)[:, None] * K + par).reshape(R)
    tok = tok.reshape(R)
    pf = fin[prow]
    return tok, par.reshape(R), s_new.reshape(R), pf | (tok == eos).to(torch.int32), glen[prow] + 1 - pf


def bench_step(rounds, reps, emit):
    ok = True
    for B, K in ((4, 4), (8, 8)):
        R = B * K
        z = torch.randn((R, LD), device=DEV).to(torch.bfloat16)
        score = -torch.rand(R, device=DEV) * 5
        fin, glen = torch.zeros((2, R), dtype=torch.int32, device=DEV)
        for r in range(rounds):
            hand = window(lambda: beam_step(z, V, K, score, fin, glen, 0, 0), reps)
            tch = window(lambda: torch_beam_step(z, K, score, fin, glen, 0), reps)
            ok = ok and hand <= tch
            emit(dict(part="i", op="beam_step", B=B, K=K, vocab=V, ld=LD, round=r, reps=reps, hand_us=hand,
                      torch_us=tch, gate_hand_not_slower=hand <= tch))
    return ok


def bench_gather(rounds, reps, emit):
    L, R, K, H, D, nmax = 12, 16, 4, 12, 64, 128
    buf = torch.randn((2, L, 2, R, nmax, H, D), device=DEV).to(torch.bfloat16)
    par = torch.randint(0, K, (R,), dtype=torch.int32, device=DEV)
    rows = torch.arange(R, device=DEV) // K * K + par
    for u in (32, 128):
        moved = 2 * L * 2 * R * u * H * D * 2
        views = [buf[0, l, kv] for l in range(L) for kv in range(2)]
        for r in range(rounds):
            hand = window(lambda: beam_gather_kv(buf, 0, par, K, u), reps)
            tch = window(lambda: [v[:, :u].index_select(0, rows) for v in views], reps)
            emit(dict(part="ii", op="beam_gather_kv", layers=L, R=R, u=u, round=r, reps=reps, hand_us=hand,
                      index_select_x24_us=tch, bytes_moved=moved, hand_GBps=moved / hand / 1e3))


def bench_end_to_end(rounds, calls, emit):
    mesh = init_mesh(pp=1, schedule_kind="1f1b", rank=0, world_size=1, device=DEV)
    eng = PipelineEngine(get_model_spec("gpt2", 2), mesh, schedule_kind="1f1b", num_microbatches=1)
    prompts = torch.randint(0, V, (4, 512), generator=torch.Generator().manual_seed(1))

    def ms(**kw):
        generate(eng, prompts, 32, **kw)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            generate(eng, prompts, 32, **kw)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / calls

    for r in range(rounds):
        emit(dict(part="iii", model="gpt2", prompts=4, prompt_len=512, new=32, round=r, calls=calls,
                  num_beams4_ms=ms(num_beams=4), num_samples4_greedy_ms=ms(num_samples=4)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=200, help="calls per timing window of (i) and (ii)")
    ap.add_argument("--calls", type=int, default=3, help="generate calls per timing of (iii)")
    ap.add_argument("--parts", default="i,ii,iii")
    ap.add_argument("--out", default="profiles/beam_step.jsonl")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_beam.py measures on the GPU; none is visible")
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
            ok = bench_step(a.rounds, a.reps, emit)
        if "ii" in parts:
            bench_gather(a.rounds, a.reps, emit)
        if "iii" in parts:
            bench_end_to_end(a.rounds, a.calls, emit)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
