"""Optimizer kernels at GPT-2 small's flat size (about 124 M elements, bf16 weights with fp32 master weights):
``sgd_momentum_mixed_``, ``adamw_mixed_`` and ``grad_sqnorm``, alternated in one process after a warm-up, each timed
by device events around every call. Writes one JSON line per kernel (median time, achieved bytes/s) to --out.

    python tools/bench_adamw.py [--n 124475904] [--calls 20] [--out profiles/adamw_kernels.jsonl]

Bytes per element: mixed AdamW 30 (read g 2, master 4, m 4, v 4; write master 4, m 4, v 4, p 2, g 2), mixed SGD
with momentum 22, grad_sqnorm 2.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from simple_distributed_machine_learning_amd import ops  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=124475904, help="elements (a multiple of 64)")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="profiles/adamw_kernels.jsonl")
    a = ap.parse_args()
    dev, n = torch.device("cuda", 0), a.n // 64 * 64
    master = torch.randn(n, device=dev) * 0.02
    p, g = master.bfloat16(), (torch.randn(n, device=dev) * 1e-3).bfloat16()
    buf, m, v = torch.zeros_like(master), torch.zeros_like(master), torch.zeros_like(master)
    decay = torch.ones(n // 64, dtype=torch.uint8, device=dev)
    ctr = torch.zeros(1, dtype=torch.int64, device=dev)
    prep = torch.zeros(ops.ADAMW_PREP_FLOATS, device=dev)
    norm2 = torch.zeros(1, dtype=torch.float64, device=dev)
    parts = torch.zeros(ops.SQNORM_MAX_BLOCKS, device=dev)
    ops.adamw_prep(ctr, prep, 3e-4, 0.9, 0.999, 1.0, None, g=g, partials=parts, norm2=norm2)
    # zero_grad on, as in the training step (the store of g is 2 of SGD's 22 and AdamW's 30 bytes); after the first call
    # the gradients read are zeros, which changes no instruction count and no traffic
    kernels = {
        "sgd_momentum_mixed": (22, lambda: ops.sgd_momentum_mixed_(master, p, g, buf, 1e-4, 0.5, zero_grad=True)),
        "adamw_mixed": (30, lambda: ops.adamw_mixed_(master, p, g, m, v, decay, prep, 0.9, 0.999, 1e-8, 0.1, True)),
        "grad_sqnorm": (2, lambda: ops.grad_sqnorm(g, out=norm2, partials=parts)),
    }
    times = {k: [] for k in kernels}
    for i in range(a.warmup + a.calls):
        for name, (_, fn) in kernels.items():  # alternated: every kernel sees the same clocks and cache state
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if i >= a.warmup:
                times[name].append(e0.elapsed_time(e1))
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        for name, (bpe, _) in kernels.items():
            t = sorted(times[name])
            med = statistics.median(t)
            rec = {"kernel": name, "n": n, "calls": len(t), "ms_median": round(med, 4), "ms_min": round(t[0], 4),
                   "ms_max": round(t[-1], 4), "bytes_per_element": bpe,
                   "TB_per_s": round(n * bpe / (med * 1e-3) / 1e12, 3)}
            print(json.dumps(rec))
            f.write(json.dumps(rec) + "\n")
    s, w, q = (statistics.median(times[k]) for k in ("sgd_momentum_mixed", "adamw_mixed", "grad_sqnorm"))
    print(json.dumps({"adamw_over_sgd": round(w / s, 3), "expected_at_most": round(30 / 22 * 1.15, 3),
                      "sqnorm_over_adamw": round(q / w, 3), "expected_at_most_": 0.15}))


if __name__ == "__main__":
    main()
