"""Shared numerics for the AdamW tests: the update rule in fp64 (the truth), torch.optim.AdamW in fp32 on the CPU
(the yardstick: its error against the truth is what an fp32 implementation of the rule may cost), seeded inputs."""
from __future__ import annotations

import math

import torch

BETAS, EPS = (0.9, 0.999), 1e-8


def seeded(n: int, seed: int = 0, steps: int = 5, dtype=torch.float32):
    """p0 ~ N(0, 1) and ``steps`` gradients whose magnitudes span 1e-6..1 (log-uniform, random sign)."""
    gen = torch.Generator().manual_seed(seed)
    p0 = torch.randn(n, generator=gen)
    grads = []
    for _ in range(steps):
        mag = torch.pow(10.0, -6.0 * torch.rand(n, generator=gen))
        sign = torch.where(torch.rand(n, generator=gen) < 0.5, -1.0, 1.0)
        grads.append((mag * sign).to(dtype))
    return p0, grads


def truth(p0, grads, lrs, clips, wd_elem, betas=BETAS, eps=EPS):
    """The rule of the issue in fp64 from fp32 (or bf16) inputs: (p, m, v) after len(grads) steps. ``lrs`` / ``clips``:
    the learning rate and clip coefficient of each step; ``wd_elem``: per-element weight decay (tensor or number)."""
    b1, b2 = betas
    p = p0.double().clone()
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    wd = wd_elem.double() if torch.is_tensor(wd_elem) else float(wd_elem)
    for t, (g, lr, c) in enumerate(zip(grads, lrs, clips), 1):
        g = g.double() * float(c)
        p = p * (1.0 - lr * wd)
        m = b1 * m + (1.0 - b1) * g
        v = b2 * v + (1.0 - b2) * g * g
        p = p - (lr / (1.0 - b1 ** t)) * m / (v.sqrt() / math.sqrt(1.0 - b2 ** t) + eps)
    return p, m, v


def torch_adamw(p0, grads, lrs, clips, wd_elem, wd: float, betas=BETAS, eps=EPS):
    """torch.optim.AdamW (fp32, CPU) on the same inputs: (p, m, v). Elements with and without decay are two
    parameter groups; the clip coefficient is applied to the fp32 gradient, as clip_grad_norm_ does."""
    p0 = p0.float()
    n = p0.numel()
    dec = (wd_elem != 0) if torch.is_tensor(wd_elem) else torch.full((n,), bool(wd_elem != 0))
    idx = [torch.nonzero(dec).flatten(), torch.nonzero(~dec).flatten()]
    ps = [torch.nn.Parameter(p0[i].clone()) for i in idx]
    groups = [{"params": [ps[0]], "weight_decay": wd}, {"params": [ps[1]], "weight_decay": 0.0}]
    groups = [g for g, i in zip(groups, idx) if i.numel()]
    opt = torch.optim.AdamW(groups, lr=lrs[0], betas=betas, eps=eps, foreach=False)
    for g, lr, c in zip(grads, lrs, clips):
        g = g.float() * torch.tensor(float(c), dtype=torch.float32) if float(c) != 1.0 else g.float()
        for grp in opt.param_groups:
            grp["lr"] = lr
        for q, i in zip(ps, idx):
            q.grad = g[i].clone()
        opt.step()
    p, m, v = torch.empty(n), torch.zeros(n), torch.zeros(n)
    for q, i in zip(ps, idx):
        if i.numel():
            p[i] = q.detach()
            m[i], v[i] = opt.state[q]["exp_avg"], opt.state[q]["exp_avg_sq"]
    return p, m, v


def errors(got, want):
    """Max abs error of each of (p, m, v) against the fp64 truth."""
    return [float((a.double() - b).abs().max()) for a, b in zip(got, want)]


def check_within_2E(got, p0, grads, lrs, clips, wd_elem, wd, what=""):
    """``got`` = (p, m, v) of the implementation under test: each within 2 E of the fp64 truth, E = torch.optim.AdamW's
    own fp32 error on the same inputs (the factor 2: torch forms m with lerp where the rule uses multiply-add, about
    one rounding per operation either way). Prints the figures before asserting."""
    want = truth(p0, grads, lrs, clips, wd_elem)
    E = errors(torch_adamw(p0, grads, lrs, clips, wd_elem, wd), want)
    err = errors(got, want)
    print(f"adamw {what}: err p/m/v = {err}, torch fp32 E = {E}")
    for name, e, lim in zip("pmv", err, E):
        assert e <= 2.0 * lim, f"{what} {name}: error {e:.3e} > 2 x {lim:.3e} (torch.optim.AdamW fp32 vs fp64)"
