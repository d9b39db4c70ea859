"""Masked fp64 references and fp32 rounding models for the GPT-2 kernels with dropout (docs/NUMERICS.md, "Dropout").
Extends tests/gpt2_numerics.py, which it imports unchanged: the same checker, the same margins. The masks come from
the torch twin of the kernels' counter hash (ops/reference.py); plain torch, runs on the CPU.

Rounding points of the kernels that the models follow:
* forward: the running max and the denominator l use the undropped p; M o p is rounded to bf16 for the PV product;
  y = bf16(o * ((1 / l) * f)), f = 256 / (256 - T) in fp32.
* backward: P recomputed from LSE; dV = bf16(sum(bf16(M o P) dO) * f); dS = P (M o dP * f - delta) rounded to bf16
  for the dK / dQ products; delta = rowsum(dO * y) with the dropped y.
* element-wise sites: xs = bf16(x + M o h * f) (one rounding); dh = bf16(d * f) where kept, from the fp32 d.
"""
import math

import torch

import gpt2_numerics as gn
from simple_distributed_machine_learning_amd.ops import reference as R

ATTN_S = [1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 257]
ATTN_FAMILIES = ["uniform 1.5", "uniform 6", "growing keys"]
BF = torch.bfloat16
SEED = 0x1234ABCD5678EF
LAYER = 3


def rnd(*shape, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.empty(shape).uniform_(-1, 1, generator=g)


def attn_inputs(family, B, S, H, seed):
    """q, k, v, dout [B, S, H, 64] bf16 on the CPU (the families of tests/test_gpt2_numerics_gpu.py)."""
    u = [rnd(B, S, H, 64, seed=seed + i) for i in range(4)]
    if family.startswith("uniform"):
        amp = float(family.split()[1])
        q, k, v = u[0] * amp, u[1] * amp, u[2] * amp
    else:  # key norms grow along S: the running maximum moves at every tile
        grow = 0.5 + 4.0 * torch.arange(S).float().view(1, S, 1, 1) / max(S - 1, 1)
        q, k, v = u[0] * 1.5, u[1] * grow, u[2] * 1.5
    return q.to(BF), k.to(BF), v.to(BF), u[3].to(BF)


def attn_keep(B, H, S, T, ctr=0, sample0=0, head0=0, seed=SEED, layer=LAYER):
    """[B, H, S, S] bool keep mask from the twin."""
    return R.gpt2_attn_keep(seed, torch.tensor([ctr]), layer, sample0, B, head0, H, S, T)


def f32scale(T):
    return R.dropout_scale(T)


# ---- attention ------------------------------------------------------------------------------------------------------
def attention_drop_ref64(q, k, v, scale, causal, keep, T, dout=None, keep_bwd=None):
    """float64 attention with dropout on the probabilities: y = (M o P f) V. keep_bwd: the mask the backward uses (a
    seeded defect; default: the forward's)."""
    q, k, v = (t.double() for t in (q, k, v))
    f = 256.0 / (256.0 - T)
    s = gn._scores(q, k) * scale
    if causal:
        s = s.masked_fill(~gn._causal_mask(s.shape[-1], s.device), -math.inf)
    lse = torch.logsumexp(s, -1)
    p = torch.exp(s - lse[..., None])
    y = torch.einsum("bhqk,bkhd->bqhd", p * keep * f, v)
    out = {"y": y, "lse": lse, "p": p}
    if dout is not None:
        kb = keep if keep_bwd is None else keep_bwd
        d = dout.double()
        delta = (d * y).sum(-1).permute(0, 2, 1)
        dp = torch.einsum("bqhd,bkhd->bhqk", d, v) * kb * f
        ds = p * (dp - delta[..., None])
        out["dv"] = torch.einsum("bhqk,bqhd->bkhd", p * kb * f, d)
        out["dk"] = torch.einsum("bhqk,bqhd->bkhd", ds, q) * scale
        out["dq"] = torch.einsum("bhqk,bkhd->bqhd", ds, k) * scale
    return out


def attention_drop_model_direct(q, k, v, scale, causal, keep, T, scale_l=False):
    """fp32 model over whole rows. scale_l: the seeded defect "the factor applied to l as well"."""
    q, k, v = (t.float() for t in (q, k, v))
    sl2, f = gn._sl2(scale), f32scale(T)
    s = gn._scores(q, k)
    if causal:
        s = s.masked_fill(~gn._causal_mask(s.shape[-1], s.device), -math.inf)
    m = s.amax(-1, keepdim=True) * sl2
    p = torch.exp2(s * sl2 - m)
    l = p.sum(-1)
    if scale_l:
        l = l * f
    o = torch.einsum("bhqk,bkhd->bqhd", gn.rbf(p * keep), v)
    y = gn.rbf(o * ((1.0 / l) * f).permute(0, 2, 1)[..., None])
    return {"y": y, "lse2": m[..., 0] + torch.log2(l)}


def attention_drop_model_tiled(q, k, v, scale, causal, keep, T, tile=gn.KEY_TILE):
    """fp32 model as the forward kernel runs it: online softmax over 64-key tiles; the undropped p feed l, M o p is
    rounded to bf16 for the PV product."""
    q, k, v = (t.float() for t in (q, k, v))
    B, S, H, D = q.shape
    sl2, f = gn._sl2(scale), f32scale(T)
    m = torch.full((B, H, S), -math.inf)
    l = torch.zeros(B, H, S)
    o = torch.zeros(B, H, S, D)
    qpos = torch.arange(S)[:, None]
    for k0 in range(0, S, tile):
        kt, vt = k[:, k0:k0 + tile], v[:, k0:k0 + tile]
        s = gn._scores(q, kt)
        if causal:
            s = s.masked_fill((torch.arange(k0, k0 + kt.shape[1])[None, :] > qpos), -math.inf)
        mx = torch.maximum(m, s.amax(-1) * sl2)
        alpha = torch.where(m == -math.inf, torch.zeros_like(m), torch.exp2(m - mx))
        msub = torch.where(mx == -math.inf, torch.zeros_like(mx), mx)
        p = torch.exp2(s * sl2 - msub[..., None])
        l = l * alpha + p.sum(-1)
        o = o * alpha[..., None] + torch.einsum("bhqk,bkhd->bhqd", gn.rbf(p * keep[..., k0:k0 + tile]), vt)
        m = mx
    y = gn.rbf(o * ((1.0 / l) * f)[..., None]).permute(0, 2, 1, 3)
    return {"y": y, "lse2": m + torch.log2(l)}


def attention_drop_model_bwd(q, k, v, y, lse2, dout, scale, causal, keep, T):
    """fp32 backward model; y and the log2-domain lse are the backward kernels' inputs (see gn.attention_model_bwd)."""
    q, k, v, d = (t.float() for t in (q, k, v, dout))
    sl2, f = gn._sl2(scale), f32scale(T)
    p = torch.exp2(gn._scores(q, k) * sl2 - lse2[..., None])
    if causal:
        p = p.masked_fill(~gn._causal_mask(p.shape[-1], p.device), 0.0)
    delta = gn._delta_fp32(dout, y)
    dp = torch.einsum("bqhd,bkhd->bhqk", d, v)
    ds = p * (torch.where(keep, dp * f, torch.zeros_like(dp)) - delta[..., None])
    dv = torch.einsum("bhqk,bqhd->bkhd", gn.rbf(p * keep), d) * f
    dk = torch.einsum("bhqk,bqhd->bkhd", gn.rbf(ds), q) * scale
    dq = torch.einsum("bhqk,bkhd->bqhd", gn.rbf(ds), k) * scale
    return {"dq": gn.rbf(dq), "dk": gn.rbf(dk), "dv": gn.rbf(dv)}


def attention_drop_cancellation_bound(q, k, v, y, dout, p64, scale, T):
    """gn.attention_cancellation_bound with dropout: dS = P (M o dP f - delta) subtracts two fp32 sums of 64 exact
    products each, of which the first is now multiplied by f <= 256 / (256 - T) (0 where dropped); each sum is bounded in
    any order by 64 * 2^-24 * sum|terms|."""
    f = 256.0 / (256.0 - T)
    q, k, v, y, d = (t.double().abs() for t in (q, k, v, y, dout))
    a = f * torch.einsum("bqhd,bkhd->bhqk", d, v) + (d * y).sum(-1).permute(0, 2, 1)[..., None]
    eds = p64 * (gn.HD * gn.U32) * a
    return {"dq": torch.einsum("bhqk,bkhd->bqhd", eds, k) * scale, "dk": torch.einsum("bhqk,bqhd->bkhd", eds, q) * scale}


# ---- element-wise sites ---------------------------------------------------------------------------------------------
def site_keep(site, B, S, C, T, ctr=0, sample0=0, seed=SEED, layer=LAYER):
    return R.gpt2_site_keep(seed, torch.tensor([ctr]), site, layer, sample0, B, S, C, T)


def drop_add_ref64(x, h, keep, T):
    return x.double() + h.double() * keep * (256.0 / (256.0 - T))


def drop_add_model(x, h, keep, T):
    """xs = bf16(x + M o h * f): the product and the sum in fp32, one rounding to bf16."""
    return gn.rbf(x.float() + torch.where(keep, h.float() * f32scale(T), torch.zeros_like(h.float())))


def drop_add_fp32_bound(x, h, T):
    """fp32 steps of xs = bf16(x + h f) before the one bf16 rounding: f itself (256 / (256 - T) rounded to fp32), the
    product h f and the sum, one rounding of 2^-24 each relative to their own results. The first two are relative to
    |h f|, not to the sum, which may cancel (x = -1, h = 115 / 128, T = 26 gives exactly 0 in real arithmetic)."""
    hf = h.double().abs() * (256.0 / (256.0 - T))
    return 2 * gn.U32 * hf + gn.U32 * (x.double().abs() + hf)


def drop_scale_ref64(g, keep, T):
    return g.double() * keep * (256.0 / (256.0 - T))


def drop_scale_model(g, keep, T):
    return gn.rbf(torch.where(keep, g.float() * f32scale(T), torch.zeros_like(g.float())))
