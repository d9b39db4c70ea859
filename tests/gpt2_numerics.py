"""fp64 references, fp32 rounding models and the error-budget checker for the GPT-2 kernels (attention, vocabulary
cross-entropy, LayerNorm, column sums). Plain torch, runs on the CPU; docs/NUMERICS.md describes the scheme.

* A reference is the operation in float64 on the kernel's bf16 inputs.
* A rounding model is the operation in float32, rounded to bf16 exactly where the kernel rounds.
* `check_elementwise` bounds |got - ref64| per element from the fp32 arithmetic of the kernel; `check_grouped` bounds a
  tensor's error by the error of its rounding model (per last-dimension row and in RMS). Neither exempts an element.
"""
import math

import torch

LOG2E = 1.4426950408889634  # the kernels' constant
LN2 = math.log(2.0)
U32 = 2.0 ** -24  # fp32 unit roundoff
ROW_MARGIN = 3.0  # grouped mode: worst element of a row, kernel error over model error
RMS_MARGIN = 1.25  # grouped mode: whole tensor RMS, kernel error over model error
HD = 64  # attention head width
KEY_TILE = 64  # keys per step of the forward kernel's online softmax


def rbf(x):
    """Round to bf16 (nearest even) and return in the input's dtype."""
    return x.to(torch.bfloat16).to(x.dtype)


def ulp_bf16(x):
    """Spacing of bf16 numbers at |x| (float64 tensor); the subnormal spacing 2^-133 at and near 0."""
    ax = x.double().abs()
    _, e = torch.frexp(ax)  # ax = m * 2^e, m in [0.5, 1)
    e = torch.where(ax == 0, torch.full_like(e, -1000), e)
    return torch.exp2((e.double() - 8).clamp_min(-133.0))


# ------------------------------------------------------------------------------------------------
# the checker
class Budget(AssertionError):
    pass


def check_elementwise(got, ref64, r=0.0, a=0.0, extra=None, bf16=True, name="value"):
    """|got - ref64| <= (1/2 ulp_bf16(ref64) if bf16) + r |ref64| + a + extra, for every element. Returns the worst
    error / bound ratio."""
    ref64 = ref64.double()
    g = got.double()
    assert g.shape == ref64.shape, f"{name}: shape {tuple(g.shape)} != {tuple(ref64.shape)}"
    bound = r * ref64.abs() + a
    if bf16:
        bound = bound + 0.5 * ulp_bf16(ref64)
    if extra is not None:
        bound = bound + extra
    err = (g - ref64).abs()
    bad = ~(err <= bound)  # a NaN / inf in got is bad
    if bad.any():
        i = int(torch.where(bad.reshape(-1))[0][0])
        raise Budget(f"{name}: {int(bad.sum())} of {bad.numel()} elements over budget; first at flat index {i}: "
                     f"got {g.reshape(-1)[i].item():.9g} ref {ref64.reshape(-1)[i].item():.9g} "
                     f"bound {bound.reshape(-1)[i].item():.3g}")
    return float((err / bound).max()) if err.numel() else 0.0


def _rms(t):
    return float(t.double().pow(2).mean().sqrt()) if t.numel() else 0.0


def grouped_stats(got, model, ref64):
    """(per-row error, per-row budget base, rms(got - ref64), rms(model - ref64)) of grouped mode; rows are the last
    dimension."""
    ref64 = ref64.double()
    eg = (got.double() - ref64).abs().amax(-1)
    em = (model.double() - ref64).abs().amax(-1)
    floor = 0.5 * ulp_bf16(ref64.abs().amax(-1))
    return eg, torch.maximum(em, floor), _rms(got.double() - ref64), _rms(model.double() - ref64)


def check_grouped(got, model, ref64, name="value", fp32_extra=None):
    """Per row: max_j |got - ref64| <= 3 max(max_j |model - ref64|, 1/2 ulp_bf16(max_j |ref64|)); whole tensor:
    rms(got - ref64) <= 1.25 rms(model - ref64). Returns (worst row ratio, rms ratio).

    fp32_extra (elementwise, optional) is a bound on an fp32 step of the kernel whose rounding order the model cannot
    reproduce (see attention_cancellation_bound); its row maximum is added to the row budget, outside the margin, as
    `extra` is in elementwise mode. The RMS condition does not see it."""
    assert got.shape == ref64.shape == model.shape, f"{name}: shapes {tuple(got.shape)} {tuple(model.shape)}"
    eg, budget, rg, rm = grouped_stats(got, model, ref64)
    if fp32_extra is not None:
        eg = (eg - fp32_extra.double().amax(-1)).clamp_min(0.0)  # (a NaN error stays NaN)
    bad = ~(eg <= ROW_MARGIN * budget)
    row_ratio = float((eg / budget).max()) if eg.numel() else 0.0
    rms_ratio = rg / rm if rm > 0 else (0.0 if rg == 0 else math.inf)
    if bad.any():
        i = int(torch.where(bad.reshape(-1))[0][0])
        raise Budget(f"{name}: {int(bad.sum())} of {bad.numel()} rows over {ROW_MARGIN} x the model's error; first "
                     f"row {i}: error {eg.reshape(-1)[i].item():.4g}, budget base {budget.reshape(-1)[i].item():.4g} "
                     f"(worst ratio {row_ratio:.3g})")
    if not rg <= RMS_MARGIN * rm:
        raise Budget(f"{name}: rms error {rg:.4g} over {RMS_MARGIN} x the model's {rm:.4g} (ratio {rms_ratio:.4g})")
    return row_ratio, rms_ratio


# ------------------------------------------------------------------------------------------------
# attention: q, k, v, dout and the outputs are [B, S, H, 64]; LSE is [B, H, S]
def _scores(q, k):
    return torch.einsum("bqhd,bkhd->bhqk", q, k)


def _causal_mask(S, device):
    return torch.ones(S, S, dtype=torch.bool, device=device).tril()


def _attention_bwd(q, k, v, p, delta, dout, scale, rnd):
    dp = torch.einsum("bqhd,bkhd->bhqk", dout, v)
    ds = p * (dp - delta[..., None])
    dv = torch.einsum("bhqk,bqhd->bkhd", rnd(p), dout)
    dk = torch.einsum("bhqk,bqhd->bkhd", rnd(ds), q) * scale
    dq = torch.einsum("bhqk,bkhd->bqhd", rnd(ds), k) * scale
    return dq, dk, dv


def attention_ref64(q, k, v, scale, causal, dout=None):
    """float64 attention on the bf16 inputs: y, natural-log lse, p and (with dout) dq, dk, dv."""
    q, k, v = (t.double() for t in (q, k, v))
    s = _scores(q, k) * scale
    if causal:
        s = s.masked_fill(~_causal_mask(s.shape[-1], s.device), -math.inf)
    lse = torch.logsumexp(s, -1)
    p = torch.exp(s - lse[..., None])
    y = torch.einsum("bhqk,bkhd->bqhd", p, v)
    out = {"y": y, "lse": lse, "p": p}
    if dout is not None:
        d = dout.double()
        delta = (d * y).sum(-1).permute(0, 2, 1)
        out["dq"], out["dk"], out["dv"] = _attention_bwd(q, k, v, p, delta, d, scale, lambda t: t)
    return out


def _sl2(scale):
    # the kernel's `a.scale * LOG2E` in fp32
    return float(torch.tensor(scale, dtype=torch.float32) * torch.tensor(LOG2E, dtype=torch.float32))


def attention_model_direct(q, k, v, scale, causal):
    """fp32 model, whole rows at once: p = exp2(s c - max c) stays fp32 in the denominator and is rounded to bf16 for the
    PV product (pack8); y = bf16(o / l). Returns y (fp32 holding bf16 values) and the log2-domain lse the kernel saves."""
    q, k, v = (t.float() for t in (q, k, v))
    sl2 = _sl2(scale)
    s = _scores(q, k)
    if causal:
        s = s.masked_fill(~_causal_mask(s.shape[-1], s.device), -math.inf)
    m = s.amax(-1, keepdim=True) * sl2
    p = torch.exp2(s * sl2 - m)
    l = p.sum(-1)
    o = torch.einsum("bhqk,bkhd->bqhd", rbf(p), v)
    y = rbf(o * (1.0 / l).permute(0, 2, 1)[..., None])
    return {"y": y, "lse2": m[..., 0] + torch.log2(l)}


def attention_model_tiled(q, k, v, scale, causal, tile=KEY_TILE):
    """fp32 model as the forward kernel runs it: an online softmax over 64-key tiles; each tile's exp2(s c - running max)
    is summed in fp32 into l and rounded to bf16 for the PV product; o and l are rescaled by exp2(old max - new max)."""
    q, k, v = (t.float() for t in (q, k, v))
    B, S, H, D = q.shape
    sl2 = _sl2(scale)
    m = torch.full((B, H, S), -math.inf)
    l = torch.zeros(B, H, S)
    o = torch.zeros(B, H, S, D)
    qpos = torch.arange(S)[:, None]
    for k0 in range(0, S, tile):
        kt, vt = k[:, k0:k0 + tile], v[:, k0:k0 + tile]
        s = _scores(q, kt)
        if causal:
            s = s.masked_fill((torch.arange(k0, k0 + kt.shape[1])[None, :] > qpos), -math.inf)
        mx = torch.maximum(m, s.amax(-1) * sl2)
        alpha = torch.where(m == -math.inf, torch.zeros_like(m), torch.exp2(m - mx))
        msub = torch.where(mx == -math.inf, torch.zeros_like(mx), mx)
        p = torch.exp2(s * sl2 - msub[..., None])
        l = l * alpha + p.sum(-1)
        o = o * alpha[..., None] + torch.einsum("bhqk,bkhd->bhqd", rbf(p), vt)
        m = mx
    y = rbf(o * (1.0 / l)[..., None]).permute(0, 2, 1, 3)
    return {"y": y, "lse2": m + torch.log2(l)}


def _delta_fp32(dout, y):
    """delta = rowsum(dO * O) in the dQ kernel's order: each lane half h chains d = 16 t + 8 h + j (t, then j) with fmaf
    (the bf16 x bf16 products are exact in fp32), then the two halves are added."""
    B, S, H, D = dout.shape
    pr = (dout.float() * y.float()).view(B, S, H, 4, 2, 8)
    acc = torch.zeros(B, S, H, 2)
    for t in range(4):
        for j in range(8):
            acc = acc + pr[..., t, :, j]
    return (acc[..., 0] + acc[..., 1]).permute(0, 2, 1)


def attention_model_bwd(q, k, v, y, lse2, dout, scale, causal):
    """fp32 backward model: P = exp2(s c - lse) is recomputed, P and dS = P (dP - delta) are rounded to bf16 before the
    dV and dK / dQ products (pack8), the outputs once more.

    y and the log2-domain lse are INPUTS of the backward kernels (the forward saves them), so the model of a backward
    run takes the y that run was given: delta = rowsum(dO * y) carries y's bf16 rounding, a sum of 64 terms of which a
    single flipped rounding moves a sharp-softmax row of dq by more than the row margin (two forward models feeding
    their own y into this function differ by 3.4 x on one row of S = 200, inputs scaled by 6). The forward's error is
    budgeted where y is checked."""
    q, k, v, d = (t.float() for t in (q, k, v, dout))
    sl2 = _sl2(scale)
    p = torch.exp2(_scores(q, k) * sl2 - lse2[..., None])
    if causal:
        p = p.masked_fill(~_causal_mask(p.shape[-1], p.device), 0.0)
    dq, dk, dv = _attention_bwd(q, k, v, p, _delta_fp32(dout, y), d, scale, rbf)
    return {"dq": rbf(dq), "dk": rbf(dk), "dv": rbf(dv)}


def attention_cancellation_bound(q, k, v, y, dout, p64, scale):
    """Elementwise fp32 bounds {"dq", "dk"} for the one step of the backward that the model cannot reproduce.

    dS = P (dP - delta) subtracts two fp32 sums of the same 64 exact bf16 x bf16 products kind: dP = dO . V is
    accumulated by four chained MFMAs (their inner order is not specified), delta = dO . O by an fmaf chain per lane
    half. Where the true difference is zero or tiny (the first causal query, whose only key gives O = V and dS = 0
    exactly; any query of a one-hot softmax) what is left is the two sums' rounding, about 1e-8 in dq where float64
    has 0, and two honest fp32 evaluations differ there by any factor. Each sum is bounded in any order by
    64 * 2^-24 * sum|terms|; that bound on dS, times P, goes through the dQ / dK products with |K| / |Q|."""
    q, k, v, y, d = (t.double().abs() for t in (q, k, v, y, dout))
    a = torch.einsum("bqhd,bkhd->bhqk", d, v) + (d * y).sum(-1).permute(0, 2, 1)[..., None]
    eds = p64 * (HD * U32) * a
    return {"dq": torch.einsum("bhqk,bkhd->bqhd", eds, k) * scale, "dk": torch.einsum("bhqk,bqhd->bkhd", eds, q) * scale}


def attention_model(q, k, v, scale, causal, dout=None, tiled=True):
    fwd = (attention_model_tiled if tiled else attention_model_direct)(q, k, v, scale, causal)
    fwd["lse"] = fwd["lse2"].double() * LN2
    if dout is not None:
        fwd.update(attention_model_bwd(q, k, v, fwd["y"], fwd["lse2"], dout, scale, causal))
    return fwd


def lse_bound(ref_lse64, n_keys):
    """fp32 bound on the natural-log LSE: the denominator is a sum of n fp32 terms (relative n 2^-24 in any order, an
    absolute error of the same size in its logarithm), the exponent arguments and max + log2(l) carry a few roundings
    of |lse| log2(e), and v_exp_f32 / v_log_f32 one ulp each."""
    return (n_keys + 8) * U32 + 8 * U32 * ref_lse64.abs() * LOG2E


# ------------------------------------------------------------------------------------------------
# vocabulary cross-entropy
def cross_entropy_ref64(logits, target, scale, ignore_index=-100):
    """float64 rows of loss, correct (first maximal index, as torch.argmax), dlogits = scale (softmax - onehot); ignored
    rows (target == ignore_index or outside [0, V)) give 0, 0 and a zero gradient row."""
    z = logits.double()
    V = z.shape[1]
    valid = (target != ignore_index) & (target >= 0) & (target < V)
    t = torch.where(valid, target, torch.zeros_like(target))
    lse = torch.logsumexp(z, 1)
    onehot = torch.zeros_like(z)
    onehot[torch.arange(z.shape[0], device=z.device), t] = 1.0
    g = scale * (torch.exp(z - lse[:, None]) - onehot) * valid[:, None]
    loss = (lse - z.gather(1, t[:, None])[:, 0]) * valid
    correct = (valid & (z.argmax(1) == t)).double()
    return {"loss": loss, "correct": correct, "dlogits": g, "lse": lse, "count": int(valid.sum())}


def cross_entropy_model(logits, target, scale, ignore_index=-100):
    """fp32 model of the kernels: lse = max + log(sum exp(z - max)), dlogits = bf16(scale (exp(z - lse) - onehot))."""
    z = logits.float()
    V = z.shape[1]
    valid = (target != ignore_index) & (target >= 0) & (target < V)
    t = torch.where(valid, target, torch.zeros_like(target))
    m = z.amax(1, keepdim=True)
    lse = m[:, 0] + torch.log(torch.exp(z - m).sum(1))
    onehot = torch.zeros_like(z)
    onehot[torch.arange(z.shape[0]), t] = 1.0
    sc = torch.where(valid, torch.tensor(float(scale)), torch.tensor(0.0))[:, None]
    return {"dlogits": rbf(sc * (torch.exp(z - lse[:, None]) - onehot)), "loss": (lse - z.gather(1, t[:, None])[:, 0]) * valid}


DLOGITS_R = 2.0 ** -14  # z - lse in fp32 with |lse| <= 128: <= 4 * 2^-23 * 128 of argument error = relative 2^-14 in exp


def dlogits_budget(scale):
    return {"r": DLOGITS_R, "a": 2.0 ** -22 * abs(scale) + 2.0 ** -126}


def check_dlogits(got, ref64, scale, name="dlogits"):
    return check_elementwise(got, ref64, bf16=True, name=name, **dlogits_budget(scale))


def loss_bound(ref):
    """fp32 bound on a row's loss = lse - z[target]: sum-exp of V fp32 terms (relative V 2^-24 in any order, so that
    much absolute error in its logarithm), the exponentials' 2^-14 relative error (DLOGITS_R), and a few roundings of
    |lse| and |loss|."""
    V = ref["dlogits"].shape[1]
    return (V + 8) * U32 + DLOGITS_R + 8 * U32 * (ref["lse"].abs() + ref["loss"].abs())


# ------------------------------------------------------------------------------------------------
# LayerNorm (x [rows, D]); the fused residual add rounds x + h to bf16 first
def residual_add(x, h):
    """bf16(x + h) as the fused kernel and the unfused bf16 add compute it (one fp32 add, one rounding)."""
    return (x.float() + h.float()).to(torch.bfloat16)


def layernorm_ref64(x, w, b, eps):
    x, w, b = (t.double() for t in (x, w, b))
    mean = x.mean(-1)
    var = (x - mean[..., None]).pow(2).mean(-1)
    rstd = (var + eps).rsqrt()
    return {"y": (x - mean[..., None]) * rstd[..., None] * w + b, "mean": mean, "rstd": rstd, "var": var}


def add_layernorm_ref64(x, h, w, b, eps):
    xs = residual_add(x, h)
    out = layernorm_ref64(xs, w, b, eps)
    out["xs"] = xs
    return out


def _ln_bwd(x, w, gy, mean, rstd, gadd, drop_xhat_term=False):
    xh = (x - mean[..., None]) * rstd[..., None]
    gw = gy * w
    s1 = gw.mean(-1, keepdim=True)
    s2 = (gw * xh).mean(-1, keepdim=True)
    dx = rstd[..., None] * (gw - s1 - (0 if drop_xhat_term else xh * s2))
    if gadd is not None:
        dx = dx + gadd
    return dx, (gy * xh).reshape(-1, x.shape[-1]).sum(0), gy.reshape(-1, x.shape[-1]).sum(0)


def layernorm_bwd_ref64(x, w, gy, eps, gadd=None):
    f = layernorm_ref64(x, w, torch.zeros_like(w), eps)
    dx, dw, db = _ln_bwd(x.double(), w.double(), gy.double(), f["mean"], f["rstd"],
                         None if gadd is None else gadd.double())
    return {"dx": dx, "dw": dw, "db": db}


def layernorm_model(x, w, b, eps):
    """fp32 model: two-pass statistics, y = bf16((x - mean) rstd w + b)."""
    x, w, b = (t.float() for t in (x, w, b))
    mean = x.mean(-1)
    var = (x - mean[..., None]).pow(2).mean(-1)
    rstd = (var + eps).rsqrt()
    return {"y": rbf((x - mean[..., None]) * rstd[..., None] * w + b), "mean": mean, "rstd": rstd}


def layernorm_bwd_model(x, w, gy, eps, gadd=None, drop_xhat_term=False):
    """fp32 model: dx = bf16(rstd (g w - mean(g w) - xhat mean(g w xhat)) + gadd), one rounding; dw, db fp32 sums."""
    f = layernorm_model(x, w, torch.zeros_like(w), eps)
    dx, dw, db = _ln_bwd(x.float(), w.float(), gy.float(), f["mean"], f["rstd"],
                         None if gadd is None else gadd.float(), drop_xhat_term)
    return {"dx": rbf(dx), "dw": dw, "db": db}


def layernorm_fp32_bounds(x, w, gy, eps):
    """Absolute fp32 bounds for mean, rstd, dw and db, derived from the kernel's arithmetic (x [rows, D] bf16):
    mean: a sum of D fp32 terms (D 2^-24 sum|x| in any order) and one division;
    rstd: the variance is summed about the computed mean (shift e_mu^2, D 2^-24 relative summation error), then the
          division, the + eps (eps itself cast to fp32) and v_rsq_f32 at about one rounding each;
    dw:   every term g xhat inherits xhat's error rstd e_mu + |xhat| (e_rstd / rstd + 2^-23), and the rows' terms are
          summed in fp32 (rows 2^-24 sum|g xhat|);  db: rows 2^-24 sum|g|."""
    x, w, g = (t.double().reshape(-1, t.shape[-1]) for t in (x, w.expand_as(x), gy if gy is not None else x))
    rows, D = x.shape
    f = layernorm_ref64(x, w[0], torch.zeros_like(w[0]), eps)
    e_mu = D * U32 * x.abs().mean(-1) + U32 * f["mean"].abs()
    rel_rs = 0.5 * (D * U32 + e_mu.pow(2) / (f["var"] + eps)) + 4 * U32
    out = {"mean": e_mu, "rstd": f["rstd"] * rel_rs}
    if gy is not None:
        xh = (x - f["mean"][:, None]) * f["rstd"][:, None]
        e_xh = (f["rstd"] * e_mu)[:, None] + xh.abs() * (rel_rs[:, None] + 2 * U32)
        out["dw"] = (g.abs() * e_xh).sum(0) + rows * U32 * (g * xh).abs().sum(0)
        out["db"] = rows * U32 * g.abs().sum(0)
    return out


# ------------------------------------------------------------------------------------------------
# column sums (bias gradient)
def colsum_ref64(gy):
    return gy.double().reshape(-1, gy.shape[-1]).sum(0)


def colsum_bound(gy):
    """Recursive-summation bound for a column of M fp32 terms, valid in any order: M 2^-24 sum|term|."""
    g = gy.double().reshape(-1, gy.shape[-1])
    return g.shape[0] * U32 * g.abs().sum(0)
