"""fp64 references, fp32 rounding models and derived error bounds for the bf16 ResNet-18 kernels (conv_bf16.hip,
batchnorm_nhwc.hip, head_pool.hip). Plain torch, runs on the CPU. The checker (check_elementwise, check_grouped,
ulp_bf16, U32 and the margins 3 and 1.25) is tests/gpt2_numerics.py's, unchanged; docs/NUMERICS.md ("ResNet-18") has
the rounding points and the derivation of every bound below.

Activations are logical [N, C, H, W] tensors (any memory format), weights torch's [Co, C, k, k]."""
import torch
import torch.nn.functional as F

import gpt2_numerics as gn
from gpt2_numerics import U32, rbf  # noqa: F401

BF = torch.bfloat16
CONV_TILE = 256  # pixels per convolution tile (conv_bf16.hip BM): the rows behind one epilogue partial


def fma32(a, b, c):
    """fmaf(a, b, c) on fp32 tensors: the product of two fp32 numbers is exact in float64; one rounding to fp32 (the
    float64 rounding of the sum in between is 2^29 times finer)."""
    return (a.double() * b.double() + c.double()).float()


# ------------------------------------------------------------------------------------------------
# convolution. Every output element is one fp32 accumulation (products of bf16 numbers are exact in fp32) rounded once:
# elementwise mode with extra = (K + 8) 2^-24 (the same operation on |inputs|), K = number of summed products.
def conv_fwd_ref64(x, w, stride=1, pad=1, add=None):
    """(ref64, extra) of y = conv(x, w) (+ add): K = ks^2 C products per output."""
    K = w.shape[1] * w.shape[2] * w.shape[3]
    ref = F.conv2d(x.double(), w.double(), stride=stride, padding=pad)
    mag = F.conv2d(x.double().abs(), w.double().abs(), stride=stride, padding=pad)
    if add is not None:  # y = bf16(acc + add): one more fp32 addition, |add| joins the magnitude
        ref, mag = ref + add.double(), mag + add.double().abs()
    return ref, (K + 8) * U32 * mag


def conv_dgrad_ref64(x_shape, w, dy, stride=1, pad=1, add=None):
    """(ref64, extra) of dx = conv_transpose(dy, w) (+ add): at most ks^2 Co products per element."""
    K = w.shape[0] * w.shape[2] * w.shape[3]
    ref = torch.nn.grad.conv2d_input(x_shape, w.double(), dy.double(), stride=stride, padding=pad)
    mag = torch.nn.grad.conv2d_input(x_shape, w.double().abs(), dy.double().abs(), stride=stride, padding=pad)
    if add is not None:
        ref, mag = ref + add.double(), mag + add.double().abs()
    return ref, (K + 8) * U32 * mag


def wgrad_splits_max(pixels, per_split=512):
    """Upper bound on the fp32 partial results a weight gradient adds: conv_bf16.hip splits the pixel range so that
    every workgroup keeps >= 8 K-steps of 64 pixels (wgrad_splits); the stem kernel takes >= 64 pixels per block."""
    return max(1, pixels // per_split)


def conv_wgrad_ref64(x, w_shape, dy, stride=1, pad=1, old=None, per_split=512):
    """(ref64, extra, r) of gw = old + dW: K = output pixels + the number of split partials; accumulating into an
    existing bf16 gradient adds |old| to the magnitude and r = 2 * 2^-24 (as linear_decode's bias and the column sums)."""
    pixels = dy.shape[0] * dy.shape[2] * dy.shape[3]
    K = pixels + wgrad_splits_max(pixels, per_split)
    ref = torch.nn.grad.conv2d_weight(x.double(), w_shape, dy.double(), stride=stride, padding=pad)
    mag = torch.nn.grad.conv2d_weight(x.double().abs(), w_shape, dy.double().abs(), stride=stride, padding=pad)
    r = 0.0
    if old is not None:
        ref, mag, r = ref + old.double(), mag + old.double().abs(), 2 * U32
    return ref, (K + 8) * U32 * mag, r


def check_conv(got, ref, extra, r=0.0, name="conv"):
    return gn.check_elementwise(got, ref, r=r, extra=extra, bf16=True, name=name)


# 4096 distinct bf16 values (2 signs x 16 exponents x 128 significands, |v| in [2^-8, 2^8)): every product of two of
# them has up to 16 significant bits, so bf16(x * w) exercises the final rounding
_TABLE = None


def distinct_table():
    global _TABLE
    if _TABLE is None:
        m = 1.0 + torch.arange(128).double() / 128
        e = torch.exp2(torch.arange(-8, 8).double())
        v = (e[:, None] * m[None, :]).reshape(-1)
        _TABLE = torch.cat([v, -v]).to(BF)
        assert _TABLE.unique().numel() == 4096
    return _TABLE


def distinct_weights(Co, C, ks, fixed_axis, seed=0):
    """[Co, C, ks, ks] bf16 weights whose values are all distinct within every slice of constant `fixed_axis` (1: an
    input channel, what a forward impulse meets; 0: an output channel, what an input-gradient impulse meets)."""
    g = torch.Generator().manual_seed(seed)
    nfix, nfree = (C, Co) if fixed_axis == 1 else (Co, C)
    assert nfree * ks * ks <= 4096
    idx = torch.rand(nfix, 4096, generator=g).argsort(1)[:, :nfree * ks * ks]
    w = distinct_table()[idx].view(nfix, nfree, ks, ks)
    return w.transpose(0, 1).contiguous() if fixed_axis == 1 else w.contiguous()


def distinct_values(*shape, seed=0):
    """bf16 tensor of independent draws from the table of 4096 distinct values."""
    g = torch.Generator().manual_seed(seed)
    return distinct_table()[torch.randint(0, 4096, shape, generator=g)]


def impulse(shape, pixel, channel, value=1.3984375):
    """[N, C, H, W] bf16 zeros with `value` at flattened pixel index `pixel` of [N H W] and at `channel`."""
    N, C, H, W = shape
    x = torch.zeros(N, H, W, C, dtype=BF)
    x.view(N * H * W, C)[pixel, channel] = value
    return x.permute(0, 3, 1, 2)


# ------------------------------------------------------------------------------------------------
# BatchNorm, training mode. x [N, C, H, W] is viewed as [M, C].
def rows(t):
    """[N, C, H, W] -> [M, C]"""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def bn_blocks(M):
    """batchnorm_nhwc.hip bn_blocks: (partial rows, pixel rows per partial)."""
    blocks = min(512, max(1, M // 64))
    rpb = (M + blocks - 1) // blocks
    return (M + rpb - 1) // rpb, rpb


def bn_partial_terms(M, C, from_conv=False):
    """Additions an element passes through on its way into one fp32 partial. BatchNorm's own pass: a block's
    rpb rows go round-robin to lanes = 256 / (C / 8) row lanes (ceil(rpb / lanes) additions in a lane's register), then
    the lanes are added in order (lanes additions). Convolution-epilogue partials: one 256-pixel tile, at most 256."""
    if from_conv:
        return CONV_TILE
    _, rpb = bn_blocks(M)
    lanes = 256 // (C // 8)
    return min(rpb, -(-rpb // lanes) + lanes)  # (idle lanes add zeros, which is exact: never more than rpb)


def bn_stats_ref64(x, eps):
    xr = rows(x).double()
    mean = xr.mean(0)
    var = (xr - mean).pow(2).mean(0)  # two-pass in float64: no cancellation
    return {"mean": mean, "var": var, "rstd": (var + eps).rsqrt(), "ex2": xr.pow(2).mean(0), "eabs": xr.abs().mean(0)}


def bn_stats_bounds(x, eps, terms):
    """Absolute bounds on the kernel's mean, variance and rstd (per channel). The kernel sums x and x^2 (exact
    products) into fp32 partials of `terms` additions each (relative terms 2^-24 of sum|.| in any order), adds the
    partials and finalises in float64: mean = S1 / M, var = max(S2 / M - mean^2, 0): the variance inherits
    e(E[x^2]) + 2 |mean| e(mean) + e(mean)^2, which is a cancellation error relative to var + eps. rstd =
    (float)(1 / sqrt(var + (double)eps)) is bounded through the exact function at var +- e_var (the linearisation fails
    for a constant channel), plus the cast of eps to fp32 and of the result (2 * 2^-24)."""
    s = bn_stats_ref64(x, eps)
    e_mu = terms * U32 * s["eabs"]
    e_var = terms * U32 * s["ex2"] + 2 * s["mean"].abs() * e_mu + e_mu.pow(2)
    lo = (s["var"] + e_var + eps).rsqrt()
    hi = ((s["var"] - e_var).clamp_min(0.0) + eps).rsqrt()
    e_rstd = torch.maximum(hi - s["rstd"], s["rstd"] - lo) + 2 * U32 * s["rstd"]
    return {"mean": e_mu + U32 * s["mean"].abs(), "var": e_var, "rstd": e_rstd, "mean_sum": e_mu}


def bn_running_ref64(x, eps, momentum, rmean0, rvar0, terms, unbiased=True):
    """References and elementwise `extra` of the running statistics: bf16((1 - m) old + m new) in fp32 (three roundings,
    4 * 2^-24 of the two terms' magnitudes with the fp32 cast of m), new = mean, and var M / (M - 1) for M > 1."""
    s, b = bn_stats_ref64(x, eps), bn_stats_bounds(x, eps, terms)
    M = rows(x).shape[0]
    f = M / (M - 1) if (M > 1 and unbiased) else 1.0
    m = float(momentum)
    rm = (1 - m) * rmean0.double() + m * s["mean"]
    rv = (1 - m) * rvar0.double() + m * s["var"] * f
    e_rm = 4 * U32 * ((1 - m) * rmean0.double().abs() + m * s["mean"].abs()) + m * b["mean"]
    e_rv = 4 * U32 * ((1 - m) * rvar0.double().abs() + m * s["var"] * f) + m * b["var"] * f
    return {"running_mean": rm, "running_var": rv, "e_running_mean": e_rm, "e_running_var": e_rv}


def _apply(x, scale, shift, res, relu, fma):
    xr = rows(x)
    v = fma(xr, scale, shift)
    if res is not None:
        v = v + rows(res).to(v.dtype)
    return torch.relu(v) if relu else v


def bn_fwd_ref64(x, gamma, beta, eps, res=None, relu=False):
    """float64 y [M, C] of relu?((x - mean) rstd gamma + beta (+ res))."""
    s = bn_stats_ref64(x, eps)
    scale = gamma.double() * s["rstd"]
    return _apply(x.double(), scale, beta.double() - s["mean"] * scale, None if res is None else res.double(), relu,
                  lambda a, b, c: a * b + c)


def bn_fold32(mean32, rstd32, gamma, beta):
    """The kernels' folded fp32 coefficients: scale = gamma * rstd, shift = fmaf(-mean, scale, beta)."""
    scale = gamma.float() * rstd32
    return scale, fma32(-mean32, scale, beta.float())


def bn_apply_model(x, scale, shift, res=None, relu=False):
    """fp32 model of bn_apply_kernel: y = bf16(relu?(fmaf(x, scale, shift) (+ res))), [M, C]."""
    return rbf(_apply(x.float(), scale, shift, None if res is None else res.float(), relu, fma32))


def eps32(eps):
    """eps as the kernels receive it: cast to fp32 (at var = 0 its last bits decide the rounding of rstd)."""
    return float(torch.tensor(eps, dtype=torch.float32))


def bn_stats32(x, eps):
    """The float64 statistics rounded to fp32 where the kernel rounds them: mean = (float)mu,
    rstd = (float)(1 / sqrt(var + (double)(float)eps))."""
    s = bn_stats_ref64(x, eps)
    return s["mean"].float(), (1.0 / torch.sqrt(s["var"] + eps32(eps))).float()


def bn_fwd_model(x, gamma, beta, eps, res=None, relu=False):
    """Training forward: the float64 statistics rounded to fp32 where the kernel rounds them, then the apply model."""
    return bn_apply_model(x, *bn_fold32(*bn_stats32(x, eps), gamma, beta), res, relu)


def bn_y_extra(x, gamma, eps, terms):
    """Elementwise fp32 bound [M, C] on what the statistics' summation error moves y by (the model holds the float64
    statistics): |x - mean| gamma e_rstd + gamma rstd e_mean."""
    s, b = bn_stats_ref64(x, eps), bn_stats_bounds(x, eps, terms)
    g = gamma.double().abs()
    return (rows(x).double() - s["mean"]).abs() * g * b["rstd"] + g * s["rstd"] * b["mean"]


def bn_eval_ref64(x, gamma, beta, rmean, rvar, eps, res=None, relu=False):
    scale = gamma.double() * (rvar.double() + eps).rsqrt()
    return _apply(x.double(), scale, beta.double() - rmean.double() * scale, None if res is None else res.double(),
                  relu, lambda a, b, c: a * b + c)


def bn_eval_model(x, gamma, beta, rmean, rvar, eps, res=None, relu=False):
    """ops/conv.py's eval coefficients (fp32 torch ops: no fma) and the apply model."""
    scale = gamma.float() * torch.rsqrt(rvar.float() + eps)
    return bn_apply_model(x, scale, beta.float() - rmean.float() * scale, res, relu)


def relu_mask(y):
    """[M, C] bool mask of the backward, from the output y the backward was given (None: no ReLU)."""
    return None if y is None else rows(y).float() > 0


def bn_bwd_ref64(x, dy, gamma, eps, mask=None, gg0=None, gb0=None):
    """float64 backward on [M, C]: g = dy * mask, dbeta = old + sum g, dgamma = old + sum g xhat,
    dx = gamma rstd (g - mean(g) - xhat mean(g xhat)), dres = g."""
    s = bn_stats_ref64(x, eps)
    g = rows(dy).double()
    if mask is not None:
        g = g * mask
    xh = (rows(x).double() - s["mean"]) * s["rstd"]
    sg, sgx = g.sum(0), (g * xh).sum(0)
    M = g.shape[0]
    dx = gamma.double() * s["rstd"] * (g - sg / M - xh * (sgx / M))
    return {"dx": dx, "dres": g, "dgamma": sgx + (0 if gg0 is None else gg0.double()),
            "dbeta": sg + (0 if gb0 is None else gb0.double()), "g": g, "xhat": xh}


def bn_bwd_model(x, dy, gamma, eps, mask=None, drop=None):
    """fp32 model of bn_bwd_apply_kernel with the kernel's folded coefficients (float64 sums rounded to fp32 where the
    kernel rounds): a = gamma * rstd, mg = (float)(sum g / M), b = -a * rstd * (float)(sum(g xhat) / M),
    dx = bf16(fmaf(a, g - mg, b * (x - mean))). drop = "xhat" / "mean" seeds the two defects."""
    mean32, rstd32 = bn_stats32(x, eps)
    g = rows(dy).float()
    if mask is not None:
        g = g * mask
    xr = rows(x).float()
    M = g.shape[0]
    xh = (xr.double() - mean32.double()) * rstd32.double()
    a = gamma.float() * rstd32
    mg = (g.double().sum(0) / M).float()
    b = -a * rstd32 * ((g.double() * xh).sum(0) / M).float()
    if drop == "xhat":
        b = torch.zeros_like(b)
    if drop == "mean":
        mg = torch.zeros_like(mg)
    return rbf(fma32(a, g - mg, b * (xr - mean32)))


def bn_bwd_bounds(x, dy, gamma, eps, mask, terms_fwd, terms_bwd, accumulate=True):
    """Elementwise extras for dgamma / dbeta ([C]) and the fp32 extra of dx ([M, C]), as LayerNorm's dW / db bounds:
    every term g xhat inherits xhat's error e_xhat = rstd e_mean + |xhat| (e_rstd / rstd + 3 * 2^-24) from the forward's
    saved fp32 statistics (bounds of bn_stats_bounds with the forward's terms per partial) and the fp32 subtraction
    and two products; the sums are fp32 partials of terms_bwd additions. dx moves by the errors of its four
    per-channel coefficients."""
    s, b = bn_stats_ref64(x, eps), bn_stats_bounds(x, eps, terms_fwd)
    ref = bn_bwd_ref64(x, dy, gamma, eps, mask)
    g, xh = ref["g"].abs(), ref["xhat"].abs()
    M = g.shape[0]
    rel_rs = b["rstd"] / s["rstd"]
    e_xh = s["rstd"] * b["mean"] + xh * (rel_rs + 3 * U32)
    e_sg = terms_bwd * U32 * g.sum(0)
    e_sgx = (g * e_xh).sum(0) + terms_bwd * U32 * (g * xh).sum(0)
    a = gamma.double().abs() * s["rstd"]
    mgx = (ref["g"] * ref["xhat"]).mean(0).abs()
    xc = (rows(x).double() - s["mean"]).abs()
    t1 = a * (ref["g"] - ref["g"].mean(0)).abs()
    t2 = a * s["rstd"] * mgx * xc
    e_dx = a * (e_sg / M) + a * s["rstd"] * xc * (e_sgx / M) + a * s["rstd"] * mgx * b["mean"] + rel_rs * (t1 + 2 * t2)
    # each coefficient (a, mg, b and the saved mean) is an fp32 rounding of a value inside its bound: two such roundings
    # are up to 2^-23 of the coefficient apart on top of the bound
    e_dx = e_dx + 2 * U32 * (2 * t1 + 2 * t2 + a * ref["g"].mean(0).abs() + a * s["rstd"] * mgx * s["mean"].abs())
    return {"dgamma": e_sgx, "dbeta": e_sg, "dx": e_dx, "r": 2 * U32 if accumulate else 0.0}


# ------------------------------------------------------------------------------------------------
# pooled head: x [N, K, H, W] (P = H W positions), w [ncls, K], b [ncls], labels t [N]
EXP_A = 2.0 ** -14  # __expf / __logf, taken as the cross-entropy rows of docs/NUMERICS.md take them


def head_ref64(x, w, b, t, scale, gw0=None, gb0=None, stats0=None):
    N, K = x.shape[0], x.shape[1]
    ncls = w.shape[0]
    xp = x.double().permute(0, 2, 3, 1).reshape(N, -1, K)
    P = xp.shape[1]
    feats = xp.mean(1)
    z = feats @ w.double().t() + b.double()
    valid = (t >= 0) & (t < ncls)
    tt = torch.where(valid, t, torch.zeros_like(t))
    lse = torch.logsumexp(z, 1)
    onehot = torch.zeros_like(z)
    onehot[torch.arange(N), tt] = 1.0
    p = torch.exp(z - lse[:, None])
    dl = scale * (p - onehot) * valid[:, None]
    loss = (lse - z.gather(1, tt[:, None])[:, 0]) * valid
    correct = (valid & (z.argmax(1) == tt)).double()  # torch.argmax: the first maximal index
    dfeat = dl @ w.double()
    out = {"feats": feats, "z": z, "lse": lse, "p": p, "dl": dl, "loss": loss, "correct": correct, "valid": valid,
           "dx": (dfeat / P)[:, None, :].expand(N, P, K), "gw": dl.t() @ feats, "gb": dl.sum(0),
           "stats": torch.stack([loss.sum(), correct.sum()]), "P": P}
    if gw0 is not None:
        out["gw"], out["gb"] = out["gw"] + gw0.double(), out["gb"] + gb0.double()
    if stats0 is not None:
        out["stats"] = out["stats"] + stats0.double()
    return out


def head_bounds(x, w, b, scale, ref, gw0=None, gb0=None, stats0=None):
    """Elementwise extras from the kernel's fp32 sums (any order: n 2^-24 sum|terms|, n = terms + 8):
    feats  P terms and the product with (float)(1 / P);
    z      K terms f w (+ b), every term carrying e_feats |w|;
    loss   lse = max + log(sum exp(z - max)): 2^-14 for __expf / __logf, (ncls + 8) 2^-24 for the sum,
           8 * 2^-24 (|lse| + |loss|), and z's error twice (in lse and in z[target]);
    dl     scale (exp(z - lse) - onehot): p (2^-14 + 2 max e_z) + 2^-22, times |scale|;
    dx     ncls terms dl w, then / P;   gW  N terms dl feats (+ old);   gb  N terms dl (+ old);
    stats  N row losses (+ old): the rows' bounds and (N + 8) 2^-24 sum|loss|; the count of correct rows is exact."""
    N, K = x.shape[0], x.shape[1]
    ncls, P = w.shape[0], ref["P"]
    xa = x.double().abs().permute(0, 2, 3, 1).reshape(N, -1, K)
    wa, ba = w.double().abs(), b.double().abs()
    e_f = (P + 8) * U32 * xa.mean(1)
    fa = ref["feats"].abs()
    e_z = e_f @ wa.t() + (K + 8) * U32 * (fa @ wa.t() + ba)
    ez_max = e_z.amax(1)
    e_loss = (EXP_A + (ncls + 8) * U32 + 8 * U32 * (ref["lse"].abs() + ref["loss"].abs()) + 2 * ez_max) * ref["valid"]
    e_dl = abs(scale) * (ref["p"] * (EXP_A + 2 * ez_max[:, None]) + 2.0 ** -22) * ref["valid"][:, None]
    dla = ref["dl"].abs()
    e_dx = (e_dl @ wa + (ncls + 8) * U32 * (dla @ wa)) / P
    e_gw = e_dl.t() @ fa + dla.t() @ e_f + (N + 8) * U32 * (dla.t() @ fa)
    e_gb = e_dl.sum(0) + (N + 8) * U32 * dla.sum(0)
    e_st = e_loss.sum() + (N + 8) * U32 * ref["loss"].abs().sum()
    if gw0 is not None:
        e_gw, e_gb = e_gw + 2 * U32 * gw0.double().abs(), e_gb + 2 * U32 * gb0.double().abs()
    if stats0 is not None:
        e_st = e_st + 2 * U32 * stats0.double().abs()[0]
    return {"dx": e_dx[:, None, :].expand(N, P, K), "gw": e_gw, "gb": e_gb, "loss_sum": e_st, "r": 2 * U32}


def head_fp32(x, w, b, t, scale, drop_tail=False):
    """An honest fp32 implementation in plain torch (drop_tail seeds the defect: the positions past the last multiple of
    8 are left out of the pool's sum). Returns dx [N, P, K], gw, gb, stats in fp32."""
    N, K = x.shape[0], x.shape[1]
    ncls = w.shape[0]
    xp = x.float().permute(0, 2, 3, 1).reshape(N, -1, K)
    P = xp.shape[1]
    feats = (xp[:, :P - P % 8] if drop_tail else xp).sum(1) * torch.tensor(1.0 / P)
    z = feats @ w.float().t() + b.float()
    valid = (t >= 0) & (t < ncls)
    tt = torch.where(valid, t, torch.zeros_like(t))
    mx = z.amax(1, keepdim=True)
    lse = mx[:, 0] + torch.log(torch.exp(z - mx).sum(1))
    onehot = torch.zeros_like(z)
    onehot[torch.arange(N), tt] = 1.0
    dl = torch.tensor(float(scale)) * (torch.exp(z - lse[:, None]) - onehot) * valid[:, None]
    loss = (lse - z.gather(1, tt[:, None])[:, 0]) * valid
    correct = (valid & (z.argmax(1) == tt)).float()
    dx = ((dl @ w.float()) * torch.tensor(1.0 / P))[:, None, :].expand(N, P, K)
    return {"dx": dx, "gw": dl.t() @ feats, "gb": dl.sum(0), "stats": torch.stack([loss.sum(), correct.sum()])}


def check_head(got, ref, bounds, bf16, name="head"):
    """got: dx [N, P, K], gw, gb (already old + new) and stats [2]. Returns the worst ratios."""
    out = {}
    # (a = the smallest fp32 subnormal: an ignored row's zeros against a zero bound then give the ratio 0, not 0 / 0)
    out["dx"] = gn.check_elementwise(got["dx"], ref["dx"], a=2.0 ** -149, extra=bounds["dx"], bf16=bf16, name=f"{name} dx")
    out["gw"] = gn.check_elementwise(got["gw"], ref["gw"], r=bounds["r"], extra=bounds["gw"], bf16=bf16, name=f"{name} gW")
    out["gb"] = gn.check_elementwise(got["gb"], ref["gb"], r=bounds["r"], extra=bounds["gb"], bf16=bf16, name=f"{name} gb")
    out["loss"] = gn.check_elementwise(got["stats"][0], ref["stats"][0], r=bounds["r"], extra=bounds["loss_sum"],
                                       bf16=False, name=f"{name} loss sum")
    assert float(got["stats"][1]) == float(ref["stats"][1]), f"{name}: correct {float(got['stats'][1])} != " \
                                                              f"{float(ref['stats'][1])}"
    return out


# ------------------------------------------------------------------------------------------------
# input families shared by the CPU self-test and the GPU tests
BN_FAMILIES = ["uniform", "offset", "constant", "sparse"]
HEAD_SHAPES = [(5, 520, 9, 10), (7, 1024, 17, 11), (4, 64, 49, 3), (1, 8, 1, 1), (130, 256, 6, 16)]  # (N, K, P, ncls)


def conv_inputs(family, N, C, Co, H, W, ks=3, seed=0, stride=1):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, C, H, W, generator=g)
    w = torch.randn(Co, C, ks, ks, generator=g) * 0.05
    OH, OW = (H + 2 * (ks // 2) - ks) // stride + 1, (W + 2 * (ks // 2) - ks) // stride + 1
    dy = torch.randn(N, Co, OH, OW, generator=g)
    if family == "positive":
        x, w, dy = x.abs(), w.abs(), dy.abs()
    return x.to(BF), w.to(BF), dy.to(BF)


def bn_inputs(family, N, C, H, W, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(N, C, H, W, generator=g) * 4 - 1.5
    if family == "offset":  # mean 64 with a spread of bf16-exact steps (0.5 at 64)
        x = 64 + 0.5 * torch.randint(-4, 5, (N, C, H, W), generator=g).float()
    elif family == "constant":  # channel 1 (and every 5th) holds one value: var = 0
        x[:, 1::5] = 0.5
    gamma = (torch.rand(C, generator=g) + 0.5).to(BF)
    beta = torch.randn(C, generator=g) * 0.2 + 0.05
    if family == "constant":
        # y = fmaf(x, scale, fmaf(-mean, scale, beta)) = beta + the rounding of shift, at most 2^-25 |mean scale| = 2^-17
        # (scale <= 1.5 / sqrt(eps)): under half an ulp of bf16 for |beta| >= 1/8, so y is beta exactly
        beta[1::5] = torch.sign(beta[1::5]) * (0.125 + beta[1::5].abs())
    beta = beta.to(BF)
    if family == "sparse":  # most pre-activations negative
        beta = (beta.float() - 1.5).to(BF)
    res = torch.randn(N, C, H, W, generator=g).to(BF)
    dy = torch.randn(N, C, H, W, generator=g).to(BF)
    return x.to(BF), gamma, beta, res, dy


def head_inputs(N, K, P, ncls, dtype, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, K, P, 1, generator=g).to(dtype)
    w = (torch.randn(ncls, K, generator=g) * 0.05).to(dtype)
    b = (torch.randn(ncls, generator=g) * 0.1).to(dtype)
    t = torch.randint(0, ncls, (N,), generator=g)
    for i, bad in enumerate((-100, -1, ncls)):  # ignored labels beside valid ones
        if N > i + 1:
            t[i + 1] = bad
    gw0 = (torch.randn(ncls, K, generator=g) * 0.01).to(dtype)
    gb0 = (torch.randn(ncls, generator=g) * 0.01).to(dtype)
    return x, w, b, t, gw0, gb0
