"""The bf16 ResNet-18 kernels (conv_bf16.hip, batchnorm_nhwc.hip, head_pool.hip) against float64 references with error
budgets from rounding models (tests/resnet_numerics.py, docs/NUMERICS.md "ResNet-18"), at the sizes where the kernels
change path. References run on the CPU. Each check prints its budget use (`NUMERICS resnet ...`, shown by `pytest -s`).
Cases whose id starts with `degenerate` have H = 1, W = 1 or a single row (M = 1)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no ROCm GPU", allow_module_level=True)

import gpt2_numerics as gn  # noqa: E402
import resnet_numerics as rn  # noqa: E402
from simple_distributed_machine_learning_amd import _native, ops  # noqa: E402
from simple_distributed_machine_learning_amd.ops import conv as conv_ops  # noqa: E402

DEV = torch.device("cuda", 0)
K = _native.kernels()
BF = torch.bfloat16
EPS = 1e-5


def cl(t):
    return t.to(DEV).contiguous(memory_format=torch.channels_last)


def note(what, **ratios):
    print(f"NUMERICS resnet | {what} | " + " | ".join(f"{k} {v:.3f}" for k, v in ratios.items()))


def randn_bf(shape, seed, scale=1.0):
    return (torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale).to(BF)


# =====================================================================================================================
# convolution
def dgrad(dy, x, w, st, pd, add=None):
    """The input gradient the way ops/conv.py runs it (stride-1 3x3: the forward kernel on the flipped weights;
    stride 2: the parity-class kernel; stride-1 1x1: the forward kernel on the transposed weights)."""
    if w.shape[2] == 3 and st == 1:
        return K.conv3x3_fwd_bf16(dy, K.conv3x3_weight_bf16(w, True), add=add)
    return conv_ops._general_dgrad(dy, x, w, st, pd, add=add)


def check_conv_case(family, N, C, Co, H, W, ks=3, st=1, seed=0, halo=True):
    """Forward, forward + addend, input gradient (+ addend), accumulated weight gradient of one geometry."""
    pd = ks // 2
    x, w, dy = rn.conv_inputs(family, N, C, Co, H, W, ks, seed=seed, stride=st)
    add_y, add_x = randn_bf(dy.shape, seed + 1), randn_bf(x.shape, seed + 2)
    old = randn_bf(w.shape, seed + 3, 0.1)
    conv = torch.nn.Conv2d(C, Co, ks, st, pd, bias=False).to(DEV, BF)
    xd, dyd, wd = cl(x), cl(dy), w.to(DEV)
    if ks == 3 and st == 1 and halo:
        assert conv_ops.hip_eligible(xd, conv)
        wf = K.conv3x3_weight_bf16(wd, False)
        y = K.conv3x3_fwd_bf16(xd, wf)
        ya = K.conv3x3_fwd_bf16(xd, wf, add=cl(add_y))
        gw = old.to(DEV).clone()
        K.conv3x3_wgrad_bf16_(dyd, xd, gw)
    else:
        assert conv_ops.general_eligible(xd, conv)
        wf = K.conv3x3_weight_bf16(wd, False) if ks == 3 else wd
        y = K.conv_fwd_bf16(xd, wf, ks, st, pd)
        ya = K.conv_fwd_bf16(xd, wf, ks, st, pd, add=cl(add_y))
        gw = old.to(DEV).clone()
        K.conv_wgrad_bf16_(dyd, xd, gw, st, pd)
    dx = dgrad(dyd, xd, wd, st, pd)
    dxa = dgrad(dyd, xd, wd, st, pd, add=cl(add_x))
    torch.cuda.synchronize()
    assert y.is_contiguous(memory_format=torch.channels_last) and dx.shape == x.shape
    out = {}
    ref, extra = rn.conv_fwd_ref64(x, w, st, pd)
    out["fwd"] = rn.check_conv(y.cpu(), ref, extra, name="fwd")
    ref, extra = rn.conv_fwd_ref64(x, w, st, pd, add=add_y)
    out["fwd+add"] = rn.check_conv(ya.cpu(), ref, extra, name="fwd + add")
    ref, extra = rn.conv_dgrad_ref64(x.shape, w, dy, st, pd)
    out["dgrad"] = rn.check_conv(dx.cpu(), ref, extra, name="dgrad")
    ref, extra = rn.conv_dgrad_ref64(x.shape, w, dy, st, pd, add=add_x)
    out["dgrad+add"] = rn.check_conv(dxa.cpu(), ref, extra, name="dgrad + add")
    ref, extra, r = rn.conv_wgrad_ref64(x, w.shape, dy, st, pd, old=old)
    out["wgrad"] = rn.check_conv(gw.cpu(), ref, extra, r=r, name="wgrad")
    note(f"conv {family} {(N, C, Co, H, W, ks, st)}", **out)


# 3x3 stride 1: W <= 31 the halo kernel with 5 chunks, 32..95 with 7, above the im2col kernel; H = 1, W = 1; Co a
# multiple of 64 but not of 128; 245 pixels (under one 256-pixel tile), 256 (one tile), 272 (a second, partial tile)
CONV3X3 = [(1, 64, 64, 1, 1), (2, 64, 64, 5, 1), (1, 64, 128, 1, 31), (1, 64, 64, 2, 32), (1, 128, 64, 1, 95),
           (1, 64, 64, 1, 96), (1, 64, 64, 3, 97), (3, 64, 192, 9, 11), (5, 64, 64, 7, 7), (2, 64, 64, 16, 8),
           (2, 64, 64, 17, 8)]


def conv_id(s):
    degenerate = s[3] == 1 or s[4] == 1
    return ("degenerate-" if degenerate else "") + "x".join(str(v) for v in s)


@pytest.mark.parametrize("family", ["random sign", "positive"])
@pytest.mark.parametrize("shape", CONV3X3, ids=conv_id)
def test_conv3x3_budget(shape, family):
    check_conv_case(family, *shape, seed=sum(shape))


def test_conv3x3_budget_128_wide_tile():
    """The 128-channel output tile, which needs 160 tiles by default, forced at 99 pixels."""
    try:
        K.set_knob("CONV_BN128_MIN", 1)
        for family in ("random sign", "positive"):
            check_conv_case(family, 1, 64, 128, 9, 11, seed=7)
            check_conv_case(family, 2, 128, 256, 17, 8, seed=8)
    finally:
        K.reset_knobs()


# the list of test_strided_and_pointwise_conv, and H x W = 1 x 1, 1 x 2, 3 x 5 at stride 2
GENERAL = [(4, 64, 128, 28, 28, 3, 2), (3, 128, 256, 14, 14, 3, 2), (2, 256, 512, 7, 7, 3, 2), (4, 64, 128, 28, 28, 1, 2),
           (2, 256, 512, 7, 7, 1, 2), (3, 64, 64, 9, 11, 1, 1), (2, 128, 64, 9, 7, 3, 2), (64, 128, 128, 28, 28, 3, 2),
           (5, 128, 256, 15, 8, 1, 2), (3, 64, 128, 10, 12, 3, 1), (2, 64, 64, 1, 1, 3, 2), (2, 64, 128, 1, 2, 3, 2),
           (2, 128, 64, 3, 5, 3, 2), (2, 64, 64, 1, 1, 1, 2), (2, 64, 128, 1, 2, 1, 2), (2, 128, 64, 3, 5, 1, 2)]


@pytest.mark.parametrize("shape", GENERAL, ids=conv_id)
def test_strided_and_pointwise_conv_budget(shape):
    N, C, Co, H, W, ks, st = shape
    big = N * H * W > 20000  # (64 x 28 x 28, the parity-class kernel's 128-wide tile: one family)
    for family in (("random sign",) if big else ("random sign", "positive")):
        check_conv_case(family, N, C, Co, H, W, ks, st, seed=sum(shape), halo=False)


@pytest.mark.parametrize("N,Co,H,W", [(3, 32, 5, 9), (1, 64, 1, 1)], ids=["3x32x5x9", "degenerate-1x64x1x1"])
def test_stem_conv_budget(N, Co, H, W):
    for family in ("random sign", "positive"):
        x, w, dy = rn.conv_inputs(family, N, 1, Co, H, W, seed=N + Co)
        old = randn_bf(w.shape, 5, 0.1)
        conv = torch.nn.Conv2d(1, Co, 3, 1, 1, bias=False).to(DEV, BF)
        assert conv_ops.stem_eligible(x.to(DEV), conv)
        y = K.conv_c1_fwd_bf16(x.to(DEV).contiguous(), w.to(DEV))
        gw = old.to(DEV).clone()
        K.conv_c1_wgrad_bf16_(cl(dy), x.to(DEV).contiguous(), gw)
        torch.cuda.synchronize()
        ref, extra = rn.conv_fwd_ref64(x, w)
        a = rn.check_conv(y.cpu(), ref, extra, name="stem fwd")
        ref, extra, r = rn.conv_wgrad_ref64(x, w.shape, dy, old=old, per_split=64)
        b = rn.check_conv(gw.cpu(), ref, extra, r=r, name="stem wgrad")
        note(f"stem {family} {(N, Co, H, W)}", fwd=a, wgrad=b)


# impulses: one non-zero pixel and channel; every output is one product, so it equals bf16(x * w) bit for bit and is
# exactly 0 elsewhere. 3 images of 11 x 9 = 297 pixels: the four corners of the first image, pixels 255 and 256 of the
# flattened [N H W] index (the edge of the first 256-pixel tile) and the last pixel of the last image.
IMP_SHAPE = (3, 128, 11, 9)
IMP_PIXELS = [0, 8, 90, 98, 255, 256, 296]
IMP_CHANNELS = [0, 63, 64, 127]


@pytest.mark.parametrize("which", ["fwd", "dgrad", "wgrad"])
def test_conv3x3_impulse_is_exact(which):
    N, C, H, W = IMP_SHAPE
    w = rn.distinct_weights(C, C, 3, fixed_axis=1 if which == "fwd" else 0, seed=3).to(DEV)
    wl = K.conv3x3_weight_bf16(w, which == "dgrad")
    dense = rn.distinct_values(N, C, H, W, seed=4)
    for p in IMP_PIXELS:
        for c in IMP_CHANNELS:
            x = rn.impulse(IMP_SHAPE, p, c)
            if which == "wgrad":
                gw = torch.zeros(C, C, 3, 3, dtype=BF, device=DEV)
                K.conv3x3_wgrad_bf16_(cl(dense), cl(x), gw)
                got = gw
                want = torch.nn.grad.conv2d_weight(x.double(), gw.shape, dense.double(), padding=1)
            else:
                got = K.conv3x3_fwd_bf16(cl(x), wl)
                if which == "fwd":
                    want = torch.nn.functional.conv2d(x.double(), w.cpu().double(), padding=1)
                else:
                    want = torch.nn.grad.conv2d_input(x.shape, w.cpu().double(), x.double(), padding=1)
            want = want.float()  # (a product of two bf16 numbers is exact in fp32)
            assert int((want != 0).sum()) in (4 * C, 6 * C, 9 * C)  # corner, edge or interior: that many taps meet it
            assert torch.equal(got.cpu().float(), rn.rbf(want)), (which, p, c)


# =====================================================================================================================
# BatchNorm
BN_SHAPES = {1: (1, 1, 1), 2: (1, 1, 2), 63: (1, 7, 9), 64: (1, 8, 8), 65: (5, 13, 1), 105: (3, 5, 7), 1568: (8, 14, 14),
             32769: (3, 3, 3641)}  # M -> (N, H, W)
BN_CASES = [(C, M) for C in (8, 24, 40, 64, 1032, 2040, 2048) for M in (1, 2, 63, 64, 65, 105, 1568)] + [(8, 32769)]
COMBOS = [(False, False), (False, True), (True, False), (True, True)]  # (relu, residual)


def bn_forward(x, res, gamma, beta, rm0, rv0, momentum, relu, part=None):
    rm, rv = rm0.to(DEV).clone(), rv0.to(DEV).clone()
    nbt = torch.zeros((), dtype=torch.int64, device=DEV)
    y, mean, rstd = K.bn_nhwc_fwd(x, res, gamma.to(DEV), beta.to(DEV), rm, rv, EPS, momentum, relu, nbt, part=part)
    torch.cuda.synchronize()
    assert int(nbt) == 1
    return {"y": y, "mean": mean, "rstd": rstd, "running_mean": rm, "running_var": rv}


def check_bn_forward(got, x, res, gamma, beta, rm0, rv0, momentum, relu, terms, name):
    s, b = rn.bn_stats_ref64(x, EPS), rn.bn_stats_bounds(x, EPS, terms)
    out = {"mean": gn.check_elementwise(got["mean"].cpu(), s["mean"], extra=b["mean"], bf16=False, name=f"{name} mean"),
           "rstd": gn.check_elementwise(got["rstd"].cpu(), s["rstd"], extra=b["rstd"], bf16=False, name=f"{name} rstd")}
    run = rn.bn_running_ref64(x, EPS, momentum, rm0, rv0, terms)
    for k in ("running_mean", "running_var"):
        out[k] = gn.check_elementwise(got[k].cpu(), run[k], extra=run["e_" + k], bf16=True, name=f"{name} {k}")
    model = rn.bn_fwd_model(x, gamma, beta, EPS, res, relu)
    ref = rn.bn_fwd_ref64(x, gamma, beta, EPS, res, relu)
    row, rms = gn.check_grouped(rn.rows(got["y"].cpu()).t(), model.t(), ref.t(), name=f"{name} y",
                                fp32_extra=rn.bn_y_extra(x, gamma, EPS, terms).t())
    out["y row"], out["y rms"] = row, rms
    return out


def bn_backward(xd, dyd, y, mean, rstd, gamma, beta, relu, need_dres, gg0, gb0, part=None, part_rows=0):
    gg, gb = gg0.to(DEV).clone(), gb0.to(DEV).clone()
    dx, dres = K.bn_nhwc_bwd(xd, dyd, y, mean, rstd, gamma.to(DEV), relu, need_dres, gg, gb, beta.to(DEV), part=part,
                             part_rows=part_rows)
    torch.cuda.synchronize()
    return {"dx": dx, "dres": dres, "dgamma": gg, "dbeta": gb}


def check_bn_backward(got, x, dy, y, gamma, gg0, gb0, terms_fwd, terms_bwd, name):
    """y: the output the backward's mask comes from (CPU tensor, None without ReLU)."""
    mask = rn.relu_mask(y)
    ref = rn.bn_bwd_ref64(x, dy, gamma, EPS, mask, gg0, gb0)
    bnd = rn.bn_bwd_bounds(x, dy, gamma, EPS, mask, terms_fwd, terms_bwd)
    out = {k: gn.check_elementwise(got[k].cpu(), ref[k], r=bnd["r"], extra=bnd[k], bf16=True, name=f"{name} {k}")
           for k in ("dgamma", "dbeta")}
    model = rn.bn_bwd_model(x, dy, gamma, EPS, mask)
    row, rms = gn.check_grouped(rn.rows(got["dx"].cpu()).t(), model.t(), ref["dx"].t(), name=f"{name} dx",
                                fp32_extra=bnd["dx"].t())
    out["dx row"], out["dx rms"] = row, rms
    if got["dres"] is not None:  # dres = bf16(g), bit for bit
        assert torch.equal(rn.rows(got["dres"].cpu()).float(), ref["dres"].float()), f"{name}: dres"
    return out


def bn_case(family, C, M, relu, use_res, momentum, seed):
    N, H, W = BN_SHAPES[M]
    x, gamma, beta, res, dy = rn.bn_inputs(family, N, C, H, W, seed=seed)
    rm0, rv0 = randn_bf((C,), seed + 1, 0.3), (randn_bf((C,), seed + 2).float().abs() + 0.5).to(BF)
    gg0, gb0 = randn_bf((C,), seed + 3, 0.1), randn_bf((C,), seed + 4, 0.1)
    res = res if use_res else None
    terms = rn.bn_partial_terms(M, C)
    name = f"bn {family} C={C} M={M} relu={int(relu)} res={int(use_res)} m={momentum}"
    xd, dyd = cl(x), cl(dy)
    resd = cl(res) if use_res else None
    f = bn_forward(xd, resd, gamma, beta, rm0, rv0, momentum, relu)
    out = check_bn_forward(f, x, res, gamma, beta, rm0, rv0, momentum, relu, terms, name)
    if family == "constant" and not use_res:  # var = 0: y = relu?(beta) exactly (rn.bn_inputs keeps |beta| >= 1/8 there)
        yb = rn.bn_apply_model(torch.zeros_like(x), torch.zeros(C), beta.float(), None, relu)
        assert torch.equal(rn.rows(f["y"].cpu()).float()[:, 1::5], yb[:, 1::5]), name
    y = f["y"].cpu() if relu else None
    b = bn_backward(xd, dyd, f["y"] if relu else None, f["mean"], f["rstd"], gamma, beta, relu, use_res, gg0, gb0)
    out.update(check_bn_backward(b, x, dy, y, gamma, gg0, gb0, terms, terms, name))
    if relu and not use_res:  # the mask recomputed from x (no y kept) gives the bits of the mask from y
        b2 = bn_backward(xd, dyd, None, f["mean"], f["rstd"], gamma, beta, True, False, gg0, gb0)
        for k in ("dx", "dgamma", "dbeta"):
            assert torch.equal(b2[k], b[k]), f"{name}: {k} with the mask from x"
    note(name, **out)


@pytest.mark.parametrize("C,M", BN_CASES, ids=[("degenerate-" if m == 1 else "") + f"C{c}-M{m}" for c, m in BN_CASES])
def test_batchnorm_budget(C, M):
    """Small sizes: every input family x every (relu, residual) combination; the large ones (over 70 K elements) rotate
    the combinations over the families. momentum alternates between 0.1 and 1.0 (at 1.0 running_var is the unbiased
    variance itself; at M = 2 its factor is 2)."""
    small = C * M <= 70000
    for i, family in enumerate(rn.BN_FAMILIES):
        combos = COMBOS if small else [COMBOS[(i + C + M) % 4]]
        for j, (relu, use_res) in enumerate(combos):
            bn_case(family, C, M, relu, use_res, (0.1, 1.0)[(i + j) % 2], seed=C + M + 10 * i)


def test_batchnorm_unbiased_factor_at_two_rows():
    """M = 2, momentum 1: running_var is twice the biased variance, bit for bit against the fp32 expression."""
    x, gamma, beta, _, _ = rn.bn_inputs("uniform", 1, 64, 1, 2, seed=9)
    f = bn_forward(cl(x), None, gamma, beta, torch.zeros(64, dtype=BF), torch.ones(64, dtype=BF), 1.0, False)
    s = rn.bn_stats_ref64(x, EPS)
    assert torch.equal(f["running_var"].cpu(), (2 * s["var"]).float().to(BF))  # (x0 - x1)^2 / 2: exact in float64


@pytest.mark.parametrize("C,M", [(64, 105), (1032, 63), (8, 1568)])
def test_batchnorm_eval_budget(C, M):
    N, H, W = BN_SHAPES[M]
    for i, (relu, use_res) in enumerate(COMBOS):
        x, gamma, beta, res, _ = rn.bn_inputs(rn.BN_FAMILIES[i], N, C, H, W, seed=C + i)
        res = res if use_res else None
        bn = torch.nn.BatchNorm2d(C).to(DEV, BF).eval()
        rm, rv = randn_bf((C,), 1, 0.3), (randn_bf((C,), 2).float().abs() + 0.5).to(BF)
        with torch.no_grad():
            bn.weight.copy_(gamma)
            bn.bias.copy_(beta)
            bn.running_mean.copy_(rm)
            bn.running_var.copy_(rv)
            y = conv_ops.batch_norm(bn, cl(x), res=cl(res) if use_res else None, relu=relu)
        ref = rn.bn_eval_ref64(x, gamma, beta, rm, rv, EPS, res, relu)
        model = rn.bn_eval_model(x, gamma, beta, rm, rv, EPS, res, relu)
        row, rms = gn.check_grouped(rn.rows(y.cpu()).t(), model.t(), ref.t(), name="bn eval y")
        note(f"bn eval C={C} M={M} relu={int(relu)} res={int(use_res)}", **{"y row": row, "y rms": rms})


@pytest.mark.parametrize("N,C,Co,H,W,relu", [(4, 64, 128, 14, 14, 0), (2, 128, 64, 9, 7, 1), (4, 64, 64, 14, 14, 2)])
def test_batchnorm_budget_from_convolution_epilogue_partials(N, C, Co, H, W, relu):
    """The forward statistics from the producing convolution's epilogue (sums over 256-pixel tiles of the stored y) and
    the backward statistics from the consuming convolution's input-gradient epilogue: the same budgets, with 256 terms
    per partial."""
    x, w, _ = rn.conv_inputs("random sign", N, C, Co, H, W, seed=N + C + relu)
    _, gamma, beta, res, _ = rn.bn_inputs("uniform", N, Co, H, W, seed=3)
    rm0, rv0 = torch.zeros(Co, dtype=BF), torch.ones(Co, dtype=BF)
    rows_ = K.conv_part_rows(N, H, W)
    part = torch.full((rows_ * 2 * Co,), float("nan"), device=DEV)
    yc = K.conv3x3_fwd_bf16(cl(x), K.conv3x3_weight_bf16(w.to(DEV), False), part=part)  # the BatchNorm's input
    use_res = relu == 1
    resd = cl(res) if use_res else None
    f = bn_forward(yc, resd, gamma, beta, rm0, rv0, 0.1, relu != 0, part=part)
    name = f"bn from conv partials {(N, C, Co, H, W)} relu={relu}"
    xb = yc.cpu()
    out = check_bn_forward(f, xb, res if use_res else None, gamma, beta, rm0, rv0, 0.1, relu != 0, rn.CONV_TILE, name)
    # backward: dy of the BatchNorm = the input gradient of a 3x3 convolution Co -> Co that consumes its output
    w2 = randn_bf((Co, Co, 3, 3), 5, 0.05)
    dy2 = randn_bf((N, Co, H, W), 6)
    bpart = torch.full((rows_ * 2 * Co,), float("nan"), device=DEV)
    dyb = K.conv3x3_fwd_bf16(cl(dy2), K.conv3x3_weight_bf16(w2.to(DEV), True), part=bpart, bn_x=yc,
                             bn_y=f["y"] if relu == 1 else None, bn_mean=f["mean"], bn_rstd=f["rstd"],
                             bn_gamma=gamma.to(DEV), bn_beta=beta.to(DEV), bn_relu=relu)
    gg0, gb0 = randn_bf((Co,), 7, 0.1), randn_bf((Co,), 8, 0.1)
    b = bn_backward(yc, dyb, f["y"] if relu == 1 else None, f["mean"], f["rstd"], gamma, beta, relu != 0, use_res, gg0,
                    gb0, part=bpart, part_rows=rows_)
    out.update(check_bn_backward(b, xb, dyb.cpu(), f["y"].cpu() if relu else None, gamma, gg0, gb0, rn.CONV_TILE,
                                 rn.CONV_TILE, name))
    note(name, **out)


# =====================================================================================================================
# pooled head
def run_head(x, w, b, t, gw0, gb0, scale, stats0, init):
    yd = cl(x)
    gw, gb = gw0.to(DEV).clone(), gb0.to(DEV).clone()
    stats = stats0.to(DEV).clone()
    assert ops.pooled_head_ok(yd, w.to(DEV))
    dy = ops.pooled_head_xent(yd, w.to(DEV), b.to(DEV), t.to(DEV), gw, gb, scale, stats, init)
    torch.cuda.synchronize()
    N, Kc = x.shape[0], x.shape[1]
    return {"dx": dy.permute(0, 2, 3, 1).reshape(N, -1, Kc).cpu(), "gw": gw.cpu(), "gb": gb.cpu(), "stats": stats.cpu()}


@pytest.mark.parametrize("dtype", [BF, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("N,Kc,P,ncls", rn.HEAD_SHAPES,
                         ids=[("degenerate-" if s[0] == 1 else "") + "x".join(map(str, s)) for s in rn.HEAD_SHAPES])
def test_pooled_head_budget(N, Kc, P, ncls, dtype):
    """K > 512 (a lane's second channel chunk), P a multiple of 8 plus a tail, N no multiple of 4; labels -100, -1 and
    ncls beside valid ones; stats added to and overwritten."""
    x, w, b, t, gw0, gb0 = rn.head_inputs(N, Kc, P, ncls, dtype, seed=N + Kc)
    scale = 1.0 / 97
    for init, stats0 in ((False, torch.tensor([3.0, 3.0])), (True, torch.tensor([float("nan"), 7.0]))):
        got = run_head(x, w, b, t, gw0, gb0, scale, stats0, init)
        ref = rn.head_ref64(x, w, b, t, scale, gw0, gb0, None if init else stats0)
        bnd = rn.head_bounds(x, w, b, scale, ref, gw0, gb0, None if init else stats0)
        out = rn.check_head(got, ref, bnd, dtype == BF, name=f"head {(N, Kc, P, ncls)}")
        note(f"head {(N, Kc, P, ncls)} {'bf16' if dtype == BF else 'fp32'} stats {'overwritten' if init else 'added'}", **out)
    if N > 3:  # the three ignored rows have no gradient at all
        assert float(got["dx"][1:4].abs().max()) == 0


@pytest.mark.parametrize("dtype", [BF, torch.float32], ids=["bf16", "fp32"])
def test_pooled_head_tied_logits(dtype):
    """Zero weights make the logits the biases: rows of all-equal logits (the first class is the argmax) and of two equal
    largest ones (the lower index is)."""
    N, Kc, P, ncls = 6, 520, 9, 4
    x = randn_bf((N, Kc, P, 1), 3).to(dtype)
    w = torch.zeros(ncls, Kc, dtype=dtype)
    z = torch.zeros(ncls, Kc, dtype=dtype), torch.zeros(ncls, dtype=dtype), torch.zeros(2)
    for b, t, correct in ((torch.full((ncls,), 0.5), torch.tensor([0, 1, 3, 0, -1, 0]), 3.0),
                          (torch.tensor([0.125, 0.5, 0.5, 0.25]), torch.tensor([1, 2, 1, 2, 0, ncls]), 2.0)):
        got = run_head(x, w, b.to(dtype), t, z[0], z[1], 0.25, z[2], False)
        ref = rn.head_ref64(x, w, b.to(dtype), t, 0.25, z[0], z[1], z[2])
        assert float(ref["stats"][1]) == correct
        rn.check_head(got, ref, rn.head_bounds(x, w, b.to(dtype), 0.25, ref, z[0], z[1], z[2]), dtype == BF, name="tied")
