"""The ResNet numerics checker (tests/resnet_numerics.py) tested on itself, on the CPU: honest fp32 implementations stay
inside every budget on every input family, seeded defects are rejected, and each defect's test states whether the
tolerance of tests/test_conv_gpu.py / tests/test_head_pool_gpu.py accepted it. `pytest -s` prints the ratios
(`NUMERICS resnet selftest ...`); docs/NUMERICS.md records them."""
import pytest
import torch
import torch.nn.functional as F

import gpt2_numerics as gn
import resnet_numerics as rn

BF = torch.bfloat16


def note(what, **ratios):
    print(f"NUMERICS resnet selftest | {what} | " + " | ".join(f"{k} {v:.3f}" for k, v in ratios.items()))


def old_conv_tolerance_accepts(y, x, w):
    """tests/test_conv_gpu.py: |y - fp32 conv| <= 2^-7 (conv(|x|, |w|) + 1e-3)."""
    yr = F.conv2d(x.float(), w.float(), padding=1)
    scale = F.conv2d(x.float().abs(), w.float().abs(), padding=1) + 1e-3
    return bool(((y.float() - yr).abs() <= 2 ** -7 * scale).all())


# ---- honest implementations ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["random sign", "positive"])
@pytest.mark.parametrize("N,C,Co,H,W,ks,st", [(2, 64, 64, 14, 14, 3, 1), (2, 256, 256, 4, 4, 3, 1), (1, 64, 128, 1, 31, 3, 1),
                                               (2, 64, 64, 5, 1, 3, 1), (2, 128, 64, 9, 7, 3, 2), (2, 64, 128, 3, 5, 1, 2),
                                               (3, 1, 32, 5, 9, 3, 1)])
def test_honest_fp32_convolution_is_inside_every_budget(N, C, Co, H, W, ks, st, family):
    x, w, dy = rn.conv_inputs(family, N, C, Co, H, W, ks, seed=N + C + H, stride=st)
    pd = ks // 2
    g = torch.Generator().manual_seed(5)
    add = torch.randn(dy.shape, generator=g).to(BF)
    old = (torch.randn(w.shape, generator=g) * 0.1).to(BF)
    ref, extra = rn.conv_fwd_ref64(x, w, st, pd)
    y32 = F.conv2d(x.float(), w.float(), stride=st, padding=pd)
    a = rn.check_conv(rn.rbf(y32), ref, extra, name="fwd")
    ref, extra = rn.conv_fwd_ref64(x, w, st, pd, add=add)
    b = rn.check_conv(rn.rbf(y32 + add.float()), ref, extra, name="fwd + add")
    ref, extra = rn.conv_dgrad_ref64(x.shape, w, dy, st, pd)
    c = rn.check_conv(rn.rbf(torch.nn.grad.conv2d_input(x.shape, w.float(), dy.float(), stride=st, padding=pd)), ref,
                      extra, name="dgrad")
    ref, extra, r = rn.conv_wgrad_ref64(x, w.shape, dy, st, pd, old=old)
    gw32 = torch.nn.grad.conv2d_weight(x.float(), w.shape, dy.float(), stride=st, padding=pd)
    d = rn.check_conv(rn.rbf(old.float() + gw32), ref, extra, r=r, name="wgrad")
    note(f"honest conv {family} {(N, C, Co, H, W, ks, st)}", fwd=a, add=b, dgrad=c, wgrad=d)


def test_all_positive_budget_is_close_to_half_an_ulp():
    """conv(|x|, |w|) is the output itself, so the fp32 term is (K + 8) 2^-24 of it: under 3 % of half an ulp of
    bf16 (2^-9 relative) at K = 576, under 8 % at K = 2304."""
    for C, lim in ((64, 0.03), (256, 0.08)):
        x, w, _ = rn.conv_inputs("positive", 1, C, 64, 4, 4, seed=C)
        ref, extra = rn.conv_fwd_ref64(x, w)
        assert float((extra / (0.5 * gn.ulp_bf16(ref))).max()) < lim * 2  # ulp is up to 2x coarser than 2^-8 |ref|
        assert float((extra / ref.abs()).max()) <= (9 * C + 8) * gn.U32 * 1.0000001


def bn_stats_fp32(x, order):
    """The kernel's statistics algorithm in torch: fp32 partial sums of x and x^2 over blocks of rows (order "blocks":
    the kernel's row blocks, summed row by row; "strided": 7 interleaved partials, summed pairwise by torch), float64
    finalisation."""
    xr = rn.rows(x).float()
    M = xr.shape[0]
    if order == "blocks":
        _, rpb = rn.bn_blocks(M)
        parts1, parts2 = [], []
        for r0 in range(0, M, rpb):
            a = torch.zeros(xr.shape[1])
            b = torch.zeros(xr.shape[1])
            for r in range(r0, min(M, r0 + rpb)):
                a = a + xr[r]
                b = b + xr[r] * xr[r]
            parts1.append(a)
            parts2.append(b)
    else:
        parts1 = [xr[i::7].sum(0) for i in range(7)]
        parts2 = [(xr[i::7] * xr[i::7]).sum(0) for i in range(7)]
    s1 = torch.stack(parts1).double().sum(0)
    s2 = torch.stack(parts2).double().sum(0)
    mu = s1 / M
    var = (s2 / M - mu * mu).clamp_min(0.0)
    return mu, var


def bn_forward_fp32(x, gamma, beta, eps, momentum, rm0, rv0, res, relu, order, unbiased=True):
    mu, var = bn_stats_fp32(x, order)
    M = rn.rows(x).shape[0]
    mean32 = mu.float()
    rstd32 = (1.0 / torch.sqrt(var + float(torch.tensor(eps, dtype=torch.float32)))).float()
    scale, shift = rn.bn_fold32(mean32, rstd32, gamma, beta)
    y = rn.bn_apply_model(x, scale, shift, res, relu)
    unb = (var * M / (M - 1) if (M > 1 and unbiased) else var).float()
    m = torch.tensor(momentum, dtype=torch.float32)
    rm = rn.rbf((1 - m) * rm0.float() + m * mean32)
    rv = rn.rbf((1 - m) * rv0.float() + m * unb)
    return {"y": y, "mean": mean32, "rstd": rstd32, "running_mean": rm, "running_var": rv}


def check_bn_forward(got, x, gamma, beta, eps, momentum, rm0, rv0, res, relu, terms, name):
    s, b = rn.bn_stats_ref64(x, eps), rn.bn_stats_bounds(x, eps, terms)
    out = {"mean": gn.check_elementwise(got["mean"], s["mean"], extra=b["mean"], bf16=False, name=f"{name} mean"),
           "rstd": gn.check_elementwise(got["rstd"], s["rstd"], extra=b["rstd"], bf16=False, name=f"{name} rstd")}
    run = rn.bn_running_ref64(x, eps, momentum, rm0, rv0, terms)
    for k in ("running_mean", "running_var"):
        out[k] = gn.check_elementwise(got[k], run[k], extra=run["e_" + k], bf16=True, name=f"{name} {k}")
    model = rn.bn_fwd_model(x, gamma, beta, eps, res, relu)
    ref = rn.bn_fwd_ref64(x, gamma, beta, eps, res, relu)
    row, rms = gn.check_grouped(got["y"].t(), model.t(), ref.t(), name=f"{name} y",
                                fp32_extra=rn.bn_y_extra(x, gamma, eps, terms).t())
    out["y_row"], out["y_rms"] = row, rms
    return out


@pytest.mark.parametrize("family", rn.BN_FAMILIES)
@pytest.mark.parametrize("N,C,H,W", [(8, 64, 14, 14), (3, 24, 5, 7), (1, 8, 1, 2), (1, 8, 1, 1), (5, 40, 13, 1)])
def test_honest_fp32_batchnorm_forward_is_inside_every_budget(N, C, H, W, family):
    """Two summation orders of the kernel's algorithm (fp32 partials, float64 finalisation) pass every forward check."""
    x, gamma, beta, res, _ = rn.bn_inputs(family, N, C, H, W, seed=N + C)
    g = torch.Generator().manual_seed(1)
    rm0, rv0 = (torch.randn(C, generator=g) * 0.3).to(BF), (torch.rand(C, generator=g) + 0.5).to(BF)
    M = N * H * W
    terms = max(rn.bn_partial_terms(M, C), -(-M // 7))  # (the strided order has partials of M / 7 rows)
    for order in ("blocks", "strided"):
        for relu, use_res, momentum in ((True, False, 0.1), (True, True, 1.0), (False, False, 1.0)):
            r = res if use_res else None
            got = bn_forward_fp32(x, gamma, beta, 1e-5, momentum, rm0, rv0, r, relu, order)
            out = check_bn_forward(got, x, gamma, beta, 1e-5, momentum, rm0, rv0, r, relu, terms,
                                   f"{family} {order}")
        note(f"honest bn fwd {family} {order} {(N, C, H, W)}", **out)
    if family == "constant":
        y = bn_forward_fp32(x, gamma, beta, 1e-5, 0.1, rm0, rv0, None, False, "blocks")["y"]
        assert torch.equal(y[:, 1::5], beta.float()[1::5].expand(M, -1))  # var = 0: y is beta exactly


def bn_backward_fp32(x, dy, y, gamma, eps, order, gg0, gb0, drop=None, skip_row=None):
    """The kernel's backward in torch from fp32 statistics of `order`: fp32 sums of g and g xhat (per 32-row chunk,
    chunks added in float64), the folded coefficients, dx. skip_row: the dgamma sum misses that row (a seeded defect)."""
    mu, var = bn_stats_fp32(x, order)
    mean32 = mu.float()
    rstd32 = (1.0 / torch.sqrt(var + float(torch.tensor(eps, dtype=torch.float32)))).float()
    g = rn.rows(dy).float()
    mask = rn.relu_mask(y)
    if mask is not None:
        g = g * mask
    xr = rn.rows(x).float()
    M = g.shape[0]
    gx = g * (xr - mean32) * rstd32
    gxs = gx.clone()
    if skip_row is not None:
        gxs[skip_row] = 0
    s1 = torch.stack([c.sum(0) for c in g.split(32)]).double().sum(0)
    s2 = torch.stack([c.sum(0) for c in gxs.split(32)]).double().sum(0)
    s2x = torch.stack([c.sum(0) for c in gx.split(32)]).double().sum(0)
    a = gamma.float() * rstd32
    mg = (s1 / M).float()
    b = -a * rstd32 * (s2x / M).float()
    if drop == "xhat":
        b = torch.zeros_like(b)
    if drop == "mean":
        mg = torch.zeros_like(mg)
    dx = rn.rbf(rn.fma32(a, g - mg, b * (xr - mean32)))
    return {"dx": dx, "dres": g, "dgamma": rn.rbf(gg0.float() + s2.float()), "dbeta": rn.rbf(gb0.float() + s1.float())}


def check_bn_backward(got, x, dy, y, gamma, eps, gg0, gb0, terms_fwd, terms_bwd, name):
    mask = rn.relu_mask(y)
    ref = rn.bn_bwd_ref64(x, dy, gamma, eps, mask, gg0, gb0)
    bnd = rn.bn_bwd_bounds(x, dy, gamma, eps, mask, terms_fwd, terms_bwd)
    out = {k: gn.check_elementwise(got[k], ref[k], r=bnd["r"], extra=bnd[k], bf16=True, name=f"{name} {k}")
           for k in ("dgamma", "dbeta")}
    model = rn.bn_bwd_model(x, dy, gamma, eps, mask)
    row, rms = gn.check_grouped(got["dx"].t(), model.t(), ref["dx"].t(), name=f"{name} dx", fp32_extra=bnd["dx"].t())
    out["dx_row"], out["dx_rms"] = row, rms
    if "dres" in got and got["dres"] is not None:
        assert torch.equal(got["dres"].float(), ref["dres"].float()), f"{name}: dres is not bf16(g) bit for bit"
    return out


@pytest.mark.parametrize("family", rn.BN_FAMILIES)
@pytest.mark.parametrize("N,C,H,W", [(8, 64, 14, 14), (3, 24, 5, 7), (1, 8, 1, 2), (1, 8, 1, 1)])
def test_honest_fp32_batchnorm_backward_is_inside_every_budget(N, C, H, W, family):
    x, gamma, beta, res, dy = rn.bn_inputs(family, N, C, H, W, seed=N + C + 1)
    g = torch.Generator().manual_seed(2)
    gg0, gb0 = (torch.randn(C, generator=g) * 0.1).to(BF), (torch.randn(C, generator=g) * 0.1).to(BF)
    M = N * H * W
    tf = max(rn.bn_partial_terms(M, C), -(-M // 7))
    for order in ("blocks", "strided"):
        for relu, use_res in ((True, False), (True, True), (False, False)):
            y = None
            if relu:
                y = bn_forward_fp32(x, gamma, beta, 1e-5, 0.1, gg0, gb0, res if use_res else None, True, order)["y"]
                y = y.view(N, H, W, C).permute(0, 3, 1, 2)
            got = bn_backward_fp32(x, dy, y, gamma, 1e-5, order, gg0, gb0)
            out = check_bn_backward(got, x, dy, y, gamma, 1e-5, gg0, gb0, tf, max(32, M // 32 + 1), f"{family} {order}")
        note(f"honest bn bwd {family} {order} {(N, C, H, W)}", **out)


@pytest.mark.parametrize("dtype", [BF, torch.float32])
@pytest.mark.parametrize("N,K,P,ncls", rn.HEAD_SHAPES)
def test_honest_fp32_pooled_head_is_inside_every_budget(N, K, P, ncls, dtype):
    x, w, b, t, gw0, gb0 = rn.head_inputs(N, K, P, ncls, dtype, seed=N + K)
    scale = 1.0 / 97
    stats0 = torch.tensor([3.0, 3.0])
    ref = rn.head_ref64(x, w, b, t, scale, gw0, gb0, stats0)
    bnd = rn.head_bounds(x, w, b, scale, ref, gw0, gb0, stats0)
    h = rn.head_fp32(x, w, b, t, scale)
    got = {"dx": h["dx"].to(dtype), "gw": (gw0.float() + h["gw"]).to(dtype), "gb": (gb0.float() + h["gb"]).to(dtype),
           "stats": stats0 + h["stats"]}
    note(f"honest head {(N, K, P, ncls)} {dtype}", **rn.check_head(got, ref, bnd, dtype == BF))


def test_pooled_head_reference_ties_and_ignored_labels():
    """Zero weights and equal biases tie every logit (the first index is the argmax); two equal largest biases tie two;
    labels -100, -1 and ncls give no loss, no count and no gradient."""
    N, K, P, ncls = 6, 8, 2, 4
    x = torch.randn(N, K, P, 1).to(BF)
    w = torch.zeros(ncls, K, dtype=BF)
    t = torch.tensor([0, 1, -100, -1, ncls, 0])
    ref = rn.head_ref64(x, w, torch.full((ncls,), 0.5, dtype=BF), t, 1.0)
    assert ref["correct"].tolist() == [1, 0, 0, 0, 0, 1] and ref["valid"].tolist() == [True, True, False, False, False, True]
    assert float(ref["dl"][2:5].abs().max()) == 0 and float(ref["loss"][2:5].abs().max()) == 0
    ref = rn.head_ref64(x, w, torch.tensor([0.1, 0.5, 0.5, 0.2], dtype=BF), torch.tensor([1, 2, 1, 2, 0, 1]), 1.0)
    assert ref["correct"].tolist() == [1, 0, 1, 0, 0, 1]


# ---- seeded defects -----------------------------------------------------------------------------------------------
def conv_bf16_per_tap(x, w):
    """3x3 forward that rounds its accumulator to bf16 after every tap."""
    acc = torch.zeros(x.shape[0], w.shape[0], x.shape[2], x.shape[3])
    xp = F.pad(x.float(), (1, 1, 1, 1))
    for kh in range(3):
        for kw in range(3):
            tap = torch.einsum("nchw,oc->nohw", xp[:, :, kh:kh + x.shape[2], kw:kw + x.shape[3]], w.float()[:, :, kh, kw])
            acc = rn.rbf(acc + tap)
    return acc


@pytest.mark.parametrize("N,C,Co,H,W,ratio", [(2, 64, 64, 14, 14, 19.7), (2, 256, 256, 4, 4, 3.3)])
def test_bf16_accumulation_per_tap_is_rejected_and_the_old_tolerance_accepted_it(N, C, Co, H, W, ratio):
    x, w, _ = rn.conv_inputs("random sign", N, C, Co, H, W, seed=N * 1000 + C + Co + H)
    bad = conv_bf16_per_tap(x, w)
    ref, extra = rn.conv_fwd_ref64(x, w)
    with pytest.raises(gn.Budget):
        rn.check_conv(bad, ref, extra, name="bf16 per tap")
    over = float(((bad.double() - ref).abs() / (0.5 * gn.ulp_bf16(ref) + extra)).max())
    note(f"defect bf16 per tap C={C}", over_budget=over)
    assert over > 2.0
    assert old_conv_tolerance_accepts(bad, x, w)  # 2^-7 conv(|x|, |w|): accepted


def test_lost_tap_channel_is_rejected_and_the_old_tolerance_accepted_it():
    """Tap (0, 0) of input channel 0 lost at C = 256: 32 x over the new budget, 0.67 of the old tolerance. (The old
    ratio depends on the channel's largest product: channels 100 and 255 give 0.90 and 0.42, channel 5 1.44.)"""
    x, w, _ = rn.conv_inputs("random sign", 2, 256, 256, 4, 4, seed=2000 + 256 + 256 + 4)
    w2 = w.clone()
    w2[:, 0, 0, 0] = 0
    bad = rn.rbf(F.conv2d(x.float(), w2.float(), padding=1))
    ref, extra = rn.conv_fwd_ref64(x, w)
    with pytest.raises(gn.Budget):
        rn.check_conv(bad, ref, extra, name="lost tap")
    over = float(((bad.double() - ref).abs() / (0.5 * gn.ulp_bf16(ref) + extra)).max())
    note("defect lost tap C=256", over_budget=over)
    assert over > 20
    assert old_conv_tolerance_accepts(bad, x, w)
    # all-positive inputs leave no room at all: the budget is within a few per cent of half an ulp
    xp, wp, _ = rn.conv_inputs("positive", 2, 256, 256, 4, 4, seed=1)
    w2 = wp.clone()
    w2[:, 5, 0, 0] = 0
    ref, extra = rn.conv_fwd_ref64(xp, wp)
    with pytest.raises(gn.Budget):
        rn.check_conv(rn.rbf(F.conv2d(xp.float(), w2.float(), padding=1)), ref, extra, name="lost tap, positive")


def test_missing_halo_column_is_rejected():
    """The taps kw = 2 do not see the last input column (a halo one column short at the right image edge). The old
    tolerance rejected this one too at 64 channels: one of nine taps of a whole column is 0.3 of the output's RMS."""
    x, w, _ = rn.conv_inputs("random sign", 2, 64, 64, 5, 31, seed=9)
    xl = torch.zeros_like(x)
    xl[..., -1] = x[..., -1]
    wk = torch.zeros_like(w)
    wk[..., 2] = w[..., 2]
    bad = rn.rbf(F.conv2d(x.float(), w.float(), padding=1) - F.conv2d(xl.float(), wk.float(), padding=1))
    ref, extra = rn.conv_fwd_ref64(x, w)
    with pytest.raises(gn.Budget):
        rn.check_conv(bad, ref, extra, name="halo column")
    assert not old_conv_tolerance_accepts(bad, x, w)


@pytest.mark.parametrize("N,C,H,W,momentum", [(8, 64, 14, 14, 1.0), (3, 24, 5, 7, 0.1), (3, 24, 5, 7, 1.0), (1, 8, 1, 2, 0.1)])
def test_biased_running_var_is_rejected_and_the_old_tolerance_accepted_it(N, C, H, W, momentum):
    """running_var from the biased variance. The new bound rejects it wherever the bf16 store can show it: var / M
    against half an ulp of bf16 (2^-9 relative) - at M = 105 with either momentum, at M = 2, and at M = 1568 with
    momentum 1 - and test_batchnorm_nhwc_train_matches_torch's rtol 2e-2, atol 1e-2 accepts it at its shapes."""
    x, gamma, beta, _, _ = rn.bn_inputs("uniform", N, C, H, W, seed=N + C + H)
    M = N * H * W
    rm0, rv0 = torch.zeros(C, dtype=BF), torch.ones(C, dtype=BF)
    terms = rn.bn_partial_terms(M, C)
    good = bn_forward_fp32(x, gamma, beta, 1e-5, momentum, rm0, rv0, None, False, "blocks")
    bad = bn_forward_fp32(x, gamma, beta, 1e-5, momentum, rm0, rv0, None, False, "blocks", unbiased=False)
    run = rn.bn_running_ref64(x, 1e-5, momentum, rm0, rv0, terms)
    gn.check_elementwise(good["running_var"], run["running_var"], extra=run["e_running_var"], name="running_var")
    with pytest.raises(gn.Budget):
        gn.check_elementwise(bad["running_var"], run["running_var"], extra=run["e_running_var"], name="biased")
    if M > 2:  # (M = 2 is none of the old test's shapes: there the factor is 2 and its tolerance would see it)
        torch.testing.assert_close(bad["running_var"], run["running_var"].float(), rtol=2e-2, atol=1e-2)


OLD_ACCEPTS_DX = {"xhat": False, "mean": False}  # measured on the CPU by the test below


@pytest.mark.parametrize("drop", ["xhat", "mean"])
def test_bn_dx_without_a_correction_term_is_rejected(drop):
    """dx without its xhat mean(g xhat) term, and without its mean(g) term, at the old test's 8 x 64 x 14 x 14 case.
    Both means are of order 1 / sqrt(M) = 0.025 there, times gamma rstd and |xhat| up to 1.7: the worst errors are 0.15
    and 0.065, so the old rtol = atol = 3e-2 rejected both as well (measured, recorded below)."""
    N, C, H, W = 8, 64, 14, 14
    x, gamma, beta, _, dy = rn.bn_inputs("uniform", N, C, H, W, seed=N + C + H)
    ref = rn.bn_bwd_ref64(x, dy, gamma, 1e-5)
    model = rn.bn_bwd_model(x, dy, gamma, 1e-5)
    bnd = rn.bn_bwd_bounds(x, dy, gamma, 1e-5, None, rn.bn_partial_terms(N * H * W, C), rn.bn_partial_terms(N * H * W, C))
    gn.check_grouped(model.t(), model.t(), ref["dx"].t(), name="dx", fp32_extra=bnd["dx"].t())
    bad = rn.bn_bwd_model(x, dy, gamma, 1e-5, drop=drop)
    with pytest.raises(gn.Budget):
        gn.check_grouped(bad.t(), model.t(), ref["dx"].t(), name=f"dx without {drop}", fp32_extra=bnd["dx"].t())
    old_ok = bool(torch.isclose(bad, ref["dx"].float(), rtol=3e-2, atol=3e-2).all())
    note(f"defect dx without {drop}", old_tolerance_accepts=float(old_ok),
         worst_error=float((bad.double() - ref["dx"]).abs().max()))
    assert old_ok == OLD_ACCEPTS_DX[drop]


def test_dgamma_missing_one_row_is_rejected():
    """One pixel row missing from the dgamma sum at 8 x 64 x 14 x 14. The old atol = 0.5 rejected it too at 22 of the 64
    channels, those where |g xhat| of the lost row is over 0.5; it accepted the other 42 channels' errors."""
    N, C, H, W = 8, 64, 14, 14
    x, gamma, beta, _, dy = rn.bn_inputs("uniform", N, C, H, W, seed=3)
    z = torch.zeros(C, dtype=BF)
    tf = rn.bn_partial_terms(N * H * W, C)
    good = bn_backward_fp32(x, dy, None, gamma, 1e-5, "blocks", z, z)
    check_bn_backward(good, x, dy, None, gamma, 1e-5, z, z, tf, 64, "dgamma")
    bad = bn_backward_fp32(x, dy, None, gamma, 1e-5, "blocks", z, z, skip_row=777)
    with pytest.raises(gn.Budget):
        check_bn_backward(bad, x, dy, None, gamma, 1e-5, z, z, tf, 64, "dgamma, row 777 missing")
    ref = rn.bn_bwd_ref64(x, dy, gamma, 1e-5)
    old_ok = torch.isclose(bad["dgamma"], ref["dgamma"].float(), rtol=2e-2, atol=0.5)  # the old atol = 0.5
    assert int(old_ok.sum()) == 42


@pytest.mark.parametrize("dtype", [BF, torch.float32])
def test_pooled_head_dropping_the_tail_position_is_rejected(dtype):
    """P = 9: the position after the batch of 8 left out of the pool. The old test (rtol = 2e-2 of the largest
    gradient for bf16, 1e-5 for fp32) has no P with a tail; at this shape its tolerance rejects the defect too."""
    N, K, P, ncls = 5, 520, 9, 10
    x, w, b, t, gw0, gb0 = rn.head_inputs(N, K, P, ncls, dtype, seed=4)
    ref = rn.head_ref64(x, w, b, t, 1 / 97, gw0, gb0)
    bnd = rn.head_bounds(x, w, b, 1 / 97, ref, gw0, gb0)
    for drop in (False, True):
        h = rn.head_fp32(x, w, b, t, 1 / 97, drop_tail=drop)
        got = {"dx": h["dx"].to(dtype), "gw": (gw0.float() + h["gw"]).to(dtype), "gb": (gb0.float() + h["gb"]).to(dtype),
               "stats": h["stats"]}
        if drop:
            with pytest.raises(gn.Budget):
                rn.check_head(got, ref, bnd, dtype == BF)
        else:
            rn.check_head(got, ref, bnd, dtype == BF)


def test_double_rounded_addend_is_rejected():
    """y = bf16(bf16(conv) + add), what the convolution epilogue computed before this check existed, against
    bf16(conv + add): where conv and addend cancel, the first rounding's error is many ulps of the result."""
    x, w, _ = rn.conv_inputs("random sign", 2, 64, 64, 7, 7, seed=11)
    y32 = F.conv2d(x.float(), w.float(), padding=1)
    add = (-y32 + 0.01 * torch.randn(y32.shape, generator=torch.Generator().manual_seed(3))).to(BF)
    ref, extra = rn.conv_fwd_ref64(x, w, add=add)
    rn.check_conv(rn.rbf(y32 + add.float()), ref, extra, name="one rounding")
    with pytest.raises(gn.Budget):
        rn.check_conv(rn.rbf(rn.rbf(y32) + add.float()), ref, extra, name="two roundings")


def test_no_exemptions_a_nan_fails():
    x, w, _ = rn.conv_inputs("random sign", 1, 64, 64, 3, 3, seed=1)
    ref, extra = rn.conv_fwd_ref64(x, w)
    y = rn.rbf(F.conv2d(x.float(), w.float(), padding=1))
    y[0, 3, 1, 1] = float("nan")
    with pytest.raises(gn.Budget):
        rn.check_conv(y, ref, extra)
    xb, gamma, beta, _, _ = rn.bn_inputs("uniform", 2, 8, 3, 3)
    model = rn.bn_fwd_model(xb, gamma, beta, 1e-5)
    bad = model.clone()
    bad[4, 2] = float("nan")
    with pytest.raises(gn.Budget):
        gn.check_grouped(bad.t(), model.t(), rn.bn_fwd_ref64(xb, gamma, beta, 1e-5).t())


def test_impulse_helpers():
    w = rn.distinct_weights(128, 64, 3, fixed_axis=1)
    assert w.shape == (128, 64, 3, 3) and all(w[:, c].unique().numel() == 128 * 9 for c in (0, 63))
    w = rn.distinct_weights(64, 128, 3, fixed_axis=0)
    assert w.shape == (64, 128, 3, 3) and all(w[o].unique().numel() == 128 * 9 for o in (0, 63))
    x = rn.impulse((3, 128, 11, 9), 256, 64)
    assert int((x != 0).sum()) == 1 and float(x[2, 64, 6, 4]) == 1.3984375  # 256 = 2 * 99 + 6 * 9 + 4
    # one product per output: the fp64 reference rounds to the exact answer
    ref, extra = rn.conv_fwd_ref64(x, rn.distinct_weights(64, 128, 3, fixed_axis=1))
    assert int((ref != 0).sum()) == 64 * 9 and float(extra[ref == 0].max()) == 0
