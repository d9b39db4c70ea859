"""The GEMM / weight-gradient / GELU / embedding-gradient budgets of tests/gemm_numerics.py tested on themselves, on the
CPU and never with a kernel: honest fp32 torch implementations stay inside every budget (worst error / bound printed as
`NUMERICS gemm-cpu` lines under `pytest -s`), and each seeded defect is rejected; each defect's test also states what the
older tolerance (tests/test_gpt2_ops_gpu.py, tests/test_kernels_gpu.py) makes of it on the same data."""
import pytest
import torch
import torch.nn.functional as F

import gemm_numerics as gm
import gpt2_numerics as gn

BF = torch.bfloat16
OLD_SHAPES = [(300, 264, 64), (257, 200, 192), (64, 776, 768), (32, 256, 3072)]  # (M, N, K)


def note(what, **ratios):
    print(f"NUMERICS gemm-cpu | {what} | " + " | ".join(f"{k} {v:.3f}" for k, v in ratios.items()))


def rejected(fn):
    with pytest.raises(gn.Budget):
        fn()


# ------------------------------------------------------------------------------------------------
# GEMM
@pytest.mark.parametrize("M,N,K", OLD_SHAPES + [(255, 184, 64), (64, 136, 320)])
def test_honest_fp32_gemm_is_inside_the_budget(M, N, K):
    out = {}
    for family in gm.GEMM_FAMILIES:
        A, B, bias, _ = gm.gemm_inputs(family, M, N, K, seed=M + K)
        for order in ("library", "ksteps", "reverse"):
            ref, mag = gm.gemm_ref64(A, B)
            r0 = gm.check_gemm(gm.gemm_fp32(A, B, order=order), ref, mag, K, name=f"{family} {order}")
            ref, mag = gm.gemm_ref64(A, B, bias)
            r1 = gm.check_gemm(gm.gemm_fp32(A, B, bias, order=order), ref, mag, K, name=f"{family} {order} + bias")
            out[f"{family[:6]} {order}"] = max(r0, r1)
            assert 0.5 <= max(r0, r1) <= 1.0  # the half ulp dominates and is reached
    note(f"gemm fp32 {(M, N, K)}", **out)


@pytest.mark.parametrize("M,N,K", OLD_SHAPES)
def test_double_rounded_bias_is_rejected(M, N, K):
    """bf16(bf16(acc) + bias), the class of defect the convolution's addend had. Older tolerance: accepted."""
    A, B, bias, _ = gm.gemm_inputs("random sign", M, N, K, seed=M + K)
    C = gm.gemm_fp32(A, B, bias, double_round=True)
    ref, mag = gm.gemm_ref64(A, B, bias)
    rejected(lambda: gm.check_gemm(C, ref, mag, K))
    assert gm.old_gemm_accepts(C, A, B, bias)


@pytest.mark.parametrize("M,N,K", [s for s in OLD_SHAPES if s[2] > 64])
def test_bf16_accumulator_between_ksteps_is_rejected(M, N, K):
    """The accumulator rounded to bf16 after every 64-deep K-step. Older tolerance: accepted on random-sign inputs."""
    A, B, bias, _ = gm.gemm_inputs("random sign", M, N, K, seed=M + K)
    C = gm.gemm_fp32(A, B, order="ksteps", acc_bf16=True)
    ref, mag = gm.gemm_ref64(A, B)
    rejected(lambda: gm.check_gemm(C, ref, mag, K))
    assert gm.old_gemm_accepts(C, A, B)


@pytest.mark.parametrize("M,N,K", [(300, 264, 192), (64, 776, 768)])
def test_lost_last_k_and_shifted_last_row_are_rejected(M, N, K):
    """The last k lost on the last 8 columns, and row M - 1 stored into row M - 2. The older tolerance rejects both on
    this data, the first only through its largest products (a typical lost product, 0.1, is under its atol of 1e-2
    max|C|: most of the affected elements pass it, all of them fail the budget's extra of (K + 8) 2^-24 |A| |B|)."""
    A, B, _, _ = gm.gemm_inputs("random sign", M, N, K, seed=M + K)
    ref, mag = gm.gemm_ref64(A, B)
    C = gm.gemm_defect_last_k(A, B)
    rejected(lambda: gm.check_gemm(C, ref, mag, K))
    assert not gm.old_gemm_accepts(C, A, B)
    err = (C.double() - ref).abs()[:, -8:]
    old_ok = err <= 1e-2 * float(ref.abs().max()) + 1e-2 * ref.abs()[:, -8:]
    new_ok = err <= (0.5 * gn.ulp_bf16(ref) + gm.gemm_extra(mag, K))[:, -8:]
    assert float(old_ok.double().mean()) > 0.5 > 0.25 > float(new_ok.double().mean())
    C = gm.gemm_defect_row_shift(A, B)
    rejected(lambda: gm.check_gemm(C, ref, mag, K))
    assert not gm.old_gemm_accepts(C, A, B)


def test_selectors_pin_every_k():
    """One-hot rows give the other operand's elements bit for bit; a k index off by one anywhere shows."""
    M, N, K = 70, 24, 128
    _, B, _, _ = gm.gemm_inputs("random sign", M, N, K, seed=1)
    S = gm.selector_rows(M, K)
    want = gm.selector_expected(S, B)
    assert torch.equal(gm.gemm_fp32(S, B).to(BF), want)
    assert float(want[4::5].float().abs().max()) == 0 and float(want[0].float().abs().max()) > 0
    assert {int(gm.selector_k(m, K)) for m in range(K)} == set(range(K))  # 7 is coprime to K: every k is selected
    assert not torch.equal(gm.gemm_fp32(S, torch.roll(B, 1, 1)).to(BF), want)


def test_dgelu_epilogue_budget_holds_for_its_rounding_model():
    """Epilogue 6, bf16(gelu'(U) * bf16(acc)), modelled in fp32; the same with the accumulator's rounding moved to after
    a wrong derivative (gelu' without its second term) is rejected."""
    M, N, K = 64, 136, 192
    A, B, _, U = gm.gemm_inputs("random sign", M, N, K, seed=2)
    ref, extra = gm.dgelu_epilogue_budget(A, B, U)
    acc = gm.gemm_fp32(A, B)
    r = gn.check_elementwise(gm.gelu_grad_fp32(acc, U), ref, extra=extra, bf16=True, name="epi 6")
    note("dgelu epilogue model", ratio=r)
    rejected(lambda: gn.check_elementwise(gm.gelu_grad_fp32(acc, U, second_term=False), ref, extra=extra, bf16=True))


# ------------------------------------------------------------------------------------------------
# weight gradient
@pytest.mark.parametrize("T,M,N", [(1, 8, 8), (65, 24, 16), (1088, 8, 8), (2112, 264, 136)])
def test_honest_fp32_wgrad_is_inside_the_budget(T, M, N):
    out = {}
    splits, tps = gm.wgrad_splits(M, N, T)
    for family in ("random sign", "positive"):
        gy, x, ow, ob = gm.wgrad_inputs(family, T, M, N, seed=T + M)
        ref = gm.wgrad_ref64(gy, x, ow, ob)
        ex = gm.wgrad_extras(ref, T, splits, gm.wgrad_bias_parts(M, N, T))
        model = gm.wgrad_model(gy, x, ow, splits, tps)
        for name, got in (("ksteps", model), ("reverse", gm.wgrad_model(gy, x, ow, splits, tps, reverse=True)),
                          ("library", gn.rbf(ow.float() + gy.float().t() @ x.float()))):
            r = gn.check_elementwise(got, ref["gw"], extra=ex["gw"], bf16=True, name=f"gw {name}")
            _, rms = gn.check_grouped(got, model, ref["gw"], name=f"gw {name} grouped")
            out[f"{family[:6]} {name}"] = r
            out[f"{family[:6]} {name} rms"] = rms
        gb = gn.rbf(ob.float() + gy.float().sum(0))
        out[f"{family[:6]} gb"] = gn.check_elementwise(gb, ref["gb"], extra=ex["gb"], bf16=True, name="gb")
    note(f"wgrad fp32 {(T, M, N)} splits {splits}", **out)


def test_wgrad_splits_follow_the_kernel_rule():
    assert gm.wgrad_splits(8, 8, 1023) == (1, 1024) and gm.wgrad_splits(8, 8, 1024) == (2, 512)
    assert gm.wgrad_splits(8, 8, 1088) == (2, 576)  # a ragged second split of 512 tokens
    assert gm.wgrad_splits(264, 136, 2112) == (4, 576) and gm.wgrad_splits(520, 136, 2112) == (4, 576)
    T, M, N = gm.WGRAD_WAVES_SHAPE
    assert gm.wgrad_splits(M, N, T, 1)[0] == 3 and gm.wgrad_splits(M, N, T, 2)[0] == 4
    assert gm.wgrad_bias_parts(264, 136, 2112) == 8 and gm.wgrad_bias_parts(264, 136, 2112, dma=False) == 4
    assert gm.impulse_tokens(2112, 4, 576) == [0, 63, 64, 575, 576, 1151, 1152, 1727, 1728, 2111]


def test_wgrad_missing_kstep_at_a_split_edge_is_rejected():
    """The first K-step of the second split left out. New shapes (T <= 2112): rejected elementwise. The older tolerance
    2^-7 (|gy|^T |x| + |old|): at T = 16384 it is about 0.64 of the output's standard deviation and accepts the defect
    (worst element about 0.4 of the tolerance); at T = 2112 it rejects it, through a few elements."""
    T, M, N = 2112, 264, 136
    splits, tps = gm.wgrad_splits(M, N, T)
    gy, x, ow, ob = gm.wgrad_inputs("random sign", T, M, N, seed=5)
    ref = gm.wgrad_ref64(gy, x, ow, ob)
    ex = gm.wgrad_extras(ref, T, splits, splits)
    bad = gm.wgrad_model(gy, x, ow, splits, tps, drop_kstep=(1, 0))
    rejected(lambda: gn.check_elementwise(bad, ref["gw"], extra=ex["gw"], bf16=True))
    rejected(lambda: gn.check_grouped(bad, gm.wgrad_model(gy, x, ow, splits, tps), ref["gw"]))
    assert not gm.old_wgrad_accepts(bad, ref)
    T, M, N = 16384, 64, 64
    splits, tps = gm.wgrad_splits(M, N, T)
    gy, x, ow, ob = gm.wgrad_inputs("random sign", T, M, N, seed=6)
    ref = gm.wgrad_ref64(gy, x, ow, ob)
    bad = gm.wgrad_model(gy, x, ow, splits, tps, drop_kstep=(1, 0))
    tol = 2.0 ** -7 * ref["gw_mag"]
    worst = float(((bad.double() - ref["gw"]).abs() / tol).max())
    rel_std = float(tol.mean() / ref["gw"].std())
    note("old wgrad tolerance at T = 16384", tolerance_over_std=rel_std, dropped_kstep_worst=worst)
    assert gm.old_wgrad_accepts(bad, ref) and 0.5 < rel_std < 0.8 and worst < 0.7
    honest = gm.wgrad_model(gy, x, ow, splits, tps)
    r = gn.check_elementwise(honest, ref["gw"], extra=gm.wgrad_extras(ref, T, splits, splits)["gw"], bf16=True)
    note("honest fp32 wgrad at T = 16384", ratio=r)
    assert r < 0.25  # the fp32 term has outgrown the half ulp: why the GPU shapes keep T <= 2112 and add the RMS check


def test_wgrad_slabs_added_in_bf16_are_rejected():
    """Each split's slab rounded to bf16 and added in bf16. Older tolerance: accepted."""
    T, M, N = 2112, 264, 136
    splits, tps = gm.wgrad_splits(M, N, T)
    gy, x, ow, ob = gm.wgrad_inputs("random sign", T, M, N, seed=7)
    ref = gm.wgrad_ref64(gy, x, ow, ob)
    bad = gm.wgrad_model(gy, x, ow, splits, tps, slabs_bf16=True)
    rejected(lambda: gn.check_elementwise(bad, ref["gw"], extra=gm.wgrad_extras(ref, T, splits, splits)["gw"], bf16=True))
    rejected(lambda: gn.check_grouped(bad, gm.wgrad_model(gy, x, ow, splits, tps), ref["gw"]))
    assert gm.old_wgrad_accepts(bad, ref)


def test_wgrad_impulse_is_one_product():
    T, M, N = 1088, 8, 16
    splits, tps = gm.wgrad_splits(M, N, T)
    gy, x, ow, ob = gm.wgrad_inputs("random sign", T, M, N, seed=8)
    for t0 in gm.impulse_tokens(T, splits, tps):
        g1 = torch.zeros_like(gy)
        g1[t0] = gy[t0]
        want = gn.rbf(ow.float() + g1[t0].float()[:, None] * x[t0].float()[None, :])
        assert torch.equal(gm.wgrad_model(g1, x, ow, splits, tps), want)
        k = (t0 - (t0 // tps) * tps) // gm.TK
        assert not torch.equal(gm.wgrad_model(g1, x, ow, splits, tps, drop_kstep=(t0 // tps, k)), want)


# ------------------------------------------------------------------------------------------------
# embedding backward
@pytest.mark.parametrize("B,S,C,V", gm.EMB_SHAPES)
def test_embedding_gradient_budget_and_overwrite_defect(B, S, C, V):
    """Honest fp32 sums pass; `=` for `+=` is rejected. The older test adds into zeroed gradients at atol 2e-2, where the
    two are the same computation: accepted."""
    tok, gout, ow, op = gm.embedding_inputs(B, S, C, V, seed=B + S)
    ref = gm.embedding_bwd_ref64(tok, gout, ow, op)
    gw, gp = gm.embedding_bwd_fp32(tok, gout, ow, op)
    a, b = gm.check_embedding_bwd(gw, gp, ref, ow, op, S)
    note(f"embedding fp32 {(B, S, C, V)}", wte=a, wpe=b)
    gw, gp = gm.embedding_bwd_fp32(tok, gout, ow, op, overwrite=True)
    rejected(lambda: gn.check_elementwise(gw, ref["gw"], extra=ref["gw_extra"], bf16=True))
    rejected(lambda: gn.check_elementwise(gp, ref["gp"], extra=ref["gp_extra"], bf16=True))
    z = torch.zeros_like(ow), torch.zeros_like(op)
    a0, b0 = gm.embedding_bwd_fp32(tok, gout, *z)
    a1, b1 = gm.embedding_bwd_fp32(tok, gout, *z, overwrite=True)
    assert torch.equal(a0, a1) and torch.equal(b0, b1)  # into zeroed gradients the defect is invisible


# ------------------------------------------------------------------------------------------------
# GELU
def test_honest_fp32_gelu_is_inside_the_budget():
    x = gm.all_bf16()
    assert x.numel() == 2 * (0x4280 + 1)  # every pattern from +-0 to +-64
    out = {"fwd": gm.check_gelu_fwd(gm.gelu_fp32(x), x)}
    for gy in (1.0, -0.37, 3.0):
        g = torch.full_like(x, gy)
        out[f"bwd gy={gy}"] = gm.check_gelu_bwd(gm.gelu_grad_fp32(g, x), g, x)
    # the fp32 part alone: the unrounded fp32 values against the derived fp32 terms (no half ulp)
    ref, extra = gm.gelu_fwd_budget(x)
    out["fwd fp32 part"] = gn.check_elementwise(gm.gelu_fp32(x, bf16=False), ref, extra=extra, bf16=False)
    g = torch.ones_like(x)
    ref, extra = gm.gelu_bwd_budget(g, x)
    out["bwd fp32 part"] = gn.check_elementwise(gm.gelu_grad_fp32(g, x, bf16=False), ref, extra=extra, bf16=False)
    note("gelu fp32, every bf16 with |x| <= 64", **out)


def test_gelu_zero_below_minus_three_is_rejected():
    """y = 0 for x < -3 (gelu(-3) = -0.0036). Older tolerance rtol = atol = 1e-2 against F.gelu: accepted."""
    x = gm.all_bf16()
    y = gm.gelu_fp32(x, zero_below=-3.0)
    rejected(lambda: gm.check_gelu_fwd(y, x))
    old = F.gelu(x.float(), approximate="tanh")
    assert bool(((y - old).abs() <= 1e-2 + 1e-2 * old.abs()).all())


def test_gelu_grad_without_second_term_is_rejected():
    """gx = gy s. Older tolerance: rejected as well (the term reaches 0.6 near |x| = 1.5)."""
    x = gm.all_bf16()
    g = torch.ones_like(x)
    gx = gm.gelu_grad_fp32(g, x, second_term=False)
    rejected(lambda: gm.check_gelu_bwd(gx, g, x))
    xr = x.float().requires_grad_(True)
    F.gelu(xr, approximate="tanh").backward(g.float())
    assert not bool(((gx - xr.grad).abs() <= 1e-2 + 1e-2 * xr.grad.abs()).all())


def test_tanh_form_float64_reference_is_unusable_below_minus_six():
    x = torch.tensor([-7.1875, -6.5, -8.0, -10.0], dtype=BF)
    good, tanh = gm.gelu_ref64(x), gm.gelu_tanh_ref64(x)
    rel = ((tanh - good) / good).abs()
    assert float(rel[0]) > 0.25 and float(rel[2]) == 1.0  # 1 + tanh u cancels; from x = -8 it is 0
    fp32 = x.float() / (1 + torch.exp(-2 * (gm.GELU_BETA * (x.float() + gm.GELU_KAPPA * x.float() ** 3))))
    assert float(((fp32.double() - good) / good).abs().max()) < 2.0 ** -14  # the fp32 kernel formula is far closer
    xs = gm.all_bf16()
    xs = xs[xs.float() > -5]
    assert float((gm.gelu_tanh_ref64(xs) - gm.gelu_ref64(xs)).abs().max()) < 1e-15  # above it the two forms agree
