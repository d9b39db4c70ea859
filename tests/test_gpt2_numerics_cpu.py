"""The GPT-2 numerics checker (tests/gpt2_numerics.py) tested on itself, on the CPU: its margins hold between two honest
implementations, it rejects seeded defects, and the tolerances it replaces accepted two of them."""
import math

import pytest
import torch
import torch.nn.functional as F

import gpt2_numerics as gn

SCALE = 0.125  # 1 / sqrt(64)


def rnd(*shape, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.empty(shape).uniform_(-1, 1, generator=g)


def qkv(B, S, H, amp, seed=0):
    return tuple((rnd(B, S, H, 64, seed=seed + i) * amp).to(torch.bfloat16) for i in range(3))


def attn64_masked(q, k, v, keep):
    """float64 attention with an arbitrary [S, S] keep mask (the seeded mask defects)."""
    s = gn._scores(q.double(), k.double()) * SCALE
    p = torch.softmax(s.masked_fill(~keep, -math.inf), -1)
    return torch.einsum("bhqk,bkhd->bqhd", p, v.double())


def test_ulp_bf16():
    x = torch.tensor([1.0, 1.5, 1.9999, 2.0, 0.75, 3e-3, 0.0, 1e-45], dtype=torch.float64)
    want = [2.0 ** -7, 2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -8, 2.0 ** -16, 2.0 ** -133, 2.0 ** -133]
    assert gn.ulp_bf16(x).tolist() == want
    # rounding to bf16 errs by at most half of it
    v = rnd(4096, seed=1).double() * 7
    assert ((gn.rbf(v.float()).double() - v.float().double()).abs() <= 0.5 * gn.ulp_bf16(v.float())).all()


@pytest.mark.parametrize("amp", [0.1, 1.5, 6.0])
@pytest.mark.parametrize("S", [33, 200, 257, 300, 1024])
def test_direct_and_tiled_attention_models_agree_within_margins(S, amp):
    """Two honest implementations of the same roundings (whole rows, and the kernel's online softmax over 64-key tiles)
    pass the checker against each other, both ways round: the margins are not tighter than that."""
    q, k, v = qkv(1, S, 1, amp, seed=S)
    dout = rnd(1, S, 1, 64, seed=S + 7).to(torch.bfloat16)
    ref = gn.attention_ref64(q, k, v, SCALE, True, dout)
    a = gn.attention_model(q, k, v, SCALE, True, tiled=False)
    b = gn.attention_model(q, k, v, SCALE, True, tiled=True)
    gn.check_grouped(a["y"], b["y"], ref["y"], name="direct vs tiled y")
    gn.check_grouped(b["y"], a["y"], ref["y"], name="tiled vs direct y")
    for m in (a, b):
        gn.check_elementwise(m["lse"], ref["lse"], extra=gn.lse_bound(ref["lse"], S), bf16=False, name="lse")
    # the backward model is a function of the saved y and lse: given one y and either model's lse, it agrees too
    for y in (a["y"], b["y"]):
        ga = gn.attention_model_bwd(q, k, v, y, a["lse2"], dout, SCALE, True)
        gb = gn.attention_model_bwd(q, k, v, y, b["lse2"], dout, SCALE, True)
        for name in ("dq", "dk", "dv"):
            gn.check_grouped(ga[name], gb[name], ref[name], name=f"direct vs tiled lse, {name}")
            gn.check_grouped(gb[name], ga[name], ref[name], name=f"tiled vs direct lse, {name}")


@pytest.mark.parametrize("causal", [True, False])
def test_attention_model_non_causal_and_ragged(causal):
    q, k, v = qkv(2, 129, 3, 1.5, seed=3)
    dout = rnd(2, 129, 3, 64, seed=9).to(torch.bfloat16)
    ref = gn.attention_ref64(q, k, v, SCALE, causal, dout)
    a = gn.attention_model(q, k, v, SCALE, causal, tiled=False)
    b = gn.attention_model(q, k, v, SCALE, causal, dout, tiled=True)
    gn.check_grouped(a["y"], b["y"], ref["y"], name="y")
    ga = gn.attention_model_bwd(q, k, v, b["y"], a["lse2"], dout, SCALE, causal)
    for name in ("dq", "dk", "dv"):
        gn.check_grouped(ga[name], b[name], ref[name], name=name)
    # and the float64 formulas are autograd's
    x = [t.double().requires_grad_(True) for t in (q, k, v)]
    s = gn._scores(x[0], x[1]) * SCALE
    if causal:
        s = s.masked_fill(~gn._causal_mask(129, s.device), -math.inf)
    y = torch.einsum("bhqk,bkhd->bqhd", torch.softmax(s, -1), x[2])
    y.backward(dout.double())
    torch.testing.assert_close(y.detach(), ref["y"], rtol=1e-12, atol=1e-12)
    for t, name in zip(x, ("dq", "dk", "dv")):
        torch.testing.assert_close(t.grad, ref[name], rtol=1e-11, atol=1e-12)


# ---- seeded defects ---------------------------------------------------------------------------------------------
def test_dropped_key_at_tile_boundary_is_rejected_and_old_tolerance_accepted_it():
    S = 1024
    q, k, v = qkv(1, S, 1, 1.5, seed=40)
    ref = gn.attention_ref64(q, k, v, SCALE, True)
    model = gn.attention_model(q, k, v, SCALE, True)
    gn.check_grouped(model["y"], model["y"], ref["y"], name="y")
    keep = gn._causal_mask(S, q.device)
    keep[513:, 512] = False  # key 512 (first of a tile) lost for every later query
    bad = gn.rbf(attn64_masked(q, k, v, keep).float())
    with pytest.raises(gn.Budget):
        gn.check_grouped(bad, model["y"], ref["y"], name="y, key 512 dropped")
    # test_flash_attention_fwd_bwd's forward tolerance passes it
    torch.testing.assert_close(bad, ref["y"].float(), rtol=2e-2, atol=2e-2)


@pytest.mark.parametrize("S", [65, 200])
def test_causal_mask_shifted_by_one_is_rejected(S):
    q, k, v = qkv(1, S, 2, 1.5, seed=41)
    ref = gn.attention_ref64(q, k, v, SCALE, True)
    model = gn.attention_model(q, k, v, SCALE, True)
    for diag in (1, -1):
        keep = torch.ones(S, S, dtype=torch.bool).tril(diag)
        keep[0, 0] = True
        bad = gn.rbf(attn64_masked(q, k, v, keep).float())
        with pytest.raises(gn.Budget):
            gn.check_grouped(bad, model["y"], ref["y"], name="y, mask shifted")


def test_dropped_key_is_rejected_in_the_backward():
    S = 200
    q, k, v = qkv(1, S, 1, 1.5, seed=42)
    dout = rnd(1, S, 1, 64, seed=43).to(torch.bfloat16)
    ref = gn.attention_ref64(q, k, v, SCALE, True, dout)
    model = gn.attention_model(q, k, v, SCALE, True, dout)
    x = [t.double().requires_grad_(True) for t in (q, k, v)]
    keep = gn._causal_mask(S, q.device)
    keep[129:, 128] = False
    attn64_masked(*x, keep).backward(dout.double())
    extra = gn.attention_cancellation_bound(q, k, v, model["y"], dout, ref["p"], SCALE)
    for t, name in zip(x, ("dq", "dk", "dv")):
        with pytest.raises(gn.Budget):
            gn.check_grouped(gn.rbf(t.grad.float()), model[name], ref[name], name=name, fp32_extra=extra.get(name))


@pytest.mark.parametrize("amp", [0.1, 1.5, 6.0])
def test_fp32_cancellation_term_is_small_except_where_the_gradient_vanishes(amp):
    """The additive fp32 term of the dq / dk row budgets (attention_cancellation_bound) is a hundredth of the row
    budget on an ordinary row. It decides only rows whose float64 gradient is zero or tiny, such as the first causal
    query (dS = 0 exactly), where the ulp floor of the row budget is the subnormal spacing."""
    S = 257
    q, k, v = qkv(1, S, 1, amp, seed=S)
    dout = rnd(1, S, 1, 64, seed=S + 7).to(torch.bfloat16)
    ref = gn.attention_ref64(q, k, v, SCALE, True, dout)
    model = gn.attention_model(q, k, v, SCALE, True, dout)
    extra = gn.attention_cancellation_bound(q, k, v, model["y"], dout, ref["p"], SCALE)
    assert not ref["dq"][:, 0].any() and extra["dq"][:, 0].min() > 0
    for name in ("dq", "dk"):
        _, budget, _, _ = gn.grouped_stats(model[name], model[name], ref[name])
        assert (extra[name].amax(-1) / (gn.ROW_MARGIN * budget)).median() < 0.05


@pytest.mark.parametrize("rows,V", [(5, 4096), (4, 50257)])
def test_zeroed_dlogits_are_rejected_and_old_tolerance_accepted_them(rows, V):
    z = (rnd(rows, V, seed=30) * 4).to(torch.bfloat16)
    t = torch.randint(0, V, (rows,), generator=torch.Generator().manual_seed(1))
    ref = gn.cross_entropy_ref64(z, t, 0.5)
    model = gn.cross_entropy_model(z, t, 0.5)
    gn.check_dlogits(model["dlogits"], ref["dlogits"], 0.5)
    gn.check_elementwise(model["loss"], ref["loss"], extra=gn.loss_bound(ref), bf16=False, name="loss")
    # honest fp32 autograd, rounded once, passes too
    zf = z.float().requires_grad_(True)
    (F.cross_entropy(zf, t, reduction="sum") * 0.5).backward()
    gn.check_dlogits(zf.grad.to(torch.bfloat16), ref["dlogits"], 0.5)
    # every non-target entry zero
    onehot = F.one_hot(t, V).bool()
    bad = torch.where(onehot, model["dlogits"], torch.zeros(()))
    with pytest.raises(gn.Budget):
        gn.check_dlogits(bad, ref["dlogits"], 0.5)
    torch.testing.assert_close(bad, zf.grad, rtol=2e-2, atol=2e-3)  # test_cross_entropy_bf16's tolerance passes it
    # one 16-byte vector of one row zero
    bad = model["dlogits"].clone()
    bad[rows - 1, 8:16] = 0
    with pytest.raises(gn.Budget):
        gn.check_dlogits(bad, ref["dlogits"], 0.5)


def test_cross_entropy_reference_ignore_index_and_ties():
    z = torch.tensor([[1.0, 3.0, 3.0, -math.inf], [2.0, 2.0, 2.0, 2.0], [0.0, 1.0, 2.0, 3.0]]).to(torch.bfloat16)
    t = torch.tensor([1, -100, 3])
    ref = gn.cross_entropy_ref64(z, t, 1.0)
    assert ref["count"] == 2 and ref["correct"].tolist() == [1.0, 0.0, 1.0]
    assert ref["loss"][1] == 0 and not ref["dlogits"][1].any() and ref["dlogits"][0, 3] == 0
    want = F.cross_entropy(z.double(), t, reduction="none", ignore_index=-100)
    torch.testing.assert_close(ref["loss"], want, rtol=1e-12, atol=1e-12)
    assert gn.cross_entropy_ref64(z, torch.tensor([2, 0, 3]), 1.0, ignore_index=0)["correct"].tolist() == [0.0, 0.0, 1.0]


@pytest.mark.parametrize("rows,D", [(5, 64), (3, 520), (7, 4096)])
def test_layernorm_dx_without_xhat_term_is_rejected(rows, D):
    x = (rnd(rows, D, seed=31) * 3 + 0.5).to(torch.bfloat16)
    w = (1 + 0.1 * rnd(D, seed=32)).to(torch.bfloat16)
    b = (0.1 * rnd(D, seed=33)).to(torch.bfloat16)
    gy = rnd(rows, D, seed=34).to(torch.bfloat16)
    gadd = rnd(rows, D, seed=35).to(torch.bfloat16)
    ref_f, ref_b = gn.layernorm_ref64(x, w, b, 1e-5), gn.layernorm_bwd_ref64(x, w, gy, 1e-5, gadd)
    mod_f, mod_b = gn.layernorm_model(x, w, b, 1e-5), gn.layernorm_bwd_model(x, w, gy, 1e-5, gadd)
    # honest fp32 autograd passes against the model
    xr, wr, br = (t.float().requires_grad_(True) for t in (x, w, b))
    yr = F.layer_norm(xr, (D,), wr, br, 1e-5)
    yr.backward(gy.float())
    gn.check_grouped(gn.rbf(yr.detach()), mod_f["y"], ref_f["y"], name="y")
    gn.check_grouped(gn.rbf(xr.grad + gadd.float()), mod_b["dx"], ref_b["dx"], name="dx")
    bounds = gn.layernorm_fp32_bounds(x, w, gy, 1e-5)
    gn.check_elementwise(wr.grad, ref_b["dw"], extra=bounds["dw"], bf16=False, name="dw")
    gn.check_elementwise(br.grad, ref_b["db"], extra=bounds["db"], bf16=False, name="db")
    gn.check_elementwise(mod_f["mean"], ref_f["mean"], extra=bounds["mean"], bf16=False, name="mean")
    gn.check_elementwise(mod_f["rstd"], ref_f["rstd"], extra=bounds["rstd"], bf16=False, name="rstd")
    bad = gn.layernorm_bwd_model(x, w, gy, 1e-5, gadd, drop_xhat_term=True)["dx"]
    with pytest.raises(gn.Budget):
        gn.check_grouped(bad, mod_b["dx"], ref_b["dx"], name="dx without the xhat term")
    # a dw that misses one row
    xh = (x.double() - ref_f["mean"][:, None]) * ref_f["rstd"][:, None]
    with pytest.raises(gn.Budget):
        gn.check_elementwise((ref_b["dw"] - gy[0].double() * xh[0]).float(), ref_b["dw"], extra=bounds["dw"], bf16=False)


@pytest.mark.parametrize("M,N", [(5, 65), (4101, 64)])
def test_column_sum_with_a_skipped_row_is_rejected(M, N):
    gy = rnd(M, N, seed=41).to(torch.bfloat16)
    old = rnd(N, seed=42).to(torch.bfloat16)
    want = old.double() + gn.colsum_ref64(gy)
    good = (old.float() + gy.float().sum(0)).to(torch.bfloat16)
    gn.check_elementwise(good, want, extra=gn.colsum_bound(gy), name="gb")
    bad = (old.float() + gy[:-1].float().sum(0)).to(torch.bfloat16)
    with pytest.raises(gn.Budget):
        gn.check_elementwise(bad, want, extra=gn.colsum_bound(gy), name="gb, last row skipped")


def test_checker_rejects_nan_and_exempts_no_row():
    ref = rnd(4, 8, seed=1).double()
    model = gn.rbf(ref.float())
    got = model.clone()
    got[2, 3] = float("nan")
    with pytest.raises(gn.Budget):
        gn.check_grouped(got, model, ref)
    with pytest.raises(gn.Budget):
        gn.check_elementwise(got, ref)
    got = model.clone()
    got[3, 0] += 0.25  # one element of one row
    with pytest.raises(gn.Budget):
        gn.check_grouped(got, model, ref)
