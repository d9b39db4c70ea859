"""The MLP error-budget checker (tests/mlp_numerics.py) tested on itself, never a kernel: honest fp32 torch
implementations of each engine's kept products must stay inside every derived bound and agree with the rounding model
within the checker's margins, at the GPU tests' shapes and families, and every seeded defect must be rejected there.
docs/NUMERICS.md ("MLP") records the figures these tests print."""
import pytest
import torch

import gpt2_numerics as gn
import mlp_numerics as mn

ORDERS = ["library", "ksteps", "reverse"]


def budget_use(got, model, ref, extra, name):
    e = gn.check_elementwise(got, ref, extra=extra, bf16=False, name=name)
    row, rms = gn.check_grouped(got, model, ref, name=name)
    return e, row, rms


def rejected(got, model, ref, extra):
    """(elementwise rejects, grouped rejects)."""
    out = []
    for f in (lambda: gn.check_elementwise(got, ref, extra=extra, bf16=False),
              lambda: gn.check_grouped(got, model, ref)):
        try:
            f()
            out.append(False)
        except gn.Budget:
            out.append(True)
    return tuple(out)


def report(what, family, uses):
    e, row, rms = (max(u[i] for u in uses) for i in range(3))
    print(f"NUMERICS self-test {what} [{family}]: worst use {e:.3f} row {row:.3f} rms {rms:.3f} over {len(uses)} cases")


X3_ALL_SHAPES = sorted(set(mn.X3_SHAPES + mn.X3_SHAPES_KM))


# ---- gemm_f32x3 ---------------------------------------------------------------------------------
def x3_epilogues(bias, old, cmask):
    return [(0, {}), (0, {"cmask": cmask}), (1, {"bias": bias}), (2, {"bias": bias}), (3, {"old": old})]


@pytest.mark.parametrize("family", mn.FAMILIES)
def test_x3_honest_implementations_fit(family):
    uses = []
    for (M, N, K) in X3_ALL_SHAPES:
        def run(seed):
            A, B, bias, old, cmask, _ = mn.gemm_inputs(family, M, N, K, seed=1000 * seed + M + K)
            passes = mn.x3_passes(A, B)
            model = mn.chain_model(passes, interleave=True)
            kp = mn.x3_passes(A, B, kernel_order=True)
            impls = [mn.honest_fp32(kp, o) for o in ORDERS] + [mn.chain_model(kp, True, group=mn.X3_BK),
                                                                mn.chain_model(kp, True), mn.chain_model(passes, True, reverse=True)]
            d = {}
            for e, (epi, kw) in enumerate(x3_epilogues(bias, old, cmask)):
                d[f"ref{e}"], d[f"extra{e}"] = mn.x3_budget(A, B, epi=epi, **kw)
                d[f"model{e}"] = mn.epilogue(model, epi, **kw)
                for j, acc in enumerate(impls):
                    d[f"got{e}.{j}"] = mn.epilogue(acc, epi, **kw)
            return d

        S = mn.stacked(M, N, run)
        for e in range(5):
            for j in range(6):
                uses.append(budget_use(S[f"got{e}.{j}"], S[f"model{e}"], S[f"ref{e}"], S[f"extra{e}"],
                                       f"x3 {M}x{N}x{K} epilogue case {e} implementation {j}"))
    report("x3", family, uses)
    assert max(u[0] for u in uses) <= 1.0


def test_x3_split_is_exact_and_the_dropped_products_are_bounded():
    g = torch.Generator().manual_seed(1)
    x = torch.randn(4096, generator=g) * torch.exp2(torch.randint(-30, 30, (4096,), generator=g).float())
    hi, mid, lo = (t.double() for t in mn.x3_split(x))
    assert torch.equal(hi + mid + lo, x.double())
    assert (mid.abs() <= 2.0 ** -8 * x.double().abs()).all() and (lo.abs() <= 2.0 ** -17 * x.double().abs()).all()
    y = torch.randn(4096, generator=g)
    yh, ym, yl = (t.double() for t in mn.x3_split(y))
    dropped = mid * yl + lo * ym + lo * yl
    assert (dropped.abs() <= mn.X3_DROP * (x.double() * y.double()).abs()).all()
    assert ((hi.abs() + mid.abs() + lo.abs()) * (yh.abs() + ym.abs() + yl.abs())
            <= mn.X3_TERMS * (x.double() * y.double()).abs()).all()


@pytest.mark.parametrize("M,N,K", X3_ALL_SHAPES)
def test_x3_without_third_order_products_is_rejected(M, N, K):
    """hi lo + lo hi + mid mid is about 2^-16.4 |a b| per term with random sign: inside K 2^-24 |A| |B|^T from K = 68 up
    (today's tolerance accepts it there), far outside the rounding model's error at every shape."""
    def run(seed):
        A, B, *_ = mn.gemm_inputs("random sign", M, N, K, seed=1000 * seed + 3)
        ref, extra = mn.x3_budget(A, B)
        return {"A": A, "ref": ref, "extra": extra, "model": mn.chain_model(mn.x3_passes(A, B), interleave=True),
                "bad": mn.chain_model(mn.x3_passes(A, B, third_order=False), interleave=True)}

    S = mn.stacked(M, N, run)
    bad, model, ref, extra = S["bad"], S["model"], S["ref"], S["extra"]
    A, B, *_ = mn.gemm_inputs("random sign", M, N, K, seed=3)
    bad0 = bad[:M]
    el, gr = rejected(bad, model, ref, extra)
    print(f"NUMERICS defect x3-third-order {M}x{N}x{K}: elementwise {el} grouped {gr} old accepts {mn.old_x3_accepts(bad0, A, B)}")
    assert gr
    assert mn.old_x3_accepts(bad0, A, B) == (K >= 68)


@pytest.mark.parametrize("M,N,K", [s for s in X3_ALL_SHAPES if s[2] % 32])
def test_x3_lost_last_k_is_rejected(M, N, K):
    A, B, *_ = mn.gemm_inputs("random sign", M, N, K, seed=4)
    ref, extra = mn.x3_budget(A, B)
    passes = mn.x3_passes(A, B)
    model = mn.chain_model(passes, interleave=True)
    bad = mn.chain_model(passes, interleave=True, drop=[K - 1])
    assert all(rejected(bad, model, ref, extra))
    assert not mn.old_x3_accepts(bad, A, B)  # (today's bound sees a whole lost product too)


@pytest.mark.parametrize("M,N,K", [X3_ALL_SHAPES[1], X3_ALL_SHAPES[-1]])
def test_mask_ge_for_gt_is_rejected(M, N, K):
    """The family's masks hold exact zeros: `>=` keeps what `>` drops."""
    A, B, _, _, cmask, _ = mn.gemm_inputs("random sign", M, N, K, seed=5)
    assert (cmask == 0).any() and (cmask < 0).any() and (cmask > 0).any()
    ref, extra = mn.x3_budget(A, B, cmask=cmask)
    model = mn.chain_model(mn.x3_passes(A, B), interleave=True)
    bad = mn.epilogue(model, 0, cmask=cmask, relu_ge=True)
    assert all(rejected(bad, mn.epilogue(model, 0, cmask=cmask), ref, extra))


@pytest.mark.parametrize("family", ["random sign", "positive"])
@pytest.mark.parametrize("M,N,K", mn.X3_WGRAD_SHAPES)
def test_x3_weight_gradient_form(M, N, K, family):
    """The weight-gradient form (accumulation over T = K rows into a non-zero gw, in the kernel's splits): the honest
    orders fit; with more than one split, the first K-step of the second split missing is rejected."""
    A, B, _, old, _, amask = mn.gemm_inputs(family, M, N, K, seed=6)
    A = A * (amask > 0)
    splits, kps = mn.x3_pick_splits(M, N, K, True)
    ref, extra = mn.x3_budget(A, B, epi=4, old=old, splits=splits)
    passes = mn.x3_passes(A, B)
    cuts = [s * kps for s in range(1, splits)]
    # the model is one chain over all T: an honest unsplit sum of all-positive terms has 1.37 x the RMS error of a model
    # cut into the kernel's splits (each restarting from zero), so the uncut chain is the safe side
    model = old + mn.chain_model(passes, interleave=True)
    uses = [budget_use(old + acc, model, ref, extra, f"x3 wgrad {M}x{N}x{K}")
            for acc in (mn.honest_fp32(passes, "ksteps"), mn.honest_fp32(passes, "library"),
                        mn.chain_model(passes, True, cuts=cuts, reverse=True))]
    report(f"x3 wgrad {M}x{N}x{K} ({splits} splits)", family, uses)
    assert max(u[0] for u in uses) <= 1.0
    if splits > 1:
        bad = old + mn.chain_model(passes, True, cuts=cuts, drop=range(kps, kps + mn.X3_BK))
        el, gr = rejected(bad, model, ref, extra)
        print(f"NUMERICS defect x3-split-kstep {M}x{N}x{K}: elementwise {el} grouped {gr} "
              f"old accepts {mn.old_assert_close_accepts(bad, ref, 1e-5, 2e-4)}")
        assert el or gr
    rs_ref, rs_extra = mn.rowsum_budget(A, old[:, 0])
    assert gn.check_elementwise(old[:, 0] + A.sum(1), rs_ref, extra=rs_extra, bf16=False) <= 1.0


def test_gemm_f32_budget_holds_for_fp32_orders():
    for (M, N, K) in mn.X3_SHAPES:
        A, B, bias, *_ = mn.gemm_inputs("random sign", M, N, K, seed=7)
        ref, extra = mn.f32_budget(A, B, epi=1, bias=bias)
        assert gn.check_elementwise(A @ B.t() + bias, ref, extra=extra, bf16=False) <= 1.0
        bad = A[:, :-1] @ B[:, :-1].t() + bias
        with pytest.raises(gn.Budget):
            gn.check_elementwise(bad, ref, extra=extra, bf16=False)


# ---- gemm_f16x2 ---------------------------------------------------------------------------------
def test_bound_exp_edges():
    assert mn.bound_exp(0.0) == -100
    assert mn.bound_exp(1.0) == 1 and mn.bound_exp(4.0) == 3 and mn.bound_exp(0.25) == -1
    below = float(torch.nextafter(torch.tensor(4.0), torch.tensor(0.0)))
    assert mn.bound_exp(below) == 2 and mn.bound_exp(3.0) == 2
    assert mn.bound_exp(2.0 ** 127) == 120 and mn.bound_exp(2.0 ** -120) == -100


@pytest.mark.parametrize("family", mn.FAMILIES)
def test_x2_planes_represent_x(family):
    A, B, *_ = mn.gemm_inputs(family, 257, 320, 192, seed=8)
    for x in (A, B):
        hi, lo, s, E = mn.x2_planes(x)
        assert torch.isfinite(hi.float()).all() and float(hi.float().abs().max()) <= 2.0 ** 14
        back = (hi.double() + lo.double()) * s
        use = ((back - x.double()).abs() / mn.x2_rep_bound(x, E)).max()
        assert use <= 1.0, float(use)
        assert (lo.double().abs() <= 2.0 ** -11 * (x.double().abs() / s) + 2.0 ** -25).all()


def test_x2_plane_scale_one_binade_too_small_overflows_loudly():
    """A bound half the true maximum puts x' at 2^15 and above: still finite in fp16 (max 65504); a bound a quarter of it
    overflows hi to inf, which the checker reports (a NaN / inf never passes)."""
    A, B, *_ = mn.gemm_inputs("pow2 max", 256, 256, 64, seed=9)
    ref, extra = mn.x2_budget(A, B)
    E = mn.bound_exp(A.abs().max())
    for short in (1, 2, 3):
        ah, al, sa, _ = mn.x2_planes(A, E=E - short)
        bh, bl, sb, _ = mn.x2_planes(B)
        got = mn.chain_model([(ah, bh), (ah, bl), (al, bh)], interleave=False) * (sa * sb)
        if torch.isfinite(ah.float()).all():
            gn.check_elementwise(got, ref, extra=extra, bf16=False)  # (more bits than needed: still inside)
        else:
            assert short >= 2
            with pytest.raises(gn.Budget):
                gn.check_elementwise(got, ref, extra=extra, bf16=False)
    assert not torch.isfinite(mn.x2_planes(A, E=E - 3)[0].float()).all()


@pytest.mark.parametrize("family", mn.FAMILIES)
def test_x2_honest_implementations_fit(family):
    uses = []
    for (M, N, K) in mn.X2_GEMM_SHAPES:
        A, B, bias, _, cmask, _ = mn.gemm_inputs(family, M, N, K, seed=M + K)
        passes, sc = mn.x2_passes(A, B)
        model = mn.chain_model(passes, interleave=False) * sc
        impls = [mn.honest_fp32(passes, o, kstep=mn.X2_TK) * sc for o in ORDERS] \
            + [mn.chain_model(passes, False, reverse=True) * sc, mn.chain_model(passes, False, group=mn.X2_TK) * sc]
        for epi, kw in ((0, {}), (0, {"cmask": cmask}), (1, {"bias": bias}), (2, {"bias": bias})):
            ref, extra = mn.x2_budget(A, B, epi=epi, **kw)
            m_out = mn.epilogue(model, epi, **kw)
            for acc in impls:
                uses.append(budget_use(mn.epilogue(acc, epi, **kw), m_out, ref, extra, f"x2 {M}x{N}x{K} epi {epi}"))
    report("x2", family, uses)
    assert max(u[0] for u in uses) <= 1.0


@pytest.mark.parametrize("M,N,K", mn.X2_GEMM_SHAPES)
def test_x2_without_lo_hi_is_rejected(M, N, K):
    """A dropped lo hi segment is 2^-12 |a b| per term with random sign: sqrt(K) 2^-12 rms(a b) against today's bound of
    2 (K 2^-24 + 2^-20) |A| |B|^T, which rejects it at these shapes too (the issue expected it to pass at K = 320: it
    does not, here or there)."""
    A, B, *_ = mn.gemm_inputs("random sign", M, N, K, seed=10)
    ref, extra = mn.x2_budget(A, B)
    passes, sc = mn.x2_passes(A, B)
    model = mn.chain_model(passes, interleave=False) * sc
    bad = mn.chain_model(mn.x2_passes(A, B, lo_hi=False)[0], interleave=False) * sc
    el, gr = rejected(bad, model, ref, extra)
    print(f"NUMERICS defect x2-lo-hi {M}x{N}x{K}: elementwise {el} grouped {gr} old accepts {mn.old_x2_accepts(bad, A, B)}")
    assert el and gr
    assert not mn.old_x2_accepts(bad, A, B)


@pytest.mark.parametrize("family", ["random sign", "positive"])
@pytest.mark.parametrize("T,M,N", mn.X2_WGRAD_SHAPES)
def test_x2_weight_gradient(T, M, N, family):
    g = torch.Generator().manual_seed(11)
    dz, x = torch.randn(T, M, generator=g) * 1e-2, torch.randn(T, N, generator=g).relu()
    old_w, old_b = torch.randn(M, N, generator=g), torch.randn(M, generator=g)
    if family == "positive":
        dz, old_w, old_b = dz.abs(), old_w.abs(), old_b.abs()
    ref = mn.x2_wgrad_budget(dz, x, old_w, old_b)
    model = mn.x2_wgrad_model(dz, x, old_w)
    passes, sc = mn.x2_passes(dz.t(), x.t())
    uses = [budget_use(got, model, ref["gw"], ref["gw_extra"], f"x2 wgrad {T}x{M}x{N}")
            for got in (mn.x2_wgrad_model(dz, x, old_w, reverse=True),
                        old_w + mn.honest_fp32(passes, "library") * sc,
                        old_w + mn.honest_fp32(passes, "ksteps", kstep=mn.X2_TK) * sc)]
    report(f"x2 wgrad {T}x{M}x{N}", family, uses)
    assert max(u[0] for u in uses) <= 1.0
    splits, _ = mn.x2_wgrad_splits(M, N, T)
    if splits > 1:
        bad = mn.x2_wgrad_model(dz, x, old_w, drop_kstep=(1, 0))
        el, gr = rejected(bad, model, ref["gw"], ref["gw_extra"])
        print(f"NUMERICS defect x2-wgrad-kstep {T}x{M}x{N}: elementwise {el} grouped {gr}")
        assert el or gr
    # the bias gradient: both honest orders fit, the hi plane alone does not
    gb_model = mn.x2_gb_fp32(dz, old_b)
    for got in (gb_model, mn.x2_gb_fp32(dz, old_b, reverse=True), (old_b.double() + dz.double().sum(0)).float()):
        assert gn.check_elementwise(got, ref["gb"], extra=ref["gb_extra"], bf16=False) <= 1.0
    bad = mn.x2_gb_fp32(dz, old_b, lo=False)
    gr = rejected(bad[None], gb_model[None], ref["gb"][None], ref["gb_extra"][None])
    old_ok = mn.old_assert_close_accepts(bad, ref["gb"], 1e-5, 1e-4)
    print(f"NUMERICS defect x2-gb-hi-only {T}x{M}x{N}: elementwise {gr[0]} grouped {gr[1]} old accepts {old_ok}")
    assert gr[0] or gr[1]
    if family == "random sign":
        assert old_ok == (T == 64)  # today's atol = 1e-4 hides the lo plane's share of a short sum only


# ---- u8_fwd -------------------------------------------------------------------------------------
def test_u8_tail_substeps_reachable():
    """K % 16 == 0 (u8_fwd_supported) leaves 16, 32, 48 or 64 k in the last K-step: 2 or 4 substeps; 1 and 3 cannot be
    reached through linear_fwd_u8."""
    assert [mn.u8_tail_substeps(K) for _, K in mn.U8_FWD_NK] == [2, 4, 4, 4, 2, 2]
    assert {mn.u8_tail_substeps(K) for K in range(16, 2048, 16)} == {2, 4}


@pytest.mark.parametrize("family", mn.PIXEL_FAMILIES)
def test_u8_fwd_honest_implementations_fit(family):
    """Rows are independent in the forward (the row count only selects the kernel's tiling), so the torch
    implementations run 300 rows at each (N, K)."""
    uses, scale = [], 1.0 / 255.0
    for (N, K) in mn.U8_FWD_NK:
        g = torch.Generator().manual_seed(N + K)
        x8 = mn.pixel_inputs(family, 300, K, seed=K)
        w, b = torch.empty(N, K).uniform_(-0.05, 0.05, generator=g), torch.randn(N, generator=g)
        sc, _ = mn.u8_scale(scale)
        passes = mn.u8_fwd_passes(x8, w)
        for relu in (False, True):
            ref, extra = mn.u8_fwd_budget(x8, w, b, scale, relu)
            model = mn.u8_fwd_model(x8, w, b, scale, relu)
            for acc in [mn.honest_fp32(passes, o, kstep=mn.U8_FBK) for o in ORDERS] + [mn.chain_model(passes, True, reverse=True)]:
                y = (acc.double() * sc + b.double()).float()
                uses.append(budget_use(torch.relu(y) if relu else y, model, ref, extra, f"u8 fwd {N}x{K}"))
    report("u8 fwd", family, uses)
    assert max(u[0] for u in uses) <= 1.0


@pytest.mark.parametrize("N,K", mn.U8_FWD_NK)
def test_u8_fwd_defects_are_rejected(N, K):
    g = torch.Generator().manual_seed(12)
    x8 = mn.pixel_inputs("uniform", 300, K, seed=13)
    w, b = torch.empty(N, K).uniform_(-0.05, 0.05, generator=g), torch.randn(N, generator=g)
    ref, extra = mn.u8_fwd_budget(x8, w, b, 1.0 / 255.0, True)
    model = mn.u8_fwd_model(x8, w, b, 1.0 / 255.0, True)
    hi_only = mn.u8_fwd_model(x8, w, b, 1.0 / 255.0, True, lo=False)
    el, gr = rejected(hi_only, model, ref, extra)
    print(f"NUMERICS defect u8-fwd-hi-plane {N}x{K}: elementwise {el} grouped {gr} "
          f"old accepts {mn.old_u8_fwd_accepts(hi_only, x8, w, b)}")
    assert el or gr
    tail = mn.u8_fwd_model(x8, w, b, 1.0 / 255.0, True, drop_last=8)  # the last substep's upper 8 k
    assert all(rejected(tail, model, ref, extra))
    y = mn.u8_fwd_model(x8, w, b, 1.0 / 255.0, True)
    assert (y == 0).any()  # the ReLU output holds exact zeros: relu_bits must read `>`, not `>=`
    assert not torch.equal(mn.relu_bits_of(y), mn.relu_bits_of(y + (y == 0)))


# ---- classifier heads ---------------------------------------------------------------------------
HEAD_DEFECTS = ["clamped rows", "last index", "no max", "overwrite", "dx zero", "lost row", "mask ge"]


def head_rejects(out, ref, h):
    try:
        mn.check_head(out, ref, h)
        return False
    except gn.Budget:
        return True


@pytest.mark.parametrize("C", [2, 10, 16])
def test_head_honest_implementations_fit(C):
    worst = {}
    for family in mn.head_families(C):
        for M in mn.HEAD_ROWS:
            h, w, b, t, ow, ob = mn.head_inputs(family, M, 128, C, seed=M)
            ref = mn.head_budget(h, w, b, t, 1.0 / M, ow, ob)
            for form in ("exp2", "library"):
                out = mn.head_fp32(h, w, b, t, 1.0 / M, ow, ob, form)
                for k, v in mn.check_head(out, ref, h, f"head {family} M {M} C {C} {form}").items():
                    worst[family, k] = max(worst.get((family, k), 0.0), v)
    for family in mn.head_families(C):
        print(f"NUMERICS self-test head C {C} [{family}]: " + " ".join(f"{k} {worst[family, k]:.3f}" for k in ("loss", "dl", "dx", "gw", "gb")))
    assert max(worst.values()) <= 1.0


def defect_cases(defect):
    """(family, M) at which a defect changes an output: every listed row count for most; the rows of a ragged last tile
    for "clamped rows"; the tie families for "last index"; the offset family (exp2 overflows) for "no max"."""
    rows = [M for M in mn.HEAD_ROWS if M % 16] if defect == "clamped rows" else mn.HEAD_ROWS
    fams = {"last index": ["equal", "tie 3 4", "tie 1 9"], "no max": ["offset"],
            "lost row": ["small"]}.get(defect, ["small", "saturated"])  # (a saturated row on target has no loss to lose)
    return [(f, M) for f in fams for M in rows]


@pytest.mark.parametrize("defect", HEAD_DEFECTS)
def test_head_defects_are_rejected(defect):
    old = []
    for family, M in defect_cases(defect):
        h, w, b, t, ow, ob = mn.head_inputs(family, M, 128, 10, seed=M)
        ref = mn.head_budget(h, w, b, t, 1.0 / M, ow, ob)
        assert not head_rejects(mn.head_fp32(h, w, b, t, 1.0 / M, ow, ob), ref, h)
        assert head_rejects(mn.head_fp32(h, w, b, t, 1.0 / M, ow, ob, defect=defect), ref, h), (defect, family, M)
        # today's test, restated: fp32 torch reference, an unmasked dx, gw / gb accumulated into zeros
        z_w, z_b = torch.zeros_like(ow), torch.zeros_like(ob)
        hp = h + 1.0  # (no zeros: today's head test has no mask, so "mask ge" is invisible to it by construction)
        bad = mn.head_fp32(hp if defect == "mask ge" else h, w, b, t, 1.0 / M, z_w, z_b, defect=defect)
        old.append((family, M, mn.old_head_accepts(bad, hp if defect == "mask ge" else h, w, b, t, 1.0 / M, z_w, z_b)))
    print(f"NUMERICS defect head-{defect.replace(' ', '-')}: rejected at {len(old)} cases; old accepts at "
          f"{[(f, M) for f, M, ok in old if ok]}")


# ---- u8_wgrad family and the remaining seeded defects ---------------------------------------------
def wgrad_inputs(M, N, seed):
    g = torch.Generator().manual_seed(seed)
    x8 = mn.pixel_inputs("uniform", M, mn.U8W_K, seed=seed)
    dz = mn.masky((M, N), g) * 1e-3
    return x8, dz, torch.randn(N, mn.U8W_K, generator=g), torch.randn(N, generator=g)


@pytest.mark.parametrize("M,N", [(M, 128) for M in mn.U8W_ROWS] + [(4096, 64), (4128, 64)])
def test_u8_wgrad_honest_orders_fit_and_defects_are_rejected(M, N):
    scale = 1.0 / 255.0
    x8, dz, ow, ob = wgrad_inputs(M, N, M + N)
    E = mn.bound_exp(dz.abs().max())
    splits, rps = mn.u8_wgrad_splits(M, N)
    ref = mn.u8_wgrad_budget(dz, x8, ow, ob, scale, E, splits)
    gw_m, gb_m = mn.u8_wgrad_model(dz, x8, ow, ob, scale, E, splits, rps)
    hi, lo, sd, _ = mn.x2_planes(dz, E=E)
    s32 = float(torch.tensor(scale, dtype=torch.float32))
    lib = ow + ((hi.float().t() @ x8.float() + lo.float().t() @ x8.float()).double() * (s32 * sd)).float()
    uses = [budget_use(got, gw_m, ref["gw"], ref["gw_extra"], f"u8 wgrad {M}x{N}")
            for got in (mn.u8_wgrad_model(dz, x8, ow, ob, scale, E, splits, rps, reverse=True)[0], lib)]
    report(f"u8 wgrad {M}x{N} ({splits} splits)", "uniform", uses)
    assert gn.check_elementwise(gb_m, ref["gb"], extra=ref["gb_extra"], bf16=False) <= 1.0
    defects = {"dz planes without lo": dict(lo=False), "bias added by every split": dict(bias_every_split=True)}
    if splits > 1:
        defects["first K-step of the second split missing"] = dict(drop_kstep=(1, 0))
    for name, kw in defects.items():
        bw, bb = mn.u8_wgrad_model(dz, x8, ow, ob, scale, E, splits, rps, **kw)
        rw = rejected(bw, gw_m, ref["gw"], ref["gw_extra"])
        rb = rejected(bb[None], gb_m[None], ref["gb"][None], ref["gb_extra"][None])
        old = mn.old_u8_wgrad_accepts(bw, ref) and mn.old_assert_close_accepts(bb, ref["gb"], 1e-5, 1e-3)
        print(f"NUMERICS defect u8-wgrad {name} {M}x{N}: gw elementwise {rw[0]} grouped {rw[1]}, gb elementwise {rb[0]} "
              f"grouped {rb[1]}, old accepts {old}")
        if name == "bias added by every split":
            assert (rb[0] or rb[1]) == (splits > 1)
        else:
            assert rw[0] or rw[1], (name, M, N)


@pytest.mark.parametrize("pixels", ["uniform", "all 255"])
def test_u8_wgrad_expanded_dz_fits(pixels):
    """The _dl forms' dz = (dl W2) (h > 0), expanded by an fp32 chain, with its error term e_dz in the budget; also
    with saturated pixels (nothing cancels in the sums over rows)."""
    M, N, C, scale = 1056, 128, 10, 1.0 / 255.0
    g = torch.Generator().manual_seed(8)
    x8 = mn.pixel_inputs(pixels, M, mn.U8W_K, seed=8)
    h = mn.masky((M, N), g).relu()
    dl, w2 = torch.randn(M, C, generator=g) * 1e-3, torch.randn(C, N, generator=g) * 0.1
    ow, ob = torch.randn(N, mn.U8W_K, generator=g), torch.randn(N, generator=g)
    d64, dmodel, e_dz = mn.dz_from_dl(dl, w2, h > 0)
    E = mn.bound_exp(d64.abs().max())
    splits, rps = mn.u8_wgrad_splits(M, N)
    ref = mn.u8_wgrad_budget(d64, x8, ow, ob, scale, E, splits, e_dz=e_dz)
    gw_m, gb_m = mn.u8_wgrad_model(dmodel, x8, ow, ob, scale, E, splits, rps)
    honest = ((dl @ w2) * (h > 0))  # the library's fp32 expansion
    gw_h, gb_h = mn.u8_wgrad_model(honest, x8, ow, ob, scale, E, splits, rps, reverse=True)
    uses = [budget_use(gw_h, gw_m, ref["gw"], ref["gw_extra"], "u8 wgrad dl"),
            budget_use(gb_h[None], gb_m[None], ref["gb"][None], ref["gb_extra"][None], "u8 wgrad dl gb")]
    report("u8 wgrad from dl 1056x128", pixels, uses)


def test_x3_slab_form_lost_kstep_is_rejected():
    """The x3 engine's uint8 weight gradient (slabs in split order): the first K-step of the second split missing."""
    M, N = 4129, 128
    x8, dz, ow, _ = wgrad_inputs(M, N, 3)
    splits, kps = mn.x3_pick_splits(N, mn.U8W_K, M, True)
    cuts = [s * kps for s in range(1, splits)]
    passes = mn.u8x3_wgrad_passes(dz, x8)
    s32 = float(torch.tensor(1.0 / 255.0, dtype=torch.float32))
    ref = mn.u8_wgrad_budget(dz, x8, ow, ow[:, 0], 1.0 / 255.0, None, splits, n_planes=3, rel=0.0)
    model = ow + (mn.chain_model(passes, True, cuts=cuts).double() * s32).float()
    bad = ow + (mn.chain_model(passes, True, cuts=cuts, drop=range(kps, kps + mn.X3_BK)).double() * s32).float()
    assert gn.check_elementwise(model, ref["gw"], extra=ref["gw_extra"], bf16=False) <= 1.0
    el, gr = rejected(bad, model, ref["gw"], ref["gw_extra"])
    print(f"NUMERICS defect x3-slab-kstep {M}x{N}: elementwise {el} grouped {gr} old accepts {mn.old_u8_wgrad_accepts(bad, ref)}")
    assert el or gr


def test_bias_added_by_every_split_is_rejected():
    """x2's bias gradient (partials per split, and per split and column tile) and gemm_f32's skinny split-K (C pre-set
    to the bias once): a version that adds the old gb, or the bias, once per split."""
    g = torch.Generator().manual_seed(4)
    T, M, N = 2112, 256, 128
    dz, x = torch.randn(T, M, generator=g) * 1e-2, torch.randn(T, N, generator=g).relu()
    old_w, old_b = torch.randn(M, N, generator=g), torch.randn(M, generator=g)
    ref = mn.x2_wgrad_budget(dz, x, old_w, old_b)
    splits, _ = mn.x2_wgrad_splits(M, N, T)
    good = mn.x2_gb_fp32(dz, old_b)
    bad = good + (splits - 1) * old_b
    assert splits > 1 and gn.check_elementwise(good, ref["gb"], extra=ref["gb_extra"], bf16=False) <= 1.0
    assert all(rejected(bad[None], good[None], ref["gb"][None], ref["gb_extra"][None]))
    assert not mn.old_assert_close_accepts(bad, ref["gb"], 1e-5, 1e-4)
    A, B, bias, *_ = mn.gemm_inputs("random sign", 512, 256, 320, seed=5)
    sk = mn.f32_skinny_splits(512, 256, 320, 1)
    ref, extra = mn.f32_budget(A, B, epi=1, bias=bias)
    acc = mn.chain_model([(A, B)], True)
    assert sk == 5 and all(rejected(acc + sk * bias, acc + bias, ref, extra))


def test_u8_forward_one_substep_tail_lost_is_rejected():
    """K = 72 leaves 8 k in the last K-step: one substep (not reachable through linear_fwd_u8, whose K is a multiple of
    16; the instantiation exists). Losing it loses k = 64 .. 71."""
    g = torch.Generator().manual_seed(6)
    N, K = 128, 72
    assert mn.u8_tail_substeps(K) == 1
    x8 = mn.pixel_inputs("uniform", 300, K, seed=7)
    w, b = torch.empty(N, K).uniform_(-0.05, 0.05, generator=g), torch.randn(N, generator=g)
    ref, extra = mn.u8_fwd_budget(x8, w, b, 1.0 / 255.0, True)
    model = mn.u8_fwd_model(x8, w, b, 1.0 / 255.0, True)
    assert all(rejected(mn.u8_fwd_model(x8, w, b, 1.0 / 255.0, True, drop_last=8), model, ref, extra))


@pytest.mark.parametrize("M", [255, 2049])
def test_head_dw2_without_the_dl_lo_plane_is_rejected(M):
    """gW2 from the hi plane of dl only: 2^-11 of every term. The elementwise gW2 bound, (3 M + 2048 + 8) u and the dl
    budget, accepts it; the rounding model (given the same dl) does not."""
    h, w, b, t, ow, ob = mn.head_inputs("small", M, 128, 10, seed=M)
    scale = 1.0 / M
    dl = mn.head_fp32(h, w, b, t, scale, ow, ob)["dl"]
    dh, dlo, sd, _ = mn.x2_planes(dl, E=mn.bound_exp(float(torch.tensor(scale, dtype=torch.float32))))
    ref64 = ow.double() + dl.double().t() @ h.double()
    model = ow + mn.chain_model([(dh.t(), h.t()), (dlo.t(), h.t())], True) * sd
    honest = ow + (dh.float().t() @ h + dlo.float().t() @ h) * sd
    bad = ow + mn.chain_model([(dh.t(), h.t())], True) * sd
    gn.check_grouped(honest, model, ref64)
    with pytest.raises(gn.Budget):
        gn.check_grouped(bad, model, ref64)
    budget = mn.head_budget(h, w, b, t, scale, ow, ob)
    el = rejected(bad, model, budget["gw"], budget["gw_extra"])[0]
    print(f"NUMERICS defect head-dw2-hi-plane M {M}: elementwise {el} grouped True")


# ---- heads without a dl output, further families, stats ---------------------------------------------
@pytest.mark.parametrize("family", ["small", "saturated"])
def test_wide_k_head_models_and_partial_losses(family):
    """4096 x 1024 x 10, the wide-K head's shape: honest fp32 heads (the kernel's operations on logits summed by the
    library and by a reversed chain) fit the fp32 budget (planes=False) and agree with the chain models of dx and gW2; a gW2 that loses half a row's contribution (512 of its 1024 columns, a row with a
    real gradient) stays inside the elementwise budget and is rejected by the model."""
    M, K, C = 4096, 1024, 10
    h, w, b, t, ow, ob = mn.head_inputs(family, M, K, C, seed=M)
    scale = 1.0 / M
    ref = mn.head_budget(h, w, b, t, scale, ow, ob, planes=False)
    model = mn.head_chain_models(h, w, b, t, scale, ow)
    for form, z in (("library logits", h @ w.t() + b), ("reversed chain", mn.chain_model([(h, w)], True, reverse=True) + b)):
        out = mn.head_fp32(h, w, b, t, scale, ow, ob, "lse", z=z)
        u = mn.check_head(out, ref, h, f"wide-K {family} {form}")
        rd = gn.check_grouped(out["dx"], model["dx"] * (h > 0), ref["dx"] * (h > 0), fp32_extra=ref["dx_form_extra"])
        rw = gn.check_grouped(out["gw"], model["gw"], ref["gw"])
        print(f"NUMERICS self-test wide-K head [{family}] {form}: " + " ".join(f"{k} {v:.4f}" for k, v in u.items())
              + f" | dx rms {rd[1]:.3f} gw rms {rw[1]:.3f}")
    row = 4095  # (odd: a random target, so the row has a gradient in both families)
    bad = mn.head_chain_models(h, w, b, t, scale, ow, lost=(row, 0, K // 2))["gw"]
    el, gr = rejected(bad, model["gw"], ref["gw"], ref["gw_extra"])
    print(f"NUMERICS defect wide-K half row of dW2 lost [{family}]: elementwise {el} grouped {gr}")
    assert gr


def test_head_stats_overwritten_instead_of_accumulated_is_rejected():
    """`=` for `+=` in the stats: accumulated into (5, 3), the loss comes back without the 5."""
    h, w, b, t, ow, ob = mn.head_inputs("small", 257, 128, 10, seed=1)
    ref = mn.head_budget(h, w, b, t, 1.0 / 257, ow, ob)
    out = mn.head_fp32(h, w, b, t, 1.0 / 257, ow, ob)
    one = lambda v: torch.as_tensor(float(v), dtype=torch.float64).reshape(1)  # noqa: E731
    extra = one(ref["loss_extra"] + 2 * mn.U32 * (5 + abs(float(ref["loss"]))))
    gn.check_elementwise(one(out["loss"] + 5.0), one(ref["loss"] + 5.0), extra=extra, bf16=False)
    with pytest.raises(gn.Budget):
        gn.check_elementwise(one(out["loss"]), one(ref["loss"] + 5.0), extra=extra, bf16=False)
    assert not ref["correct_min"] <= out["correct"] - 3.0 <= ref["correct_max"]  # (the count without its 3)


@pytest.mark.parametrize("family", ["small", "saturated", "equal", "tie 3 4"])
@pytest.mark.parametrize("M", [255, 2049])
def test_head_models_given_dl_fit_honest_orders(M, family):
    """The models of dx and gW2 given dl, against two honest implementations (the library's matmul; the reversed chain)
    in four families."""
    h, w, b, t, ow, ob = mn.head_inputs(family, M, 128, 10, seed=M)
    scale = 1.0 / M
    dl = mn.head_fp32(h, w, b, t, scale, ow, ob)["dl"]
    dh, dlo, sd, _ = mn.x2_planes(dl, E=mn.bound_exp(float(torch.tensor(scale, dtype=torch.float32))))
    passes = [(dh.t(), h.t()), (dlo.t(), h.t())]
    r_gw, r_dx = ow.double() + dl.double().t() @ h.double(), dl.double() @ w.double()
    m_gw, m_dx = ow + mn.chain_model(passes, True) * sd, mn.chain_model([(dl, w.t())], True)
    cancel = 18 * mn.U32 * (dl.double().abs() @ w.double().abs()) if family == "equal" else None
    for gw, dx in ((ow + (dh.float().t() @ h + dlo.float().t() @ h) * sd, dl @ w),
                   (ow + mn.chain_model(passes, True, reverse=True) * sd, mn.chain_model([(dl, w.t())], True, reverse=True))):
        gn.check_grouped(gw, m_gw, r_gw)
        gn.check_grouped(dx, m_dx, r_dx, fp32_extra=cancel)
