"""The GPT-2 bf16 GEMMs (gemm_bf16.hip: every kernel variant and epilogue), the weight gradient (gemm_bf16_wgrad.hip: both
main loops, token splits, the fused bias gradient), the tanh-GELU kernels and the embedding backward (gpt2_ops.hip), and
ops.linear's Linear / lm_head, against float64 references with derived error budgets (tests/gemm_numerics.py,
docs/NUMERICS.md "GPT-2 GEMMs, GELU, embedding gradient"). The references run on the device with torch. Each check prints
its budget use (`NUMERICS gemm ...`, shown by `pytest -s`). Knobs are set through `knobs(...)`, which restores them."""
import contextlib

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no ROCm GPU", allow_module_level=True)

import gemm_numerics as gm  # noqa: E402
import gpt2_numerics as gn  # noqa: E402
from simple_distributed_machine_learning_amd import _native  # noqa: E402

DEV = torch.device("cuda", 0)
K = _native.kernels()
BF = torch.bfloat16


def note(what, **ratios):
    print(f"NUMERICS gemm | {what} | " + " | ".join(f"{k} {v:.3f}" for k, v in ratios.items()))


@contextlib.contextmanager
def knobs(**kw):
    try:
        for name, value in kw.items():
            K.set_knob(name, value)
        yield
    finally:
        K.reset_knobs()


# =====================================================================================================================
# gemm_bf16
# name -> (knobs, b_kn, needs K >= 128)
VARIANTS = {
    "default": ({}, False, False),
    "n192=0": ({"GEMM_BF16_N192": 0}, False, False),
    "n192=1": ({"GEMM_BF16_N192": 1}, False, False),
    "persist n192=0": ({"GEMM_BF16_PERSIST": 1, "GEMM_BF16_N192": 0}, False, True),
    "persist n192=1": ({"GEMM_BF16_PERSIST": 1, "GEMM_BF16_N192": 1}, False, True),
    "tr=0 n192=0": ({"GEMM_BF16_TR": 0, "GEMM_BF16_N192": 0}, False, False),
    "tr=0 n192=1": ({"GEMM_BF16_TR": 0, "GEMM_BF16_N192": 1}, False, False),
    "2phase": ({"GEMM_BF16_2PHASE": 1}, False, False),
    "w4": ({"GEMM_BF16_W4": 1}, False, False),
    "t2": ({"GEMM_BF16_T2": 1}, False, False),
    "nn": ({}, True, False),
}
MULTI_TILE = [s for s in gm.GEMM_SHAPES if s[0] > 256 or s[1] > 192]
for _g in (0, 2):  # the tile order, on the shapes with more than one tile
    VARIANTS[f"group_m={_g}"] = ({"GEMM_GROUP_M": _g}, False, False)
    VARIANTS[f"group_m={_g} n192=1"] = ({"GEMM_GROUP_M": _g, "GEMM_BF16_N192": 1}, False, False)
    VARIANTS[f"group_m={_g} nn"] = ({"GEMM_GROUP_M": _g}, True, False)
GEMM_CASES = [(s, v) for v, (_, _, k128) in VARIANTS.items() for s in gm.GEMM_SHAPES
              if (not k128 or s[2] >= 128) and (not v.startswith("group_m") or s in MULTI_TILE)]

_REFS = {}


def gemm_case(family, shape):
    """Inputs and float64 references of one (family, shape), computed once on the device and left unchanged."""
    key = (family,) + tuple(shape)
    if key not in _REFS:
        M, N, Kd = shape
        A, B, bias, U = gm.gemm_inputs(family, M, N, Kd, seed=M + N + Kd, device=DEV)
        c = {"A": A, "B": B, "Bkn": B.t().contiguous(), "bias": bias, "U": U}
        c["ref0"], c["mag0"] = gm.gemm_ref64(A, B)
        c["ref1"], c["mag1"] = gm.gemm_ref64(A, B, bias)
        c["ref6"], c["extra6"] = gm.dgelu_epilogue_budget(A, B, U)
        _REFS[key] = c
    return _REFS[key]


def run_gemm(A, c, b_kn, epi, bias=None, aux=None):
    return K.gemm_bf16(A, c["Bkn"] if b_kn else c["B"], bias, b_kn, epi, aux)


@pytest.mark.parametrize("shape,variant", GEMM_CASES, ids=[f"{'x'.join(map(str, s))}-{v.replace(' ', '_')}"
                                                            for s, v in GEMM_CASES])
def test_gemm_bf16_budget(shape, variant):
    """Every epilogue of one kernel variant at one shape, three input families: epilogues 0 and 1 within the budget,
    5 / 7 / 8 tied bit for bit to epilogue 1 / 0 and the standalone GELU kernels, 6 within its two-rounding budget and
    equal to the unfused pair. A is a column slice of a NaN-filled buffer with a NaN row after row M - 1."""
    M, N, Kd = shape
    kn, b_kn, _ = VARIANTS[variant]
    for family in gm.GEMM_FAMILIES:
        c = gemm_case(family, shape)
        Av, Abuf = gm.in_nan_frame(c["A"])
        assert Av.stride(0) % 8 == 0 and Av.stride(0) > Kd
        with knobs(**kn):
            C0, _ = run_gemm(Av, c, b_kn, 0)
            C1, _ = run_gemm(Av, c, b_kn, 1, c["bias"])
            y5, u5 = run_gemm(Av, c, b_kn, 5, c["bias"])
            y7, a7 = run_gemm(Av, c, b_kn, 7, c["bias"])
            C6, _ = run_gemm(Av, c, b_kn, 6, None, c["U"])
            C8, _ = run_gemm(Av, c, b_kn, 8, None, a7)
        torch.cuda.synchronize()
        name = f"{variant} {shape} {family}"
        assert gm.frame_untouched(Abuf, c["A"]), f"{name}: the frame around A changed"
        out = {"epi0": gm.check_gemm(C0, c["ref0"], c["mag0"], Kd, name=f"{name} epi 0"),
               "epi1": gm.check_gemm(C1, c["ref1"], c["mag1"], Kd, name=f"{name} epi 1"),
               "epi6": gn.check_elementwise(C6, c["ref6"], extra=c["extra6"], bf16=True, name=f"{name} epi 6")}
        assert torch.equal(u5, C1), f"{name}: epi 5 U"
        assert torch.equal(y5, K.gelu_fwd_bf16(u5)), f"{name}: epi 5 y"
        out["epi5 y"] = gm.check_gelu_fwd(y5, u5, name=f"{name} epi 5 y")
        assert torch.equal(y7, y5), f"{name}: epi 7 y"
        assert torch.equal(a7, K.gelu_bwd_bf16(torch.ones_like(u5), u5, False)), f"{name}: epi 7 aux"
        assert torch.equal(C6, K.gelu_bwd_bf16(C0, c["U"], False)), f"{name}: epi 6 against the unfused pair"
        assert torch.equal(C8, (a7.float() * C0.float()).to(BF)), f"{name}: epi 8"
        note(name, **out)


@pytest.mark.parametrize("shape,variant", GEMM_CASES, ids=[f"{'x'.join(map(str, s))}-{v.replace(' ', '_')}"
                                                            for s, v in GEMM_CASES])
def test_gemm_bf16_selectors_are_exact(shape, variant):
    """One-hot rows of A (k(m) = (7 m + 3) mod K; every fifth row all zero) give C[m][n] == B[n][k(m)] bit for bit, one-hot
    rows of B give C[m][n] == A[m][k(n)]: the k index of every fragment, in every variant and at the ragged shapes."""
    M, N, Kd = shape
    kn, b_kn, _ = VARIANTS[variant]
    c = gemm_case("random sign", shape)
    Sa, Sb = gm.selector_rows(M, Kd, DEV), gm.selector_rows(N, Kd, DEV)
    Sav, Sabuf = gm.in_nan_frame(Sa)
    Av, Abuf = gm.in_nan_frame(c["A"])
    with knobs(**kn):
        Ca, _ = K.gemm_bf16(Sav, c["Bkn"] if b_kn else c["B"], None, b_kn, 0)
        Cb, _ = K.gemm_bf16(Av, Sb.t().contiguous() if b_kn else Sb, None, b_kn, 0)
    torch.cuda.synchronize()
    assert gm.frame_untouched(Sabuf, Sa) and gm.frame_untouched(Abuf, c["A"])
    assert torch.equal(Ca, gm.selector_expected(Sa, c["B"])), f"{variant} {shape}: one-hot rows of A"
    assert torch.equal(Cb, gm.selector_expected(Sb, c["A"]).t()), f"{variant} {shape}: one-hot rows of B"


@pytest.mark.parametrize("persist", [0, 1])
@pytest.mark.parametrize("n192", [0, 1])
def test_gemm_bf16_budget_more_tiles_than_compute_units(persist, n192):
    """(2200, 7432, 128): 9 x 30 = 270 tiles of 256 columns, 9 x 39 = 351 of 192. More than the compute units and no
    multiple of them, so some persistent workgroups take a second tile and some do not."""
    M, N, Kd = gm.PERSIST_SHAPE
    tiles = -(-M // 256) * -(-N // (192 if n192 else 256))
    assert tiles == (351 if n192 else 270)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert tiles > cus and tiles % cus != 0, f"{tiles} tiles on {cus} compute units: choose another N"
    c = _REFS.get("persist")
    if c is None:
        A, B, bias, _ = gm.gemm_inputs("random sign", M, N, Kd, seed=3, device=DEV)
        c = {"A": A, "B": B, "bias": bias}
        c["ref0"], c["mag0"] = gm.gemm_ref64(A, B)
        _REFS["persist"] = c
    Av, Abuf = gm.in_nan_frame(c["A"])
    with knobs(GEMM_BF16_PERSIST=persist, GEMM_BF16_N192=n192):
        C0, _ = K.gemm_bf16(Av, c["B"], None, False, 0)
        C1, _ = K.gemm_bf16(Av, c["B"], c["bias"], False, 1)
    torch.cuda.synchronize()
    assert gm.frame_untouched(Abuf, c["A"])
    b = c["bias"].double()
    r0 = gm.check_gemm(C0, c["ref0"], c["mag0"], Kd, name="epi 0")
    r1 = gm.check_gemm(C1, c["ref0"] + b, c["mag0"] + b.abs(), Kd, name="epi 1")
    note(f"persist={persist} n192={n192} {gm.PERSIST_SHAPE} random sign", epi0=r0, epi1=r1)


# =====================================================================================================================
# wgrad_bf16_
def run_wgrad(gy, x, ow, ob):
    """gw, gb with the fused bias gradient, from operands inside NaN frames; also asserts that the run without the bias
    gradient gives the same gw and that the frames are untouched."""
    gyv, gybuf = gm.in_nan_frame(gy)
    xv, xbuf = gm.in_nan_frame(x)
    gw, gb, gw2 = ow.clone(), ob.clone(), ow.clone()
    K.wgrad_bf16_(gyv, xv, gw, gb)
    K.wgrad_bf16_(gyv, xv, gw2)
    torch.cuda.synchronize()
    assert gm.frame_untouched(gybuf, gy) and gm.frame_untouched(xbuf, x)
    assert torch.equal(gw, gw2), "gw with and without the fused bias gradient"
    return gw, gb


def check_wgrad_case(T, M, N, dma, nfast, waves):
    splits, tps = gm.wgrad_splits(M, N, T, waves)
    parts = gm.wgrad_bias_parts(M, N, T, waves, dma=bool(dma))
    name = f"wgrad {(T, M, N)} dma={dma} nfast={nfast} waves={waves} splits={splits}"
    with knobs(WGRAD_DMA=dma, WGRAD_NFAST=nfast, WGRAD_WAVES=waves):
        for family in ("random sign", "positive"):
            gy, x, ow, ob = gm.wgrad_inputs(family, T, M, N, seed=T + M + N, device=DEV)
            gw, gb = run_wgrad(gy, x, ow, ob)
            ref = gm.wgrad_ref64(gy, x, ow, ob)
            ex = gm.wgrad_extras(ref, T, splits, parts)
            out = {"gw": gn.check_elementwise(gw, ref["gw"], extra=ex["gw"], bf16=True, name=f"{name} {family} gw"),
                   "gb": gn.check_elementwise(gb, ref["gb"], extra=ex["gb"], bf16=True, name=f"{name} {family} gb")}
            model = gm.wgrad_model(gy, x, ow, splits, tps)
            out["gw row"], out["gw rms"] = gn.check_grouped(gw, model, ref["gw"], name=f"{name} {family} gw grouped")
            note(f"{name} {family}", **out)
        # impulses: one non-zero token; every output is old + one product, rounded once
        gy, x, ow, ob = gm.wgrad_inputs("random sign", T, M, N, seed=T + M + N + 1, device=DEV)
        for t0 in gm.impulse_tokens(T, splits, tps):
            g1 = torch.zeros_like(gy)
            g1[t0] = gy[t0]
            gw, gb = run_wgrad(g1, x, ow, ob)
            want = (ow.float() + gy[t0].float()[:, None] * x[t0].float()[None, :]).to(BF)  # (the product is exact in fp32)
            assert torch.equal(gw, want), f"{name}: impulse at token {t0}, gw"
            assert torch.equal(gb, (ob.float() + gy[t0].float()).to(BF)), f"{name}: impulse at token {t0}, gb"


@pytest.mark.parametrize("dma", [1, 0])
@pytest.mark.parametrize("T,M,N", gm.WGRAD_SHAPES, ids=["x".join(map(str, s)) for s in gm.WGRAD_SHAPES])
def test_wgrad_bf16_budget(T, M, N, dma):
    """Both main loops (T % 64 != 0 always runs the staged one) and both tile orders."""
    for nfast in (0, 1):
        check_wgrad_case(T, M, N, dma, nfast, 1)


@pytest.mark.parametrize("waves", [1, 2])
@pytest.mark.parametrize("T,M,N", [gm.WGRAD_SHAPES[-2], gm.WGRAD_WAVES_SHAPE], ids=["2112x264x136", "2112x2056x1032"])
def test_wgrad_bf16_budget_grid_waves(T, M, N, waves):
    """WGRAD_WAVES: at T <= 2112 the split count is capped at 4 by the 8 K-steps a split must keep, so only 9 x 9 tiles
    see it change (3 splits with one grid wave, 4 with two)."""
    check_wgrad_case(T, M, N, 1, 0, waves)


# =====================================================================================================================
# GELU
def gelu_vector(n, offset=0):
    """n values cycling through every bf16 with |x| <= 64, starting at `offset`."""
    x = gm.all_bf16(device=DEV)
    idx = (torch.arange(n, device=DEV) + offset) % x.numel()
    return x[idx]


@pytest.mark.parametrize("n", [8, 2040, 2048, 2056, 65536 + 8])
def test_gelu_budget(n):
    """The 8-per-lane and 2048-per-block edges; at n = 65544 every bf16 bit pattern with |x| <= 64 (both zeros, the
    subnormals) at every gy. The short lengths are windows of that list centred on x = -4 (n = 2040 .. 2056 reach from
    -0.016 to -64, across the zero of gelu' near -0.75, and wrap on into +0 and the positive subnormals)."""
    total = gm.all_bf16().numel()
    assert n < 65536 or n >= total
    x = gelu_vector(n, 0 if n >= total else total // 2 + 0x4080 - n // 2)  # (-0 sits at total / 2, -4 = bits 0x4080 on)
    y = K.gelu_fwd_bf16(x)
    out = {"fwd": gm.check_gelu_fwd(y, x, name=f"gelu n={n}")}
    for gyv in (1.0, -0.37, 3.0):
        gy = torch.full_like(x, gyv)
        gx = K.gelu_bwd_bf16(gy, x, False)
        gx2 = gy.clone()
        assert K.gelu_bwd_bf16(gx2, x, True).data_ptr() == gx2.data_ptr()
        assert torch.equal(gx2, gx) and torch.equal(gy, torch.full_like(x, gyv)), "in-place and copying form"
        out[f"bwd gy={gyv}"] = gm.check_gelu_bwd(gx, gy, x, name=f"gelu' n={n} gy={gyv}")
    # the fp32 part of the budget alone, where the half ulp cannot hide it: errors beyond half an ulp of the output
    ref, extra = gm.gelu_fwd_budget(x)
    over = ((y.double() - ref).abs() - 0.5 * gn.ulp_bf16(ref)).clamp_min(0)
    out["fwd beyond half ulp / fp32 terms"] = float((over / extra).max())
    note(f"gelu n={n}", **out)


def test_gelu_beyond_64():
    """Every finite bf16 with |x| > 64. By the code: s is exactly 1 (x > 0) or 0 (x < 0), so y == x resp. a zero, and
    gelu' is exactly 1 resp. 0 while x * x is finite (|x| < 2^64). From |x| = 2^64 the factor 1 + 3 kappa x^2 is inf and
    meets s (1 - s) = 0: what gelu' gives there is recorded, not promised (PyTorch's formula does the same)."""
    x = gm.bf16_beyond(device=DEV)
    x = torch.cat([x, torch.full(((-x.numel()) % 8,), 128.0, dtype=BF, device=DEV)])
    y = K.gelu_fwd_bf16(x)
    xf = x.float()
    assert bool(torch.isfinite(y.float()).all()), "a finite input gave a non-finite gelu"
    assert torch.equal(y[xf > 0], x[xf > 0]) and bool((y[xf < 0].float() == 0).all())
    gx = K.gelu_bwd_bf16(torch.ones_like(x), x, False).float()
    safe = xf.abs() < 2.0 ** 64
    assert bool((gx[safe & (xf > 0)] == 1).all()) and bool((gx[safe & (xf < 0)] == 0).all())
    far = gx[~safe]
    print(f"NUMERICS gemm | gelu' for |x| >= 2^64 | {far.numel()} values | {int(torch.isnan(far).sum())} NaN | "
          f"{int(torch.isinf(far).sum())} inf | {int((far == 1).sum())} one | {int((far == 0).sum())} zero")


# =====================================================================================================================
# embedding backward
@pytest.mark.parametrize("B,S,C,V", gm.EMB_SHAPES)
def test_embedding_bwd_budget(B, S, C, V):
    """Into non-zero gradients; absent tokens' rows and the wpe rows past S keep their bits."""
    from simple_distributed_machine_learning_amd.ops.transformer import embedding

    tok, gout, ow, op = gm.embedding_inputs(B, S, C, V, seed=B + S, device=DEV)
    wte = torch.zeros(V, C, dtype=BF, device=DEV).requires_grad_(True)
    wpe = torch.zeros(S + 5, C, dtype=BF, device=DEV).requires_grad_(True)
    wte.grad, wpe.grad = ow.clone(), op.clone()
    embedding(tok, wte, wpe).backward(gout)
    torch.cuda.synchronize()
    ref = gm.embedding_bwd_ref64(tok, gout, ow, op)
    a, b = gm.check_embedding_bwd(wte.grad, wpe.grad, ref, ow, op, S, name=f"embedding {(B, S, C, V)}")
    if V > 50:
        assert int(ref["touched"].sum()) < V and int(torch.bincount(tok.reshape(-1)).max()) >= B * S // 3
    note(f"embedding {(B, S, C, V)}", wte=a, wpe=b)


# =====================================================================================================================
# the ops level
def test_linear_budget_two_micro_batches():
    """ops.linear.Linear 96 -> 200 on 3 x 40 rows, two micro-batches into preset gradients: y, dx and each accumulation of
    weight.grad / bias.grad (from the gradient it was actually given) within the budgets of the GEMM and the weight
    gradient."""
    from simple_distributed_machine_learning_amd.ops.linear import Linear

    g = torch.Generator().manual_seed(3)
    lin = Linear(96, 200, bias=True).to(DEV, BF)
    with torch.no_grad():
        lin.weight.copy_(torch.randn(200, 96, generator=g) * 0.1)
        lin.bias.copy_(torch.randn(200, generator=g))
    lin.weight.grad = (torch.randn(200, 96, generator=g) * 0.5).to(DEV, BF)
    lin.bias.grad = torch.randn(200, generator=g).to(DEV, BF)
    w, b = lin.weight.detach(), lin.bias.detach()
    for mb in range(2):
        x = torch.randn(3, 40, 96, generator=g).to(DEV, BF).requires_grad_(True)
        gy = torch.randn(3, 40, 200, generator=g).to(DEV, BF)
        ow, ob = lin.weight.grad.clone(), lin.bias.grad.clone()
        y = lin(x)
        y.backward(gy)
        torch.cuda.synchronize()
        x2, g2 = x.detach().reshape(-1, 96), gy.reshape(-1, 200)
        ref, mag = gm.gemm_ref64(x2, w, b)
        out = {"y": gm.check_gemm(y.detach().reshape(-1, 200), ref, mag, 96, name="Linear y")}
        ref, mag = gm.gemm_ref64(g2, w.t())
        out["dx"] = gm.check_gemm(x.grad.reshape(-1, 96), ref, mag, 200, name="Linear dx")
        ref = gm.wgrad_ref64(g2, x2, ow, ob)
        ex = gm.wgrad_extras(ref, 120, 1, 1)
        out["gw"] = gn.check_elementwise(lin.weight.grad, ref["gw"], extra=ex["gw"], bf16=True, name="Linear weight.grad")
        out["gb"] = gn.check_elementwise(lin.bias.grad, ref["gb"], extra=ex["gb"], bf16=True, name="Linear bias.grad")
        note(f"Linear 96 -> 200, micro-batch {mb}", **out)


def test_lm_head_budget_padded_vocabulary():
    """ops.linear.lm_head at (T, C, V) = (72, 64, 97) in FlatParams' row-padded storage (Vp = 128): logits on the real
    columns, dx and the padded weight gradient within budget; pad columns of the logits and pad rows of the gradient are
    exact zeros."""
    from simple_distributed_machine_learning_amd.ops.linear import lm_head
    from simple_distributed_machine_learning_amd.ops.transformer import cross_entropy_sum
    from simple_distributed_machine_learning_amd.utils.flat import FlatParams

    T, C, V = 72, 64, 97
    g = torch.Generator().manual_seed(V)
    head = torch.nn.Linear(C, V, bias=False)
    head.flat_row_multiple = {"weight": 64}
    with torch.no_grad():
        head.weight.copy_(torch.randn(V, C, generator=g) * 0.02)
    flat = FlatParams([(0, head)], DEV, BF)
    w = head.weight
    Vp = -(-V // 64) * 64
    assert w._sdml_rows_padded == Vp and w.grad is not None
    old = (torch.randn(V, C, generator=g) * 0.01).to(DEV, BF)
    with torch.no_grad():
        w.grad.copy_(old)
    x = torch.randn(T, C, generator=g).to(DEV, BF).requires_grad_(True)
    tgt = torch.randint(0, V, (T,), generator=g).to(DEV)
    logits = lm_head(x, w)
    assert type(logits.grad_fn).__name__.startswith("_LMHeadFn") and logits.stride() == (Vp, 1)
    wd, xd = w.detach(), x.detach()
    ref, mag = gm.gemm_ref64(xd, wd)
    out = {"logits": gm.check_gemm(logits.detach(), ref, mag, C, name="lm_head logits")}
    assert int((logits.detach().as_strided((T, Vp), (Vp, 1))[:, V:] != 0).sum()) == 0
    _, _, _, gl = cross_entropy_sum(logits.detach(), tgt, 1.0 / T, True)
    assert gl.stride() == (Vp, 1)
    torch.autograd.backward(logits, gl)
    torch.cuda.synchronize()
    ref, mag = gm.gemm_ref64(gl, wd.t())
    out["dx"] = gm.check_gemm(x.grad, ref, mag, Vp, name="lm_head dx")
    gw = flat.grads[:Vp * C].view(Vp, C)
    ref = gm.wgrad_ref64(gl, xd, old, torch.zeros(V, device=DEV))
    out["gw"] = gn.check_elementwise(gw[:V], ref["gw"], extra=gm.wgrad_extras(ref, T, 1, 1)["gw"], bf16=True,
                                     name="lm_head weight.grad")
    assert int((gw[V:] != 0).sum()) == 0 and int((flat.params[V * C:Vp * C] != 0).sum()) == 0
    note(f"lm_head {(T, C, V)}", **out)
