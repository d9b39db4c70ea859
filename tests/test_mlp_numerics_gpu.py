"""The MLP kernels that compute fp32-accurate GEMMs on low-precision matrix cores, against float64 references with derived
error budgets (tests/mlp_numerics.py, docs/NUMERICS.md "MLP"): the bf16x3 engine (gemm_f32x3.hip) and the exact fp32
engine (gemm_f32.hip) in every layout and epilogue, the weight-gradient form with masks, row sums and atomics; the
two-fp16-plane engine (gemm_f16x2.hip: the splits, both GEMM forms with their epilogues and per-wave maxima, the weight
and bias gradient in both main loops); the uint8-pixel forward (mlp_u8.hip: every tail, the ReLU bits, the per-wave
maxima, the block geometries, the plane cache); the classifier heads (head_xent.hip: block, VALU, wide-K and generic,
head_dx_from_dlogits, the bounds they return) and the fused uint8 forward + head; the uint8 weight-gradient family
(linear_wgrad_u8, linear_wgrad_u8_dl, their variants, the x3 engine's slab form), fed with the bounds the heads
produce. The references run on the device with torch. Each check prints its
budget use (`NUMERICS mlp ...`, shown by `pytest -s`). Knobs are set through `knobs(...)`, which restores them."""
import contextlib

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no ROCm GPU", allow_module_level=True)

import gpt2_numerics as gn  # noqa: E402
import mlp_numerics as mn  # noqa: E402
from simple_distributed_machine_learning_amd import _native, ops  # noqa: E402

DEV = torch.device("cuda", 0)
K = _native.kernels()
F16 = torch.float16
NAN = float("nan")


def note(what, **ratios):
    print(f"NUMERICS mlp | {what} | " + " | ".join(f"{k} {v:.3f}" for k, v in ratios.items()))


def check(what, got, model, ref, extra):
    """Elementwise budget, then the grouped comparison with the rounding model; prints the use of both."""
    # (a = 1e-300 only keeps the reported ratio defined where a mask makes the bound exactly 0: any fp32 error is larger)
    use = gn.check_elementwise(got, ref, extra=extra, a=1e-300, bf16=False, name=what)
    row, rms = gn.check_grouped(got, model, ref, name=what)
    note(what, use=use, row=row, rms=rms)


@contextlib.contextmanager
def knobs(**kw):
    try:
        for name, value in kw.items():
            K.set_knob(name, value)
        yield
    finally:
        K.reset_knobs()


@contextlib.contextmanager
def f32_engine(exact):
    mode = K.gemm_f32_mode()
    try:
        K.gemm_f32_set_mode(0 if exact else 1)
        yield
    finally:
        K.gemm_f32_set_mode(mode)


def poison(n):
    """Leave a freed NaN block of n floats in the allocator: a binding's torch.empty of that size then starts from NaN
    (most likely), so a slot its kernel does not write shows."""
    t = torch.full((n,), NAN, device=DEV)
    del t


def lay(A, km):
    return A.t().contiguous() if km else A


# =====================================================================================================================
# gemm_f32x3 and gemm_f32: four layouts x epilogues 0-4 (+ cmask)
LAYOUTS = [(False, False), (False, True), (True, False), (True, True)]
X3_CASES = [(s, l) for l in LAYOUTS for s in (mn.X3_SHAPES if l == (False, False) else mn.X3_SHAPES_KM)]
F32_CASES = [(s, l) for l in LAYOUTS for s in mn.X3_SHAPES]
_GEMM = {}


def gemm_case(family, shape):
    """Inputs, references, extras and models of one (family, shape) for both engines, computed once on the device and
    left unchanged; a small shape is n_problems independently seeded problems."""
    key = (family,) + tuple(shape)
    if key not in _GEMM:
        M, N, Kd = shape
        probs = []
        for seed in range(mn.n_problems(M, N)):
            A, B, bias, old, cmask, _ = mn.gemm_inputs(family, M, N, Kd, seed=1000 * seed + M + Kd, device=DEV)
            acc = {"x3": mn.chain_model(mn.x3_passes(A, B), True), "f32": mn.chain_model([(A, B)], True)}
            out = {}
            for e, (epi, kw) in enumerate([(0, {}), (0, {"cmask": cmask}), (1, {"bias": bias}), (2, {"bias": bias}),
                                           (3, {"old": old}), (4, {"old": old})]):
                for eng, budget in (("x3", mn.x3_budget), ("f32", mn.f32_budget)):
                    out[eng, e] = budget(A, B, epi=epi, **kw) + (mn.epilogue(acc[eng], epi, **kw),)
            for splits in (3, 8):  # gemm_f32's atomic epilogue with the caller's split count
                out["f32", 5, splits] = mn.f32_budget(A, B, epi=4, old=old, splits=splits) + (out["f32", 5][2],)
            probs.append(((A, B, bias, old, cmask), out))
        _GEMM[key] = probs
    return _GEMM[key]


EPILOGUES = [(0, "store"), (0, "cmask"), (1, "bias"), (2, "bias relu"), (3, "accum"), (4, "atomic")]


def run_epilogues(call, probs, eng, what, cases=range(6), splits=None):
    """call(A, B, C, epi, bias, cmask) for the epilogue cases (indices into EPILOGUES) of each problem; the problems'
    outputs are stacked."""
    for e in cases:
        epi, name = EPILOGUES[e]
        got = []
        for (A, B, bias, old, cmask), _ in probs:
            C = old.clone() if epi >= 3 else torch.full_like(old, NAN)
            call(A, B, C, epi, bias if epi in (1, 2) else None, cmask if e == 1 else None)
            got.append(C)
        key = (eng, e, splits) if splits else (eng, e)
        ref, extra, model = (torch.cat([out[key][i] for _, out in probs]) for i in range(3))
        check(f"{what} | {name}", torch.cat(got), model, ref, extra)


@pytest.mark.parametrize("family", mn.FAMILIES)
@pytest.mark.parametrize("shape,layout", X3_CASES, ids=lambda v: "x".join(str(int(i)) for i in v))
def test_x3_layouts_epilogues(shape, layout, family):
    a_km, b_km = layout
    assert mn.x3_eligible(*shape, a_km, b_km)

    def call(A, B, C, epi, bias, cmask):
        K.gemm_f32x3(lay(A, a_km), lay(B, b_km), C, a_km, b_km, epi, bias, None, None, cmask)

    run_epilogues(call, gemm_case(family, shape), "x3", f"x3 {shape} akm {int(a_km)} bkm {int(b_km)} | {family}")


@pytest.mark.parametrize("family", ["random sign", "row norms"])
@pytest.mark.parametrize("shape,layout", F32_CASES, ids=lambda v: "x".join(str(int(i)) for i in v))
def test_gemm_f32_layouts_epilogues(shape, layout, family):
    """The exact fp32 engine (the reference-size fallback) under the same contract; the atomic epilogue with 1, 3 and
    8 splits."""
    a_km, b_km = layout
    probs = gemm_case(family, shape)
    with f32_engine(exact=True):
        for splits in (1, 3, 8):
            def call(A, B, C, epi, bias, cmask):
                K.gemm_f32(lay(A, a_km), lay(B, b_km), C, a_km, b_km, epi, splits if epi == 4 else 1, bias)

            run_epilogues(call, probs, "f32", f"f32 {shape} akm {int(a_km)} bkm {int(b_km)} splits {splits} | {family}",
                          cases=(0, 2, 3, 4, 5) if splits == 1 else (5,),  # (the binding has no cmask)
                          splits=None if splits == 1 else splits)


@pytest.mark.parametrize("a_km,b_km", LAYOUTS)
def test_x3_selector_rows_are_bit_exact(a_km, b_km):
    """One-hot rows of A (then of B) pick single entries of the other operand: hi + mid + lo of one fp32 number summed
    in fp32 is that number, so the output equals it bit for bit (and is exactly 0 for an all-zero row)."""
    M, N, Kd = 260, 132, 100
    B, *_ = mn.gemm_inputs("row norms", N, M, Kd, seed=1, device=DEV)  # [N, K] with a spread of magnitudes
    S = mn.selector_rows_f32(M, Kd, device=DEV)
    C = torch.full((M, N), NAN, device=DEV)
    K.gemm_f32x3(lay(S, a_km), lay(B, b_km), C, a_km, b_km, 0)
    assert torch.equal(C, mn.selected(S, B))
    A, *_ = mn.gemm_inputs("row norms", M, N, Kd, seed=2, device=DEV)
    S = mn.selector_rows_f32(N, Kd, device=DEV)
    K.gemm_f32x3(lay(A, a_km), lay(S, b_km), C, a_km, b_km, 0)
    assert torch.equal(C, mn.selected(S, A).t())


@pytest.mark.parametrize("family", ["random sign", "positive"])
@pytest.mark.parametrize("a_km", [False, True])
@pytest.mark.parametrize("M,N,T", mn.X3_WGRAD_SHAPES)
def test_x3_weight_gradient_form(M, N, T, a_km, family):
    """gw [M, N] += (gy amask)^T x over T rows with fp32 atomics in the kernel's splits, gb += the fused row sums, both
    into non-zero values; amask holds exact zeros."""
    A, B, _, old, _, amask = mn.gemm_inputs(family, M, N, T, seed=T + M, device=DEV)  # A = gy^T [M, T], B = x^T [N, T]
    old_b = old[:, 0].clone()
    Am = A * (amask > 0)
    splits, kps = mn.x3_pick_splits(M, N, T, a_km)
    ref, extra = mn.x3_budget(Am, B, epi=4, old=old, splits=splits)
    # (one chain over all T rows: with all-positive terms a single long accumulation has more error than the kernel's
    # splits from zero, and an honest unsplit sum must fit the model too)
    model = old + mn.chain_model(mn.x3_passes(Am, B), True)
    gw, gb = old.clone(), old_b.clone()
    K.gemm_f32x3(lay(A, a_km), B.t().contiguous(), gw, a_km, True, 4, None, gb, lay(amask, a_km))
    what = f"x3 wgrad {M}x{N} T {T} akm {int(a_km)} splits {splits} | {family}"
    check(what, gw, model, ref, extra)
    rs_ref, rs_extra = mn.rowsum_budget(Am, old_b)
    note(what + " | row sums", use=gn.check_elementwise(gb, rs_ref, extra=rs_extra, bf16=False, name=what + " gb"))


def linear_case(M, seed):
    N, Kd = 128, 784
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, Kd, generator=g).relu().to(DEV)
    w, b = (torch.randn(N, Kd, generator=g) * 0.05).to(DEV), torch.randn(N, generator=g).to(DEV)
    gy = mn.masky((M, N), g).to(DEV)
    return x, w, b, gy, torch.randn(N, Kd, generator=g).to(DEV), torch.randn(N, generator=g).to(DEV)


def check_linear_ops(what, M, budget, passes_of):
    """ops.linear_relu_fwd / linear_fwd / linear_relu_bwd (ReLU mask from y, dx masked by x > 0), gw / gb accumulated
    into non-zero values."""
    x, w, b, gy, gw0, gb0 = linear_case(M, M)
    y, y_lin = ops.linear_relu_fwd(x, w, b), ops.linear_fwd(x, w, b)
    gw, gb = gw0.clone(), gb0.clone()
    dx = ops.linear_relu_bwd(x, y, gy, w, gw, gb, need_dx=True, gy_masked=False, mask_dx=True)
    gz = gy * (y > 0)
    acc = mn.chain_model(passes_of(x, w), True)
    for name, got, model, (ref, extra) in (
            ("fwd relu", y, torch.relu(acc + b), budget(x, w, epi=2, bias=b)),
            ("fwd", y_lin, acc + b, budget(x, w, epi=1, bias=b)),
            ("dx", dx, mn.chain_model(passes_of(gz, w.t()), True) * (x > 0), budget(gz, w.t(), cmask=x)),
            ("gw", gw, gw0 + mn.chain_model(passes_of(gz.t(), x.t()), True), budget(gz.t(), x.t(), epi=3, old=gw0))):
        check(f"{what} | {name}", got, model, ref, extra)
    gb_ref, gb_extra = mn.rowsum_budget(gz.t(), gb0)
    note(f"{what} | gb", use=gn.check_elementwise(gb, gb_ref, extra=gb_extra, bf16=False, name=f"{what} gb"))


@pytest.mark.parametrize("M", [1, 7, 60, 128, 129])
def test_linear_ops_small_batches(M):
    """The reference sizes: below 2^26 multiply-adds gemm_f32 keeps its own kernels (the small-batch VALU forward, the
    split-K forward with its bias-init and ReLU passes, the fp32 MFMA kernel)."""
    assert M * 128 * 784 < 2 ** 26 and K.gemm_f32_mode() == 1
    check_linear_ops(f"linear ops M {M} (fp32 engine)", M, mn.f32_budget, lambda a, b: [(a, b)])


def test_linear_ops_presplit_weight_route():
    """The smallest batch whose 784 -> 128 layer runs on the x3 engine (2^26 multiply-adds): the forward against W
    pre-split into bf16 planes, dx against the transposed pre-split W, the weight gradient with atomics."""
    M = 672
    assert M * 128 * 784 >= 2 ** 26 > (M - 4) * 128 * 784 and K.gemm_f32_mode() == 1
    check_linear_ops(f"linear ops M {M} (x3 engine, pre-split W)", M, mn.x3_budget, mn.x3_passes)


# =====================================================================================================================
# gemm_f16x2
def planes_of(p):
    return p[0].view(F16), p[1].view(F16)


@pytest.mark.parametrize("family", mn.FAMILIES)
@pytest.mark.parametrize("namax", [1, 5])
def test_x2_split_is_the_documented_representation(family, namax):
    """x2_split and x2_split_t write exactly hi = fp16(x 2^(14 - E)), lo = fp16(x 2^(14 - E) - hi) with E from the
    largest |amax| entry, which represent x to max(2^-23 |x|, 2^(E - 39))."""
    A, B, *_ = mn.gemm_inputs(family, 257, 320, 192, seed=3, device=DEV)
    for x in (A, B):
        m = x.abs().max()
        amax = m.reshape(1) if namax == 1 else torch.stack([0.1 * m, -0.5 * m, m * 0.0, -m, 0.25 * m])
        hi, lo, s, E = mn.x2_planes(x)
        p, sc = K.x2_split(x, amax.contiguous())
        assert float(sc) == s
        assert torch.equal(planes_of(p)[0], hi) and torch.equal(planes_of(p)[1], lo)
        back = (planes_of(p)[0].double() + planes_of(p)[1].double()) * s
        use = float(((back - x.double()).abs() / mn.x2_rep_bound(x, E)).max())
        note(f"x2 split | {family} | namax {namax}", use=use)
        assert use <= 1.0
        pt, st = K.x2_split_t(x, amax.contiguous())
        assert float(st) == s and torch.equal(planes_of(pt)[0], hi.t()) and torch.equal(planes_of(pt)[1], lo.t())
    # a looser bound (the next binade) moves every element down one bit, still inside its own representation bound
    p, sc = K.x2_split(A, (2 * A.abs().max()).reshape(1))
    assert float(sc) == 2 * mn.x2_planes(A)[2]


X2_VARIANTS = {"default": {}, "2phase": {"X2_2PHASE": 1}, "group_m=0": {"GEMM_GROUP_M": 0}, "group_m=2": {"GEMM_GROUP_M": 2}}
_X2 = {}


def x2_case(family, shape):
    key = (family,) + tuple(shape)
    if key not in _X2:
        M, N, Kd = shape
        A, B, bias, _, cmask, _ = mn.gemm_inputs(family, M, N, Kd, seed=M + Kd, device=DEV)
        passes, sc = mn.x2_passes(A, B)
        acc = mn.chain_model(passes, False).double() * sc
        out = {}
        for name, epi, kw in (("plain", 0, {}), ("bias", 1, {"bias": bias}), ("bias relu", 2, {"bias": bias}),
                              ("mask", 0, {"cmask": cmask})):
            model = (acc + bias.double()).float() if epi else acc.float()
            if epi == 2:
                model = torch.relu(model)
            if "cmask" in kw:
                model = model * (cmask > 0)
            out[name] = mn.x2_budget(A, B, epi=epi, **kw) + (model,)
        _X2[key] = (A, B, bias, cmask, out)
    return _X2[key]


# (X2_2PHASE selects between the two NT loops only)
X2_FORMS = [(b_kn, v) for b_kn in (False, True) for v in X2_VARIANTS if not (b_kn and v == "2phase")]


@pytest.mark.parametrize("family", mn.FAMILIES)
@pytest.mark.parametrize("b_kn,variant", X2_FORMS, ids=lambda v: v if isinstance(v, str) else ("nn" if v else "nt"))
@pytest.mark.parametrize("shape", mn.X2_GEMM_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_x2_gemm(shape, b_kn, variant, family):
    M, N, Kd = shape
    A, B, bias, cmask, out = x2_case(family, shape)
    pa, sa = K.x2_split(A, A.abs().max().reshape(1))
    if b_kn:
        pb, sb = K.x2_split(B.t().contiguous(), B.abs().max().reshape(1))
    else:
        pb, sb = K.x2_split(B, B.abs().max().reshape(1))
    slots = -(-M // 256) * -(-N // 256) * 8
    with knobs(**X2_VARIANTS[variant]):
        for name, b_, relu, mask in (("plain", None, False, None), ("bias", bias, False, None),
                                     ("bias relu", bias, True, None), ("mask", None, False, cmask)):
            poison(slots)
            C, wm = K.x2_gemm(pa, sa, pb, sb, b_kn, b_, relu, mask, True)
            ref, extra, model = out[name]
            check(f"x2 gemm {shape} {'nn' if b_kn else 'nt'} {variant} | {family} | {name}", C, model, ref, extra)
            assert wm.numel() == slots and torch.isfinite(wm).all() and (wm >= 0).all()
            assert float(wm.max()) == float(C.abs().max())
            if mask is not None:
                assert (C[cmask <= 0] == 0).all()


def test_x2_selector_rows():
    """One-hot rows of A pick B's entries: the output is B's two-plane representation, one rounding away."""
    M, N, Kd = 257, 320, 192
    _, B, *_ = mn.gemm_inputs("random sign", M, N, Kd, seed=4, device=DEV)
    S = mn.selector_rows_f32(M, Kd, device=DEV)
    pa, sa = K.x2_split(S, S.abs().max().reshape(1))
    pb, sb = K.x2_split(B, B.abs().max().reshape(1))
    C, _ = K.x2_gemm(pa, sa, pb, sb, False, None, False, None, False)
    want = mn.selected(S, B).double()
    E = mn.bound_exp(B.abs().max())
    extra = (mn.x2_rep_bound(want, E) + mn.U32 * want.abs()) * (want != 0)
    note("x2 selector rows of A", use=gn.check_elementwise(C, want, extra=extra, a=1e-300, bf16=False, name="x2 selector"))
    # one-hot rows of B pick A's entries
    A, *_ = mn.gemm_inputs("random sign", M, N, Kd, seed=5, device=DEV)
    S = mn.selector_rows_f32(N, Kd, device=DEV)
    pa, sa = K.x2_split(A, A.abs().max().reshape(1))
    pb, sb = K.x2_split(S, S.abs().max().reshape(1))
    C, _ = K.x2_gemm(pa, sa, pb, sb, False, None, False, None, False)
    want = mn.selected(S, A).t().double()
    extra = (mn.x2_rep_bound(want, mn.bound_exp(A.abs().max())) + mn.U32 * want.abs()) * (want != 0)
    note("x2 selector rows of B", use=gn.check_elementwise(C, want, extra=extra, a=1e-300, bf16=False, name="x2 selector B"))


# (the LDS-DMA loop takes whole 64-token K-steps only: T = 2100 runs the staged loop whatever the knob says)
X2_WGRAD_CASES = [(T, M, N, dma) for (T, M, N) in mn.X2_WGRAD_SHAPES for dma in (1, 0) if not (dma and T % mn.X2_TK)]


@pytest.mark.parametrize("family", ["random sign", "positive"])
@pytest.mark.parametrize("T,M,N,dma", X2_WGRAD_CASES)
def test_x2_weight_gradient(T, M, N, dma, family):
    g = torch.Generator().manual_seed(T + M)
    dz, x = torch.randn(T, M, generator=g) * 1e-2, torch.randn(T, N, generator=g).relu()
    old_w, old_b = torch.randn(M, N, generator=g), torch.randn(M, generator=g)
    if family == "positive":
        dz, old_w, old_b = dz.abs(), old_w.abs(), old_b.abs()
    dz, x, old_w, old_b = (t.to(DEV) for t in (dz, x, old_w, old_b))
    ref = mn.x2_wgrad_budget(dz, x, old_w, old_b)
    pd, sd = K.x2_split(dz, dz.abs().max().reshape(1))
    px, sx = K.x2_split(x, x.abs().max().reshape(1))
    gw, gb = old_w.clone(), old_b.clone()
    with knobs(WGRAD_DMA=dma):
        K.x2_wgrad_(pd, sd, px, sx, gw, gb)
    what = f"x2 wgrad T {T} {M}x{N} dma {dma} | {family}"
    check(what + " | gw", gw, mn.x2_wgrad_model(dz, x, old_w), ref["gw"], ref["gw_extra"])
    check(what + " | gb", gb[None], mn.x2_gb_fp32(dz, old_b)[None], ref["gb"][None], ref["gb_extra"][None])


def test_x2_linear_layer_ops():
    """ops.linear_relu_fwd_x2 + linear_relu_bwd_x2 once at the rows from which the MLP takes this engine."""
    M, N, Kd = ops._X2_MIN_ROWS, 128, 128
    g = torch.Generator().manual_seed(5)
    x = torch.randn(M, Kd, generator=g).relu().to(DEV)
    w, b = (torch.randn(N, Kd, generator=g) * 0.1).to(DEV), torch.randn(N, generator=g).to(DEV)
    gz = mn.masky((M, N), g).to(DEV) * 1e-3
    gw0, gb0 = torch.randn(N, Kd, generator=g).to(DEV), torch.randn(N, generator=g).to(DEV)
    assert ops.x2_ok(x, w)
    y, planes = ops.linear_relu_fwd_x2(x, w, b)
    gw, gb = gw0.clone(), gb0.clone()
    dx = ops.linear_relu_bwd_x2(x, gz, gw, gb, planes, need_dx=True, mask_dx=True)
    assert float(y._sdml_wmax.max()) == float(y.abs().max()) and float(dx._sdml_wmax.max()) == float(dx.abs().max())
    ref = mn.x2_wgrad_budget(gz, x, gw0, gb0)
    py, sy = mn.x2_passes(x, w)
    pdx, sdx = mn.x2_passes(gz, w.t().contiguous())
    grouped("x2 layer ops | y", y, torch.relu((mn.chain_model(py, False).double() * sy + b.double()).float()),
            mn.x2_budget(x, w, epi=2, bias=b)[0])
    grouped("x2 layer ops | dx", dx, mn.chain_model(pdx, False) * sdx * (x > 0), mn.x2_budget(gz, w.t(), cmask=x)[0])
    grouped("x2 layer ops | gw", gw, mn.x2_wgrad_model(gz, x, gw0), ref["gw"])
    grouped("x2 layer ops | gb", gb[None], mn.x2_gb_fp32(gz, gb0)[None], ref["gb"][None])
    for name, got, (r, e) in (("y", y, mn.x2_budget(x, w, epi=2, bias=b)), ("dx", dx, mn.x2_budget(gz, w.t(), cmask=x)),
                              ("gw", gw, (ref["gw"], ref["gw_extra"])), ("gb", gb, (ref["gb"], ref["gb_extra"]))):
        note(f"x2 layer ops | {name}", use=gn.check_elementwise(got, r, extra=e, a=1e-300, bf16=False, name=f"x2 layer {name}"))


# =====================================================================================================================
# u8_fwd
def u8_weights(N, Kd, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.empty(N, Kd).uniform_(-0.05, 0.05, generator=g).to(DEV), torch.randn(N, generator=g).to(DEV)


def check_u8_fwd(what, x8, w, b, planes=None, planes_valid=False, relus=(False, True)):
    """linear_fwd_u8 with and without ReLU against the budget; the ReLU bits and the per-wave maxima are those of the
    stored values. Returns whether the per-wave maxima differ between slots (the uint8 kernel's own epilogue)."""
    M, N = x8.shape[0], w.shape[0]
    scale = ops.PIXEL_SCALE
    distinct = False
    for relu in relus:
        mask = torch.full((M, N // 32), -1, dtype=torch.int32, device=DEV) if relu else None
        wm = torch.full((int(K.u8_fwd_wmax_slots(M, N)),), NAN, device=DEV)
        y = K.linear_fwd_u8(x8, w, b, relu, scale, planes, planes_valid, mask, wm)
        ref, extra = mn.u8_fwd_budget(x8, w, b, scale, relu)
        check(f"{what} | relu {int(relu)}", y, mn.u8_fwd_model(x8, w, b, scale, relu), ref, extra)
        assert torch.isfinite(wm).all() and float(wm.max()) == float(y.abs().max())
        distinct = distinct or wm.unique().numel() > 1
        if relu:
            assert torch.equal(mask, mn.relu_bits_of(y)) and torch.equal(mask, K.relu_bits(y))
    return distinct


@pytest.mark.parametrize("family", mn.PIXEL_FAMILIES)
@pytest.mark.parametrize("M", mn.U8_FWD_ROWS)
@pytest.mark.parametrize("N,Kd", mn.U8_FWD_NK)
def test_u8_fwd(N, Kd, M, family):
    assert M >= mn.U8_FWD_MIN_ROWS and Kd % 16 == 0 and N % 128 == 0  # the route: mlp_u8.hip's kernel, not the fp32 engines
    x8 = mn.pixel_inputs(family, M, Kd, seed=M + Kd, device=DEV)
    w, b = u8_weights(N, Kd, N + Kd)
    distinct = check_u8_fwd(f"u8 fwd {M}x{N}x{Kd} tail {mn.u8_tail_substeps(Kd)} | {family}", x8, w, b)
    if family == "uniform":
        assert distinct  # (the fp32 fallback fills every slot with one inf-norm)


@pytest.mark.parametrize("variant,kn", [("wmt4", {"U8_FWD_WMT": 4}), ("waves16", {"U8_FWD_WAVES": 16}),
                                        ("waves8", {"U8_FWD_WAVES": 8})])
@pytest.mark.parametrize("N,Kd", [(128, 784), (256, 96)])
def test_u8_fwd_block_geometries(N, Kd, variant, kn):
    """The 128-row-wave and the 16-wave kernels, reached below their natural threshold through their knobs."""
    M = 4617
    x8 = mn.pixel_inputs("uniform", M, Kd, seed=6, device=DEV)
    w, b = u8_weights(N, Kd, 7)
    with knobs(**kn):
        assert check_u8_fwd(f"u8 fwd {M}x{N}x{Kd} {variant}", x8, w, b)


def test_u8_fwd_at_the_512_row_block_threshold():
    M, N, Kd = 131072, 128, 784
    x8 = mn.pixel_inputs("uniform", M, Kd, seed=8, device=DEV)
    w, b = u8_weights(N, Kd, 9)
    assert int(K.u8_fwd_wmax_slots(M, N)) == M // 512 * 16  # 16 waves of 512-row blocks
    assert check_u8_fwd(f"u8 fwd {M}x{N}x{Kd} natural", x8, w, b, relus=(True,))


@pytest.mark.parametrize("deep", [0, 1])
def test_u8_fwd_on_the_x3_engine(deep):
    """U8_FWD_X3 = 1: pixels as one exact bf16 plane against W's three (3 K products), both register pipelines."""
    M, N, Kd = 4617, 128, 784
    x8 = mn.pixel_inputs("uniform", M, Kd, seed=10, device=DEV)
    w, b = u8_weights(N, Kd, 11)
    _, s64 = mn.u8_scale(ops.PIXEL_SCALE)
    ref, extra = mn.gemm_budget(x8, w, 3, terms=mn.X3_TERMS)
    ref, extra = torch.relu(ref * s64 + b.double()), s64 * extra + 2 * mn.U32 * (s64 * ref.abs() + b.double().abs())
    wh, wm_, wl = mn.x3_split(w)
    acc = mn.chain_model([(x8, wh), (x8, wm_), (x8, wl)], True)
    model = torch.relu(((acc.double() * s64).float().double() + b.double()).float())
    with knobs(U8_FWD_X3=1, X3_DEEP=deep):
        y = K.linear_fwd_u8(x8, w, b, True, ops.PIXEL_SCALE)
    check(f"u8 fwd x3 engine deep {deep}", y, model, ref, extra)


def test_u8_fwd_plane_cache():
    """A caller-owned plane cache holds exactly u8_planes.h's planes, zero-padded; a stale token re-splits."""
    M, N, Kd = 4140, 128, 112
    x8 = mn.pixel_inputs("uniform", M, Kd, seed=12, device=DEV)
    w, b = u8_weights(N, Kd, 13)
    cache = ops.PlaneCache(w)
    cache.planes.fill_(0x7e00)  # fp16 NaN bits: the split must write the padding too

    def planes_match():
        hi, lo = mn.u8_w_planes(w)
        got = cache.planes.view(F16)
        return (torch.equal(got[0, :, :Kd], hi) and torch.equal(got[1, :, :Kd].float(), lo.float())
                and bool((got[:, :, Kd:] == 0).all()))

    y1 = ops.linear_relu_fwd_u8(x8, w, b, cache, epoch=0)
    assert planes_match()
    check_u8_fwd("u8 fwd plane cache | valid", x8, w, b, cache.planes, True, relus=(True,))
    assert torch.equal(y1, ops.linear_relu_fwd_u8(x8, w, b, cache, epoch=0))  # the cached planes, same bits
    w.mul_(1.5)  # an in-place write: the token is stale, the forward must re-split
    y2 = ops.linear_relu_fwd_u8(x8, w, b, cache, epoch=0)
    assert planes_match()
    ref, extra = mn.u8_fwd_budget(x8, w, b, ops.PIXEL_SCALE, True)
    note("u8 fwd plane cache | stale token", use=gn.check_elementwise(y2, ref, extra=extra, bf16=False, name="re-split"))


# =====================================================================================================================
# classifier heads
def one(v):
    return torch.as_tensor(v, dtype=torch.float64, device=DEV).reshape(1)


def check_bound(what, amax, got_dx, ref, w, scale, form):
    """The bound a head attaches to its dx / dl (`_sdml_amax`, one entry per block) against the float64 values it is
    documented to bound. form "block" (head_block_kernel, 256-row blocks in row order): entry b is
    2 max_r sum_c |dl_c| max |W2| over the block's rows; it must be that float64 value to within the dl budget (both
    sides: the derived factor is the formula itself) and dominate the block's float64 max |dl W2|. form "lds"
    (head_lds_kernel, block b takes row pairs (8 i + b') ...): entry b equals the max |dx| the block stored. form None:
    the head returns no bound (VALU and generic heads); a bound appearing or vanishing is a route change."""
    if form is None:
        assert amax is None, f"{what}: unexpected bound"
        return
    assert amax is not None, f"{what}: the head returned no bound"
    assert torch.isfinite(amax).all()
    M = ref["dl"].shape[0]
    if form == "lds":
        nb = min((M + 7) // 8, 1024)
        assert amax.numel() == nb
        owner = (torch.arange(M, device=DEV) // 2 // 4) % nb  # row pair p belongs to wave p % 4 of block (p // 4) % nb
        want = torch.zeros(nb, device=DEV).scatter_reduce(0, owner, got_dx.abs().amax(1), "amax")
        assert torch.equal(amax, want), f"{what}: per-block max |dx|"
        return
    nb = (M + 255) // 256
    assert amax.numel() == nb
    blk = torch.arange(M, device=DEV) // 256
    zeros = torch.zeros(nb, dtype=torch.float64, device=DEV)
    wmax = float(w.abs().max())
    l1, e1 = ref["dl"].abs().sum(1), ref["dl_extra"].sum(1)
    hi = 2 * zeros.scatter_reduce(0, blk, l1 + e1, "amax") * wmax * (1 + 8 * mn.U32)
    lo = 2 * zeros.scatter_reduce(0, blk, (l1 - e1).clamp_min(0), "amax") * wmax * (1 - 8 * mn.U32)
    true = zeros.scatter_reduce(0, blk, ref["dx"].abs().amax(1), "amax")
    a64 = amax.double()
    assert (a64 <= hi).all() and (a64 >= lo).all(), f"{what}: a block's bound is not 2 max_r sum_c |dl_c| max |W2|"
    assert (a64 * (1 + 8 * mn.U32) >= true).all(), f"{what}: a block's bound is below its max |dl W2|"
    note(f"{what} | per-block bound over max |dl W2|", worst=float((a64 / true.clamp_min(1e-300)).min()), blocks=float(nb))


def head_models(dl, h, w, scale, ow, ob):
    """fp32 rounding models and float64 references of the head's GEMM-like outputs GIVEN the dl the kernel produced (as
    the attention backward's model takes the y its run was given: dl's own error is budgeted where dl is checked, and
    would otherwise drown the products' error here): dx = dl W2 a class-ordered chain; gW2 = old + dl^T h a row-ordered
    chain over the two fp16 planes of dl scaled from |dl| <= scale (head_block.h; h taken exactly: the dl planes carry
    the dominant plane error)."""
    d = dl.double()
    dh, dlo, sd, _ = mn.x2_planes(dl, E=mn.bound_exp(float(torch.tensor(scale, dtype=torch.float32))))
    model = {"dx": mn.chain_model([(dl, w.t())], True),
             "gw": ow + mn.chain_model([(dh.t(), h.t()), (dlo.t(), h.t())], True) * sd}
    ref = {"dx": d @ w.double(), "gw": ow.double() + d.t() @ h.double()}
    return model, ref


def grouped(what, got, model, ref, fp32_extra=None):
    row, rms = gn.check_grouped(got, model, ref, name=what, fp32_extra=fp32_extra)
    note(what + " | grouped", row=row, rms=rms)


def run_head(what, family, M, Kd, C, dl_path, bound=None, planes=False):
    """planes: the head computes on fp16 planes (head_block.h); the others are held to the tighter fp32 budget."""
    h, w, b, t, ow, ob = mn.head_inputs(family, M, Kd, C, seed=M, device=DEV)
    scale = 1.0 / M
    ref = mn.head_budget(h, w, b, t, scale, ow, ob, planes=planes)
    what = f"{what} | {family}"

    def uses(tag, out, masked=True):
        u = mn.check_head(out, ref, h, f"{what} {tag}", masked=masked)
        if u:
            note(f"{what} | {tag}", **u)

    # training head, dx masked by h > 0, loss and correct returned, gw / gb accumulated into non-zero values
    gw, gb = ow.clone(), ob.clone()
    loss, correct, dx = ops.linear_logsoftmax_nll(h, w, b, t, gw, gb, scale, True, mask_dx=True)
    uses("train", {"loss": loss, "correct": correct, "dx": dx, "gw": gw, "gb": gb})
    check_bound(f"{what} | dx", getattr(dx, "_sdml_amax", None), dx, ref, w, scale, bound)
    if bound == "lds":  # no dl comes out of this head: dx and gW2 against the chain models of the whole head
        model = mn.head_chain_models(h, w, b, t, scale, ow)
        grouped(f"{what} | dx", dx, model["dx"] * (h > 0), ref["dx"] * (h > 0), fp32_extra=ref["dx_form_extra"])
        grouped(f"{what} | gw", gw, model["gw"], ref["gw"])
    # dx unmasked; stats accumulated into non-zero values, then overwritten (stats_init) from NaN
    st = torch.tensor([5.0, 3.0], device=DEV)
    gw2, gb2 = ow.clone(), ob.clone()
    _, _, dx_u = ops.linear_logsoftmax_nll(h, w, b, t, gw2, gb2, scale, True, stats=st, mask_dx=False, stats_init=False)
    uses("unmasked", {"dx": dx_u, "gw": gw2, "gb": gb2}, masked=False)
    gn.check_elementwise(st[:1], one(ref["loss"] + 5.0), extra=one(ref["loss_extra"] + 2 * mn.U32 * (5 + abs(float(ref["loss"])))),
                         bf16=False, name=f"{what} stats +=")
    assert ref["correct_min"] <= float(st[1]) - 3.0 <= ref["correct_max"]
    st = torch.full((2,), NAN, device=DEV)
    ops.linear_logsoftmax_nll(h, w, b, t, ow.clone(), ob.clone(), scale, True, stats=st, stats_init=True)
    uses("stats_init", {"loss": st[0], "correct": st[1]})
    # eval mode
    loss_e, correct_e, dx_e = ops.linear_logsoftmax_nll(h, w, b, t, None, None, 1.0, False)
    assert dx_e is None
    uses("eval", {"loss": loss_e, "correct": correct_e})
    if not dl_path:
        return
    # the factored head: dl out, then dx from dl, masked and not
    st = torch.full((2,), NAN, device=DEV)
    gw3, gb3 = ow.clone(), ob.clone()
    dl = ops.linear_logsoftmax_nll_dl(h, w, b, t, gw3, gb3, scale, st, stats_init=True)
    uses("dl", {"loss": st[0], "correct": st[1], "dl": dl, "gw": gw3, "gb": gb3})
    check_bound(f"{what} | dl", getattr(dl, "_sdml_amax", None), None, ref, w, scale, bound)
    dx_dl = ops.head_dx_from_dlogits(dl, w, h, mask=True)
    uses("dx from dl", {"dx": dx_dl})
    if M >= 255:  # (enough elements for an RMS) the GEMM-like outputs against their rounding models, given this dl
        model, r64 = head_models(dl, h, w, scale, ow, ob)
        # equal family: dx = w sum_c dl_c with sum_c dl_c = 0, what is left is the fp32 sum's rounding in an order the
        # model cannot reproduce; its any-order bound goes in as the checker's fp32_extra (rows only)
        cancel = (C + 8) * mn.U32 * (dl.double().abs() @ w.double().abs()) if family == "equal" else None
        grouped(f"{what} | dx", dx_dl, model["dx"] * (h > 0), r64["dx"] * (h > 0), fp32_extra=cancel)
        grouped(f"{what} | gw", gw3, model["gw"], r64["gw"])
        # (gb2 has C <= 16 numbers per case, each dominated by the one rounding of old + sum: no RMS to compare)
    uses("dx from dl unmasked", {"dx": ops.head_dx_from_dlogits(dl, w, h, mask=False)}, masked=False)


@pytest.mark.parametrize("M", mn.HEAD_ROWS)
@pytest.mark.parametrize("C", [2, 10, 16])
@pytest.mark.parametrize("variant,kn", [("block", {}), ("valu", {"HEAD_VALU": 1})])
def test_head_k128(variant, kn, C, M):
    """K = 128, C in {2, 10, 16}: head_block_kernel by default, head_fused_kernel with HEAD_VALU = 1 (16 threads per
    row up to 2048 rows, 4 above); every family, with the factored (dl) form and head_dx_from_dlogits."""
    with knobs(**kn):
        for family in mn.head_families(C):
            run_head(f"head {variant} M {M} C {C}", family, M, 128, C, dl_path=True, bound="block" if variant == "block" else None,
                     planes=variant == "block")


@pytest.mark.parametrize("M", mn.HEAD_ROWS)
@pytest.mark.parametrize("Kd,C", [(128, 3), (50, 10)])
def test_head_generic(Kd, C, M):
    """Shapes outside the fused kernels: head_generic_kernel writes dz, the weight gradient is gemm_f32's."""
    for family in mn.head_families(C):
        run_head(f"head generic M {M} K {Kd} C {C}", family, M, Kd, C, dl_path=False)


@pytest.mark.parametrize("variant,kn", [("default", {}), ("stages3", {"U8_FH_STAGES": 3}), ("rows512", {"U8_FH_ROWS512": 1})])
@pytest.mark.parametrize("C", [10, 2, 16])
@pytest.mark.parametrize("M", [256, 300, 777])
def test_fused_forward_head(M, C, variant, kn):
    """linear_relu_head_u8: the uint8 forward and the block head in one launch, h never stored. Held to the float64
    head budget end to end: the reference h is the float64 forward, its forward budget enters e_z and gW2. The ReLU bits
    must be those of the float64 pre-activation wherever it is further from 0 than the forward budget. The returned
    per-block bounds are checked as the block head's, and then consumed at every M: linear_wgrad_u8_dl with those bounds,
    the kernel's dl and its ReLU bits must meet the weight-gradient budget and its rounding model at the E they give."""
    N, Kd = 128, mn.U8W_K
    assert K.u8_fwd_head_supported(M, N, Kd, C)
    g = torch.Generator().manual_seed(M + C)
    x8 = mn.pixel_inputs("uniform", M, Kd, seed=M, device=DEV)
    w1, b1 = u8_weights(N, Kd, M + 1)
    _, w2, b2, t, ow2, ob2 = mn.head_inputs("small", M, N, C, seed=M, device=DEV)
    w2 = w2 * 4  # (h here is about 0.5, not 0.4 of 128 half-zero units: logits of a few tenths)
    pre, e_h = mn.u8_fwd_budget(x8, w1, b1, ops.PIXEL_SCALE, False)
    h64 = torch.relu(pre)
    scale = 1.0 / M
    ref = mn.head_budget(h64, w2, b2, t, scale, ow2, ob2, e_h=e_h)
    cache = ops.PlaneCache(w1)
    gw2, gb2 = ow2.clone(), ob2.clone()
    stats = torch.full((2,), NAN, device=DEV)
    dl = torch.full((M, C), NAN, device=DEV)
    bits = torch.full((M, N // 32), -1, dtype=torch.int32, device=DEV)
    what = f"fused fwd+head M {M} C {C} {variant}"
    with knobs(**kn):
        bounds, pending = ops.linear_relu_head_u8(x8, w1, b1, cache, 0, w2, b2, t, gw2, gb2, scale, stats, True, dl, bits)
    assert pending is None
    u = mn.check_head({"loss": stats[0], "correct": stats[1], "dl": dl, "gw": gw2, "gb": gb2}, ref, h64, what)
    note(what, **u)
    sure = pre.abs() > e_h
    assert torch.equal(ops.relu_bits_unpack(bits).bool()[sure], (pre > 0)[sure]), f"{what}: ReLU bits"
    check_bound(what, bounds, None, ref, w2, scale, "block")
    # the consumer: the first layer's weight gradient from this dl, these bits and these bounds
    # (the weight-gradient kernels take whole 32-row K-steps: at M = 300 and 777 the first 288 and 768 rows, still under
    # the same per-block bounds)
    Mw = M - M % 32
    _, _, ow, ob = wgrad_case(Mw, N, M + 2)
    x8w, dlw, bitsw = x8[:Mw].contiguous(), dl[:Mw].contiguous(), bits[:Mw].contiguous()
    assert_dl_route(x8w, Mw, N, C)
    keep = ops.relu_bits_unpack(bitsw).bool()
    d64, dmodel, e_dz = mn.dz_from_dl(dlw, w2, keep)
    E = mn.bound_exp(bounds.max())
    assert float(bounds.max()) >= float(d64.abs().max())
    splits, rps = mn.u8_wgrad_splits(Mw, N)
    gw, gb = flat_pair(ow, ob)
    ops.linear_wgrad_u8_dl(x8w, dlw, w2, bitsw, gw, gb, amax=bounds)
    check_wgrad(what + " | wgrad from its dl, bits and bounds", gw, gb,
                mn.u8_wgrad_model(dmodel, x8w, ow, ob, ops.PIXEL_SCALE, E, splits, rps),
                mn.u8_wgrad_budget(d64, x8w, ow, ob, ops.PIXEL_SCALE, E, splits, e_dz=e_dz))


def test_head_wide_k():
    """K = 1024, C = 10 from 4096 rows: head_lds_kernel (the 4 x 1024 MLP's head); its bound is the exact max |dx|."""
    for family in mn.head_families(10):
        run_head("head lds M 4096 K 1024 C 10", family, 4096, 1024, 10, dl_path=False, bound="lds")


# =====================================================================================================================
# u8_wgrad family
def flat_pair(old_w, old_b):
    """gw and gb adjacent in one buffer (the flat gradient layout mlp_u8.hip's kernels write through)."""
    N, Kd = old_w.shape
    buf = torch.cat([old_w.reshape(-1), old_b])
    gw, gb = buf[:N * Kd].view(N, Kd), buf[N * Kd:]
    assert gb.data_ptr() == gw.data_ptr() + 4 * N * Kd and gw.is_contiguous()  # (what the bindings test for this route)
    return gw, gb


def assert_dl_route(x8, M, N, C):
    """The conditions under which linear_wgrad_u8_dl runs u8_wgrad_kernel<1 / 2> (or the ring kernel) and not its
    torch fallback: u8_wgrad_dl_supported and head_fused_supported restated, with the flat pair of flat_pair()."""
    assert M % 32 == 0 and M >= 32 and N == 128 and C in (2, 10, 16) and x8.shape[1] == mn.U8W_K
    assert x8.is_contiguous() and x8.data_ptr() % 16 == 0


def wgrad_case(M, N, seed):
    g = torch.Generator().manual_seed(seed)
    x8 = mn.pixel_inputs("uniform", M, mn.U8W_K, seed=seed, device=DEV)
    dz = (mn.masky((M, N), g) * 1e-3).to(DEV)
    return x8, dz, torch.randn(N, mn.U8W_K, generator=g).to(DEV), torch.randn(N, generator=g).to(DEV)


def check_wgrad(what, gw, gb, model, ref):
    check(what + " | gw", gw, model[0], ref["gw"], ref["gw_extra"])
    check(what + " | gb", gb[None], model[1][None], ref["gb"][None], ref["gb_extra"][None])


@pytest.mark.parametrize("bound", ["given", "loose", "none"])
@pytest.mark.parametrize("N", [64, 128, 256])
@pytest.mark.parametrize("M", [4096, 4128])
def test_u8_wgrad_from_dz(M, N, bound):
    """linear_wgrad_u8 on the flat layout (u8_wgrad_kernel<0>): a bound given as several entries, a bound a binade
    and a half loose (dz keeps fewer low bits: the floor term carries it), and none (the binding's inf-norm)."""
    assert M >= mn.U8W_MIN_ROWS_DZ and M % 32 == 0 and N % 64 == 0
    x8, dz, ow, ob = wgrad_case(M, N, M + N)
    m = dz.abs().max()
    amax = {"given": torch.stack([0.5 * m, m, 0.1 * m]), "loose": (3 * m).reshape(1), "none": None}[bound]
    E = mn.bound_exp(m if amax is None else amax.max())
    splits, rps = mn.u8_wgrad_splits(M, N)
    gw, gb = flat_pair(ow, ob)
    ops.linear_wgrad_u8(x8, dz, gw, gb, amax=amax)
    check_wgrad(f"u8 wgrad dz {M}x{N} bound {bound} splits {splits}", gw, gb,
                mn.u8_wgrad_model(dz, x8, ow, ob, ops.PIXEL_SCALE, E, splits, rps),
                mn.u8_wgrad_budget(dz, x8, ow, ob, ops.PIXEL_SCALE, E, splits))


@pytest.mark.parametrize("M,flat,kn", [(4096, False, {}), (4096 + 33, True, {}), (4096, True, {"U8_WGRAD_X3": 1}),
                                       (4096, True, {"U8_WGRAD_X3": 1, "X3_DEEP": 0})])
def test_u8_wgrad_on_the_x3_engine(M, flat, kn):
    """gw / gb apart, M % 32 != 0 or U8_WGRAD_X3 = 1: the bf16x3 engine's slab form, dz in three exact bf16 planes
    against one exact pixel plane."""
    N = 128
    s32 = float(torch.tensor(ops.PIXEL_SCALE, dtype=torch.float32))
    splits, _ = mn.x3_pick_splits(N, mn.U8W_K, M, True)
    assert splits == 8
    runs = []
    for seed in range(4):  # gb has 128 numbers per problem: four problems stacked for a stable RMS (n_problems' reason)
        x8, dz, ow, ob = wgrad_case(M, N, M + 1 + seed)
        gw, gb = flat_pair(ow, ob) if flat else (ow.clone(), ob.clone())
        with knobs(**kn):
            ops.linear_wgrad_u8(x8, dz, gw, gb)
        acc = mn.chain_model(mn.u8x3_wgrad_passes(dz, x8), True)
        # the fused row sums leave as one fp32 atomic per wave and split (8 waves x 8 splits of 16 K-steps or more), each
        # a rounding at the magnitude of the gb it lands in: the model adds that many partials one by one
        gb_model = ob.clone()
        for part in range(8 * splits):
            rows = torch.arange(part, M, 8 * splits, device=DEV)
            gb_model = gb_model + mn.chain_model([(dz[rows].t(), torch.ones(1, rows.numel(), device=DEV))], True)[:, 0]
        ref = mn.u8_wgrad_budget(dz, x8, ow, ob, ops.PIXEL_SCALE, None, 8 * splits, n_planes=3, rel=0.0)
        runs.append((gw, gb, ow + (acc.double() * s32).float(), gb_model, ref))
    cat = lambda i: torch.cat([r[i] for r in runs])  # noqa: E731
    ref = {k: torch.cat([r[4][k] for r in runs]) for k in ("gw", "gw_extra", "gb", "gb_extra")}
    check_wgrad(f"u8 wgrad x3 engine M {M} flat {int(flat)} {kn}", cat(0), cat(1), (cat(2), cat(3)), ref)


def test_u8_wgrad_consumes_the_heads_bound():
    """The bound hand-off: the dx a head returns carries its per-block bounds, and linear_wgrad_u8 scales dz's planes
    from them. The weight gradient must meet the budget at the E those bounds give (a bound too large costs low bits
    and shows against the model; one too small overflows fp16 and shows as inf)."""
    M, N, C = 4096, 128, 10
    h, w2, b2, t, ow2, ob2 = mn.head_inputs("small", M, N, C, seed=3, device=DEV)
    x8, _, ow, ob = wgrad_case(M, N, 4)
    _, _, dx = ops.linear_logsoftmax_nll(h, w2, b2, t, ow2.clone(), ob2.clone(), 1.0 / M, True, mask_dx=True)
    assert dx._sdml_amax is not None and float(dx._sdml_amax.max()) >= float(dx.abs().max())
    E = mn.bound_exp(dx._sdml_amax.max())
    assert E - mn.bound_exp(dx.abs().max()) <= 3  # 2 sum_c |dl_c| max |W2| over max |dl W2|: 5.5 - 6.5 here
    splits, rps = mn.u8_wgrad_splits(M, N)
    gw, gb = flat_pair(ow, ob)
    ops.linear_wgrad_u8(x8, dx, gw, gb)
    check_wgrad("u8 wgrad dz from the block head's dx and bounds", gw, gb,
                mn.u8_wgrad_model(dx, x8, ow, ob, ops.PIXEL_SCALE, E, splits, rps),
                mn.u8_wgrad_budget(dx, x8, ow, ob, ops.PIXEL_SCALE, E, splits))


DL_VARIANTS = {"default": {}, "ring=0": {"U8_WGRAD_RING": 0}, "bal": {"U8_WGRAD_BAL": 1}, "pair": {"U8_WGRAD_PAIR": 1},
               "ilv": {"U8_WGRAD_ILV": 1}}


@pytest.mark.parametrize("variant", list(DL_VARIANTS))
@pytest.mark.parametrize("src", ["h", "bits"])
@pytest.mark.parametrize("C", [10, 2])
@pytest.mark.parametrize("M", mn.U8W_ROWS)
def test_u8_wgrad_from_dl(M, C, src, variant):
    """linear_wgrad_u8_dl: dz = (dl W2) (h > 0) expanded in the kernel, from h and from its ReLU bits, with a given
    bound (held to the model as well) and without (every workgroup's own bound: E at most that of
    2 max_r sum_c |dl_c| max |W2|; elementwise), and one hidden-group range (`groups`)."""
    N = 128
    g = torch.Generator().manual_seed(M + C)
    x8, _, ow, ob = wgrad_case(M, N, M + C)
    h = mn.masky((M, N), g).relu().to(DEV)
    dl = (torch.randn(M, C, generator=g) * 1e-3).to(DEV)
    w2 = (torch.randn(C, N, generator=g) * 0.1).to(DEV)
    act = h if src == "h" else ops.relu_bits(h)
    d64, dmodel, e_dz = mn.dz_from_dl(dl, w2, h > 0)
    splits, rps = mn.u8_wgrad_splits(M, N)
    assert_dl_route(x8, M, N, C)
    assert act.data_ptr() % 16 == 0 and dl.data_ptr() % 16 == 0
    what = f"u8 wgrad dl M {M} C {C} from {src} {variant}"
    with knobs(**DL_VARIANTS[variant]):
        amax = d64.abs().max().float().reshape(1) * (1 + 2.0 ** -20)
        E = mn.bound_exp(amax)
        gw, gb = flat_pair(ow, ob)
        ops.linear_wgrad_u8_dl(x8, dl, w2, act, gw, gb, amax=amax)
        check_wgrad(what + " | bound given", gw, gb, mn.u8_wgrad_model(dmodel, x8, ow, ob, ops.PIXEL_SCALE, E, splits, rps),
                    mn.u8_wgrad_budget(d64, x8, ow, ob, ops.PIXEL_SCALE, E, splits, e_dz=e_dz))
        Eg = mn.bound_exp(2 * float(dl.abs().sum(1).max()) * float(w2.abs().max()) * (1 + 2.0 ** -20))
        ref = mn.u8_wgrad_budget(d64, x8, ow, ob, ops.PIXEL_SCALE, Eg, splits, e_dz=e_dz)
        gw, gb = flat_pair(ow, ob)
        ops.linear_wgrad_u8_dl(x8, dl, w2, act, gw, gb)
        note(what + " | own bound", gw=gn.check_elementwise(gw, ref["gw"], extra=ref["gw_extra"], bf16=False, name=what),
             gb=gn.check_elementwise(gb, ref["gb"], extra=ref["gb_extra"], bf16=False, name=what))
        if variant == "default" and M >= 128:
            gw, gb = flat_pair(ow, ob)
            ops.linear_wgrad_u8_dl(x8, dl, w2, act, gw, gb, amax=amax, groups=(1, 1, 4))
            gs, grps = mn.u8_wgrad_splits(M, N, blocks=4)
            r2 = mn.u8_wgrad_budget(d64, x8, ow, ob, ops.PIXEL_SCALE, E, gs, e_dz=e_dz)
            assert torch.equal(gw[:64], ow[:64]) and torch.equal(gb[:64], ob[:64])  # the other range is untouched
            note(what + " | groups (1, 1, 4)",
                 gw=gn.check_elementwise(gw[64:], r2["gw"][64:], extra=r2["gw_extra"][64:], bf16=False, name=what),
                 gb=gn.check_elementwise(gb[64:], r2["gb"][64:], extra=r2["gb_extra"][64:], bf16=False, name=what))


def test_u8_wgrad_dominating_row():
    """One row of dz 2^20 times the rest: every other row sits on the planes' absolute floor 2^(E - 39), which the
    budget carries as 2^(E - 39) sum_m x (the term the older test allowed 1e-5 for)."""
    M, N = 4096, 128
    x8, dz, ow, ob = wgrad_case(M, N, 9)
    dz[17] = dz[17] * 2.0 ** 20
    E = mn.bound_exp(dz.abs().max())
    splits, rps = mn.u8_wgrad_splits(M, N)
    gw, gb = flat_pair(ow, ob)
    ops.linear_wgrad_u8(x8, dz, gw, gb)
    check_wgrad("u8 wgrad dominating row", gw, gb, mn.u8_wgrad_model(dz, x8, ow, ob, ops.PIXEL_SCALE, E, splits, rps),
                mn.u8_wgrad_budget(dz, x8, ow, ob, ops.PIXEL_SCALE, E, splits))
