"""fp64 references, fp32 rounding models, derived error bounds, input families and seeded defects for the GPT-2 bf16 GEMMs
(gemm_bf16.hip), the weight gradient (gemm_bf16_wgrad.hip), the tanh-GELU (gelu.h) and the embedding backward
(gpt2_ops.hip). Plain torch, runs on the CPU and on any device. The checker (check_elementwise, check_grouped, ulp_bf16,
U32 and the margins 3 and 1.25) is tests/gpt2_numerics.py's, unchanged; docs/NUMERICS.md ("GPT-2 GEMMs, GELU, embedding
gradient") has the rounding points and the derivation of every bound below."""
import math

import torch

import gpt2_numerics as gn
from gpt2_numerics import U32, rbf  # noqa: F401

BF = torch.bfloat16
TK = 64  # K-step of gemm_bf16.hip and of the weight gradient (tokens)
NAN = float("nan")

# ------------------------------------------------------------------------------------------------
# gemm_bf16: C[M, N] = A[M, K] . B[N, K]^T (+ bias). Products of bf16 numbers are exact in fp32; every output is one
# fp32 accumulation rounded once: elementwise mode with extra = (K + 8) 2^-24 (|A| |B|^T (+ |bias|)).
GEMM_SHAPES = [(1, 8, 64), (255, 184, 64), (257, 200, 128), (300, 264, 192), (513, 776, 320), (64, 776, 768)]
GEMM_FAMILIES = ["random sign", "positive", "row norms"]
PERSIST_SHAPE = (2200, 7432, 128)


def gemm_ref64(A, B, bias=None):
    """(ref64, magnitude) of A B^T (+ bias); B is [N, K]."""
    a, b = A.double(), B.double()
    ref, mag = a @ b.t(), a.abs() @ b.abs().t()
    if bias is not None:
        ref, mag = ref + bias.double(), mag + bias.double().abs()
    return ref, mag


def gemm_extra(mag, K):
    return (K + 8) * U32 * mag


def check_gemm(got, ref, mag, K, name="gemm"):
    return gn.check_elementwise(got, ref, extra=gemm_extra(mag, K), bf16=True, name=name)


def gemm_inputs(family, M, N, K, seed=0, device="cpu"):
    """A [M, K], B [N, K] (weights x 0.1), bias [N], U [M, N] (a pre-activation for the gelu' epilogues), all bf16."""
    g = torch.Generator().manual_seed(seed)
    A = torch.randn(M, K, generator=g)
    B = torch.randn(N, K, generator=g) * 0.1
    bias = torch.randn(N, generator=g)
    U = torch.randn(M, N, generator=g) * 2
    if family == "positive":  # |A| |B| is the result: nothing cancels
        A, B, bias = A.abs(), B.abs(), bias.abs()
    elif family == "row norms":  # row m scaled by 2^((m mod 9) - 4): a tolerance scaled by max|C| leaves small rows unchecked
        A = A * torch.exp2((torch.arange(M) % 9 - 4).float())[:, None]
    return tuple(t.to(BF).to(device) for t in (A, B, bias, U))


def selector_k(m, K):
    return (7 * m + 3) % K


def selector_rows(M, K, device="cpu"):
    """[M, K] bf16, row m one-hot at k(m) = (7 m + 3) mod K with value 1, rows m % 5 == 4 with value 0 (all-zero rows):
    C[m][n] == B[n][k(m)] bit for bit, and exactly 0 where the one-hot value is 0."""
    m = torch.arange(M)
    S = torch.zeros(M, K)
    S[m, selector_k(m, K)] = (m % 5 != 4).float()
    return S.to(BF).to(device)


def selector_expected(S, other):
    """S [R, K] selector rows, other [Q, K]: the [R, Q] matrix other[q][k(r)] * value(r) (exact)."""
    k = selector_k(torch.arange(S.shape[0], device=S.device), S.shape[1])
    val = S.float().sum(1)
    return (other.float()[:, k].t() * val[:, None]).to(BF)


def in_nan_frame(t, pad=8, guard_rows=1):
    """`t` [R, C] as a column slice (offset `pad`, row stride C + 2 pad, both multiples of 8 when C is) of a wider
    NaN-filled buffer with `guard_rows` NaN rows after the last one. Returns (view, buffer)."""
    R, C = t.shape
    buf = torch.full((R + guard_rows, C + 2 * pad), NAN, dtype=t.dtype, device=t.device)
    buf[:R, pad:pad + C] = t
    return buf[:R, pad:pad + C], buf


def frame_untouched(buf, t, pad=8):
    """The frame still holds NaN everywhere outside the slice, and the slice its data."""
    R, C = t.shape
    inner = torch.equal(buf[:R, pad:pad + C], t)
    mask = torch.ones_like(buf, dtype=torch.bool)
    mask[:R, pad:pad + C] = False
    return inner and bool(torch.isnan(buf[mask]).all())


# honest fp32 implementations and seeded defects (fp32 in, bf16 values out as fp32)
def gemm_fp32(A, B, bias=None, order="library", acc_bf16=False, double_round=False):
    """bf16(A B^T (+ bias)) in fp32. order "library": torch's fp32 matmul; "ksteps": 64-deep partial products added in
    order; "reverse": the same from the last K-step. Defects: acc_bf16 rounds the accumulator to bf16 after every K-step,
    double_round gives bf16(bf16(acc) + bias)."""
    a, b = A.float(), B.float()
    K = a.shape[1]
    if order == "library" and not acc_bf16:
        acc = a @ b.t()
    else:
        ks = list(range(0, K, TK))
        if order == "reverse":
            ks = ks[::-1]
        acc = torch.zeros(a.shape[0], b.shape[0], device=a.device)
        for k0 in ks:
            acc = acc + a[:, k0:k0 + TK] @ b[:, k0:k0 + TK].t()
            if acc_bf16:
                acc = rbf(acc)
    if bias is None:
        return rbf(acc)
    return rbf(rbf(acc) + bias.float()) if double_round else rbf(acc + bias.float())


def gemm_defect_last_k(A, B):
    """The last k lost on the last 8 columns."""
    C = gemm_fp32(A, B)
    C[:, -8:] = gemm_fp32(A[:, :-1], B[-8:, :-1], order="ksteps")
    return C


def gemm_defect_row_shift(A, B):
    """Row M - 1 written into row M - 2 of a ragged tile (row M - 1 keeps what the buffer held: zeros)."""
    C = gemm_fp32(A, B)
    C[-2] = C[-1]
    C[-1] = 0
    return C


def old_gemm_accepts(C, A, B, bias=None):
    """tests/test_gpt2_ops_gpu.py: assert_close(C, fp32 ref, rtol=1e-2, atol=1e-2 max|ref|) (the bias check keeps the
    atol of the product)."""
    ref = A.float() @ B.float().t()
    atol = 1e-2 * float(ref.abs().max())
    if bias is not None:
        ref = ref + bias.float()
    return bool(((C.float() - ref).abs() <= atol + 1e-2 * ref.abs()).all())


# ------------------------------------------------------------------------------------------------
# tanh-GELU in the kernels' sigmoid form: gelu(x) = x s, s = sigmoid(t), t = 2 beta (x + kappa x^3);
# gelu'(x) = s + 2 x s (1 - s) beta (1 + 3 kappa x^2)
GELU_BETA = math.sqrt(2.0 / math.pi)
GELU_KAPPA = 0.044715
GELU_XMAX = 64.0  # the exhaustive domain |x| <= 64
FLUSH = 2.0 ** -126  # the smallest normal fp32 number


def _gelu_parts64(x):
    """float64 t, s = sigmoid(t), w = 1 - s = sigmoid(-t) (each from exp of a non-positive argument: no cancellation,
    no overflow) and q = 2 x beta (1 + 3 kappa x^2)."""
    x = x.double()
    t = 2 * GELU_BETA * (x + GELU_KAPPA * x * x * x)
    e = torch.exp(-t.abs())
    big, small = 1 / (1 + e), e / (1 + e)
    s = torch.where(t >= 0, big, small)
    w = torch.where(t >= 0, small, big)
    return t, s, w, 2 * x * GELU_BETA * (1 + 3 * GELU_KAPPA * x * x)


def gelu_ref64(x):
    _, s, _, _ = _gelu_parts64(x)
    return x.double() * s


def gelu_grad_ref64(x):
    """gelu'(x) in float64 (both terms are products of factors without cancellation; their sum cancels near x = -0.75)."""
    _, s, w, q = _gelu_parts64(x)
    return s + q * s * w


def gelu_tanh_ref64(x):
    """0.5 x (1 + tanh u) in float64: cancels below x of about -6 (1 + tanh u is 0 in float64 for u < -18.4). Kept to show
    why it is not the reference."""
    x = x.double()
    return 0.5 * x * (1 + torch.tanh(GELU_BETA * (x + GELU_KAPPA * x * x * x)))


def _sig_abs_error(t, s, w):
    """Absolute fp32 error of the device's s = __fdividef(1, 1 + __expf(-t)), in units of 2^-24 (docs/NUMERICS.md):
    t carries 5 roundings (kappa and beta as fp32 constants, two products, one sum; x^3 of a bf16 x is exact in fp32),
    __expf is v_exp_f32(-t * log2(e)) (the constant and the product: 2 more roundings of the argument, so a relative
    (5 + 2) |t| 2^-24 in the result, plus the instruction's 1 ulp = 2 * 2^-24), E = exp(-t) enters s with the weight
    (1 - s), the sum 1 + E is one rounding and v_rcp_f32 1 ulp. Where 1 - s < 2^-26 the sum rounds to 1 and s is 1 exactly:
    the error is 1 - s itself."""
    e = s * (w * (7 * t.abs() + 2) + 3)
    return torch.where(w < 0.25 * U32, w / U32, e)


def gelu_fwd_budget(x):
    """(ref64, extra) of y = bf16(x s): relative error of s as above, one rounding of the product, and a = (|x| + 1)
    2^-126 for an s or a product below the fp32 normal range that the device may flush."""
    t, s, w, _ = _gelu_parts64(x)
    ref = x.double() * s
    extra = (_sig_abs_error(t, s, w) + s) * U32 * x.double().abs() + (x.double().abs() + 1) * FLUSH
    return ref, extra


def gelu_grad_abs_error(x):
    """Absolute fp32 error bound of gelu'(x) as gelu.h evaluates it (gy = 1, before the product with gy):
    e_s (1 + |q|) + 11 * 2^-24 |q s (1 - s)| + 2^-24 |gelu'|, q = 2 x beta (1 + 3 kappa x^2). The computed 1 - s inherits
    e_s absolutely (around s = 1 that is a large RELATIVE error of 1 - s, times q), and the two terms cancel near
    x = -0.75, so the bound is absolute."""
    t, s, w, q = _gelu_parts64(x)
    e_s = _sig_abs_error(t, s, w) * U32
    term2 = q * s * w
    return e_s * (1 + q.abs()) + 11 * U32 * term2.abs() + U32 * (s + term2).abs() + (1 + q.abs()) * FLUSH


def gelu_bwd_budget(gy, x):
    """(ref64, extra) of gx = bf16(gy gelu'(x)): |gy| e_gelu'(x), one rounding of the product, a = 2^-126."""
    d = gelu_grad_ref64(x)
    ref = gy.double() * d
    return ref, gy.double().abs() * gelu_grad_abs_error(x) + U32 * ref.abs() + FLUSH


def check_gelu_fwd(y, x, name="gelu"):
    ref, extra = gelu_fwd_budget(x)
    return gn.check_elementwise(y, ref, extra=extra, bf16=True, name=name)


def check_gelu_bwd(gx, gy, x, name="gelu'"):
    ref, extra = gelu_bwd_budget(gy, x)
    return gn.check_elementwise(gx, ref, extra=extra, bf16=True, name=name)


def gelu_fp32(x, zero_below=None, bf16=True):
    """Honest fp32 torch evaluation of gelu.h's formula, rounded to bf16 (bf16=False: left in fp32). zero_below seeds the
    defect y = 0 for x < it."""
    x = x.float()
    s = 1 / (1 + torch.exp(-2 * (GELU_BETA * (x + GELU_KAPPA * (x * x * x)))))
    y = x * s
    if zero_below is not None:
        y = torch.where(x < zero_below, torch.zeros_like(y), y)
    return rbf(y) if bf16 else y


def gelu_grad_fp32(gy, x, second_term=True, bf16=True):
    """gelu.h's gelu_grad_f in fp32 torch, rounded to bf16 (bf16=False: left in fp32). second_term=False seeds the defect
    gx = gy s."""
    x, gy = x.float(), gy.float()
    s = 1 / (1 + torch.exp(-2 * (GELU_BETA * (x + GELU_KAPPA * (x * x * x)))))
    d = s + 2 * x * s * (1 - s) * GELU_BETA * (1 + 3 * GELU_KAPPA * (x * x)) if second_term else s
    return rbf(gy * d) if bf16 else gy * d


def all_bf16(xmax=GELU_XMAX, device="cpu"):
    """Every bf16 bit pattern with |x| <= xmax: both zeros, the subnormals, both signs."""
    bits = torch.arange(0, 1 << 16, dtype=torch.int32).to(torch.int16)
    x = bits.view(BF)
    return x[x.float().abs() <= xmax].to(device)  # (NaN and inf compare false)


def bf16_beyond(xmax=GELU_XMAX, device="cpu"):
    """Every finite bf16 with |x| > xmax."""
    bits = torch.arange(0, 1 << 16, dtype=torch.int32).to(torch.int16)
    x = bits.view(BF)
    f = x.float()
    return x[torch.isfinite(f) & (f.abs() > xmax)].to(device)


def dgelu_epilogue_budget(A, B, U):
    """(ref64, extra) of epilogue 6, bf16(gelu'(U) * bf16(acc)): ref64 = gelu'64(U) acc64; two roundings."""
    K = A.shape[1]
    acc, mag = gemm_ref64(A, B)
    d = gelu_grad_ref64(U)
    extra = d.abs() * (0.5 * gn.ulp_bf16(acc) + gemm_extra(mag, K)) + gelu_grad_abs_error(U) * acc.abs() \
        + U32 * (d * acc).abs() + FLUSH
    return d * acc, extra


# ------------------------------------------------------------------------------------------------
# wgrad_bf16_: gw[M, N] = bf16(old + gy[T, M]^T x[T, N]), gb[M] = bf16(old + colsum(gy))
WG_BM, WG_BN = 256, 128  # wgrad_tiles.h's output tile
WGRAD_SHAPES = [(1, 8, 8), (63, 8, 16), (64, 8, 16), (65, 264, 136), (576, 264, 136), (1024, 8, 8), (1088, 8, 8),
                (2112, 264, 136), (2112, 520, 136)]  # (T, M, N)
WGRAD_WAVES_SHAPE = (2112, 2056, 1032)  # 9 x 9 tiles: 3 splits with WGRAD_WAVES = 1, 4 with 2


def wgrad_splits(M, N, T, waves=1):
    """(splits, tokens per split) as wgrad_bf16_splits and wgrad_bf16 compute them: floor(256 waves / tiles) splits, at
    least 8 K-steps of 64 tokens each, the tokens per split rounded up to whole K-steps."""
    tiles = -(-M // WG_BM) * -(-N // WG_BN)
    s = max(1, min(256 * max(1, waves) // tiles, T // (8 * TK)))
    tps = -(-(-(-T // s)) // TK) * TK
    return -(-T // tps), tps


def wgrad_bias_parts(M, N, T, waves=1, dma=True):
    """Partial sums added into gb: per split one, or (the DMA loop with several splits) one per column tile."""
    s, _ = wgrad_splits(M, N, T, waves)
    bparts = -(-N // WG_BN) if (dma and T % TK == 0 and s > 1) else 1
    return s * bparts


def wgrad_ref64(gy, x, old_w, old_b):
    g, xx = gy.double(), x.double()
    return {"gw": old_w.double() + g.t() @ xx, "gw_mag": g.abs().t() @ xx.abs() + old_w.double().abs(),
            "gb": old_b.double() + g.sum(0), "gb_mag": g.abs().sum(0) + old_b.double().abs()}


def wgrad_extras(ref, T, splits, parts):
    return {"gw": (T + splits + 8) * U32 * ref["gw_mag"], "gb": (T + parts + 8) * U32 * ref["gb_mag"]}


def wgrad_model(gy, x, old_w, splits, tps, drop_kstep=None, slabs_bf16=False, reverse=False):
    """fp32 model: per split the 64-token K-steps' products added in order, the splits' slabs added in split order,
    bf16(old + sum). Defects: drop_kstep = (split, K-step) left out, slabs_bf16 adds the slabs in bf16; reverse is a
    second honest order (K-steps and slabs from the last)."""
    g, xx = gy.float(), x.float()
    T = g.shape[0]
    slabs = []
    for s in range(splits):
        acc = torch.zeros(g.shape[1], xx.shape[1], device=g.device)
        ks = list(range(s * tps, min(T, (s + 1) * tps), TK))
        for i, k0 in (list(enumerate(ks))[::-1] if reverse else enumerate(ks)):
            if drop_kstep == (s, i):
                continue
            acc = acc + g[k0:k0 + TK].t() @ xx[k0:k0 + TK]
        slabs.append(acc)
    if reverse:
        slabs = slabs[::-1]
    if slabs_bf16:
        tot = old_w.float()
        for sl in slabs:
            tot = rbf(tot + rbf(sl))
        return tot
    tot = slabs[0]
    for sl in slabs[1:]:
        tot = tot + sl
    return rbf(old_w.float() + tot)


def wgrad_inputs(family, T, M, N, seed=0, device="cpu"):
    g = torch.Generator().manual_seed(seed)
    gy, x = torch.randn(T, M, generator=g), torch.randn(T, N, generator=g)
    old_w, old_b = torch.randn(M, N, generator=g), torch.randn(M, generator=g)
    if family == "positive":
        gy, x, old_w, old_b = gy.abs(), x.abs(), old_w.abs(), old_b.abs()
    return tuple(t.to(BF).to(device) for t in (gy, x, old_w, old_b))


def impulse_tokens(T, splits, tps):
    """0, 63, 64, T - 1 and the first and last token of every split."""
    ts = {0, 63, 64, T - 1}
    for s in range(splits):
        ts.update((s * tps, min(T, (s + 1) * tps) - 1))
    return sorted(t for t in ts if 0 <= t < T)


def old_wgrad_accepts(gw, ref):
    """tests/test_kernels_gpu.py test_wgrad_bf16: |err| <= 2^-7 (|gy|^T |x| + |old|) + 1e-6."""
    return bool(((gw.double() - ref["gw"]).abs() <= 2.0 ** -7 * ref["gw_mag"] + 1e-6).all())


# ------------------------------------------------------------------------------------------------
# embedding backward: wte.grad[v] = bf16(old + sum of g over the positions holding v), wpe.grad[s] = bf16(old + sum_b g)
EMB_SHAPES = [(3, 7, 64, 5), (4, 16, 32, 97), (2, 65, 260, 11), (5, 4, 768, 3)]  # (B, S, C, V)


def embedding_inputs(B, S, C, V, seed=0, device="cpu", extra_pos=5):
    g = torch.Generator().manual_seed(seed)
    tok = torch.randint(0, V, (B, S), generator=g)
    if V > 50:  # one token on a third of the positions: a long segment
        tok[:, ::3] = 11
    gout = torch.randn(B, S, C, generator=g).to(BF)
    old_w = (torch.randn(V, C, generator=g) * 0.5).to(BF)
    old_p = (torch.randn(S + extra_pos, C, generator=g) * 0.5).to(BF)
    return tuple(t.to(device) for t in (tok, gout, old_w, old_p))


def embedding_bwd_ref64(tok, gout, old_w, old_p):
    """References, magnitudes and term counts of both gradients; `touched` marks the wte rows some position holds."""
    B, S, C = gout.shape
    V = old_w.shape[0]
    g = gout.double().reshape(-1, C)
    flat = tok.reshape(-1)
    zw = torch.zeros(V, C, dtype=torch.float64, device=g.device)
    sw, mw = zw.clone().index_add_(0, flat, g), zw.clone().index_add_(0, flat, g.abs())
    count = torch.bincount(flat, minlength=V)
    gp, mp = old_p.double().clone(), old_p.double().abs()
    gp[:S] += gout.double().sum(0)
    mp[:S] += gout.double().abs().sum(0)
    return {"gw": old_w.double() + sw, "gw_extra": (count[:, None] + 8) * U32 * (mw + old_w.double().abs()),
            "gp": gp, "gp_extra": (B + 8) * U32 * mp, "touched": count > 0}


def embedding_bwd_fp32(tok, gout, old_w, old_p, overwrite=False):
    """fp32 sums in position / batch order, one rounding. overwrite seeds `=` for `+=` (the old gradient is lost)."""
    B, S, C = gout.shape
    g = gout.float().reshape(-1, C)
    sw = torch.zeros(old_w.shape, device=g.device).index_add_(0, tok.reshape(-1), g)
    touched = torch.bincount(tok.reshape(-1), minlength=old_w.shape[0]) > 0
    gw = rbf(sw if overwrite else old_w.float() + sw)
    gw = torch.where(touched[:, None], gw, old_w.float())
    gp = old_p.float().clone()
    gp[:S] = rbf(gout.float().sum(0) + (0 if overwrite else old_p.float()[:S]))
    return gw, gp


def check_embedding_bwd(gw, gp, ref, old_w, old_p, S, name="embedding"):
    a = gn.check_elementwise(gw, ref["gw"], extra=ref["gw_extra"], bf16=True, name=f"{name} wte.grad")
    b = gn.check_elementwise(gp, ref["gp"], extra=ref["gp_extra"], bf16=True, name=f"{name} wpe.grad")
    assert torch.equal(gw[~ref["touched"]].float(), old_w[~ref["touched"]].float()), f"{name}: an absent token's row moved"
    assert torch.equal(gp[S:].float(), old_p[S:].float()), f"{name}: a wpe row past S moved"
    return a, b
