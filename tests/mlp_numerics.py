"""fp64 references, fp32 rounding models, derived error bounds, input families and seeded defects for the MLP kernels
that compute fp32-accurate GEMMs on low-precision matrix cores: the bf16x3 engine (gemm_f32x3.hip) and the exact fp32
engine with the same contract (gemm_f32.hip), the two-fp16-plane engine (gemm_f16x2.hip: x2_split, x2_gemm, x2_wgrad_),
the uint8-pixel forward (mlp_u8.hip: u8_fwd), the classifier heads (head_xent.hip, head_block.h, head_tile.h: the block,
VALU, wide-K and generic heads, and the fused uint8 forward + head) and the uint8 weight-gradient family (mlp_u8.hip:
u8_wgrad in its dz, dl and ring forms, and the x3 engine's slab form). Plain torch, runs on the CPU and on any device.
The checker (check_elementwise with bf16=False, check_grouped, U32 and the margins 3 and 1.25) is tests/gpt2_numerics.py's,
unchanged; docs/NUMERICS.md ("MLP") has the rounding points and the derivation of every bound below.

A rounding model here is `chain_model`: the kernel's split done in torch, the kept products exact in float64, summed by
a k-ordered fp32 chain (one rounding per product). mlp_u8.hip's header records that the MFMA accumulates more accurately
than such a chain, so the chain is the safe side of the one-sided grouped test."""
import torch

import gpt2_numerics as gn
from gemm_numerics import NAN, selector_k  # noqa: F401
from gpt2_numerics import U32, check_elementwise, check_grouped  # noqa: F401

F16 = torch.float16
BF = torch.bfloat16

# ------------------------------------------------------------------------------------------------
# input families (fp32, built on the CPU generator)
FAMILIES = ["random sign", "positive", "row norms", "pow2 max", "dominant"]


def masky(shape, g):
    """A mask source with negative values, positive values and (a quarter of the elements) exact zeros: a kernel that
    keeps an element where mask >= 0 instead of mask > 0 differs on every zero."""
    r = torch.randn(shape, generator=g)
    return torch.where(r.abs() < 0.32, torch.zeros_like(r), r)


def gemm_inputs(family, M, N, K, seed=0, device="cpu"):
    """A [M, K], B [N, K] (x 0.1, weights), bias [N], old [M, N] (a non-zero accumulation target), cmask [M, N] and
    amask [M, K] (mask sources with exact zeros), all fp32.

    random sign: the plain case. positive: |A| |B| is the result, nothing cancels. row norms: row m of A scaled by
    2^(5 m mod 25 - 12), spread over 2^+-12 (a tolerance scaled by max|C| leaves the small rows unchecked). pow2 max:
    max|A| exactly 4 and max|B| one ulp below 1/4, the two sides of the bound_exp edge. dominant: one element of A and
    one of B 2^20 times their tensor's next largest (the fp16 planes' absolute floor carries every other element)."""
    g = torch.Generator().manual_seed(seed)
    A = torch.randn(M, K, generator=g)
    B = torch.randn(N, K, generator=g) * 0.1
    bias = torch.randn(N, generator=g)
    old = torch.randn(M, N, generator=g)
    cmask, amask = masky((M, N), g), masky((M, K), g)
    if family == "positive":
        A, B, bias, old = A.abs(), B.abs(), bias.abs(), old.abs()
    elif family == "row norms":
        A = A * torch.exp2(((5 * torch.arange(M)) % 25 - 12).float())[:, None]
    elif family == "pow2 max":
        A = A.clamp(-3.9, 3.9)
        A[M // 2, K // 3] = -4.0
        B = B.clamp(-0.24, 0.24)
        B[N // 3, K // 2] = float(torch.nextafter(torch.tensor(0.25), torch.tensor(0.0)))
    elif family == "dominant":
        A[M // 3, K // 2] = float(A.abs().max()) * 2.0 ** 20
        B[N // 2, K // 3] = -float(B.abs().max()) * 2.0 ** 20
    return tuple(t.float().to(device) for t in (A, B, bias, old, cmask, amask))


def selector_rows_f32(M, K, device="cpu"):
    """[M, K] fp32, row m one-hot at k(m) = (7 m + 3) mod K with value 1, rows m % 5 == 4 all zero: the product with B
    picks B[n][k(m)] (or exactly 0)."""
    m = torch.arange(M)
    S = torch.zeros(M, K)
    S[m, selector_k(m, K)] = (m % 5 != 4).float()
    return S.to(device)


def selected(S, other):
    """S [R, K] selector rows, other [Q, K] fp32: the [R, Q] matrix other[q][k(r)] * value(r), exact."""
    k = selector_k(torch.arange(S.shape[0], device=S.device), S.shape[1])
    return other[:, k].t() * S.sum(1)[:, None]


def n_problems(M, N):
    """A grouped check needs a few thousand elements for its RMS to be a stable statistic (with the 32 outputs of an
    8 x 4 problem two honest summation orders differ by 1.3 x in RMS): a small shape runs as this many independently
    seeded problems of that shape, whose outputs are stacked before they are checked."""
    return max(1, -(-4096 // (M * N)))


def stacked(M, N, fn):
    """fn(seed) -> {name: tensor [M, ...]} for n_problems(M, N) seeds, concatenated along the rows."""
    runs = [fn(seed) for seed in range(n_problems(M, N))]
    return {k: torch.cat([r[k] for r in runs]) for k in runs[0]}


PIXEL_FAMILIES = ["uniform", "all 0", "all 255", "one byte"]


def pixel_inputs(family, M, K, seed=0, device="cpu"):
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(0, 256, (M, K), generator=g, dtype=torch.uint8)
    if family == "all 0":
        x.zero_()
    elif family == "all 255":
        x.fill_(255)
    elif family == "one byte":  # one non-zero byte per row: y[m] = b + scale x W[:, k(m)], the selector of the pixel operand
        v = x[torch.arange(M), selector_k(torch.arange(M), K)].clamp_min(1)
        x.zero_()
        x[torch.arange(M), selector_k(torch.arange(M), K)] = v
    return x.to(device)


# ------------------------------------------------------------------------------------------------
# the rounding model
def chain_model(passes, interleave, cuts=(), reverse=False, group=1, drop=()):
    """fp32 model of a GEMM over planes: an fp32 chain over every kept product, one rounding each. passes:
    [(a [M, K], b [N, K])] of plane values (any float dtype, taken exactly in float64; a product is exact in float64).

    The chain runs over units. interleave=True: unit k holds the products of every pass at that k, added one after the
    other in the order of `passes` (the engines that issue all plane pairs inside a K-step: P K roundings).
    interleave=False: the passes follow each other on one extended k axis, one product per unit (x2's tripled K axis).
    `cuts` (unit indices) start a new slab from zero; the slabs are added in order in fp32. `group` > 1 adds that many
    consecutive units as one exact partial ("one fp32 add per K-step"). reverse runs every slab's units and the slabs
    backwards (a second honest order). `drop` (unit indices) are left out (seeded defects). Returns fp32 [M, N]."""
    A = torch.cat([p[0].double() for p in passes], 1)
    B = torch.cat([p[1].double() for p in passes], 1)
    P, K = len(passes), passes[0][0].shape[1]
    if interleave:
        units = [[p * K + k for p in range(P)] for k in range(K)]
    else:
        units = [[e] for e in range(P * K)]
    dropped = set(drop)
    bounds = [0] + [c for c in cuts if 0 < c < len(units)] + [len(units)]
    slabs = []
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        kept = [units[i] for i in range(lo, hi) if i not in dropped]
        if group > 1:
            chunks = [sum(kept[i:i + group], []) for i in range(0, len(kept), group)]
        else:
            chunks = [[e] for u in kept for e in u]
        if reverse:
            chunks = chunks[::-1]
        acc = torch.zeros(A.shape[0], B.shape[0], device=A.device)
        for idx in chunks:
            if len(idx) == 1:
                t = A[:, idx[0]:idx[0] + 1] @ B[:, idx[0]:idx[0] + 1].t()
            else:
                ix = torch.tensor(idx, device=A.device)
                t = A[:, ix] @ B[:, ix].t()
            acc = (acc.double() + t).float()
        slabs.append(acc)
    if reverse:
        slabs = slabs[::-1]
    tot = slabs[0]
    for s in slabs[1:]:
        tot = tot + s
    return tot


def honest_fp32(passes, order="library", kstep=32):
    """An honest fp32 torch implementation of the same kept products (the planes are exact in fp32): "library": torch's
    fp32 matmul per plane pair, the pairs added in the order of `passes`; "ksteps" / "reverse": kstep-deep fp32 matmuls added in k
    order / from the last."""
    K = passes[0][0].shape[1]
    if order == "library":
        acc = None
        for a, b in passes:
            t = a.float() @ b.float().t()
            acc = t if acc is None else acc + t
        return acc
    ks = list(range(0, K, kstep))
    if order == "reverse":
        ks = ks[::-1]
    acc = torch.zeros(passes[0][0].shape[0], passes[0][1].shape[0], device=passes[0][0].device)
    for k0 in ks:
        for a, b in passes:
            acc = acc + a[:, k0:k0 + kstep].float() @ b[:, k0:k0 + kstep].float().t()
    return acc


def epilogue(acc, epi, bias=None, old=None, cmask=None, relu_ge=False):
    """The engines' epilogues on an fp32 accumulator (one fp32 rounding per operation): 0 store (with cmask: kept where
    cmask > 0), 1 + bias, 2 relu(+ bias), 3 / 4 old + acc. relu_ge seeds the defect `>=` for `>` in the mask."""
    if epi == 0:
        if cmask is None:
            return acc
        keep = cmask >= 0 if relu_ge else cmask > 0
        return torch.where(keep, acc, torch.zeros_like(acc))
    if epi == 1:
        return acc + bias
    if epi == 2:
        return torch.relu(acc + bias)
    return old + acc


def gemm_budget(A, B, n_per_k, rel=0.0, floor=None, epi=0, bias=None, old=None, cmask=None, terms=1.0, adds=0):
    """(ref64, extra) of an epilogue of A B^T computed on planes, fp32 output, elementwise mode.

    extra = (n_per_k K + 8) u `terms` mag + rel mag + floor + epilogue, mag = |A| |B|^T: the project's any-order bound
    for the n_per_k K plane products actually summed (`terms` bounds the sum of the planes' |products| over |a b|),
    `rel` the relative error of what the planes represent (representation and dropped products), `floor` an absolute
    term. Epilogue: bias / accumulate add one operand and one rounding, u (mag + |bias| + |old|), accumulation
    2 u |old| more; ReLU and the masks add none (|relu(x) - relu(y)| <= |x - y|; a masked element is exactly 0).
    `adds`: split-K partials added into C one by one (atomics or slabs), each a rounding at the magnitude of what C
    holds by then: adds u (mag + |bias| + |old|)."""
    a, b = A.double(), B.double()
    K = a.shape[1]
    ref, mag = a @ b.t(), a.abs() @ b.abs().t()
    extra = (n_per_k * K + 8) * U32 * terms * mag + rel * mag
    if floor is not None:
        extra = extra + floor
    if epi in (1, 2):
        ref = ref + bias.double()
        extra = extra + U32 * (mag + bias.double().abs())
    if epi == 2:
        ref = torch.relu(ref)
    if epi in (3, 4):
        ref = ref + old.double()
        extra = extra + U32 * (mag + old.double().abs()) + 2 * U32 * old.double().abs()
    if adds:
        extra = extra + adds * U32 * (mag + (bias.double().abs() if epi in (1, 2) else 0.0)
                                      + (old.double().abs() if epi in (3, 4) else 0.0))
    if epi == 0 and cmask is not None:
        keep = cmask > 0
        ref, extra = ref * keep, extra * keep
    return ref, extra


def rowsum_budget(A, old):
    """(ref64, extra) of the fused row sums old[m] + sum_k A[m][k] (fp32 partial sums and atomics, any order)."""
    a = A.double()
    return old.double() + a.sum(1), (a.shape[1] + 8) * U32 * (a.abs().sum(1) + old.double().abs()) + 2 * U32 * old.double().abs()


# ------------------------------------------------------------------------------------------------
# gemm_f32x3: x = hi + mid + lo in bf16 (exact), six of the nine products
X3_BK = 32  # K-step
# x in [2^e, 2^(e + 1)): |mid| = |x - hi| <= 2^(e - 8) (half a bf16 ulp; 8 significant bits), and x - hi either is that
# power of two (then lo = 0) or lies in a binade at or below 2^(e - 9), so |lo| <= 2^(e - 17). The dropped
# mid lo + lo mid + lo lo is at most (2 * 2^-25 + 2^-34) |a b| (gemm_f32x3.hip's header: "below 2^-24 |a b|"); the
# typical element is near 2^-26, the worst case is what a bound may use
X3_DROP = 2.0 ** -24 + 2.0 ** -34
# sum of the kept |products| over |a b|: (|hi| + |mid| + |lo|)^2 <= (1 + 2^-7 + 2^-16)^2 < 1 + 2^-5
X3_TERMS = 1.0 + 2.0 ** -5
X3_SHAPES = [(8, 4, 4), (129, 130, 36), (257, 129, 100), (300, 132, 68), (512, 256, 320)]  # (M, N, K)
# a k-major operand needs rows % 4 == 0 (operand_ok): the shapes that take the place of (129, 130, 36) and
# (257, 129, 100) in the three layouts with a k-major operand, same tile straddles
X3_SHAPES_KM = [(8, 4, 4), (132, 132, 36), (260, 132, 100), (300, 132, 68), (512, 256, 320)]
X3_WGRAD_SHAPES = [(128, 784, 64), (128, 784, 1056), (128, 784, 2112), (36, 96, 2112)]  # (M = out, N = in, K = rows T)


def x3_eligible(M, N, K, a_km, b_km):
    """gemm_f32x3_eligible for contiguous fp32 operands (16-byte aligned bases)."""
    lda, ldb = (M if a_km else K), (N if b_km else K)
    ok_a = lda % 4 == 0 and (M % 4 == 0 if a_km else K % 4 == 0)
    ok_b = ldb % 4 == 0 and (N % 4 == 0 if b_km else K % 4 == 0)
    return ok_a and ok_b


def x3_pick_splits(M, N, K, a_km):
    """(splits, k per split) of the atomic epilogue as gemm_f32x3 computes them: one grid wave of 256 workgroups over
    the tiles (256 x 128, k-major A 128 x 128), at least 16 K-steps per split, whole K-steps."""
    bm = 128 if a_km else 256
    tiles = -(-M // bm) * -(-N // 128)
    s = max(1, min(256 // tiles, K // (16 * X3_BK)))
    kps = -(-(-(-K // s)) // X3_BK) * X3_BK
    return -(-K // kps), kps


def x3_split(x):
    """(hi, mid, lo) as fp32 tensors holding bf16 values, split3's arithmetic."""
    x = x.float()
    hi = gn.rbf(x)
    r1 = x - hi
    mid = gn.rbf(r1)
    lo = gn.rbf(r1 - mid)
    return hi, mid, lo


def x3_passes(A, B, third_order=True, kernel_order=False):
    """The six kept products of a k. kernel_order=True: as the kernel issues them inside a K-step, small terms first
    (mid mid, lo hi, hi lo, mid hi, hi mid, hi hi). The rounding model takes the other order, leading term first: every
    small term is then rounded at the accumulator's full magnitude, the safe side of a one-sided test (an honest chain
    in that order has 1.4 x the RMS error of the small-first one at K = 4). third_order=False seeds the defect that
    drops hi lo, lo hi and mid mid."""
    ah, am, al = x3_split(A)
    bh, bm, bl = x3_split(B)
    passes = [(ah, bh), (ah, bm), (am, bh)] + ([(ah, bl), (al, bh), (am, bm)] if third_order else [])
    return passes[::-1] if kernel_order else passes


def x3_budget(A, B, splits=0, **kw):
    """`splits`: the partials the atomic epilogue adds into C (x3_pick_splits)."""
    return gemm_budget(A, B, 6, rel=X3_DROP, terms=X3_TERMS, adds=splits, **kw)


def f32_skinny_splits(M, N, K, epi):
    """gemm_f32_skinny_splits: few output tiles (128 x 128) and a long K run as split-K, C pre-set to the bias (or kept,
    when accumulating) and every split's partial added with an fp32 atomic, then ReLU / the mask in a separate pass.
    0 = one pass."""
    tiles = -(-M // 128) * -(-N // 128)
    if epi == 4 or tiles > 32 or K < 256:
        return 0
    s = min(256 // tiles, K // 64)
    return s if s >= 4 else 0


def f32_budget(A, B, epi=0, splits=1, **kw):
    """gemm_f32 (fp32-input MFMA, VALU and small-K paths): K products, each rounded once more than an fma chain would
    (the product, then the sum): n = 2 K; the atomic adds of `splits` partials (epilogue 4), or of the skinny
    split-K form that the other epilogues take on their own."""
    M, K = A.shape
    adds = splits if epi == 4 else f32_skinny_splits(M, B.shape[0], K, epi)
    return gemm_budget(A, B, 2, epi=epi, adds=adds, **kw)


def old_x3_accepts(C, A, B):
    """tests/test_gemm_x3_gpu.py: |err| <= K 2^-24 |A| |B|^T + 1e-30."""
    a, b = A.double(), B.double()
    return bool(((C.double() - a @ b.t()).abs() <= a.shape[1] * U32 * (a.abs() @ b.abs().t()) + 1e-30).all())


def old_assert_close_accepts(C, ref64, rtol=1e-5, atol=1e-5):
    """torch.testing.assert_close against the fp32-rounded fp64 result (test_x3_epilogues and the gb checks)."""
    r = ref64.float().double()
    return bool(((C.double() - r).abs() <= atol + rtol * r.abs()).all())


# ------------------------------------------------------------------------------------------------
# gemm_f16x2: two fp16 planes of x 2^(14 - E), E = bound_exp(max |amax|)
X2_TK = 64  # K-step of x2_gemm; also the token K-step of x2_wgrad_
X2_REP = 2.0 ** -23  # |hi + lo - x'| <= 2^-23 |x'| where lo is a normal fp16
X2_LL = 2.0 ** -22  # the dropped lo lo: |lo| <= 2^-11 |x'| on both sides
X2_GEMM_SHAPES = [(256, 256, 64), (257, 320, 192), (700, 320, 256)]  # (M, N, K)
X2_WGRAD_SHAPES = [(64, 256, 128), (2112, 256, 128), (2112, 520, 136), (64, 520, 136), (2100, 520, 136),
                   (2100, 256, 128)]  # (T, M, N); T = 2100 runs the staged loop only
X2_WBM, X2_WBN = 256, 128  # wgrad_tiles.h's output tile


def bound_exp(v):
    """E with |v| < 2^E for finite v >= 0 (v = 2^k gives k + 1), -100 for 0, clamped to [-100, 120]."""
    v = float(v)
    if v == 0.0:
        return -100
    _, e = torch.frexp(torch.tensor(v, dtype=torch.float32))  # v = m 2^e, m in [0.5, 1)
    return min(max(int(e), -100), 120)


def x2_planes(x, amax=None, E=None):
    """(hi, lo, scale, E): fp16 planes of x' = x 2^(14 - E) as x2_split computes them (x' exact, hi = fp16(x'),
    lo = fp16(x' - hi) with the difference exact in fp32) and the dequantisation factor 2^(E - 14). amax: any tensor
    whose max |.| is the bound (default: x itself). A bound that is too small overflows hi to inf."""
    if E is None:
        E = bound_exp((x if amax is None else amax).abs().max())
    xs = x.float() * 2.0 ** (14 - E)
    hi = xs.to(F16)
    lo = (xs - hi.float()).to(F16)
    return hi, lo, 2.0 ** (E - 14), E


def x2_rep_bound(x, E):
    """|(hi + lo) 2^(E - 14) - x| <= max(2^-23 |x|, 2^(E - 39)). x' - hi is below half an fp16 ulp of x', 2^(e - 11) for
    x' in [2^e, 2^(e + 1)), so it sits in a binade at or below 2^(e - 12) and rounds to lo within 2^(e - 23) <= 2^-23
    |x'| while lo is normal (e >= -2); a subnormal lo is a multiple of 2^-24: 2^-25 absolute, 2^(E - 39) unscaled.
    (The relative bound alone holds for |x| >= 2^(E - 16): one binade above the 2^(E - 17) of gemm_f16x2.hip's header,
    whose 2^(E - 39) covers that binade.)"""
    return torch.maximum(X2_REP * x.double().abs(), torch.full_like(x.double(), 2.0 ** (E - 39)))


def x2_passes(A, B, Ea=None, Eb=None, lo_hi=True):
    """Scaled plane passes in the kernel's segment order (hi hi, hi lo, lo hi) and the product of the two scales.
    lo_hi=False seeds the defect that drops the third segment."""
    ah, al, sa, _ = x2_planes(A, E=Ea)
    bh, bl, sb, _ = x2_planes(B, E=Eb)
    passes = [(ah, bh), (ah, bl)] + ([(al, bh)] if lo_hi else [])
    return passes, sa * sb


def x2_budget(A, B, **kw):
    """x2_gemm: 3 K products on the tripled K axis; per operand the representation error 2^-23 relative plus the
    2^(E - 39) floor against the other operand's row sum; the dropped lo lo 2^-22 (cross terms of the three below
    2^-44); the epilogue's fma(acc, sa sb, bias) is the one rounding gemm_budget counts for a bias and exact (powers of
    two) without one."""
    a, b = A.double().abs(), B.double().abs()
    Ea, Eb = bound_exp(a.max()), bound_exp(b.max())
    floor = 2.0 ** (Ea - 39) * b.sum(1)[None, :] + 2.0 ** (Eb - 39) * a.sum(1)[:, None] + 2.0 ** (Ea + Eb - 78) * a.shape[1]
    return gemm_budget(A, B, 3, rel=2 * X2_REP + X2_LL + 2.0 ** -40, floor=floor, terms=1.0 + 2.0 ** -9, **kw)


def x2_wgrad_splits(M, N, T):
    """(splits, K-steps per split) of x2_wgrad_ over the extended axis of 3 ceil(T / 64) K-steps."""
    tiles = -(-M // X2_WBM) * -(-N // X2_WBN)
    nks = -(-T // X2_TK)
    s = max(1, min(max(1, 256 // tiles), 3 * nks // 8))
    kps = -(-3 * nks // s)
    return -(-3 * nks // kps), kps


def x2_wgrad_model(dz, x, old_w, reverse=False, drop_kstep=None):
    """fp32 model of gw = old + sdz sx sum_slabs: dz^T x on the extended token axis (hi hi, hi lo, lo hi; ragged T padded
    with zero tokens to whole 64-token K-steps as the kernel's K-steps are), cut into the kernel's splits, each slab a
    token-ordered fp32 chain, the slabs added in order, one multiply by the scales (exact) and one add.
    drop_kstep = (split, K-step) seeds a lost K-step."""
    T = dz.shape[0]
    pad = -T % X2_TK
    zp = lambda t: torch.cat([t, torch.zeros(pad, t.shape[1], dtype=t.dtype, device=t.device)])  # noqa: E731
    dh, dl, sd, _ = x2_planes(dz)
    xh, xl, sx, _ = x2_planes(x)
    passes = [(zp(dh).t(), zp(xh).t()), (zp(dh).t(), zp(xl).t()), (zp(dl).t(), zp(xh).t())]
    splits, kps = x2_wgrad_splits(dz.shape[1], x.shape[1], T)
    cuts = [s * kps * X2_TK for s in range(1, splits)]
    drop = ()
    if drop_kstep is not None:
        e0 = (drop_kstep[0] * kps + drop_kstep[1]) * X2_TK
        drop = range(e0, e0 + X2_TK)
    acc = chain_model(passes, False, cuts=cuts, reverse=reverse, drop=drop)
    return old_w.float() + acc * (sd * sx)


def x2_wgrad_budget(dz, x, old_w, old_b):
    """References and extras of gw [M, N] and gb [M]. gw: x2_budget's terms over K = T with the slab adds and the
    accumulation; gb = old + sdz sum_t (hi + lo): 2 T fp16 values summed in fp32 in any order, dz's representation
    error (relative and, per token, the floor), the scale (exact) and the accumulation."""
    splits, _ = x2_wgrad_splits(dz.shape[1], x.shape[1], dz.shape[0])
    ref, extra = x2_budget(dz.t(), x.t(), epi=3, old=old_w)
    g, ob = dz.double(), old_b.double()
    T = g.shape[0]
    extra = extra + splits * U32 * (g.abs().t() @ x.double().abs())
    E = bound_exp(g.abs().max())
    parts = splits * -(-x.shape[1] // X2_WBN) + 32  # bias partials of the DMA loop, 16 + 16 partial sums of the reduction
    gb_extra = (2 * T + parts + 8) * U32 * g.abs().sum(0) + X2_REP * g.abs().sum(0) + T * 2.0 ** (E - 39) \
        + U32 * (g.abs().sum(0) + ob.abs()) + 2 * U32 * ob.abs()
    return {"gw": ref, "gw_extra": extra, "gb": ob + g.sum(0), "gb_extra": gb_extra}


def x2_gb_fp32(dz, old_b, lo=True, reverse=False):
    """fp32 model of the bias gradient: token-ordered chain of hi, then of lo (segment 0, segment 2), scaled, added.
    lo=False seeds the defect that sums the hi plane only."""
    dh, dl, sd, _ = x2_planes(dz)
    rows = [dh.float()] + ([dl.float()] if lo else [])
    acc = torch.zeros(dz.shape[1], device=dz.device)
    for pl in rows:
        for t in (range(pl.shape[0] - 1, -1, -1) if reverse else range(pl.shape[0])):
            acc = acc + pl[t]
    return old_b.float() + acc * sd


def old_x2_accepts(C, A, B, K=None):
    """tests/test_gemm_x2_gpu.py's `bound`: 2 ((K 2^-24 + 2^-20) |A| |B|^T + 2^(Ea - 38) sum|b| + 2^(Eb - 38) sum|a|)."""
    a, b = A.double(), B.double()
    K = a.shape[1] if K is None else K
    Ea, Eb = bound_exp(a.abs().max()), bound_exp(b.abs().max())
    bound = 2 * ((K * U32 + 2.0 ** -20) * (a.abs() @ b.abs().t())
                 + 2.0 ** (Ea - 38) * b.abs().sum(1)[None, :] + 2.0 ** (Eb - 38) * a.abs().sum(1)[:, None]) + 1e-30
    return bool(((C.double() - a @ b.t()).abs() <= bound).all())


# ------------------------------------------------------------------------------------------------
# u8_fwd: y = relu?(fma(acc, scale / 2^8, b)), acc = sum_k x[m][k] (hi + lo)[n][k] with fp16 planes of W 2^8
U8_FBK = 64  # K-step; the last one runs tail_substeps(K) of its 4 MFMA substeps
U8_FWD_MIN_ROWS = 4096  # linear_fwd_u8 takes the uint8 kernel from this many rows (fewer: the fp32 engines)
U8_FWD_NK = [(128, 16), (128, 64), (256, 96), (128, 112), (128, 784), (256, 784)]  # (N, K)
U8_FWD_ROWS = [4096, 4097, 4140, 4617]  # 4096 + the issue's M mod 256 (0, 1, 44, 9): see NUMERICS.md


def u8_tail_substeps(K):
    v = K - (-(-K // U8_FBK) - 1) * U8_FBK
    return 4 if v > 24 else 3 if v > 16 else 2 if v > 8 else 1


def u8_w_planes(w):
    """fp16 planes (hi, lo) of W 2^8 (u8_planes.h)."""
    s = w.float() * 256.0
    hi = s.to(F16)
    return hi, (s - hi.float()).to(F16)


def u8_scale(scale):
    """The epilogue's factor: fp32(scale) / 2^8, and the float64 value of fp32(scale) the reference uses."""
    s = float(torch.tensor(scale, dtype=torch.float32))
    return s / 256.0, s


def u8_fwd_passes(x8, w, lo=True):
    """(x, hi) then (x, lo) at every k (both planes' MFMAs run inside the K-step; leading term first is the safe order,
    see x3_passes). lo=False seeds the forward on the hi plane only."""
    hi, lo_ = u8_w_planes(w)
    return [(x8, hi)] + ([(x8, lo_)] if lo else [])


def u8_fwd_model(x8, w, b, scale, relu, lo=True, reverse=False, drop_last=0):
    """fp32 model: the k-ordered chain, then one fma with the bias. drop_last leaves the last k's out (a lost tail
    substep)."""
    K = x8.shape[1]
    acc = chain_model(u8_fwd_passes(x8, w, lo), True, reverse=reverse, drop=range(K - drop_last, K))
    sc, _ = u8_scale(scale)
    y = (acc.double() * sc + b.double()).float()
    return torch.relu(y) if relu else y


def u8_fwd_budget(x8, w, b, scale, relu):
    """(ref64, extra): 2 K exact products summed in fp32; W's planes are W to 2^-23 relative for |W| >= 2^-9 and to
    2^-33 below (u8_planes.h; the bound takes their sum); one rounding for the epilogue's fma. The reference multiplies
    by the fp32 value of `scale` (the kernel's input)."""
    sc, s64 = u8_scale(scale)
    x, wd = x8.double(), w.double()
    acc, mag = x @ wd.t(), x @ wd.abs().t()
    ref = acc * s64 + b.double()
    extra = s64 * ((2 * x8.shape[1] + 8) * U32 * (1 + 2.0 ** -10) * mag + X2_REP * mag + 2.0 ** -33 * x.sum(1)[:, None]) \
        + U32 * (s64 * mag + b.double().abs())
    return (torch.relu(ref) if relu else ref), extra


def relu_bits_of(y):
    """int32 [M, N / 32]: bit n % 32 of word n / 32 = (y[m][n] > 0), the uint8 kernels' mask layout."""
    M, N = y.shape
    sh = torch.arange(32, dtype=torch.int64, device=y.device)
    b = (y > 0).view(M, N // 32, 32).to(torch.int64)
    return (b << sh).sum(-1).to(torch.int32)


def old_u8_fwd_accepts(y, x8, w, b):
    """tests/test_gemm_x3_gpu.py test_linear_fwd_u8_matches_fp32_reference: |err| <= 2 K 2^-24 (x/255 |W|^T + |b|)."""
    xf, wd = x8.double() / 255.0, w.double()
    want = torch.relu(xf @ wd.t() + b.double())
    bound = x8.shape[1] * U32 * (xf @ wd.abs().t() + b.double().abs()) + 1e-30
    return bool(((y.double() - want).abs() <= 2 * bound).all())


# ------------------------------------------------------------------------------------------------
# classifier heads (head_xent.hip: head_block_kernel on fp16 planes, head_fused_kernel (VALU, both rows-per-chunk
# forms), head_lds_kernel, head_generic_kernel; head_tile.h's softmax_dz). One budget for all of them: the plane
# arithmetic of head_block.h gives the loosest logit error, the fp32 VALU heads stay inside it.
HEAD_ROWS = [1, 15, 16, 17, 255, 256, 257, 2049]
HEAD_FAMILIES = ["small", "saturated", "offset", "equal", "tie 3 4", "tie 1 9", "tie 0 15"]
HEAD_BLOCKS_MAX = 2048  # more slabs than any head grid writes (1024 blocks at most)


def head_families(C):
    return [f for f in HEAD_FAMILIES if not f.startswith("tie") or int(f.split()[2]) < C]


def head_inputs(family, M, K, C, seed=0, device="cpu"):
    """h [M, K] (a ReLU output: half exact zeros), W2 [C, K], b2 [C], target [M] in [0, C), old gW2 / gb2 (non-zero).

    small: logits about +-0.3. saturated: logits spread to +-30, the target at the maximum on even rows and random on
    odd rows. offset: |z| about 10^4 through a common bias offset. equal: every class the same row of W2 and the same
    bias (all logits bit-equal: the first index wins). tie i j: classes i and j identical and lifted above the others,
    an exact two-way tie for the maximum on most rows."""
    g = torch.Generator().manual_seed(seed)
    h = torch.randn(M, K, generator=g).relu()
    w = torch.randn(C, K, generator=g) * (0.03 * (128.0 / K) ** 0.5)
    b = torch.randn(C, generator=g) * 0.1
    t = torch.randint(0, C, (M,), generator=g)
    if family == "saturated":
        w = w * 100.0
        top = (h.double() @ w.double().t() + b.double()).argmax(1)
        t = torch.where(torch.arange(M) % 2 == 0, top, t)
    elif family == "offset":
        b = b + 1.0e4
    elif family == "equal":
        w, b = w[:1].expand(C, K).contiguous(), b[:1].expand(C).contiguous()
        t = torch.where(torch.arange(M) % 2 == 0, torch.zeros_like(t), t)
    elif family.startswith("tie"):
        i, j = (int(v) for v in family.split()[1:])
        w[j], b[j] = w[i], b[i] + 0.0
        b[i] = b[j] = float(b.max()) + 0.5
        r = torch.arange(M) % 4  # the first of the pair twice as often as the second: the two tie rules count differently
        t = torch.where(r < 2, torch.full_like(t, i), torch.where(r == 2, torch.full_like(t, j), t))
    old_w, old_b = torch.randn(C, K, generator=g), torch.randn(C, generator=g)
    return tuple(v.to(device) for v in (h.float(), w.float(), b.float(), t, old_w, old_b))


def head_budget(h, w, b, t, scale, old_w=None, old_b=None, e_h=None, planes=True):
    """float64 references and derived extras of every head output (docs/NUMERICS.md "MLP", heads).

    e_z (per row, the largest over the classes): z_c = b_c + sum_k h_k W_ck on fp16 planes, 3 K products,
      (3 K + 8) u (1 + 2^-9) mag_c + (2 * 2^-23 + 2^-22) mag_c + 2^(Eh - 39) sum_k |W_ck| + 2^(Ew - 39) sum_k |h_k|
      + 2 u |z_c|, mag_c = sum_k |h_k W_ck| + |b_c|, Eh / Ew = bound_exp of max |h| / max |W2|.
    d_c: the relative error of p_c = exp2(fma(z_c, log2e, -max log2e)) beyond the factor all classes of a row share
      (the rounding of max log2e, which cancels in p / sum p): expm1(2 e_z + 2 u |z_c - max| + 2 u).
    dl_c = fma(p_c, scale rcp(sum p), -scale [c = t]): scale (s_c (d_c + d_den + (C + 8) u) + 2 u) + u |dl_c| + 2^-126,
      d_den = sum_c s_c d_c the relative error of the denominator's terms, (C + 8) u its sum, v_rcp_f32 and the product;
      2 u scale for an implementation that rounds softmax - onehot before the product (the VALU heads; the fma of
      softmax_dz does not).
    loss_r = fma(log(sum p), ln2, max) - z_t: 2 e_z + d_den + (C + 8) u + 4 u (|lse| + |max| + |z_t|) + u |loss_r|; the
      sum over rows and blocks (rows + blocks + 8) u sum |loss_r|.
    dx = sum_c dl_c W_c: sum_c e_dl |W_c| + (C + 8) u sum_c |dl_c W_c|.
    gW2 = old + dl^T h on planes of dl scaled from |dl| <= loss_scale: sum_r e_dl |h| + (3 M + blocks + 8) u mag
      + (2 * 2^-23 + 2^-22) mag + 2^(Es - 39) sum_r |h| + 2^(Eh - 39) sum_r |dl| + 3 u |old|.
    gb2 = old + sum_r dl: sum_r e_dl + (M + blocks + 8) u sum_r |dl| + 3 u |old|.
    e_h (the fused forward + head: h is the float64 forward and e_h its forward budget): e_z gains sum_k e_h |W_ck|, gW2
    gains sum_r |dl| e_h.
    planes=False: the fp32 heads (head_fused_kernel, head_lds_kernel, head_generic_kernel), whose logits and dW2 are
    fp32 FMA sums of the fp32 operands: e_z = max_c [(K + 8) u mag_c + 2 u |z_c|] and gW2 = sum_r e_dl |h| +
    (M + blocks + 8) u |dl|^T |h| + 3 u |old|, no plane terms."""
    hd, wd, bd = h.double(), w.double(), b.double()
    M, K = hd.shape
    C = wd.shape[0]
    s = float(torch.tensor(scale, dtype=torch.float32))
    z = hd @ wd.t() + bd
    mag = hd.abs() @ wd.abs().t() + bd.abs()
    Eh, Ew, Es = bound_exp(hd.abs().max()), bound_exp(wd.abs().max()), bound_exp(abs(s))
    if planes:
        ez_c = ((3 * K + 8) * U32 * (1 + 2.0 ** -9) + 2 * X2_REP + X2_LL) * mag + 2.0 ** (Eh - 39) * wd.abs().sum(1)[None, :] \
            + 2.0 ** (Ew - 39) * hd.abs().sum(1)[:, None] + 2 * U32 * z.abs()
    else:
        ez_c = (K + 8) * U32 * mag + 2 * U32 * z.abs()
    if e_h is not None:
        ez_c = ez_c + e_h.double() @ wd.abs().t()
    ez = ez_c.amax(1)
    mx = z.amax(1)
    lse = torch.logsumexp(z, 1)
    sm = torch.exp(z - lse[:, None])
    onehot = torch.zeros_like(z)
    onehot[torch.arange(M, device=z.device), t] = 1.0
    dl = s * (sm - onehot)
    d_c = torch.expm1(2 * ez[:, None] + 2 * U32 * (z - mx[:, None]).abs() + 2 * U32)
    d_den = (sm * d_c).sum(1)
    e_dl = s * (sm * (d_c + d_den[:, None] + (C + 8) * U32) + 2 * U32) + U32 * dl.abs() + 2.0 ** -126
    zt = z.gather(1, t[:, None])[:, 0]
    loss_r = lse - zt
    e_loss_r = 2 * ez + d_den + (C + 8) * U32 + 4 * U32 * (lse.abs() + mx.abs() + zt.abs()) + U32 * loss_r.abs()
    top2 = z.topk(min(2, C), 1).values
    gap = (top2[:, 0] - top2[:, -1]) if C > 1 else torch.full_like(mx, float("inf"))
    first = z.argmax(1)
    ambiguous = (gap > 0) & (gap <= 2 * ez)  # a bit-exact tie (gap 0) is decided by the first-index rule
    sure = ((first == t) & ~ambiguous).sum()
    out = {"z": z, "ez": ez, "dl": dl, "dl_extra": e_dl, "loss": loss_r.sum(),
           "loss_extra": e_loss_r.sum() + (M + HEAD_BLOCKS_MAX + 8) * U32 * loss_r.abs().sum(),
           "correct_min": int(sure), "correct_max": int(sure + ambiguous.sum()),
           "dx": dl @ wd, "dx_extra": e_dl @ wd.abs() + (C + 8) * U32 * (dl.abs() @ wd.abs())}
    # rows of the grouped dx check (check_grouped's fp32_extra): the fp32 steps of dl whose rounding a torch model cannot
    # reproduce. exp(z - lse) takes the rounding of lse and of the difference, u (|lse| + |z - lse|), twice (log and
    # exp arguments), the device's exp and log at 1 ulp each and their constants (6 u); softmax - onehot one rounding
    # (2 u scale, where the two cancel it is the whole result); the class sum (C + 8) u
    e_form = s * (sm * (2 * U32 * (lse.abs()[:, None] + (z - lse[:, None]).abs()) + 6 * U32) + 2 * U32)
    out["dx_form_extra"] = e_form @ wd.abs() + (C + 8) * U32 * (dl.abs() @ wd.abs())
    if old_w is not None:
        gmag = dl.abs().t() @ hd.abs()
        out["gw"] = old_w.double() + dl.t() @ hd
        if planes:
            out["gw_extra"] = e_dl.t() @ hd.abs() + ((3 * M + HEAD_BLOCKS_MAX + 8) * U32 + 2 * X2_REP + X2_LL) * gmag \
                + 2.0 ** (Es - 39) * hd.abs().sum(0)[None, :] + 2.0 ** (Eh - 39) * dl.abs().sum(0)[:, None] \
                + 3 * U32 * old_w.double().abs() + (0.0 if e_h is None else dl.abs().t() @ e_h.double())
        else:
            out["gw_extra"] = e_dl.t() @ hd.abs() + (M + HEAD_BLOCKS_MAX + 8) * U32 * gmag + 3 * U32 * old_w.double().abs()
        out["gb"] = old_b.double() + dl.sum(0)
        out["gb_extra"] = e_dl.sum(0) + (M + HEAD_BLOCKS_MAX + 8) * U32 * dl.abs().sum(0) + 3 * U32 * old_b.double().abs()
    return out


def head_fp32(h, w, b, t, scale, old_w, old_b, form="exp2", defect=None, z=None):
    """An honest fp32 torch head. form "exp2": softmax_dz's operations (exp2 / log with the kernel's constants);
    "lse": head_lds_kernel's (exp(z - lse): with saturated logits the rounding of lse, u |lse|, is the whole error of
    the target's dl); "library": torch's log_softmax. Seeded defects: "clamped rows" (row M - 1 counted again for the rows of a last
    16-row tile past M), "last index" (the last maximal index wins a tie), "no max" (softmax without the max
    subtraction), "overwrite" (`=` for `+=` in gW2 / gb2), "dx zero", "lost row" (one row's loss lost), "mask ge"
    (dx kept where h >= 0). `z`: logits computed by the caller (head_chain_models). Returns loss, correct, dl, dx
    (masked by h > 0), gw, gb."""
    h, w, b = h.float(), w.float(), b.float()
    M = h.shape[0]
    s = torch.tensor(scale, dtype=torch.float32)
    # (one reduction per (row, class) in the same order: identical W2 rows give bit-equal logits, as the kernels' do; a
    # library matmul blocks the classes and does not)
    if z is None:
        z = (h[:, None, :] * w[None, :, :]).sum(-1) + b
    ar = torch.arange(M, device=h.device)
    if form == "library" and defect != "no max":
        lp = torch.log_softmax(z, 1)
        sm, loss_r = lp.exp(), -lp[ar, t]
    elif form == "lse":  # head_lds_kernel's operations: lse = max + log(sum exp(z - max)), softmax = exp(z - lse)
        mx = z.amax(1, keepdim=True)
        lse = mx + torch.log(torch.exp(z - mx).sum(1, keepdim=True))
        sm, loss_r = torch.exp(z - lse), lse[:, 0] - z[ar, t]
    else:
        mx = torch.zeros_like(z[:, :1]) if defect == "no max" else z.amax(1, keepdim=True)
        p = torch.exp2(z * gn.LOG2E - mx * gn.LOG2E)
        se = p.sum(1, keepdim=True)
        sm = p * (1.0 / se)
        loss_r = (torch.log(se) + mx)[:, 0] - z[ar, t]
    first = z.argmax(1)
    if defect == "last index":
        first = z.shape[1] - 1 - z.flip(1).argmax(1)
    onehot = torch.zeros_like(z)
    onehot[ar, t] = 1.0
    dl = s * (sm - onehot)
    corr = (first == t).float()
    gdl, gh = dl, h
    if defect == "clamped rows" and M % 16:
        extra = 16 - M % 16
        loss_r = torch.cat([loss_r, loss_r[-1:].expand(extra)])
        corr = torch.cat([corr, corr[-1:].expand(extra)])
        gdl, gh = torch.cat([dl, dl[-1:].expand(extra, -1)]), torch.cat([h, h[-1:].expand(extra, -1)])
    if defect == "lost row":
        loss_r = loss_r[1:]
    dx = dl @ w
    dx = torch.zeros_like(dx) if defect == "dx zero" else dx * ((h >= 0) if defect == "mask ge" else (h > 0))
    gw, gb = gdl.t() @ gh, gdl.sum(0)
    if defect != "overwrite":
        gw, gb = old_w.float() + gw, old_b.float() + gb
    return {"loss": loss_r.sum(), "correct": int(corr.sum()), "dl": dl, "dx": dx, "gw": gw, "gb": gb}


def head_chain_models(h, w, b, t, scale, old_w, lost=None):
    """fp32 rounding models of dx and gW2 for the wide-K head, which returns no dl (head_lds_kernel): the logits a
    k-ordered fp32 chain plus the bias (the safe side: the kernel's lane tree is more accurate), dl from them with the
    kernel's own operations (head_fp32's "lse" form), dx = dl W2 a class-ordered chain, gW2 = old + dl^T h a row-ordered chain.
    lost = (row, k0, k1) seeds a dW2 that loses that row's contribution to columns k0 .. k1 - 1. Returns {dx, gw}."""
    z = chain_model([(h, w)], True) + b.float()
    dl = head_fp32(h, w, b, t, scale, old_w, old_w[:, 0], form="lse", z=z)["dl"]
    hh = h.float()
    if lost is not None:
        hh = hh.clone()
        hh[lost[0], lost[1]:lost[2]] = 0
    return {"dx": chain_model([(dl, w.t())], True), "gw": old_w.float() + chain_model([(dl.t(), hh.t())], True), "dl": dl}


def check_head(out, ref, h, what="head", masked=True, note=None):
    """Every output present in `out` against its budget: loss (one number), correct (the first-index rule's count,
    exact up to the rows whose float64 top-two gap is inside the logits' error), dl, dx (times h > 0 when masked: a
    masked element is exactly 0), gw, gb. Returns {name: use}."""
    use = {}
    one = lambda v: torch.as_tensor(v, dtype=torch.float64, device=h.device).reshape(1)  # noqa: E731
    if "loss" in out:
        use["loss"] = check_elementwise(one(out["loss"]), one(ref["loss"]), extra=one(ref["loss_extra"]), bf16=False,
                                        name=f"{what} loss")
    if "correct" in out:
        c = int(out["correct"])
        if not ref["correct_min"] <= c <= ref["correct_max"]:
            raise gn.Budget(f"{what}: correct {c} outside [{ref['correct_min']}, {ref['correct_max']}]")
    if "dl" in out:
        use["dl"] = check_elementwise(out["dl"], ref["dl"], extra=ref["dl_extra"], bf16=False, a=1e-300, name=f"{what} dl")
    if "dx" in out:
        keep = (h > 0) if masked else torch.ones_like(h, dtype=torch.bool)
        use["dx"] = check_elementwise(out["dx"], ref["dx"] * keep, extra=ref["dx_extra"] * keep, bf16=False, a=1e-300,
                                      name=f"{what} dx")
    for k in ("gw", "gb"):
        if k in out:
            use[k] = check_elementwise(out[k], ref[k], extra=ref[k + "_extra"], bf16=False, name=f"{what} {k}")
    return use


def old_head_accepts(out, h, w, b, t, scale, old_w, old_b):
    """tests/test_kernels_gpu.py test_head_logsoftmax_nll's tolerances against the fp32 torch head: loss rtol 2e-5 atol
    1e-3, correct equal, dx atol 2e-6 rtol 1e-4, gw / gb atol 2e-5 rtol 1e-4. (That test accumulates into zeros: call
    this with zero old_w / old_b to restate it, as the defect table does for `=` for `+=`.)"""
    r = head_fp32(h, w, b, t, scale, old_w, old_b, form="library")
    ok = lambda a, c, rt, at: bool(((a.double() - c.double()).abs() <= at + rt * c.double().abs()).all())  # noqa: E731
    return (ok(torch.as_tensor(out["loss"]), torch.as_tensor(r["loss"]), 2e-5, 1e-3) and int(out["correct"]) == r["correct"]
            and ok(out["dx"], r["dx"], 1e-4, 2e-6) and ok(out["gw"], r["gw"], 1e-4, 2e-5)
            and ok(out["gb"], r["gb"], 1e-4, 2e-5))


# ------------------------------------------------------------------------------------------------
# u8_wgrad family (mlp_u8.hip): gw[N, 784] += scale sum_m dz[m][n] x[m][k], gb[n] += sum_m dz[m][n]; dz as two fp16 planes
# of dz 2^(14 - E), E from the given bound (or per workgroup from 2 max_row sum_c |dl_c| max |W2|); pixel bytes exact;
# fp32 MFMA sums over 32-row K-steps per split; partial tiles times out_scale = scale 2^(E - 14) as slabs, reduced in a
# fixed order into gw / gb. FD = 0 reads dz, FD = 1 / 2 expand dz = (dl W2) (h > 0 / bits) on fp32 MFMAs first.
U8W_K = 784
U8W_BK = 32  # rows per K-step
U8W_ROWS = [32, 128, 160, 1056, 4096]
U8W_MIN_ROWS_DZ = 4096  # linear_wgrad_u8 (dz given) takes the uint8 kernels from here; the _dl forms from 32 rows


def u8_wgrad_splits(M, N, blocks=0):
    """(splits, rows per split): u8_wgrad_splits / u8_wgrad_group_splits."""
    if blocks:
        s = blocks
    else:
        s = min(max(1, 256 // max(1, N // 64)), max(1, M // (4 * U8W_BK)))
    rps = -(-(-(-M // s)) // U8W_BK) * U8W_BK
    return -(-M // rps), rps


def u8x3_wgrad_passes(dz, x8, third=True):
    """The x3 engine's uint8 weight gradient: pixels one exact plane, dz three bf16 planes (leading term first)."""
    h, m, l = x3_split(dz)
    return [(h.t(), x8.t()), (m.t(), x8.t())] + ([(l.t(), x8.t())] if third else [])


def u8_wgrad_model(dz, x8, old_w, old_b, scale, E, splits, rps, lo=True, reverse=False, drop_kstep=None, bias_every_split=False):
    """fp32 model: dz planes at 2^(14 - E); per split a row-ordered chain of (hi, lo) products, the slab times out_scale
    (one rounding), slabs added in order, then old + sum. The bias partials are chains of the planes' values. Defects:
    lo=False (dz planes without lo), drop_kstep = (split, K-step), bias_every_split (old gb added once per split).
    Returns (gw, gb)."""
    hi, lo_, _, _ = x2_planes(dz, E=E)
    s32 = float(torch.tensor(scale, dtype=torch.float32))
    out_scale = float(torch.tensor(s32 * 2.0 ** (E - 14), dtype=torch.float32))
    passes = [(hi.t(), x8.t())] + ([(lo_.t(), x8.t())] if lo else [])
    M = dz.shape[0]
    gw = gb = None
    order = range(splits - 1, -1, -1) if reverse else range(splits)
    for s in order:
        r0, r1 = s * rps, min(M, (s + 1) * rps)
        drop = ()
        if drop_kstep is not None and drop_kstep[0] == s:
            drop = range(drop_kstep[1] * U8W_BK, (drop_kstep[1] + 1) * U8W_BK)
        acc = chain_model([(a[:, r0:r1], b[:, r0:r1]) for a, b in passes], True, reverse=reverse, drop=drop)
        slab = (acc.double() * out_scale).float()
        ones = torch.ones(1, r1 - r0, device=dz.device)
        bacc = chain_model([(a[:, r0:r1], ones) for a, _ in passes], True, reverse=reverse, drop=drop)[:, 0]
        bslab = (bacc.double() * 2.0 ** (E - 14)).float()
        gw = slab if gw is None else gw + slab
        gb = bslab if gb is None else gb + bslab
        if bias_every_split and s != list(order)[0]:
            gb = gb + old_b.float()
    return old_w.float() + gw, old_b.float() + gb


def u8_wgrad_budget(dz64, x8, old_w, old_b, scale, E, splits, e_dz=None, n_planes=2, rel=X2_REP):
    """References and extras. gw: scale ((n M + 8) u (1 + 2^-5) mag + rel mag + 2^(E - 39) sum_m x + sum_m e_dz x) (the
    planes' products, dz's representation, its floor against the pixel column sums, the error of an expanded dz), the
    partials' out_scale product and their adds into the slab sum or (atomics) into the output, (splits + 2) u
    (scale mag + |old|), and 2 u |old| for the accumulation;
    mag = |dz|^T x. gb the same against ones, without `scale`. n_planes = 3, rel = 0, E = None: the x3 engine's form."""
    s64 = float(torch.tensor(scale, dtype=torch.float32))
    d, x = dz64.double(), x8.double()
    M = d.shape[0]
    floor = 0.0 if E is None else 2.0 ** (E - 39)
    ed = torch.zeros_like(d) if e_dz is None else e_dz.double()
    out = {}
    for name, old, right, sc in (("gw", old_w, x, s64), ("gb", old_b, torch.ones(M, 1, dtype=torch.float64, device=d.device), 1.0)):
        mag = d.abs().t() @ right
        ref = old.double().reshape(mag.shape) + sc * (d.t() @ right)
        extra = sc * (((n_planes * M + 8) * U32 * X3_TERMS + rel) * mag + floor * right.sum(0)[None, :] + ed.t() @ right) \
            + (splits + 2) * U32 * (sc * mag + old.double().reshape(mag.shape).abs()) + 2 * U32 * old.double().reshape(mag.shape).abs()
        out[name], out[name + "_extra"] = ref.reshape(old.shape), extra.reshape(old.shape)
        out[name + "_mag"] = (sc * mag + old.double().reshape(mag.shape).abs()).reshape(old.shape)
    out["M"] = M
    return out


def dz_from_dl(dl, w2, act_pos):
    """(float64 dz, its fp32 chain model, the error bound of the kernels' expansion): dz = (dl W2) [h > 0], C products
    summed in fp32 from zero: (C + 8) u sum_c |dl_c W2_cn|."""
    keep = act_pos.double()
    d64 = (dl.double() @ w2.double()) * keep
    model = chain_model([(dl, w2.t())], True) * act_pos.float()
    e = (dl.shape[1] + 8) * U32 * (dl.double().abs() @ w2.double().abs()) * keep
    return d64, model, e


def old_u8_wgrad_accepts(gw, ref):
    """tests/test_gemm_x3_gpu.py test_linear_wgrad_u8_matches_fp32_reference: |err| <= 2 M 2^-24 (|gz|^T x/255 + |gw0|);
    `ref` from u8_wgrad_budget."""
    return bool(((gw.double() - ref["gw"]).abs() <= 2 * ref["M"] * U32 * ref["gw_mag"] + 1e-30).all())
