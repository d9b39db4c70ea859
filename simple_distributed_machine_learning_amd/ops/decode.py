"""Generation-time ops: the wrappers of the decode kernels (csrc/kernels/attention_decode.hip, attention_append.hip,
attention_extend.hip, attention_fork.hip, attention_decode_fp8.hip, kv_quantize.hip, attention_decode_fp4.hip,
kv_quantize_fp4.hip, linear_decode.hip,
linear_rows.hip, sample.hip, lookup.hip, beam.hip) and their torch twins.

Dispatch: ROCm bf16 tensors (head width 64 for the attention) run the hand-written kernels, and a shape the kernels do
not take is an error there, never a library call. CPU tensors, fp32 and other head widths run the twins below, which
define the semantics. Nothing here builds an autograd graph: generation runs under ``torch.no_grad()``.
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

from .._native import kernels
from . import reference as _ref

EPI_STORE, EPI_BIAS, EPI_BIAS_GELU = 0, 1, 5  # csrc/kernels/kernels.h GemmEpi
LINEAR_DECODE_MAX_M = 64  # kLinearDecodeMaxM
LINEAR_ROWS_MAX_M = 512  # kLinearRowsMaxM
LINEAR_ROWS_DISPATCH_M = 512  # kLinearRowsDispatchM: measured against gemm_bf16 (README.md, "linear_rows")
ATTENTION_APPEND_MAX_T = 8  # kAttnAppendMaxT
ATTENTION_FORK_MAX_N = 64  # kAttnForkMaxN
ATTENTION_DECODE_GQA_GROUPS = (2, 3, 4, 6, 12)  # attention_decode_gqa_supported: n_head / n_kv_head on the kernel
LOOKUP_MAX_DRAFTS, LOOKUP_MAX_NGRAM = 7, 8  # kLookupMaxDrafts, kLookupMaxNgram
BEAM_MAX_K, BEAM_MAX_ROWS, BEAM_MAX_VOCAB = 8, 64, 65536  # kBeamMaxK, kBeamMaxRows, kBeamMaxVocab
BEAM_THREADS = 1024  # beam.hip's threads per logits row


def _hip_bf16(*ts) -> bool:
    return all(t.is_cuda and t.dtype == torch.bfloat16 for t in ts)


def linear_decode_supported(M: int, N: int, K: int, ldx: int = None, ldw: int = None) -> bool:
    """Shapes the weight-streaming kernel takes: 1 <= M <= 64, K % 64 == 0, N % 16 == 0, row strides % 8 == 0."""
    return bool(kernels().linear_decode_supported(M, N, K, K if ldx is None else ldx, K if ldw is None else ldw))


def linear_rows_supported(M: int, N: int, K: int, ldx: int = None, ldw: int = None) -> bool:
    """Shapes linear_rows.hip takes: 64 < M <= 512, else ``linear_decode_supported``'s rules."""
    return bool(kernels().linear_rows_supported(M, N, K, K if ldx is None else ldx, K if ldw is None else ldw))


def linear_decode(x, w, b=None, gelu: bool = False, tickets=None):
    """y [M, N] = x [M, K] w[N, K]^T (+ b) (then tanh-GELU; needs b). ROCm bf16: linear_decode.hip for M <= 64 (W
    streamed once over the whole chip); linear_rows.hip for 64 < M <= ``LINEAR_ROWS_DISPATCH_M`` where
    ``linear_rows_supported`` holds (64-row panels of x in LDS; every row keeps the bits linear_decode.hip gives it,
    so a row's result does not change when the batch crosses 64 rows); gemm_bf16.hip for more rows or another shape;
    anything else: torch.

    ``tickets``: the one-launch form of linear_decode.hip. An int32 tensor on x's device with at least N / 16 entries,
    all zero on entry; the kernel leaves them zero. Where the shape is split over K, the last split to arrive at a
    column tile sums the tile instead of a second launch; the bits are those of the call without tickets. A wrong
    dtype, device or size is a RuntimeError. The torch twins and the M > 64 paths ignore it."""
    if gelu and b is None:
        raise ValueError("linear_decode: the GELU epilogue comes with a bias")
    if _hip_bf16(x, w):
        epi = EPI_BIAS_GELU if gelu else (EPI_BIAS if b is not None else EPI_STORE)
        M = x.shape[0]
        if M <= LINEAR_DECODE_MAX_M:
            if tickets is None:
                return kernels().linear_decode(x, w, b, epi)
            return kernels().linear_decode(x, w, b, epi, tickets)
        if M <= LINEAR_ROWS_DISPATCH_M and x.dim() == 2 and w.dim() == 2 and x.stride(1) == 1 and w.stride(1) == 1 \
                and x.data_ptr() % 16 == 0 and w.data_ptr() % 16 == 0 \
                and kernels().linear_rows_supported(M, w.shape[0], x.shape[1], x.stride(0), w.stride(0)):
            return kernels().linear_rows(x, w, b, epi)
        return kernels().gemm_bf16(x, w, b, False, epi)[0]
    y = F.linear(x, w, b)
    return F.gelu(y, approximate="tanh") if gelu else y


def attention_decode_ref(qkv, k_cache, v_cache, lens, n_head: int, n_keys: int):
    """The twin: write the new k, v at cache row lens[b]; softmax(q K[0..lens[b]]^T / sqrt(D)) V[0..lens[b]] in fp32.
    Rows past lens[b] are selected away (a cache from torch.empty may hold NaN patterns). A grouped cache
    [B, Smax, Hkv, D] with Hkv < n_head: qkv is [B, (n_head + 2 Hkv) D] = (q | k | v) and query head h reads kv head
    h // (n_head // Hkv)."""
    B = qkv.shape[0]
    Hkv = k_cache.shape[2]
    D = qkv.shape[1] // (n_head + 2 * Hkv)
    q, k, v = qkv.split((n_head * D, Hkv * D, Hkv * D), dim=1)
    q, k, v = q.view(B, n_head, D), k.view(B, Hkv, D), v.view(B, Hkv, D)
    idx = lens.to(torch.int64)
    rows = torch.arange(B, device=qkv.device)
    k_cache[rows, idx] = k
    v_cache[rows, idx] = v
    live = torch.arange(n_keys, device=qkv.device)[None, :] <= idx[:, None]  # [B, n_keys]
    kc = torch.where(live[:, :, None, None], k_cache[:, :n_keys], torch.zeros_like(k_cache[:, :n_keys])).float()
    vc = torch.where(live[:, :, None, None], v_cache[:, :n_keys], torch.zeros_like(v_cache[:, :n_keys])).float()
    if Hkv != n_head:  # the head map
        kc, vc = (t.repeat_interleave(n_head // Hkv, 2) for t in (kc, vc))
    C = n_head * D
    s = torch.einsum("bhd,bshd->bhs", q.float(), kc) * (1.0 / math.sqrt(D))
    p = torch.softmax(s.masked_fill(~live[:, None, :], -math.inf), dim=-1)
    return torch.einsum("bhs,bshd->bhd", p, vc).to(qkv.dtype).reshape(B, C)


def attention_decode(qkv, k_cache, v_cache, lens, n_head: int, n_keys: int, tickets=None):
    """One new token per sample against a KV cache. qkv [B, 3C]: the token's fused projection; k_cache / v_cache
    [B, Smax, H, D] (views with any row strides); lens int32 [B] on the device: keys already cached. Writes the new
    k, v to cache row lens[b] and returns the attention output [B, C] over keys 0..lens[b]. ``lens`` is not changed:
    the caller advances it once per step, on the device. ``n_keys`` is the host's bound lens[b] + 1 <= n_keys (the
    caller counts the steps itself, so no length is read back); n_keys <= Smax or a ValueError.

    ``tickets``: the one-launch form of attention_decode.hip. An int32 tensor on qkv's device with at least B * H
    entries, all zero on entry; the kernel leaves them zero. The last live chunk of a (sample, head) to arrive combines
    the chunks instead of a second launch, so the caller may pass ``n_keys = Smax`` (the bound then never changes);
    the bits are those of the call without tickets at any n_keys > max(lens). A wrong dtype, device or size is a
    RuntimeError. The bound n_keys > max(lens) cannot be checked without reading the device: if it is violated, the
    rows concerned are not written and their counters are left non-zero, so zero the tensor before using it again
    (``decode_step`` passes Smax and zeroes its buffer every step). The torch twin ignores it.

    A grouped cache, ``k_cache.shape[2]`` = Hkv < n_head (grouped-query attention; Hkv must divide n_head): qkv is
    [B, (n_head + 2 Hkv) D] = (q | k | v) and query head h reads kv head h // (n_head // Hkv). On the kernels
    (attention_decode_gqa.hip, group sizes ``ATTENTION_DECODE_GQA_GROUPS``) a wave loads a chunk's rows once for the
    group's queries; the output and the cache are, bit for bit, those of this function on the cache and qkv expanded
    to n_head heads. Two launches; ``tickets`` is refused."""
    Smax = k_cache.shape[1]
    if k_cache.dtype == torch.uint8:
        raise ValueError("attention_decode: an fp8 cache goes through attention_decode_fp8, which has no one-launch "
                         "(tickets) form")
    if not 1 <= n_keys <= Smax:
        raise ValueError(f"attention_decode: {n_keys} keys with the new one, but the cache has {Smax} rows")
    D = k_cache.shape[-1]
    if k_cache.dim() == 4 and k_cache.shape[2] < n_head:  # a grouped cache (n_kv_head < n_head)
        Hkv = k_cache.shape[2]
        if tickets is not None:
            raise ValueError("attention_decode: a grouped cache (n_kv_head < n_head) has no one-launch (tickets) form")
        if Hkv < 1 or n_head % Hkv or qkv.shape[-1] != (n_head + 2 * Hkv) * D:
            raise ValueError(f"attention_decode: n_kv_head={Hkv} must divide n_head={n_head} and qkv be "
                             f"[B, (n_head + 2 n_kv_head) D], got {tuple(qkv.shape)} with D={D}")
        if _hip_bf16(qkv, k_cache, v_cache) and D == 64:
            if n_head // Hkv not in ATTENTION_DECODE_GQA_GROUPS:
                raise ValueError(f"attention_decode: n_head / n_kv_head = {n_head // Hkv} is not a group size the "
                                 f"grouped kernel serves ({ATTENTION_DECODE_GQA_GROUPS})")
            return kernels().attention_decode_gqa(qkv, k_cache, v_cache, lens, int(n_head), 1.0 / math.sqrt(D),
                                                  int(n_keys))
        return attention_decode_ref(qkv, k_cache, v_cache, lens, n_head, n_keys)
    if _hip_bf16(qkv, k_cache, v_cache) and D == 64:
        if tickets is not None:
            return kernels().attention_decode(qkv, k_cache, v_cache, lens, 1.0 / math.sqrt(D), int(n_keys), tickets)
        return kernels().attention_decode(qkv, k_cache, v_cache, lens, 1.0 / math.sqrt(D), int(n_keys))
    return attention_decode_ref(qkv, k_cache, v_cache, lens, n_head, n_keys)


# ---- fp8 KV cache (csrc/kernels/kv_fp8.h, kv_quantize.hip, attention_decode_fp8.hip; docs/NUMERICS.md) ---------------
KV_DTYPES = ("bf16", "fp8", "fp4")
KV_EXP_MIN, KV_EXP_MAX = -120, 120  # kv_fp8.h kExpMin, kExpMax


def _pow2(e):
    """2^e as fp32 for an integer tensor e in [-126, 127], from the exponent field: exact on every device."""
    return ((e.to(torch.int32) + 127) << 23).view(torch.float32)


def kv_quantize(x):
    """The fp8 KV-cache format, which the kernels reproduce bit for bit. x [..., D]: rows of D channels. Returns
    (bytes uint8 [..., D], exps int8 [...]): a row is OCP e4m3 bytes and one exponent e, value = e4m3(byte) * 2^e.
    e is the smallest integer with amax * 2^-e <= 448 (amax = f 2^x, f in [1, 2): x - 8 if f <= 1.75, else x - 7),
    clamped to [-120, 120], and 0 for an all-zero row: the scaled row peaks in (224, 448], e4m3's top binade, and never
    overflows. x * 2^-e is exact, so the e4m3 round-to-nearest-even is the only rounding."""
    xf = x.float()
    amax = xf.abs().amax(-1)
    f, ex = torch.frexp(amax)  # amax = f 2^ex with f in [0.5, 1)
    e = ex - 1 - torch.where(f <= 0.875, 8, 7)
    e = torch.where(amax == 0, torch.zeros_like(e), e.clamp(KV_EXP_MIN, KV_EXP_MAX))
    q = (xf * _pow2(-e)[..., None]).to(torch.float8_e4m3fn).view(torch.uint8)
    return q, e.to(torch.int8)


def kv_dequantize(q, e):
    """fp32 [..., D] = e4m3(q) * 2^e for bytes uint8 [..., D] and exponents int8 [...]: exact."""
    return q.view(torch.float8_e4m3fn).float() * _pow2(e)[..., None]


def _check_kv_fp8(who: str, qkv, k8, ke, v8, ve):
    B, Smax, H = k8.shape[:3] if k8.dim() == 4 else (0, 0, 0)
    if k8.dim() != 4 or k8.shape != v8.shape or ke.shape != (B, H, Smax) or ve.shape != ke.shape or \
            k8.dtype != torch.uint8 or v8.dtype != torch.uint8 or ke.dtype != torch.int8 or ve.dtype != torch.int8:
        raise ValueError(f"{who}: an fp8 cache is k8 / v8 uint8 [B, Smax, H, D] with ke / ve int8 [B, H, Smax], got "
                         f"{k8.dtype} {tuple(k8.shape)}, {ke.dtype} {tuple(ke.shape)}, {v8.dtype} {tuple(v8.shape)}, "
                         f"{ve.dtype} {tuple(ve.shape)}")
    if qkv.shape[0] != B or qkv.shape[-1] != 3 * H * k8.shape[3]:
        raise ValueError(f"{who}: qkv {tuple(qkv.shape)} does not match a {tuple(k8.shape)} cache")


def kv_quantize_rows_ref(qkv, k8, ke, v8, ve, S: int):
    """The twin: ``kv_quantize`` of the k and v of positions 0..S-1 of qkv [B, S', 3C] into cache rows 0..S-1."""
    B, _, H, D = k8.shape
    C = H * D
    for o, (q8, ex) in enumerate(((k8, ke), (v8, ve)), 1):
        q, e = kv_quantize(qkv[:, :S, o * C:(o + 1) * C].reshape(B, S, H, D))
        q8[:, :S] = q
        ex[:, :, :S] = e.transpose(1, 2)


def kv_quantize_rows(qkv, k8, ke, v8, ve, S: int):
    """Prefill's write of an fp8 cache: the k and v of positions 0..S-1 of a layer's fused projection qkv [B, S', 3C]
    become the bytes k8 / v8 [B, Smax, H, D] uint8 and exponents ke / ve [B, H, Smax] int8 of rows 0..S-1
    (``kv_quantize`` is the format). ROCm bf16 with D = 64: kv_quantize.hip, one launch for both operands."""
    _check_kv_fp8("kv_quantize_rows", qkv, k8, ke, v8, ve)
    if qkv.dim() != 3 or not 0 <= S <= min(qkv.shape[1], k8.shape[1]):
        raise ValueError(f"kv_quantize_rows: S = {S} positions of qkv {tuple(qkv.shape)} into a cache of "
                         f"{k8.shape[1]} rows")
    if _hip_bf16(qkv) and k8.is_cuda and k8.shape[-1] == 64:
        return kernels().kv_quantize_rows(qkv, k8, ke, v8, ve, int(S))
    return kv_quantize_rows_ref(qkv, k8, ke, v8, ve, int(S))


def attention_decode_fp8_ref(qkv, k8, ke, v8, ve, lens, n_head: int, n_keys: int):
    """The twin: quantise the new k, v (``kv_quantize``) and write bytes and exponents at cache row lens[b]; then
    ``attention_decode_ref``'s lines on the dequantised cache, the new row included as dequantised. Rows at or past
    lens[b] other than the new one are selected away there (they may hold NaN bytes)."""
    B, C3 = qkv.shape
    C = C3 // 3
    D = C // n_head
    idx = lens.to(torch.int64)
    rows = torch.arange(B, device=qkv.device)
    new = [qkv[:, :C].float()]
    for o, (q8, ex) in enumerate(((k8, ke), (v8, ve)), 1):
        q, e = kv_quantize(qkv[:, o * C:(o + 1) * C].view(B, n_head, D))
        q8[rows, idx] = q
        ex[rows, :, idx] = e
        new.append(kv_dequantize(q, e).reshape(B, C))
    kd = kv_dequantize(k8[:, :n_keys], ke[:, :, :n_keys].transpose(1, 2))
    vd = kv_dequantize(v8[:, :n_keys], ve[:, :, :n_keys].transpose(1, 2))
    return attention_decode_ref(torch.cat(new, 1), kd, vd, lens, n_head, n_keys).to(qkv.dtype)


def attention_decode_fp8(qkv, k8, ke, v8, ve, lens, n_head: int, n_keys: int):
    """``attention_decode`` on an fp8 KV cache: k8 / v8 [B, Smax, H, D] uint8 with ke / ve [B, H, Smax] int8
    (``kv_quantize`` is the format; all four contiguous). The new token's k and v are quantised, written to cache row
    lens[b], bytes and exponent, and scored as the dequantised row, so the result is the attention over the cache as
    later steps read it. Returns [B, C]; ``lens`` is not changed; ``n_keys`` as ``attention_decode`` takes it. ROCm
    bf16 with D = 64: attention_decode_fp8.hip and attention_decode.hip's combine, two launches (there is no
    one-launch form: ``attention_decode(..., tickets=)`` refuses an fp8 cache)."""
    _check_kv_fp8("attention_decode_fp8", qkv, k8, ke, v8, ve)
    Smax = k8.shape[1]
    if not 1 <= n_keys <= Smax:
        raise ValueError(f"attention_decode_fp8: {n_keys} keys with the new one, but the cache has {Smax} rows")
    if _hip_bf16(qkv) and k8.is_cuda and k8.shape[-1] == 64:
        return kernels().attention_decode_fp8(qkv, k8, ke, v8, ve, lens, 1.0 / math.sqrt(64), int(n_keys))
    return attention_decode_fp8_ref(qkv, k8, ke, v8, ve, lens, n_head, n_keys)


# ---- fp4 KV cache (csrc/kernels/kv_fp4.h, kv_quantize_fp4.hip, attention_decode_fp4.hip; docs/NUMERICS.md) -----------
KV_FP4_BLOCK = 32  # channels per MX block: 16 bytes of nibbles and one exponent


def kv_fp4_blocks(D: int) -> int:
    """Blocks per row of D channels: D / 32, or one block for an even D that is no multiple of 32 (the twin only)."""
    return D // KV_FP4_BLOCK if D % KV_FP4_BLOCK == 0 else 1
_E2M1 = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)
# (threshold, inclusive): a magnitude's code is the count of thresholds it passes; a tie goes to the even code
_E2M1_TIES = ((0.25, False), (0.75, True), (1.25, False), (1.75, True), (2.5, False), (3.5, True), (5.0, False))


def kv_quantize_fp4(x):
    """The fp4 KV-cache format (OCP microscaling e2m1), which the kernels reproduce bit for bit. x [..., D], D a
    multiple of 32: rows of D / 32 blocks (``kv_fp4_blocks``: a narrower row is one block, for small models on the
    twin). Returns (bytes uint8 [..., D / 2], exps int8 [..., D / 32]). A block is 32 channels: 16 bytes, channel 2 i the low nibble of byte i and channel 2 i + 1 the high one, and one exponent e; the
    value is e2m1(nibble) * 2^e. A nibble is sign, two exponent bits, one mantissa bit: magnitudes {0, 0.5, 1, 1.5, 2,
    3, 4, 6}. e is the smallest integer with amax * 2^-e <= 6 (amax = f 2^x, f in [1, 2): x - 2 if f <= 1.5, else
    x - 1), clamped to [-120, 120], and 0 for an all-zero block: the scaled block peaks in (3, 6] and never saturates.
    x * 2^-e is exact, so the round-to-nearest-even onto the e2m1 grid is the only rounding (ties to the code with
    mantissa bit 0: 0.25 -> 0, 0.75 -> 1, 1.25 -> 1, 1.75 -> 2, 2.5 -> 2, 3.5 -> 4, 5 -> 4); the sign is kept, -0
    included. Finite inputs only: e2m1 has no NaN or Inf, and what a non-finite input becomes is not specified."""
    xf = x.float().unflatten(-1, (kv_fp4_blocks(x.shape[-1]), -1))
    amax = xf.abs().amax(-1)
    f, ex = torch.frexp(amax)  # amax = f 2^ex with f in [0.5, 1)
    e = ex - 1 - torch.where(f <= 0.75, 2, 1)
    e = torch.where(amax == 0, torch.zeros_like(e), e.clamp(KV_EXP_MIN, KV_EXP_MAX))
    y = xf * _pow2(-e)[..., None]
    a = y.abs()
    code = torch.zeros_like(a, dtype=torch.uint8)
    for t, inclusive in _E2M1_TIES:
        code += (a >= t) if inclusive else (a > t)
    code |= torch.signbit(y).to(torch.uint8) << 3
    q = code[..., 0::2] | (code[..., 1::2] << 4)
    return q.flatten(-2), e.to(torch.int8)


def kv_dequantize_fp4(q, e):
    """fp32 [..., D] = e2m1(nibbles of q) * 2^e for bytes uint8 [..., D / 2] and exponents int8 [..., D / 32]: exact."""
    nib = torch.stack((q & 0xF, q >> 4), -1).flatten(-2).to(torch.int64)
    mag = torch.tensor(_E2M1, dtype=torch.float32, device=q.device)[nib & 7]
    val = torch.where((nib & 8) != 0, -mag, mag).unflatten(-1, (e.shape[-1], -1))
    return (val * _pow2(e)[..., None]).flatten(-2)


def _check_kv_fp4(who: str, qkv, k4, ke, v4, ve):
    B, Smax, H = k4.shape[:3] if k4.dim() == 4 else (0, 0, 0)
    nb = kv_fp4_blocks(2 * k4.shape[3]) if k4.dim() == 4 else 0
    if k4.dim() != 4 or k4.shape != v4.shape or ke.shape != (B, H, Smax, nb) or ve.shape != ke.shape or \
            k4.dtype != torch.uint8 or v4.dtype != torch.uint8 or \
            ke.dtype != torch.int8 or ve.dtype != torch.int8:
        raise ValueError(f"{who}: an fp4 cache is k4 / v4 uint8 [B, Smax, H, D / 2] with ke / ve int8 "
                         f"[B, H, Smax, D / 32], got {k4.dtype} {tuple(k4.shape)}, {ke.dtype} {tuple(ke.shape)}, "
                         f"{v4.dtype} {tuple(v4.shape)}, {ve.dtype} {tuple(ve.shape)}")
    if qkv.shape[0] != B or qkv.shape[-1] != 3 * H * 2 * k4.shape[3]:
        raise ValueError(f"{who}: qkv {tuple(qkv.shape)} does not match a {tuple(k4.shape)} cache")


def kv_quantize_rows_fp4_ref(qkv, k4, ke, v4, ve, S: int):
    """The twin: ``kv_quantize_fp4`` of the k and v of positions 0..S-1 of qkv [B, S', 3C] into cache rows 0..S-1."""
    B, _, H, D2 = k4.shape
    C = H * 2 * D2
    for o, (q4, ex) in enumerate(((k4, ke), (v4, ve)), 1):
        q, e = kv_quantize_fp4(qkv[:, :S, o * C:(o + 1) * C].reshape(B, S, H, 2 * D2))
        q4[:, :S] = q
        ex[:, :, :S] = e.transpose(1, 2)


def kv_quantize_rows_fp4(qkv, k4, ke, v4, ve, S: int):
    """Prefill's write of an fp4 cache: the k and v of positions 0..S-1 of a layer's fused projection qkv [B, S', 3C]
    become the nibbles k4 / v4 [B, Smax, H, D / 2] uint8 and block exponents ke / ve [B, H, Smax, D / 32] int8 of rows
    0..S-1 (``kv_quantize_fp4`` is the format). ROCm bf16 with D = 64: kv_quantize_fp4.hip, one launch for both
    operands."""
    _check_kv_fp4("kv_quantize_rows_fp4", qkv, k4, ke, v4, ve)
    if qkv.dim() != 3 or not 0 <= S <= min(qkv.shape[1], k4.shape[1]):
        raise ValueError(f"kv_quantize_rows_fp4: S = {S} positions of qkv {tuple(qkv.shape)} into a cache of "
                         f"{k4.shape[1]} rows")
    if _hip_bf16(qkv) and k4.is_cuda and k4.shape[-1] == 32:
        return kernels().kv_quantize_rows_fp4(qkv, k4, ke, v4, ve, int(S))
    return kv_quantize_rows_fp4_ref(qkv, k4, ke, v4, ve, int(S))


def attention_decode_fp4_ref(qkv, k4, ke, v4, ve, lens, n_head: int, n_keys: int):
    """The twin: quantise the new k, v (``kv_quantize_fp4``) and write nibbles and exponents at cache row lens[b]; then
    ``attention_decode_ref``'s lines on the dequantised cache, the new row included as dequantised. Rows at or past
    lens[b] other than the new one are selected away there."""
    B, C3 = qkv.shape
    C = C3 // 3
    D = C // n_head
    idx = lens.to(torch.int64)
    rows = torch.arange(B, device=qkv.device)
    new = [qkv[:, :C].float()]
    for o, (q4, ex) in enumerate(((k4, ke), (v4, ve)), 1):
        q, e = kv_quantize_fp4(qkv[:, o * C:(o + 1) * C].view(B, n_head, D))
        q4[rows, idx] = q
        ex[rows, :, idx] = e
        new.append(kv_dequantize_fp4(q, e).reshape(B, C))
    kd = kv_dequantize_fp4(k4[:, :n_keys], ke[:, :, :n_keys].transpose(1, 2))
    vd = kv_dequantize_fp4(v4[:, :n_keys], ve[:, :, :n_keys].transpose(1, 2))
    return attention_decode_ref(torch.cat(new, 1), kd, vd, lens, n_head, n_keys).to(qkv.dtype)


def attention_decode_fp4(qkv, k4, ke, v4, ve, lens, n_head: int, n_keys: int, run: int = 0):
    """``attention_decode`` on an fp4 KV cache: k4 / v4 [B, Smax, H, D / 2] uint8 with ke / ve [B, H, Smax, D / 32]
    int8 (``kv_quantize_fp4`` is the format; all four contiguous). The new token's k and v are quantised, written to
    cache row lens[b], nibbles and exponents, and scored as the dequantised row, so the result is the attention over
    the cache as later steps read it. Returns [B, C]; ``lens`` is not changed; ``n_keys`` as ``attention_decode`` takes
    it. ROCm bf16 with D = 64: attention_decode_fp4.hip and attention_decode.hip's combine, two launches, no
    one-launch form. ``run``: the consecutive 64-key chunks one wave of the kernel owns, 1..4, 0: chosen from the
    grid's size; the result's bits do not depend on it (the twin ignores it)."""
    _check_kv_fp4("attention_decode_fp4", qkv, k4, ke, v4, ve)
    Smax = k4.shape[1]
    if not 1 <= n_keys <= Smax:
        raise ValueError(f"attention_decode_fp4: {n_keys} keys with the new one, but the cache has {Smax} rows")
    if not 0 <= run <= 4:
        raise ValueError(f"attention_decode_fp4: run must be 0 or 1..4, got {run}")
    if _hip_bf16(qkv) and k4.is_cuda and k4.shape[-1] == 32:
        return kernels().attention_decode_fp4(qkv, k4, ke, v4, ve, lens, 1.0 / math.sqrt(64), int(n_keys), int(run))
    return attention_decode_fp4_ref(qkv, k4, ke, v4, ve, lens, n_head, n_keys)


def _check_lens_nq(who: str, B: int, lens, nq):
    for name, t in (("lens", lens), ("nq", nq)):
        if t.dtype != torch.int32 or t.shape != (B,):
            raise ValueError(f"{who}: {name} must be int32 [B], got {t.dtype} {tuple(t.shape)}")


def attention_append_ref(qkv, k_cache, v_cache, lens, nq, n_head: int, n_keys: int):
    """The twin: query t of sample b is live iff t < nq[b] and lens[b] + t < n_keys. A live query writes its k, v at
    cache row lens[b] + t and returns softmax(q_t K[0..lens[b]+t]^T / sqrt(D)) V[0..lens[b]+t] in fp32, which is
    ``attention_decode_ref`` for that token with lens[b] + t keys cached; a dead query writes nothing and returns
    zeros. Rows past a query's own are selected away (they may hold NaN patterns)."""
    B, T, C3 = qkv.shape
    C = C3 // 3
    D = C // n_head
    Smax = k_cache.shape[1]
    rows = torch.arange(B, device=qkv.device)
    keys = torch.arange(n_keys, device=qkv.device)[None, :]
    out = torch.zeros((B, T, C), dtype=qkv.dtype, device=qkv.device)
    for t in range(T):
        q, k, v = (qkv[:, t, i * C:(i + 1) * C].view(B, n_head, D) for i in range(3))
        at = lens.to(torch.int64) + t
        alive = (nq.to(torch.int64) > t) & (at < n_keys)  # [B]
        idx = at.clamp(0, Smax - 1)
        sel = alive[:, None, None]
        k_cache[rows, idx] = torch.where(sel, k, k_cache[rows, idx])
        v_cache[rows, idx] = torch.where(sel, v, v_cache[rows, idx])
        live = (keys <= idx[:, None]) & alive[:, None]  # [B, n_keys]
        kc = torch.where(live[:, :, None, None], k_cache[:, :n_keys], torch.zeros_like(k_cache[:, :n_keys])).float()
        vc = torch.where(live[:, :, None, None], v_cache[:, :n_keys], torch.zeros_like(v_cache[:, :n_keys])).float()
        s = torch.einsum("bhd,bshd->bhs", q.float(), kc) * (1.0 / math.sqrt(D))
        s = s.masked_fill(~live[:, None, :], -math.inf).masked_fill(~alive[:, None, None], 0.0)
        o = torch.einsum("bhs,bshd->bhd", torch.softmax(s, dim=-1), vc).to(qkv.dtype).reshape(B, C)
        out[:, t] = torch.where(alive[:, None], o, torch.zeros_like(o))
    return out


def attention_append(qkv, k_cache, v_cache, lens, nq, n_head: int, n_keys: int):
    """T = 1..8 new tokens per sample against a KV cache (attention_append.hip). qkv [B, T, 3C]: the tokens' fused
    projections; the caches and ``lens`` as ``attention_decode`` takes them; ``nq`` int32 [B] on the device: the
    sample's live queries, 0..T. Query t is live iff t < nq[b] and lens[b] + t < n_keys (the host's bound on the rows
    in use, 1 <= n_keys <= Smax or a ValueError): it writes its k, v to cache row lens[b] + t and its output row is,
    bit for bit on the kernels, what ``attention_decode`` returns for that token with lens[b] + t keys cached. A dead
    query writes no cache row and returns zeros. Returns [B, T, C]; ``lens`` is not changed."""
    T = qkv.shape[1] if qkv.dim() == 3 else 0
    if not 1 <= T <= ATTENTION_APPEND_MAX_T:
        raise ValueError(f"attention_append: qkv must be [B, T, 3C] with T in 1..{ATTENTION_APPEND_MAX_T}, got "
                         f"{tuple(qkv.shape)}")
    Smax = k_cache.shape[1]
    if not 1 <= n_keys <= Smax:
        raise ValueError(f"attention_append: n_keys = {n_keys}, but the cache has {Smax} rows")
    _check_lens_nq("attention_append", qkv.shape[0], lens, nq)
    D = k_cache.shape[-1]
    if _hip_bf16(qkv, k_cache, v_cache) and D == 64:
        return kernels().attention_append(qkv, k_cache, v_cache, lens, nq, 1.0 / math.sqrt(D), int(n_keys))
    return attention_append_ref(qkv, k_cache, v_cache, lens, nq, n_head, n_keys)


def attention_extend_ref(qkv, k_cache, v_cache, lens, nq, n_head: int, n_keys: int):
    """The twin of ``attention_extend``: ``attention_append_ref``'s semantics at any T, one masked softmax per sample
    in fp32 over keys 0..n_keys-1. The live positions' k, v go to cache rows lens[b] + t first; position t then sees
    keys 0..lens[b]+t. Rows it does not see are selected away (they may hold NaN patterns); a dead position writes
    nothing and returns zeros."""
    B, T, C3 = qkv.shape
    C = C3 // 3
    D = C // n_head
    Smax = k_cache.shape[1]
    q, k, v = (qkv[..., i * C:(i + 1) * C].view(B, T, n_head, D) for i in range(3))
    at = lens.to(torch.int64)[:, None] + torch.arange(T, device=qkv.device)[None, :]  # [B, T]: absolute positions
    alive = (torch.arange(T, device=qkv.device)[None, :] < nq.to(torch.int64)[:, None]) & (at < n_keys) & \
        (lens.to(torch.int64)[:, None] >= 0)
    idx = at.clamp(0, Smax - 1)
    rows = torch.arange(B, device=qkv.device)[:, None].expand(B, T)
    sel = alive[:, :, None, None]
    k_cache[rows[alive], idx[alive]] = k[alive]
    v_cache[rows[alive], idx[alive]] = v[alive]
    keys = torch.arange(n_keys, device=qkv.device)
    live = (keys[None, None, :] <= idx[:, :, None]) & alive[:, :, None]  # [B, T, n_keys]
    used = live.any(dim=1)[:, :, None, None]  # [B, n_keys, 1, 1]: rows some position of the sample sees
    kc = torch.where(used, k_cache[:, :n_keys], torch.zeros_like(k_cache[:, :n_keys])).float()
    vc = torch.where(used, v_cache[:, :n_keys], torch.zeros_like(v_cache[:, :n_keys])).float()
    s = torch.einsum("bthd,bshd->bhts", q.float(), kc) * (1.0 / math.sqrt(D))
    s = s.masked_fill(~live[:, None], -math.inf).masked_fill(~alive[:, None, :, None], 0.0)
    o = torch.einsum("bhts,bshd->bthd", torch.softmax(s, dim=-1), vc).to(qkv.dtype)
    return torch.where(sel, o, torch.zeros_like(o)).reshape(B, T, C)


def attention_extend(qkv, k_cache, v_cache, lens, nq, n_head: int, n_keys: int):
    """Any T >= 1 new positions per sample against a KV cache plus themselves (attention_extend.hip): chunked prefill
    and a session's catch-up. qkv [B, T, 3C]: the chunk's fused projections, right-padded; the caches, ``lens`` and
    ``nq`` as ``attention_append`` takes them. Position t is live iff t < nq[b] and lens[b] + t < n_keys (the host's
    bound on the rows in use, 1 <= n_keys <= Smax or a ValueError): it writes its k, v to cache row lens[b] + t and
    returns the causal attention over keys 0..lens[b]+t, on the kernels with the bits ``causal_attention`` gives that
    position of the full sequence (docs/NUMERICS.md). A dead position writes no cache row and returns zeros. Returns
    [B, T, C]; ``lens`` is not changed."""
    if qkv.dim() != 3 or qkv.shape[1] < 1 or k_cache.dim() != 4 or k_cache.shape != v_cache.shape or \
            qkv.shape[0] != k_cache.shape[0] or qkv.shape[2] != 3 * k_cache.shape[2] * k_cache.shape[3] or \
            k_cache.shape[2] != n_head:
        raise ValueError(f"attention_extend: qkv must be [B, T >= 1, 3C] against caches [B, Smax, H, D] with C = H D, "
                         f"got {tuple(qkv.shape)}, {tuple(k_cache.shape)}, {tuple(v_cache.shape)}, n_head={n_head}")
    if not (qkv.dtype == k_cache.dtype == v_cache.dtype):
        raise ValueError(f"attention_extend: qkv and the caches must share one dtype, got {qkv.dtype}, "
                         f"{k_cache.dtype}, {v_cache.dtype}")
    Smax = k_cache.shape[1]
    if not 1 <= n_keys <= Smax:
        raise ValueError(f"attention_extend: n_keys = {n_keys}, but the cache has {Smax} rows")
    _check_lens_nq("attention_extend", qkv.shape[0], lens, nq)
    D = k_cache.shape[-1]
    if _hip_bf16(qkv, k_cache, v_cache) and D == 64:
        return kernels().attention_extend(qkv, k_cache, v_cache, lens, nq, 1.0 / math.sqrt(D), int(n_keys))
    return attention_extend_ref(qkv, k_cache, v_cache, lens, nq, n_head, n_keys)


def attention_fork_ref(qkv, kp, vp, plens, ks, vs, lens, n: int, n_head: int, n_keys: int):
    """The twin of ``attention_fork``: materialise each row's cache, the group's ``plens[g]`` prompt rows followed by
    the row's ``lens[r] - plens[g]`` suffix rows, run ``attention_decode_ref`` on it with ``lens[r]`` keys cached, and
    write the new k, v to suffix row ``lens[r] - plens[g]``. Rows the token does not see are zeros in the materialised
    cache (the tails of both caches may hold NaN patterns)."""
    R = qkv.shape[0]
    Pmax, Nmax = kp.shape[1], ks.shape[1]
    C = qkv.shape[1] // 3
    rows = torch.arange(R, device=qkv.device)
    grp = rows // int(n)
    pl, ln = plens.to(torch.int64)[grp], lens.to(torch.int64)
    i = torch.arange(Pmax + Nmax, device=qkv.device)[None, :]  # key index
    from_p, from_s = i < pl[:, None], (i >= pl[:, None]) & (i < ln[:, None])
    ip = i.clamp(max=Pmax - 1).expand(R, -1)
    is_ = (i - pl[:, None]).clamp(0, Nmax - 1)
    caches = []
    for pre, suf in ((kp, ks), (vp, vs)):
        both = torch.where(from_p[:, :, None, None], pre[grp[:, None], ip],
                           torch.where(from_s[:, :, None, None], suf[rows[:, None], is_],
                                       torch.zeros((), dtype=suf.dtype, device=suf.device)))
        caches.append(both)
    out = attention_decode_ref(qkv, caches[0], caches[1], lens, n_head, n_keys)
    ks[rows, ln - pl] = qkv[:, C:2 * C].view(R, n_head, -1)
    vs[rows, ln - pl] = qkv[:, 2 * C:].view(R, n_head, -1)
    return out


def attention_fork(qkv, kp, vp, plens, ks, vs, lens, n: int, n_head: int, n_keys: int):
    """One new token for each of R = G n rows, n continuations per prompt (attention_fork.hip). Row g n + j is sibling
    j of group g. qkv [R, 3C]: the tokens' fused projections; ``kp`` / ``vp`` [G, Pmax, H, D] with ``plens`` int32 [G]
    on the device: the groups' prompt keys, stored once and only read; ``ks`` / ``vs`` [R, Nmax, H, D]: every row's own
    later keys; ``lens`` int32 [R] on the device: ``plens[g]`` plus the row's suffix keys. Key i of row r is
    ``kp[g, i]`` for i < plens[g], ``ks[r, i - plens[g]]`` up to lens[r], and the row's own ``qkv`` at i == lens[r],
    which is written to suffix row lens[r] - plens[g]. Returns [R, C], bit for bit on the kernels what
    ``attention_decode`` returns for that token on a cache holding the prompt rows followed by the suffix rows; the
    kernel loads a 64-key chunk of the prompt once for the n siblings. ``n_keys`` is the host's bound lens[r] + 1 <=
    n_keys <= Pmax + Nmax, or a ValueError; ``lens`` and ``plens`` are not changed."""
    if isinstance(n, bool) or not isinstance(n, int) or not 1 <= n <= ATTENTION_FORK_MAX_N:
        raise ValueError(f"attention_fork: n must be an integer in 1..{ATTENTION_FORK_MAX_N} (samples per group), got "
                         f"{n!r}")
    ts = (qkv, kp, vp, ks, vs)
    if _hip_bf16(*ts) and kp.dim() == 4 and kp.shape[-1] == 64 and kp.shape[2] == n_head:
        # the kernel path: the binding checks every argument (the decode loop calls this once per layer and step, so
        # nothing is checked twice); its refusals name the function and leave here as ValueError, like the twin path's
        try:
            return kernels().attention_fork(qkv, kp, vp, plens, ks, vs, lens, n, 1.0 / math.sqrt(64), int(n_keys))
        except RuntimeError as e:
            if not str(e).startswith("attention_fork:"):
                raise
            raise ValueError(str(e).split("\n")[0]) from None
    if qkv.dim() != 2 or kp.dim() != 4 or ks.dim() != 4 or kp.shape != vp.shape or ks.shape != vs.shape or \
            kp.shape[2:] != ks.shape[2:] or kp.shape[2] != n_head or qkv.shape[1] != 3 * kp.shape[2] * kp.shape[3] or \
            qkv.shape[0] != kp.shape[0] * n or ks.shape[0] != qkv.shape[0] or kp.shape[1] < 1 or ks.shape[1] < 1:
        raise ValueError(f"attention_fork: qkv must be [G n, 3C] against prefix caches [G, Pmax, H, D] and suffix "
                         f"caches [G n, Nmax, H, D] with C = H D, got {tuple(qkv.shape)}, {tuple(kp.shape)}, "
                         f"{tuple(vp.shape)}, {tuple(ks.shape)}, {tuple(vs.shape)}, n={n}, n_head={n_head}")
    if any(t.dtype != qkv.dtype for t in ts) or any(t.device != qkv.device for t in ts + (plens, lens)):
        raise ValueError(f"attention_fork: qkv and the caches must share one dtype, and all tensors one device, got "
                         f"{[str(t.dtype) for t in ts]} on {[str(t.device) for t in ts + (plens, lens)]}")
    if kp.stride() != vp.stride() or ks.stride() != vs.stride():
        raise ValueError("attention_fork: kp / vp and ks / vs must each share one layout, got strides "
                         f"{kp.stride()}, {vp.stride()}, {ks.stride()}, {vs.stride()}")
    G, Pmax, Nmax = kp.shape[0], kp.shape[1], ks.shape[1]
    if not 1 <= n_keys <= Pmax + Nmax:
        raise ValueError(f"attention_fork: n_keys = {n_keys}, but the caches have {Pmax} + {Nmax} rows")
    for name, t, want in (("plens", plens, G), ("lens", lens, G * n)):
        if t.dtype != torch.int32 or t.shape != (want,):
            raise ValueError(f"attention_fork: {name} must be int32 [{want}], got {t.dtype} {tuple(t.shape)}")
    return attention_fork_ref(qkv, kp, vp, plens, ks, vs, lens, n, n_head, n_keys)


def lookup_step(g, tok_in, nq_in, out, lens, limit, done, gen_len, row_steps, k: int, ngram: int, eos: int = -1,
                pad: int = 0):
    """Prompt-lookup speculation's bookkeeping, one launch per verify step: accept the step's drafts against the
    sampler's tokens ``g``, then draft the next step's tokens from the row's own history (ops/reference.py lookup_step
    is the definition). Returns (tok_next [B, k + 1], nq_next [B], all_done [1]). Device tensors: lookup.hip, integer
    work with no host synchronisation; CPU tensors: the twin."""
    if not 1 <= int(k) <= LOOKUP_MAX_DRAFTS:
        raise ValueError(f"lookup_step: k must be in 1..{LOOKUP_MAX_DRAFTS}, got {k}")
    if not 1 <= int(ngram) <= LOOKUP_MAX_NGRAM:
        raise ValueError(f"lookup_step: ngram must be in 1..{LOOKUP_MAX_NGRAM}, got {ngram}")
    if out.is_cuda:
        return tuple(kernels().lookup_step(g, tok_in, nq_in, out, lens, limit, done, gen_len, row_steps, int(k),
                                           int(ngram), int(eos), int(pad)))
    return _ref.lookup_step(g, tok_in, nq_in, out, lens, limit, done, gen_len, row_steps, int(k), int(ngram), int(eos),
                            int(pad))


def _beam_kernel_error(e: RuntimeError, who: str):
    """A binding's refusal (its message names the op) leaves as ValueError, like the twin path's; else re-raise."""
    if not str(e).startswith(who + ":"):
        raise e
    raise ValueError(str(e).split("\n")[0]) from None


def beam_step(logits, vocab: int, K: int, score, fin, glen, eos: int = -1, pad: int = 0, tok_out=None, par_out=None):
    """One step of beam search over R = B K rows (ops/reference.py beam_step is the definition): every live row's K
    best continuations with their cumulative scores, then the K best per prompt. Returns (tok int64, par int32,
    score_new fp32, fin_new int32, glen_new int32, all [R], all_done int32 [1]); the inputs are not changed, so the
    state is double-buffered. ``tok_out`` / ``par_out`` [R]: rows of the caller's histories to write tok / par into.
    ROCm bf16: beam.hip, two launches and no host synchronisation, for 2 <= K <= 8, R <= 64, vocab <= 65536."""
    if isinstance(K, bool) or not isinstance(K, int) or not 2 <= K <= BEAM_MAX_K:
        raise ValueError(f"beam_step: K must be an integer in 2..{BEAM_MAX_K} (beams per prompt), got {K!r}")
    R = logits.shape[0] if logits.dim() == 2 else 0
    if R < K or R % K or not K <= int(vocab) <= logits.shape[1]:
        raise ValueError(f"beam_step: logits must be [B K, ld >= vocab >= K], got {tuple(logits.shape)}, K={K}, "
                         f"vocab={vocab}")
    for name, t, dt in (("score", score, torch.float32), ("fin", fin, torch.int32), ("glen", glen, torch.int32)):
        if t.dtype != dt or t.shape != (R,):
            raise ValueError(f"beam_step: {name} must be {dt} [{R}], got {t.dtype} {tuple(t.shape)}")
    if _hip_bf16(logits):
        try:
            return tuple(kernels().beam_step(logits, int(vocab), K, score, fin, glen, int(eos), int(pad), tok_out,
                                             par_out))
        except RuntimeError as e:
            _beam_kernel_error(e, "beam_step")
    return _ref.beam_step(logits, int(vocab), K, score, fin, glen, int(eos), int(pad), tok_out, par_out)


def beam_gather_kv(buf, half: int, par, K: int, u: int):
    """Re-parent the beams' suffix caches: ``buf`` [2, L, 2, R, nmax, H, D], both halves of the ping-pong for all local
    layers' k and v; positions < u of buf[1 - half][l, kv, r] become those of buf[half][l, kv, (r // K) K + par[r]]
    (``par`` int32 [R] on the device). ROCm bf16: one launch of beam.hip's gather."""
    if buf.dim() != 7 or buf.shape[0] != 2 or buf.shape[2] != 2 or half not in (0, 1) or buf.shape[3] % int(K) or \
            not 0 <= int(u) <= buf.shape[4] or par.dtype != torch.int32 or par.shape != (buf.shape[3],):
        raise ValueError(f"beam_gather_kv: buf must be [2, L, 2, R, nmax, H, D] with R a multiple of K, half 0 or 1, "
                         f"u in 0..nmax and par int32 [R], got {tuple(buf.shape)}, half={half}, K={K}, u={u}, "
                         f"{par.dtype} {tuple(par.shape)}")
    if buf.shape[1] == 0 or int(u) == 0:
        return
    if _hip_bf16(buf):
        try:
            return kernels().beam_gather_kv(buf, int(half), par, int(K), int(u))
        except RuntimeError as e:
            _beam_kernel_error(e, "beam_gather_kv")
    return _ref.beam_gather_kv(buf, int(half), par, int(K), int(u))


def beam_backtrack(out, plen, tok_hist, par_hist, glen, steps: int, K: int, pad: int = 0):
    """Write every row's hypothesis into the token matrix: out[r, plen[r] + t], t < steps, traced back through
    ``tok_hist`` int64 / ``par_hist`` int32 [>= steps, R]; ``pad`` at t >= glen[r]. Device tensors: one launch."""
    if out.is_cuda:
        try:
            return kernels().beam_backtrack(out, plen, tok_hist, par_hist, glen, int(steps), int(K), int(pad))
        except RuntimeError as e:
            _beam_kernel_error(e, "beam_backtrack")
    return _ref.beam_backtrack(out, plen, tok_hist, par_hist, glen, int(steps), int(K), int(pad))


def beam_score_budget(vocab: int, lse: float, score: float, logp: float, threads: int = BEAM_THREADS) -> float:
    """The bound E on |c - exact| of one candidate score c = score + (z - lse) of beam.hip's row pass (and of the fp32
    twin summing in any order no deeper), derived in docs/NUMERICS.md "Beam step": ``lse`` the row's log-sum-exp,
    ``score`` the row's cumulative score, ``logp`` = z - lse, the three as magnitudes of the exact values."""
    u = 2.0 ** -24  # fp32 unit roundoff; a library function good to 2 ulp has a relative error of 4 u
    pieces = (int(vocab) + 7) // 8  # 16-byte pieces of 8 logits, dealt round-robin to the threads
    per_thread = 8 * ((pieces + threads - 1) // threads)  # logits a thread sums
    depth = per_thread + 6 + threads // 64  # adds on the longest path: the thread's, the wave's 6, the wave sums'
    d_sum = (depth + 4 + 2 * math.log(max(int(vocab), 3))) * u  # relative error of S: adds, exp, rounded z - m
    d_lse = d_sum + 4 * u * math.log(max(int(vocab), 3)) + u * abs(lse)  # + the log, + the rounding of m + log S
    return 1.01 * (d_lse + u * abs(logp) + u * (abs(score) + abs(logp)))  # + z - lse, + score + (z - lse)


def embedding_at(tok, pos, wte, wpe):
    """wte[tok[b]] + wpe[pos[b]] -> [B, C] for tok int64 [B] and pos int32 [B] on the device."""
    if _hip_bf16(wte, wpe) and tok.is_cuda and wte.shape[1] % 4 == 0:
        return kernels().embedding_at(tok.contiguous(), pos, wte, wpe)
    return F.embedding(tok, wte) + F.embedding(pos.to(torch.int64), wpe)


def sample_logits(logits, vocab: int, temperature: float, top_k: int, seed: int, sample0: int, positions,
                  rows_per_sample: int = 1):
    """Tokens int64 [B] from logits [B, ld]: greedy at temperature 0, else top-k Gumbel-max keyed by
    (seed, sample0 + row // rows_per_sample, positions[row], token) (ops/reference.py sample_logits is the
    definition). ROCm bf16: the on-device sampler, no host synchronisation."""
    if int(rows_per_sample) < 1:
        raise ValueError(f"sample_logits: rows_per_sample must be >= 1, got {rows_per_sample}")
    if _hip_bf16(logits):
        return kernels().sample_logits(logits, int(vocab), float(temperature), int(top_k), int(seed), int(sample0),
                                       positions, int(rows_per_sample))
    return _ref.sample_logits(logits, vocab, temperature, top_k, seed, sample0, positions, int(rows_per_sample))


def sample_step(logits, vocab: int, temperature: float, top_k: int, top_p: float, seed: int, sample0: int, positions,
                out=None, done=None, gen_len=None, eos: int = -1, pad: int = 0, rows_per_sample: int = 1,
                repetition_penalty: float = 1.0, no_repeat_ngram_size: int = 0, logp=None):
    """sample_logits over the top-p nucleus of the top-k candidates, with one generation step's bookkeeping in the
    same launch (ops/reference.py sample_step is the definition): tokens int64 [B]; ``out`` int64 [B, W] gets the token
    at column positions[row], ``gen_len`` int32 [B] grows by one, ``done`` int32 [B] is set on ``eos`` (-1: none); a
    row already done emits ``pad`` and changes nothing. ``rows_per_sample``: row r is sample sample0 + r //
    rows_per_sample (the verify step of prompt-lookup speculation draws several positions of a sample at once).
    ``repetition_penalty`` theta != 1 and ``no_repeat_ngram_size`` n in 1..8: the token is drawn from
    ``process_logits`` (ops/reference.py) of the row and its history out[row, :positions[row]]; ``logp`` fp32 [B, W]
    gets the raw row's log-probability of the token where ``out`` gets the token. Still one launch (the variant of
    csrc/kernels/sample_penalty.hip, vocab <= 65536 with a penalty or a ban); with the three off it is the call it
    always was. ROCm bf16: the on-device sampler, no host synchronisation."""
    if int(rows_per_sample) < 1:
        raise ValueError(f"sample_step: rows_per_sample must be >= 1, got {rows_per_sample}")
    extra = float(repetition_penalty) != 1.0 or no_repeat_ngram_size != 0 or logp is not None
    if _hip_bf16(logits):
        args = (logits, int(vocab), float(temperature), int(top_k), float(top_p), int(seed), int(sample0), positions,
                out, done, gen_len, int(eos), int(pad), int(rows_per_sample))
        if not extra:
            return kernels().sample_step(*args)
        _ref.check_penalty("sample_step", repetition_penalty, no_repeat_ngram_size)
        try:
            return kernels().sample_step(*args, float(repetition_penalty), int(no_repeat_ngram_size), logp)
        except RuntimeError as e:
            _beam_kernel_error(e, "sample_step")
    if not extra:
        return _ref.sample_step(logits, vocab, temperature, top_k, top_p, seed, sample0, positions, out, done, gen_len,
                                eos, pad, int(rows_per_sample))
    return _ref.sample_step(logits, vocab, temperature, top_k, top_p, seed, sample0, positions, out, done, gen_len,
                            eos, pad, int(rows_per_sample), repetition_penalty, no_repeat_ngram_size, logp)
