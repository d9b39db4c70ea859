"""References, rounding models and bounds for the generation kernels (attention_decode, linear_decode, sample_logits),
in the scheme of tests/gpt2_numerics.py: float64 references on the kernels' bf16 inputs, an fp32 model that rounds where
the kernel rounds, bounds derived from the arithmetic. Plain torch / Python, runs on the CPU."""
import math

import torch

import gpt2_numerics as gn

CHUNK = 64  # kAttnDecodeChunk: keys per wave of attention_decode
_M32 = 0xFFFFFFFF
_M64 = (1 << 64) - 1


# ------------------------------------------------------------------------------------------------
# the sampler's hash in Python integers, independent of the torch twin
def _splitmix64(x):
    x = (x + 0x9E3779B97F4A7C15) & _M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & _M64
    return x ^ (x >> 31)


def _fmix32(h):
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & _M32
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & _M32
    return h ^ (h >> 16)


def py_uniform(seed, sample, position, v):
    """u of (seed, sample, position, vocabulary id) as a Python float (exact): site 5, layer 0, head 0."""
    skey = _splitmix64((seed & _M64) ^ ((5 << 32) | 0))
    rkey = _splitmix64(skey ^ ((sample << 32) | 0)) >> 32
    word = _fmix32(rkey ^ ((position * 0x9E3779B1) & _M32) ^ ((v * 0x85EBCA77) & _M32))
    return ((word >> 9) + 0.5) * 2.0 ** -23


# ------------------------------------------------------------------------------------------------
# attention_decode: q [B, H, 64]; K, V [B, Smax, H, 64] with the new token's row already at index lens[b]; keys
# 0..lens[b] take part
def _live(lens, Smax):
    return torch.arange(Smax)[None, :] <= lens.long()[:, None]  # [B, Smax]


def attention_decode_ref64(q, K, V, lens, scale):
    live = _live(lens, K.shape[1])
    Kz = torch.where(live[:, :, None, None], K, torch.zeros_like(K)).double()
    Vz = torch.where(live[:, :, None, None], V, torch.zeros_like(V)).double()
    s = torch.einsum("bhd,bshd->bhs", q.double(), Kz) * scale
    p = torch.softmax(s.masked_fill(~live[:, None, :], -math.inf), -1)
    return torch.einsum("bhs,bshd->bhd", p, Vz)


def attention_decode_model(q, K, V, lens, scale, chunk=CHUNK):
    """fp32 model of the kernel: per chunk of 64 keys m_c = max, p = exp2(s c - m_c) (kept fp32), l_c, o_c = p . V;
    the chunks are combined with exp2(m_c - M); y = bf16(O / L), the only rounding to bf16."""
    B, Smax, H, D = K.shape
    live = _live(lens, Smax)
    nC = (Smax + chunk - 1) // chunk
    pad = nC * chunk - Smax
    Kz = torch.where(live[:, :, None, None], K, torch.zeros_like(K)).float()
    Vz = torch.where(live[:, :, None, None], V, torch.zeros_like(V)).float()
    s = torch.einsum("bhd,bshd->bhs", q.float(), Kz) * gn._sl2(scale)
    s = s.masked_fill(~live[:, None, :], -math.inf)
    if pad:
        s = torch.cat([s, torch.full((B, H, pad), -math.inf)], -1)
        Vz = torch.cat([Vz, torch.zeros(B, pad, H, D)], 1)
    sc = s.view(B, H, nC, chunk)
    m = sc.amax(-1)
    p = torch.exp2(sc - torch.where(m == -math.inf, torch.zeros_like(m), m)[..., None])
    l = p.sum(-1)
    o = torch.einsum("bhck,bckhd->bhcd", p, Vz.view(B, nC, chunk, H, D))
    w = torch.exp2(m - m.amax(-1, keepdim=True))
    L = (l * w).sum(-1)
    O = (o * w[..., None]).sum(2)
    return gn.rbf(O / L[..., None])


# ------------------------------------------------------------------------------------------------
# linear_decode
def linear_ref64(x, w, b=None):
    y = x.double() @ w.double().t()
    return y if b is None else y + b.double()


def linear_abs_bound(x, w, b=None):
    """fp32 sums of K exact products (+ the bias) in any order: (K + 1) 2^-24 (sum_k |x_k w_k| + |b|)."""
    K = x.shape[1]
    a = x.double().abs() @ w.double().abs().t()
    if b is not None:
        a = a + b.double().abs()
    return (K + 1) * gn.U32 * a


# ------------------------------------------------------------------------------------------------
# sample_logits
def sample_eps(g64, l_over_t64):
    """Per-token bound on the fp32 score l / T + g: one multiply, one add and two logf of at most 1 ulp each (the inner
    one's relative error becomes an absolute error of the outer), with a factor 2 of slack."""
    return 4.0 * 2.0 ** -23 * (1.0 + g64.abs() + l_over_t64.abs())


def check_sampled(tokens, logits, vocab, temperature, top_k, uniforms, cand, name="sample"):
    """Every row's token must be a candidate and an eps-argmax of the float64 scores built from the twin's uniforms."""
    l = logits[:, :vocab].double() / temperature
    g = -torch.log(-torch.log(uniforms.double()))
    score = torch.where(cand, l + g, torch.full_like(l, -math.inf))
    eps = sample_eps(g, l)
    rows = torch.arange(l.shape[0])
    t = tokens.cpu().long()
    assert bool(((t >= 0) & (t < vocab)).all()), f"{name}: token outside the vocabulary"
    assert bool(cand[rows, t].all()), f"{name}: a token outside the candidate set"
    best = score.argmax(1)
    slack = eps[rows, t] + eps[rows, best]
    bad = ~(score[rows, t] >= score[rows, best] - slack)
    assert not bool(bad.any()), (f"{name}: rows {torch.where(bad)[0].tolist()} are no eps-argmax: "
                                 f"{(score[rows, best] - score[rows, t])[bad].tolist()} over {slack[bad].tolist()}")
    return float(((score[rows, best] - score[rows, t]) / slack).max())
