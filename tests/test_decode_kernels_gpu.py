"""The generation kernels (attention_decode, linear_decode, sample_logits, embedding_at) against float64 references
with derived budgets (tests/gpt2_decode_numerics.py, docs/NUMERICS.md), and their exactness properties: cache writes,
NaN-proof masking, batch invariance, determinism. Grouped checks print `NUMERICS ...` lines (`pytest -s`)."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no ROCm GPU", allow_module_level=True)

import gpt2_decode_numerics as dn  # noqa: E402
import gpt2_numerics as gn  # noqa: E402
from simple_distributed_machine_learning_amd import _native  # noqa: E402
from simple_distributed_machine_learning_amd.ops import decode as dec  # noqa: E402
from simple_distributed_machine_learning_amd.ops import reference as ref  # noqa: E402

DEV = torch.device("cuda", 0)
K = _native.kernels()
BF = torch.bfloat16
SCALE = 0.125
EPI_STORE, EPI_BIAS, EPI_BIAS_GELU = 0, 1, 5


def rnd(*shape, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.empty(shape).uniform_(-1, 1, generator=g)


def bits(t):
    return t.contiguous().view(torch.int16)


# =====================================================================================================================
# attention_decode
FAMILIES = ["uniform 0.1", "uniform 1.5", "uniform 6", "scores +60"]
LENS = [0, 1, 30, 31, 32, 62, 63, 64, 126, 127, 128, 255, 256, 511, 1022, 1023]


def family_qkv(family, B, S, H, seed):
    u = [rnd(B, S, H, 64, seed=seed + i) for i in range(3)]
    if family.startswith("uniform"):
        amp = float(family.split()[1])
        q, k, v = u[0] * amp, u[1] * amp, u[2] * amp
    else:  # every score is about 64 * 2.75^2 / 8 = 60
        q, k, v = u[0] * 0.5 + 2.75, u[1] * 0.5 + 2.75, u[2] * 1.5
    return q.to(BF), k.to(BF), v.to(BF)


def decode_case(family, seed, B=16, H=3, Smax=1024):
    """The new token's qkv [B, 3C], the caches [B, Smax, H, 64] and lens; cache rows >= lens[b] are left to the caller."""
    _, k, v = family_qkv(family, B, Smax, H, seed)
    qn, kn, vn = family_qkv(family, B, 1, H, seed + 7)
    qkv = torch.cat([t.reshape(B, H * 64) for t in (qn, kn, vn)], 1).contiguous()
    lens = torch.tensor((LENS * ((B + len(LENS) - 1) // len(LENS)))[:B], dtype=torch.int32)
    return qkv, k, v, lens, (qn[:, 0], kn[:, 0], vn[:, 0])


def fill_tail(cache, lens, value):
    c = cache.clone()
    for b, n in enumerate(lens.tolist()):
        c[b, n:] = value
    return c


def run_decode(qkv, kc, vc, lens, n_keys):
    kd, vd = kc.to(DEV), vc.to(DEV)
    out = K.attention_decode(qkv.to(DEV), kd, vd, lens.to(DEV), SCALE, n_keys)
    torch.cuda.synchronize()
    return out.cpu(), kd.cpu(), vd.cpu()


@pytest.fixture(scope="module")
def batch_case():
    """Check 9's launch (family uniform 1.5) with its inputs, shared by the invariance tests."""
    qkv, k, v, lens, new = decode_case("uniform 1.5", seed=11)
    kn, vn = fill_tail(k, lens, math.nan), fill_tail(v, lens, math.nan)
    out, kd, vd = run_decode(qkv, kn, vn, lens, 1024)
    return dict(qkv=qkv, k=kn, v=vn, lens=lens, out=out)


@pytest.mark.parametrize("family", FAMILIES)
def test_attention_decode_budget_and_cache(family):
    B, H, Smax = 16, 3, 1024
    qkv, k, v, lens, (qn, kn, vn) = decode_case(family, seed=11 + 100 * FAMILIES.index(family))
    k_nan, v_nan = fill_tail(k, lens, math.nan), fill_tail(v, lens, math.nan)
    out, kd, vd = run_decode(qkv, k_nan, v_nan, lens, Smax)
    assert bool(torch.isfinite(out.float()).all()), "NaN rows above lens[b] reached the output"
    # cache: row lens[b] holds the new k, v bit for bit, every other row is unchanged
    for b, n in enumerate(lens.tolist()):
        assert torch.equal(bits(kd[b, n]), bits(kn[b])) and torch.equal(bits(vd[b, n]), bits(vn[b])), b
        keep = torch.ones(Smax, dtype=torch.bool)
        keep[n] = False
        assert torch.equal(bits(kd[b][keep]), bits(k_nan[b][keep])), b
        assert torch.equal(bits(vd[b][keep]), bits(v_nan[b][keep])), b
    # the same bits with zeros in place of the NaNs
    out0, _, _ = run_decode(qkv, fill_tail(k, lens, 0.0), fill_tail(v, lens, 0.0), lens, Smax)
    assert torch.equal(bits(out0), bits(out))
    # the numbers
    Kf, Vf = k.clone(), v.clone()
    for b, n in enumerate(lens.tolist()):
        Kf[b, n], Vf[b, n] = kn[b], vn[b]
    r64 = dn.attention_decode_ref64(qn, Kf, Vf, lens, SCALE)
    model = dn.attention_decode_model(qn, Kf, Vf, lens, SCALE)
    row, rms = gn.check_grouped(out.view(B, H, 64), model, r64, name=f"attention_decode {family}")
    print(f"NUMERICS attention_decode {family} | y | row {row:.3f} | rms {rms:.4f}")


@pytest.mark.parametrize("S", [1, 33, 64, 65, 257])
def test_attention_decode_agrees_with_flash(S):
    B, H = 2, 3
    q, k, v = family_qkv("uniform 1.5", B, S, H, seed=31 * S)
    flash, _ = K.attention_fwd(q.to(DEV), k.to(DEV), v.to(DEV), SCALE, True)
    flash = flash.view(B, S, H, 64)[:, S - 1].cpu()
    qkv = torch.cat([t[:, S - 1].reshape(B, H * 64) for t in (q, k, v)], 1).contiguous()
    lens = torch.full((B,), S - 1, dtype=torch.int32)
    kc, vc = k.clone(), v.clone()
    kc[:, S - 1], vc[:, S - 1] = math.nan, math.nan
    out, _, _ = run_decode(qkv, kc, vc, lens, S)
    out = out.view(B, H, 64)
    r64 = gn.attention_ref64(q, k, v, SCALE, True)["y"][:, S - 1]
    m_flash = gn.attention_model(q, k, v, SCALE, True)["y"][:, S - 1]
    m_dec = dn.attention_decode_model(q[:, S - 1], k, v, lens, SCALE)
    gn.check_grouped(flash, m_flash, r64, name=f"flash last row S={S}")
    row, rms = gn.check_grouped(out, m_dec, r64, name=f"decode S={S}")
    print(f"NUMERICS attention_decode vs flash S={S} | y | row {row:.3f} | rms {rms:.4f}")
    eg, base, _, _ = gn.grouped_stats(out, m_flash, r64)  # base: the flash row's own error bound
    assert bool((eg <= gn.ROW_MARGIN * base).all()), (eg / base).max()


def test_attention_decode_batch_invariance_and_determinism(batch_case):
    c = batch_case
    out2, _, _ = run_decode(c["qkv"], c["k"], c["v"], c["lens"], 1024)
    assert torch.equal(bits(out2), bits(c["out"]))
    one, _, _ = run_decode(c["qkv"][5:6], c["k"][5:6], c["v"][5:6], c["lens"][5:6], 1024)
    assert torch.equal(bits(one[0]), bits(c["out"][5]))
    # ... and on a tighter bound of the lengths (fewer chunk blocks launched)
    n5 = int(c["lens"][5]) + 1
    one, _, _ = run_decode(c["qkv"][5:6], c["k"][5:6, :n5], c["v"][5:6, :n5], c["lens"][5:6], n5)
    assert torch.equal(bits(one[0]), bits(c["out"][5]))


def test_attention_decode_refuses_a_full_cache_and_bad_layouts():
    qkv, k, v, lens, _ = decode_case("uniform 1.5", seed=3, B=2, H=3, Smax=64)
    args = (qkv.to(DEV), k.to(DEV), v.to(DEV), lens[:2].to(DEV), SCALE)
    with pytest.raises(RuntimeError, match="cache is full"):
        K.attention_decode(*args, 65)
    with pytest.raises(ValueError, match="cache has 64 rows"):
        dec.attention_decode(*args[:4], 3, 65)
    with pytest.raises(RuntimeError):
        K.attention_decode(args[0], args[1], args[2].transpose(1, 2), args[3], SCALE, 8)


# =====================================================================================================================
# linear_decode
SHAPES = [(2304, 768), (768, 768), (3072, 768), (768, 3072), (16, 64)]
CASES = [(M, N, Kd) for (N, Kd) in SHAPES for M in (1, 15, 16, 17, 64)] + [(16, 50304, 768)]


def linear_inputs(M, N, Kd, seed):
    x = (rnd(M, Kd, seed=seed) * 2.0).to(BF)
    w = (rnd(N, Kd, seed=seed + 1) * 0.08).to(BF)
    b = (rnd(N, seed=seed + 2) * 0.5).to(BF)
    return x, w, b


@pytest.mark.parametrize("M,N,Kd", CASES)
def test_linear_decode_budget(M, N, Kd):
    x, w, b = linear_inputs(M, N, Kd, seed=M + N + Kd)
    xd, wd, bd = x.to(DEV), w.to(DEV), b.to(DEV)
    assert K.linear_decode_supported(M, N, Kd, Kd, Kd)
    y0 = K.linear_decode(xd, wd, None, EPI_STORE)
    y1 = K.linear_decode(xd, wd, bd, EPI_BIAS)
    y2 = K.linear_decode(xd, wd, bd, EPI_BIAS_GELU)
    r0 = gn.check_elementwise(y0.cpu(), dn.linear_ref64(x, w), a=dn.linear_abs_bound(x, w), name="linear_decode")
    r1 = gn.check_elementwise(y1.cpu(), dn.linear_ref64(x, w, b), a=dn.linear_abs_bound(x, w, b),
                              name="linear_decode bias")
    print(f"NUMERICS linear_decode M={M} N={N} K={Kd} | store {r0:.3f} | bias {r1:.3f}")
    assert torch.equal(bits(y2), bits(K.gelu_fwd_bf16(y1)))  # the unfused pair's bits
    assert torch.equal(bits(K.linear_decode(xd, wd, bd, EPI_BIAS_GELU)), bits(y2))  # deterministic
    assert torch.equal(bits(K.linear_decode(xd, wd, None, EPI_STORE)), bits(y0))


@pytest.mark.parametrize("N,Kd", [(2304, 768), (768, 3072), (16, 64)])
def test_linear_decode_identity_returns_rows_of_w(N, Kd):
    """x = 16 unit rows at scattered k with an asymmetric, exactly representable W: y[i] = W[:, k_i] exactly (a
    transposed fragment, a wrong C map or a k permutation applied to one operand only would show)."""
    n, k = torch.arange(N)[:, None], torch.arange(Kd)[None, :]
    w = (((n * 7 + k * 3) % 251) - 125).float()
    ks = [(i * 37 + 5) % Kd for i in range(16)]
    x = torch.zeros(16, Kd)
    for i, kk in enumerate(ks):
        x[i, kk] = 1.0
    y = K.linear_decode(x.to(BF).to(DEV), w.to(BF).to(DEV), None, EPI_STORE).cpu().float()
    assert torch.equal(y, w[:, ks].t().contiguous())


@pytest.mark.parametrize("N,Kd", SHAPES)
def test_linear_decode_rows_do_not_depend_on_m(N, Kd):
    x, w, b = linear_inputs(64, N, Kd, seed=5)
    xd, wd, bd = x.to(DEV), w.to(DEV), b.to(DEV)
    y64 = K.linear_decode(xd, wd, bd, EPI_BIAS)
    y15 = K.linear_decode(xd[:15], wd, bd, EPI_BIAS)
    assert torch.equal(bits(y15), bits(y64[:15]))


def test_linear_decode_refuses_other_shapes():
    for M, N, Kd in [(65, 768, 768), (16, 24, 64), (16, 768, 96), (0, 16, 64)]:
        assert not K.linear_decode_supported(M, N, Kd, Kd, Kd)
        if M:
            with pytest.raises(RuntimeError, match="unsupported shape"):
                K.linear_decode(torch.zeros(M, Kd, dtype=BF, device=DEV), torch.zeros(N, Kd, dtype=BF, device=DEV),
                                None, EPI_STORE)
    with pytest.raises(RuntimeError):  # fp32 operands
        K.linear_decode(torch.zeros(16, 64, device=DEV), torch.zeros(16, 64, device=DEV), None, EPI_STORE)
    # above 64 rows the wrapper runs the big GEMM
    x, w, b = linear_inputs(80, 768, 768, seed=9)
    y = dec.linear_decode(x.to(DEV), w.to(DEV), b.to(DEV))
    gn.check_elementwise(y.cpu(), dn.linear_ref64(x, w, b), a=dn.linear_abs_bound(x, w, b), name="M = 80")


# =====================================================================================================================
# sample_logits
def sampler_logits(B, V, ld, seed):
    g = torch.Generator().manual_seed(seed)
    z = torch.zeros(B, ld)
    z[:, :V] = torch.randn(B, V, generator=g) * 2.0
    return z.to(BF)


@pytest.fixture(scope="module", params=[(64, 50257, 50304), (5, 97, 128)], ids=["gpt2", "tiny"])
def sampler_case(request):
    B, V, ld = request.param
    z = sampler_logits(B, V, ld, seed=V)
    pos = (torch.arange(B, dtype=torch.int32) * 7 + 3) % 1024
    seed, sample0 = 0x1234567890ABCDE, 11
    samples = torch.arange(sample0, sample0 + B)
    return dict(B=B, V=V, z=z, zd=z.to(DEV), pos=pos, posd=pos.to(DEV), seed=seed, sample0=sample0,
                u=ref.sample_uniforms(seed, samples, pos, V))


def test_sample_greedy_matches_twin(sampler_case):
    c = sampler_case
    z = c["z"].clone()
    z[0, :c["V"]] = -z[0, :c["V"]].abs() - 1.0  # all real logits negative: the zero pads must not win
    z[1, 5], z[1, 40] = 30.0, 30.0  # a tie: the lowest index
    got = K.sample_logits(z.to(DEV), c["V"], 0.0, 0, c["seed"], c["sample0"], c["posd"]).cpu()
    want = ref.sample_logits(z, c["V"], 0.0, 0, c["seed"], c["sample0"], c["pos"])
    assert torch.equal(got, want)
    assert int(got[1]) == 5 and int(got[0]) < c["V"]


@pytest.mark.parametrize("T", [0.7, 1.0])
@pytest.mark.parametrize("top_k", [0, 1, 50, 50257])
def test_sample_is_eps_argmax_of_the_float64_scores(sampler_case, T, top_k):
    c = sampler_case
    got = K.sample_logits(c["zd"], c["V"], T, top_k, c["seed"], c["sample0"], c["posd"])
    cand = ref.top_k_candidates(c["z"][:, :c["V"]], top_k)
    worst = dn.check_sampled(got, c["z"], c["V"], T, top_k, c["u"], cand, name=f"T={T} top_k={top_k}")
    print(f"NUMERICS sample_logits V={c['V']} T={T} top_k={top_k} | gap / eps {worst:.3f}")
    if top_k == 1:  # the candidates are the row's maxima (bf16 logits tie): the noise picks among those
        zr = c["z"][:, :c["V"]].float()
        assert torch.equal(zr.gather(1, got.cpu()[:, None])[:, 0], zr.amax(1))
    again = K.sample_logits(c["zd"], c["V"], T, top_k, c["seed"], c["sample0"], c["posd"])
    assert torch.equal(again, got)


def test_sample_top_k_keeps_boundary_ties():
    V, ld = 97, 128
    z = torch.zeros(3, ld)
    z[:, :V] = torch.arange(V).float().flip(0) * 0.25 - 30.0  # strictly decreasing, all negative
    z[1, 3] = z[1, 2]  # rows 1, 2: ties across the k = 3 boundary
    z[2, 2:9] = z[2, 2]
    z = z.to(BF)
    pos = torch.zeros(3, dtype=torch.int32)
    cand = ref.top_k_candidates(z[:, :V], 3)
    assert cand.sum(1).tolist() == [3, 4, 9]
    seen = [set() for _ in range(3)]
    for s in range(64):  # 64 seeds at a high temperature: every candidate of the small sets shows up, nothing else
        got = K.sample_logits(z.to(DEV), V, 50.0, 3, s, 0, pos.to(DEV)).cpu()
        want = ref.sample_logits(z, V, 50.0, 3, s, 0, pos)
        assert torch.equal(got, want)  # (gaps between candidates' scores are far above an ulp here)
        for r in range(3):
            seen[r].add(int(got[r]))
    assert [len(x) for x in seen] == [3, 4, 9]
    assert all(bool(cand[r, list(seen[r])].all()) for r in range(3))


# =====================================================================================================================
# embedding_at
def test_embedding_at_rounds_once():
    V, P, C, B = 97, 64, 128, 37
    wte, wpe = rnd(V, C, seed=1).to(BF), rnd(P, C, seed=2).to(BF)
    tok = torch.randint(0, V, (B,), generator=torch.Generator().manual_seed(3))
    pos = torch.randint(0, P, (B,), generator=torch.Generator().manual_seed(4)).to(torch.int32)
    got = K.embedding_at(tok.to(DEV), pos.to(DEV), wte.to(DEV), wpe.to(DEV)).cpu()
    want = (wte[tok].float() + wpe[pos.long()].float()).to(BF)
    assert torch.equal(bits(got), bits(want))
    assert torch.equal(bits(dec.embedding_at(tok, pos, wte, wpe)), bits(want))  # the twin (bf16 add: one rounding)
