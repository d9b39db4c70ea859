"""Grouped-query attention on the kernels: flash output, LSE, dQ and the decode kernel against today's kernels on the
expanded tensors, bit for bit; dK / dV against float64 (docs/NUMERICS.md "Grouped-query attention"; budget use is
printed as `NUMERICS ...` lines, pytest -s); graph replay and batch invariance on a small grouped model."""
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no ROCm GPU", allow_module_level=True)

import gpt2_dropout_numerics as dn  # noqa: E402
import gpt2_numerics as gn  # noqa: E402
from simple_distributed_machine_learning_amd import _native  # noqa: E402
from simple_distributed_machine_learning_amd.models.gpt2 import GPT2Config, gpt2_spec  # noqa: E402
from simple_distributed_machine_learning_amd.ops import reference as R  # noqa: E402
from simple_distributed_machine_learning_amd.ops.decode import attention_decode  # noqa: E402
from simple_distributed_machine_learning_amd.ops.transformer import (Drop, causal_attention, expand_gqa,  # noqa: E402
                                                                     split_gqa)
from simple_distributed_machine_learning_amd.parallel import PipelineEngine, init_mesh  # noqa: E402
from simple_distributed_machine_learning_amd.parallel.generate import generate  # noqa: E402

DEV = torch.device("cuda", 0)
K = _native.kernels()
BF = torch.bfloat16
SCALE = 0.125


def model_dkdv(q, k, v, y, lse2, dout, keep, T, G):
    """gn.attention_model_bwd / dn.attention_drop_model_bwd on the expanded tensors, with each kv head's dK and dV
    summed over its G query heads in fp32 ahead of the one bf16 rounding, as the grouped kernel accumulates them."""
    q, k, v, d = (t.float() for t in (q, k, v, dout))
    f = dn.f32scale(T) if T else 1.0
    p = torch.exp2(gn._scores(q, k) * gn._sl2(SCALE) - lse2[..., None])
    p = p.masked_fill(~gn._causal_mask(p.shape[-1], p.device), 0.0)
    dp = torch.einsum("bqhd,bkhd->bhqk", d, v)
    ds = p * (torch.where(keep, dp * f, torch.zeros_like(dp)) - gn._delta_fp32(dout, y)[..., None])
    dv = torch.einsum("bhqk,bqhd->bkhd", gn.rbf(p * keep), d) * f
    dk = torch.einsum("bhqk,bqhd->bkhd", gn.rbf(ds), q) * SCALE
    return gn.rbf(group_sum(dk, G)), gn.rbf(group_sum(dv, G))


def group_sum(t, G):
    return t.unflatten(2, (-1, G)).sum(3)


@pytest.mark.parametrize("T", [0, 26], ids=["nodrop", "p0.1"])
@pytest.mark.parametrize("S", [64, 192, 200])
@pytest.mark.parametrize("H,Hkv", [(4, 1), (4, 2), (12, 3)])
def test_flash_gqa(H, Hkv, S, T):
    B, G = 2, H // Hkv
    q, _, _, dout = dn.attn_inputs("uniform 1.5", B, S, H, seed=S + H)
    _, k, v, _ = dn.attn_inputs("uniform 1.5", B, S, Hkv, seed=S + H + 7)
    qkv = torch.cat([t.flatten(2) for t in (q, k, v)], -1).to(DEV)
    exp = expand_gqa(qkv, H, Hkv).contiguous()
    kw = {} if T == 0 else dict(drop_t=T, drop_seed=dn.SEED, drop_ctr=torch.tensor([2], device=DEV),
                                drop_site_layer=(R.DROP_SITE_ATTN << 16) | dn.LAYER, sample0=5, head0=0)
    dqkv, dexp = torch.full_like(qkv, torch.nan), torch.full_like(exp, torch.nan)
    dod = dout.to(DEV)
    y, lse = K.attention_fwd(*split_gqa(qkv, H, Hkv), SCALE, True, **kw)
    K.attention_bwd(*split_gqa(qkv, H, Hkv), y, dod, lse, *split_gqa(dqkv, H, Hkv), SCALE, True, **kw)
    ye, lse_e = K.attention_fwd(*split_gqa(exp, H, H), SCALE, True, **kw)
    K.attention_bwd(*split_gqa(exp, H, H), ye, dod, lse_e, *split_gqa(dexp, H, H), SCALE, True, **kw)
    assert torch.equal(y, ye) and torch.equal(lse, lse_e)
    assert torch.equal(split_gqa(dqkv, H, Hkv)[0], split_gqa(dexp, H, H)[0])
    drop = None if T == 0 else Drop(T, dn.SEED, kw["drop_ctr"], R.DROP_SITE_ATTN, dn.LAYER, 5)
    leaf = qkv.clone().requires_grad_(True)
    out = causal_attention(leaf, H, drop, n_kv_head=Hkv)
    out.backward(dod.flatten(2))
    assert torch.equal(out, y.flatten(2)) and torch.equal(leaf.grad, dqkv)
    # dK, dV: float64 MHA gradients summed over the group; the model sums the group in fp32 and rounds once
    ke, ve = (t.repeat_interleave(G, 2) for t in (k, v))
    keep = dn.attn_keep(B, H, S, T, ctr=2, sample0=5) if T else torch.ones(B, H, S, S, dtype=torch.bool)
    ref = dn.attention_drop_ref64(q, ke, ve, SCALE, True, keep, T, dout)
    mk, mv = model_dkdv(q, ke, ve, y.cpu(), lse.view(B, H, S).cpu(), dout, keep, T, G)
    extra = dn.attention_drop_cancellation_bound(q, ke, ve, y.cpu(), dout, ref["p"], SCALE, T)["dk"]
    _, dk, dv = (t.cpu() for t in split_gqa(dqkv, H, Hkv))
    for name, got, model, r64, ex in (("dk", dk, mk, ref["dk"], group_sum(extra, G)), ("dv", dv, mv, ref["dv"], None)):
        row, rms = gn.check_grouped(got, model, group_sum(r64, G), name=f"gqa H={H} Hkv={Hkv} S={S} T={T} {name}",
                                    fp32_extra=ex)
        print(f"NUMERICS gqa H={H} Hkv={Hkv} S={S} T={T} | {name} | row {row:.3f} of {gn.ROW_MARGIN} | rms {rms:.4f} "
              f"of {gn.RMS_MARGIN}")


# lens per sample: the new key lands at 0, 62, 63, 64, 127, 128 and 190 (first key, both sides of the chunk edges, last)
@pytest.mark.parametrize("lens", [(0, 63, 128), (62, 64, 190), (127, 1, 189)], ids=str)
@pytest.mark.parametrize("Hkv", [6, 4, 3, 2, 1])
def test_decode_gqa(Hkv, lens):
    H, B, Smax, G = 12, 3, 192, 12 // Hkv
    g = torch.Generator().manual_seed(Hkv * 1000 + lens[0])
    qkv = torch.empty(B, 64 * (H + 2 * Hkv)).uniform_(-1.5, 1.5, generator=g).to(BF).to(DEV)
    kc, vc = (torch.empty(B, Smax, Hkv, 64).uniform_(-1.5, 1.5, generator=g).to(BF).to(DEV) for _ in range(2))
    lens_d = torch.tensor(lens, dtype=torch.int32, device=DEV)
    dead = torch.arange(Smax, device=DEV)[None, :] >= lens_d[:, None]
    kc[dead], vc[dead] = torch.nan, torch.nan  # NaN bit patterns where nothing is cached
    ke, ve = (t.repeat_interleave(G, 2).contiguous() for t in (kc, vc))
    n_keys = max(lens) + 1
    alone_in = [(kc[b:b + 1].clone(), vc[b:b + 1].clone()) for b in range(B)]
    kc2, vc2 = kc.clone(), vc.clone()
    out = attention_decode(qkv, kc, vc, lens_d, H, n_keys)
    ref = attention_decode(expand_gqa(qkv, H, Hkv).contiguous(), ke, ve, lens_d, H, n_keys)
    assert torch.equal(out, ref) and not out.isnan().any()
    for got, want in ((kc, ke), (vc, ve)):  # the caches after the call, NaN rows included: compare the bits
        assert torch.equal(got.repeat_interleave(G, 2).view(torch.int16), want.view(torch.int16))
    rows = torch.arange(B, device=DEV)
    _, kn, vn = split_gqa(qkv, H, Hkv)
    assert torch.equal(kc[rows, lens_d.long()], kn) and torch.equal(vc[rows, lens_d.long()], vn)
    assert torch.equal(attention_decode(qkv, kc2, vc2, lens_d, H, n_keys), out)  # the same bits again
    assert torch.equal(kc2.view(torch.int16), kc.view(torch.int16))
    for b, (k1, v1) in enumerate(alone_in):  # a sample alone, at its own bound
        assert torch.equal(attention_decode(qkv[b:b + 1], k1, v1, lens_d[b:b + 1], H, lens[b] + 1), out[b:b + 1])


@pytest.fixture(scope="module")
def engine():
    cfg = GPT2Config(n_layer=2, n_head=4, n_embd=256, vocab_size=512, block_size=192, n_kv_head=1)
    mesh = init_mesh(pp=1, schedule_kind="1f1b", rank=0, world_size=1, device=DEV)
    e = PipelineEngine(gpt2_spec(2, cfg=cfg, seq_len=64, dtype=BF, name="gpt2_gqa"), mesh, schedule_kind="1f1b",
                       num_microbatches=1, seed=3)
    e.eval()
    return e


def test_generate_graph_and_batch_invariance(engine):
    prompts = torch.randint(0, 512, (3, 60), generator=torch.Generator().manual_seed(1))
    kw = dict(temperature=0.9, top_k=20, seed=7)
    eager = generate(engine, prompts, 80, **kw)  # positions 60..139: across the 64- and 128-key chunk edges
    assert torch.equal(generate(engine, prompts, 80, graph=True, **kw), eager)
    for b in range(3):
        assert torch.equal(generate(engine, prompts[b:b + 1], 80, sample0=b, **kw)[0], eager[b])
