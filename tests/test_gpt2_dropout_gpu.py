"""GPT-2 dropout on the GPU: the masks the HIP kernels draw are the torch twin's bit for bit; the attention kernels with
dropout and the element-wise sites against float64 with the twin's mask (error budgets from the masked rounding models,
tests/gpt2_dropout_numerics.py); invariance under batch / head splits; p = 0 is today's call bit for bit; and the engine
on the real kernels against the CPU engine with the same masks. Grouped checks print `NUMERICS ...` lines (pytest -s)."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no ROCm GPU", allow_module_level=True)

import gpt2_dropout_numerics as dn  # noqa: E402
import gpt2_numerics as gn  # noqa: E402
from simple_distributed_machine_learning_amd import _native  # noqa: E402
from simple_distributed_machine_learning_amd.data import SyntheticTokens  # noqa: E402
from simple_distributed_machine_learning_amd.models import GPT2Config  # noqa: E402
from simple_distributed_machine_learning_amd.models.gpt2 import gpt2_spec  # noqa: E402
from simple_distributed_machine_learning_amd.ops import reference as R  # noqa: E402
from simple_distributed_machine_learning_amd.ops.transformer import (Drop, add_layer_norm, dropout_add,  # noqa: E402
                                                                     embedding)
from simple_distributed_machine_learning_amd.parallel import PipelineEngine, init_mesh  # noqa: E402

DEV = torch.device("cuda", 0)
K = _native.kernels()
BF = torch.bfloat16
SCALE = 0.125
SITE_LAYER = (R.DROP_SITE_ATTN << 16) | dn.LAYER


def dkw(T, ctr=0, sample0=0, head0=0, site_layer=SITE_LAYER):
    """The bindings' trailing keyword arguments."""
    return dict(drop_t=T, drop_seed=dn.SEED, drop_ctr=torch.tensor([ctr], device=DEV), drop_site_layer=site_layer,
                sample0=sample0, head0=head0)


def grouped(got, model, ref64, family, name, fp32_extra=None):
    row, rms = gn.check_grouped(got.cpu(), model, ref64, name=f"{family} {name}", fp32_extra=fp32_extra)
    print(f"NUMERICS {family} | {name} | row {row:.3f} | rms {rms:.4f}")


def run(q, k, v, dout, causal, **kw):
    qd, kd, vd = (t.contiguous().to(DEV) for t in (q, k, v))
    out, lse = K.attention_fwd(qd, kd, vd, SCALE, causal, **kw)
    res = {"y": out, "lse2": lse.view(q.shape[0], q.shape[2], q.shape[1])}
    if dout is not None:
        dq, dk, dv = (torch.full_like(qd, math.nan) for _ in range(3))
        K.attention_bwd(qd, kd, vd, out, dout.to(DEV).contiguous(), lse, dq, dk, dv, SCALE, causal, **kw)
        res.update(dq=dq, dk=dk, dv=dv)
    torch.cuda.synchronize()
    return {n: t.cpu() for n, t in res.items()}


# =====================================================================================================================
# B1: the kernels' mask is the twin's
@pytest.mark.parametrize("T", [26, 128])
@pytest.mark.parametrize("S", [1, 33, 64, 65, 129, 257])
def test_kernel_masks_are_the_twins(S, T):
    """q = k = 0: every probability of a row is equal and positive. Forward: V = identity on one 64-key block, so the
    non-zero pattern of y is that block's mask. dV: dO one-hot per 64-query block, so dV[k][j] != 0 iff (query
    q0 + j, key k) is kept."""
    B, H = 2, 3
    keep = dn.attn_keep(B, H, S, T, ctr=5, sample0=11, head0=2)
    z = torch.zeros(B, S, H, 64, dtype=BF)
    for causal in (False, True):
        allowed = gn._causal_mask(S, "cpu") if causal else torch.ones(S, S, dtype=torch.bool)
        for b0 in range(0, S, 64):
            n = min(64, S - b0)
            eye = z.clone()
            eye[:, b0:b0 + n] = torch.eye(64, dtype=BF)[:n].view(1, n, 1, 64)
            got = run(z, z, eye, eye, causal, **dkw(T, 5, 11, 2))
            want = (keep & allowed)[..., b0:b0 + n]  # [B, H, q, key in block]
            assert torch.equal((got["y"] != 0)[..., :n].permute(0, 2, 1, 3), want), (S, T, causal, b0, "fwd")
            want_dv = (keep & allowed)[:, :, b0:b0 + n, :]  # [B, H, query in block, k]
            assert torch.equal((got["dv"] != 0)[..., :n].permute(0, 2, 3, 1), want_dv), (S, T, causal, b0, "dv")


# =====================================================================================================================
# B2: numerics
def check_attention_drop(family, B, S, H, causal, T, seed):
    q, k, v, dout = dn.attn_inputs(family, B, S, H, seed)
    keep = dn.attn_keep(B, H, S, T, ctr=2)
    got = run(q, k, v, dout, causal, **dkw(T, 2))
    plain = run(q, k, v, None, causal)
    assert torch.equal(got["lse2"], plain["lse2"])  # LSE is unchanged by dropout, bit for bit
    ref = dn.attention_drop_ref64(q, k, v, SCALE, causal, keep, T, dout)
    model = dn.attention_drop_model_tiled(q, k, v, SCALE, causal, keep, T)
    fam = f"attention dropout T={T} {'causal' if causal else 'full'} {family}"
    grouped(got["y"], model["y"], ref["y"], fam, "y")
    mb = dn.attention_drop_model_bwd(q, k, v, got["y"], got["lse2"], dout, SCALE, causal, keep, T)
    extra = dn.attention_drop_cancellation_bound(q, k, v, got["y"], dout, ref["p"], SCALE, T)
    for name in ("dv", "dk", "dq"):
        grouped(got[name], mb[name], ref[name], fam, name, extra.get(name))
    if causal:  # the first query has one key: y = bf16(v * f) or 0, and a dropped row has zero gradients
        k00 = keep[:, :, 0, 0]
        want = torch.where(k00[..., None], (v[:, 0].float() * dn.f32scale(T)).to(BF).float(), torch.zeros(B, H, 64))
        assert torch.equal(got["y"][:, 0].float(), want)
        assert (got["dq"][:, 0][~k00] == 0).all()
    assert all(torch.isfinite(got[n].float()).all() for n in ("y", "dq", "dk", "dv"))


@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("S", dn.ATTN_S)
def test_attention_dropout_budget(S, causal):
    for i, family in enumerate(dn.ATTN_FAMILIES):
        check_attention_drop(family, 2, S, 3, causal, 26, seed=900 * S + 10 * i)
    check_attention_drop("uniform 1.5", 1, S, 1, causal, 128, seed=900 * S + 77)


# =====================================================================================================================
# B3: invariance and bit-identity
def test_batch_and_head_splits_draw_the_same_masks():
    B, S, H, T = 4, 129, 4, 26
    q, k, v, dout = dn.attn_inputs("uniform 1.5", B, S, H, 31)
    whole = run(q, k, v, dout, True, **dkw(T, 1, 40, 0))
    for lo in (0, 2):
        part = run(q[lo:lo + 2], k[lo:lo + 2], v[lo:lo + 2], dout[lo:lo + 2], True, **dkw(T, 1, 40 + lo, 0))
        for n in ("y", "dq", "dk", "dv"):
            assert torch.equal(part[n], whole[n][lo:lo + 2]), (n, "batch", lo)
        part = run(q[:, :, lo:lo + 2], k[:, :, lo:lo + 2], v[:, :, lo:lo + 2], dout[:, :, lo:lo + 2], True,
                   **dkw(T, 1, 40, lo))
        for n in ("y", "dq", "dk", "dv"):
            assert torch.equal(part[n], whole[n][:, :, lo:lo + 2]), (n, "heads", lo)
    other = run(q, k, v, dout, True, **dkw(T, 2, 40, 0))
    assert not torch.equal(other["y"], whole["y"]) and not torch.equal(other["dv"], whole["dv"])


@pytest.mark.parametrize("causal", [True, False])
def test_p0_is_todays_call_bit_for_bit(causal):
    q, k, v, dout = dn.attn_inputs("growing keys", 2, 257, 3, 9)
    a = run(q, k, v, dout, causal)
    b = run(q, k, v, dout, causal, **dkw(0, 7, 123, 5))
    for n in ("y", "lse2", "dq", "dk", "dv"):
        assert torch.equal(a[n], b[n]), n


# =====================================================================================================================
# B4: element-wise sites
EPS = 1e-5


def site_drop(site, T, ctr=3, sample0=21):
    return Drop(T, dn.SEED, torch.tensor([ctr], device=DEV), site, dn.LAYER, sample0)


@pytest.mark.parametrize("rows", [1, 3, 5])
@pytest.mark.parametrize("C", [8, 64, 768, 1032])
def test_add_layernorm_dropout(C, rows):
    """x: [B = 2, S = rows, C]; xs = bf16(x + M o h f), y = LN(xs); dx = d, dh = bf16(d M f) from the fp32 d."""
    T, B, S = 26, 2, rows
    u = [dn.rnd(B, S, C, seed=100 * C + rows + i) for i in range(4)]
    x, h, gy, gadd = (t.to(BF) for t in (u[0] * 3 + 0.5, u[1] * 2, u[2], u[3]))
    w = (1 + 0.1 * dn.rnd(C, seed=5)).to(BF)
    b = (0.1 * dn.rnd(C, seed=6)).to(BF)
    keep = dn.site_keep(R.DROP_SITE_RESID_ATTN, B, S, C, T, ctr=3, sample0=21)
    skw = dkw(T, 3, 21, site_layer=(R.DROP_SITE_RESID_ATTN << 16) | dn.LAYER)
    skw.pop("head0")
    xd, hd, gyd, gaddd, wd, bd = (t.to(DEV) for t in (x, h, gy, gadd, w, b))
    fam = f"add+LN dropout C={C} rows={rows}"
    # forward: the sum has one rounding (bit for bit the fp32 model, and within the fp32 product + sum of float64);
    # the rest is the checked LayerNorm kernel on xs
    xs, y, mean, rstd = K.add_layernorm_drop_fwd_bf16(xd, hd, wd, bd, EPS, **skw)
    assert torch.equal(xs.cpu().float(), dn.drop_add_model(x, h, keep, T))
    gn.check_elementwise(xs.cpu(), dn.drop_add_ref64(x, h, keep, T), extra=dn.drop_add_fp32_bound(x, h, T),
                         name=f"{fam} xs")
    y3, mean3, rstd3 = K.layernorm_fwd_bf16(xs, wd, bd, EPS)
    assert torch.equal(y, y3) and torch.equal(mean, mean3) and torch.equal(rstd, rstd3)
    xs_c = xs.cpu()
    grouped(y, gn.layernorm_model(xs_c, w, b, EPS)["y"], gn.layernorm_ref64(xs_c, w, b, EPS)["y"], fam, "y")
    # backward: dx, dw, db are the plain fused backward's bits; dh masks and scales the fp32 d, rounded once
    gw0, gb0 = dn.rnd(C, seed=8).to(BF).to(DEV), dn.rnd(C, seed=9).to(BF).to(DEV)
    gw, gb, gw2, gb2 = gw0.clone(), gb0.clone(), gw0.clone(), gb0.clone()
    dx, dh = K.layernorm_bwd_bf16_accum_drop(xs, wd, gyd, mean, rstd, gw, gb, gaddd, **skw)
    dx2 = K.layernorm_bwd_bf16_accum(xs, wd, gyd, mean, rstd, gw2, gb2, gaddd)
    assert torch.equal(dx, dx2) and torch.equal(gw, gw2) and torch.equal(gb, gb2)
    rb, mb = gn.layernorm_bwd_ref64(xs_c, w, gy, EPS, gadd), gn.layernorm_bwd_model(xs_c, w, gy, EPS, gadd)
    grouped(dx, mb["dx"], rb["dx"], fam, "dx")
    st = gn.layernorm_model(xs_c, w, torch.zeros_like(w), EPS)
    d32, _, _ = gn._ln_bwd(xs_c.float(), w.float(), gy.float(), st["mean"], st["rstd"], gadd.float())
    dh_model = gn.rbf(torch.where(keep, d32 * dn.f32scale(T), torch.zeros_like(d32)))
    grouped(dh, dh_model, rb["dx"] * keep * (256.0 / (256 - T)), fam, "dh")
    assert (dh.cpu()[~keep] == 0).all() and torch.isfinite(dh.float()).all()


@pytest.mark.parametrize("rows", [1, 3, 5])
@pytest.mark.parametrize("C", [8, 64, 768, 1032])
def test_dropout_add_and_its_backward(C, rows):
    T, B, S = 128, 2, rows
    x, h, g = (dn.rnd(B, S, C, seed=7 * C + rows + i).mul(2).to(BF) for i in range(3))
    keep = dn.site_keep(R.DROP_SITE_RESID_MLP, B, S, C, T, ctr=3, sample0=21)
    xd, hd = x.to(DEV).requires_grad_(True), h.to(DEV).requires_grad_(True)
    out = dropout_add(xd, hd, site_drop(R.DROP_SITE_RESID_MLP, T))
    out.backward(g.to(DEV))
    torch.cuda.synchronize()
    assert torch.equal(out.cpu().float(), dn.drop_add_model(x, h, keep, T))
    gn.check_elementwise(out.detach().cpu(), dn.drop_add_ref64(x, h, keep, T), extra=dn.drop_add_fp32_bound(x, h, T),
                         name="dropout_add")
    assert torch.equal(xd.grad.cpu(), g)
    assert torch.equal(hd.grad.cpu().float(), dn.drop_scale_model(g, keep, T))
    gn.check_elementwise(hd.grad.cpu(), dn.drop_scale_ref64(g, keep, T), r=2 * gn.U32, name="dropout_add dh")
    # the mask read back exactly: x = 0, h = 1
    ones = torch.ones(B, S, C, dtype=BF, device=DEV)
    m = dropout_add(torch.zeros_like(ones), ones, site_drop(R.DROP_SITE_RESID_MLP, T))
    assert torch.equal(m.cpu() != 0, keep)
    ln = torch.nn.LayerNorm(C).to(DEV).to(BF)
    m2, _ = add_layer_norm(torch.zeros_like(ones), ones, ln, site_drop(R.DROP_SITE_RESID_MLP, T))
    assert torch.equal(m2.cpu() != 0, keep) and torch.equal(m2, m)


def test_embedding_dropout():
    V, C, B, S, T = 97, 32, 3, 19, 26
    wte = dn.rnd(V, C, seed=1).to(BF)
    wpe = dn.rnd(S + 5, C, seed=2).to(BF)
    tok = torch.randint(0, V, (B, S), generator=torch.Generator().manual_seed(3))
    g = dn.rnd(B, S, C, seed=4).to(BF)
    keep = dn.site_keep(R.DROP_SITE_EMBD, B, S, C, T, ctr=3, sample0=21, layer=0)
    drop = Drop(T, dn.SEED, torch.tensor([3], device=DEV), R.DROP_SITE_EMBD, 0, 21)
    wd, pd = wte.to(DEV).requires_grad_(True), wpe.to(DEV).requires_grad_(True)
    out = embedding(tok.to(DEV), wd, pd, drop)
    out.backward(g.to(DEV))
    e32 = wte.float()[tok] + wpe.float()[:S][None]
    assert torch.equal(out.cpu().float(), gn.rbf(torch.where(keep, e32 * dn.f32scale(T), torch.zeros_like(e32))))
    # backward: the masked, scaled g through the plain (deterministic) embedding backward
    gm = dn.drop_scale_model(g, keep, T).to(BF)
    w2, p2 = wte.to(DEV).requires_grad_(True), wpe.to(DEV).requires_grad_(True)
    embedding(tok.to(DEV), w2, p2).backward(gm.to(DEV))
    assert torch.equal(wd.grad, w2.grad) and torch.equal(pd.grad, p2.grad)
    ref = torch.zeros(V, C, dtype=torch.float64).index_add_(0, tok.reshape(-1), gm.double().reshape(-1, C))
    gn.check_elementwise(wd.grad.cpu(), ref, r=B * S * gn.U32, name="wte.grad")


# =====================================================================================================================
# B5: the engine on the real kernels
CFG = dict(n_layer=2, n_head=2, n_embd=128, vocab_size=97, block_size=64)


def _engine(p, dev, M=2, lr=0.05):
    mesh = init_mesh(pp=1, schedule_kind="1f1b", rank=0, world_size=1, device=dev)
    spec = gpt2_spec(2, GPT2Config(dropout=p, **CFG))
    return PipelineEngine(spec, mesh, schedule_kind="1f1b", num_microbatches=M, lr=lr, momentum=0.5, seed=11)


def _train(p, dev, steps=3):
    e = _engine(p, dev)
    ds = SyntheticTokens(4 * steps, 64, 97, seed=5, device=dev)
    losses = [float(e.run(ds, 4 * s, 4, train=True).loss_sum) / (4 * 64) for s in range(steps)]
    return losses, e.flat.params.float().cpu()


def test_engine_gpu_matches_cpu_with_the_same_masks():
    """bf16, B = 4, S = 64, M = 2, 3 steps: the GPU engine (HIP kernels, masks in-kernel) against the CPU engine (masks
    from the torch twin). Yardstick: the same pair of engines at p = 0; the p = 0.1 differences are at most twice those,
    plus 1e-7."""
    diffs = {}
    for p in (0.0, 0.1):
        lg, pg = _train(p, DEV)
        lc, pc = _train(p, torch.device("cpu"))
        diffs[p] = (max(abs(a - b) for a, b in zip(lg, lc)), float((pg - pc).abs().max()))
    print(f"DROPOUT engine gpu-vs-cpu | p=0: loss {diffs[0.0][0]:.3e} params {diffs[0.0][1]:.3e} | "
          f"p=0.1: loss {diffs[0.1][0]:.3e} params {diffs[0.1][1]:.3e}")
    assert diffs[0.1][0] <= 2 * diffs[0.0][0] + 1e-7
    assert diffs[0.1][1] <= 2 * diffs[0.0][1] + 1e-7


def test_graphed_step_draws_fresh_masks_equal_to_eager():
    """lr = 0 and the same batch every step: the losses differ through the masks alone. The captured launch arguments
    (sample0 included) are frozen; the device counter refreshes the masks per replay, as in the eager step."""
    from simple_distributed_machine_learning_amd.parallel.graphs import GraphedStep

    ds = SyntheticTokens(8, 64, 97, seed=5, device=DEV)
    e1, e2 = _engine(0.1, DEV, lr=0.0), _engine(0.1, DEV, lr=0.0)
    g = GraphedStep(e2)
    eager = [float(e1.run(ds, 0, 4, train=True).loss_sum) for _ in range(4)]
    graph = [float(g(ds, 0, 4).loss_sum) for _ in range(4)]
    assert g.replays == 3 and not g.disabled
    assert len(set(graph[1:])) == 3
    assert int(e2.step_ctr) == 4
    for a, b in zip(eager, graph):
        assert a == pytest.approx(b, rel=1e-6)
