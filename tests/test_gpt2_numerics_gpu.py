"""The GPT-2 kernels (attention, vocabulary cross-entropy, LayerNorm, column sums) against float64 references with
error budgets from rounding models (tests/gpt2_numerics.py, docs/NUMERICS.md), at the sizes where the kernels change
path. Each grouped check prints its budget use (`NUMERICS ...` lines, shown by `pytest -s`)."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no ROCm GPU", allow_module_level=True)

import gpt2_numerics as gn  # noqa: E402
from simple_distributed_machine_learning_amd import _native  # noqa: E402
from simple_distributed_machine_learning_amd.ops.transformer import (add_layer_norm, causal_attention,  # noqa: E402
                                                                     cross_entropy_sum, layer_norm, layer_norm_pass)

DEV = torch.device("cuda", 0)
K = _native.kernels()
BF = torch.bfloat16
SCALE = 0.125  # 1 / sqrt(64)
INF = math.inf


def rnd(*shape, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.empty(shape).uniform_(-1, 1, generator=g)


def grouped(got, model, ref64, family, name, fp32_extra=None):
    row, rms = gn.check_grouped(got.cpu(), model, ref64, name=f"{family} {name}", fp32_extra=fp32_extra)
    print(f"NUMERICS {family} | {name} | row {row:.3f} | rms {rms:.4f}")


# =====================================================================================================================
# attention
ATTN_S = [1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 257]
ATTN_FAMILIES = ["uniform 0.1", "uniform 1.5", "uniform 6", "scores +60", "growing keys"]


def attn_inputs(family, B, S, H, seed):
    """q, k, v, dout [B, S, H, 64] bf16 on the CPU."""
    u = [rnd(B, S, H, 64, seed=seed + i) for i in range(4)]
    if family.startswith("uniform"):
        amp = float(family.split()[1])
        q, k, v = u[0] * amp, u[1] * amp, u[2] * amp
    elif family == "scores +60":  # a common component of q and k: every score is about 64 * 2.75^2 / 8 = 60
        q, k, v = u[0] * 0.5 + 2.75, u[1] * 0.5 + 2.75, u[2] * 1.5
    else:  # key norms grow along S: the running maximum moves at every tile
        grow = 0.5 + 4.0 * torch.arange(S).float().view(1, S, 1, 1) / max(S - 1, 1)
        q, k, v = u[0] * 1.5, u[1] * grow, u[2] * 1.5
    return q.to(BF), k.to(BF), v.to(BF), u[3].to(BF)


def fuse(q, k, v):
    B, S, H, _ = q.shape
    return torch.cat([t.reshape(B, S, H * 64) for t in (q, k, v)], -1).contiguous()


def split_views(qkv, H):
    B, S, C3 = qkv.shape
    C = C3 // 3
    return tuple(qkv[..., i * C:(i + 1) * C].view(B, S, H, 64) for i in range(3))


def run_attention(mode, q, k, v, dout):
    """Runs the kernels; returns y, dq, dk, dv [B, S, H, 64] and the kernel's log2-domain lse [B, H, S], on the CPU.
    mode: 'fused' = causal_attention on a fused qkv; 'views' = the bindings on slices of a fused qkv, non-causal;
    'separate' / 'separate-nc' = the bindings on three contiguous tensors, causal / non-causal."""
    B, S, H, _ = q.shape
    causal = mode in ("fused", "separate")
    if mode == "fused":
        qkv = fuse(q, k, v).to(DEV).requires_grad_(True)
        y = causal_attention(qkv, H)
        y.backward(dout.reshape(B, S, H * 64).to(DEV))
        out, lse = K.attention_fwd(*split_views(qkv.detach(), H), SCALE, True)
        assert torch.equal(out.view(B, S, H * 64), y)
        dq, dk, dv = split_views(qkv.grad, H)
    else:
        if mode == "views":
            qd, kd, vd = split_views(fuse(q, k, v).to(DEV), H)
            dq, dk, dv = split_views(torch.full((B, S, 3 * H * 64), math.nan, dtype=BF, device=DEV), H)
        else:
            qd, kd, vd = (t.contiguous().to(DEV) for t in (q, k, v))
            dq, dk, dv = (torch.full_like(qd, math.nan) for _ in range(3))
        out, lse = K.attention_fwd(qd, kd, vd, SCALE, causal)
        K.attention_bwd(qd, kd, vd, out, dout.to(DEV).contiguous(), lse, dq, dk, dv, SCALE, causal)
    torch.cuda.synchronize()
    return {"y": out.view(B, S, H, 64).cpu(), "lse2": lse.view(B, H, S).cpu(), "dq": dq.cpu(), "dk": dk.cpu(),
            "dv": dv.cpu(), "causal": causal}


def check_attention(mode, family, B, S, H, seed):
    q, k, v, dout = attn_inputs(family, B, S, H, seed)
    got = run_attention(mode, q, k, v, dout)
    causal = got["causal"]
    ref = gn.attention_ref64(q, k, v, SCALE, causal, dout)
    model = gn.attention_model(q, k, v, SCALE, causal)
    fam = f"attention {mode} {family}"
    grouped(got["y"], model["y"], ref["y"], fam, "y")
    gn.check_elementwise(got["lse2"].double() * gn.LN2, ref["lse"], extra=gn.lse_bound(ref["lse"], S), bf16=False,
                         name=f"{fam} lse")
    # the backward model reads the y and lse the backward kernels were given
    mb = gn.attention_model_bwd(q, k, v, got["y"], got["lse2"], dout, SCALE, causal)
    extra = gn.attention_cancellation_bound(q, k, v, got["y"], dout, ref["p"], SCALE)
    for name in ("dv", "dk", "dq"):
        grouped(got[name], mb[name], ref[name], fam, name, extra.get(name))
    if causal:
        assert torch.equal(got["y"][:, 0], v[:, 0])  # the first query sees one key: y = v, bit for bit


@pytest.mark.parametrize("mode", ["fused", "views", "separate", "separate-nc"])
@pytest.mark.parametrize("S", ATTN_S)
def test_attention_budget(S, mode):
    for i, family in enumerate(ATTN_FAMILIES):
        check_attention(mode, family, 1, S, 1, seed=1000 * S + 10 * i)


@pytest.mark.parametrize("mode", ["fused", "views", "separate", "separate-nc"])
@pytest.mark.parametrize("B,S,H", [(1, 129, 3), (3, 129, 3), (1, 257, 3), (3, 257, 3)])
def test_attention_budget_batch_and_heads(B, S, H, mode):
    """Grids of 6 and 27 workgroups (no multiple of 8: the plain block order) and the b / h indexing."""
    for i, family in enumerate(("uniform 1.5", "growing keys")):
        check_attention(mode, family, B, S, H, seed=77 * S + B + 10 * i)


@pytest.mark.parametrize("S", [33, 129, 257])
def test_attention_causal_prefix_is_independent_of_later_positions(S):
    """Changing q, k, v after position p leaves y[:, :p + 1] bit-identical."""
    B, H = 2, 3
    q, k, v, _ = attn_inputs("uniform 1.5", B, S, H, seed=5)
    q2, k2, v2, _ = attn_inputs("uniform 6", B, S, H, seed=6)
    y0 = causal_attention(fuse(q, k, v).to(DEV), H).cpu()
    for p in sorted({0, 30, 31, 32, 63, 64, 127, 128, 200} & set(range(S - 1))):
        a, b, c = q.clone(), k.clone(), v.clone()
        a[:, p + 1:], b[:, p + 1:], c[:, p + 1:] = q2[:, p + 1:], k2[:, p + 1:], v2[:, p + 1:]
        y1 = causal_attention(fuse(a, b, c).to(DEV), H).cpu()
        assert torch.equal(y1[:, :p + 1], y0[:, :p + 1]), p
        assert not torch.equal(y1[:, p + 1:], y0[:, p + 1:])


@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("B,S", [(1, 129), (3, 257)])
def test_attention_head_permutation_permutes_outputs(B, S, causal):
    H, perm = 3, [2, 0, 1]
    q, k, v, dout = attn_inputs("uniform 1.5", B, S, H, seed=9)
    mode = "separate" if causal else "views"
    a = run_attention(mode, q, k, v, dout)
    b = run_attention(mode, q[:, :, perm], k[:, :, perm], v[:, :, perm], dout[:, :, perm])
    for name in ("y", "dq", "dk", "dv"):
        assert torch.equal(a[name][:, :, perm], b[name]), name
    assert torch.equal(a["lse2"][:, perm], b["lse2"])


@pytest.mark.parametrize("mode", ["fused", "views"])
def test_attention_knob_variants_bit_identical(mode):
    """Two query sub-blocks per wave (ATTN_FWD_QS 2 and 3) and two key tiles per wave (ATTN_DKDV_KT 2) write the
    default kernels' bits at every sequence length around the wave, tile and workgroup sizes."""
    B, H = 2, 2
    for S in ATTN_S:
        q, k, v, dout = attn_inputs("uniform 1.5", B, S, H, seed=S)
        base = run_attention(mode, q, k, v, dout)
        try:
            for knob, val in (("ATTN_FWD_QS", 2), ("ATTN_FWD_QS", 3), ("ATTN_DKDV_KT", 2)):
                K.reset_knobs()
                K.set_knob(knob, val)
                other = run_attention(mode, q, k, v, dout)
                for name in ("y", "lse2", "dq", "dk", "dv"):
                    assert torch.equal(base[name], other[name]), (S, knob, val, name)
        finally:
            K.reset_knobs()


# =====================================================================================================================
# vocabulary cross-entropy
CE_V = [1, 7, 8, 9, 97, 16384, 16385, 32768, 32769, 53248, 53249, 65536, 65537, 65543, 65544]


def check_cross_entropy(z, t, scale, ignore_index=-100, name="ce"):
    """z [rows, V] bf16 (possibly a padded-row view) and t on the CPU; runs the binding and the wrapper, checks both
    against float64 and returns the binding's dlogits (device)."""
    zd, td = z.to(DEV) if not z.is_cuda else z, t.to(DEV)
    zc = zd.cpu()
    ref = gn.cross_entropy_ref64(zc, t, scale, ignore_index)
    loss, ok, g = K.cross_entropy_bf16(zd, td, scale, ignore_index, True)
    loss_e, ok_e, g_e = K.cross_entropy_bf16(zd, td, scale, ignore_index, False)
    lsum, csum, count, g2 = cross_entropy_sum(zd, td, scale, True, ignore_index)
    torch.cuda.synchronize()
    gn.check_dlogits(g.cpu(), ref["dlogits"], scale, name=f"{name} dlogits")
    bound = gn.loss_bound(ref)
    gn.check_elementwise(loss.cpu(), ref["loss"], extra=bound, bf16=False, name=f"{name} loss")
    assert torch.equal(ok.cpu().double(), ref["correct"]), f"{name} correct"
    assert g_e is None and torch.equal(loss_e, loss) and torch.equal(ok_e, ok)  # evaluation mode: the same rows
    assert torch.equal(g2, g)
    rows = z.shape[0]
    gn.check_elementwise(lsum.cpu(), ref["loss"].sum(), extra=bound.sum() + rows * gn.U32 * ref["loss"].abs().sum(),
                         bf16=False, name=f"{name} loss sum")
    assert float(csum) == float(ref["correct"].sum()) and count == ref["count"], f"{name} correct / count"
    valid = (t != ignore_index) & (t >= 0) & (t < z.shape[1])
    gi = g.cpu()[~valid]
    assert (gi == 0).all() and (loss.cpu()[~valid] == 0).all() and (ok.cpu()[~valid] == 0).all(), f"{name} ignored rows"
    return g


def ce_targets(rows, V, seed):
    return torch.randint(0, V, (rows,), generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize("rows", [1, 3])
@pytest.mark.parametrize("V", CE_V)
def test_cross_entropy_budget(V, rows):
    """Contiguous rows: with an odd V the odd rows start misaligned (head / tail element paths of the register
    kernel, the scalar path of the online kernel)."""
    u = rnd(rows, V, seed=V + rows)
    t = ce_targets(rows, V, V)
    shift = torch.tensor([80.0, -80.0, 0.0])[:rows, None]
    dominant = u.clone()
    dominant[torch.arange(rows), ce_targets(rows, V, V + 1)] = 30.0
    for fam, z, scale in (("x4", u * 4, 0.5), ("shifted", u * 4 + shift, 1.0 / 64), ("dominant", dominant, 1.0),
                          ("dominant target", dominant, 2.0)):
        tt = dominant.argmax(1) if fam == "dominant target" else t
        check_cross_entropy(z.to(BF), tt, scale, name=f"V={V} {fam}")


@pytest.mark.parametrize("V", [9, 97, 16385, 53249, 65543, 65544])
def test_cross_entropy_target_and_maximum_placement(V):
    """Targets and maxima at the first and last element and inside the unaligned head and tail of a row; ties for the
    maximum across head / vectors / tail and across threads resolve to the first index (torch.argmax)."""
    pos = sorted({p for p in (0, 1, 5, 7, 8, V // 2, V - 9, V - 8, V - 3, V - 2, V - 1) if 0 <= p < V})
    ties = [(0, V - 1), (3, V // 2, V - 2), (V - 2, V - 1), (1, 2), (6, 8 * 600 + 3, 8 * 5000 + 1, V - 4)]
    ties = [tuple(sorted({p for p in tie if 0 <= p < V})) for tie in ties]
    rows = 2 * len(pos) + 2 * len(ties)
    z = rnd(rows, V, seed=V) * 4
    t = ce_targets(rows, V, V + 3)
    r = 0
    for p in pos:  # a target at p; a maximum at p that is the target
        t[r] = p
        z[r + 1, p] = 9.0
        t[r + 1] = p
        r += 2
    for tie in ties:  # the maximum at all of tie: the first index is the argmax
        z[r, list(tie)] = 9.0
        t[r] = tie[0]
        z[r + 1, list(tie)] = 9.0
        t[r + 1] = tie[-1]
        r += 2
    zc = z.to(BF)
    check_cross_entropy(zc, t, 0.25, name=f"V={V} placement")
    ref = gn.cross_entropy_ref64(zc, t, 0.25)
    n_single = sum(1 for tie in ties if len(tie) == 1)
    assert ref["correct"][2 * len(pos):].sum() == len(ties) + n_single  # the tie rows really tell first from last


@pytest.mark.parametrize("V", [9, 97, 16385, 65536, 65543, 65544])
def test_cross_entropy_minus_infinity_logits(V):
    """Rows with -inf logits (masked vocabulary entries): they add 0 to the sum and get a zero gradient. In the online
    kernel (V > 65536) a thread, and a whole wave, may see nothing but -inf before its first finite logit."""
    idx = torch.arange(V)
    masks = [idx < 8, rnd(V, seed=1) < -0.8, (idx // 8) % 256 == 5, ((idx // 8) % 256) // 64 == 2, idx % 256 == 0,
             (idx > 0) & (idx < V - 1)]
    rows = len(masks)
    z = rnd(rows, V, seed=V + 11) * 4
    t = ce_targets(rows, V, V + 5)
    for r, m in enumerate(masks):
        if m.all():
            m = m.clone()
            m[V // 2] = False
        z[r, m] = -INF
        finite = torch.where(~m)[0]
        t[r] = finite[int(t[r]) % len(finite)]
    g = check_cross_entropy(z.to(BF), t, 0.5, name=f"V={V} -inf")
    assert torch.isfinite(g.float()).all()


@pytest.mark.parametrize("rows,V,ld", [(7, 97, 128), (1, 97, 128), (4, 50257, 50304)])
def test_cross_entropy_padded_rows(rows, V, ld):
    """Padded rows (ld > V, the lm_head's layout): the logits' pad columns are never read (NaN there) and the
    gradient's pad columns are written as exact zeros."""
    buf = torch.full((rows, ld), math.nan, dtype=BF)
    buf[:, :V] = (rnd(rows, V, seed=V + rows) * 4).to(BF)
    zd = buf.to(DEV)[:, :V]
    t = ce_targets(rows, V, 3)
    t[0], t[-1] = V - 1, 0
    g = check_cross_entropy(zd, t, 0.5, name=f"V={V} ld={ld}")
    if rows > 1:
        assert g.stride(0) == ld
        full = torch.as_strided(g, (rows, ld), (ld, 1))
        assert (full[:, V:] == 0).all() and torch.isfinite(full.float()).all()


@pytest.mark.parametrize("V", [8, 97, 50257, 65544])
def test_cross_entropy_ignore_index(V):
    rows = 5
    z = (rnd(rows, V, seed=V + 2) * 4).to(BF)
    t = ce_targets(rows, V, V + 1)
    some = t.clone()
    some[1], some[3] = -100, -100
    check_cross_entropy(z, some, 0.5, -100, name=f"V={V} some ignored")
    _, _, n, _ = cross_entropy_sum(z.to(DEV), some.to(DEV), 0.5, True)
    assert n == 3
    check_cross_entropy(z, torch.full((rows,), -100), 0.5, -100, name=f"V={V} all ignored")
    for ii in (0, V - 1):
        tt = t.clone()
        tt[0], tt[2] = ii, ii
        tt[4] = (ii + 1) % V
        check_cross_entropy(z, tt, 0.5, ii, name=f"V={V} ignore_index={ii}")
    # ignore_index=None: nothing is ignored and nothing is counted on the host
    l0, c0, n0, g0 = cross_entropy_sum(z.to(DEV), t.to(DEV), 0.5, True, None)
    l1, c1, n1, g1 = cross_entropy_sum(z.to(DEV), t.to(DEV), 0.5, True, -100)
    assert n0 == n1 == rows and torch.equal(g0, g1) and torch.equal(l0, l1) and torch.equal(c0, c1)


# =====================================================================================================================
# LayerNorm
LN_D = [8, 64, 504, 512, 520, 1024, 1032, 2048, 2056, 4096]
EPS = 1e-5


def ln_inputs(family, rows, D, seed):
    u = [rnd(rows, D, seed=seed + i) for i in range(4)]
    if family == "uniform":
        x = u[0] * 3 + 0.5
    elif family == "offset":  # mean much larger than spread, bf16-exact values 64, 64.5, ..., 67.5
        x = 64 + torch.floor((u[0] + 1) * 4).clamp(0, 7) / 2
    else:  # constant rows (var = 0)
        x = ((torch.arange(rows).float() % 7) - 1.5).view(rows, 1).expand(rows, D)
    w = 1 + 0.1 * rnd(D, seed=seed + 5)
    b = 0.1 * rnd(D, seed=seed + 6)
    return [t.contiguous().to(BF) for t in (x, u[1], u[2], u[3], w, b)]  # x, gy, gadd, h, w, b


def check_layernorm(family, rows, D, seed):
    x, gy, gadd, h, w, b = ln_inputs(family, rows, D, seed)
    xd, gyd, gaddd, hd, wd, bd = (t.to(DEV) for t in (x, gy, gadd, h, w, b))
    fam = f"layernorm {family}"
    # forward
    y, mean, rstd = K.layernorm_fwd_bf16(xd, wd, bd, EPS)
    ref, model = gn.layernorm_ref64(x, w, b, EPS), gn.layernorm_model(x, w, b, EPS)
    bounds = gn.layernorm_fp32_bounds(x, w, gy, EPS)
    grouped(y, model["y"], ref["y"], fam, "y")
    gn.check_elementwise(mean.cpu(), ref["mean"], extra=bounds["mean"], bf16=False, name=f"{fam} mean")
    gn.check_elementwise(rstd.cpu(), ref["rstd"], extra=bounds["rstd"], bf16=False, name=f"{fam} rstd")
    if family == "constant":
        assert torch.equal(y, bd.expand(rows, D))
    # backward, fp32 dw / db
    dx, dw, db = K.layernorm_bwd_bf16(xd, wd, gyd, mean, rstd)
    rb, mb = gn.layernorm_bwd_ref64(x, w, gy, EPS), gn.layernorm_bwd_model(x, w, gy, EPS)
    grouped(dx, mb["dx"], rb["dx"], fam, "dx")
    gn.check_elementwise(dw.cpu(), rb["dw"], extra=bounds["dw"], bf16=False, name=f"{fam} dw")
    gn.check_elementwise(db.cpu(), rb["db"], extra=bounds["db"], bf16=False, name=f"{fam} db")
    # backward accumulating into bf16 grads, with and without the residual-path gradient
    gw0, gb0 = rnd(D, seed=seed + 8).to(BF).to(DEV), rnd(D, seed=seed + 9).to(BF).to(DEV)
    gw, gb = gw0.clone(), gb0.clone()
    dx1 = K.layernorm_bwd_bf16_accum(xd, wd, gyd, mean, rstd, gw, gb, None)
    assert torch.equal(dx1, dx)
    assert torch.equal(gw, (gw0.float() + dw).to(BF)) and torch.equal(gb, (gb0.float() + db).to(BF))  # one rounding
    gn.check_elementwise(gw.cpu(), gw0.cpu().double() + rb["dw"], r=2 * gn.U32, extra=bounds["dw"], name=f"{fam} gw")
    gn.check_elementwise(gb.cpu(), gb0.cpu().double() + rb["db"], r=2 * gn.U32, extra=bounds["db"], name=f"{fam} gb")
    gw2, gb2 = gw0.clone(), gb0.clone()
    dx2 = K.layernorm_bwd_bf16_accum(xd, wd, gyd, mean, rstd, gw2, gb2, gaddd)
    assert torch.equal(gw2, gw) and torch.equal(gb2, gb)
    rb2, mb2 = gn.layernorm_bwd_ref64(x, w, gy, EPS, gadd), gn.layernorm_bwd_model(x, w, gy, EPS, gadd)
    grouped(dx2, mb2["dx"], rb2["dx"], fam, "dx + residual gradient")
    assert torch.isfinite(dx2.float()).all()
    # fused residual add: xs is the bf16 add bit for bit, the rest is LayerNorm(xs)
    xs, y2, mean2, rstd2 = K.add_layernorm_fwd_bf16(xd, hd, wd, bd, EPS)
    assert torch.equal(xs, xd + hd) and torch.equal(xs.cpu(), gn.residual_add(x, h))
    y3, mean3, rstd3 = K.layernorm_fwd_bf16(xs, wd, bd, EPS)
    assert torch.equal(y2, y3) and torch.equal(mean2, mean3) and torch.equal(rstd2, rstd3)
    ra = gn.add_layernorm_ref64(x, h, w, b, EPS)
    grouped(y2, gn.layernorm_model(ra["xs"], w, b, EPS)["y"], ra["y"], fam, "add + y")
    ba = gn.layernorm_fp32_bounds(ra["xs"], w, None, EPS)
    gn.check_elementwise(mean2.cpu(), ra["mean"], extra=ba["mean"], bf16=False, name=f"{fam} add mean")
    gn.check_elementwise(rstd2.cpu(), ra["rstd"], extra=ba["rstd"], bf16=False, name=f"{fam} add rstd")


@pytest.mark.parametrize("rows", [1, 3, 5])
@pytest.mark.parametrize("D", LN_D)
def test_layernorm_budget(D, rows):
    for i, family in enumerate(("uniform", "offset", "constant")):
        check_layernorm(family, rows, D, seed=D + 100 * rows + 10 * i)


@pytest.mark.parametrize("family", ["uniform", "offset"])
def test_layernorm_budget_grid_stride(family):
    """16389 rows of D = 8: past the forward's 4096 x 4 and the backward's 1024 x 4 rows per grid pass."""
    check_layernorm(family, 16389, 8, seed=3)


@pytest.mark.parametrize("flat_grads", [True, False])
@pytest.mark.parametrize("rows,D", [(5, 64), (3, 520)])
def test_layernorm_wrappers_run_the_checked_kernels(rows, D, flat_grads):
    """layer_norm, add_layer_norm and layer_norm_pass give the bindings' results bit for bit (the bindings are checked
    against float64 above); without flat gradient buffers the residual-path gradient is one more bf16 add."""
    x, gy, gadd, h, w, b = (t.to(DEV) for t in ln_inputs("uniform", rows, D, seed=D))
    old_w, old_b = rnd(D, seed=1).to(BF).to(DEV), rnd(D, seed=2).to(BF).to(DEV)

    def params():
        ln = torch.nn.LayerNorm(D, eps=EPS).to(DEV, BF)
        with torch.no_grad():
            ln.weight.copy_(w)
            ln.bias.copy_(b)
        if flat_grads:
            ln.weight.grad, ln.bias.grad = old_w.clone(), old_b.clone()
        return ln

    def check_param_grads(ln, xin, mean, rstd):
        _, dw, db = K.layernorm_bwd_bf16(xin, w, gy, mean, rstd)
        if flat_grads:
            assert torch.equal(ln.weight.grad, (old_w.float() + dw).to(BF))
            assert torch.equal(ln.bias.grad, (old_b.float() + db).to(BF))
        else:
            assert torch.equal(ln.weight.grad, dw.to(BF)) and torch.equal(ln.bias.grad, db.to(BF))

    def want_dx(xin, mean, rstd, g_res):
        if flat_grads:
            return K.layernorm_bwd_bf16_accum(xin, w, gy, mean, rstd, old_w.clone(), old_b.clone(), g_res)
        dx = K.layernorm_bwd_bf16(xin, w, gy, mean, rstd)[0]
        return dx if g_res is None else dx + g_res

    y0, mean, rstd = K.layernorm_fwd_bf16(x, w, b, EPS)
    # layer_norm
    ln, xin = params(), x.clone().requires_grad_(True)
    y = layer_norm(xin, ln.weight, ln.bias, EPS)
    y.backward(gy)
    assert torch.equal(y, y0) and torch.equal(xin.grad, want_dx(x, mean, rstd, None))
    check_param_grads(ln, x, mean, rstd)
    # layer_norm_pass
    ln, xin = params(), x.clone().requires_grad_(True)
    xo, y = layer_norm_pass(xin, ln)
    torch.autograd.backward([xo, y], [gadd, gy])
    assert torch.equal(xo, x) and torch.equal(y, y0) and torch.equal(xin.grad, want_dx(x, mean, rstd, gadd))
    check_param_grads(ln, x, mean, rstd)
    # add_layer_norm
    ln, xin, hin = params(), x.clone().requires_grad_(True), h.clone().requires_grad_(True)
    xs, y = add_layer_norm(xin, hin, ln)
    torch.autograd.backward([xs, y], [gadd, gy])
    xs0, ys0, mean_s, rstd_s = K.add_layernorm_fwd_bf16(x, h, w, b, EPS)
    assert torch.equal(xs, xs0) and torch.equal(xs, x + h) and torch.equal(y, ys0)
    assert torch.equal(xin.grad, want_dx(xs0, mean_s, rstd_s, gadd)) and torch.equal(xin.grad, hin.grad)
    check_param_grads(ln, xs0, mean_s, rstd_s)


# =====================================================================================================================
# bias gradient (column sums accumulated into a bf16 gradient)
@pytest.mark.parametrize("padded", [False, True])
@pytest.mark.parametrize("M", [1, 3, 4, 5, 16, 17, 63, 64, 65, 4101])
def test_bias_grad_budget(M, padded):
    for N in (1, 63, 64, 65, 776):
        gy = rnd(M, N, seed=M + N).to(BF)
        gb0 = rnd(N, seed=M + N + 1).to(BF)
        if padded:  # rows with stride(0) > N; the pad is never read (NaN there)
            buf = torch.full((M, N + 8), math.nan, dtype=BF)
            buf[:, :N] = gy
            gd = buf.to(DEV)[:, :N]
            assert M == 1 or gd.stride(0) == N + 8
        else:
            gd = gy.to(DEV)
        gb = gb0.clone().to(DEV)
        K.bias_grad_bf16_(gd, gb)
        want = gb0.double() + gn.colsum_ref64(gy)
        # fp32 sum of M terms in any order, the fp32 add of the old value, one bf16 rounding
        gn.check_elementwise(gb.cpu(), want, r=2 * gn.U32, extra=gn.colsum_bound(gy), name=f"bias grad M={M} N={N}")
    gy3 = rnd(3, M, 64, seed=M).to(BF)  # leading dimensions are flattened
    gb = torch.zeros(64, dtype=BF, device=DEV)
    K.bias_grad_bf16_(gy3.to(DEV), gb)
    gn.check_elementwise(gb.cpu(), gn.colsum_ref64(gy3), r=2 * gn.U32, extra=gn.colsum_bound(gy3), name="bias grad 3-D")


# =====================================================================================================================
def test_bindings_refuse_unsupported_layouts_before_launching():
    """Host-side checks only: each call raises in the binding, before any kernel is launched."""
    q = torch.zeros(1, 4, 1, 32, dtype=BF, device=DEV)
    with pytest.raises(RuntimeError, match="64"):
        K.attention_fwd(q, q, q, SCALE, True)  # head width 32
    q = torch.zeros(1, 4, 1, 64, dtype=BF, device=DEV)
    with pytest.raises(RuntimeError, match="share shape and strides"):
        K.attention_fwd(q, q, torch.zeros(1, 5, 1, 64, dtype=BF, device=DEV), SCALE, False)
    with pytest.raises(RuntimeError, match="logits"):
        K.cross_entropy_bf16(torch.zeros(8, dtype=BF, device=DEV), torch.zeros(1, dtype=torch.int64, device=DEV), 1.0,
                             -100, True)
    with pytest.raises(RuntimeError, match="target"):
        K.cross_entropy_bf16(torch.zeros(2, 8, dtype=BF, device=DEV), torch.zeros(3, dtype=torch.int64, device=DEV),
                             1.0, -100, True)
    w = torch.ones(12, dtype=BF, device=DEV)
    with pytest.raises(RuntimeError, match="layernorm"):
        K.layernorm_fwd_bf16(torch.zeros(2, 12, dtype=BF, device=DEV), w, w, EPS)  # D % 8 != 0
    w = torch.ones(4104, dtype=BF, device=DEV)
    with pytest.raises(RuntimeError, match="layernorm"):
        K.layernorm_fwd_bf16(torch.zeros(2, 4104, dtype=BF, device=DEV), w, w, EPS)  # D > 4096
    with pytest.raises(RuntimeError, match="gb size"):
        K.bias_grad_bf16_(torch.zeros(3, 8, dtype=BF, device=DEV), torch.zeros(9, dtype=BF, device=DEV))
