"""The fp8 KV-cache kernels (kv_quantize.hip, attention_decode_fp8.hip) against the torch twin bit for bit where the
format decides (bytes, exponents, cache writes) and against the float64 reference with attention_decode's budget on
the dequantised cache (docs/NUMERICS.md "fp8 KV cache"); liveness, batch invariance, determinism; generate(kv_dtype=
"fp8") eager against graph-replayed and alone against in the batch. Grouped checks print `NUMERICS ...` lines."""
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no ROCm GPU", allow_module_level=True)

import gpt2_decode_numerics as dn  # noqa: E402
import gpt2_numerics as gn  # noqa: E402
import test_decode_kernels_gpu as tk  # noqa: E402  (FAMILIES, LENS, decode_case, rnd)
from generate_util import VOCAB  # noqa: E402
from test_kv_fp8_cpu import edge_rows  # noqa: E402
from simple_distributed_machine_learning_amd import _native  # noqa: E402
from simple_distributed_machine_learning_amd.ops import decode as dec  # noqa: E402
from simple_distributed_machine_learning_amd.parallel.generate import generate  # noqa: E402

DEV = torch.device("cuda", 0)
K = _native.kernels()
BF = torch.bfloat16
SCALE = 0.125
B, H, SMAX = 16, 3, 1024


# =====================================================================================================================
# kv_quantize_rows
@pytest.mark.parametrize("S", [1, 5, 65])
@pytest.mark.parametrize("data", ["0.1", "1.5", "6", "edges"])
def test_kv_quantize_rows_matches_the_twin(data, S):
    nb, smax = 2, 70
    if data == "edges":  # the format's edge rows, dealt over every (sample, position, head) of k and v
        rows = edge_rows()[1]
        pick = (torch.arange(nb * S * 3 * H) * 5 + S) % rows.shape[0]
        qkv = rows[pick].view(nb, S, 3 * H * 64)
    else:
        qkv = (tk.rnd(nb, S, 3 * H * 64, seed=S) * float(data)).to(BF)
    want = [torch.full((nb, smax, H, 64), 0xAB, dtype=torch.uint8), torch.full((nb, H, smax), 77, dtype=torch.int8)]
    want = [t.clone() for t in want * 2]
    got = [t.to(DEV) for t in want]
    dec.kv_quantize_rows_ref(qkv, *want, S)
    K.kv_quantize_rows(qkv.to(DEV), *got, S)
    for g, w, name in zip(got, want, ("k8", "ke", "v8", "ve")):  # rows >= S keep their fill
        assert torch.equal(g.cpu(), w), name


# =====================================================================================================================
# attention_decode_fp8
def fp8_case(family, seed):
    """tk.decode_case with the caches quantised by the twin: (qkv, [k8, ke, v8, ve], lens, (qn, kn, vn))."""
    qkv, k, v, lens, new = tk.decode_case(family, seed, B, H, SMAX)
    cache = []
    for t in (k, v):
        q, e = dec.kv_quantize(t)
        cache += [q, e.transpose(1, 2).contiguous()]
    return qkv, cache, lens, new


def fill_tail(cache, lens, byte, exp):
    out = [t.clone() for t in cache]
    for b, n in enumerate(lens.tolist()):
        for q8, ex in (out[0:2], out[2:4]):
            q8[b, n:] = byte
            ex[b, :, n:] = exp
    return out


def run_decode(qkv, cache, lens, n_keys):
    dev = [t.to(DEV) for t in cache]
    out = K.attention_decode_fp8(qkv.to(DEV), *dev, lens.to(DEV), SCALE, n_keys)
    torch.cuda.synchronize()
    return out.cpu(), [t.cpu() for t in dev]


@pytest.mark.parametrize("family", tk.FAMILIES)
def test_attention_decode_fp8_budget_and_cache(family):
    qkv, cache, lens, (qn, kn, vn) = fp8_case(family, seed=11 + 100 * tk.FAMILIES.index(family))
    nan_tail = fill_tail(cache, lens, 0xFF, 127)  # e4m3fn NaN bytes under the largest exponent
    out, after = run_decode(qkv, nan_tail, lens, SMAX)
    assert bool(torch.isfinite(out.float()).all()), "NaN rows above lens[b] reached the output"
    # cache: row lens[b] holds the twin's quantisation of the new k, v; every other byte and exponent is unchanged
    full = [t.clone() for t in cache]  # the cache as later steps read it, live rows only
    for new, (q8, ex), (a8, ax), (n8, nx) in ((kn, full[0:2], after[0:2], nan_tail[0:2]),
                                              (vn, full[2:4], after[2:4], nan_tail[2:4])):
        q, e = dec.kv_quantize(new)  # [B, H, 64], [B, H]
        for b, n in enumerate(lens.tolist()):
            assert torch.equal(a8[b, n], q[b]) and torch.equal(ax[b, :, n], e[b]), b
            n8[b, n], nx[b, :, n], q8[b, n], ex[b, :, n] = q[b], e[b], q[b], e[b]
        assert torch.equal(a8, n8) and torch.equal(ax, nx)
    # the same bits with zeros in place of the NaNs
    out0, _ = run_decode(qkv, fill_tail(cache, lens, 0, 0), lens, SMAX)
    assert torch.equal(tk.bits(out0), tk.bits(out))
    # the numbers: dequantisation is exact, so the budget is attention_decode's on the dequantised cache
    Kd = dec.kv_dequantize(full[0], full[1].transpose(1, 2))
    Vd = dec.kv_dequantize(full[2], full[3].transpose(1, 2))
    r64 = dn.attention_decode_ref64(qn, Kd, Vd, lens, SCALE)
    model = dn.attention_decode_model(qn, Kd, Vd, lens, SCALE)
    row, rms = gn.check_grouped(out.view(B, H, 64), model, r64, name=f"attention_decode_fp8 {family}")
    print(f"NUMERICS attention_decode_fp8 {family} | y | row {row:.3f} | rms {rms:.4f}")
    # the twin on the same cache agrees to the same budget
    twin = dec.attention_decode_fp8_ref(qkv, *fill_tail(cache, lens, 0xFF, 127), lens, H, SMAX)
    gn.check_grouped(twin.view(B, H, 64), model, r64, name=f"attention_decode_fp8_ref {family}")


def test_attention_decode_fp8_batch_invariance_and_determinism():
    qkv, cache, lens, _ = fp8_case("uniform 1.5", seed=11)
    cache = fill_tail(cache, lens, 0xFF, 127)
    out, _ = run_decode(qkv, cache, lens, SMAX)
    again, _ = run_decode(qkv, cache, lens, SMAX)
    assert torch.equal(tk.bits(again), tk.bits(out))
    five = [t[5:6].contiguous() for t in cache]
    one, _ = run_decode(qkv[5:6], five, lens[5:6], SMAX)
    assert torch.equal(tk.bits(one[0]), tk.bits(out[5]))
    one, _ = run_decode(qkv[5:6], five, lens[5:6], int(lens[5]) + 1)  # fewer chunk blocks launched
    assert torch.equal(tk.bits(one[0]), tk.bits(out[5]))


def test_attention_decode_fp8_refusals():
    qkv, cache, lens, _ = fp8_case("uniform 1.5", seed=3)
    qkv, lens, dev = qkv.to(DEV), lens.to(DEV), [t.to(DEV) for t in cache]
    with pytest.raises(RuntimeError, match="cache is full"):
        K.attention_decode_fp8(qkv, *dev, lens, SCALE, SMAX + 1)
    with pytest.raises(RuntimeError, match="contiguous uint8"):
        K.attention_decode_fp8(qkv, dev[0].view(torch.int8), *dev[1:], lens, SCALE, 8)
    with pytest.raises(RuntimeError, match="contiguous uint8"):
        K.attention_decode_fp8(qkv, dev[0][:, ::2], dev[1][:, :, ::2], dev[2][:, ::2], dev[3][:, :, ::2], lens, SCALE,
                               8)
    with pytest.raises(RuntimeError, match="contiguous int8"):
        K.attention_decode_fp8(qkv, dev[0], dev[1].view(torch.uint8), dev[2], dev[3], lens, SCALE, 8)
    with pytest.raises(RuntimeError, match="lens must be int32"):
        K.attention_decode_fp8(qkv, *dev, lens.long(), SCALE, 8)
    with pytest.raises(RuntimeError, match="head width 64"):
        K.attention_decode_fp8(qkv, dev[0].view(B, SMAX, 2 * H, 32), dev[1], dev[2].view(B, SMAX, 2 * H, 32), dev[3],
                               lens, SCALE, 8)
    with pytest.raises(ValueError, match="no one-launch"):
        dec.attention_decode(qkv, dev[0], dev[2], lens, H, 8, tickets=torch.zeros(B * H, dtype=torch.int32, device=DEV))


# =====================================================================================================================
# generate(kv_dtype="fp8") on the kernels
@pytest.fixture(scope="module")
def engine():
    from simple_distributed_machine_learning_amd.models.gpt2 import GPT2Config, gpt2_spec
    from simple_distributed_machine_learning_amd.parallel import PipelineEngine, init_mesh

    cfg = GPT2Config(n_layer=2, n_head=2, n_embd=128, vocab_size=VOCAB, block_size=160)
    mesh = init_mesh(pp=1, schedule_kind="1f1b", rank=0, world_size=1, device=DEV, timeout_s=120)
    spec = gpt2_spec(2, cfg=cfg, seq_len=32, dtype=BF, name="gpt2_d64_long")
    return PipelineEngine(spec, mesh, schedule_kind="1f1b", num_microbatches=1, seed=1)


@pytest.mark.parametrize("kw", [{}, {"temperature": 0.9, "top_k": 20, "seed": 5}], ids=["greedy", "top_k"])
def test_generate_fp8_graph_and_batch_invariance(engine, kw):
    """Prompts of 60 tokens and 80 new ones: the cache crosses the 64- and the 128-key edges."""
    prompts = (torch.arange(3 * 60).view(3, 60) * 7 + 3) % VOCAB
    eager = generate(engine, prompts, 80, kv_dtype="fp8", **kw)
    graphed = generate(engine, prompts, 80, kv_dtype="fp8", graph=True, **kw)
    assert torch.equal(graphed, eager)
    assert torch.equal(generate(engine, prompts, 80, kv_dtype="fp8", graph=True, **kw), eager)  # a replayed session
    one = generate(engine, prompts[1:2], 80, kv_dtype="fp8", sample0=1, **kw)
    assert torch.equal(one[0], eager[1])
    for c in engine.decode_session.caches.values():
        for t, e in zip(c.k + c.v, c.ke + c.ve):
            assert (t.dtype, tuple(t.shape)) == (torch.uint8, (3, 140, 2, 64))
            assert (e.dtype, tuple(e.shape)) == (torch.int8, (3, 2, 140))
