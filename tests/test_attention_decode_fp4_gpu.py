"""The fp4 KV-cache kernels (kv_quantize_fp4.hip, attention_decode_fp4.hip) against the torch twin bit for bit where
the format decides (nibbles, exponents, cache writes) and against the float64 reference with attention_decode's budget
on the dequantised cache (docs/NUMERICS.md "fp4 KV cache"); liveness, batch invariance, determinism, the run length;
generate(kv_dtype="fp4") eager against graph-replayed. Grouped checks print `NUMERICS ...` lines."""
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no ROCm GPU", allow_module_level=True)

import gpt2_decode_numerics as dn  # noqa: E402
import gpt2_numerics as gn  # noqa: E402
import test_decode_kernels_gpu as tk  # noqa: E402  (FAMILIES, decode_case, rnd, bits)
from generate_util import VOCAB  # noqa: E402
from test_kv_fp4_cpu import edge_rows  # noqa: E402
from simple_distributed_machine_learning_amd import _native  # noqa: E402
from simple_distributed_machine_learning_amd.ops import decode as dec  # noqa: E402
from simple_distributed_machine_learning_amd.parallel.generate import generate  # noqa: E402

DEV = torch.device("cuda", 0)
K = _native.kernels()
BF = torch.bfloat16
SCALE = 0.125
B, H, SMAX = 16, 3, 1024


@pytest.mark.parametrize("S", [1, 5, 65])
@pytest.mark.parametrize("data", ["0.1", "1.5", "6", "edges"])
def test_kv_quantize_rows_fp4_matches_the_twin(data, S):
    nb, smax = 2, 70
    if data == "edges":  # the format's edge rows, dealt over every (sample, position, head) of k and v
        rows = torch.stack(list(edge_rows().values()))
        pick = (torch.arange(nb * S * 3 * H) * 5 + S) % rows.shape[0]
        qkv = rows[pick].view(nb, S, 3 * H * 64)
    else:
        qkv = (tk.rnd(nb, S, 3 * H * 64, seed=S) * float(data)).to(BF)
    want = [torch.full((nb, smax, H, 32), 0xAB, dtype=torch.uint8), torch.full((nb, H, smax, 2), 77, dtype=torch.int8)]
    want = [t.clone() for t in want * 2]
    got = [t.to(DEV) for t in want]
    dec.kv_quantize_rows_fp4_ref(qkv, *want, S)
    K.kv_quantize_rows_fp4(qkv.to(DEV), *got, S)
    for g, w, name in zip(got, want, ("k4", "ke", "v4", "ve")):  # rows >= S keep their fill
        assert torch.equal(g.cpu(), w), name


def fp4_case(family, seed):
    """tk.decode_case with the caches quantised by the twin: (qkv, [k4, ke, v4, ve], lens, (qn, kn, vn))."""
    qkv, k, v, lens, new = tk.decode_case(family, seed, B, H, SMAX)
    cache = []
    for t in (k, v):
        q, e = dec.kv_quantize_fp4(t)
        cache += [q, e.transpose(1, 2).contiguous()]
    return qkv, cache, lens, new


def fill_tail(cache, lens, byte, exp):
    out = [t.clone() for t in cache]
    for b, n in enumerate(lens.tolist()):
        for q4, ex in (out[0:2], out[2:4]):
            q4[b, n:] = byte
            ex[b, :, n:] = exp
    return out


def run_decode(qkv, cache, lens, n_keys, run=0):
    dev = [t.to(DEV) for t in cache]
    out = K.attention_decode_fp4(qkv.to(DEV), *dev, lens.to(DEV), SCALE, n_keys, run)
    torch.cuda.synchronize()
    return out.cpu(), [t.cpu() for t in dev]


@pytest.mark.parametrize("family", tk.FAMILIES)
def test_attention_decode_fp4_budget_and_cache(family):
    qkv, cache, lens, (qn, kn, vn) = fp4_case(family, seed=11 + 100 * tk.FAMILIES.index(family))
    huge_tail = fill_tail(cache, lens, 0x77, 120)  # dead rows of 6 * 2^120: their products would overflow
    out, after = run_decode(qkv, huge_tail, lens, SMAX)
    assert bool(torch.isfinite(out.float()).all()), "rows above lens[b] reached the output"
    # cache: row lens[b] holds the twin's quantisation of the new k, v; every other byte and exponent is unchanged
    full = [t.clone() for t in cache]  # the cache as later steps read it, live rows only
    for new, (q4, ex), (a4, ax), (n4, nx) in ((kn, full[0:2], after[0:2], huge_tail[0:2]),
                                              (vn, full[2:4], after[2:4], huge_tail[2:4])):
        q, e = dec.kv_quantize_fp4(new)  # [B, H, 32], [B, H, 2]
        for b, n in enumerate(lens.tolist()):
            assert torch.equal(a4[b, n], q[b]) and torch.equal(ax[b, :, n], e[b]), b
            n4[b, n], nx[b, :, n], q4[b, n], ex[b, :, n] = q[b], e[b], q[b], e[b]
        assert torch.equal(a4, n4) and torch.equal(ax, nx)
    # the same bits with zeros in place of the huge rows
    out0, _ = run_decode(qkv, fill_tail(cache, lens, 0, 0), lens, SMAX)
    assert torch.equal(tk.bits(out0), tk.bits(out))
    # the numbers: dequantisation is exact, so the budget is attention_decode's on the dequantised cache
    Kd = dec.kv_dequantize_fp4(full[0], full[1].transpose(1, 2))
    Vd = dec.kv_dequantize_fp4(full[2], full[3].transpose(1, 2))
    r64 = dn.attention_decode_ref64(qn, Kd, Vd, lens, SCALE)
    model = dn.attention_decode_model(qn, Kd, Vd, lens, SCALE)
    row, rms = gn.check_grouped(out.view(B, H, 64), model, r64, name=f"attention_decode_fp4 {family}")
    print(f"NUMERICS attention_decode_fp4 {family} | y | row {row:.3f} | rms {rms:.4f}")


def test_attention_decode_fp4_batch_invariance_determinism_and_run_length():
    qkv, cache, lens, _ = fp4_case("uniform 1.5", seed=11)
    cache = fill_tail(cache, lens, 0x77, 120)
    out, after = run_decode(qkv, cache, lens, SMAX)
    again, _ = run_decode(qkv, cache, lens, SMAX)
    assert torch.equal(tk.bits(again), tk.bits(out))
    for run in (1, 2, 4):  # the chunks one wave owns: the same slots, the same bits, the same cache
        o, a = run_decode(qkv, cache, lens, SMAX, run)
        assert torch.equal(tk.bits(o), tk.bits(out)) and all(torch.equal(x, y) for x, y in zip(a, after)), run
    five = [t[5:6].contiguous() for t in cache]
    one, _ = run_decode(qkv[5:6], five, lens[5:6], SMAX)
    assert torch.equal(tk.bits(one[0]), tk.bits(out[5]))
    one, _ = run_decode(qkv[5:6], five, lens[5:6], int(lens[5]) + 1)  # fewer chunk blocks launched
    assert torch.equal(tk.bits(one[0]), tk.bits(out[5]))


@pytest.fixture(scope="module")
def engine():
    from simple_distributed_machine_learning_amd.models.gpt2 import GPT2Config, gpt2_spec
    from simple_distributed_machine_learning_amd.parallel import PipelineEngine, init_mesh

    cfg = GPT2Config(n_layer=2, n_head=2, n_embd=128, vocab_size=VOCAB, block_size=160)
    mesh = init_mesh(pp=1, schedule_kind="1f1b", rank=0, world_size=1, device=DEV, timeout_s=120)
    spec = gpt2_spec(2, cfg=cfg, seq_len=32, dtype=BF, name="gpt2_d64_long")
    return PipelineEngine(spec, mesh, schedule_kind="1f1b", num_microbatches=1, seed=1)


@pytest.mark.parametrize("kw", [{}, {"temperature": 0.9, "top_k": 20, "seed": 5}], ids=["greedy", "top_k"])
def test_generate_fp4_graph_and_batch_invariance(engine, kw):
    """Prompts of 60 tokens and 80 new ones: the cache crosses the 64- and the 128-key edges."""
    prompts = (torch.arange(3 * 60).view(3, 60) * 7 + 3) % VOCAB
    eager = generate(engine, prompts, 80, kv_dtype="fp4", **kw)
    graphed = generate(engine, prompts, 80, kv_dtype="fp4", graph=True, **kw)
    assert torch.equal(graphed, eager)
    assert torch.equal(generate(engine, prompts, 80, kv_dtype="fp4", graph=True, **kw), eager)  # a replayed session
    one = generate(engine, prompts[1:2], 80, kv_dtype="fp4", sample0=1, **kw)
    assert torch.equal(one[0], eager[1])
    for c in engine.decode_session.caches.values():
        for t, e in zip(c.k + c.v, c.ke + c.ve):
            assert (t.dtype, tuple(t.shape)) == (torch.uint8, (3, 140, 2, 32))
            assert (e.dtype, tuple(e.shape)) == (torch.int8, (3, 2, 140, 2))
