"""The fp8 KV cache's torch twins on the CPU with gpt2_tiny (ops/decode.py kv_quantize is the format; docs/NUMERICS.md
"fp8 KV cache"): the format's properties on rows built for its edges, batch invariance of generate(kv_dtype="fp8"),
kv_dtype="bf16" as the default, and the refusals."""
import pytest
import torch

from generate_util import make_engine
from simple_distributed_machine_learning_amd.ops.decode import kv_dequantize, kv_quantize
from simple_distributed_machine_learning_amd.parallel.generate import generate
from simple_distributed_machine_learning_amd.parallel.session import GenerationSession

BF = torch.bfloat16


def edge_rows():
    """bf16 rows [R, 64] at the format's edges; every row also carries small entries and a -0."""
    base = torch.linspace(-1.0, 1.0, 64)
    rows = {"zero": torch.zeros(64)}
    for k in (-130, -9, 0, 7, 119):  # amax exactly 448 * 2^k (the clamps at both ends included)
        rows[f"448*2^{k}"] = torch.ldexp(base * 448.0, torch.tensor(k))
    for x in (-3, 0, 5):  # amax 1.75 * 2^x and its bf16 neighbour above: the exponent steps between them
        rows[f"1.75*2^{x}"] = torch.ldexp(base * 1.75, torch.tensor(x))
        rows[f"1.7578125*2^{x}"] = torch.ldexp(base * 1.7578125, torch.tensor(x))
    sub = base * 300.0  # entries below 2^-6 of the scaled row land in e4m3's subnormals, below 2^-10 on zero
    sub[1:40] = torch.ldexp(torch.linspace(1.0, 1.96875, 39), torch.arange(39) % 14 - 12) * (-1.0) ** torch.arange(39)
    rows["subnormals"] = sub
    out = torch.stack(list(rows.values())).to(BF)
    out[:, 5] = -0.0
    return list(rows), out


def test_kv_quantize_format_on_edge_rows():
    names, x = edge_rows()
    q, e = kv_quantize(x)
    assert q.dtype == torch.uint8 and e.dtype == torch.int8 and q.shape == x.shape and e.shape == x.shape[:1]
    xd, ed = x.double(), e.double()
    scaled_max = (xd.abs().amax(-1) * torch.exp2(-ed))
    for n, m, ee in zip(names, scaled_max.tolist(), e.tolist()):
        clamped = ee in (-120, 120)
        assert m == 0 and ee == 0 if n == "zero" else (224 < m <= 448 or (clamped and m <= 448)), (n, m, ee)
    assert e[names.index("1.75*2^0")] == -8 and e[names.index("1.7578125*2^0")] == -7
    assert bool((q[:, 5] == 0x80).all()), "-0 keeps its sign"
    deq = kv_dequantize(q, e)
    assert deq.dtype == torch.float32
    err = (xd - deq.double()).abs()
    bound = torch.maximum(xd.abs() * 2.0 ** -4, torch.exp2(ed - 10)[:, None])
    assert bool((err <= bound).all()), (err / bound).max()
    sub = q[names.index("subnormals"), 1:40] & 0x7F
    assert bool((sub < 8).any()) and bool((sub == 0).any()), "the row reaches e4m3's subnormals and its zero"
    q2, e2 = kv_quantize(deq)  # the dequantised row is a fixed point
    assert torch.equal(kv_dequantize(q2, e2), deq)


@pytest.fixture(scope="module")
def tiny():
    return make_engine("gpt2_tiny", "cpu", torch.float32)


PROMPTS = torch.tensor([[3, 14, 15, 92, 65, 35], [8, 9, 79, 32, 38, 46], [2, 6, 43, 38, 32, 79]])


@pytest.mark.parametrize("kw", [{}, {"temperature": 0.9, "top_k": 20, "top_p": 0.9, "seed": 5}],
                         ids=["greedy", "sampled"])
def test_fp8_rows_do_not_depend_on_the_batch(tiny, kw):
    out = generate(tiny, PROMPTS, 12, kv_dtype="fp8", **kw)
    assert out.shape == (3, 18)
    for b in range(3):
        assert torch.equal(generate(tiny, PROMPTS[b:b + 1], 12, kv_dtype="fp8", sample0=b, **kw)[0], out[b]), b
    lens = torch.tensor([6, 3, 5], dtype=torch.int32)  # ragged prompts, an eos
    rag, n = generate(tiny, PROMPTS, 12, kv_dtype="fp8", prompt_lens=lens, eos_token=7, return_lengths=True, **kw)
    one, n1 = generate(tiny, PROMPTS[1:2, :3], 12, kv_dtype="fp8", prompt_lens=lens[1:2], eos_token=7, sample0=1,
                       return_lengths=True, **kw)
    assert int(n1[0]) == int(n[1]) and torch.equal(one[0, :int(n1[0])], rag[1, :int(n[1])])


def test_bf16_is_the_default(tiny):
    kw = {"temperature": 0.9, "top_k": 20, "seed": 5}
    assert torch.equal(generate(tiny, PROMPTS, 12, kv_dtype="bf16", **kw), generate(tiny, PROMPTS, 12, **kw))
    cache = tiny.stages[0].new_cache(2, 8)
    assert cache.kv_dtype == "bf16" and cache.ke is None and cache.k[0].dtype == torch.float32


@pytest.mark.parametrize("kw,msg", [
    ({"lookup": 2}, "not supported with lookup > 0"),
    ({"num_samples": 2}, "not supported with num_samples > 1"),
    ({"num_beams": 2}, "not supported with num_beams > 1"),
    ({"prefill_chunk": 4}, "not supported with prefill_chunk > 0"),
])
def test_fp8_refusals(tiny, kw, msg):
    with pytest.raises(ValueError, match=msg):
        generate(tiny, PROMPTS, 4, kv_dtype="fp8", **kw)


def test_fp8_refusals_below_generate(tiny):
    with pytest.raises(ValueError, match="kv_dtype must be one of"):
        generate(tiny, PROMPTS, 4, kv_dtype="int8")
    with pytest.raises(ValueError, match="GenerationSession: kv_dtype='fp8' is not supported"):
        GenerationSession(tiny, PROMPTS, 16, kv_dtype="fp8")
    st = tiny.stages[0]
    cache = st.new_cache(3, 16, kv_dtype="fp8")
    assert cache.k[0].dtype == torch.uint8 and cache.ke[0].dtype == torch.int8 and cache.ke[0].shape[0::2] == (3, 16)
    nq = torch.ones(3, dtype=torch.int32)
    for call, who in ((lambda: st.extend(PROMPTS, cache), "extend"), (lambda: st.decode_block(PROMPTS, cache, nq),
                      "decode_block"), (lambda: st.fork_cache(cache, 2, 4), "fork_cache"),
                      (lambda: st.beam_cache(cache, 2, 4), "beam_cache")):
        with pytest.raises(ValueError, match=f"{who}: a kv_dtype='fp8' cache"):
            call()
