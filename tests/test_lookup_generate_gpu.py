"""Prompt-lookup speculation on the real kernels: decode_block's logits against sequential decode_step logits bit for
bit (teacher forcing), generate(lookup=K) against generate() bit for bit in tokens and lengths, and the step counts
against the pure-Python simulation. The d = 64 config of tests/generate_util.py trained on the device, and the same
config with block_size 192, whose cache crosses the decode attention's 64- and 128-key chunk edges."""
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no ROCm GPU", allow_module_level=True)

import lookup_util as lu  # noqa: E402
from generate_util import VOCAB, make_engine, rule_holds, train_steps  # noqa: E402
from simple_distributed_machine_learning_amd.parallel.generate import generate, pad_prompts  # noqa: E402

BF = torch.bfloat16
DEV = torch.device("cuda", 0)
PROMPTS = lu.rule_prompts([1, 2, 5, 17, 40, 63, 77, 96])  # B = 8: 64 rows per verify step at K = 7


@pytest.fixture(scope="module")
def trained():
    """tests/test_generate_gpu.py's model: block_size 64, 200 AdamW steps (lr 3e-3) of 16 x 32 tokens."""
    return train_steps(make_engine("gpt2_d64", "cuda:0", BF), 200, 16, 32)


@pytest.fixture(scope="module")
def long_model():
    """block_size 192, 60 steps: bit equality does not need this model to be good."""
    return train_steps(lu.make_engine_d64("cuda:0", BF, 192), 60, 16, 32)


def bits(t):
    return t.contiguous().view(torch.int16)


# ---- 1. the teacher-forced block ------------------------------------------------------------------------------------
def _block_vs_steps(engine, S0, T, nq_rows=None, smax=None):
    """Prefill S0 tokens of a B = 4 batch twice; T decode_step logits on one cache against one decode_block on the
    other. Returns (block logits [B, T, ld], step logits [B, T, ld], the caches)."""
    s0, s1 = engine.stages[0], engine.stages[1]
    smax = smax or s0.cfg.block_size
    g = torch.Generator().manual_seed(100 * S0 + T)
    seq = torch.randint(0, VOCAB, (4, S0 + T), generator=g).to(DEV)
    a0, a1 = s0.new_cache(4, smax), s1.new_cache(4, smax)
    b0, b1 = s0.new_cache(4, smax), s1.new_cache(4, smax)
    s1.prefill(s0.prefill(seq[:, :S0], a0), a1)
    s1.prefill(s0.prefill(seq[:, :S0], b0), b1)
    steps = torch.stack([s1.decode_step(s0.decode_step(seq[:, S0 + t], a0), a1) for t in range(T)], 1)
    b1.lens = b0.lens  # one device-side length for the rank's stages
    nq = torch.tensor(nq_rows or [T] * 4, dtype=torch.int32, device=DEV)
    block = s1.decode_block(s0.decode_block(seq[:, S0:].contiguous(), b0, nq), b1, nq)
    assert block.shape == (4 * T, steps.shape[-1]) and b0.lens.tolist() == [S0] * 4  # the lengths are not advanced
    assert b0.n == b1.n == min(S0 + T, smax) and a0.n == S0 + T
    return block.view(4, T, -1), steps, (a0, a1, b0, b1)


@pytest.mark.parametrize("T", [2, 4, 8])
def test_decode_block_logits_are_decode_step_logits_bit_for_bit(trained, long_model, T):
    """The crux: every kernel of the step computes a row from that row alone, and attention_append keeps
    attention_decode's bits."""
    for engine, S0 in ((trained, 17), (long_model, 62), (long_model, 125)):
        block, steps, (a0, a1, b0, b1) = _block_vs_steps(engine, S0, T)
        assert torch.equal(bits(block), bits(steps)), (S0, T)
        for ca, cb in ((a0, b0), (a1, b1)):  # and the caches hold the same rows
            for i in range(len(ca.k)):
                assert torch.equal(bits(ca.k[i][:, :S0 + T]), bits(cb.k[i][:, :S0 + T]))
                assert torch.equal(bits(ca.v[i][:, :S0 + T]), bits(cb.v[i][:, :S0 + T]))
    # rows with fewer live tokens: the live ones are unchanged
    nq = [T, 1, T // 2, 0]
    block, steps, _ = _block_vs_steps(long_model, 62, T, nq)
    for b, n in enumerate(nq):
        assert torch.equal(bits(block[b, :n]), bits(steps[b, :n])), (b, n)
    assert bool(torch.isfinite(block.float()).all())


def test_decode_block_refuses_more_than_64_rows(trained):
    s0 = trained.stages[0]
    cache = s0.new_cache(9, 32)
    with pytest.raises(ValueError, match="at most 64 rows"):
        s0.decode_block(torch.zeros(9, 8, dtype=torch.int64, device=DEV), cache,
                        torch.ones(9, dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError, match="at most 64"):
        generate(trained, torch.arange(VOCAB)[:, None], 8, lookup=3)
    with pytest.raises(ValueError, match="at most 64"):
        generate(trained, lu.rule_prompts(range(1, 10)), 8, lookup=7)


# ---- 2./3. end to end ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def plain(trained):
    """The plain runs, shared and left unchanged: mode -> (kwargs, tokens, lengths)."""
    ragged, plens = pad_prompts([PROMPTS[0].tolist(), PROMPTS[1, :3].tolist(), PROMPTS[2, :7].tolist(),
                                 PROMPTS[3, :1].tolist(), PROMPTS[4, :5].tolist()], 0)
    modes = {"greedy": (PROMPTS, {}),
             "sampled": (PROMPTS, dict(temperature=0.9, top_k=20, seed=3)),
             "ragged": (ragged, dict(temperature=0.9, top_k=20, top_p=0.9, seed=5, prompt_lens=plens,
                                     eos_token=int(PROMPTS[0, 3]), pad_token=0))}
    return {m: (p, kw) + tuple(generate(trained, p, 24, return_lengths=True, **kw)) for m, (p, kw) in modes.items()}


@pytest.mark.parametrize("K", [1, 3, 7])
@pytest.mark.parametrize("mode", ["greedy", "sampled", "ragged"])
def test_lookup_returns_the_plain_tokens_and_lengths_bit_for_bit(trained, plain, mode, K):
    prompts, kw, want, wlen = plain[mode]
    if mode == "greedy":
        assert bool(rule_holds(want).all())  # (the model learnt the rule: the drafts are right)
    for sc in (0, 4):
        got, glen, stats = generate(trained, prompts, 24, lookup=K, stop_check=sc, return_lengths=True,
                                    return_stats=True, **kw)
        assert torch.equal(got, want) and torch.equal(glen, wlen), (mode, K, sc)
        plens = kw["prompt_lens"].tolist() if "prompt_lens" in kw else [prompts.shape[1]] * len(prompts)
        steps = lu.check_row_steps(got, glen, stats, plens, 24, K, 2, kw.get("eos_token"))
        # the host's loop: all 23 steps, or up to the first look (every 4 steps) that finds all rows done or full
        assert stats["steps"] == (23 if sc == 0 else min(23, -(-max(max(steps), 1) // 4) * 4))
    if mode == "greedy":  # the rule prompt's figure: 4 tokens per step, ceil(23 / 4) = 6 at K = 3
        assert steps == [-(-23 // (min(K, 6) + 1))] * len(prompts)
        assert K != 3 or stats["row_steps"].tolist() == [6] * len(prompts)


@pytest.mark.parametrize("K", [3, 7])
def test_150_tokens_across_the_chunk_edges(long_model, K):
    """block_size 192: the cache grows from 8 to 158 rows, across the 64- and 128-key edges, in steps of up to K + 1."""
    for kw in ({}, dict(temperature=0.8, top_k=10, seed=7)):
        want, wlen = generate(long_model, PROMPTS, 150, return_lengths=True, **kw)
        got, glen, stats = generate(long_model, PROMPTS, 150, lookup=K, stop_check=8, return_lengths=True,
                                    return_stats=True, **kw)
        assert torch.equal(got, want) and torch.equal(glen, wlen)
        steps = lu.check_row_steps(got, glen, stats, [8] * len(PROMPTS), 150, K, 2)
        print(f"150 tokens, K={K}, {'sampled' if kw else 'greedy'}: row steps {steps}, host steps {stats['steps']}")
        assert max(steps) <= 149
