"""Several samples per prompt on the real kernels: generate(num_samples=n) against the call on the n-fold repeated
prompts, bit for bit in tokens, lengths and stats, in every sampling mode. The d = 64 config of tests/lookup_util.py with
block_size 192, whose caches cross the decode attention's 64- and 128-key chunk edges."""
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no ROCm GPU", allow_module_level=True)

import fork_util as fu  # noqa: E402
import lookup_util as lu  # noqa: E402
from generate_util import VOCAB, train_steps  # noqa: E402
from simple_distributed_machine_learning_amd.parallel.generate import generate, pad_prompts  # noqa: E402

BF = torch.bfloat16
PROMPTS = lu.rule_prompts([1, 2, 5, 17])


@pytest.fixture(scope="module")
def model():
    """block_size 192, 60 steps, as tests/test_lookup_generate_gpu.py trains it: bit equality does not need this model
    to be good."""
    return train_steps(lu.make_engine_d64("cuda:0", BF, 192), 60, 16, 32)


def test_sampled_across_the_chunk_edges(model):
    """8-token prompts, 150 new tokens: the rows grow across the 64- and 128-key edges; the prompt never fills a chunk,
    so every chunk here is per sibling (the whole prompt chunks: the 72-token prompts below)."""
    kw = dict(temperature=1.5, top_k=0, seed=5, return_lengths=True, return_stats=True)
    want = fu.repeated(generate, model, PROMPTS, 150, 3, **kw)
    groups = want[0].view(4, 3, -1)
    assert any(not torch.equal(groups[b, 0], groups[b, j]) for b in range(4) for j in (1, 2)), \
        "the siblings of the repeated call do not differ: raise the temperature"
    got = generate(model, PROMPTS, 150, num_samples=3, **kw)
    fu.same(got, want)
    assert got[0].shape == (12, 158) and got[1].tolist() == [158] * 12


def test_whole_prompt_chunks_are_shared(model):
    """72- and 130-token prompts: one and two whole 64-key chunks of the prompt are served once per group, the chunk
    that straddles the prompt's end is per sibling; sample0 shifts the sampler's sample index."""
    g = torch.Generator().manual_seed(11)
    for S0, new in ((72, 60), (130, 40)):
        prompts = torch.randint(0, VOCAB, (3, S0), generator=g)
        kw = dict(temperature=1.2, top_k=30, seed=9, sample0=4)
        fu.same(generate(model, prompts, new, num_samples=4, **kw), fu.repeated(generate, model, prompts, new, 4, **kw))


def test_greedy_siblings_are_the_plain_rows(model):
    plain = generate(model, PROMPTS, 70)
    got = generate(model, PROMPTS, 70, num_samples=3)
    assert torch.equal(got, plain.repeat_interleave(3, 0))


def test_ragged_prompts_top_p_eos_and_lengths(model):
    rows = [PROMPTS[0].tolist(), PROMPTS[1, :3].tolist(), PROMPTS[2, :7].tolist(), PROMPTS[3, :1].tolist()]
    rows.append(torch.arange(70).remainder(VOCAB).tolist())  # (a prompt with a whole chunk next to short ones)
    prompts, plens = pad_prompts(rows, 0)
    kw = dict(temperature=0.9, top_k=20, top_p=0.9, seed=5, prompt_lens=plens, eos_token=int(PROMPTS[0, 3]),
              pad_token=0, return_lengths=True, return_stats=True)
    want = fu.repeated(generate, model, prompts, 40, 2, **kw)
    for sc in (0, 4, 16):
        got = generate(model, prompts, 40, num_samples=2, stop_check=sc, **kw)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), sc  # stop_check does not change them
        fu.same(got, want if sc == 16 else fu.repeated(generate, model, prompts, 40, 2, stop_check=sc, **kw))
    assert got[0].shape == (10, 70 + 40) and got[1].shape == (10,)


def test_66_rows_leave_linear_decode(model):
    """22 prompts x 3 samples: the step's projections and the lm_head run 66 rows, beyond linear_decode's 64, in the
    forked call and in the repeated one alike; the prefill's lm_head too, though the prefill itself runs 22 rows."""
    prompts = lu.rule_prompts(range(1, 23))
    kw = dict(temperature=1.5, top_k=0, seed=5)
    fu.same(generate(model, prompts, 60, num_samples=3, **kw), fu.repeated(generate, model, prompts, 60, 3, **kw))


def test_refusals(model):
    for kw, msg in ((dict(num_samples=2, graph=True), "graph=True"), (dict(num_samples=2, lookup=2), "lookup > 0"),
                    (dict(num_samples=2, prefill_chunk=4), "prefill_chunk > 0"),
                    (dict(num_samples=0), "num_samples must be"), (dict(num_samples=65), "num_samples must be"),
                    (dict(num_samples=2.5), "num_samples must be")):
        with pytest.raises(ValueError, match=msg):
            generate(model, PROMPTS, 4, **kw)
