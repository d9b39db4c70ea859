"""generate() with a repetition penalty, an n-gram ban and logprobs on the torch twins (gpt2_tiny): the ban's property,
the refusals, a session's two calls against one, and the knobs at their defaults."""
import pytest
import torch

from fork_util import same
from generate_util import VOCAB, make_engine
from simple_distributed_machine_learning_amd.parallel.generate import generate
from simple_distributed_machine_learning_amd.parallel.session import GenerationSession

PROMPTS = (torch.arange(3 * 6).view(3, 6) * 7 + 3) % VOCAB
PEN = {"repetition_penalty": 1.3, "no_repeat_ngram_size": 3}


@pytest.fixture(scope="module")
def engine():
    return make_engine("gpt2_tiny", "cpu", torch.float32)


@pytest.mark.parametrize("kw", [{}, {"temperature": 0.9, "top_k": 20, "seed": 5}, {"prefill_chunk": 4},
                                {"temperature": 0.9, "num_samples": 2}], ids=["greedy", "top_k", "chunked", "forked"])
def test_no_row_repeats_a_3_gram(engine, kw):
    tok, logp = generate(engine, PROMPTS, 24, return_logprobs=True, **PEN, **kw)
    for row in tok.tolist():
        grams = [tuple(row[i:i + 3]) for i in range(len(row) - 2)]
        assert len(set(grams)) == len(grams)
    assert logp.dtype == torch.float32 and logp.shape == tok.shape
    assert bool((logp[:, :6] == 0).all()) and bool((logp[:, 6:] < 0).all())


@pytest.mark.parametrize("kw,match", [
    ({"repetition_penalty": 0.0}, "repetition_penalty must be"), ({"repetition_penalty": float("inf")}, "finite"),
    ({"no_repeat_ngram_size": 9}, "0..8"), ({"no_repeat_ngram_size": -1}, "0..8"),
    ({"repetition_penalty": 1.3, "lookup": 2}, "lookup > 0"), ({"return_logprobs": True, "lookup": 2}, "lookup > 0"),
    ({"no_repeat_ngram_size": 2, "num_beams": 2}, "num_beams > 1")])
def test_refusals(engine, kw, match):
    with pytest.raises(ValueError, match=match):
        generate(engine, PROMPTS, 4, **kw)


def test_two_session_calls_equal_one_long_call(engine):
    kw = {"temperature": 0.9, "top_k": 20, **PEN}
    want = generate(engine, PROMPTS, 24, seed=5, return_lengths=True, return_logprobs=True, **kw)
    s = GenerationSession(engine, PROMPTS, 30, seed=5)
    s.generate(10, return_logprobs=True, **kw)
    same(s.generate(14, return_logprobs=True, **kw), want)


def test_knobs_at_their_defaults_change_nothing(engine):
    for kw in ({}, {"temperature": 0.9, "top_p": 0.8, "seed": 5}):
        same(generate(engine, PROMPTS, 12, repetition_penalty=1.0, no_repeat_ngram_size=0, **kw),
             generate(engine, PROMPTS, 12, **kw))
