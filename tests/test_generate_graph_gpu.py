"""generate(graph=True): one captured decode step (the one-launch kernels, the sampler, the token copy) replayed per
token must return the eager call's tokens and lengths bit for bit, in every sampling mode, across attention chunks, and
from a session that is reused."""
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no ROCm GPU", allow_module_level=True)

import ragged_generate_util as ru  # noqa: E402
from generate_util import VOCAB, make_engine, train_steps  # noqa: E402
from simple_distributed_machine_learning_amd.models.gpt2 import GPT2Config, gpt2_spec  # noqa: E402
from simple_distributed_machine_learning_amd.parallel import PipelineEngine, init_mesh  # noqa: E402
from simple_distributed_machine_learning_amd.parallel.generate import generate, pad_prompts  # noqa: E402

PROMPTS = torch.arange(VOCAB)[:, None]
BF = torch.bfloat16


@pytest.fixture(scope="module")
def trained():
    """GPT2Config(n_layer=2, n_head=2, n_embd=128, vocab_size=97, block_size=64), 2 stages, bf16, one process on the
    GPU: 200 AdamW steps (lr 3e-3) of 16 x 32 tokens."""
    return train_steps(make_engine("gpt2_d64", "cuda:0", BF), 200, 16, 32)


def test_graphed_greedy_and_top_k_equal_the_eager_call(trained):
    want = generate(trained, PROMPTS, 63)
    got = generate(trained, PROMPTS, 63, graph=True)
    assert got.shape == (97, 64) and got.is_cuda and torch.equal(got, want)
    assert trained.decode_session is not None and trained.stages[0].training is False
    kw = dict(temperature=0.9, top_k=20, seed=3)
    want_s = generate(trained, PROMPTS, 63, **kw)
    assert torch.equal(generate(trained, PROMPTS, 63, graph=True, **kw), want_s) and not torch.equal(want_s, want)


def test_graphed_ragged_top_p_eos_equals_the_eager_call(trained):
    """Prompts of lengths 1..5; rows 0, 2 and 4 lie on the eos's orbit of the rule (a 6-cycle) and meet it after 3, 5
    and 2 tokens, rows 1 and 3 lie on another orbit and never do. Tokens and lengths."""
    lens, new = [1, 2, 3, 4, 5], 31
    on, eos = ru.eos_prompts([1, 3, 5], [3, 5, 2])
    assert eos not in ru.rule_seq(1, 8)
    rows = [on[0], ru.rule_seq(1, 2), on[1], ru.rule_seq(1, 4), on[2]]
    p, plens = pad_prompts(rows, 0)
    kw = dict(prompt_lens=plens, temperature=0.8, top_p=0.9, seed=5, eos_token=eos, pad_token=96, stop_check=4,
              return_lengths=True)
    want, n = generate(trained, p, new, **kw)
    ended = [int(n[b]) < lens[b] + new for b in range(5)]
    assert any(ended) and not all(ended), f"the case must have rows that draw the eos and rows that do not: {n.tolist()}"
    got, m = generate(trained, p, new, graph=True, **kw)
    assert torch.equal(got, want) and torch.equal(m, n)
    # all rows end early: the stop check breaks out of the replay loop, the result is the same
    rows, eos = ru.eos_prompts(lens, [3, 5, 2, 6, 4])
    p, plens = pad_prompts(rows, 0)
    kw.update(prompt_lens=plens, eos_token=eos, temperature=0.0, top_p=1.0)
    want, n = generate(trained, p, new, **kw)
    got, m = generate(trained, p, new, graph=True, **kw)
    assert torch.equal(got, want) and torch.equal(m, n) and int(n.max()) < 5 + new


def test_graphed_generation_across_three_attention_chunks():
    """block_size 192, random weights, 8 one-token prompts, 191 tokens at temperature 1: 190 replays at fixed
    addresses while the rows grow through three 64-key chunks."""
    cfg = GPT2Config(n_layer=2, n_head=2, n_embd=128, vocab_size=VOCAB, block_size=192)
    mesh = init_mesh(pp=1, schedule_kind="1f1b", rank=0, world_size=1, device=torch.device("cuda", 0), backend=None,
                     timeout_s=120, transport=None)
    eng = PipelineEngine(gpt2_spec(2, cfg=cfg, seq_len=32, dtype=BF, name="gpt2_d64_192"), mesh,
                         schedule_kind="1f1b", num_microbatches=1, seed=1)
    p = torch.arange(8)[:, None] * 11
    kw = dict(temperature=1.0, seed=2)
    want = generate(eng, p, 191, **kw)
    got = generate(eng, p, 191, graph=True, **kw)
    assert want.shape == (8, 192) and torch.equal(got, want)
    assert len({tuple(r) for r in want.tolist()}) == 8  # (sampled rows, not one repeated sequence)
    assert eng.decode_graph_captures == 1


def test_a_session_is_reused_until_its_key_changes_and_reads_trained_weights_in_place(trained):
    trained.decode_session = None
    c0 = trained.decode_graph_captures
    kw = dict(temperature=0.9, top_k=20, seed=3)
    a = PROMPTS[:32]
    assert torch.equal(generate(trained, a, 40, graph=True, **kw), generate(trained, a, 40, **kw))
    assert trained.decode_graph_captures - c0 == 1
    b = PROMPTS[40:72]  # other prompts of the same shape: no capture
    got = generate(trained, b, 40, graph=True, sample0=0, **kw)
    assert trained.decode_graph_captures - c0 == 1
    assert torch.equal(got, generate(trained, b, 40, **kw))
    kw2 = dict(kw, top_k=10)  # another key: the session is replaced
    assert torch.equal(generate(trained, b, 40, graph=True, **kw2), generate(trained, b, 40, **kw2))
    assert trained.decode_graph_captures - c0 == 2
    before = trained.flat.params.clone()
    train_steps(trained, 5, 16, 32)  # the optimizer writes the weights in place: the captured step reads the new ones
    assert not torch.equal(trained.flat.params, before)
    assert torch.equal(generate(trained, b, 40, graph=True, **kw2), generate(trained, b, 40, **kw2))
    assert trained.decode_graph_captures - c0 == 2
