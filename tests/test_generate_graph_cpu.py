"""generate(graph=True) where no GPU is needed: the refusals, the fused decode step on the torch twins, the command
line."""
import pytest
import torch

from dist_util import run_ranks
from generate_graph_util import refused_worker
from generate_util import VOCAB, make_engine
from simple_distributed_machine_learning_amd.parallel.generate import generate

PROMPTS = torch.arange(VOCAB)[:, None]


@pytest.fixture(scope="module")
def tiny():
    return make_engine("gpt2_tiny", "cpu", torch.float32)


def test_graph_is_refused_on_a_cpu_engine(tiny):
    with pytest.raises(ValueError, match="ROCm device.*cpu"):
        generate(tiny, PROMPTS, 4, graph=True)
    with pytest.raises(ValueError, match="ROCm device"):  # also where nothing would be generated
        generate(tiny, PROMPTS, 0, graph=True)
    assert tiny.decode_graph_captures == 0 and tiny.decode_session is None
    assert generate(tiny, PROMPTS, 4, graph=False).shape == (97, 5)


@pytest.mark.slow
def test_graph_is_refused_on_a_two_rank_pipeline():
    res = run_ranks(refused_worker, 2, "gpt2_tiny", "cpu", torch.float32)
    for msg in res:
        assert msg is not None and "pp=2" in msg and "cross ranks" in msg, msg


def test_fused_decode_step_equals_the_plain_step_on_the_twins(tiny):
    """fused=True on CPU fp32 tensors: the twins ignore the counters, so the logits and the caches are equal."""
    s0, s1 = tiny.stages[0].eval(), tiny.stages[1].eval()
    B, S0, total = 5, 3, 12
    seq = torch.randint(0, VOCAB, (B, total), generator=torch.Generator().manual_seed(2))
    plain = [s0.new_cache(B, total), s1.new_cache(B, total)]
    fused = [s0.new_cache(B, total, fused=True), s1.new_cache(B, total, fused=True)]
    assert plain[0].tickets is None and fused[0].tickets.dtype == torch.int32
    assert fused[0].tickets.numel() % 4 == 0 and not bool(fused[0].tickets.any())
    for c in (plain, fused):
        s1.prefill(s0.prefill(seq[:, :S0], c[0]), c[1])
    for t in range(S0, total):
        want = s1.decode_step(s0.decode_step(seq[:, t], plain[0]), plain[1])
        got = s1.decode_step(s0.decode_step(seq[:, t], fused[0], fused=True), fused[1], fused=True)
        assert torch.equal(got, want)
    for p, f in zip(plain, fused):
        assert f.n == p.n == total and torch.equal(f.lens, p.lens)
        assert all(torch.equal(a, b) for a, b in zip(p.k + p.v, f.k + f.v))
        assert not bool(f.tickets.any())
    with pytest.raises(ValueError, match="fused=True"):
        s0.decode_step(seq[:, 0], s0.new_cache(B, total), fused=True)


def test_cli_parses_graph_and_refuses_it_on_the_cpu():
    from simple_distributed_machine_learning_amd import generate as gen_cli

    common = ["--rank", "0", "--world_size", "1", "--model", "gpt2_tiny", "--prompt_tokens", "1,2"]
    assert gen_cli.parse_args(common).graph is False
    assert gen_cli.parse_args(common + ["--graph"]).graph is True
    with pytest.raises(SystemExit, match="--graph.*ROCm device.*cpu"):
        gen_cli.main(common + ["--graph", "--device", "cpu"])
