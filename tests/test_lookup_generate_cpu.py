"""Prompt-lookup speculation end to end on the CPU (the torch twins) with a trained gpt2_tiny: the tokens and lengths of
the plain loop in fewer steps, the step counts against a pure-Python simulation, the refusals, the command line.

CPU fp32 ``F.linear`` rows depend on the row count (rows differ bitwise between M = 1..24 and M = 64 on the torch build
this was written on), so bit-equal logits are not promised on the twins: the equality tests first require the plain
run's smallest top-1 / top-2 logit gap to exceed 1e-3, far above what the row count can move."""
import json
from types import SimpleNamespace

import pytest
import torch

import lookup_util as lu
from dist_util import run_ranks
from generate_util import make_engine, nocache_logits, rule_holds, train_steps
from simple_distributed_machine_learning_amd.parallel.generate import _check_lookup, generate
from simple_distributed_machine_learning_amd.utils.checkpoint import save_checkpoint

NEW = 24
PROMPTS = lu.rule_prompts([1, 2, 5, 17, 40, 96])


@pytest.fixture(scope="module")
def trained():
    """gpt2_tiny as tests/test_generate_cpu.py trains it: 2 stages in one process, fp32, AdamW lr 3e-3, seed 1, 100
    steps of 32 x 16 tokens."""
    return train_steps(make_engine("gpt2_tiny", "cpu", torch.float32), 100, 32, 16)


@pytest.fixture(scope="module")
def plain(trained):
    """The plain greedy run, shared and left unchanged: (tokens, lengths)."""
    return generate(trained, PROMPTS, NEW, return_lengths=True)


def test_the_plain_run_has_a_clear_top1(trained, plain):
    """The precondition of the equality tests, an assertion and not a skip."""
    out, lengths = plain
    assert lengths.tolist() == [8 + NEW] * len(PROMPTS) and bool(rule_holds(out).all())
    top2 = nocache_logits(trained, out)[:, 7:-1].float().topk(2, dim=-1).values
    gap = float((top2[..., 0] - top2[..., 1]).min())
    print(f"smallest top-1 / top-2 logit gap of the plain run: {gap:.4f}")
    assert gap > 1e-3


@pytest.mark.parametrize("K", [1, 3, 7])
def test_greedy_lookup_returns_the_plain_tokens_in_fewer_steps(trained, plain, K):
    out, lengths = plain
    got, glen, stats = generate(trained, PROMPTS, NEW, lookup=K, return_lengths=True, return_stats=True)
    assert torch.equal(got, out) and torch.equal(glen, lengths)
    want = lu.check_row_steps(got, glen, stats, [8] * len(PROMPTS), NEW, K, 2)
    # full drafts from the first verify step; the most recent match lies one period (6) back, so 6 tokens follow it
    assert want == [-(-(NEW - 1) // (min(K, 6) + 1))] * len(PROMPTS)
    assert stats["steps"] == 16  # the default stop_check: the host first looks after 16 steps, all rows are full by then


def test_the_six_step_figure_and_stop_check(trained, plain):
    out, lengths = plain
    res = {}
    for sc in (0, 1, 4):
        got, glen, stats = generate(trained, PROMPTS, NEW, lookup=3, lookup_ngram=2, stop_check=sc,
                                    return_lengths=True, return_stats=True)
        assert torch.equal(got, out) and torch.equal(glen, lengths), sc
        assert stats["row_steps"].tolist() == [6] * len(PROMPTS), sc  # ceil(23 / 4)
        lu.check_row_steps(got, glen, stats, [8] * len(PROMPTS), NEW, 3, 2)
        res[sc] = stats["steps"]
    assert res == {0: NEW - 1, 1: 6, 4: 8}  # the host's loop count is what stop_check changes
    # other n-gram lengths, a one-token prompt (nothing to look up at first) and no new tokens
    for n in (1, 3):
        got, glen, stats = generate(trained, PROMPTS, NEW, lookup=3, lookup_ngram=n, return_lengths=True,
                                    return_stats=True)
        assert torch.equal(got, out)
        lu.check_row_steps(got, glen, stats, [8] * len(PROMPTS), NEW, 3, n)
    p1 = PROMPTS[:, :1].contiguous()
    want1 = generate(trained, p1, 31)
    got1, len1, stats1 = generate(trained, p1, 31, lookup=3, stop_check=1, return_lengths=True, return_stats=True)
    assert torch.equal(got1, want1) and len1.tolist() == [32] * len(PROMPTS)
    steps1 = lu.check_row_steps(got1, len1, stats1, [1] * len(PROMPTS), 31, 3, 2)
    assert all(s < 30 for s in steps1)
    got0, stats0 = generate(trained, PROMPTS, 0, lookup=3, return_stats=True)
    assert torch.equal(got0, PROMPTS) and stats0["steps"] == 0


def test_ragged_prompts_and_an_eos(trained):
    from simple_distributed_machine_learning_amd.parallel.generate import pad_prompts

    rows = [PROMPTS[0].tolist(), PROMPTS[1, :3].tolist(), PROMPTS[2, :7].tolist(), PROMPTS[3, :1].tolist()]
    prompts, plens = pad_prompts(rows, 0)
    eos = int(PROMPTS[0, 3])  # row 0 meets it again after a few tokens: the period is 6
    kw = dict(prompt_lens=plens, eos_token=eos, pad_token=0, return_lengths=True)
    want, wlen = generate(trained, prompts, 20, **kw)
    assert int(wlen[0]) < 8 + 20, "the eos never came"
    for K, sc in ((1, 0), (3, 1), (7, 4)):
        got, glen, stats = generate(trained, prompts, 20, lookup=K, stop_check=sc, return_stats=True, **kw)
        assert torch.equal(got, want) and torch.equal(glen, wlen), K
        lu.check_row_steps(got, glen, stats, plens.tolist(), 20, K, 2, eos)


def test_lookup_0_is_todays_call(trained, plain):
    out, lengths = plain
    a = generate(trained, PROMPTS, NEW, lookup=0)
    assert isinstance(a, torch.Tensor) and torch.equal(a, out) and torch.equal(a, generate(trained, PROMPTS, NEW))
    b = generate(trained, PROMPTS, NEW, lookup=0, return_lengths=True)
    assert isinstance(b, tuple) and len(b) == 2 and torch.equal(b[0], out) and torch.equal(b[1], lengths)
    c = generate(trained, PROMPTS, NEW, lookup=0, return_stats=True)
    assert len(c) == 2 and torch.equal(c[0], out) and c[1]["steps"] == NEW
    assert c[1]["row_steps"].tolist() == [NEW] * len(PROMPTS) == c[1]["generated"].tolist()
    s = generate(trained, PROMPTS, NEW, temperature=0.9, top_k=20, seed=3)
    assert torch.equal(generate(trained, PROMPTS, NEW, temperature=0.9, top_k=20, seed=3, lookup=0), s)


def test_refusals(trained):
    for kw, msg in ((dict(lookup=-1), "lookup must be"), (dict(lookup=8), "lookup must be"),
                    (dict(lookup=1.5), "lookup must be"), (dict(lookup=3, lookup_ngram=0), "lookup_ngram"),
                    (dict(lookup=3, lookup_ngram=9), "lookup_ngram"), (dict(lookup_ngram=0), "lookup_ngram"),
                    (dict(lookup=3, graph=True), "graph=True")):
        with pytest.raises(ValueError, match=msg):
            generate(trained, PROMPTS, 4, **kw)
    # the kernel path's row bound (B * (K + 1) <= 64), on a stand-in for a ROCm bf16 engine with head width 64
    cfg = SimpleNamespace(n_embd=128, n_head=2)
    rocm = SimpleNamespace(mesh=SimpleNamespace(pp=1), device=torch.device("cuda", 0), dtype=torch.bfloat16)
    _check_lookup(rocm, cfg, 16, 3, 2, False)
    _check_lookup(rocm, cfg, 8, 7, 2, False)
    for B, K in ((17, 3), (9, 7), (33, 1)):
        with pytest.raises(ValueError, match="at most 64"):
            _check_lookup(rocm, cfg, B, K, 2, False)
    _check_lookup(SimpleNamespace(mesh=rocm.mesh, device=torch.device("cpu"), dtype=torch.float32), cfg, 97, 7, 2, False)
    # the model's entry point
    s0 = trained.stages[0]
    with pytest.raises(ValueError, match="T in 1..8"):
        s0.decode_block(torch.zeros(2, 9, dtype=torch.int64), s0.new_cache(2, 16), torch.ones(2, dtype=torch.int32))


@pytest.mark.slow
def test_two_ranks_refuse_lookup():
    res = run_ranks(lu.lookup_pp_refusal_worker, 2, "gpt2_tiny", torch.float32)
    assert all("pp=2 is not supported" in r for r in res), res


def test_command_line(trained, tmp_path, capsys):
    from simple_distributed_machine_learning_amd import generate as gen_cli

    save_checkpoint(trained, str(tmp_path / "ckpt"), 1, 0)
    common = ["--rank", "0", "--world_size", "1", "--interface", "lo", "--model", "gpt2_tiny", "--dtype", "fp32",
              "--device", "cpu", "--ckpt_dir", str(tmp_path / "ckpt"), "--max_new_tokens", str(NEW)]
    common += [a for row in PROMPTS[:3].tolist() for a in ("--prompt_tokens", ",".join(map(str, row)))]
    assert gen_cli.main(common) == 0
    want = [l for l in capsys.readouterr().out.splitlines() if l and l[0].isdigit()]
    mpath = tmp_path / "m.jsonl"
    assert gen_cli.main(common + ["--lookup", "3", "--lookup_ngram", "2", "--stop_check", "2",
                                  "--metrics", str(mpath)]) == 0
    got = [l for l in capsys.readouterr().out.splitlines() if l and l[0].isdigit()]
    assert got == want and len(got) == 3
    ev = [json.loads(l) for l in mpath.read_text().splitlines()]
    assert [e["event"] for e in ev] == ["generate"]
    assert ev[0]["lookup"] == 3 and ev[0]["lookup_ngram"] == 2 and ev[0]["steps"] == 6 and ev[0]["tokens"] == 3 * NEW
    assert ev[0]["tokens_per_step"] == 3 * NEW / 6
    for bad in (["--lookup", "8"], ["--lookup", "3", "--lookup_ngram", "0"]):
        with pytest.raises(SystemExit, match="lookup"):
            gen_cli.main(common + bad)
