"""Ragged prompts, stop tokens and top-p on the CPU (the torch twins): the nucleus rule in float64, the draws'
distribution, the margins that make the GPU tests' inputs unambiguous, and generate() on a trained gpt2_tiny: ragged
against alone, eos / pad / lengths, the stop check, teacher forcing through a ragged prefill, the refusals, the command
line and a two-process pipeline over Gloo."""
import json
import math

import numpy as np
import pytest
import torch

import ragged_generate_util as ru
from dist_util import run_ranks
from generate_util import VOCAB, make_engine, nocache_greedy, nocache_logits, rule_holds, train_steps
from simple_distributed_machine_learning_amd.models.gpt2 import GPT2Stage, dropout_seed
from simple_distributed_machine_learning_amd.ops import decode as dec
from simple_distributed_machine_learning_amd.ops import reference as ref
from simple_distributed_machine_learning_amd.parallel.generate import generate, pad_prompts
from simple_distributed_machine_learning_amd.utils.checkpoint import save_checkpoint

PROMPTS = torch.arange(VOCAB)[:, None]
LENS = [1, 5, 2, 9]
RAGGED = [ru.rule_seq(s, n) for s, n in zip((3, 40, 77, 11), LENS)]
SAMPLED = dict(temperature=0.9, top_k=20, top_p=0.9, seed=3)


# ---- 1. the rule, exactly --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,V", [(5, 97), (4, 50257)])
def test_top_p_candidates_equal_a_plain_sort_and_cumsum(B, V):
    z = ru.sampler_logits(B, V, V, seed=V)
    z[1, 3] = math.nan
    for T, k, p in ru.CASES + [(1.3, 7, 0.3), (0.7, 1, 0.9)]:
        cand, theta, _ = ru.nucleus64(z, k, p, T)
        got = ref.top_p_candidates(z, k, p, T)
        assert torch.equal(got, cand), (T, k, p)
        assert torch.equal(ref.top_p_threshold(z, k, p, T), theta), (T, k, p)
        assert not bool(got[1, 3]), "a NaN logit among the candidates"
        assert bool((got <= ref.top_k_candidates(z, k)).all()), "the nucleus left the top-k candidates"
        zr = torch.nan_to_num(z.float(), nan=-math.inf)
        assert bool(got[zr == zr.amax(1, keepdim=True)].all()), "a maximal logit outside the nucleus"


def test_top_p_keeps_boundary_ties_and_a_dominant_token_stands_alone():
    z = torch.full((3, 8), -2.0)
    z[0, 2] = 12.0  # one dominant token: e^-14 each for the others
    z[1, :] = torch.tensor([3.0, 1.0, 1.0, 1.0, 1.0, 0.0, -1.0, -5.0])  # 3.0 holds 0.621 at T = 1; the 1.0s tie
    z[2, :] = 0.5  # all equal
    c = ref.top_p_candidates(z, 0, 0.9, 1.0)
    assert c[0].tolist() == [False, False, True] + [False] * 5
    assert c[1].tolist() == [True] * 5 + [False] * 3  # 0.621 + one 1.0 (0.084) < 0.9: the boundary value's ties all stay
    assert bool(c[2].all())
    assert ref.top_p_candidates(z, 0, 0.5, 1.0)[1].tolist() == [True] + [False] * 7
    # temperature applies before top-p: at T = 4 the first token alone holds less than a half
    assert int(ref.top_p_candidates(z, 0, 0.5, 4.0)[1].sum()) > 1
    # top-k first: with k = 1 there is nothing left to cut
    assert ref.top_p_candidates(z, 1, 0.99, 1.0)[1].tolist() == [True] + [False] * 7


def test_top_p_off_is_top_k_and_nans_are_excluded():
    z = ru.sampler_logits(5, 97, 97, seed=97)
    z[0, 5], z[2, 96] = math.nan, math.nan
    pos = torch.arange(5, dtype=torch.int32) * 3
    for k in (0, 5, 97):
        for p in (0.0, 1.0):
            assert torch.equal(ref.top_p_candidates(z, k, p, 0.8), ref.top_k_candidates(z, k))
            assert torch.equal(ref.sample_step(z, 97, 0.8, k, p, 9, 2, pos), ref.sample_logits(z, 97, 0.8, k, 9, 2, pos))
        assert torch.equal(ref.top_p_candidates(z, k, 0.9, 0.0), ref.top_k_candidates(z, k))  # greedy ignores top_p
        assert torch.equal(ref.sample_step(z, 97, 0.0, k, 0.9, 9, 2, pos), ref.sample_logits(z, 97, 0.0, k, 9, 2, pos))
        c = ref.top_p_candidates(z, k, 0.9, 0.8)
        assert not bool(c[0, 5]) and not bool(c[2, 96])
    assert torch.equal(dec.sample_step(z, 97, 0.8, 5, 0.9, 9, 2, pos), ref.sample_step(z, 97, 0.8, 5, 0.9, 9, 2, pos))


def test_sample_step_bookkeeping_twin():
    V, W = 97, 6
    z = ru.sampler_logits(5, V, V, seed=1)
    z[1, 11] = 30.0  # row 1 draws the eos
    pos = torch.tensor([2, 3, W - 1, W, 0], dtype=torch.int32)  # row 3: outside the matrix
    out = torch.full((5, W), 7, dtype=torch.int64)
    done = torch.tensor([0, 0, 0, 0, 1], dtype=torch.int32)  # row 4: done before
    n = torch.tensor([1, 2, 3, 4, 5], dtype=torch.int32)
    tok = ref.sample_step(z, V, 0.8, 0, 0.9, 5, 0, pos, out, done, n, eos=11, pad=96)
    free = ref.sample_step(z, V, 0.8, 0, 0.9, 5, 0, pos)
    assert tok.tolist() == free[:4].tolist() + [96] and int(tok[1]) == 11
    want = torch.full((5, W), 7, dtype=torch.int64)
    want[0, 2], want[1, 3], want[2, W - 1] = tok[0], 11, tok[2]
    assert torch.equal(out, want)
    assert done.tolist() == [0, 1, 0, 0, 1] and n.tolist() == [2, 3, 4, 4, 5]


# ---- 2. the distribution over the nucleus ----------------------------------------------------------------------------
def _chi2_999(df):
    try:
        from scipy.stats import chi2

        return float(chi2.ppf(0.999, df))
    except ImportError:  # Wilson-Hilferty
        return df * (1 - 2 / (9 * df) + 3.090232 * math.sqrt(2 / (9 * df))) ** 3


@pytest.mark.parametrize("V,T,top_k,top_p", [(16, 2.0, 0, 0.9), (16, 2.0, 6, 0.8), (97, 1.3, 0, 0.95)])
def test_sample_step_distribution_chi_square(V, T, top_k, top_p):
    """65,536 draws (samples 0..65535, positions cycling through 0..1023, seed 1) of one logits row against the
    nucleus' softmax."""
    l32 = (2.0 * np.random.default_rng(3).standard_normal(V)).astype(np.float32)
    logits = torch.from_numpy((l32.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32).copy())  # bf16 values
    n = 65536
    z = logits[None, :].expand(n, V)
    tok = ref.sample_step(z, V, T, top_k, top_p, dropout_seed(1), 0, (torch.arange(n) % 1024).to(torch.int32))
    c, _, _ = ru.nucleus64(logits[None, :], top_k, top_p, T)
    c = c[0]
    df = int(c.sum()) - 1
    assert 1 <= df < (top_k or V) - 1, "the case must cut the candidates and leave more than one"
    assert bool(c[tok].all()), "a draw outside the nucleus"
    p = torch.softmax(torch.where(c, logits.double() / T, torch.tensor(-math.inf, dtype=torch.float64)), 0)
    cnt = torch.bincount(tok, minlength=V).double()
    e = p * n
    chi2 = float((((cnt - e) ** 2)[c] / e[c]).sum())
    print(f"chi2 V={V} T={T} top_k={top_k} top_p={top_p}: {chi2:.2f} (df {df}, 0.999 quantile {_chi2_999(df):.1f})")
    assert chi2 < _chi2_999(df)


# ---- 3. the GPU tests' sampler inputs are unambiguous -----------------------------------------------------------------
@pytest.mark.parametrize("name", list(ru.SAMPLER_SETS))
def test_gpu_sampler_inputs_keep_their_margin_to_top_p(name):
    """Every row's nearest cumulative mass fraction is further than 4 delta from top_p (docs/NUMERICS.md: the kernel's
    fraction is within delta of the exact one), so the kernel's threshold must be the float64 one."""
    B, V, ld = ru.SAMPLER_SETS[name]
    z = ru.sampler_logits(B, V, ld, seed=V)[:, :V]
    worst = (math.inf, None)
    for T, k, p in ru.CASES:
        m = float(ru.nucleus64(z, k, p, T)[2].min())
        worst = min(worst, (m, (T, k, p)))
        assert m > 4 * ru.delta(V), (T, k, p, m)
    print(f"NUMERICS top-p margin V={V}: smallest {worst[0]:.3g} at (T, top_k, top_p) = {worst[1]}, "
          f"4 delta = {4 * ru.delta(V):.3g}")


# ---- 4. generate on a trained gpt2_tiny --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def trained():
    """gpt2_tiny, 2 stages in one process, fp32, AdamW lr 3e-3, seed 1, 100 steps of 32 x 16 tokens."""
    return train_steps(make_engine("gpt2_tiny", "cpu", torch.float32), 100, 32, 16)


@pytest.mark.parametrize("kw", [{}, SAMPLED], ids=["greedy", "sampled"])
def test_a_ragged_row_equals_its_prompt_alone(trained, kw):
    new = 20
    p, lens = pad_prompts(RAGGED, 0)
    assert p.shape == (4, 9) and lens.tolist() == LENS and lens.dtype == torch.int32
    out, n = generate(trained, p, new, prompt_lens=lens, pad_token=96, return_lengths=True, **kw)
    assert out.shape == (4, 9 + new) and out.dtype == torch.int64
    assert n.tolist() == [l + new for l in LENS]
    assert torch.equal(out, generate(trained, p, new, prompt_lens=LENS, pad_token=96, **kw))  # a list of lengths
    for b, row in enumerate(RAGGED):
        alone = generate(trained, [row], new, sample0=b, **kw)
        assert torch.equal(out[b, :LENS[b] + new], alone[0]), b
        assert bool((out[b, LENS[b] + new:] == 96).all()), b
        ok = rule_holds(out[b:b + 1, :LENS[b] + new])
        if not kw:  # greedy follows the rule; a draw at T = 0.9 may leave it and is held to the row alone only
            assert bool(ok.all()), f"row {b}: {int(ok.sum())} of {ok.numel()} transitions obey the rule"


def test_eos_pads_the_rest_and_the_stop_check_changes_nothing(trained, monkeypatch):
    steps, new = [3, 5, 2, 6], 20
    rows, eos = ru.eos_prompts(LENS, steps)
    p, lens = pad_prompts(rows, 0)
    free = generate(trained, p, new, prompt_lens=lens, pad_token=95)
    calls = []
    step = GPT2Stage.decode_step
    monkeypatch.setattr(GPT2Stage, "decode_step", lambda self, x, cache: (calls.append(self.stage_id), step(self, x, cache))[1])
    res = {}
    for check in (0, 1, 16):
        calls.clear()
        res[check] = generate(trained, p, new, prompt_lens=lens, eos_token=eos, pad_token=95, stop_check=check,
                              return_lengths=True)
        res[check] += (len(calls),)
    out, n, _ = res[0]
    assert n.tolist() == [l + s for l, s in zip(LENS, steps)]
    for b in range(4):
        assert torch.equal(out[b, :int(n[b])], free[b, :int(n[b])]), b  # up to and including the eos
        assert int(out[b, int(n[b]) - 1]) == eos and eos not in out[b, LENS[b]:int(n[b]) - 1].tolist()
        assert bool((out[b, int(n[b]):] == 95).all()), b
    for check in (1, 16):
        assert torch.equal(res[check][0], out) and torch.equal(res[check][1], n), check
    # the loop really ends: all rows are done after 6 tokens (prefill + 5 decode steps of 2 stages)
    assert [res[c][2] for c in (0, 1, 16)] == [2 * (new - 1), 2 * 5, 2 * 15]


def test_ragged_prefill_and_decode_logits_match_the_full_forward(trained):
    """Teacher forcing through prefill(lens=...) + decode_step: each row's logits at its own positions against the
    training forward's."""
    lens = [3, 7, 1, 6]
    seq = nocache_greedy(trained, PROMPTS[[5, 30, 60, 90]], 31)
    want = nocache_logits(trained, seq)
    s0, s1 = trained.stages[0], trained.stages[1]
    c0, c1 = s0.new_cache(4, 32), s1.new_cache(4, 32)
    x = torch.stack([torch.where(torch.arange(7) < n, seq[b, :7], torch.tensor(0)) for b, n in enumerate(lens)])
    ld = torch.tensor(lens, dtype=torch.int32)
    got = [s1.prefill(s0.prefill(x, c0, lens=ld), c1, lens=ld)]
    assert c0.n == 7 and c1.n == 7 and c0.lens.tolist() == lens and c1.lens.tolist() == lens
    rows = torch.arange(4)
    steps = 32 - 7
    for t in range(steps):
        tok = seq[rows, ld.long() + t]
        got.append(s1.decode_step(s0.decode_step(tok, c0), c1))
    assert c0.n == 32 and c1.lens.tolist() == [n + steps for n in lens]
    got = torch.stack(got, 1)  # [4, 26, V]: row b, entry t is position lens[b] - 1 + t
    idx = (ld.long()[:, None] - 1 + torch.arange(steps + 1)[None, :])
    torch.testing.assert_close(got, want[rows[:, None], idx], rtol=1e-4, atol=1e-4)


def test_new_refusals(trained):
    p, lens = pad_prompts(RAGGED, 0)
    for bad in (-0.1, 1.5):
        with pytest.raises(ValueError, match="top_p"):
            generate(trained, PROMPTS, 4, temperature=1.0, top_p=bad)
    for bad in ([1, 5, 2, 10], [0, 5, 2, 9], [1, 5, 2]):
        with pytest.raises(ValueError, match="prompt_lens"):
            generate(trained, p, 4, prompt_lens=bad)
    for bad in (-1, VOCAB):
        with pytest.raises(ValueError, match="eos_token"):
            generate(trained, PROMPTS, 4, eos_token=bad)
        with pytest.raises(ValueError, match="pad_token"):
            generate(trained, PROMPTS, 4, eos_token=3, pad_token=bad)
    with pytest.raises(ValueError, match="stop_check"):
        generate(trained, PROMPTS, 4, eos_token=3, stop_check=-1)
    with pytest.raises(ValueError, match="block_size"):
        generate(trained, p, 24, prompt_lens=lens)  # Lmax + max_new_tokens, not a row's own length
    with pytest.raises(ValueError, match="at least one token"):
        pad_prompts([[1], []])


def test_old_paths_are_unchanged(trained):
    with pytest.raises(ValueError, match="unequal lengths"):
        generate(trained, [[1, 2], [3]], 4)
    with pytest.raises(ValueError, match="unequal lengths"):
        generate(trained, RAGGED, 4, eos_token=3)  # lists of unequal lengths go through pad_prompts
    # without the new arguments: the tokens of the loop as it was (prefill, decode_step, sample_logits, a column store)
    s0, s1 = trained.stages[0], trained.stages[1]
    for T, k in ((0.0, 0), (0.9, 20)):
        c0, c1 = s0.new_cache(VOCAB, 16), s1.new_cache(VOCAB, 16)
        want = torch.empty((VOCAB, 16), dtype=torch.int64)
        want[:, :1] = PROMPTS
        tok = None
        for t in range(15):
            z = s1.prefill(s0.prefill(PROMPTS, c0), c1) if t == 0 else s1.decode_step(s0.decode_step(tok, c0), c1)
            tok = ref.sample_logits(z, VOCAB, T, k, dropout_seed(3), 0, c1.lens)
            want[:, 1 + t] = tok
        got, n = generate(trained, PROMPTS, 15, temperature=T, top_k=k, seed=3, return_lengths=True)
        assert torch.equal(got, want) and n.tolist() == [16] * VOCAB
        # the step path draws the same tokens when nothing cuts and nothing stops
        assert torch.equal(generate(trained, PROMPTS, 15, temperature=T, top_k=k, seed=3, prompt_lens=[1] * VOCAB), want)


# ---- 5. the command line ---------------------------------------------------------------------------------------------
def test_cli_ragged_eos_top_p(trained, tmp_path, capsys):
    from simple_distributed_machine_learning_amd import generate as gen_cli

    save_checkpoint(trained, str(tmp_path / "ckpt"), 1, 0)
    steps = [3, 5, 2, 6]
    rows, eos = ru.eos_prompts(LENS, steps)
    common = ["--rank", "0", "--world_size", "1", "--interface", "lo", "--model", "gpt2_tiny", "--dtype", "fp32",
              "--device", "cpu", "--ckpt_dir", str(tmp_path / "ckpt"), "--max_new_tokens", "12"]
    prompts = [a for r in rows for a in ("--prompt_tokens", ",".join(map(str, r)))]
    mpath = tmp_path / "m.jsonl"
    assert gen_cli.main(common + prompts + ["--ragged", "--eos_token", str(eos), "--top_p", "0.9", "--temperature",
                                            "0.5", "--pad_token", "1", "--stop_check", "4", "--metrics", str(mpath)]) == 0
    lines = [[int(t) for t in l.split(",")] for l in capsys.readouterr().out.splitlines() if l and l[0].isdigit()]
    assert len(lines) == 4
    for b, l in enumerate(lines):
        assert l[:LENS[b]] == rows[b] and l[-1] == eos and 2 <= len(l) - LENS[b] <= 12, (b, l)
    ev = [json.loads(l) for l in mpath.read_text().splitlines()]
    assert [e["event"] for e in ev] == ["generate"] and ev[0]["top_p"] == 0.9
    assert ev[0]["tokens"] == sum(len(l) for l in lines) - sum(LENS)
    with pytest.raises(SystemExit, match="top_p"):
        gen_cli.main(common + prompts + ["--ragged", "--top_p", "2"])
    with pytest.raises(SystemExit):  # unequal lengths still need the flag
        gen_cli.main(common + prompts)


# ---- 6. two processes over Gloo --------------------------------------------------------------------------------------
@pytest.mark.slow
def test_two_process_pipeline_returns_the_single_process_ragged_result(trained, tmp_path):
    save_checkpoint(trained, str(tmp_path), 1, 0)
    rows, eos = ru.eos_prompts(LENS, [3, 5, 2, 6])
    p, lens = pad_prompts(rows, 0)
    for kw in (dict(stop_check=2), dict(stop_check=0, **SAMPLED)):
        want, n = generate(trained, p, 20, prompt_lens=lens, eos_token=eos, return_lengths=True, **kw)
        res = run_ranks(ru.ragged_worker, 2, "gpt2_tiny", "cpu", torch.float32, str(tmp_path), None, rows, 20, eos, kw)
        assert [r["stages"] for r in res] == [[0], [1]]
        for r in res:
            assert torch.equal(r["tokens"], want) and torch.equal(r["lengths"], n)
