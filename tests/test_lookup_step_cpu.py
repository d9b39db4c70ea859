"""Prompt-lookup speculation's bookkeeping on the CPU: the torch twin of lookup_step (ops/reference.py, the definition
of csrc/kernels/lookup.hip) against draft + accept in plain Python integers (tests/lookup_util.py), every cell of the
state and of the results; and the sampler twin's keying with several rows per sample."""
import pytest
import torch

import lookup_util as lu
from simple_distributed_machine_learning_amd.ops import decode as dec
from simple_distributed_machine_learning_amd.ops import reference as ref


def test_python_drafts_by_hand():
    """The plain-Python side itself, on cases small enough to do by hand."""
    rep = [1, 2, 3, 1, 2, 4, 1, 2, 5, 1, 2]
    assert lu.py_drafts(rep, 2, 3, 30) == [5, 1, 2]  # starts 0, 3 and 6 match: the most recent wins
    assert lu.py_drafts(rep, 1, 7, 30) == [5, 1, 2]  # cut by the history's end
    assert lu.py_drafts(rep, 3, 3, 30) == []  # [5, 1, 2] did not occur before
    assert lu.py_drafts(rep, 2, 3, len(rep) + 2) == [5] and lu.py_drafts(rep, 2, 3, len(rep) + 1) == []
    assert lu.py_drafts([5], 1, 3, 30) == [] and lu.py_drafts([5, 5], 1, 3, 30) == [5]
    assert lu.py_drafts([1, 2, 3, 4], 2, 3, 30) == []
    # period 6, 8 tokens, 24 new: 4 tokens per step, the last step 3
    seq = [(3 * i) % 6 + 10 * (i % 6) for i in range(32)]
    assert lu.simulate_row_steps(seq, 8, 32, 3, 2) == 6 and lu.simulate_row_steps(seq, 8, 32, 1, 2) == 12
    assert lu.simulate_row_steps(list(range(32)), 8, 32, 3, 2) == 23  # nothing repeats: one token per step


@pytest.mark.parametrize("N", [1, 2, 3])
@pytest.mark.parametrize("K", [1, 3, 7])
def test_twin_equals_python_integers(K, N):
    before, after, tags, nq = lu.check_against_python(ref.lookup_step, K, N)
    by = {t: i for i, t in enumerate(tags)}
    emitted = lambda t: after[by[t]]["lens"] - before[by[t]]["lens"]  # noqa: E731
    assert emitted("no draft accepted") == 1 and emitted("partial acceptance") == 2
    assert emitted("full acceptance and the bonus token") == min(K, 3) + 1
    assert emitted("an eos in the middle of an accepted run") == 2  # the eos is kept, what follows it is not
    assert after[by["an eos in the middle of an accepted run"]]["done"] == 1
    assert emitted("an eos as the first token") == 1 and after[by["an eos as the first token"]]["done"] == 1
    assert emitted("accepted run cut by limit") == 2
    for t in ("a done row", "a full row"):
        assert after[by[t]] == before[by[t]] and nq[by[t]] == 0
    assert emitted("a row one short of full") == 1 and nq[by["a row one short of full"]] == 0
    # nothing to accept: only the drafts, and the situations really occur
    before, after, _, nq = lu.check_against_python(ref.lookup_step, K, N, accept=False)
    assert after == before
    assert nq[by["no match"]] == 1 and nq[by["history shorter than N + 1"]] == 1
    assert nq[by["several matches, the most recent wins"]] == (1 + min(K, 3) if N < 3 else 1)
    assert nq[by["drafts cut by limit (none left)"]] == 1 and nq[by["drafts cut by limit (one left)"]] == (2 if N < 3 else 1)
    assert nq[by["history of N + 1 equal tokens"]] == 2  # one token follows the match
    assert nq[by["drafts cut by the history's end"]] == 1 + min(K, N + 1)


def test_all_done_flag_and_dispatch():
    done_rows = [14, 15]  # "a done row", "a full row"
    _, _, tags, nq = lu.check_against_python(dec.lookup_step, 3, 2, subset=done_rows)
    assert tags == ["a done row", "a full row"] and nq == [0, 0]  # (the flag's value 1 is checked inside)
    lu.check_against_python(dec.lookup_step, 3, 2, subset=[0, 14])  # one live row: flag 0
    for k, n in ((0, 2), (8, 2), (3, 0), (3, 9)):
        with pytest.raises(ValueError, match="lookup_step"):
            lu.check_against_python(dec.lookup_step, k, n)


@pytest.mark.parametrize("temperature,top_k,top_p", [(0.0, 0, 1.0), (0.8, 0, 1.0), (1.1, 5, 1.0), (0.9, 20, 0.8)])
def test_sampler_keying_with_rows_per_sample(temperature, top_k, top_p):
    B, T, V, seed, sample0 = 3, 4, 97, 12345, 40
    g = torch.Generator().manual_seed(5)
    logits = (3.0 * torch.randn(B * T, 128, generator=g)).to(torch.bfloat16)
    lens = torch.tensor([8, 3, 17], dtype=torch.int32)
    pos = (lens[:, None] + torch.arange(1, T + 1, dtype=torch.int32)[None, :]).reshape(-1)
    got = dec.sample_step(logits, V, temperature, top_k, top_p, seed, sample0, pos, rows_per_sample=T)
    for b in range(B):
        for t in range(T):
            r = b * T + t
            one = dec.sample_step(logits[r:r + 1], V, temperature, top_k, top_p, seed, sample0 + b, pos[r:r + 1])
            assert int(got[r]) == int(one), (b, t)
            if top_p == 1.0:
                assert int(got[r]) == int(dec.sample_logits(logits[r:r + 1], V, temperature, top_k, seed, sample0 + b,
                                                            pos[r:r + 1]))
    if top_p == 1.0:
        assert torch.equal(got, dec.sample_logits(logits, V, temperature, top_k, seed, sample0, pos, rows_per_sample=T))
    # the default is one row per sample, as before
    plain = dec.sample_logits(logits, V, temperature, top_k, seed, sample0, pos)
    assert torch.equal(plain, dec.sample_logits(logits, V, temperature, top_k, seed, sample0, pos, rows_per_sample=1))
    for r in range(B * T):
        assert int(plain[r]) == int(dec.sample_logits(logits[r:r + 1], V, temperature, top_k, seed, sample0 + r,
                                                      pos[r:r + 1]))
    if temperature > 0:
        assert not torch.equal(plain, got[:B * T])  # (the keying matters)
    with pytest.raises(ValueError, match="rows_per_sample"):
        dec.sample_step(logits, V, temperature, top_k, top_p, seed, sample0, pos, rows_per_sample=0)
