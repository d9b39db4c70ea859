"""What the generation drivers (plain, stepped, lookup, forked, chunked; parallel/generate.py, parallel/session.py)
share and the other generation tests leave unpinned, on the CPU with gpt2_tiny: the form of the result under every
combination of ``return_lengths`` / ``return_stats``, ``max_new_tokens=0``, the host's reads per call, and the stages'
training flags after a driver that raised mid-loop."""
import os
import sys

import pytest
import torch

from generate_util import make_engine
from simple_distributed_machine_learning_amd import parallel
from simple_distributed_machine_learning_amd.ops import decode
from simple_distributed_machine_learning_amd.parallel.generate import generate
from simple_distributed_machine_learning_amd.parallel.session import GenerationSession

NEW = 9
PROMPTS = torch.tensor([[3, 14, 15, 92, 65, 35, 89, 79], [2, 71, 82, 81, 82, 84, 59, 4],
                        [1, 41, 42, 13, 56, 23, 73, 9]])
B, S0 = PROMPTS.shape
RAGGED_LENS = [8, 3, 5]  # (a list: the argument checks then read nothing back)
RAGGED = torch.where(torch.arange(S0)[None, :] < torch.tensor(RAGGED_LENS)[:, None], PROMPTS, 0)
DRIVER_FILES = {os.path.join(os.path.dirname(parallel.__file__), f)
                for f in ("generate.py", "decode_graph.py", "session.py", "gen_common.py")}


@pytest.fixture(scope="module")
def tiny():
    eng = make_engine("gpt2_tiny", "cpu", torch.float32)
    eng.eval()
    return eng


def drivers(eos):
    """The arguments that select each eager driver; the stepped ones get ``eos``."""
    return {"plain": dict(), "stepped": dict(eos_token=eos, prompt_lens=RAGGED_LENS), "lookup": dict(lookup=2),
            "forked": dict(num_samples=2), "chunked": dict(prefill_chunk=2)}


@pytest.fixture(scope="module")
def eos(tiny):
    """A token no driver draws from PROMPTS (the plain outputs are looked at), so that no row finishes early."""
    drawn = {0}
    for kw in drivers(None).values():
        drawn |= set(generate(tiny, RAGGED if "prompt_lens" in kw else PROMPTS, NEW, **kw).flatten().tolist())
    return min(set(range(97)) - drawn)


# ---- return forms ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["plain", "stepped", "lookup", "forked", "chunked"])
@pytest.mark.parametrize("new", [NEW, 0])
def test_return_forms(tiny, eos, name, new):
    kw = drivers(eos)[name]
    prompts, plens = (RAGGED, RAGGED_LENS) if "prompt_lens" in kw else (PROMPTS, [S0] * B)
    n = kw.get("num_samples", 1)
    tokens = generate(tiny, prompts, new, **kw)
    both = generate(tiny, prompts, new, return_lengths=True, return_stats=True, **kw)
    with_len = generate(tiny, prompts, new, return_lengths=True, **kw)
    with_stats = generate(tiny, prompts, new, return_stats=True, **kw)
    assert torch.is_tensor(tokens) and tokens.shape == (B * n, S0 + new) and tokens.dtype == torch.int64
    assert isinstance(both, tuple) and len(both) == 3  # (tokens, lengths, stats)
    assert isinstance(with_len, tuple) and len(with_len) == 2  # (tokens, lengths)
    assert isinstance(with_stats, tuple) and len(with_stats) == 2  # (tokens, stats)
    lengths = both[1]
    assert lengths.shape == (B * n,) and lengths.dtype == torch.int64
    for got in (both[0], with_len[0], with_stats[0]):
        assert torch.equal(got, tokens)
    assert torch.equal(with_len[1], lengths)
    for stats in (both[2], with_stats[1]):
        assert isinstance(stats, dict) and set(stats) == {"steps", "row_steps", "generated"}
        assert isinstance(stats["steps"], int)
        for k in ("row_steps", "generated"):
            assert stats[k].shape == (B * n,) and stats[k].dtype == torch.int64
        assert stats["steps"] == both[2]["steps"]
        assert all(torch.equal(stats[k], both[2][k]) for k in ("row_steps", "generated"))
    want_lens = torch.tensor(plens).repeat_interleave(n)
    assert torch.equal(both[2]["generated"], lengths - want_lens)
    if new == 0:
        assert torch.equal(tokens, prompts.repeat_interleave(n, 0)) and torch.equal(lengths, want_lens)
        assert both[2]["steps"] == 0 and not bool(both[2]["row_steps"].any()) and not bool(both[2]["generated"].any())
    else:  # (the eos is never drawn: every row runs to the end)
        assert torch.equal(lengths, want_lens + new)
        assert 1 <= both[2]["steps"] <= new - 1 if name == "lookup" else both[2]["steps"] == new


# ---- host reads per call ---------------------------------------------------------------------------------------------
@pytest.fixture
def reads(monkeypatch):
    """Counts of Tensor.item / Tensor.tolist calls made from the driver modules."""
    counts = {"item": 0, "tolist": 0}
    for name in counts:
        def counting(self, *a, _orig=getattr(torch.Tensor, name), _name=name, **k):
            if sys._getframe(1).f_code.co_filename in DRIVER_FILES:
                counts[_name] += 1
            return _orig(self, *a, **k)
        monkeypatch.setattr(torch.Tensor, name, counting)
    return counts


@pytest.mark.parametrize("name", ["plain", "forked", "chunked", "session"])
@pytest.mark.parametrize("c", [0, 1, 4, None], ids=["c0", "c1", "c4", "no_eos"])
def test_host_reads_of_the_step_loop(tiny, eos, reads, name, c):
    """The loop draws NEW tokens and asks after token t + 1 whether to stop when (t + 1) % c == 0 and t + 1 < NEW: at
    t + 1 = c, 2c, ... <= NEW - 1, which is floor((NEW - 1) / c) reads of one flag (8 for c = 1, 2 for c = 4), and
    none for c = 0 or without an eos. No row meets the eos, so no check ends the loop. A session reads its lengths and
    done flags back once at the end of a call, in one ``tolist``; the other drivers never call it."""
    kw = dict(stop_check=4) if c is None else dict(eos_token=eos, stop_check=c)
    if name == "session":
        s = GenerationSession(tiny, PROMPTS, S0 + NEW)
        reads.update(item=0, tolist=0)
        _, lengths = s.generate(NEW, **kw)
    else:
        kw.update(dict(plain={}, forked=dict(num_samples=2), chunked=dict(prefill_chunk=2))[name])
        reads.update(item=0, tolist=0)
        _, lengths = generate(tiny, PROMPTS, NEW, return_lengths=True, **kw)
    got = dict(reads)
    assert lengths.tolist() == [S0 + NEW] * len(lengths)
    assert got == {"item": (NEW - 1) // c if c else 0, "tolist": int(name in ("chunked", "session"))}


@pytest.mark.parametrize("c", [0, 1, 4])
def test_host_reads_of_the_lookup_loop(tiny, eos, reads, c):
    """The verify loop runs at most NEW - 1 steps and reads its flag (all rows done or full?) after step s when
    s % c == 0 and s < NEW - 1, with or without an eos. It ran ``steps`` steps, and a read that ended it was the last
    one, so it read at s = c, 2c, ... <= min(steps, NEW - 2): floor(min(steps, NEW - 2) / c) reads, none for c = 0."""
    reads.update(item=0, tolist=0)
    _, stats = generate(tiny, PROMPTS, NEW, lookup=2, stop_check=c, return_stats=True)
    got = dict(reads)
    assert 1 <= stats["steps"] <= NEW - 1
    assert got == {"item": min(stats["steps"], NEW - 2) // c if c else 0, "tolist": 0}


# ---- training flags --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["stepped", "lookup", "forked", "chunked"])
def test_training_flags_are_restored_after_a_raise(eos, name, monkeypatch):
    eng = make_engine("gpt2_tiny", "cpu", torch.float32)
    eng.stages[0].train()
    eng.stages[1].eval()
    calls = []

    def sample_step(*a, **k):
        assert not any(m.training for m in eng.stages.values())  # (the drivers run their stages in eval mode)
        calls.append(1)
        if len(calls) == 3:
            raise RuntimeError("raised mid-loop")
        return decode.sample_step(*a, **k)

    # (the sampler as the driver modules bind it)
    for mod in [m for k, m in sys.modules.items() if k.startswith(parallel.__name__ + ".")]:
        if hasattr(mod, "sample_step"):
            monkeypatch.setattr(mod, "sample_step", sample_step)
    kw = {k: v for k, v in drivers(eos)[name].items() if k != "prompt_lens"}
    with pytest.raises(RuntimeError, match="raised mid-loop"):
        generate(eng, PROMPTS, NEW, **dict(kw, eos_token=eos))  # (with an eos every driver samples through sample_step)
    assert len(calls) == 3
    assert eng.stages[0].training and not eng.stages[1].training
