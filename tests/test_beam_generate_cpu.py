"""Beam search on the CPU (the torch twins) with a trained gpt2_tiny: generate(num_beams=3) against a plain-Python
beam search over the model's full forward (no cache) under the same rule in fp64, num_beams=1, and the refusals."""
import math
from types import SimpleNamespace

import pytest
import torch

import lookup_util as lu
from generate_util import make_engine, nocache_logits, train_steps
from simple_distributed_machine_learning_amd.parallel.generate import generate

PROMPTS = lu.rule_prompts([1, 2, 5])
# The gap the Python search requires between a step's K + 1 best candidates, and the tolerance of the final scores.
# Not the step test's 8 E: the two sides here differ by more than the beam step's own error E (5e-6 at this
# vocabulary, ops.decode.beam_score_budget). One runs the cached decode path in fp32, the other the full forward in
# fp32 with the log-softmax in fp64; their fp32 logits come out of differently ordered sums and differ by a few ulps
# of values up to some tens, i.e. by some 1e-6 to 1e-5 per step, which 12 steps add up. 1e-4 is 20 E: room for both,
# and still below the gaps this trained model's candidates have (the test asserts them).
GAP = 1e-4


@pytest.fixture(scope="module")
def trained():
    return train_steps(make_engine("gpt2_tiny", "cpu", torch.float32), 100, 32, 16)


def python_beam_search(eng, prompt, new, K, eos, pad, min_gap):
    """Hypotheses (score, tokens, finished), best first, of one prompt (a list). Requires the K + 1 best candidates of
    every step to be ``min_gap`` apart or exactly equal: fp32 against fp64 may not decide an order."""
    beams = [(0.0, list(prompt), False)] + [(-math.inf, list(prompt), False)] * (K - 1)
    for _ in range(new):
        cands = []
        for j, (s, seq, done) in enumerate(beams):
            if done:
                cands.append((s, j, 0, seq + [pad], True))
                continue
            lp = torch.log_softmax(nocache_logits(eng, torch.tensor([[t for t in seq]]))[0, -1].double(), 0)
            top = torch.sort(lp, descending=True, stable=True).indices[:K].tolist()
            cands += [(s + float(lp[v]), j, i, seq + [v], v == eos) for i, v in enumerate(top)]
        cands.sort(key=lambda c: (-c[0], c[1], c[2]))
        for a, b in zip(cands[:K], cands[1:K + 1]):
            assert a[0] == b[0] or a[0] - b[0] >= min_gap, (a[0], b[0])
        beams = [(c[0], c[3], c[4]) for c in cands[:K]]
    return sorted(beams, key=lambda b: -b[0])  # (stable: the lowest beam first on ties)


def test_the_twin_driven_search_is_the_plain_python_search(trained):
    K, new, eos, pad = 3, 12, int(PROMPTS[0, 3]), 0
    tok, lengths, scores = generate(trained, PROMPTS, new, num_beams=K, eos_token=eos, pad_token=pad, return_beams=True,
                                    return_lengths=True)
    S0 = PROMPTS.shape[1]
    for b, prompt in enumerate(PROMPTS.tolist()):
        for j, (s, seq, _) in enumerate(python_beam_search(trained, prompt, new, K, eos, pad, GAP)):
            r = b * K + j
            n = seq.index(eos, S0) + 1 if eos in seq[S0:] else len(seq)
            assert tok[r].tolist() == seq[:n] + [pad] * (len(seq) - n) and int(lengths[r]) == n, (b, j)
            assert abs(float(scores[r]) - s) < GAP, (b, j, float(scores[r]), s)
    best = generate(trained, PROMPTS, new, num_beams=K, eos_token=eos, pad_token=pad)
    assert torch.equal(best, tok[::K])


def test_one_beam_is_the_call_without_the_argument(trained):
    kw = dict(temperature=0.8, top_k=10, seed=3, return_lengths=True)
    got, want = generate(trained, PROMPTS, 10, num_beams=1, **kw), generate(trained, PROMPTS, 10, **kw)
    assert all(torch.equal(a, b) for a, b in zip(got, want))


@pytest.mark.parametrize("kw,msg", [
    (dict(num_beams=0), "num_beams must be"), (dict(num_beams=9), "num_beams must be"),
    (dict(num_beams=2.0), "num_beams must be"), (dict(num_beams=2, temperature=0.7), "temperature > 0"),
    (dict(num_beams=2, top_k=5), "top_k > 0"), (dict(num_beams=2, top_p=0.9), "top_p in"),
    (dict(num_beams=2, num_samples=2), "num_samples > 1"), (dict(num_beams=2, graph=True), "graph=True"),
    (dict(num_beams=2, lookup=2), "lookup > 0"), (dict(num_beams=2, prefill_chunk=4), "prefill_chunk > 0"),
    (dict(num_beams=2, pp=2), "does not cross pipeline ranks")])
def test_refusals(trained, kw, msg):
    kw = dict(kw)
    mesh = SimpleNamespace(pp=kw.pop("pp", 1), tp=1, dp=1)  # (a stand-in engine: the check reads the mesh's pp only)
    eng = trained if mesh.pp == 1 else SimpleNamespace(mesh=mesh, kind=trained.kind, stages=trained.stages,
                                                       spec=trained.spec, device=trained.device, dtype=trained.dtype)
    with pytest.raises(ValueError, match=msg):
        generate(eng, PROMPTS, 4, **kw)
