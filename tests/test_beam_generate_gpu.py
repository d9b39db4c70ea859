"""generate(num_beams=K) on the real kernels against a reference driver written here: prefill + decode_step on the
K-fold repeated batch with a plain KVCache, re-parented with index_select, stepped with the same beam_step op, traced
back in Python. The fork's row has attention_decode's bits on the concatenated cache, so both drivers feed beam_step
the same logits: tokens, lengths and scores are equal bit for bit. The d = 64 config of tests/lookup_util.py with
block_size 192, trained as tests/test_fork_generate_gpu.py trains it."""
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no ROCm GPU", allow_module_level=True)

import lookup_util as lu  # noqa: E402
from generate_util import VOCAB, train_steps  # noqa: E402
from simple_distributed_machine_learning_amd.ops.decode import beam_score_budget, beam_step  # noqa: E402
from simple_distributed_machine_learning_amd.parallel.gen_common import eval_stages  # noqa: E402
from simple_distributed_machine_learning_amd.parallel.generate import generate, pad_prompts  # noqa: E402

PAD = 0


@pytest.fixture(scope="module")
def model():
    return train_steps(lu.make_engine_d64("cuda:0", torch.bfloat16, 192), 60, 16, 32)


@torch.no_grad()
def reference_beams(eng, prompts, plens, new, K, eos):
    """(tokens [B K, S0 + new], lengths, scores) best first per prompt, and every hypothesis' score recomputed in fp64
    from the logits this driver saw, with the budget of its steps."""
    stages = [eng.stages[s] for s in range(eng.P)]
    dev, (B, S0), R = eng.device, prompts.shape, prompts.shape[0] * K
    lens0 = (torch.full((B,), S0) if plens is None else plens).repeat_interleave(K).tolist()
    score = torch.tensor([0.0] + [-float("inf")] * (K - 1), device=dev).repeat(B)
    fin = glen = torch.zeros(R, dtype=torch.int32, device=dev)
    toks, pars, logps, lses = [], [], [], []
    with eval_stages(stages):
        caches = [m.new_cache(R, S0 + new) for m in stages]
        x = prompts.repeat_interleave(K, 0).to(dev)
        for m, c in zip(stages, caches):
            x = m.prefill(x, c, lens=None if plens is None else torch.tensor(lens0, dtype=torch.int32, device=dev))
        for t in range(new):
            tok, par, score, fin, glen, _ = beam_step(x, VOCAB, K, score, fin, glen, -1 if eos is None else eos, PAD)
            src = torch.arange(R, device=dev) // K * K + par
            lp = torch.log_softmax(x[:, :VOCAB].double(), 1)[src]
            logps.append(lp.gather(1, tok[:, None])[:, 0].tolist())
            lses.append(torch.logsumexp(x[:, :VOCAB].double(), 1)[src].tolist())
            toks.append(tok.tolist())
            pars.append(par.tolist())
            if t + 1 == new:
                break
            for c in caches:
                c.k, c.v = [k.index_select(0, src) for k in c.k], [v.index_select(0, src) for v in c.v]
            x = tok
            for m, c in zip(stages, caches):
                x = m.decode_step(x, c)
    out = torch.full((R, S0 + new), PAD, dtype=torch.int64)
    out[:, :S0] = prompts.repeat_interleave(K, 0)
    exact, budget = [0.0] * R, [0.0] * R
    for r in range(R):
        base, j, path = r // K * K, r % K, []
        for t in range(new - 1, -1, -1):
            path.append((t, base + j))
            j = pars[t][base + j]
        for t, row in reversed(path):
            if t < int(glen[r]):
                out[r, lens0[r] + t] = toks[t][row]
                budget[r] += beam_score_budget(VOCAB, abs(lses[t][row]), abs(exact[r]), abs(logps[t][row]))
                exact[r] += logps[t][row]
    order = torch.sort(score.view(B, K), dim=1, descending=True, stable=True).indices.cpu()
    rows = (torch.arange(B)[:, None] * K + order).reshape(R)
    pick = lambda v: [v[i] for i in rows.tolist()]  # noqa: E731
    return out[rows], (torch.tensor(lens0) + glen.cpu())[rows], score.cpu()[rows], pick(exact), pick(budget)


def cases(model, which):
    if which == "short":  # 8-token prompts, 70 new: the rows cross the 64-key edge on suffix chunks alone
        return 2, lu.rule_prompts([1, 2, 5]), None, 70, None
    g = torch.Generator().manual_seed(11)  # 72-token ragged prompts: a whole shared prompt chunk, the 128-key edge
    prompts, plens = pad_prompts([torch.randint(1, VOCAB, (n,), generator=g).tolist() for n in (72, 70, 65)], PAD)
    # the eos: what the search without one gives prompt 0's best hypothesis as its 10th token, so a row finishes early
    eos = int(reference_beams(model, prompts, plens, 60, 4, None)[0][0, 72 + 9])
    return 4, prompts, plens, 60, eos


@pytest.mark.parametrize("which", ["short", "ragged_eos"])
def test_beams_equal_the_reference_driver(model, which):
    K, prompts, plens, new, eos = cases(model, which)
    want_tok, want_len, want_score, exact, budget = reference_beams(model, prompts, plens, new, K, eos)
    if eos is not None:  # the case is about finished rows: some hypothesis ended early and rode along on the pad token
        assert bool((want_len < plens.repeat_interleave(K) + new).any()), "no hypothesis drew the eos"
    kw = dict(num_beams=K, prompt_lens=plens, eos_token=eos, pad_token=PAD)
    tok, lengths, scores = generate(model, prompts, new, return_beams=True, return_lengths=True, **kw)
    assert torch.equal(tok.cpu(), want_tok) and torch.equal(lengths.cpu(), want_len)
    assert torch.equal(scores.cpu(), want_score) and scores.dtype == torch.float32
    for r, (s, e, b) in enumerate(zip(scores.tolist(), exact, budget)):
        assert abs(s - e) <= b, (r, s, e, b)
    best, best_len = generate(model, prompts, new, return_lengths=True, **kw)
    assert torch.equal(best, tok[::K]) and torch.equal(best_len, lengths[::K])
    for sc in (0, 4):
        assert torch.equal(generate(model, prompts, new, return_beams=True, stop_check=sc, **kw)[0], tok), sc


def test_more_than_64_rows_are_refused_on_the_kernels(model):
    with pytest.raises(ValueError, match="at most 64"):
        generate(model, lu.rule_prompts(range(1, 10)), 4, num_beams=8)
