"""Generation sessions and chunked prefill on the real kernels: the d = 64 config with block_size 192 trained on the
device (tests/lookup_util.py make_engine_d64). Two session calls against one long ``generate()`` bit for bit, 150-token
prompts through ``extend`` in chunks of 64 and 50 (across the 64- and 128-key tile edges) against a float64 forward of
the same bf16 weights, a session with appended tokens against a fresh call, and the cache invariant."""
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no ROCm GPU", allow_module_level=True)

import gpt2_numerics as gn  # noqa: E402
import lookup_util as lu  # noqa: E402
import session_util as su  # noqa: E402
from generate_util import VOCAB, nocache_logits, train_steps  # noqa: E402
from simple_distributed_machine_learning_amd.models.gpt2 import GPT2Stage  # noqa: E402
from simple_distributed_machine_learning_amd.parallel.generate import generate, pad_prompts  # noqa: E402
from simple_distributed_machine_learning_amd.parallel.session import GenerationSession  # noqa: E402

BF = torch.bfloat16
DEV = torch.device("cuda", 0)
PROMPTS = lu.rule_prompts([1, 2, 5, 17, 40, 63, 77, 96])
B = len(PROMPTS)
LONG = su.rule_rows([3, 8, 21, 34, 55, 60, 71, 90], 150)
EOS = int(PROMPTS[0, 3])


@pytest.fixture(scope="module")
def trained():
    """block_size 192, 60 AdamW steps of 16 x 32 tokens, as tests/test_lookup_generate_gpu.py trains it."""
    return train_steps(lu.make_engine_d64("cuda:0", BF, 192), 60, 16, 32)


@pytest.mark.parametrize("kw", [dict(), dict(temperature=0.9, top_k=20)], ids=["greedy", "sampled"])
def test_two_calls_return_the_bits_of_one_long_call(trained, kw):
    """The second call's catch-up is the decode_step the long call runs, so every bit is the long call's; 8 + 70 + 90
    tokens cross the decode attention's 64- and 128-key chunks."""
    a, b = 70, 90
    seed = 3 if kw else None
    want, wlen = generate(trained, PROMPTS, a + b, seed=seed, return_lengths=True, **kw)
    s = GenerationSession(trained, PROMPTS, 8 + a + b, seed=seed)
    first, _ = s.generate(a, **kw)
    assert torch.equal(first[:, :8 + a], want[:, :8 + a])
    su.check_invariant(s)
    got, glen = s.generate(b, **kw)
    assert torch.equal(got, want) and torch.equal(glen, wlen)
    su.check_invariant(s)


def test_two_calls_with_ragged_prompts_top_p_and_an_eos(trained):
    rows = [PROMPTS[0].tolist(), PROMPTS[1, :3].tolist(), PROMPTS[2, :7].tolist(), PROMPTS[3, :1].tolist()]
    prompts, plens = pad_prompts(rows, 0)
    a, b = 6, 60
    kw = dict(temperature=0.7, top_k=20, top_p=0.9, eos_token=EOS)
    want, wlen = generate(trained, prompts, a + b, seed=5, prompt_lens=plens, return_lengths=True, **kw)
    s = GenerationSession(trained, prompts, 8 + a + b, prompt_lens=plens, seed=5)
    s.generate(a, stop_check=2, **kw)
    print(f"done after the first call: {s.done.tolist()}, lengths {s.lengths.tolist()}")
    assert any(s.done.tolist()) and not all(s.done.tolist()), "the first call must end some rows and not all"
    su.check_invariant(s)  # rows that went done rode along in decode_step and were taken back
    got, glen = s.generate(b, **kw)
    assert torch.equal(got, want) and torch.equal(glen, wlen)
    su.check_invariant(s)
    assert bool((glen < plens.to(DEV) + a + b).any()), "no row drew the eos"


def _f64_logits(engine, seq):
    """float64 on the CPU, the same bf16 weights: logits [B, S, V]."""
    cfg = engine.stages[0].cfg
    x = seq.cpu()
    for s in range(engine.P):
        m64 = GPT2Stage(cfg, s, engine.P)
        m64.load_state_dict({k: v.detach().cpu() for k, v in engine.stages[s].state_dict().items()})
        with torch.no_grad():
            x = m64.double().eval()(x)
    return x


@pytest.fixture(scope="module")
def long_refs(trained):
    """For the 150-token prompts, computed once: the float64 logits, the training forward's, one-shot prefill's."""
    r64 = _f64_logits(trained, LONG)[..., :VOCAB]
    train = nocache_logits(trained, LONG.to(DEV))[..., :VOCAB].float().cpu()
    one = su.prefill_logits(trained, LONG)
    return r64, train, one


@pytest.mark.parametrize("chunk", [64, 50])
def test_chunked_prefill_logits_are_as_accurate_as_the_training_forward(trained, long_refs, chunk):
    """Every extend call on the last stage returns the logits of the chunk's last position: three positions per row,
    against float64, with the training forward's error at the same positions as the yardstick."""
    r64, train, one = long_refs
    caches = [trained.stages[s].new_cache(B, 150) for s in range(trained.P)]
    got, pos = [], []
    for c0 in range(0, 150, chunk):
        x = LONG[:, c0:c0 + chunk].contiguous().to(DEV)
        for s in range(trained.P):
            x = trained.stages[s].extend(x, caches[s])
        got.append(x)
        pos.append(min(c0 + chunk, 150) - 1)
    assert all(c.lens.tolist() == [150] * B and c.n == 150 for c in caches)
    same = torch.equal(got[-1], one)
    print(f"chunked prefill (chunks of {chunk}) equals one-shot prefill bit for bit at the last position: {same}")
    assert not bool(got[-1][..., VOCAB:].float().abs().max() > 0), "the pad columns of the logits must be zeros"
    got = torch.stack(got, 1)[..., :VOCAB].float().cpu()
    r, t = r64[:, pos], train[:, pos]
    row_c, row_t = (got.double() - r).abs().amax(-1), (t.double() - r).abs().amax(-1)
    rms_c, rms_t = gn._rms(got.double() - r), gn._rms(t.double() - r)
    print(f"NUMERICS chunked prefill {chunk} | logits | chunked rms {rms_c:.4g} train rms {rms_t:.4g} | "
          f"chunked worst row {float(row_c.max()):.4g} train worst row {float(row_t.max()):.4g}")
    assert rms_c <= gn.RMS_MARGIN * rms_t
    assert float(row_c.max()) <= gn.ROW_MARGIN * float(row_t.max())


def test_generate_with_prefill_chunk_returns_the_tokens_of_generate(trained):
    new = 20
    want, wlen = generate(trained, LONG, new, return_lengths=True)
    gap = su.min_gap(trained, want, wlen, [150] * B)
    print(f"smallest top-1 / top-2 logit gap of the one-shot run: {gap:.4f}")
    assert gap > 1e-3
    for chunk in (64, 50):
        got, glen = generate(trained, LONG, new, prefill_chunk=chunk, return_lengths=True)
        assert torch.equal(got, want) and torch.equal(glen, wlen), chunk


def test_append_then_continue_equals_a_fresh_call(trained):
    a, b = 60, 40
    s = GenerationSession(trained, PROMPTS, 8 + a + 7 + b)
    out, lens = s.generate(a, eos_token=EOS, stop_check=4)
    done = s.done.tolist()
    # a done row gets the next turn after its eos; of the live ones, the first gets 7 tokens and the others none
    live = [r for r in range(B) if not done[r]]
    n = [3 if done[r] else (7 if live and r == live[0] else 0) for r in range(B)]
    add = [su.rule_next(out[r, int(lens[r]) - 1], n[r]) for r in range(B)]
    s.append(add)
    got, glen = s.generate(b)
    su.check_invariant(s)
    rows = [r + x for r, x in zip(su.rows_of(out, lens), add)]
    fp, fl = pad_prompts(rows, 0)
    want, wlen = generate(trained, fp, b, prompt_lens=fl, return_lengths=True)
    gap = su.min_gap(trained, want, wlen, fl.tolist())
    print(f"done after the first call: {done}; smallest top-1 / top-2 logit gap of the fresh run: {gap:.4f}")
    assert gap > 1e-3
    assert su.rows_of(got, glen) == su.rows_of(want, wlen)
