"""Generation sessions and chunked prefill on the CPU (the torch twins) with a trained gpt2_tiny: the extend-attention
twin against the append twin and a float64 masked softmax, two session calls against one long ``generate()``, a session
with appended tokens against a fresh call on the concatenated rows, ``extend`` in chunks against one-shot ``prefill``,
the cache invariant, the refusals and the command line.

CPU fp32 ``F.linear`` rows depend on the row count, so where two runs process a position in passes of different shapes
the tokens are compared only after the fresh run's smallest top-1 / top-2 logit gap is shown to exceed 1e-3 (as
tests/test_lookup_generate_cpu.py does). Two session calls against one long call need no such condition: the second
call's catch-up is the ``decode_step`` the long call runs."""
import math

import pytest
import torch

import lookup_util as lu
import session_util as su
from generate_util import make_engine, rule_holds, train_steps
from simple_distributed_machine_learning_amd.ops import decode as dec
from simple_distributed_machine_learning_amd.parallel.generate import generate, pad_prompts
from simple_distributed_machine_learning_amd.parallel.session import GenerationSession
from simple_distributed_machine_learning_amd.utils.checkpoint import save_checkpoint

PROMPTS = lu.rule_prompts([1, 2, 5, 17, 40, 96])
B = len(PROMPTS)
RAGGED = [PROMPTS[0].tolist(), PROMPTS[1, :3].tolist(), PROMPTS[2, :7].tolist(), PROMPTS[3, :1].tolist()]
EOS = int(PROMPTS[0, 3])  # row 0 meets it again after a few tokens: the rule's period is 6


@pytest.fixture(scope="module")
def trained():
    """gpt2_tiny as tests/test_generate_cpu.py trains it: 2 stages in one process, fp32, AdamW lr 3e-3, seed 1, 100
    steps of 32 x 16 tokens."""
    return train_steps(make_engine("gpt2_tiny", "cpu", torch.float32), 100, 32, 16)


# ---- the twin ------------------------------------------------------------------------------------------------------
def twin_case(T, seed):
    g = torch.Generator().manual_seed(seed)
    Bt, H, D, S = 3, 2, 8, 24
    qkv = torch.randn(Bt, T, 3 * H * D, generator=g)
    k, v = torch.randn(Bt, S, H, D, generator=g), torch.randn(Bt, S, H, D, generator=g)
    lens = torch.tensor([0, 5, 13], dtype=torch.int32)
    nq = torch.tensor([T, 0, max(1, T // 2)], dtype=torch.int32)
    for b in range(Bt):
        k[b, int(lens[b]):] = math.nan
        v[b, int(lens[b]):] = math.nan
    return qkv, k, v, lens, nq, H, S


@pytest.mark.parametrize("T", [1, 2, 5, 8])
def test_the_twin_is_the_append_twin_up_to_8_positions(T):
    qkv, k, v, lens, nq, H, S = twin_case(T, T)
    k2, v2 = k.clone(), v.clone()
    got = dec.attention_extend(qkv, k, v, lens, nq, H, S)
    want = dec.attention_append_ref(qkv, k2, v2, lens, nq, H, S)
    torch.testing.assert_close(got, want, rtol=1e-5, atol=1e-6)
    assert torch.equal(torch.nan_to_num(k, nan=7.0), torch.nan_to_num(k2, nan=7.0))
    assert torch.equal(torch.nan_to_num(v, nan=7.0), torch.nan_to_num(v2, nan=7.0))
    assert lens.tolist() == [0, 5, 13]


@pytest.mark.parametrize("T", [1, 11])
def test_the_twin_against_a_float64_masked_softmax(T):
    qkv, k, v, lens, nq, H, S = twin_case(T, 100 + T)
    k0, v0 = k.clone(), v.clone()
    n_keys = 20  # sample 2 (lens 13): positions at rows >= 20 are dead
    got = dec.attention_extend(qkv, k, v, lens, nq, H, n_keys)
    C, D = qkv.shape[2] // 3, k.shape[-1]
    for b in range(qkv.shape[0]):
        ln = int(lens[b])
        n = max(0, min(int(nq[b]), n_keys - ln))
        K64, V64 = k0[b].double().clone(), v0[b].double().clone()
        K64[ln:ln + n] = qkv[b, :n, C:2 * C].double().view(n, H, D)
        V64[ln:ln + n] = qkv[b, :n, 2 * C:].double().view(n, H, D)
        assert torch.equal(k[b, :ln + n].double(), K64[:ln + n]) and bool(torch.isnan(k[b, ln + n:]).all())
        assert torch.equal(v[b, :ln + n].double(), V64[:ln + n]) and bool(torch.isnan(v[b, ln + n:]).all())
        for t in range(T):
            if t >= n:
                assert not bool(got[b, t].any())
                continue
            q = qkv[b, t, :C].double().view(H, D)
            s = torch.einsum("hd,shd->hs", q, K64[:ln + t + 1]) / math.sqrt(D)
            y = torch.einsum("hs,shd->hd", torch.softmax(s, -1), V64[:ln + t + 1]).reshape(C)
            torch.testing.assert_close(got[b, t].double(), y, rtol=1e-5, atol=1e-6)


def test_the_twin_refuses_bad_arguments():
    qkv, k, v, lens, nq, H, S = twin_case(3, 9)
    k0 = k.clone()
    for args in ((qkv, k, v, lens, nq, H, 0), (qkv, k, v, lens, nq, H, S + 1), (qkv, k, v, lens.long(), nq, H, S),
                 (qkv, k, v, lens, nq[:2], H, S), (qkv.double(), k, v, lens, nq, H, S),
                 (qkv[:, :, 1:], k, v, lens, nq, H, S), (qkv[:, :0], k, v, lens, nq, H, S),
                 (qkv, k, v[:, :5], lens, nq, H, S)):
        with pytest.raises(ValueError, match="attention_extend"):
            dec.attention_extend(*args)
    assert torch.equal(torch.nan_to_num(k), torch.nan_to_num(k0))


# ---- two calls are one long call --------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(), dict(temperature=0.9, top_k=20)], ids=["greedy", "sampled"])
def test_two_calls_return_the_tokens_of_one_long_call(trained, kw):
    a, b = 9, 15
    seed = 3 if kw else None
    want, wlen = generate(trained, PROMPTS, a + b, seed=seed, return_lengths=True, **kw)
    s = GenerationSession(trained, PROMPTS, 8 + a + b, seed=seed)
    first, flen = s.generate(a, **kw)
    assert torch.equal(first[:, :8 + a], want[:, :8 + a]) and flen.tolist() == [8 + a] * B
    assert not bool(first[:, 8 + a:].any())  # the pad token
    su.check_invariant(s)
    got, glen = s.generate(b, **kw)
    assert torch.equal(got, want) and torch.equal(glen, wlen)
    su.check_invariant(s)
    if not kw:
        assert bool(rule_holds(got).all())
    with pytest.raises(ValueError, match="would pass max_len"):
        s.generate(1)
    s.close()
    with pytest.raises(ValueError, match="closed"):
        s.generate(1)


def test_two_calls_with_ragged_prompts_top_p_and_an_eos(trained):
    prompts, plens = pad_prompts(RAGGED, 0)
    a, b = 6, 14
    kw = dict(temperature=0.7, top_k=20, top_p=0.9, eos_token=EOS)
    want, wlen = generate(trained, prompts, a + b, seed=5, prompt_lens=plens, pad_token=0, return_lengths=True, **kw)
    s = GenerationSession(trained, prompts, prompts.shape[1] + a + b, prompt_lens=plens, seed=5)
    _, flen = s.generate(a, stop_check=2, **kw)
    done = s.done.tolist()
    assert any(done) and not all(done), "the first call must end some rows and not all"
    assert all(int(n) < int(p) + a for n, p, d in zip(flen, plens, done) if d)
    su.check_invariant(s)  # the rows that went done rode along and were taken back
    got, glen = s.generate(b, **kw)
    assert torch.equal(got, want) and torch.equal(glen, wlen)
    su.check_invariant(s)


# ---- a session with appended tokens is a fresh call on the concatenated rows ------------------------------------
def test_append_then_continue_equals_a_fresh_call(trained):
    a, b = 5, 10
    s = GenerationSession(trained, PROMPTS, 8 + a + 4 + b)
    out, lens = s.generate(a)
    # rows 0, 2, 4 get the rule's next 4, 1, 3 tokens; rows 1, 3, 5 none
    n = [4, 0, 1, 0, 3, 0]
    add = [su.rule_next(out[r, int(lens[r]) - 1], n[r]) for r in range(B)]
    s.append(add)
    assert s.lengths.tolist() == [8 + a + k for k in n]
    got, glen = s.generate(b)
    su.check_invariant(s)
    rows = [r + x for r, x in zip(su.rows_of(out, lens), add)]
    assert su.rows_of(got, glen)[0][:len(rows[0])] == rows[0]
    fp, fl = pad_prompts(rows, 0)
    want, wlen = generate(trained, fp, b, prompt_lens=fl, return_lengths=True)
    gap = su.min_gap(trained, want, wlen, fl.tolist())
    print(f"smallest top-1 / top-2 logit gap of the fresh run: {gap:.4f}")
    assert gap > 1e-3
    assert su.rows_of(got, glen) == su.rows_of(want, wlen)
    assert not bool(got[:, fp.shape[1] + b:].any())
    # a tensor with counts is the same append
    s2 = GenerationSession(trained, PROMPTS, 8 + a + 4 + b)
    s2.generate(a)
    width = torch.tensor([x + [0] * (4 - len(x)) for x in add], dtype=torch.int64)
    s2.append(width, torch.tensor(n))
    got2, glen2 = s2.generate(b)
    assert torch.equal(got2, got) and torch.equal(glen2, glen)


def test_a_row_that_drew_the_eos_is_revived_by_an_append(trained):
    prompts, plens = pad_prompts(RAGGED, 0)
    a, b = 8, 8
    s = GenerationSession(trained, prompts, 8 + a + 3 + b, prompt_lens=plens)
    out, lens = s.generate(a, eos_token=EOS, stop_check=1)
    done = s.done.tolist()
    assert any(done) and not all(done)
    # every done row gets the rule's next tokens after its eos (the next turn); a live row gets 2, the others none
    live = [r for r in range(len(RAGGED)) if not done[r]]
    n = [3 if done[r] else (2 if r == live[0] else 0) for r in range(len(RAGGED))]
    add = [su.rule_next(out[r, int(lens[r]) - 1], n[r]) for r in range(len(RAGGED))]
    s.append(add)
    assert s.done.tolist() == [0] * len(RAGGED)
    got, glen = s.generate(b)  # no eos in the second turn: every row runs b tokens
    su.check_invariant(s)
    rows = [r + x for r, x in zip(su.rows_of(out, lens), add)]
    fp, fl = pad_prompts(rows, 0)
    want, wlen = generate(trained, fp, b, prompt_lens=fl, return_lengths=True)
    gap = su.min_gap(trained, want, wlen, fl.tolist())
    print(f"smallest top-1 / top-2 logit gap of the fresh run: {gap:.4f}")
    assert gap > 1e-3
    assert su.rows_of(got, glen) == su.rows_of(want, wlen)
    # a done row that gets nothing stays done: the next call leaves it alone
    s3 = GenerationSession(trained, prompts, 8 + a + b, prompt_lens=plens)
    o3, l3 = s3.generate(a, eos_token=EOS)
    d3 = s3.done.tolist()
    o4, l4 = s3.generate(b, eos_token=EOS)
    for r in range(len(RAGGED)):
        if d3[r]:
            assert int(l4[r]) == int(l3[r]) and torch.equal(o4[r], o3[r])
    su.check_invariant(s3)


# ---- chunked prefill --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk", [1, 3, 8])
def test_extend_in_chunks_gives_the_logits_of_one_shot_prefill(trained, chunk):
    want = su.prefill_logits(trained, PROMPTS)
    got, caches = su.extend_logits(trained, PROMPTS, chunk)
    torch.testing.assert_close(got, want, rtol=1e-4, atol=1e-4)
    assert all(c.lens.tolist() == [8] * B and c.n == 8 for c in caches)
    prompts, plens = pad_prompts(RAGGED, 0)
    want = su.prefill_logits(trained, prompts, plens)
    got, caches = su.extend_logits(trained, prompts, chunk, plens)
    torch.testing.assert_close(got, want, rtol=1e-4, atol=1e-4)
    assert all(c.lens.tolist() == plens.tolist() for c in caches)


def test_generate_with_prefill_chunk_returns_the_tokens_of_generate(trained):
    want, wlen = generate(trained, PROMPTS, 16, return_lengths=True)
    assert su.min_gap(trained, want, wlen, [8] * B) > 1e-3
    got, glen, stats = generate(trained, PROMPTS, 16, prefill_chunk=3, return_lengths=True, return_stats=True)
    assert torch.equal(got, want) and torch.equal(glen, wlen) and stats["steps"] == 16
    assert stats["generated"].tolist() == [16] * B
    assert torch.equal(generate(trained, PROMPTS, 16, prefill_chunk=3), want)
    assert torch.equal(generate(trained, PROMPTS, 16, prefill_chunk=0), want)
    prompts, plens = pad_prompts(RAGGED, 0)
    kw = dict(prompt_lens=plens, eos_token=EOS, return_lengths=True)
    want, wlen = generate(trained, prompts, 12, **kw)
    assert su.min_gap(trained, want, wlen, plens.tolist()) > 1e-3
    for chunk in (1, 3, 64):
        got, glen = generate(trained, prompts, 12, prefill_chunk=chunk, **kw)
        assert torch.equal(got, want) and torch.equal(glen, wlen), chunk
    assert torch.equal(generate(trained, PROMPTS, 0, prefill_chunk=3), PROMPTS)


# ---- refusals and the command line ------------------------------------------------------------------------------
def test_refusals(trained):
    from types import SimpleNamespace

    for kw, msg in ((dict(prefill_chunk=-1), "prefill_chunk must be"), (dict(prefill_chunk=1.5), "prefill_chunk must be"),
                    (dict(prefill_chunk=4, graph=True), "prefill_chunk > 0 with graph=True or lookup"),
                    (dict(prefill_chunk=4, lookup=3), "prefill_chunk > 0 with graph=True or lookup"),
                    (dict(lookup=3, graph=True), "graph=True")):
        with pytest.raises(ValueError, match=msg):
            generate(trained, PROMPTS, 4, **kw)
    block = trained.stages[0].cfg.block_size
    with pytest.raises(ValueError, match="exceeds block_size"):
        GenerationSession(trained, PROMPTS, block + 1)
    with pytest.raises(ValueError, match="do not fit max_len"):
        GenerationSession(trained, PROMPTS, 7)
    for field, val, msg in (("pp", 2, "pp=2 is not supported"), ("tp", 2, "tensor parallelism"),
                            ("dp", 2, "data parallelism")):
        mesh = SimpleNamespace(pp=1, tp=1, dp=1)
        setattr(mesh, field, val)
        fake = SimpleNamespace(mesh=mesh, kind=trained.kind, stages=trained.stages, spec=trained.spec)
        with pytest.raises(ValueError, match=msg):
            GenerationSession(fake, PROMPTS, 16)
    fake = SimpleNamespace(mesh=SimpleNamespace(pp=1, tp=1, dp=1), kind="rotate", stages=trained.stages,
                           spec=trained.spec)
    with pytest.raises(ValueError, match="rotate"):
        GenerationSession(fake, PROMPTS, 16)
    s = GenerationSession(trained, PROMPTS, 12)
    with pytest.raises(ValueError, match="would pass max_len"):
        s.generate(5)
    with pytest.raises(ValueError, match="would pass max_len"):
        s.append([[1] * 5] + [[]] * (B - 1))
    with pytest.raises(ValueError, match="prefill_chunk must be"):
        s.generate(2, prefill_chunk=-1)
    with pytest.raises(ValueError, match="token ids"):
        s.append([[97]] + [[]] * (B - 1))
    with pytest.raises(ValueError, match="lens must be"):
        s.append(torch.zeros(B, 2, dtype=torch.int64), [3] * B)
    assert s.lengths.tolist() == [8] * B  # a refused call changes nothing
    out, lens = s.generate(4)
    assert lens.tolist() == [12] * B and torch.equal(out, generate(trained, PROMPTS, 4))
    s0 = trained.stages[0]
    with pytest.raises(ValueError, match="extend of 6 x 9 positions"):
        s0.extend(torch.zeros(B, 9, dtype=torch.int64), s0.new_cache(B, 8))


def test_command_line(trained, tmp_path, capsys):
    from simple_distributed_machine_learning_amd import generate as gen_cli

    save_checkpoint(trained, str(tmp_path / "ckpt"), 1, 0)
    common = ["--rank", "0", "--world_size", "1", "--interface", "lo", "--model", "gpt2_tiny", "--dtype", "fp32",
              "--device", "cpu", "--ckpt_dir", str(tmp_path / "ckpt"), "--max_new_tokens", "16"]
    common += [a for row in PROMPTS[:3].tolist() for a in ("--prompt_tokens", ",".join(map(str, row)))]
    assert gen_cli.main(common) == 0
    want = [l for l in capsys.readouterr().out.splitlines() if l and l[0].isdigit()]
    assert gen_cli.main(common + ["--prefill_chunk", "3"]) == 0
    got = [l for l in capsys.readouterr().out.splitlines() if l and l[0].isdigit()]
    assert got == want and len(got) == 3
    for bad in (["--prefill_chunk", "-2"], ["--prefill_chunk", "4", "--lookup", "3"]):
        with pytest.raises(SystemExit, match="prefill_chunk"):
            gen_cli.main(common + bad)
