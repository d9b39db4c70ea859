"""Several samples per prompt on the CPU (the torch twins) with a trained gpt2_tiny: attention_fork_ref against
attention_decode_ref on the concatenated cache, generate(num_samples=n) against the call on the n-fold repeated
prompts, the refusals, the command line.

CPU fp32 ``F.linear`` rows depend on the row count, and the forked call prefills B rows where the repeated call
prefills B n (the decode steps run B n rows in both), so the greedy test first requires a clear top-1 of the repeated
run, as tests/test_lookup_generate_cpu.py does."""
import json

import pytest
import torch

import fork_util as fu
import lookup_util as lu
from generate_util import make_engine, nocache_logits, train_steps
from simple_distributed_machine_learning_amd.ops import decode as dec
from simple_distributed_machine_learning_amd.parallel.generate import generate, pad_prompts
from simple_distributed_machine_learning_amd.utils.checkpoint import save_checkpoint

NEW = 20
PROMPTS = lu.rule_prompts([1, 2, 5, 17])


@pytest.fixture(scope="module")
def trained():
    """gpt2_tiny as tests/test_generate_cpu.py trains it: 2 stages in one process, fp32, AdamW lr 3e-3, seed 1, 100
    steps of 32 x 16 tokens."""
    return train_steps(make_engine("gpt2_tiny", "cpu", torch.float32), 100, 32, 16)


# ---- the twin --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", fu.NS)
def test_the_twin_is_attention_decode_ref_on_the_concatenated_cache(n):
    """Exact fp32 equality, the written suffix rows, the untouched rest; NaN tails in both caches."""
    for i in range(len(fu.PLENS)):
        qkv, kp, vp, plens, ks, vs, suf, lens = fu.fork_inputs(n, i, dtype=torch.float32, pmax=136, nmax=68)
        kf, vf = fu.materialise(kp, ks, plens, suf, n), fu.materialise(vp, vs, plens, suf, n)
        want = dec.attention_decode_ref(qkv, kf, vf, fu.i32(lens), fu.H, 136 + 68)
        kp0, vp0, ks0, vs0 = kp.clone(), vp.clone(), ks.clone(), vs.clone()
        got = dec.attention_fork(qkv, kp, vp, fu.i32(plens), ks, vs, fu.i32(lens), n, fu.H, 136 + 68)
        assert torch.equal(got, want) and bool(torch.isfinite(got).all()), (n, i)
        tight = dec.attention_fork(qkv, kp0.clone(), vp0.clone(), fu.i32(plens), ks0.clone(), vs0.clone(), fu.i32(lens),
                                   n, fu.H, max(lens) + 1)
        # (the twins' fp32 sums run over n_keys terms: equal bits at an equal bound, close ones across bounds)
        assert torch.equal(tight, dec.attention_decode_ref(qkv, kf, vf, fu.i32(lens), fu.H, max(lens) + 1)), (n, i)
        torch.testing.assert_close(tight, want, atol=1e-5, rtol=1e-5)
        for r in range(fu.G * n):
            s = suf[r]
            assert torch.equal(ks[r, s].reshape(-1), qkv[r, fu.C:2 * fu.C]), (n, i, r)
            assert torch.equal(vs[r, s].reshape(-1), qkv[r, 2 * fu.C:]), (n, i, r)
            assert torch.equal(ks[r, s], kf[r, plens[r // n] + s])
            for a, b in ((ks, ks0), (vs, vs0)):
                assert torch.equal(a[r, :s], b[r, :s]) and bool(torch.isnan(a[r, s + 1:]).all()), (n, i, r)
        assert torch.equal(fu.bits(kp), fu.bits(kp0)) and torch.equal(fu.bits(vp), fu.bits(vp0))


def test_the_twin_serves_other_head_widths_and_the_wrapper_refuses_bad_arguments():
    R, n, Hh, D = 4, 2, 3, 16
    qkv = fu.rnd(R, 3 * Hh * D, seed=1, dtype=torch.float32)
    kp, vp = fu.rnd(2, 10, Hh, D, seed=2, dtype=torch.float32), fu.rnd(2, 10, Hh, D, seed=3, dtype=torch.float32)
    ks, vs = fu.rnd(R, 6, Hh, D, seed=4, dtype=torch.float32), fu.rnd(R, 6, Hh, D, seed=5, dtype=torch.float32)
    plens, lens = fu.i32([3, 10]), fu.i32([3, 5, 10, 15])
    full = torch.cat([kp.repeat_interleave(n, 0), torch.zeros(R, 6, Hh, D)], 1), \
        torch.cat([vp.repeat_interleave(n, 0), torch.zeros(R, 6, Hh, D)], 1)
    for r, (p, ln) in enumerate(zip([3, 3, 10, 10], lens.tolist())):
        full[0][r, p:ln], full[1][r, p:ln] = ks[r, :ln - p], vs[r, :ln - p]
    want = dec.attention_decode_ref(qkv, full[0], full[1], lens, Hh, 16)
    ks0 = ks.clone()
    assert torch.equal(dec.attention_fork(qkv, kp, vp, plens, ks, vs, lens, n, Hh, 16), want)
    ks.copy_(ks0)
    for args in ((qkv, kp, vp, plens, ks, vs, lens, 0, Hh, 16), (qkv, kp, vp, plens, ks, vs, lens, 65, Hh, 16),
                 (qkv, kp, vp, plens, ks, vs, lens, True, Hh, 16), (qkv, kp, vp, plens, ks, vs, lens, 4, Hh, 16),
                 (qkv, kp, vp, plens, ks, vs, lens, n, Hh, 0), (qkv, kp, vp, plens, ks, vs, lens, n, Hh, 17),
                 (qkv, kp, vp, plens.long(), ks, vs, lens, n, Hh, 16), (qkv, kp, vp, plens, ks, vs, lens[:3], n, Hh, 16),
                 (qkv, kp, vp, lens, ks, vs, lens, n, Hh, 16), (qkv.double(), kp, vp, plens, ks, vs, lens, n, Hh, 16),
                 (qkv, kp, vp[:, :9], plens, ks, vs, lens, n, Hh, 16), (qkv, kp, vp, plens, ks, vs, lens, n, Hh + 1, 16),
                 (qkv[:, 1:], kp, vp, plens, ks, vs, lens, n, Hh, 16)):
        with pytest.raises(ValueError, match="attention_fork"):
            dec.attention_fork(*args)
    assert torch.equal(ks, ks0)


# ---- generate ------------------------------------------------------------------------------------------------------
def test_greedy_siblings_are_the_plain_rows(trained):
    want = fu.repeated(generate, trained, PROMPTS, NEW, 3, return_lengths=True, return_stats=True)
    top2 = nocache_logits(trained, want[0])[:, 7:-1].float().topk(2, dim=-1).values
    gap = float((top2[..., 0] - top2[..., 1]).min())
    print(f"smallest top-1 / top-2 logit gap of the repeated run: {gap:.4f}")
    assert gap > 1e-3  # the precondition, an assertion and not a skip
    got = generate(trained, PROMPTS, NEW, num_samples=3, return_lengths=True, return_stats=True)
    fu.same(got, want)
    plain = generate(trained, PROMPTS, NEW)
    assert got[0].shape == (12, 8 + NEW) and torch.equal(got[0], plain.repeat_interleave(3, 0))
    assert got[2]["steps"] == NEW and got[2]["generated"].tolist() == [NEW] * 12


def test_sampled_siblings_differ_and_equal_the_repeated_call(trained):
    kw = dict(temperature=1.5, top_k=0, seed=5, sample0=7)
    want = fu.repeated(generate, trained, PROMPTS, NEW, 4, **kw)
    groups = want.view(4, 4, -1)
    assert any(not torch.equal(groups[b, 0], groups[b, j]) for b in range(4) for j in range(1, 4)), \
        "the siblings of the repeated call do not differ: raise the temperature"
    fu.same(generate(trained, PROMPTS, NEW, num_samples=4, **kw), want)
    # two samples, no new tokens, one new token (no decode step at all)
    for new in (0, 1):
        fu.same(generate(trained, PROMPTS, new, num_samples=2, return_lengths=True, return_stats=True, **kw),
                fu.repeated(generate, trained, PROMPTS, new, 2, return_lengths=True, return_stats=True, **kw))


def test_ragged_prompts_with_an_eos(trained):
    rows = [PROMPTS[0].tolist(), PROMPTS[1, :3].tolist(), PROMPTS[2, :7].tolist(), PROMPTS[3, :1].tolist()]
    prompts, plens = pad_prompts(rows, 0)
    prompts[1, 3:] = 55  # (whatever the caller left in the padding)
    kw = dict(temperature=0.9, top_k=20, top_p=0.9, seed=3, prompt_lens=plens, eos_token=int(PROMPTS[0, 3]), pad_token=0,
              return_lengths=True, return_stats=True)
    want = fu.repeated(generate, trained, prompts, NEW, 2, **kw)
    assert int(want[1].min()) < int(want[1].max()), "no row met the eos"
    for sc in (0, 1, 16):
        got = generate(trained, prompts, NEW, num_samples=2, stop_check=sc, **kw)
        ref = want if sc == 16 else fu.repeated(generate, trained, prompts, NEW, 2, stop_check=sc, **kw)
        fu.same(got, ref)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])  # stop_check does not change them
    assert got[0].shape == (8, 8 + NEW) and got[1].shape == (8,)


def test_one_sample_is_todays_call(trained):
    kw = dict(temperature=0.9, top_k=20, seed=3)
    assert torch.equal(generate(trained, PROMPTS, NEW, num_samples=1, **kw), generate(trained, PROMPTS, NEW, **kw))
    assert torch.equal(generate(trained, PROMPTS, NEW, num_samples=1, lookup=3), generate(trained, PROMPTS, NEW))


def test_refusals(trained):
    for kw, msg in ((dict(num_samples=0), "num_samples must be"), (dict(num_samples=65), "num_samples must be"),
                    (dict(num_samples=2.5), "num_samples must be"), (dict(num_samples=True), "num_samples must be"),
                    (dict(num_samples=2, graph=True), "graph=True"), (dict(num_samples=2, lookup=2), "lookup > 0"),
                    (dict(num_samples=2, prefill_chunk=4), "prefill_chunk > 0")):
        with pytest.raises(ValueError, match=msg):
            generate(trained, PROMPTS, 4, **kw)
    s0 = trained.stages[0]
    cache = s0.new_cache(2, 8)
    with pytest.raises(ValueError, match="prefill it first"):
        s0.fork_cache(cache, 2, 4)
    s0.prefill(PROMPTS[:2], cache)
    for n, nmax in ((0, 4), (65, 4), (2, 0), (2, s0.cfg.block_size - 7)):
        with pytest.raises(ValueError, match="fork_cache"):
            s0.fork_cache(cache, n, nmax)
    fc = s0.fork_cache(cache, 2, 1)
    assert fc.lens.tolist() == [8] * 4 and fc.n == 8 and fc.nmax == 1 and fc.ks[0].shape[:2] == (4, 1)
    s0.decode_step_forked(torch.zeros(4, dtype=torch.int64), fc)
    assert fc.lens.tolist() == [9] * 4 and fc.n == 9 and cache.lens.tolist() == [8] * 2 and cache.n == 8
    with pytest.raises(ValueError, match="forked cache is full"):
        s0.decode_step_forked(torch.zeros(4, dtype=torch.int64), fc)


def test_command_line(trained, tmp_path, capsys):
    from simple_distributed_machine_learning_amd import generate as gen_cli

    save_checkpoint(trained, str(tmp_path / "ckpt"), 1, 0)
    common = ["--rank", "0", "--world_size", "1", "--interface", "lo", "--model", "gpt2_tiny", "--dtype", "fp32",
              "--device", "cpu", "--ckpt_dir", str(tmp_path / "ckpt"), "--max_new_tokens", str(NEW), "--temperature",
              "1.5", "--seed", "5"]
    common += [a for row in PROMPTS[:3].tolist() for a in ("--prompt_tokens", ",".join(map(str, row)))]
    mpath = tmp_path / "m.jsonl"
    assert gen_cli.main(common + ["--num_samples", "2", "--metrics", str(mpath)]) == 0
    got = [l for l in capsys.readouterr().out.splitlines() if l and l[0].isdigit()]
    want = generate(trained, PROMPTS[:3], NEW, temperature=1.5, seed=5, num_samples=2).tolist()
    assert len(got) == 6 and got == [",".join(map(str, r)) for r in want]
    ev = [json.loads(l) for l in mpath.read_text().splitlines()]
    assert [e["event"] for e in ev] == ["generate"]
    assert ev[0]["num_samples"] == 2 and ev[0]["samples"] == 6 and ev[0]["tokens"] == 6 * NEW and ev[0]["steps"] == NEW
    with pytest.raises(SystemExit, match="num_samples"):
        gen_cli.main(common + ["--num_samples", "65"])
    with pytest.raises(SystemExit, match="num_samples"):
        gen_cli.main(common + ["--num_samples", "2", "--lookup", "2"])
