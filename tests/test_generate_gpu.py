"""Generation end to end on the real kernels: a d = 64 GPT-2 trained on the device, then prefill (flash attention) and
decode steps (linear_decode, attention_decode, the fused add + LayerNorm kernels, the on-device sampler)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no ROCm GPU", allow_module_level=True)

import gpt2_numerics as gn  # noqa: E402
from dist_util import run_ranks  # noqa: E402
from generate_util import (VOCAB, generate_worker, make_engine, nocache_greedy, nocache_logits, rule_holds,  # noqa: E402
                           train_steps)
from simple_distributed_machine_learning_amd.models.gpt2 import GPT2Stage  # noqa: E402
from simple_distributed_machine_learning_amd.parallel.generate import generate  # noqa: E402
from simple_distributed_machine_learning_amd.utils.checkpoint import save_checkpoint  # noqa: E402

PROMPTS = torch.arange(VOCAB)[:, None]
BF = torch.bfloat16


@pytest.fixture(scope="module")
def trained():
    """GPT2Config(n_layer=2, n_head=2, n_embd=128, vocab_size=97, block_size=64), 2 stages, bf16, one process on the
    GPU: 200 AdamW steps (lr 3e-3) of 16 x 32 tokens."""
    return train_steps(make_engine("gpt2_d64", "cuda:0", BF), 200, 16, 32)


@pytest.fixture(scope="module")
def greedy(trained):
    return generate(trained, PROMPTS, 63)


def test_greedy_generation_obeys_the_rule_and_equals_the_no_cache_loop(trained, greedy):
    """64 tokens: past the trained length of 32 and across the 64-key chunk of the decode attention."""
    assert greedy.shape == (97, 64) and greedy.is_cuda
    ok = rule_holds(greedy)
    assert int(ok.sum()) == 97 * 63, f"{int(ok.sum())} of {97 * 63} transitions obey the rule"
    assert torch.equal(greedy, nocache_greedy(trained, PROMPTS, 63))
    assert torch.equal(greedy, generate(trained, PROMPTS, 63))  # the same bits on every run
    # sampling: invariant to the batch split, keyed by the seed
    kw = dict(temperature=0.9, top_k=20, seed=3)
    whole = generate(trained, PROMPTS, 63, **kw)
    parts = torch.cat([generate(trained, PROMPTS[:40], 63, sample0=0, **kw),
                       generate(trained, PROMPTS[40:], 63, sample0=40, **kw)])
    assert torch.equal(whole, parts) and not torch.equal(whole, greedy)


def test_teacher_forced_decode_logits_are_as_accurate_as_the_training_forward(trained, greedy):
    """Prefill of 17 tokens, then 47 decode steps, against a float64 forward of the same bf16 weights; the yardstick is
    the training path's error at the same positions."""
    seq = greedy[5:9].contiguous()  # B = 4, 64 tokens
    s0, s1 = trained.stages[0], trained.stages[1]
    c0, c1 = s0.new_cache(4, 64), s1.new_cache(4, 64)
    got = [s1.prefill(s0.prefill(seq[:, :17], c0), c1)]
    for t in range(17, 64):
        got.append(s1.decode_step(s0.decode_step(seq[:, t], c0), c1))
    got = torch.stack(got, 1)
    assert got.shape[:2] == (4, 48) and got.shape[2] >= VOCAB
    assert not bool(got[..., VOCAB:].float().abs().max() > 0), "the pad columns of the logits must be zeros"
    got = got[..., :VOCAB].float().cpu()
    train = nocache_logits(trained, seq)[:, 16:].float().cpu()
    cfg = s0.cfg
    x = seq.cpu()
    for s, mod in ((0, s0), (1, s1)):  # float64 on the CPU, the same bf16 weights
        m64 = GPT2Stage(cfg, s, 2)
        m64.load_state_dict({k: v.detach().cpu() for k, v in mod.state_dict().items()})
        with torch.no_grad():
            x = m64.double().eval()(x)
    r64 = x[:, 16:]
    row_d, row_t = (got.double() - r64).abs().amax(-1), (train.double() - r64).abs().amax(-1)
    rms_d, rms_t = gn._rms(got.double() - r64), gn._rms(train.double() - r64)
    print(f"NUMERICS generate teacher forcing | logits | decode rms {rms_d:.4g} train rms {rms_t:.4g} | "
          f"decode worst row {float(row_d.max()):.4g} train worst row {float(row_t.max()):.4g}")
    assert rms_d <= gn.RMS_MARGIN * rms_t
    assert float(row_d.max()) <= gn.ROW_MARGIN * float(row_t.max())


@pytest.mark.slow
def test_two_processes_on_one_gpu_return_the_single_process_tokens(trained, greedy, tmp_path):
    save_checkpoint(trained, str(tmp_path), 1, 0)
    res = run_ranks(generate_worker, 2, "gpt2_d64", "cuda:0", BF, str(tmp_path), "host", 63, False, timeout=300)
    assert [r["stages"] for r in res] == [[0], [1]] and all(r["bytes_sent"] > 0 for r in res)
    for r in res:
        assert torch.equal(r["greedy"], greedy.cpu())
