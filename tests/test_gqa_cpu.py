"""Grouped-query attention (GPT2Config.n_kv_head) on the torch twins: gpt2_tiny (H = 2) with one kv head trains,
checkpoints and resumes bit for bit, generates with batch invariance; n_kv_head unset or equal to n_head is today's
model; what a grouped model does not serve yet is refused by name."""
import pytest
import torch

from simple_distributed_machine_learning_amd.data import SyntheticTokens
from simple_distributed_machine_learning_amd.models import GPT2Config, get_model_spec
from simple_distributed_machine_learning_amd.ops.decode import attention_decode
from simple_distributed_machine_learning_amd.parallel import PipelineEngine, init_mesh
from simple_distributed_machine_learning_amd.parallel.generate import generate
from simple_distributed_machine_learning_amd.parallel.session import GenerationSession
from simple_distributed_machine_learning_amd.parallel.tp import TPContext
from simple_distributed_machine_learning_amd.utils.checkpoint import load_checkpoint, save_checkpoint

VOCAB = 97


def _engine(n_kv_head):
    mesh = init_mesh(pp=1, schedule_kind="1f1b", rank=0, world_size=1, device=torch.device("cpu"))
    spec = get_model_spec("gpt2_tiny", 2, dtype=torch.float32, n_kv_head=n_kv_head)
    return PipelineEngine(spec, mesh, schedule_kind="1f1b", num_microbatches=1, lr=3e-3, seed=1, optimizer="adamw")


def _train(engine, ds, first: int, steps: int):
    engine.train()
    for i in range(first, first + steps):
        engine.run(ds, i * 8, 8, train=True)
    return engine


@pytest.fixture(scope="module")
def mqa():
    """gpt2_tiny with one kv head for its two query heads, three optimizer steps in; eval mode."""
    e = _train(_engine(1), SyntheticTokens(64, 16, VOCAB, seed=1234), 0, 3)
    e.eval()
    return e


def test_train_checkpoint_resume(tmp_path):
    ds = SyntheticTokens(64, 16, VOCAB, seed=1234)
    a = _train(_engine(1), ds, 0, 3)
    assert a.stages[0].state_dict()["h.0.attn.c_attn.weight"].shape == (32 + 2 * 16, 32)  # (q | k | v), D = 16
    assert a.stages[0].new_cache(3, 8).k[0].shape == (3, 8, 1, 16)
    save_checkpoint(a, str(tmp_path), epoch=1, batch=2)
    b = _engine(1)
    load_checkpoint(b, str(tmp_path))
    assert torch.equal(a.flat.params, b.flat.params)
    ra, rb = a.run(ds, 24, 8, train=True), b.run(ds, 24, 8, train=True)
    assert float(ra.loss_sum) == float(rb.loss_sum) and torch.isfinite(ra.loss_sum)
    assert torch.equal(a.flat.params, b.flat.params)
    with pytest.raises(RuntimeError, match="size mismatch|shape"):  # another n_kv_head: torch's own message
        load_checkpoint(_engine(None), str(tmp_path))


def test_generate_batch_invariance(mqa):
    prompts = torch.tensor([[1, 2, 3, 4], [5, 6, 7, 0], [9, 0, 0, 0]])
    lens = torch.tensor([4, 3, 1], dtype=torch.int32)
    kw = dict(temperature=0.9, top_k=20, top_p=0.9, seed=5, eos_token=11)
    full = generate(mqa, prompts, 10, prompt_lens=lens, **kw)
    for b in range(3):
        alone = generate(mqa, prompts[b:b + 1], 10, prompt_lens=lens[b:b + 1], sample0=b, **kw)
        assert torch.equal(alone[0], full[b])
    assert torch.equal(full, generate(mqa, prompts, 10, prompt_lens=lens, **kw))


def test_unset_is_todays_model():
    ds = SyntheticTokens(64, 16, VOCAB, seed=1234)
    none, full = _train(_engine(None), ds, 0, 2), _train(_engine(2), ds, 0, 2)
    sa, sb = none.stages[0].state_dict(), full.stages[0].state_dict()
    assert list(sa) == list(sb) and sa["h.0.attn.c_attn.weight"].shape == (96, 32)
    assert all(torch.equal(sa[k], sb[k]) for k in sa)
    assert not GPT2Config(n_kv_head=12).grouped and GPT2Config().kv_heads == 12
    none.eval(), full.eval()
    prompts = torch.arange(6)[:, None]
    assert torch.equal(generate(none, prompts, 8, temperature=0.8, seed=3), generate(full, prompts, 8, temperature=0.8, seed=3))


@pytest.mark.parametrize("kw", [dict(lookup=2), dict(num_samples=2), dict(num_beams=2), dict(prefill_chunk=4),
                                dict(kv_dtype="fp8"), dict(kv_dtype="fp4")], ids=lambda kw: next(iter(kw)))
def test_generate_refusals(mqa, kw):
    with pytest.raises(ValueError, match="n_kv_head"):
        generate(mqa, torch.tensor([[1, 2, 3]]), 4, **kw)


def test_other_refusals(mqa):
    st = mqa.stages[0]
    cache = st.new_cache(1, 8)
    st.prefill(torch.tensor([[1, 2, 3]]), cache)
    x = torch.tensor([[4, 5]])
    nq = torch.tensor([2], dtype=torch.int32)
    tk = torch.zeros(2, dtype=torch.int32)
    for call in (lambda: GenerationSession(mqa, torch.tensor([[1, 2, 3]]), 8),
                 lambda: st.extend(x, cache), lambda: st.decode_block(x, cache, nq),
                 lambda: st.fork_cache(cache, 2, 4), lambda: st.beam_cache(cache, 2, 4),
                 lambda: st.new_cache(1, 8, kv_dtype="fp8"), lambda: st.shard_tp(TPContext(2, 0, None)),
                 lambda: GPT2Config(n_head=12, n_kv_head=5), lambda: get_model_spec("mlp", 2, n_kv_head=1),
                 lambda: attention_decode(torch.zeros(1, 64), cache.k[0], cache.v[0], cache.lens, 2, 4, tickets=tk)):
        with pytest.raises(ValueError, match="n_kv_head"):
            call()
