"""GPT-2 dropout on the CPU: statistics of the counter-hash masks (the torch twin of csrc/kernels/dropout_hash.h), a
self-test of the masked references / rounding models that the GPU tests use, and the engine: with dropout on, every
schedule, micro-batch count, dp x pp mesh and tensor-parallel split trains to the weights of one process."""
import math

import pytest
import torch

import gpt2_dropout_numerics as dn
import gpt2_numerics as gn
from dist_util import run_ranks
from dist_workers import train_worker
from simple_distributed_machine_learning_amd import cli
from simple_distributed_machine_learning_amd.models import GPT2Config, get_model_spec
from simple_distributed_machine_learning_amd.ops import reference as R
from test_pipeline_gloo import _compare, _merge_tp

SCALE = 0.125
P3 = {"embd_pdrop": 0.1, "attn_pdrop": 0.1, "resid_pdrop": 0.1}


# =====================================================================================================================
# A1: the twin's statistics
def _masks(S, T, site=R.DROP_SITE_ATTN):
    """{(layer, step): [3 samples, 3 heads, S, S] bool}"""
    out = {}
    for layer in (0, 5):
        for step in (0, 1):
            smp = torch.arange(10, 13)[:, None]
            hd = torch.arange(4, 7)[None, :]
            rk = R.gpt2_dropout_row_keys(dn.SEED, torch.tensor([step]), site, layer, smp, hd)
            out[(layer, step)] = R.gpt2_dropout_keep(rk, S, S, T)
    return out


def _corr(a, b):
    a, b = a.double().reshape(-1), b.double().reshape(-1)
    a, b = a - a.mean(), b - b.mean()
    return float((a * b).sum() / math.sqrt(float((a * a).sum()) * float((b * b).sum())))


@pytest.mark.parametrize("T", [26, 128])
def test_twin_mask_statistics(T):
    """144 masks (S in {33, 64, 129, 257}; 3 samples x 3 heads x 2 layers x 2 steps): every mask's kept fraction within
    5 binomial standard deviations of 1 - T / 256; lag-1 correlation along either axis below 0.01 and the agreement of
    two steps / heads / layers / sites within 0.01 of the independent rate (both pooled over the masks of a size)."""
    p = T / 256.0
    indep = p * p + (1 - p) * (1 - p)
    worst_sigma = worst_corr = worst_agree = 0.0
    for S in (33, 64, 129, 257):
        ms = _masks(S, T)
        allm = torch.stack(list(ms.values()))  # [4, 3, 3, S, S]
        frac = allm.double().mean((-1, -2))
        sigma = (frac - (1 - p)).abs() / math.sqrt(p * (1 - p) / (S * S))
        worst_sigma = max(worst_sigma, float(sigma.max()))
        worst_corr = max(worst_corr, abs(_corr(allm[..., :, 1:], allm[..., :, :-1])),
                         abs(_corr(allm[..., 1:, :], allm[..., :-1, :])))
        other_site = torch.stack(list(_masks(S, T, site=R.DROP_SITE_RESID_ATTN).values()))
        pairs = {"steps": (ms[(0, 0)], ms[(0, 1)]), "layers": (ms[(0, 0)], ms[(5, 0)]),
                 "heads": (allm[:, :, 0], allm[:, :, 1]), "samples": (allm[:, 0], allm[:, 1]),
                 "sites": (allm, other_site)}
        for name, (a, b) in pairs.items():
            worst_agree = max(worst_agree, abs(float((a == b).double().mean()) - indep))
    print(f"DROPOUT twin T={T}: kept fraction {worst_sigma:.2f} sigma, lag-1 |corr| {worst_corr:.4f}, "
          f"|agreement - independent| {worst_agree:.4f}")
    assert worst_sigma <= 5.0
    assert worst_corr < 0.01
    assert worst_agree <= 0.01


def test_twin_is_a_function_of_what_is_dropped():
    """A batch or head range cut in two draws the same bits; sample, head, step, layer and seed all change them."""
    T = 26
    whole = R.gpt2_attn_keep(7, torch.tensor([3]), 2, 100, 4, 0, 4, 33, T)
    assert torch.equal(whole[2:], R.gpt2_attn_keep(7, torch.tensor([3]), 2, 102, 2, 0, 4, 33, T))
    assert torch.equal(whole[:, 2:], R.gpt2_attn_keep(7, torch.tensor([3]), 2, 100, 4, 2, 2, 33, T))
    assert torch.equal(whole[..., :17, :17], R.gpt2_attn_keep(7, torch.tensor([3]), 2, 100, 4, 0, 4, 17, T))
    for other in (R.gpt2_attn_keep(8, torch.tensor([3]), 2, 100, 4, 0, 4, 33, T),
                  R.gpt2_attn_keep(7, torch.tensor([4]), 2, 100, 4, 0, 4, 33, T),
                  R.gpt2_attn_keep(7, torch.tensor([3]), 1, 100, 4, 0, 4, 33, T)):
        assert not torch.equal(whole, other)
    assert torch.equal(R.gpt2_attn_keep(7, None, 2, 0, 1, 0, 1, 9, T),
                       R.gpt2_attn_keep(7, torch.tensor([0]), 2, 0, 1, 0, 1, 9, T))
    assert [R.dropout_threshold(p) for p in (0.0, 0.001, 0.1, 0.5, 0.999)] == [0, 1, 26, 128, 255]


# =====================================================================================================================
# A2: the checker and the masked models
def _honest(family, S, causal, T, seed):
    B, H = 2, 3
    q, k, v, dout = dn.attn_inputs(family, B, S, H, seed)
    keep = dn.attn_keep(B, H, S, T, ctr=2)
    ref = dn.attention_drop_ref64(q, k, v, SCALE, causal, keep, T, dout)
    tiled = dn.attention_drop_model_tiled(q, k, v, SCALE, causal, keep, T)
    return (q, k, v, dout), keep, ref, tiled


@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("S", dn.ATTN_S)
def test_masked_models_agree_and_defects_are_rejected(S, causal):
    T = 26
    for i, family in enumerate(dn.ATTN_FAMILIES):
        (q, k, v, dout), keep, ref, tiled = _honest(family, S, causal, T, seed=900 * S + 10 * i)
        direct = dn.attention_drop_model_direct(q, k, v, SCALE, causal, keep, T)
        # two honest models: whole rows against 64-key tiles
        gn.check_grouped(direct["y"], tiled["y"], ref["y"], name=f"{family} y")
        mb = dn.attention_drop_model_bwd(q, k, v, tiled["y"], tiled["lse2"], dout, SCALE, causal, keep, T)
        md = dn.attention_drop_model_bwd(q, k, v, tiled["y"], direct["lse2"], dout, SCALE, causal, keep, T)
        extra = dn.attention_drop_cancellation_bound(q, k, v, tiled["y"], dout, ref["p"], SCALE, T)
        for n in ("dv", "dk", "dq"):
            gn.check_grouped(md[n], mb[n], ref[n], name=f"{family} {n}", fp32_extra=extra.get(n))
        # LSE does not see the mask
        plain = gn.attention_model_tiled(q, k, v, SCALE, causal)
        assert torch.equal(plain["lse2"], tiled["lse2"])

        allowed = gn._causal_mask(S, "cpu").expand_as(keep) if causal else torch.ones_like(keep)
        # defect 1: one flipped mask bit, where the probability is largest
        flat = int((ref["p"] * allowed).reshape(-1).argmax())
        bad_keep = keep.clone().reshape(-1)
        bad_keep[flat] = ~bad_keep[flat]
        bad = dn.attention_drop_model_tiled(q, k, v, SCALE, causal, bad_keep.view_as(keep), T)
        with pytest.raises(gn.Budget):
            gn.check_grouped(bad["y"], tiled["y"], ref["y"])
        # defect 2: the factor applied to l as well
        bad = dn.attention_drop_model_direct(q, k, v, SCALE, causal, keep, T, scale_l=True)
        with pytest.raises(gn.Budget):
            gn.check_grouped(bad["y"], tiled["y"], ref["y"])
        # defect 3: the backward regenerates the mask of another step (the first step whose mask differs where allowed)
        other = next(m for m in (dn.attn_keep(2, 3, S, T, ctr=c) for c in range(3, 40))
                     if not torch.equal(m & allowed, keep & allowed))
        bad = dn.attention_drop_model_bwd(q, k, v, tiled["y"], tiled["lse2"], dout, SCALE, causal, other, T)
        with pytest.raises(gn.Budget):
            gn.check_grouped(bad["dv"], mb["dv"], ref["dv"])


def test_fully_dropped_rows_are_zero_not_nan():
    """The first causal query has one key; where its bit is dropped y = 0 and its gradients are 0."""
    B, H, S, T = 8, 3, 5, 128
    q, k, v, dout = dn.attn_inputs("uniform 1.5", B, S, H, 5)
    keep = dn.attn_keep(B, H, S, T)
    dropped = ~keep[:, :, 0, 0]
    assert dropped.any() and not dropped.all()
    m = dn.attention_drop_model_tiled(q, k, v, SCALE, True, keep, T)
    mb = dn.attention_drop_model_bwd(q, k, v, m["y"], m["lse2"], dout, SCALE, True, keep, T)
    y0 = m["y"][:, 0]  # [B, H, 64]
    assert torch.isfinite(m["y"]).all() and all(torch.isfinite(t).all() for t in mb.values())
    assert (y0[dropped] == 0).all() and (mb["dq"][:, 0][dropped] == 0).all()


# =====================================================================================================================
# A3: engine invariance (gpt2_tiny, fp32: the torch twin draws the masks)
KW = dict({"stages": 2, "seq_len": 16}, **P3)
STEPS = 3


@pytest.fixture(scope="module")
def single():
    """One process, M = 1, B = 8 (and its p = 0 twin run)."""
    ref = train_worker(0, 1, "gpt2_tiny", "1f1b", 1, 1, STEPS, 8, 3, KW)
    off = train_worker(0, 1, "gpt2_tiny", "1f1b", 1, 1, STEPS, 8, 3, {"stages": 2, "seq_len": 16})
    return ref, off


def test_dropout_is_on(single):
    ref, off = single
    assert all(abs(a - b) > 1e-4 for a, b in zip(ref["losses"], off["losses"]))


def test_microbatch_count_does_not_change_the_run(single):
    res = train_worker(0, 1, "gpt2_tiny", "1f1b", 4, 1, STEPS, 8, 3, KW)
    _compare([res], single[0], rtol=1e-4, atol=1e-5)


@pytest.mark.slow
@pytest.mark.parametrize("kind", ["gpipe", "1f1b"])
def test_two_ranks_match_single_process(single, kind):
    res = run_ranks(train_worker, 2, "gpt2_tiny", kind, 2, 2, STEPS, 8, 3, KW)
    _compare(res, single[0], rtol=1e-4, atol=1e-5)


@pytest.mark.slow
def test_dp2_pp2_matches_single_process(single):
    res = run_ranks(train_worker, 4, "gpt2_tiny", "1f1b", 2, 2, STEPS, 4, 3, KW)
    _compare(res, single[0], rtol=1e-4, atol=1e-5)


@pytest.mark.slow
def test_tensor_parallel_matches_single_process(single):
    ref = single[0]
    res = run_ranks(train_worker, 2, "gpt2_tiny", "1f1b", 2, 1, STEPS, 8, 3, KW, 2)
    st = _merge_tp(res, 2, 32)
    for s in st:
        for k in ref["state"][s]:
            torch.testing.assert_close(st[s][k], ref["state"][s][k], rtol=1e-4, atol=1e-5, msg=f"stage {s} {k}")
    for a, b in zip(res[0]["losses"], ref["losses"]):
        assert a == pytest.approx(b, rel=1e-5, abs=1e-6)


# =====================================================================================================================
# A4
def _engine(p=0.1, M=2, kind="1f1b", seed=3):
    from simple_distributed_machine_learning_amd.parallel import PipelineEngine, init_mesh

    mesh = init_mesh(pp=1, schedule_kind=kind, rank=0, world_size=1, device=torch.device("cpu"))
    spec = get_model_spec("gpt2_tiny", 2, seq_len=16, embd_pdrop=p, attn_pdrop=p, resid_pdrop=p)
    return PipelineEngine(spec, mesh, schedule_kind=kind, num_microbatches=M, lr=0.1, momentum=0.5, seed=seed)


def _tokens():
    from simple_distributed_machine_learning_amd.data import SyntheticTokens

    return SyntheticTokens(64, 16, 97, seed=7)


def test_checkpoint_resume_continues_bit_for_bit(tmp_path):
    from simple_distributed_machine_learning_amd.utils.checkpoint import load_checkpoint, save_checkpoint

    ds = _tokens()
    a = _engine()
    for s in range(2):
        a.run(ds, 8 * s, 8, train=True)
    save_checkpoint(a, str(tmp_path), epoch=1, batch=1)
    la = [float(a.run(ds, 8 * s, 8, train=True).loss_sum) for s in (2, 3)]
    b = _engine()
    load_checkpoint(b, str(tmp_path))
    assert int(b.step_ctr) == 2
    lb = [float(b.run(ds, 8 * s, 8, train=True).loss_sum) for s in (2, 3)]
    assert la == lb
    assert torch.equal(a.flat.params, b.flat.params)


def test_eval_is_deterministic_and_equals_the_plain_forward():
    ds = _tokens()
    a, b = _engine(0.1), _engine(0.0)
    assert torch.equal(a.flat.params, b.flat.params)
    a.eval(), b.eval()
    la = [float(a.run(ds, 0, 8, train=False).loss_sum) for _ in range(2)]
    assert la[0] == la[1] == float(b.run(ds, 0, 8, train=False).loss_sum)
    assert not b._uses_rng and a._uses_rng  # the step counter advances only for models that draw masks


def test_refusals():
    with pytest.raises(ValueError, match="dropout is not supported with schedule 'rotate'"):
        _engine(0.1, M=2, kind="rotate")
    with pytest.raises(ValueError, match="GPT-2 model"):
        get_model_spec("mlp", 2, attn_pdrop=0.1)
    with pytest.raises(ValueError):
        GPT2Config(attn_pdrop=1.0)
    args = cli.build_parser().parse_args(["--rank", "0", "--model", "gpt2_tiny", "--attn_pdrop", "0.1"])
    assert (args.embd_pdrop, args.attn_pdrop, args.resid_pdrop) == (0.0, 0.1, 0.0)
    assert args.dropout == 0.5  # the reference CNN's flag keeps its meaning and default


def test_train_cli_records_effective_probabilities_and_refuses(tmp_path):
    import json

    from simple_distributed_machine_learning_amd import train

    def argv(*extra):
        return ["--rank", "0", "--world_size", "1", "--interface", "lo", "--device", "cpu", "--batch_size", "8",
                "--train_size", "16", "--test_size", "8", "--log_interval", "1", "--no_test", "--epochs", "1",
                "--master_port", str(__import__("dist_util").free_port()), *extra]

    m = tmp_path / "m.jsonl"
    hist = train.run(cli.parse_args(argv("--model", "gpt2_tiny", "--seq_len", "16", "--attn_pdrop", "0.1",
                                         "--resid_pdrop", "0.5", "--metrics", str(m))))
    train.shutdown(hist["mesh"])
    cfg = [json.loads(l) for l in open(m) if '"config"' in l]
    assert len(cfg) == 1
    assert (cfg[0]["embd_pdrop"], cfg[0]["attn_pdrop"], cfg[0]["resid_pdrop"]) == (0.0, 26 / 256, 0.5)
    assert int(hist["engine"].step_ctr) == 2
    with pytest.raises(SystemExit, match="dropout is not supported with schedule 'rotate'"):
        train.run(cli.parse_args(argv("--model", "gpt2_tiny", "--seq_len", "16", "--attn_pdrop", "0.1", "--schedule",
                                      "rotate")))
    with pytest.raises(SystemExit, match="GPT-2 model"):
        train.run(cli.parse_args(argv("--model", "mlp", "--embd_pdrop", "0.1")))


def test_config_dropout_sets_all_three():
    c = GPT2Config(dropout=0.1)
    assert (c.embd_pdrop, c.attn_pdrop, c.resid_pdrop) == (0.1, 0.1, 0.1)
    assert c.thresholds() == {"embd_pdrop": 26, "attn_pdrop": 26, "resid_pdrop": 26}
    assert c.effective_pdrop()["attn_pdrop"] == 26 / 256
    c = GPT2Config(dropout=0.1, attn_pdrop=0.0)
    assert (c.embd_pdrop, c.attn_pdrop, c.resid_pdrop) == (0.1, 0.0, 0.1)
    assert GPT2Config().thresholds() == {"embd_pdrop": 0, "attn_pdrop": 0, "resid_pdrop": 0}
