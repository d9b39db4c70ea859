"""AdamW on the device: the gfx950 kernels (csrc/kernels/adamw.hip) against the rule in fp64, the prep block against
the CPU schedule / clip numerics, the bindings' argument checks, the engine, hipGraph replay and two processes."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("no ROCm GPU", allow_module_level=True)

import adamw_util as au  # noqa: E402
from adamw_workers import max_param_diff, train_worker  # noqa: E402
from dist_util import run_ranks  # noqa: E402
from simple_distributed_machine_learning_amd import ops  # noqa: E402
from simple_distributed_machine_learning_amd._native import kernels  # noqa: E402
from simple_distributed_machine_learning_amd.data import SyntheticMNIST, SyntheticTokens  # noqa: E402
from simple_distributed_machine_learning_amd.models import get_model_spec  # noqa: E402
from simple_distributed_machine_learning_amd.ops import reference as ref  # noqa: E402
from simple_distributed_machine_learning_amd.ops.optim import make_schedule  # noqa: E402
from simple_distributed_machine_learning_amd.parallel import PipelineEngine, init_mesh  # noqa: E402
from simple_distributed_machine_learning_amd.parallel.graphs import GraphedStep  # noqa: E402

DEV = torch.device("cuda", 0)
U = 2.0 ** -24  # fp32 unit roundoff
DTYPES = [torch.float32, torch.bfloat16]


def _sizes(dtype):
    """64 (one granule), 4096 + 64 (several blocks, ragged), and two full grid strides of grad_sqnorm plus a ragged
    tail (the kernels' loops run twice, then partly: the update kernels' grids are capped like grad_sqnorm's)."""
    bf16 = dtype == torch.bfloat16
    blocks, threads, per = ops.grad_sqnorm_geometry(1 << 30, bf16)
    assert blocks == ops.SQNORM_MAX_BLOCKS
    return [64, 4096 + 64, 2 * blocks * threads * per + 8 * 1000 + 64]


def _ulps(got: float, want: float) -> float:
    w = torch.tensor(want, dtype=torch.float32)
    ulp = float(torch.nextafter(w.abs(), torch.tensor(math.inf)) - w.abs())
    return abs(float(got) - float(w)) / ulp


# ---- grad_sqnorm -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("which", [0, 1, 2])
@pytest.mark.parametrize("tail_heavy", [False, True])
def test_grad_sqnorm(dtype, which, tail_heavy):
    n = _sizes(dtype)[which]
    gen = torch.Generator().manual_seed(n)
    g = torch.randn(n, generator=gen)
    if tail_heavy:  # the largest entries sit in the last, partial chunk of the grid-stride loop
        g *= 1e-3
        g[-min(n, 8 * 1000 + 64) // 2:] = 100.0
    g = g.to(dtype)
    want = float(g.double().pow(2).sum())
    gd = g.to(DEV)
    a, b = ops.grad_sqnorm(gd), ops.grad_sqnorm(gd)
    assert a.dtype == torch.float64 and a.shape == (1,)
    assert torch.equal(a, b)  # no atomics: the same bits
    # the longest chain of fp32 roundings an element passes through (adamw.hip): one fma per element into the thread's
    # accumulator, trips * elements-per-lane of them; then 6 additions across the wave and 3 across the block's 4
    # waves. The partials are summed in fp64. All terms are >= 0, so the relative error is at most k u.
    blocks, threads, per = ops.grad_sqnorm_geometry(n, dtype == torch.bfloat16)
    trips = -(-(n // per) // (blocks * threads))
    k = trips * per + 6 + 3
    rel = abs(float(a) - want) / want
    print(f"grad_sqnorm n={n} {dtype}: rel err {rel:.3e}, bound {k} u = {k * U:.3e}")
    assert rel <= k * U


# ---- the update kernels ----------------------------------------------------------------------------------------------
_INPUTS = {}


def _inputs(n):
    if n not in _INPUTS:
        p0, grads = au.seeded(n, seed=n % 1000, steps=3)
        pad = torch.zeros(n, dtype=torch.bool)  # "padding": a ragged tail and (when there is room) a whole granule
        pad[n - 24:] = True
        if n >= 192:
            pad[64:128] = True
        p0[pad] = 0
        for g in grads:
            g[pad] = 0
        decay = (torch.arange((n + 63) // 64) % 2 == 0).to(torch.uint8)  # alternating per granule
        _INPUTS[n] = (p0, grads, pad, decay)
    return _INPUTS[n]


def _prep(t, lr, c):
    b1, b2 = au.BETAS
    return torch.tensor([t, lr, c, lr / (1 - b1 ** t), 1 / math.sqrt(1 - b2 ** t), 0, 0, 0], dtype=torch.float32)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("which", [0, 1, 2])
@pytest.mark.parametrize("wd,c,zero_grad", [(0.0, 1.0, False), (0.1, 1.0, True), (0.0, 0.37, True), (0.1, 0.37, False)])
def test_adamw_kernels(dtype, which, wd, c, zero_grad):
    """3 steps (the first, with zero moments, and later ones) against the rule in fp64, within 2 E; E is the CPU
    torch.optim.AdamW's own fp32 error on the same inputs."""
    n = _sizes(dtype)[which]
    mixed = dtype == torch.bfloat16
    p0, grads, pad, decay = _inputs(n)
    grads = [g.to(dtype) for g in grads]
    lrs = [1e-3, 7e-4, 1.3e-3]
    wd_elem = decay.repeat_interleave(64)[:n].float() * wd
    master = p0.to(DEV)
    p = master.to(dtype) if mixed else master
    m, v = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    dec = decay.to(DEV)
    for t, (g, lr) in enumerate(zip(grads, lrs), 1):
        gd = g.to(DEV)
        prep = _prep(t, lr, c).to(DEV)
        if mixed:
            ops.adamw_mixed_(master, p, gd, m, v, dec, prep, *au.BETAS, au.EPS, wd, zero_grad)
        else:
            ops.adamw_(p, gd, m, v, dec, prep, *au.BETAS, au.EPS, wd, zero_grad)
        assert torch.equal(gd.cpu(), torch.zeros_like(g) if zero_grad else g)
    got = (master.cpu(), m.cpu(), v.cpu())
    au.check_within_2E(got, p0, grads, lrs, [c] * 3, wd_elem, wd, what=f"n={n} {dtype} wd={wd} c={c}")
    for x in got:
        assert torch.equal(x[pad], torch.zeros_like(x[pad]))  # padding stays exactly zero
    if mixed:
        assert torch.equal(p, master.to(torch.bfloat16))
        assert torch.equal(p.cpu()[pad], torch.zeros(int(pad.sum()), dtype=torch.bfloat16))


# ---- the prep block ----------------------------------------------------------------------------------------------------
def test_prep_block_schedule_bias_correction_and_clip():
    n, lr, max_norm = 4096 + 64, 3e-4, 1.0
    sched = make_schedule("cosine", 2, 12, 3e-5)
    b1, b2 = au.BETAS
    g = torch.randn(n, generator=torch.Generator().manual_seed(5))
    gd = g.to(DEV)
    ctr = torch.zeros(1, dtype=torch.int64, device=DEV)
    prep = torch.zeros(ops.ADAMW_PREP_FLOATS, device=DEV)
    norm2 = torch.zeros(1, dtype=torch.float64, device=DEV)
    parts = torch.zeros(ops.SQNORM_MAX_BLOCKS, device=DEV)
    want_norm = float(g.double().norm())
    want_c = float(ref.clip_coef(ref.grad_sqnorm(g), max_norm))
    assert want_c < 1
    for t in range(1, 11):
        ops.adamw_prep(ctr, prep, lr, b1, b2, max_norm, sched, g=gd, partials=parts, norm2=norm2)
        if t not in (1, 2, 10):
            continue
        got = prep.cpu().tolist()
        assert int(ctr) == t and got[ops.PREP_T] == float(t)
        lr_t = ref.lr_at(t, lr, **sched)
        figs = {"lr": _ulps(got[ops.PREP_LR], lr_t), "step": _ulps(got[ops.PREP_STEP], lr_t / (1 - b1 ** t)),
                "rbc2": _ulps(got[ops.PREP_RBC2], 1 / math.sqrt(1 - b2 ** t)), "c": _ulps(got[ops.PREP_CLIP], want_c),
                "norm": _ulps(got[ops.PREP_NORM], want_norm)}
        print(f"prep t={t}: ulps {figs}")
        assert figs["lr"] <= 1 and figs["step"] <= 2 and figs["rbc2"] <= 2 and figs["c"] <= 2
        # the norm: the sum's k u (k = 1 trip x 4 + 9, test_grad_sqnorm), halved by the square root, + 1 for the cast
        assert figs["norm"] <= 13 / 2 + 1
    # clipping off: c = 1 and no norm; the total given by the caller (cross-rank sum) is used as it is
    ops.adamw_prep(ctr, prep, lr, b1, b2, 0.0, None)
    assert prep[ops.PREP_CLIP].item() == 1.0 and prep[ops.PREP_LR].item() == pytest.approx(lr, rel=1e-7)
    norm2.fill_(16.0)
    ops.adamw_prep(ctr, prep, lr, b1, b2, 2.0, None, norm2=norm2)
    assert _ulps(prep[ops.PREP_CLIP].item(), 2.0 / (4.0 + 1e-6)) <= 1 and prep[ops.PREP_NORM].item() == 4.0
    assert int(ctr) == 12


# ---- the bindings refuse wrong calls (nothing is launched) ----------------------------------------------------------------
def test_bindings_refuse_bad_arguments():
    k, n = kernels(), 256
    f = lambda dt=torch.float32, m=n: torch.zeros(m, device=DEV, dtype=dt)  # noqa: E731
    dec, prep = f(torch.uint8, n // 64), f(m=8)
    args = (0.9, 0.999, 1e-8, 0.0, False)
    k.adamw_(f(), f(), f(), f(), dec, prep, *args)  # the well-formed call
    k.adamw_mixed_(f(), f(torch.bfloat16), f(torch.bfloat16), f(), f(), dec, prep, *args)
    bad = [
        lambda: k.adamw_(f(torch.float64), f(), f(), f(), dec, prep, *args),  # dtype
        lambda: k.adamw_(f(), f(torch.bfloat16), f(), f(), dec, prep, *args),
        lambda: k.adamw_(f(), f(), f(), f(), dec.to(torch.int32), prep, *args),
        lambda: k.adamw_mixed_(f(), f(), f(torch.bfloat16), f(), f(), dec, prep, *args),
        lambda: k.adamw_(f(), f(m=n - 64), f(), f(), dec, prep, *args),  # lengths
        lambda: k.adamw_(f(), f(), f(m=n + 64), f(), dec, prep, *args),
        lambda: k.adamw_mixed_(f(), f(torch.bfloat16, n + 8), f(torch.bfloat16), f(), f(), dec, prep, *args),
        lambda: k.adamw_(f(), f(), f(), f(), dec[:-1].clone(), prep, *args),  # short decay table
        lambda: k.adamw_mixed_(f(), f(torch.bfloat16), f(torch.bfloat16), f(), f(), dec[:-1].clone(), prep, *args),
        lambda: k.adamw_(f(), f(), f(), f(), dec, f(m=4), *args),  # prep size
        lambda: k.adamw_(f(m=n + 4)[1:n + 1], f(), f(), f(), dec, prep, *args),  # alignment (4 B off)
        lambda: k.adamw_(f(), f(), f(), f(m=n + 4)[1:n + 1], dec, prep, *args),
        lambda: k.adamw_(f().cpu(), f(), f(), f(), dec, prep, *args),  # device
        lambda: k.adamw_(f(m=2 * n)[::2], f(), f(), f(), dec, prep, *args),  # contiguity
        lambda: k.grad_sqnorm(f(torch.float16), f(m=2048), f(torch.float64, 1)),
        lambda: k.grad_sqnorm(f(), f(m=2048), f(torch.float32, 1)),
        lambda: k.grad_sqnorm(f(m=n + 2), f(m=2048), f(torch.float64, 1)),
        lambda: k.grad_sqnorm(f(m=1 << 20), f(m=8), f(torch.float64, 1)),  # partials too short
        lambda: k.adamw_prep(None, None, None, f(torch.int32, 1), prep, 1e-3, 0.9, 0.999, 0.0, False, 0, 0, 0.0),
        lambda: k.adamw_prep(None, None, None, f(torch.int64, 1), prep, 1e-3, 0.9, 0.999, 1.0, False, 0, 0, 0.0),
    ]
    for i, call in enumerate(bad):
        with pytest.raises(RuntimeError):
            call()
            pytest.fail(f"bad call {i} was accepted")


# ---- engine ----------------------------------------------------------------------------------------------------------
def _engine(model, M=1, dtype=None, **opt):
    mesh = init_mesh(pp=1, schedule_kind="1f1b", rank=0, world_size=1, device=DEV)
    kw = {"seq_len": 16} if model == "gpt2_tiny" else {}
    if dtype is not None:
        kw["dtype"] = dtype
    opt = {"optimizer": "adamw", "lr": 1e-3, "weight_decay": 0.1, "clip_grad": 1.0, **opt}
    return PipelineEngine(get_model_spec(model, None, **kw), mesh, "1f1b", M, seed=5, **opt)


class _CpuRule:
    """reference.adamw_ on the CPU, fed one step's gradients at a time; norm, clip coefficient and decay mask computed
    here. Keeps what the 2 E bound needs (adamw_util.check_within_2E's yardstick) for the whole trajectory."""

    def __init__(self, eng, lr, wd, max_norm):
        n = eng.flat.numel
        self.lr, self.wd, self.max_norm = lr, wd, max_norm
        self.p0 = eng.flat.params.cpu().clone()
        self.p, self.m, self.v = self.p0.clone(), torch.zeros(n), torch.zeros(n)
        self.wd_elem = eng.optimizer.decay.cpu().repeat_interleave(64)[:n].float() * wd
        self.grads, self.clips = [], []

    def step(self, g):
        c = float(ref.clip_coef(ref.grad_sqnorm(g), self.max_norm))
        ref.adamw_(self.p, g, self.m, self.v, len(self.grads) + 1, self.lr, *au.BETAS, au.EPS, self.wd_elem, c)
        self.grads.append(g)
        self.clips.append(c)
        return c

    def yardstick(self):
        """E: torch.optim.AdamW's fp32 error in p against the rule in fp64 on this trajectory's gradients."""
        lrs = [self.lr] * len(self.grads)
        want = au.truth(self.p0, self.grads, lrs, self.clips, self.wd_elem)
        return au.errors(au.torch_adamw(self.p0, self.grads, lrs, self.clips, self.wd_elem, self.wd), want)[0]


@pytest.mark.parametrize("B", [192, 60])
def test_engine_mlp_matches_cpu_rule_on_its_own_gradients(B):
    """One engine steps on the device; the gradients its optimizer consumed go to the CPU and through
    reference.adamw_ (norm, clip coefficient, decay mask computed there); after 3 steps the two agree within the
    kernel-level bound (2 E). Gradients in hand, not a CPU engine's: Adam divides by sqrt(v), so last-bit gradient
    differences show at the scale of lr.

    A second engine from the same seed, run with step_optimizer=False and updated from the CPU, supplies a second set
    of gradients. Where it reproduces the first engine's step-1 gradients bit for bit (B = 60) the same bound is
    asserted for it too. At B = 192 it does not: the fp32 weight-gradient GEMM splits K and accumulates with atomics
    (gemm_f32.hip), so two runs of the same step differ in the last bits, elements whose gradient nearly cancels
    differ by a large relative amount, and AdamW turns that into a difference of about lr x 1e-4 in the weight:
    measured 9.2e-08 against 2 E = 3.0e-08 there (7.5e-09 against 2.8e-08 at B = 60). That is the gradient kernels'
    run-to-run difference, not the optimizer's, so for that engine the figure is printed and not asserted."""
    lr, wd, max_norm = 1e-3, 0.1, 0.05
    ds = SyntheticMNIST(3 * B, seed=3, device=DEV)
    e1, e2 = _engine("mlp", lr=lr, weight_decay=wd, clip_grad=max_norm), _engine("mlp", lr=lr, weight_decay=wd,
                                                                               clip_grad=max_norm)
    assert torch.equal(e1.flat.params, e2.flat.params)
    own, other = _CpuRule(e1, lr, wd, max_norm), _CpuRule(e2, lr, wd, max_norm)
    seen, eng_step = [], e1.optimizer.step

    def step(zero_grad=True):  # the gradients the device step is about to consume (it clears them)
        seen.append(e1.flat.grads.clone())
        eng_step(zero_grad)

    e1.optimizer.step = step
    for t in range(1, 4):
        e1.run(ds, (t - 1) * B, B, train=True)
        c = own.step(seen[-1].cpu())
        # (k u / 2 + 1 ulps: one trip of 4 elements + 9, as for the norm in the prep test)
        assert c < 1 and _ulps(float(e1.optimizer.prep[ops.PREP_CLIP]), c) <= 13 / 2 + 1
        e2.run(ds, (t - 1) * B, B, train=True, step_optimizer=False)
        other.step(e2.flat.grads.cpu().clone())
        e2.flat.params.copy_(other.p)
    assert len(seen) == 3 and e1.optimizer.steps == 3 and int(e1.optimizer.step_ctr) == 3
    assert e1.fast_steps["mlp_small"] == 0 and e2.fast_steps["mlp_small"] == 0  # the one-launch SGD step is bypassed
    got = e1.flat.params.cpu().double()
    same_grads = torch.equal(own.grads[0], other.grads[0])
    figs = [(float((got - r.p.double()).abs().max()), r.yardstick()) for r in (own, other)]
    print(f"mlp B={B}: device engine vs CPU rule max |dp| = {figs[0][0]:.3e} on its own gradients (E = {figs[0][1]:.3e}), "
          f"{figs[1][0]:.3e} on the second engine's (E = {figs[1][1]:.3e}); step-1 gradients equal: {same_grads}, "
          f"max |dg| = {float((own.grads[0] - other.grads[0]).abs().max()):.3e}")
    assert figs[0][0] <= 2 * figs[0][1]
    if same_grads:
        assert figs[1][0] <= 2 * figs[1][1]


@pytest.mark.parametrize("dtype", DTYPES)
def test_engine_gpt2_tiny(dtype):
    """lr wd = 3 lr: a LayerNorm weight (1.0) that were decayed would move by at least 2 lr, past the bound."""
    lr, wd = 1e-3, 3.0
    e = _engine("gpt2_tiny", M=2, dtype=dtype, lr=lr, weight_decay=wd)
    ds = SyntheticTokens(16, 16, 97, seed=3, device=DEV)
    opt = e.optimizer
    w = lambda: (opt.master if opt.master is not None else e.flat.params).float().cpu().clone()  # noqa: E731
    p0 = w()
    dec = opt.decay.cpu().repeat_interleave(64)[:e.flat.numel].bool()
    assert (opt.master is not None) == (dtype == torch.bfloat16)
    for step in range(2):
        e.run(ds, step * 8, 8, train=True)
        assert torch.isfinite(e.flat.params.float()).all() and torch.isfinite(opt.exp_avg).all()
        assert torch.isfinite(opt.exp_avg_sq).all() and torch.isfinite(opt.prep).all()
        if opt.master is not None:
            assert torch.equal(e.flat.params, opt.master.to(torch.bfloat16))
        if step == 0:
            dp = (w() - p0).abs()
            assert bool((dp <= lr * (1 + wd * dec * p0.abs()) * (1 + 1e-3)).all())
            assert float(dp.max()) > 0.5 * lr
    seen = 0
    for seg in e.flat.segments:
        if len(seg.shape) < 2:
            assert not dec[seg.offset:seg.offset + seg.numel].any(), seg.name
            seen += "ln" in seg.name and "weight" in seg.name
    assert seen >= 2 and float(opt.last_grad_norm) > 0


def test_hipgraph_replays_advance_the_device_step():
    sched = make_schedule("cosine", 2, 10, 1e-5)
    ds = SyntheticMNIST(600, seed=3, device=DEV)
    e1, e2 = _engine("mlp", lr_schedule=sched, clip_grad=0.05), _engine("mlp", lr_schedule=sched, clip_grad=0.05)
    g = GraphedStep(e2)
    sizes = [60, 60, 60, 60, 40, 60]  # as test_graphs_gpu.py: the 40 is a ragged batch with its own graph
    start = 0
    for B in sizes:
        r1 = e1.run(ds, start, B, train=True)
        r2 = g(ds, start, B)
        assert abs(float(r1.loss_sum) - float(r2.loss_sum)) <= 1e-4 * max(1.0, abs(float(r1.loss_sum)))
        start += B
    assert g.replays == len(sizes) - 1 and len(g.graphs) == 2 and not g.disabled
    torch.testing.assert_close(e1.flat.params, e2.flat.params, rtol=1e-5, atol=1e-6)
    assert int(e2.optimizer.step_ctr) == 6 and e2.optimizer.steps == 6 and e1.optimizer.steps == 6
    assert _ulps(float(e2.optimizer.last_lr), ref.lr_at(6, 1e-3, **sched)) <= 1
    assert float(e2.optimizer.prep[ops.PREP_T]) == 6.0 and float(e2.optimizer.prep[ops.PREP_CLIP]) < 1
    assert e2.fast_steps == {"mlp_small": 0, "cnn": 0}


def test_graphed_step_refuses_scheduled_sgd():
    e = _engine("mlp", optimizer="sgd", lr=0.1, weight_decay=0.0, clip_grad=0.0,
                lr_schedule=make_schedule("cosine", 2, 10))
    with pytest.raises(ValueError, match="schedule"):
        GraphedStep(e)
    assert e._sgd_fast is False


@pytest.mark.slow
def test_two_processes_on_one_gpu_global_norm():
    """gpt2_tiny, 1F1B, pp = 2, both ranks on cuda:0 over the host-staged transport, against the single-process device
    engine. Tolerance as in the Gloo test: the SGD difference of the same pair, x 2, + 1e-7; lr = 1e-4 for the
    reason given there."""
    steps, B, M = 3, 8, 2
    kw = {"seq_len": 16, "device": "cuda:0", "transport": "host"}
    diffs = {}
    for name, opt in (("sgd", {"optimizer": "sgd", "lr": 0.1}),
                      ("adamw", {"optimizer": "adamw", "lr": 1e-4, "weight_decay": 0.1, "clip_grad": 0.25})):
        res = run_ranks(train_worker, 2, "gpt2_tiny", "1f1b", M, 2, steps, B, opt, kw, timeout=300)
        one = train_worker(0, 1, "gpt2_tiny", "1f1b", M, 1, steps, B, opt, {"seq_len": 16, "device": "cuda:0"})
        assert all(r["transport"] == "host" for r in res)
        diffs[name] = max_param_diff(res, one)
        if name == "adamw":
            for r in res + [one]:
                assert len(r["clips"]) == steps and all(0 < c < 1 for c in r["clips"]), r["clips"]
                assert r["steps"] == (steps, steps)
            assert res[0]["norms"] == res[1]["norms"]
    print("max |dp| two processes vs one:", diffs)
    assert diffs["adamw"] <= 2 * diffs["sgd"] + 1e-7
