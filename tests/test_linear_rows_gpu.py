"""linear_rows.hip, the decode projections for 65..512 rows: every row carries the bits linear_decode.hip gives it in a
call of at most 64 rows, within linear_decode's fp64 budget (tests/gpt2_decode_numerics.py), through the kernel binding,
the ``ops.decode.linear_decode`` wrapper and ``generate()`` across the 64-row line."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no ROCm GPU", allow_module_level=True)

import gpt2_decode_numerics as dn  # noqa: E402
import gpt2_numerics as gn  # noqa: E402
import lookup_util as lu  # noqa: E402
from generate_util import train_steps  # noqa: E402
from simple_distributed_machine_learning_amd import _native  # noqa: E402
from simple_distributed_machine_learning_amd.ops import decode as dec  # noqa: E402
from simple_distributed_machine_learning_amd.parallel.generate import generate  # noqa: E402

DEV = torch.device("cuda", 0)
K = _native.kernels()
BF = torch.bfloat16
EPIS = (dec.EPI_STORE, dec.EPI_BIAS, dec.EPI_BIAS_GELU)
SHAPES = [(768, 768), (2304, 768), (3072, 768), (768, 3072), (16, 64)]
CASES = [(M, N, Kd) for (N, Kd) in SHAPES for M in (65, 80, 129, 512)] + [(65, 50304, 768)]


@functools.lru_cache(maxsize=2)
def inputs(M, N, Kd):
    """test_decode_kernels_gpu.py's linear_inputs: (x, w, b) on the CPU and on the device."""
    def rnd(*shape, seed):
        return torch.empty(shape).uniform_(-1, 1, generator=torch.Generator(device="cpu").manual_seed(seed))
    seed = M + N + Kd
    cpu = ((rnd(M, Kd, seed=seed) * 2.0).to(BF), (rnd(N, Kd, seed=seed + 1) * 0.08).to(BF),
           (rnd(N, seed=seed + 2) * 0.5).to(BF))
    return cpu, tuple(t.to(DEV) for t in cpu)


def bits(t):
    return t.contiguous().view(torch.int16)


@pytest.mark.parametrize("M,N,Kd", CASES)
def test_rows_carry_linear_decode_bits(M, N, Kd):
    _, (x, w, b) = inputs(M, N, Kd)
    assert K.linear_rows_supported(M, N, Kd, Kd, Kd)
    for epi in EPIS:
        bias = None if epi == dec.EPI_STORE else b
        y = K.linear_rows(x, w, bias, epi)
        want = torch.cat([K.linear_decode(x[i:i + 64], w, bias, epi) for i in range(0, M, 64)])
        assert torch.equal(bits(y), bits(want)), f"epi {epi}: not the 64-row slices' bits"
        if M >= 107:  # rows 70..106: off a 16-row group and off a panel
            assert torch.equal(bits(y[70:107]), bits(K.linear_decode(x[70:107], w, bias, epi))), f"epi {epi}: rows 70.."
        assert torch.equal(bits(K.linear_rows(x, w, bias, epi)), bits(y)), f"epi {epi}: not deterministic"


@pytest.mark.parametrize("N,Kd", SHAPES)
def test_budget_against_fp64(N, Kd):
    (x, w, b), (xd, wd, bd) = inputs(129, N, Kd)
    y0 = K.linear_rows(xd, wd, None, dec.EPI_STORE)
    y1 = K.linear_rows(xd, wd, bd, dec.EPI_BIAS)
    r0 = gn.check_elementwise(y0.cpu(), dn.linear_ref64(x, w), a=dn.linear_abs_bound(x, w), name="linear_rows")
    r1 = gn.check_elementwise(y1.cpu(), dn.linear_ref64(x, w, b), a=dn.linear_abs_bound(x, w, b),
                              name="linear_rows bias")
    print(f"NUMERICS linear_rows M=129 N={N} K={Kd} | store {r0:.3f} | bias {r1:.3f}")


def test_strided_x():
    _, (x, w, b) = inputs(80, 768, 768)
    wide = torch.zeros(80, 768 + 264, dtype=BF, device=DEV)
    wide[:, 8:8 + 768] = x
    xs = wide[:, 8:8 + 768]
    assert xs.stride(0) == 1032 and K.linear_rows_supported(80, 768, 768, 1032, 768)
    assert torch.equal(bits(K.linear_rows(xs, w, b, dec.EPI_BIAS_GELU)), bits(K.linear_rows(x, w, b, dec.EPI_BIAS_GELU)))


def test_wrapper_and_refusals():
    _, (x, w, b) = inputs(80, 768, 768)
    assert dec.LINEAR_ROWS_DISPATCH_M <= dec.LINEAR_ROWS_MAX_M == K.linear_rows_max_m() == 512
    assert dec.LINEAR_ROWS_DISPATCH_M == K.linear_rows_dispatch_m() >= 80
    assert torch.equal(bits(dec.linear_decode(x, w, b, gelu=True)), bits(K.linear_rows(x, w, b, dec.EPI_BIAS_GELU)))
    assert torch.equal(bits(dec.linear_decode(x[:64], w, b)), bits(K.linear_decode(x[:64], w, b, dec.EPI_BIAS)))
    for M, N, Kd in [(64, 768, 768), (513, 768, 768), (80, 24, 64), (80, 768, 96)]:
        assert not dec.linear_rows_supported(M, N, Kd)
        with pytest.raises(RuntimeError, match="linear_rows: unsupported shape"):
            K.linear_rows(torch.zeros(M, Kd, dtype=BF, device=DEV), torch.zeros(N, Kd, dtype=BF, device=DEV), None, 0)
    with pytest.raises(RuntimeError):  # fp32 operands
        K.linear_rows(torch.zeros(80, 64, device=DEV), torch.zeros(16, 64, device=DEV), None, 0)


def test_generate_splits_across_the_64_row_line():
    """80 prompts in one call draw, row for row, the tokens of two calls of 40 with the matching sample0 (the d = 64
    model of tests/test_fork_generate_gpu.py: bit equality does not need it to be good)."""
    model = train_steps(lu.make_engine_d64("cuda:0", BF, 192), 60, 16, 32)
    prompts = lu.rule_prompts([t for t in range(1, 82) if t != 60])  # (60 is the rule's fixed point)
    kw = dict(temperature=1.5, top_k=0, seed=5)
    whole = generate(model, prompts, 24, **kw)
    halves = [generate(model, prompts[i:i + 40], 24, sample0=i, **kw) for i in (0, 40)]
    assert torch.equal(whole, torch.cat(halves))
