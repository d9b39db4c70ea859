"""Exact check of the uint8 forward's 16x16x32 MFMA loop (mlp_u8.hip u8_fwd_kernel), independent of summation order:
random pixel bytes against integer weights in [-8, 8] (the hi planes hold 256 w exactly, the lo planes are zero), zero
bias, scale 1, no ReLU. Every partial sum is an integer below 2^24 (times the planes' 2^8), so whatever order the
MFMAs add in, the output must equal the integer matrix product bit for bit; a wrong lane map, swizzle, tail or k
permutation is a gross mismatch. The integer product is taken in float64 on the device (exact: every value is below
2^53; checked once against the int64 product)."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no ROCm GPU", allow_module_level=True)

import mlp_numerics as mn  # noqa: E402
from simple_distributed_machine_learning_amd import _native  # noqa: E402

DEV = torch.device("cuda", 0)
K = _native.kernels()

MS = (mn.U8_FWD_MIN_ROWS, mn.U8_FWD_MIN_ROWS + 100)  # whole blocks; a ragged last block that is no multiple of 16
VARIANTS = {"waves16": ("U8_FWD_WAVES", 16), "wmt4": ("U8_FWD_WMT", 4)}


@functools.lru_cache(maxsize=None)
def case(M, N, Kd):
    g = torch.Generator().manual_seed(1000 * N + Kd + M)
    x8 = torch.randint(0, 256, (M, Kd), dtype=torch.uint8, generator=g).to(DEV)
    w = torch.randint(-8, 9, (N, Kd), generator=g).float().to(DEV)
    want = (x8.double() @ w.double().t()).float()  # = (x8.long() @ w.long().T).float()
    return x8, w, want


def run(variant, *args):
    name, value = VARIANTS[variant]
    try:
        K.set_knob(name, value)
        return K.linear_fwd_u8(*args)
    finally:
        K.reset_knobs()


def test_the_float64_product_is_the_integer_product():
    x8, w, want = case(MS[1], 128, 16)
    assert torch.equal(want.cpu(), (x8.cpu().long() @ w.cpu().long().t()).float())


@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("Kd", [16, 64, 96, 784])  # tail only, no tail, a 32-k tail, the flagship's 16-k tail
@pytest.mark.parametrize("N", [128, 256])
@pytest.mark.parametrize("M", MS)
def test_integer_product_is_exact(M, N, Kd, variant):
    x8, w, want = case(M, N, Kd)
    assert float(want.abs().max()) < 2.0 ** 24
    y = run(variant, x8, w, torch.zeros(N, device=DEV), False, 1.0)
    assert torch.equal(y, want), f"{int((y != want).sum())} of {y.numel()} outputs differ"


@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("N,Kd", [(128, 784), (256, 96)])
def test_relu_bits_are_those_of_the_output(N, Kd, variant):
    M = MS[1]
    x8, w, want = case(M, N, Kd)
    g = torch.Generator().manual_seed(N + Kd)
    b = torch.randint(-1000, 1001, (N,), generator=g).float().to(DEV)  # integers: y stays exact
    mask = torch.full((M, N // 32), -1, dtype=torch.int32, device=DEV)
    y = run(variant, x8, w, b, True, 1.0, None, False, mask)
    assert torch.equal(y, torch.relu(want + b))
    frac = float((y > 0).float().mean())
    assert 0.3 < frac < 0.7, frac  # about half the outputs are cut
    assert torch.equal(mask, K.relu_bits(y)) and torch.equal(mask, mn.relu_bits_of(y))
