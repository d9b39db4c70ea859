"""The one-launch forms of linear_decode and attention_decode (``tickets``): the last split / chunk to arrive reduces
inside the launch. They must return the bits of the two-launch forms, call after call through the same counters and
the same recycled workspace, and leave the counters zero."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no ROCm GPU", allow_module_level=True)

from simple_distributed_machine_learning_amd import _native  # noqa: E402
from simple_distributed_machine_learning_amd.ops import decode as dec  # noqa: E402

DEV = torch.device("cuda", 0)
K = _native.kernels()
BF = torch.bfloat16
CALLS = 24
SHAPES = {(768, 768): 6, (2304, 768): 2, (768, 3072): 6, (128, 512): 8, (64, 1024): 16, (16, 64): 1}  # (N, K): KS


def bits(t):
    return t.contiguous().view(torch.int16)


@pytest.mark.parametrize("M", [1, 16, 17, 64])
@pytest.mark.parametrize("N,Kd", list(SHAPES))
def test_linear_decode_with_tickets_returns_the_two_launch_bits(N, Kd, M):
    """24 consecutive calls per epilogue with fresh inputs through one tickets tensor. The caching allocator hands each
    call the workspace the call before it used, so a slab line left stale in a cache, or a counter left non-zero,
    shows as a mismatch."""
    assert K.linear_decode_splits(N, Kd) == SHAPES[(N, Kd)]
    g = torch.Generator(device=DEV).manual_seed(1000 * M + N + Kd)
    tickets = torch.zeros(N // 16, dtype=torch.int32, device=DEV)
    w = torch.empty(N, Kd, device=DEV).uniform_(-1, 1, generator=g).to(BF)
    for bias, gelu in ((False, False), (True, False), (True, True)):
        bad = torch.zeros((), dtype=torch.int64, device=DEV)
        for _ in range(CALLS):
            x = torch.empty(M, Kd, device=DEV).uniform_(-1, 1, generator=g).to(BF)
            b = torch.empty(N, device=DEV).uniform_(-1, 1, generator=g).to(BF) if bias else None
            got = dec.linear_decode(x, w, b, gelu=gelu, tickets=tickets)
            want = dec.linear_decode(x, w, b, gelu=gelu)
            bad += (bits(got) != bits(want)).sum()
            del got, want
        assert int(bad) == 0, f"bias={bias} gelu={gelu}: {int(bad)} elements differ over {CALLS} calls"
        assert not bool(tickets.any()), "the counters must be left zero"


def test_attention_decode_with_tickets_over_the_whole_cache_returns_the_two_launch_bits():
    """B = 5, H = 3, lens = [0, 63, 64, 127, 300] growing by one over 24 steps (63 -> 64 and 127 -> 128 add a chunk):
    the one-launch call at n_keys = Smax against the two-launch call at n_keys = max(lens) + 1, on two copies of a
    cache whose rows at and past lens[b] hold NaN patterns. Smax is 384, not 320: row 4 reaches 323 cached keys."""
    B, H, Smax = 5, 3, 384
    g = torch.Generator(device=DEV).manual_seed(7)
    lens = torch.tensor([0, 63, 64, 127, 300], dtype=torch.int32, device=DEV)
    caches = []
    for _ in range(2):
        c = torch.empty(B, Smax, H, 64, device=DEV).uniform_(-1.5, 1.5, generator=g).to(BF)
        for b, n in enumerate(lens.tolist()):
            c[b, n:] = math.nan
        caches.append(c)
    k1, v1 = caches
    k2, v2 = k1.clone(), v1.clone()
    tickets = torch.zeros(B * H, dtype=torch.int32, device=DEV)
    for step in range(CALLS):
        qkv = torch.empty(B, 3 * H * 64, device=DEV).uniform_(-1.5, 1.5, generator=g).to(BF)
        got = dec.attention_decode(qkv, k1, v1, lens, H, Smax, tickets=tickets)
        want = dec.attention_decode(qkv, k2, v2, lens, H, int(lens.max()) + 1)
        assert bool(torch.isfinite(want.float()).all()), step
        assert torch.equal(bits(got), bits(want)), f"step {step}, lens {lens.tolist()}"
        assert not bool(tickets.any()), f"step {step}: the counters must be left zero"
        del got, want
        lens += 1
    assert torch.equal(bits(k1), bits(k2)) and torch.equal(bits(v1), bits(v2))
    assert bool(torch.isnan(k1[0, 24:].float()).all()) and bool(torch.isfinite(k1[0, :24].float()).all())


def test_tickets_of_the_wrong_dtype_device_or_size_are_refused():
    x = torch.zeros(4, 768, dtype=BF, device=DEV)
    w = torch.zeros(768, 768, dtype=BF, device=DEV)
    with pytest.raises(RuntimeError, match="linear_decode: tickets must be a contiguous int32"):
        dec.linear_decode(x, w, tickets=torch.zeros(48, dtype=torch.int64, device=DEV))
    with pytest.raises(RuntimeError, match="linear_decode: tickets must be on the operands' device"):
        dec.linear_decode(x, w, tickets=torch.zeros(48, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="linear_decode: 47 tickets, but 48 are needed"):
        dec.linear_decode(x, w, tickets=torch.zeros(47, dtype=torch.int32, device=DEV))
    B, H, Smax = 2, 3, 64
    qkv = torch.zeros(B, 3 * H * 64, dtype=BF, device=DEV)
    kc, vc = (torch.zeros(B, Smax, H, 64, dtype=BF, device=DEV) for _ in range(2))
    lens = torch.zeros(B, dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError, match="attention_decode: tickets must be a contiguous int32"):
        dec.attention_decode(qkv, kc, vc, lens, H, Smax, tickets=torch.zeros(6, dtype=torch.float32, device=DEV))
    with pytest.raises(RuntimeError, match="attention_decode: tickets must be on the operands' device"):
        dec.attention_decode(qkv, kc, vc, lens, H, Smax, tickets=torch.zeros(6, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="attention_decode: 5 tickets, but 6 are needed"):
        dec.attention_decode(qkv, kc, vc, lens, H, Smax, tickets=torch.zeros(5, dtype=torch.int32, device=DEV))
    # (nothing was launched: the caches are untouched and a good call still works)
    assert not bool(kc.any())
    out = dec.attention_decode(qkv, kc, vc, lens, H, Smax, tickets=torch.zeros(6, dtype=torch.int32, device=DEV))
    assert out.shape == (B, H * 64)
