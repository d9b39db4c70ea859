"""attention_extend (any T new positions per sample against the KV cache plus themselves) on the GPU: its bit contract
with attention_fwd (raw bits of the full-sequence causal forward at positions L .. S - 1, for every split L, over
several consecutive calls and with ragged lengths in one call), the cache rows it writes, dead positions, batch
invariance, determinism, the host bound, attention_fwd's fp64 budget and the refusals. Cache tails and the padding of
qkv hold NaN patterns throughout: rows a position does not see are never used as data."""
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no ROCm GPU", allow_module_level=True)

import gpt2_numerics as gn  # noqa: E402
from simple_distributed_machine_learning_amd import _native  # noqa: E402
from simple_distributed_machine_learning_amd.ops import decode as dec  # noqa: E402

DEV = torch.device("cuda", 0)
K = _native.kernels()
BF = torch.bfloat16
SCALE = 0.125
B, H, S = 3, 2, 192  # three key tiles, two 128-query blocks
C = H * 64
SPLITS = [0, 1, 37, 64, 100, 128, 191]
RAGGED = [0, 37, 130]


def rnd(*shape, seed=0, amp=1.5):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.empty(shape).uniform_(-1, 1, generator=g) * amp).to(BF)


def bits(t):
    return t.contiguous().view(torch.int16)


def i32(v):
    return torch.tensor(list(v), dtype=torch.int32, device=DEV)


@functools.lru_cache(maxsize=None)
def sequence():
    """The full sequence's fused projection [B, S, 3C] and attention_fwd over it (causal, default knobs) [B, S, C].
    Computed once, left unchanged."""
    qkv = rnd(B, S, 3 * C, seed=11)
    q, k, v = (qkv[..., i * C:(i + 1) * C].reshape(B, S, H, 64).to(DEV) for i in range(3))
    out, _ = K.attention_fwd(q, k, v, SCALE, True)
    torch.cuda.synchronize()
    return qkv, out.view(B, S, C).cpu()


def seq_kv():
    qkv, _ = sequence()
    return qkv[..., C:2 * C].reshape(B, S, H, 64), qkv[..., 2 * C:].reshape(B, S, H, 64)


def caches(lens, smax=S):
    """k, v caches [B, smax, H, 64] on the device: rows [0, lens[b]) from the sequence, NaN after."""
    ks, vs = seq_kv()
    k = torch.full((B, smax, H, 64), math.nan, dtype=BF)
    v = torch.full((B, smax, H, 64), math.nan, dtype=BF)
    for b, n in enumerate(lens):
        k[b, :n], v[b, :n] = ks[b, :n], vs[b, :n]
    return k.to(DEV), v.to(DEV)


def chunk(lens, T):
    """qkv [B, T, 3C]: positions lens[b] .. of each sample, NaN where the sequence has ended."""
    qkv, _ = sequence()
    x = torch.full((B, T, 3 * C), math.nan, dtype=BF)
    for b, n in enumerate(lens):
        m = min(T, S - n)
        x[b, :m] = qkv[b, n:n + m]
    return x.to(DEV)


def check_rows(out, k, v, lens, nq, what):
    """Output rows against the full-sequence forward, the written cache rows against the sequence's k, v, and the rows
    past them still NaN."""
    _, full = sequence()
    ks, vs = seq_kv()
    out, k, v = out.cpu(), k.cpu(), v.cpu()
    for b, (ln, n) in enumerate(zip(lens, nq)):
        assert torch.equal(bits(out[b, :n]), bits(full[b, ln:ln + n])), f"{what}: sample {b} output"
        assert torch.equal(bits(out[b, n:]), torch.zeros_like(bits(out[b, n:]))), f"{what}: sample {b} dead rows"
        assert torch.equal(bits(k[b, :ln + n]), bits(ks[b, :ln + n])), f"{what}: sample {b} k rows"
        assert torch.equal(bits(v[b, :ln + n]), bits(vs[b, :ln + n])), f"{what}: sample {b} v rows"
        assert bool(torch.isnan(k[b, ln + n:]).all()) and bool(torch.isnan(v[b, ln + n:]).all()), what


# ---- 1. bits -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", SPLITS)
def test_bits_are_those_of_attention_fwd_at_every_split(L):
    T = S - L
    k, v = caches([L] * B)
    lens = i32([L] * B)
    out = dec.attention_extend(chunk([L] * B, T), k, v, lens, i32([T] * B), H, S)
    check_rows(out, k, v, [L] * B, [T] * B, f"L={L}")
    assert lens.tolist() == [L] * B  # lens is not changed


@pytest.mark.parametrize("steps", [(5, 187), (5, 91, 96)])
def test_consecutive_calls_give_the_same_bits(steps):
    k, v = caches([0] * B)
    L = 0
    for T in steps:
        out = dec.attention_extend(chunk([L] * B, T), k, v, i32([L] * B), i32([T] * B), H, L + T)
        check_rows(out, k, v, [L] * B, [T] * B, f"steps={steps} at {L}")
        L += T
    assert L == S


@functools.lru_cache(maxsize=None)
def ragged():
    """Ragged lengths in one call, each sample running to the end of its sequence."""
    T = S - min(RAGGED)
    nq = [S - n for n in RAGGED]
    k, v = caches(RAGGED)
    out = dec.attention_extend(chunk(RAGGED, T), k, v, i32(RAGGED), i32(nq), H, S)
    torch.cuda.synchronize()
    return out.cpu(), k.cpu(), v.cpu(), nq


def test_ragged_lengths_in_one_call():
    out, k, v, nq = ragged()
    check_rows(out, k, v, RAGGED, nq, "ragged")


# ---- 2. dead positions, invariance, determinism, the host bound -------------------------------------------------
def test_dead_positions_batch_invariance_determinism_and_the_host_bound():
    lens, nq, T = [10, 50, 100], [62, 0, 9], 64
    x = chunk(lens, T)
    k, v = caches(lens)
    out = dec.attention_extend(x, k, v, i32(lens), i32(nq), H, S)
    check_rows(out, k, v, lens, nq, "dead")  # dead rows exact zeros, their cache rows still NaN
    k2, v2 = caches(lens)
    again = dec.attention_extend(x, k2, v2, i32(lens), i32(nq), H, S)
    assert torch.equal(bits(again), bits(out)) and torch.equal(bits(k2), bits(k)) and torch.equal(bits(v2), bits(v))
    tight = max(ln + n for ln, n in zip(lens, nq))
    k3, v3 = caches(lens)
    bound = dec.attention_extend(x, k3, v3, i32(lens), i32(nq), H, tight)
    assert torch.equal(bits(bound), bits(out)) and torch.equal(bits(k3), bits(k))
    for b in range(B):  # a sample alone, on strided views of the batch's cache
        kb, vb = caches(lens)
        one = dec.attention_extend(x[b:b + 1], kb[b:b + 1], vb[b:b + 1], i32(lens[b:b + 1]), i32(nq[b:b + 1]), H, S)
        assert torch.equal(bits(one[0]), bits(out[b])) and torch.equal(bits(kb[b]), bits(k[b]))
    # a bound inside a sample's new positions: those at or past it are dead
    k4, v4 = caches(lens)
    cut = dec.attention_extend(x, k4, v4, i32(lens), i32(nq), H, 40)  # sample 0: rows 10..39 live; 1, 2: lens >= 40
    assert torch.equal(bits(cut[0, :30]), bits(out[0, :30])) and not bool(cut[0, 30:].float().any())
    assert not bool(cut[1:].float().any()) and bool(torch.isnan(k4[0, 40:]).all())
    assert bool(torch.isnan(k4[2, 100:]).all())
    # the twin agrees to bf16 accuracy (it defines the semantics; the bits are the kernel's own)
    kt, vt = (t.cpu() for t in caches(lens))
    twin = dec.attention_extend_ref(x.cpu(), kt, vt, i32(lens).cpu(), i32(nq).cpu(), H, S)
    torch.testing.assert_close(out.cpu().float(), twin.float(), atol=2e-2, rtol=2e-2)
    assert torch.equal(bits(kt), bits(k.cpu()))


# ---- 3. fp64 -------------------------------------------------------------------------------------------------------
def test_the_ragged_call_stays_inside_the_fp64_budget_of_attention_fwd():
    out, _, _, nq = ragged()
    qkv, _ = sequence()
    q, k, v = (qkv[..., i * C:(i + 1) * C].reshape(B, S, H, 64) for i in range(3))
    ref = gn.attention_ref64(q, k, v, SCALE, True)["y"]
    model = gn.attention_model_tiled(q, k, v, SCALE, True)["y"]
    got = torch.cat([out[b, :nq[b]].view(nq[b], H, 64) for b in range(B)])
    rows = lambda t: torch.cat([t[b, RAGGED[b]:] for b in range(B)])  # noqa: E731
    row, rms = gn.check_grouped(got, rows(model), rows(ref), name="attention_extend ragged")
    print(f"NUMERICS attention_extend ragged | y | {got.shape[0]} positions | row {row:.3f} | rms {rms:.4f}")


# ---- 4. refusals ---------------------------------------------------------------------------------------------------
def test_refusals_leave_the_cache_alone():
    lens, nq = i32([1, 57, 120]), i32([2, 2, 2])
    k, v = rnd(B, S, H, 64, seed=1).to(DEV), rnd(B, S, H, 64, seed=2).to(DEV)
    k0 = k.clone()
    q = rnd(B, 2, 3 * C, seed=3).to(DEV)
    k32 = rnd(B, S, 4, 32, seed=5).to(DEV)
    for args, msg in (((q, k, v, lens, nq, SCALE, 0), "n_keys"),
                      ((q, k, v, lens, nq, SCALE, S + 1), "n_keys"),
                      ((q[:, :0], k, v, lens, nq, SCALE, S), "at least 1"),
                      ((q, k32, k32.clone(), lens, nq, SCALE, S), "head width 64"),
                      ((q, k, v, lens.long(), nq, SCALE, S), "lens must be int32"),
                      ((q, k, v, lens, nq.long(), SCALE, S), "nq must be int32"),
                      ((q, k, v, lens[:2], nq, SCALE, S), "lens must be int32"),
                      ((q.float(), k, v, lens, nq, SCALE, S), "bf16"),
                      ((q, k, v.float(), lens, nq, SCALE, S), "bf16"),
                      ((q, k, v, lens.cpu(), nq, SCALE, S), "one device"),
                      ((q[:, :, 1:], k, v, lens, nq, SCALE, S), "does not match"),
                      ((q, k[..., ::2], v[..., ::2], lens, nq, SCALE, S), "head width 64")):
        with pytest.raises(RuntimeError, match=msg):
            K.attention_extend(*args)
    for args in ((q, k, v, lens, nq, H, 0), (q, k, v, lens, nq, H, S + 1), (q, k, v, lens.long(), nq, H, S),
                 (q, k, v, lens, nq[:2], H, S), (q.float(), k, v, lens, nq, H, S), (q[:, :, 1:], k, v, lens, nq, H, S),
                 (q[:, :0], k, v, lens, nq, H, S), (q, k, v[:, :100], lens, nq, H, S)):
        with pytest.raises(ValueError, match="attention_extend"):
            dec.attention_extend(*args)
    torch.cuda.synchronize()
    assert torch.equal(k, k0)
