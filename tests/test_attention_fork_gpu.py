"""attention_fork (one new token for each of G n rows, n siblings sharing a group's prefix cache) on the GPU: its bit
contract with attention_decode on the materialised cache (outputs and written rows), n = 1 as attention_decode itself,
the host bound, group invariance, determinism, the twin and the refusals. The tails of both caches hold NaN patterns
throughout."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no ROCm GPU", allow_module_level=True)

import fork_util as fu  # noqa: E402
from fork_util import C, G, H, NMAX, PMAX, SCALE, bits  # noqa: E402
from simple_distributed_machine_learning_amd import _native  # noqa: E402
from simple_distributed_machine_learning_amd.ops import decode as dec  # noqa: E402

DEV = torch.device("cuda", 0)
K = _native.kernels()
CASES = range(len(fu.PLENS))


@functools.lru_cache(maxsize=None)
def case(n, i, n_keys=PMAX + NMAX):
    """Inputs of case i at n samples per group, attention_fork's results, and the reference: attention_decode on the
    materialised [R, Pmax + Nmax] cache. Computed once, left unchanged."""
    qkv, kp, vp, plens, ks, vs, suf, lens = fu.fork_inputs(n, i)
    kpd, vpd, ksd, vsd = kp.to(DEV), vp.to(DEV), ks.to(DEV), vs.to(DEV)
    plens_d, lens_d = fu.i32(plens, DEV), fu.i32(lens, DEV)
    out = dec.attention_fork(qkv.to(DEV), kpd, vpd, plens_d, ksd, vsd, lens_d, n, H, n_keys)
    kf, vf = fu.materialise(kp, ks, plens, suf, n).to(DEV), fu.materialise(vp, vs, plens, suf, n).to(DEV)
    ref = K.attention_decode(qkv.to(DEV), kf, vf, lens_d, SCALE, PMAX + NMAX)
    torch.cuda.synchronize()
    assert lens_d.tolist() == lens and plens_d.tolist() == list(plens)  # the lengths are not changed
    return dict(qkv=qkv, kp0=kp, vp0=vp, ks0=ks, vs0=vs, plens=plens, suf=suf, lens=lens, out=out.cpu(), ref=ref.cpu(),
                kp=kpd.cpu(), vp=vpd.cpu(), ks=ksd.cpu(), vs=vsd.cpu(), kf=kf.cpu(), vf=vf.cpu())


def test_the_cases_cover_the_paths():
    """A condition on the inputs: whole prompt chunks (0, 1, 2), chunks that straddle plens[g], a new key on both sides
    of the 64- and 128-key edges."""
    shared, straddle, new = set(), set(), set()
    for n in fu.NS:
        for i in CASES:
            _, _, _, plens, _, _, suf, lens = fu.fork_inputs(n, i)
            for r, ln in enumerate(lens):
                p = plens[r // n]
                shared.add(p // 64)
                straddle.add(p % 64 != 0 and suf[r] > 0)  # the chunk of plens[g] holds prefix, suffix and new keys
                new.add(ln)
    assert shared == {0, 1, 2} and True in straddle and {63, 64, 65, 127, 128, 129} <= new, (shared, sorted(new))


# ---- 1. bits -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", fu.NS)
def test_bits_are_those_of_attention_decode_on_the_materialised_cache(n):
    for i in CASES:
        c = case(n, i)
        for r in range(G * n):
            p, s = c["plens"][r // n], c["suf"][r]
            what = f"n={n} plens={c['plens']} suffix={c['suf']} row {r}"
            assert torch.equal(bits(c["out"][r]), bits(c["ref"][r])), what
            for got, orig, full, off in ((c["ks"], c["ks0"], c["kf"], C), (c["vs"], c["vs0"], c["vf"], 2 * C)):
                # the written suffix row: the row's qkv bits, which is what attention_decode wrote at row lens[r]
                assert torch.equal(bits(got[r, s].reshape(C)), bits(c["qkv"][r, off:off + C])), what
                assert torch.equal(bits(got[r, s]), bits(full[r, p + s])), what
                # every other suffix row is untouched, NaN tails included
                assert torch.equal(bits(got[r, :s]), bits(orig[r, :s])), what
                assert torch.equal(bits(got[r, s + 1:]), bits(orig[r, s + 1:])), what
                assert bool(torch.isnan(got[r, s + 1:]).all()), what
        assert torch.equal(bits(c["kp"]), bits(c["kp0"])) and torch.equal(bits(c["vp"]), bits(c["vp0"]))
        assert bool(torch.isfinite(c["out"].float()).all())


# ---- 2. n = 1 ------------------------------------------------------------------------------------------------------
def test_one_sample_is_attention_decode_itself():
    """One cache of Smax rows split into prefix rows [0, plens) and suffix rows: the outputs and the new row are those of
    attention_decode on the unsplit cache; also with an empty prefix."""
    smax = PMAX
    q = fu.rnd(G, 3 * C, seed=77).to(DEV)
    k0, v0 = fu.rnd(G, smax, H, 64, seed=78), fu.rnd(G, smax, H, 64, seed=79)
    for lens_h in fu.PLENS:
        lens = fu.i32(lens_h, DEV)
        kd, vd = fu.nan_tail(k0, lens_h).to(DEV), fu.nan_tail(v0, lens_h).to(DEV)
        want = K.attention_decode(q, kd, vd, lens, SCALE, smax)
        for plens_h in ([ln - min(ln, s) for ln, s in zip(lens_h, (0, 3, 64))], [1] * G, [0] * G):
            kp = fu.nan_tail(k0, plens_h).to(DEV)
            vp = fu.nan_tail(v0, plens_h).to(DEV)
            ks = torch.full((G, NMAX + smax, H, 64), float("nan"), dtype=k0.dtype, device=DEV)
            vs = ks.clone()
            for g, (p, ln) in enumerate(zip(plens_h, lens_h)):
                ks[g, :ln - p], vs[g, :ln - p] = k0[g, p:ln].to(DEV), v0[g, p:ln].to(DEV)
            got = dec.attention_fork(q, kp, vp, fu.i32(plens_h, DEV), ks, vs, lens, 1, H, smax)
            assert torch.equal(bits(got), bits(want)), (lens_h, plens_h)
            for g, (p, ln) in enumerate(zip(plens_h, lens_h)):
                assert torch.equal(bits(ks[g, ln - p]), bits(kd[g, ln])), (lens_h, plens_h)
                assert torch.equal(bits(vs[g, ln - p]), bits(vd[g, ln])), (lens_h, plens_h)


# ---- 3. the host bound ---------------------------------------------------------------------------------------------
def test_the_host_bound_does_not_change_the_bits():
    """n_keys only sizes the grid and the workspace."""
    for n, i in ((2, 0), (8, 2), (3, 6)):
        c = case(n, i)
        t = case(n, i, max(c["lens"]) + 1)
        for key in ("out", "ks", "vs", "kp", "vp"):
            assert torch.equal(bits(t[key]), bits(c[key])), (n, i, key)


# ---- 4. invariance and determinism ---------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 8])
def test_group_invariance_determinism_and_the_twin(n):
    c = case(n, 0)
    q = c["qkv"].to(DEV)
    plens, lens = fu.i32(c["plens"], DEV), fu.i32(c["lens"], DEV)
    ks, vs = c["ks0"].to(DEV), c["vs0"].to(DEV)
    again = dec.attention_fork(q, c["kp0"].to(DEV), c["vp0"].to(DEV), plens, ks, vs, lens, n, H, PMAX + NMAX)
    assert torch.equal(bits(again.cpu()), bits(c["out"]))  # two runs
    assert torch.equal(bits(ks.cpu()), bits(c["ks"])) and torch.equal(bits(vs.cpu()), bits(c["vs"]))
    for i in (0, 2, 6):  # a group alone, on strided views of the batch's caches
        c = case(n, i)
        q = c["qkv"].to(DEV)
        plens, lens = fu.i32(c["plens"], DEV), fu.i32(c["lens"], DEV)
        for g in range(G):
            kp, vp, ks, vs = c["kp0"].to(DEV), c["vp0"].to(DEV), c["ks0"].to(DEV), c["vs0"].to(DEV)
            rows = slice(g * n, g * n + n)
            one = dec.attention_fork(q[rows], kp[g:g + 1], vp[g:g + 1], plens[g:g + 1], ks[rows], vs[rows], lens[rows],
                                     n, H, PMAX + NMAX)
            assert torch.equal(bits(one.cpu()), bits(c["out"][rows])), (n, i, g)
            assert torch.equal(bits(ks[rows].cpu()), bits(c["ks"][rows])), (n, i, g)
            assert torch.equal(bits(vs[rows].cpu()), bits(c["vs"][rows])), (n, i, g)
        # views with other strides: every second row of caches twice as long, and qkv inside a wider matrix
        wide = lambda t: torch.stack([t, torch.zeros_like(t)], 2).flatten(1, 2).to(DEV)  # noqa: E731
        kp, vp, ks, vs = wide(c["kp0"]), wide(c["vp0"]), wide(c["ks0"]), wide(c["vs0"])
        qw = torch.zeros(G * n, 3 * C + 8, dtype=q.dtype, device=DEV)
        qw[:, :3 * C] = q
        got = dec.attention_fork(qw[:, :3 * C], kp[:, ::2], vp[:, ::2], plens, ks[:, ::2], vs[:, ::2], lens, n, H,
                                 PMAX + NMAX)
        assert torch.equal(bits(got.cpu()), bits(c["out"])), (n, i)
        assert torch.equal(bits(ks[:, ::2].cpu()), bits(c["ks"])) and not bool(ks[:, 1::2].any())
    # the twin agrees to bf16 accuracy (it defines the semantics; the bits are the kernel's own)
    c = case(n, 0)
    kt, vt = c["ks0"].clone(), c["vs0"].clone()
    twin = dec.attention_fork_ref(c["qkv"], c["kp0"], c["vp0"], fu.i32(c["plens"]), kt, vt, fu.i32(c["lens"]), n, H,
                                  PMAX + NMAX)
    torch.testing.assert_close(c["out"].float(), twin.float(), atol=2e-2, rtol=2e-2)
    assert torch.equal(bits(kt), bits(c["ks"])) and torch.equal(bits(vt), bits(c["vs"]))


# ---- 5. refusals ---------------------------------------------------------------------------------------------------
def test_refusals_leave_both_caches_alone():
    n = 2
    R = G * n
    plens, lens = fu.i32([1, 57, 120], DEV), fu.i32([1, 2, 57, 60, 120, 185], DEV)
    kp, vp = fu.rnd(G, PMAX, H, 64, seed=1).to(DEV), fu.rnd(G, PMAX, H, 64, seed=2).to(DEV)
    ks, vs = fu.rnd(R, NMAX, H, 64, seed=3).to(DEV), fu.rnd(R, NMAX, H, 64, seed=4).to(DEV)
    kp0, vp0, ks0, vs0 = kp.clone(), vp.clone(), ks.clone(), vs.clone()
    q = fu.rnd(R, 3 * C, seed=5).to(DEV)
    kp32, ks32 = fu.rnd(G, PMAX, 4, 32, seed=6).to(DEV), fu.rnd(R, NMAX, 4, 32, seed=7).to(DEV)
    NK = PMAX + NMAX
    for args, msg in (((q, kp, vp, plens, ks, vs, lens, 0, SCALE, NK), "n = 0"),
                      ((q, kp, vp, plens, ks, vs, lens, 65, SCALE, NK), "n = 65"),
                      ((q, kp, vp, plens, ks, vs, lens, 3, SCALE, NK), "do not match"),
                      ((q[:5], kp, vp, plens, ks[:5], vs[:5], lens[:5], n, SCALE, NK), "do not match"),
                      ((q, kp, vp, plens, ks[:5], vs[:5], lens, n, SCALE, NK), "do not match"),
                      ((q[:, 8:], kp, vp, plens, ks, vs, lens, n, SCALE, NK), "do not match"),
                      ((q, kp, vp, plens, ks, vs, lens, n, SCALE, 0), "n_keys"),
                      ((q, kp, vp, plens, ks, vs, lens, n, SCALE, NK + 1), "n_keys"),
                      ((q, kp32, kp32.clone(), plens, ks32, ks32.clone(), lens, n, SCALE, NK), "head width 64"),
                      ((q, kp[..., ::2], vp[..., ::2], plens, ks, vs, lens, n, SCALE, NK), "head width 64"),
                      ((q, kp, vp, plens, ks[..., 1:], vs[..., 1:], lens, n, SCALE, NK), "head width 64"),
                      ((q, kp, vp, plens.long(), ks, vs, lens, n, SCALE, NK), "plens must be int32"),
                      ((q, kp, vp, plens, ks, vs, lens.long(), n, SCALE, NK), "lens must be int32"),
                      ((q, kp, vp, plens[:2], ks, vs, lens, n, SCALE, NK), "plens must be int32"),
                      ((q, kp, vp, plens, ks, vs, lens[:5], n, SCALE, NK), "lens must be int32"),
                      ((q.float(), kp, vp, plens, ks, vs, lens, n, SCALE, NK), "bf16"),
                      ((q, kp, vp.float(), plens, ks, vs, lens, n, SCALE, NK), "bf16"),
                      ((q, kp, vp, plens, ks.float(), vs.float(), lens, n, SCALE, NK), "bf16"),
                      ((q, kp, vp, plens.cpu(), ks, vs, lens, n, SCALE, NK), "one device"),
                      ((q, kp, vp, plens, ks, vs, lens.cpu(), n, SCALE, NK), "one device"),
                      ((q, kp, vp, plens, ks.cpu(), vs.cpu(), lens, n, SCALE, NK), "device"),
                      ((q.t().contiguous().t(), kp, vp, plens, ks, vs, lens, n, SCALE, NK), "unit column stride"),
                      ((q, kp, vp.transpose(1, 2).contiguous().transpose(1, 2), plens, ks, vs, lens, n, SCALE, NK),
                       "one layout"),
                      ((q, kp, vp, plens, ks[:, :, :, 4:], vs[:, :, :, 4:], lens, n, SCALE, NK), "head width 64")):
        with pytest.raises(RuntimeError, match=msg):
            K.attention_fork(*args)
    for args in ((q, kp, vp, plens, ks, vs, lens, 0, H, NK), (q, kp, vp, plens, ks, vs, lens, 65, H, NK),
                 (q, kp, vp, plens, ks, vs, lens, 2.0, H, NK), (q, kp, vp, plens, ks, vs, lens, 3, H, NK),
                 (q, kp, vp, plens, ks, vs, lens, n, H, 0), (q, kp, vp, plens, ks, vs, lens, n, H, NK + 1),
                 (q, kp, vp, plens.long(), ks, vs, lens, n, H, NK), (q, kp, vp, plens, ks, vs, lens[:5], n, H, NK),
                 (q.float(), kp, vp, plens, ks, vs, lens, n, H, NK), (q, kp, vp, plens, ks.cpu(), vs.cpu(), lens, n, H, NK),
                 (q, kp, vp.transpose(1, 2).contiguous().transpose(1, 2), plens, ks, vs, lens, n, H, NK)):
        with pytest.raises(ValueError, match="attention_fork"):
            dec.attention_fork(*args)
    torch.cuda.synchronize()
    for t, t0 in ((kp, kp0), (vp, vp0), (ks, ks0), (vs, vs0)):
        assert torch.equal(t, t0)


def test_rows_outside_the_caches_are_not_indexed():
    """Lengths the host cannot check (they live on the device): a row whose suffix is full, whose length lies below its
    prompt's or past n_keys, or whose prompt lies outside the prefix cache writes nothing; the other rows are
    unchanged."""
    n, i = 2, 1
    c = case(n, i)
    bad = {0: ("lens", c["plens"][0] + NMAX), 3: ("lens", c["plens"][1] - 1), 4: ("plens", PMAX + 1)}
    plens, lens = list(c["plens"]), list(c["lens"])
    for r, (what, v) in bad.items():
        if what == "lens":
            lens[r] = v
        else:
            plens[r // n] = v
    dead = {0, 3, 4, 5}  # (group 2's prompt length is out of range: both of its rows)
    ks, vs = c["ks0"].to(DEV), c["vs0"].to(DEV)
    kp, vp = c["kp0"].to(DEV), c["vp0"].to(DEV)
    out = dec.attention_fork(c["qkv"].to(DEV), kp, vp, fu.i32(plens, DEV), ks, vs, fu.i32(lens, DEV), n, H,
                             PMAX + NMAX).cpu()
    torch.cuda.synchronize()
    for r in range(G * n):
        if r in dead:
            assert torch.equal(bits(ks[r].cpu()), bits(c["ks0"][r])) and torch.equal(bits(vs[r].cpu()), bits(c["vs0"][r]))
        else:
            assert torch.equal(bits(out[r]), bits(c["out"][r])) and torch.equal(bits(ks[r].cpu()), bits(c["ks"][r]))
    assert torch.equal(bits(kp.cpu()), bits(c["kp0"]))
