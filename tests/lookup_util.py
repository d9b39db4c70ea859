"""Shared pieces of the prompt-lookup tests: draft + accept in plain Python integers (independent of the torch twin in
ops/reference.py and of the kernel), the cases of the lookup_step tests, and the step simulation that turns a finished
sequence into the number of verify steps its row must have taken."""
from __future__ import annotations

import random

import torch

PAD, EOS, W = 0, 9, 40


# ---- plain Python ---------------------------------------------------------------------------------------------------
def py_drafts(hist, N, K, limit):
    """Drafts for a history (list of ints, the newest token last): what followed the most recent earlier occurrence
    of its last N tokens, at most K, no further than the history's end, leaving room below ``limit`` for the token
    after the drafts."""
    L = len(hist) - 1
    if L < N:
        return []
    tail = hist[L - N + 1:]
    for s in range(L - N, -1, -1):
        if hist[s:s + N] == tail:
            n = max(0, min(K, L - s - N + 1, limit - 2 - L))
            return hist[s + N:s + N + n]
    return []


def py_step(rows, g, K, N, eos=EOS, pad=PAD, width=W):
    """One lookup_step on ``rows`` (dicts: out list, lens, limit, done, gen_len, row_steps, tok_in list, nq_in) with the
    sampler's tokens g (list of K + 1 per row, or None: nothing to accept). Changes the rows in place and returns
    (tok_next, nq_next, all_done)."""
    tok_next, nq_next = [], []
    for b, r in enumerate(rows):
        lim = min(r["limit"], width)
        L = r["lens"]
        if g is not None and not r["done"] and L + 1 < lim:
            drafts = r["tok_in"][1:r["nq_in"]]
            a = 0
            while a < len(drafts) and drafts[a] == g[b][a]:
                a += 1
            emit = g[b][:a + 1][:lim - 1 - L]
            if eos in emit:
                emit = emit[:emit.index(eos) + 1]
                r["done"] = 1
            r["out"][L + 1:L + 1 + len(emit)] = emit
            L += len(emit)
            r["lens"] = L
            r["gen_len"] += len(emit)
            r["row_steps"] += 1
        if r["done"] or L + 1 >= lim:
            tok_next.append([pad] * (K + 1))
            nq_next.append(0)
            continue
        d = py_drafts(r["out"][:L + 1], N, K, lim)
        tok_next.append([r["out"][L]] + d + [pad] * (K - len(d)))
        nq_next.append(1 + len(d))
    return tok_next, nq_next, int(not any(nq_next))


def simulate_row_steps(seq, prompt_len, limit, K, N, eos=None):
    """Verify steps in which a row emitted a token, from its finished sequence alone: an accepted draft is the token the
    plain loop drew, so the sampler's tokens of a step are the sequence's next ones. ``seq``: the row's tokens (list),
    valid up to its final length; the first generated token (column prompt_len) comes from the prefill."""
    L, steps = prompt_len, 0
    done = eos is not None and seq[L] == eos
    while not done and L + 1 < limit:
        d = py_drafts(seq[:L + 1], N, K, limit)
        a = 0
        while a < len(d) and d[a] == seq[L + 1 + a]:
            a += 1
        emit = seq[L + 1:L + 2 + a][:limit - 1 - L]
        if eos is not None and eos in emit:
            emit = emit[:emit.index(eos) + 1]
            done = True
        L += len(emit)
        steps += 1
    return steps


# ---- the cases of the lookup_step tests ---------------------------------------------------------------------------
def _row(hist, limit, tok_drafts=(), done=0, gen_len=3, row_steps=2, K=3):
    out = list(hist) + [PAD] * (W - len(hist))
    d = list(tok_drafts)[:K]
    return dict(out=out, lens=len(hist) - 1, limit=limit, done=done, gen_len=gen_len, row_steps=row_steps,
                tok_in=[hist[-1]] + d + [PAD] * (K - len(d)), nq_in=1 + len(d))


def lookup_cases(K, N, seed=0):
    """(rows, g, tags): a batch of hand-built rows, one per situation the kernel must handle, then random rows over a
    three-token alphabet (many matches). g [B][K + 1] is built per row to give the tagged acceptance."""
    rows, g, tags = [], [], []

    def add(tag, row, gs):
        rows.append(row)
        g.append((list(gs) + [7] * (K + 1))[:K + 1])
        tags.append(tag)

    rep = [1, 2, 3, 1, 2, 4, 1, 2, 5, 1, 2]
    d3 = [5, 1, 2]
    add("no match", _row([1, 2, 3, 4, 5, 6, 7, 8], 30, K=K), [3])
    add("several matches, the most recent wins", _row(rep, 30, K=K), [6])
    add("history shorter than N + 1", _row([5], 30, K=K), [5])
    add("history of N + 1 equal tokens", _row([5] * (N + 1), 30, K=K), [5, 5])
    gram = list(range(1, N + 1))
    add("drafts cut by the history's end", _row(gram + [8] + gram, 30, K=K), [4])  # N + 1 tokens follow the match
    add("drafts cut by limit (one left)", _row(rep, len(rep) + 2, K=K), [1, 2])
    add("drafts cut by limit (none left)", _row(rep, len(rep) + 1, K=K), [3])
    add("partial acceptance", _row(rep, 30, d3, K=K), [d3[0], 8, 8, 8])
    add("no draft accepted", _row(rep, 30, d3, K=K), [8, 1, 2, 6])
    add("full acceptance and the bonus token", _row(rep, 30, d3, K=K), d3[:K] + [6])
    add("full acceptance into a repeat", _row(rep, 30, d3, K=K), d3[:K] + [1] if K < 3 else d3 + [5])
    add("an eos in the middle of an accepted run", _row(rep, 30, [5, EOS, 2], K=K), [5, EOS, 2, 6])
    add("an eos as the first token", _row(rep, 30, d3, K=K), [EOS, 1, 2, 6])
    add("accepted run cut by limit", _row(rep, len(rep) + 2, d3, K=K), d3[:K] + [6])
    add("a done row", _row(rep, 30, d3, done=1, K=K), d3[:K] + [6])
    add("a full row", _row(rep, len(rep), d3, K=K), d3[:K] + [6])
    add("a row one short of full", _row(rep, len(rep) + 1, d3, K=K), d3[:K] + [6])
    rng = random.Random(seed * 131 + K * 17 + N)
    for i in range(23):
        n_h = rng.randint(1, 30)
        hist = [rng.randint(1, 3) for _ in range(n_h)]
        limit = rng.choice([n_h, n_h + 1, n_h + 2, n_h + 5, W, W + 3])
        d = py_drafts(hist, N, K, min(limit, W)) if rng.random() < 0.7 else [rng.randint(1, 3) for _ in range(K)]
        gs = [(t if rng.random() < 0.75 else rng.randint(1, 3)) for t in d]
        gs += [rng.choice([1, 2, 3, EOS]) for _ in range(K + 1 - len(gs))]
        add(f"random {i}", _row(hist, limit, d, done=int(rng.random() < 0.1), gen_len=rng.randint(1, 5),
                                row_steps=rng.randint(0, 5), K=K), gs)
    return rows, g, tags


def to_tensors(rows, g, device="cpu"):
    """The rows as lookup_step's tensors: (g, tok_in, nq_in, out, lens, limit, done, gen_len, row_steps)."""
    i32 = lambda k: torch.tensor([r[k] for r in rows], dtype=torch.int32, device=device)  # noqa: E731
    i64 = lambda v: torch.tensor(v, dtype=torch.int64, device=device)  # noqa: E731
    return (None if g is None else i64(g), i64([r["tok_in"] for r in rows]), i32("nq_in"),
            i64([r["out"] for r in rows]), i32("lens"), i32("limit"), i32("done"), i32("gen_len"), i32("row_steps"))


def check_against_python(step_fn, K, N, device="cpu", accept=True, seed=0, subset=None):
    """Run ``step_fn`` (lookup_step's signature) on the cases and require every cell of its results and of the state
    to equal the plain-Python step. Returns (rows before, rows after, tags, nq_next)."""
    import copy

    rows, g, tags = lookup_cases(K, N, seed)
    if subset is not None:
        rows, g, tags = [rows[i] for i in subset], [g[i] for i in subset], [tags[i] for i in subset]
    before = copy.deepcopy(rows)
    gt, tok_in, nq_in, out, lens, limit, done, gen_len, row_steps = to_tensors(rows, g if accept else None, device)
    if not accept:
        tok_in = nq_in = None
    tok_next, nq_next, flag = step_fn(gt, tok_in, nq_in, out, lens, limit, done, gen_len, row_steps, K, N, EOS, PAD)
    want_tok, want_nq, want_flag = py_step(rows, g if accept else None, K, N)
    for b, (r, tag) in enumerate(zip(rows, tags)):
        what = f"K={K} N={N} row {b} ({tag})"
        assert out[b].tolist() == r["out"], what
        got = dict(lens=int(lens[b]), done=int(done[b]), gen_len=int(gen_len[b]), row_steps=int(row_steps[b]))
        assert got == {k: r[k] for k in got}, (what, got, r)
        assert int(nq_next[b]) == want_nq[b] and tok_next[b].tolist() == want_tok[b], (what, tok_next[b].tolist(),
                                                                                         want_tok[b])
    assert flag.tolist() == [want_flag] and flag.dtype == torch.int32 and nq_next.dtype == torch.int32
    assert tok_next.dtype == torch.int64 and tuple(tok_next.shape) == (len(rows), K + 1)
    return before, rows, tags, want_nq


# ---- generation ---------------------------------------------------------------------------------------------------
def rule_prompts(starts, length=8):
    """[len(starts), length] int64 prompts that follow the synthetic data's rule t' = (62 t + 26) mod 97. The map has
    order 6 (62^3 = -1 mod 97), so every sequence but the fixed point's has period 6: an 8-token prompt holds its last
    two tokens once before, and what followed them is what the rule brings next."""
    from generate_util import RULE_A, RULE_B, VOCAB

    rows = []
    for t in starts:
        row = [int(t)]
        while len(row) < length:
            row.append((row[-1] * RULE_A + RULE_B) % VOCAB)
        assert row[6] == row[0] and row[1] != row[0], "a start on the rule's fixed point"
        rows.append(row)
    return torch.tensor(rows, dtype=torch.int64)


def check_row_steps(tokens, lengths, stats, prompt_lens, new, K, N, eos=None):
    """``row_steps`` and ``generated`` of a lookup run against the simulation on its own result. Returns the steps."""
    toks, lens = tokens.cpu().tolist(), lengths.cpu().tolist()
    want = [simulate_row_steps(toks[b], prompt_lens[b], prompt_lens[b] + new, K, N, eos) for b in range(len(toks))]
    assert stats["row_steps"].cpu().tolist() == want, (stats["row_steps"].cpu().tolist(), want)
    assert stats["generated"].cpu().tolist() == [n - p for n, p in zip(lens, prompt_lens)]
    assert max(want) <= stats["steps"] <= max(new - 1, 0)
    return want


def lookup_pp_refusal_worker(rank, world, model, dtype):
    """One rank of a two-rank pipeline: lookup > 0 must be refused on every rank before anything is exchanged."""
    from generate_util import make_engine
    from simple_distributed_machine_learning_amd.parallel.generate import generate

    eng = make_engine(model, "cpu", dtype, rank, world, pp=world, kind="gpipe", backend="gloo")
    try:
        generate(eng, rule_prompts([1, 2]), 4, lookup=3)
    except ValueError as e:
        return str(e)
    return "no refusal"


def make_engine_d64(device, dtype, block_size=192, seed=1, lr=3e-3):
    """generate_util's "gpt2_d64" config (2 layers, 2 heads of width 64, vocabulary 97) with another block_size, one
    process: a cache that crosses the decode attention's 64- and 128-key chunk edges end to end."""
    from generate_util import VOCAB
    from simple_distributed_machine_learning_amd.models.gpt2 import GPT2Config, gpt2_spec
    from simple_distributed_machine_learning_amd.parallel import PipelineEngine, init_mesh

    cfg = GPT2Config(n_layer=2, n_head=2, n_embd=128, vocab_size=VOCAB, block_size=block_size)
    spec = gpt2_spec(2, cfg=cfg, seq_len=32, dtype=dtype, name=f"gpt2_d64_b{block_size}")
    mesh = init_mesh(pp=1, schedule_kind="1f1b", rank=0, world_size=1, device=torch.device(device), timeout_s=120)
    return PipelineEngine(spec, mesh, schedule_kind="1f1b", num_microbatches=1, lr=lr, seed=seed, optimizer="adamw")
