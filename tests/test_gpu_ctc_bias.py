"""GPU: contextual biasing of the CTC prefix beam search, one-shot form (csrc/ctc_beam_bias.hip; ops.ctc_beam_decode(bias=)) — against the enumeration of every label
sequence where nothing is pruned, bit-equal to the unbiased search at weight 0, against the float64 restatement on the draws tests/test_ctc_bias_cpu.py certifies, over
batches, lengths and dtypes, at the edges of the tables, with a malformed context handed to the C entry, and through engine.transcribe."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import ctc_beam_ref as R  # noqa: E402
import ctc_bias_ref as BR  # noqa: E402
from test_ctc_bias_cpu import LISTS, SMALL, small_logits  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAD = -5
SCORE_TOL = 1e-3                                                           # the project's bar for fp32 accumulation over T <= 64 (tests/test_gpu_ctc_beam.py)
DRAWS = 12
KEYS = ("tokens", "n_tokens", "scores", "frames")


def context(phrases, w, V1, blank):
    from huggingface_asr_amd.ctc_bias import CtcBias
    return CtcBias(phrases, w, V1, blank)


def decode(x, blank, lengths=None, **kw):
    from huggingface_asr_amd import ops
    out = ops.ctc_beam_decode(torch.as_tensor(x).to(DEV), blank, PAD, None if lengths is None else torch.as_tensor(lengths, dtype=torch.int32).to(DEV), **kw)
    return {k: v.cpu().numpy() for k, v in out.items()}


def rows_of(out, b):
    """[(labels, score, credit)] of utterance b's rows that exist; rows that do not: 0 tokens, -inf, credit 0, pad"""
    res = []
    for r in range(out["tokens"].shape[1]):
        n, sc, cr = int(out["n_tokens"][b, r]), float(out["scores"][b, r]), int(out["credit"][b, r])
        assert (out["tokens"][b, r, n:] == PAD).all()
        if sc == float("-inf"):
            assert n == 0 and cr == 0 and all(float(s) == float("-inf") for s in out["scores"][b, r:])
            continue
        res.append((tuple(int(v) for v in out["tokens"][b, r, :n]), sc, cr))
    return res


def check_invariants(out, b, ctx, x=None, n=None):
    """what holds whatever the margins: every credit is the host walk's of its tokens, the rows are distinct and ordered by the fp32 biased value, and a score is at most
    its hypothesis' exact CTC log-probability"""
    rows = rows_of(out, b)
    assert len({r[0] for r in rows}) == len(rows)
    w = np.float32(ctx.weight)
    vals = [np.float32(sc) + w * np.float32(cr) for _, sc, cr in rows]
    assert all(a >= c for a, c in zip(vals, vals[1:])), vals
    for labels, sc, cr in rows:
        assert cr == ctx.credit(labels), (labels, cr)
        if x is not None:
            assert sc <= R.ctc_logp(R.log_softmax(np.asarray(x, dtype=np.float64)[:n]), labels, ctx.blank) + SCORE_TOL
    return rows


# ------------------------------------------------------------------------------------------------ 1. nothing pruned: the enumeration
@functools.lru_cache(maxsize=None)
def exhaustive(T, V1):
    x = np.stack([small_logits(T, V1, s) for s in range(DRAWS)])
    return x


@pytest.mark.parametrize("w", [0.5, 2.0, -1.0])
@pytest.mark.parametrize("T,V1", SMALL)
def test_nothing_pruned_equals_the_biased_enumeration(T, V1, w):
    blank = V1 - 1
    x = exhaustive(T, V1)
    kept = 0
    for li in range(3):                                                    # three phrase lists, each over a third of the draws in one launch
        phrases = [p for p in LISTS[li] if max(p) < blank]
        draws = [s for s in range(DRAWS) if s % 3 == li]
        out = decode(x[draws], blank, beams=64, token_topk=V1 - 1, nbest=8, bias=context(phrases, w, V1, blank))
        assert out["credit"].shape == (len(draws), 8) and out["credit"].dtype == np.int32
        for b, s in enumerate(draws):
            want = BR.enumerate_all(x[s], blank, phrases, w)
            top = want[:9]
            got = rows_of(out, b)
            assert len(got) == min(8, len(want))
            vals = [BR.biased(e[1], w, e[2]) for e in top]
            if any(a - c < 2e-3 for a, c in zip(vals, vals[1:])):          # two fp32 values within SCORE_TOL of their exact ones can swap: the order is then not defined
                continue
            kept += 1
            assert [g[0] for g in got] == [e[0] for e in top[:8]], (s, got, top)
            for (labels, sc, cr), (_, exact, n) in zip(got, top):
                print(f"T={T} V1={V1} w={w} draw {s}: {labels} device {sc:.6f} exact {exact:.6f} credit {cr}")
                assert cr == n and abs(sc - exact) <= SCORE_TOL
    assert kept * 3 >= DRAWS * 2, kept


# ------------------------------------------------------------------------------------------------ 2. weight 0: the unbiased search, bit for bit
@pytest.mark.parametrize("B,T,V1,W,K", [(3, 48, 40, 8, 8), (2, 300, 301, 64, 24)])
def test_zero_weight_is_bit_equal_to_the_unbiased_search(B, T, V1, W, K):
    x = np.stack([R.peaky(500 + b, T, V1, V1 - 1) for b in range(B)])
    rng = np.random.default_rng(5)
    phrases = [list(R.greedy(x[0], V1 - 1)[1:4])] + [[int(t) for t in rng.integers(0, V1 - 1, size=3)] for _ in range(20)]
    kw = dict(beams=W, token_topk=K, nbest=4, return_frames=True)
    plain = decode(x, V1 - 1, **kw)
    zero = decode(x, V1 - 1, bias=context(phrases, 0.0, V1, V1 - 1), **kw)
    empty = decode(x, V1 - 1, bias=context([], 3.0, V1, V1 - 1), **kw)
    for k in KEYS:
        assert np.array_equal(plain[k], zero[k]) and np.array_equal(plain[k], empty[k]), k
    assert (empty["credit"] == 0).all() and zero["credit"].max() > 0
    ctx = context(phrases, 0.0, V1, V1 - 1)
    for b in range(B):
        check_invariants(zero, b, ctx)


# ------------------------------------------------------------------------------------------------ 3. certified draws: the float64 restatement
@pytest.mark.parametrize("w", BR.CERT_WEIGHTS)
def test_certified_draws_match_the_float64_restatement(w):
    c = BR
    cases = [c.cert_case(s) for s in c.CERT_SEEDS]
    for seed, (x, blank, phrases) in zip(c.CERT_SEEDS, cases):
        ref = c.beam_search(x, blank, c.CERT_W, c.CERT_K, nbest=c.CERT_NBEST, phrases=phrases, w=w)
        assert c.min_margin(ref) >= c.CERT_MARGIN                          # (certified on the CPU: tests/test_ctc_bias_cpu.py)
        out = decode(x[None], blank, beams=c.CERT_W, token_topk=c.CERT_K, nbest=c.CERT_NBEST, return_frames=True, bias=context(phrases, w, c.CERT_V1, blank))
        got = rows_of(out, 0)
        assert [g[0] for g in got] == [h[0] for h in ref["hyps"]], seed
        for r, ((labels, sc, cr), (_, want, frames, n)) in enumerate(zip(got, ref["hyps"])):
            print(f"certified draw {seed} w={w}: {len(labels)} tokens, device {sc:.6f} float64 {want:.6f} credit {cr}")
            assert cr == n and abs(sc - want) <= SCORE_TOL
            assert out["frames"][0, r, :len(frames)].tolist() == frames


# ------------------------------------------------------------------------------------------------ 4. batch, lengths, dtype, reproducibility
def test_batch_independence_lengths_bf16_and_reproducibility():
    from huggingface_asr_amd import ops
    T, V1, W, K = 48, 40, 8, 8
    lengths = [T, T - 7, 1, 0, T]
    x = torch.from_numpy(np.stack([R.peaky(300 + b, T, V1, V1 - 1) for b in range(5)])).to(torch.bfloat16)          # values both dtypes hold exactly
    g = R.greedy(x[0].float().numpy(), V1 - 1)
    ctx = context([list(g[0:3]), list(g[4:6]), [3, 4, 5], [7]], 1.5, V1, V1 - 1)
    xf, xb = x.float().to(DEV), x.to(DEV)
    lens = torch.tensor(lengths, dtype=torch.int32, device=DEV)
    kw = dict(beams=W, token_topk=K, nbest=4, return_frames=True, bias=ctx)
    out = ops.ctc_beam_decode(xf, V1 - 1, PAD, lens, **kw)
    again = ops.ctc_beam_decode(xf, V1 - 1, PAD, lens, **kw)
    half = ops.ctc_beam_decode(xb, V1 - 1, PAD, lens, **kw)
    i32 = ops.ctc_beam_decode(xf, V1 - 1, PAD, lens, dtype=torch.int32, **kw)
    for k in KEYS + ("credit",):
        assert torch.equal(out[k], again[k]), k                            # two runs: the same bits
        assert torch.equal(out[k], half[k]), k                             # bf16 logits: the bits of fp32 logits holding the same values
    assert i32["tokens"].dtype == torch.int32 and torch.equal(i32["tokens"].long(), out["tokens"]) and torch.equal(i32["credit"], out["credit"])
    for b, n in enumerate(lengths):
        one = ops.ctc_beam_decode(xf[b:b + 1, :max(n, 1)].contiguous(), V1 - 1, PAD, None if n else lens[b:b + 1], **kw)
        m = max(n, 1)
        for k in ("scores", "n_tokens", "credit"):
            assert torch.equal(one[k][0], out[k][b]), (k, b)
        assert torch.equal(one["tokens"][0, :, :m], out["tokens"][b, :, :m]) and (out["tokens"][b, :, m:] == PAD).all(), b
        assert torch.equal(one["frames"][0, :, :m], out["frames"][b, :, :m]) and (out["frames"][b, :, m:] == -1).all(), b
    o = {k: v.cpu().numpy() for k, v in out.items()}
    assert rows_of(o, 3) == [((), 0.0, 0)]                                 # no frames: the empty hypothesis with score 0 and no credit
    for b in (0, 1, 2, 4):
        check_invariants(o, b, ctx, x[b].float().numpy(), lengths[b])
    assert o["credit"][0].max() >= 3


# ------------------------------------------------------------------------------------------------ 5. the edges of the tables
def planted(tokens, V1, blank, seed, gap=True):
    """logits whose best alignment is `tokens`, one frame each (and a blank frame after each, so that equal neighbours stay two tokens), 9 above standard-normal noise"""
    step = 2 if gap else 1
    x = np.random.default_rng(seed).standard_normal((step * len(tokens), V1)).astype(np.float32)
    for i, t in enumerate(tokens):
        x[step * i, t] += 9.0
        if gap:
            x[step * i + 1, blank] += 9.0
    return x


def test_phrase_tokens_at_class_0_and_at_the_last_class():
    V1, blank = 12, 5                                                      # the blank elsewhere: class V1 - 1 is a token, and in a phrase
    ctx = context([[0, 11], [11, 11, 0]], 2.0, V1, blank)
    assert ctx.col[0] > 0 and ctx.col[11] > 0 and ctx.col[blank] == 0
    x = np.stack([planted([3, 0, 11, 4, 11, 11, 0], V1, blank, 1), planted([11, 0, 0, 11, 2, 0, 11], V1, blank, 2)])
    out = decode(x, blank, beams=8, token_topk=6, nbest=4, bias=ctx)
    for b, (best, n) in enumerate((((3, 0, 11, 4, 11, 11, 0), 5), ((11, 0, 0, 11, 2, 0, 11), 4))):
        rows = check_invariants(out, b, ctx, x[b])
        assert rows[0][0] == best and rows[0][2] == n == BR.credit(ctx.phrases, best)


def test_a_64_token_phrase_and_a_context_of_4096_states():
    V1, blank = 100, 99
    phrases = BR.phrases_4096()
    ctx = context(phrases, 1.0, V1, blank)
    assert ctx.S == 4096 and ctx.tab.shape == (4096, ctx.A1)
    long_one = context([phrases[-1]], 1.0, V1, blank)                      # a single 64-token phrase: S = 65
    x = np.stack([planted(phrases[-1], V1, blank, 3), planted(phrases[5][:40] + [1, 2] + phrases[-2][:22], V1, blank, 4)])
    for c in (ctx, long_one):
        out = decode(x, blank, beams=8, token_topk=8, nbest=4, bias=c)
        rows = check_invariants(out, 0, c)
        assert rows[0][0] == tuple(phrases[-1]) and rows[0][2] == 64       # the deepest state of the trie, all of it credited
        rows = check_invariants(out, 1, c)
        assert rows[0][2] == BR.credit(c.phrases, rows[0][0])


def test_a_context_of_1024_columns():
    V1, blank = 1100, 1099
    ctx = context([[i] for i in range(1023)], 0.5, V1, blank)
    assert ctx.tab.shape == (1024, 1024)
    toks = [1022, 5, 700, 0, 1022, 1050, 33]                               # 1050 is in no phrase
    x = planted(toks, V1, blank, 6, gap=False)[None]
    out = decode(x, blank, beams=8, token_topk=8, nbest=4, bias=ctx)
    rows = check_invariants(out, 0, ctx)
    assert rows[0][0] == tuple(toks) and rows[0][2] == 6


def test_long_utterance_with_64_beams_at_weight_0():
    T, V1 = 1030, 40
    g = np.random.default_rng(77)
    x = g.standard_normal((1, T, V1)).astype(np.float32)
    t = 0
    while t < T:
        run = int(g.integers(1, 4))
        x[0, t:t + run, int(g.integers(0, V1))] += 30.0
        t += run
    phrases = [[int(v) for v in g.integers(0, V1 - 1, size=3)] for _ in range(30)]
    kw = dict(beams=64, nbest=2, return_frames=True)
    plain = decode(x, V1 - 1, **kw)
    zero = decode(x, V1 - 1, bias=context(phrases, 0.0, V1, V1 - 1), **kw)
    for k in KEYS:
        assert np.array_equal(plain[k], zero[k]), k
    assert int(plain["n_tokens"][0, 0]) > 200 and int(zero["credit"][0, 0]) == context(phrases, 0.0, V1, V1 - 1).credit(zero["tokens"][0, 0, :int(zero["n_tokens"][0, 0])])


# ------------------------------------------------------------------------------------------------ 6. a malformed context
def test_a_malformed_table_gives_defined_outputs():
    """a `tab` word whose next state lies beyond S, written into a copy of the tables and handed to the C entry: the kernel clamps every index it takes from the tables
    (ctc_walk_step.hpp bias_step: the token into [0, V1), the column into [0, A1), a state and `next` into [0, S)), so the call returns and every output is defined"""
    from huggingface_asr_amd import _lib, ops
    T, V1, W, K, nbest = 12, 10, 4, 4, 2
    blank = V1 - 1
    ctx = context([[1, 2, 3], [2, 2]], 1.0, V1, blank)
    x = torch.from_numpy(planted([1, 2, 3, 2, 2, 4], V1, blank, 9)[None]).to(DEV)
    col, tab = (t.clone() for t in ctx.to(DEV))
    tab.view(-1)[:] = (tab.view(-1) & ~0xFFFF) | 0xFFFF                    # every next state: 65535 >= S
    col[4] = 10 ** 6                                                       # and a column beyond A1
    cut = ops.ctc_beam_cut(x, blank, K)
    L = _lib.lib()
    nbytes = int(L.mi_ctc_beam_workspace_bytes(1, T, W))
    ws = torch.empty((nbytes,), device=DEV, dtype=torch.uint8)
    tokens = torch.full((1, nbest, T), 77, device=DEV, dtype=torch.int64)
    n, scores = torch.full((1, nbest), -1, device=DEV, dtype=torch.int32), torch.full((1, nbest), float("nan"), device=DEV)
    credit = torch.full((1, nbest), -12345, device=DEV, dtype=torch.int32)
    rc = L.mi_ctc_beam_walk_bias(x.data_ptr(), x.stride(1), x.stride(0), 0, 1, T, V1, None, blank, PAD, W, K, nbest, cut["lse"].data_ptr(), cut["lp_blank"].data_ptr(),
                                 cut["lp"].data_ptr(), cut["ids"].data_ptr(), ws.data_ptr(), nbytes, tokens.data_ptr(), 1, n.data_ptr(), scores.data_ptr(), None,
                                 col.data_ptr(), tab.data_ptr(), ctx.S, ctx.A1, ctypes.c_float(1.0), credit.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    assert torch.isfinite(scores).all() and (n >= 0).all() and (n <= T).all() and (credit != -12345).all()
    for r in range(nbest):
        k = int(n[0, r])
        assert ((tokens[0, r, :k] >= 0) & (tokens[0, r, :k] < blank)).all() and (tokens[0, r, k:] == PAD).all()


# ------------------------------------------------------------------------------------------------ 7. the engine
def test_engine_transcribe_with_bias():
    from helpers import case_inputs, load_golden
    from huggingface_asr_amd import ops, shapes
    from huggingface_asr_amd.engine import EBranchformerEngine
    cfg = dict(shapes.TINY)
    cfg.update(ctc_zero_infinity=True, ctc_loss_reduction="mean")
    sd, x, am, _ = case_inputs(load_golden("tiny_rel"), cfg)
    eng = EBranchformerEngine(cfg, DEV)
    eng.load_state_dict(sd)
    xd, lens = x.to(DEV), am.sum(-1).to(DEV, torch.int32)
    V, pad = cfg["vocab_size"], 3
    fwd = eng.forward(xd, lens)
    plain = eng.transcribe(xd, lens, pad_id=pad, beams=4, nbest=2)
    first = [int(t) for t in plain["tokens"][0, :3]]
    ctx = context([first[1:3], [(first[0] + 1) % V, first[1]]], 3.0, V + 1, V)
    want = ops.ctc_beam_decode(fwd["logits"], V, pad, fwd["outer_len"], beams=4, nbest=2, bias=ctx)
    got = eng.transcribe(xd, lens, pad_id=pad, beams=4, nbest=2, bias=ctx)
    for a, b in (("nbest_tokens", "tokens"), ("nbest_n", "n_tokens"), ("scores", "scores"), ("nbest_credit", "credit")):
        assert torch.equal(got[a], want[b]), a
    assert torch.equal(got["credit"], want["credit"][:, 0]) and torch.equal(got["tokens"], want["tokens"][:, 0])
    assert "credit" not in plain and "nbest_credit" not in plain
    o = {k: v.cpu().numpy() for k, v in want.items()}
    for b in range(xd.shape[0]):
        for r in range(2):
            assert int(o["credit"][b, r]) == ctx.credit(o["tokens"][b, r, :int(o["n_tokens"][b, r])])