"""GPU: the CTC prefix beam search on a stream (csrc/ctc_beam_stream.hip, ops.CtcBeamStream) against the one-shot search on the logits concatenated so far
(ops.ctc_beam_decode, the kernel its own tests pin): after EVERY call, for every partition of the frames, the n-best are equal — tokens, counts and entry frames as
integers, scores as bit patterns.  The committed prefix against the host LCP of the one-shot result's rows; one test against the float64 restatement
(tests/ctc_beam_ref.py) so that the feature does not rest on its sibling kernel alone: scores within 1e-3 absolute, DESIGN §4's bar for fp32 accumulation over
T <= 64 frames."""
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
import ctc_beam_stream_ref as S  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAD = -5
NEG_INF = float("-inf")


def partitions(T, seed):
    """all ones; one call; 1, 2, 3, 5, 7, ... (odd and even counts, the rest in the last call); chunks of 16; a seeded random one holding calls without frames"""
    grow, left = [], T
    for n in (1, 2, 3, 5, 7, 11, 13, 17, 19, 23):
        if left <= 0:
            break
        grow.append(min(n, left)); left -= grow[-1]
    if left > 0:
        grow.append(left)
    g = np.random.default_rng(seed)
    rand, left = [0], T
    while left > 0:
        n = int(g.choice([0, 0, 1, 1, 2, 3, 4, 6, 9]))
        rand.append(min(n, left)); left -= rand[-1]
    rand.append(0)
    assert 0 in rand[1:-1] or rand.count(0) >= 2
    out = dict(ones=[1] * T, one=[T], grow=grow, sixteen=S.chunks(T, 16), random=rand)
    assert all(sum(p) == T for p in out.values())
    return out


def one_shot(x, blank, W, K, t, lengths=None, nbest=None):
    """the oracle on x[:, :t]: numpy dict(tokens (B, nbest, t), n_tokens, scores, frames); t = 0: the empty hypothesis with score 0 and nothing else"""
    from huggingface_asr_amd import ops
    B, nb = x.shape[0], nbest or W
    if t == 0:
        sc = np.full((B, nb), NEG_INF, dtype=np.float32)
        sc[:, 0] = 0.0
        return dict(tokens=np.zeros((B, nb, 0), dtype=np.int64), n_tokens=np.zeros((B, nb), dtype=np.int32), scores=sc, frames=np.zeros((B, nb, 0), dtype=np.int32))
    out = ops.ctc_beam_decode(x[:, :t], blank, PAD, lengths, beams=W, token_topk=K, nbest=nb, return_frames=True)
    return {k: v.cpu().numpy() for k, v in out.items()}


def same_nbest(got, want, where):
    """got: a stream call's dict (rows max_frames wide); want: the one-shot dict (rows t wide, t <= max_frames)"""
    g = {k: got[k].cpu().numpy() for k in ("tokens", "n_tokens", "scores", "frames")}
    t = want["tokens"].shape[2]
    assert np.array_equal(g["n_tokens"], want["n_tokens"]), where
    assert np.array_equal(g["scores"].view(np.int32), want["scores"].view(np.int32)), (where, g["scores"], want["scores"])
    assert np.array_equal(g["tokens"][..., :t], want["tokens"]) and (g["tokens"][..., t:] == PAD).all(), where
    assert np.array_equal(g["frames"][..., :t], want["frames"]) and (g["frames"][..., t:] == -1).all(), where
    cols = np.arange(g["tokens"].shape[2])[None, None, :] >= g["n_tokens"][..., None]                   # the padding rule, and rows that do not exist
    assert (g["tokens"][cols] == PAD).all() and (g["frames"][cols] == -1).all(), where
    assert (g["n_tokens"][np.isneginf(g["scores"])] == 0).all(), where


def stream_and_compare(view, oracle, blank, W, K, parts, max_frames, where):
    from huggingface_asr_amd import ops
    st = ops.CtcBeamStream(view.shape[0], max_frames, beams=W, token_topk=K, nbest=W, blank=blank, pad_id=PAD, return_frames=True)
    t = 0
    for j, n in enumerate(parts):
        out = st.feed(view[:, t:t + n], final=j == len(parts) - 1, partial=True)
        t += n
        same_nbest(out, oracle(t), f"{where} call {j} ({n} frames, {t} so far)")
    return st, out


# ------------------------------------------------------------------------------------------------ 1. exactness, every partition
SHAPES = [(3, 48, 5, 4, 4), (2, 64, 40, 8, 8), (2, 96, 301, 64, 24), (1, 40, 70, 64, 64)]        # B, T, V1, W, K: K > V1 - 1; 256 threads; 1024 threads; 4160 candidates


@functools.lru_cache(maxsize=None)
def exact_case(shape):
    B, T, V1, W, K = shape
    g = torch.Generator().manual_seed(1000 + V1)
    x = (torch.randn((B, T, V1), generator=g) * 3.0).to(torch.bfloat16)                                 # values both dtypes hold exactly: one oracle serves the three layouts
    xf = x.float().to(DEV)
    ld = (V1 + 7) // 8 * 8 + 8
    padded = torch.full((B, T, ld), 1e30, dtype=torch.float32, device=DEV)                             # would win every row if the padding were read as classes
    padded[..., :V1] = xf
    oracle = functools.lru_cache(maxsize=None)(lambda t: one_shot(xf, V1 - 1, W, K, t))
    return dict(fp32=xf, bf16=x.to(DEV), strided=padded[..., :V1]), oracle


@pytest.mark.parametrize("layout", ["fp32", "bf16", "strided"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_every_call_of_every_partition_equals_the_one_shot_search(shape, layout):
    B, T, V1, W, K = shape
    views, oracle = exact_case(shape)
    view = views[layout]
    assert (view.stride(2) == 1) and (view.is_contiguous() != (layout == "strided"))
    for name, parts in partitions(T, 7 + V1).items():
        stream_and_compare(view, oracle, V1 - 1, W, K, parts, T + 3, f"{shape} {layout} {name}")


def test_ties_across_call_boundaries():
    """integer logits in {0, 1, 2}: equal scores occur, so the tie rules decide, also in the frames on either side of a call boundary.  Classes 0 and 1 carry the
    same column, so every hypothesis ties bit for bit with the one that has them swapped: the final beam itself holds equal scores."""
    B, T, V1, W, K = 2, 40, 6, 8, 5
    x = torch.randint(0, 3, (B, T, V1), generator=torch.Generator().manual_seed(3)).float()
    x[..., 1] = x[..., 0]
    x = x.to(DEV)
    oracle = functools.lru_cache(maxsize=None)(lambda t: one_shot(x, V1 - 1, W, K, t))
    assert all(len(set(oracle(T)["scores"][b].tolist())) < W for b in range(B))
    for name, parts in partitions(T, 11).items():
        stream_and_compare(x, oracle, V1 - 1, W, K, parts, T, f"ties {name}")


# ------------------------------------------------------------------------------------------------ 2. ragged ends, independence, reproducibility
def test_ragged_final_call_batch_independence_and_reproducibility():
    from huggingface_asr_amd import ops
    B, T, V1, W, K = 4, 33, 12, 5, 5
    x = (torch.randn((B, T, V1), generator=torch.Generator().manual_seed(5)) * 3.0).to(DEV)
    parts = [8, 8, 8, 9]
    n = parts[-1]
    n_valid = [n, n - 3, 0, 1]
    lengths = torch.tensor([24 + v for v in n_valid], dtype=torch.int32, device=DEV)
    want = one_shot(x, V1 - 1, W, K, T, lengths)

    def run(st, rows, valid):
        t = 0
        for j, m in enumerate(parts):
            last = j == len(parts) - 1
            out = st.feed(x[rows, t:t + m], valid if last else None, final=last)
            t += m
        return {k: v.clone() for k, v in out.items()}

    st = ops.CtcBeamStream(B, T, beams=W, token_topk=K, nbest=W, blank=V1 - 1, pad_id=PAD, return_frames=True)
    a = run(st, slice(0, B), torch.tensor(n_valid, dtype=torch.int32, device=DEV))
    same_nbest(a, want, "ragged")
    st.reset()
    b = run(st, slice(0, B), n_valid)                                                                   # reset(), the same feed (the counts as a list): the same bits
    c = run(ops.CtcBeamStream(B, T, beams=W, token_topk=K, nbest=W, blank=V1 - 1, pad_id=PAD, return_frames=True), slice(0, B), n_valid)
    for k in a:
        assert torch.equal(a[k], b[k]) and torch.equal(a[k], c[k]), k
    for s in range(B):                                                                                  # each stream alone
        one = run(ops.CtcBeamStream(1, T, beams=W, token_topk=K, nbest=W, blank=V1 - 1, pad_id=PAD, return_frames=True), slice(s, s + 1), n_valid[s:s + 1])
        for k in a:
            assert torch.equal(one[k][0], a[k][s]), (s, k)
    nc = a["n_committed"].cpu().tolist()
    assert nc == a["n_tokens"][:, 0].cpu().tolist()                                                     # after final: hypothesis 0
    for s in range(B):
        assert torch.equal(a["committed"][s, :nc[s]].long(), a["tokens"][s, 0, :nc[s]]) and torch.equal(a["committed_frames"][s, :nc[s]], a["frames"][s, 0, :nc[s]])


def test_a_stream_without_frames_is_the_empty_hypothesis():
    from huggingface_asr_amd import ops
    st = ops.CtcBeamStream(2, 8, beams=4, blank=4, pad_id=PAD, nbest=2, return_frames=True)
    out = st.feed(torch.zeros((2, 0, 5), device=DEV), final=True)
    assert out["scores"].cpu().tolist() == [[0.0, NEG_INF]] * 2 and out["n_tokens"].sum().item() == 0 and (out["tokens"] == PAD).all() and (out["frames"] == -1).all()
    assert out["n_committed"].cpu().tolist() == [0, 0] and out["n_new"].cpu().tolist() == [0, 0]


# ------------------------------------------------------------------------------------------------ 3. the committed prefix
def test_committed_prefix_is_the_lcp_of_the_whole_beam_and_only_grows():
    from huggingface_asr_amd import ops
    c = S.PLANTED
    T, V1, W, K = c["T"], c["V1"], c["W"], c["K"]
    x = torch.from_numpy(np.stack([S.planted_logits(), R.peaky(3, T, V1, V1 - 1)])).to(DEV)           # the CPU test's planted case, and a second stream beside it
    parts = S.chunks(T, c["chunk"])
    st = ops.CtcBeamStream(2, T, beams=W, token_topk=K, nbest=2, blank=V1 - 1, pad_id=PAD, return_frames=True)
    t, before, lens = 0, [[], []], []
    for j, n in enumerate(parts):
        final = j == len(parts) - 1
        out = st.feed(x[:, t:t + n], final=final)
        t += n
        want = one_shot(x, V1 - 1, W, K, t)
        nc, new = out["n_committed"].cpu().tolist(), out["n_new"].cpu().tolist()
        for s in range(2):
            rows = [want["tokens"][s, r, :want["n_tokens"][s, r]].tolist() for r in range(W) if want["scores"][s, r] > NEG_INF]
            lcp = list(rows[0] if final else S.lcp(rows))
            got = out["committed"][s, :nc[s]].cpu().tolist()
            assert got == lcp, (j, s, got, lcp)
            assert out["committed_frames"][s, :nc[s]].cpu().tolist() == want["frames"][s, 0, :nc[s]].tolist(), (j, s)
            assert got[:len(before[s])] == before[s] and new[s] == len(got) - len(before[s])           # earlier entries never change
            assert (out["committed"][s, nc[s]:] == PAD).all()
            before[s] = got
        lens.append(nc[0])
    assert "tokens" in out and out["tokens"].shape == (2, 2, T)                                          # the final call returns the n best unasked
    assert any(0 < v < lens[-1] for v in lens[:-1]) and len(set(lens)) >= 4                             # not vacuous: the prefix grew in steps (the CPU test plants this)


# ------------------------------------------------------------------------------------------------ 4. the float64 restatement
def test_streamed_hypotheses_match_the_float64_restatement():
    from huggingface_asr_amd import ops
    T, V1, W, K, draws = 48, 40, 8, 8, 24                                                               # the certified regime of tests/test_gpu_ctc_beam.py
    x = np.stack([R.peaky(s, T, V1, V1 - 1) for s in range(draws)])
    ref = [R.beam_search(x[s], V1 - 1, W, K, nbest=W) for s in range(draws)]
    kept = [s for s in range(draws) if R.min_margin(ref[s]) >= 1e-3]                                    # every cut of the float64 search certified by 1e-3
    assert len(kept) >= 8, kept
    st = ops.CtcBeamStream(draws, T, beams=W, token_topk=K, nbest=W, blank=V1 - 1, pad_id=PAD, return_frames=True)
    xd = torch.from_numpy(x).to(DEV)
    t = 0
    for n in S.chunks(T, 5):
        out = st.feed(xd[:, t:t + n], final=t + n == T)
        t += n
    o = {k: v.cpu().numpy() for k, v in out.items()}
    for s in kept:
        for r, (labels, score, frames) in enumerate(ref[s]["hyps"]):
            n = int(o["n_tokens"][s, r])
            print(f"draw {s} rank {r}: {n} tokens, device {float(o['scores'][s, r]):.6f} float64 {score:.6f}")
            assert tuple(o["tokens"][s, r, :n].tolist()) == labels and o["frames"][s, r, :n].tolist() == frames, (s, r)
            assert abs(float(o["scores"][s, r]) - score) <= 1e-3, (s, r)


# ------------------------------------------------------------------------------------------------ 5. a long utterance
def test_long_utterance_in_chunks_of_16_equals_the_one_shot_bits():
    from huggingface_asr_amd import ops
    T, V1, W, K, M = 1030, 40, 64, 20, 1040
    g = np.random.default_rng(77)
    x = g.standard_normal((2, T, V1)).astype(np.float32)
    for b in range(2):
        t = 0
        while t < T:
            run = int(g.integers(1, 4))
            x[b, t:t + run, int(g.integers(0, V1))] += 30.0                                            # runs of one class (the blank among them) 30 above the noise
            t += run
    xd = torch.from_numpy(x).to(DEV)
    st = ops.CtcBeamStream(2, M, beams=W, token_topk=K, nbest=2, blank=V1 - 1, pad_id=PAD, return_frames=True)
    t = 0
    for n in S.chunks(T, 16):
        out = st.feed(xd[:, t:t + n])
        t += n
    assert t == T and st.walked == T and "tokens" not in out
    held = out["n_committed"].clone()
    with pytest.raises(RuntimeError, match="max_frames"):                                               # 1030 + 16 > 1040: refused on the host
        st.feed(xd[:, :16])
    out = st.feed(xd[:, :0], final=True)                                                                # a call without frames closes the streams
    want = one_shot(xd, V1 - 1, W, K, T, nbest=2)
    same_nbest(out, want, "long")
    assert int(want["n_tokens"].min()) > 200 and (out["n_committed"] >= held).all()
    nc = out["n_committed"].cpu().tolist()
    for s in range(2):
        assert out["committed"][s, :nc[s]].cpu().tolist() == want["tokens"][s, 0, :nc[s]].tolist() and nc[s] == want["n_tokens"][s, 0]


# ------------------------------------------------------------------------------------------------ 6. refusals leave the state alone
def test_refused_calls_launch_nothing_and_leave_the_state_alone():
    from huggingface_asr_amd import ops
    B, T, V1, W, K = 2, 24, 9, 4, 4
    x = (torch.randn((B, T, V1), generator=torch.Generator().manual_seed(9)) * 3.0).to(DEV)
    oracle = lambda t: one_shot(x, V1 - 1, W, K, t)
    st = ops.CtcBeamStream(B, T, beams=W, token_topk=K, nbest=W, blank=V1 - 1, pad_id=PAD, return_frames=True)
    same_nbest(st.feed(x[:, :10], partial=True), oracle(10), "before")
    state = st._state.clone()
    with pytest.raises(RuntimeError, match="max_frames"):
        st.feed(x[:, :15])                                                                              # 10 + 15 > 24
    with pytest.raises(ValueError):
        st.feed(x[:1, 10:12])
    with pytest.raises(ValueError):
        st.feed(x[:, 10:12, :8])
    with pytest.raises(TypeError):
        st.feed(x[:, 10:12].double())
    with pytest.raises(TypeError):
        st.feed(x[0, 10:12])
    with pytest.raises(ValueError, match="n_valid"):
        st.feed(x[:, 10:12], torch.ones(3, dtype=torch.int32, device=DEV))
    with pytest.raises(RuntimeError, match="device"):
        st.feed(x[:, 10:12].cpu())
    assert st.walked == 10 and torch.equal(st._state, state)
    same_nbest(st.feed(x[:, 10:17], partial=True), oracle(17), "after the refusals")
    same_nbest(st.feed(x[:, 17:], final=True), oracle(T), "final")
    state = st._state.clone()
    with pytest.raises(RuntimeError, match="finished"):
        st.feed(x[:, :1])
    assert torch.equal(st._state, state)
    st.reset()
    same_nbest(st.feed(x[:, :10], partial=True), oracle(10), "after reset")
