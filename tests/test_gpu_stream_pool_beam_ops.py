"""GPU: the CTC prefix beam search on the slots of a pool (ops.CtcBeamPool; csrc/ctc_beam_pool.hip) on synthetic logits.  Every session must equal — torch.equal,
scores as int32 bits — `ops.CtcBeamStream(1, ...)` fed the same pieces, after every step: committed tokens / frames / counts, and the n-best wherever it is asked for
(`partial`) or due (`final`); at its end it must equal ops.ctc_beam_decode on its concatenated rows.  Whatever the other records do, in whichever order they come,
wherever the session's rows lie in the step's compact logits, whichever slot it holds and whoever held that slot before."""
import functools
import os
import sys

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
SLOTS, M = 3, 48
COMMITTED = ("committed", "committed_frames", "n_committed", "n_new")
NBEST = ("tokens", "n_tokens", "scores", "frames")

# V1, W, K, nbest: many merges and exact ties, 256 threads; 4160 candidates, 1024 threads; a beam of one
CASES = {"small": (7, 4, None, 4), "wide": (66, 64, 64, 64), "one": (7, 1, None, 1)}


def _logits(seed, T, V1):
    """multiples of 0.25, which bf16 holds exactly at this range: sums of equal terms tie bit for bit, and one array serves both dtypes"""
    x = torch.randn((T, V1), generator=torch.Generator().manual_seed(seed)) * 2.0
    return (x * 4).round().clamp(-24, 24) / 4


def _snap(out, row_c, row_n):
    """one stream's / slot's part of a call's dict, copied"""
    s = {k: out[k][row_c].clone() for k in COMMITTED}
    if row_n is not None:
        s.update({k: out[k][row_n].clone() for k in NBEST})
    return s


def run_alone(x, pieces, case, dtype):
    """the oracle: ops.CtcBeamStream of one stream fed the pieces [(n, final, partial)] of x (T, V1) -> a snapshot per call"""
    from huggingface_asr_amd import ops
    V1, W, K, nb = CASES[case]
    st = ops.CtcBeamStream(1, M, beams=W, token_topk=K, nbest=nb, blank=V1 - 1, pad_id=PAD, dtype=torch.int32, return_frames=True)
    xd, t, snaps = x.to(DEV).to(dtype), 0, []
    for n, final, partial in pieces:
        out = st.feed(xd[None, t:t + n], final=final, partial=partial)
        t += n
        snaps.append(_snap(out, 0, 0 if (final or partial) else None))
    return snaps


def new_pool(case):
    from huggingface_asr_amd import ops
    V1, W, K, nb = CASES[case]
    return ops.CtcBeamPool(SLOTS, M, beams=W, token_topk=K, nbest=nb, blank=V1 - 1, pad_id=PAD, dtype=torch.int32, return_frames=True)


def run_pool(bp, sessions, steps, dtype, strided=False):
    """sessions {name: (x (T, V1), slot)}; steps: lists of ("open", name) and (name, n, final, partial) — the records in the order listed.  The step's compact logits
    hold a row that belongs to nobody first, then the records' rows in REVERSE record order, so row0 neither starts at 0 nor grows with the record index.
    -> ({name: [snapshot per step that named it]}, the last step's dict)"""
    pos = {k: 0 for k in sessions}
    snaps = {k: [] for k in sessions}
    V1 = next(iter(sessions.values()))[0].shape[1]
    for step in steps:
        recs = [e for e in step if e[0] != "open"]
        for e in step:
            if e[0] == "open":
                bp.open(sessions[e[1]][1])
        rows, row0 = [torch.full((1, V1), 3.0)], {}
        at = 1
        for name, n, _, _ in reversed(recs):
            row0[name] = at
            rows.append(sessions[name][0][pos[name]:pos[name] + n])
            at += n
        flat = torch.cat(rows).to(DEV).to(dtype)
        if strided:
            wide = torch.full((flat.shape[0], V1 + 9), 1e30, dtype=dtype, device=DEV)       # would win every row if the padding were read as classes
            wide[:, :V1] = flat
            flat = wide[:, :V1]
        out = bp.step(flat, [(sessions[name][1], row0[name], n, final, partial) for name, n, final, partial in recs])
        want_rows = [sessions[name][1] for name, _, final, partial in recs if final or partial]
        assert [s for s, _ in sorted(out["rows"].items(), key=lambda kv: kv[1])] == want_rows         # the n-best rows: compact, in record order
        assert ("tokens" in out) == bool(want_rows) and (not want_rows or out["tokens"].shape == (len(want_rows), bp.nbest, M))
        for name, n, final, partial in recs:
            slot = sessions[name][1]
            snaps[name].append(_snap(out, slot, out["rows"].get(slot)))
            pos[name] += n
    return snaps, out


def pieces_of(steps, name):
    return [(e[1], e[2], e[3]) for step in steps for e in step if e[0] == name]


def same(got, want, where):
    assert len(got) == len(want), where
    for j, (g, w) in enumerate(zip(got, want)):
        assert set(g) == set(w), (where, j, sorted(g), sorted(w))
        for k in g:
            a, b = (g[k].view(torch.int32), w[k].view(torch.int32)) if k == "scores" else (g[k], w[k])
            assert a.dtype == b.dtype and torch.equal(a, b), f"{where}, call {j}, {k}: {g[k].tolist()} vs {w[k].tolist()}"


def same_as_one_shot(last, x, case, dtype, where):
    """a session's final snapshot against ops.ctc_beam_decode on all its rows; committed == hypothesis 0"""
    from huggingface_asr_amd import ops
    V1, W, K, nb = CASES[case]
    T = x.shape[0]
    assert {"tokens", "scores"} <= set(last), where
    if T == 0:                                                             # the empty hypothesis with score 0 and nothing else
        assert last["scores"].tolist() == [0.0] + [NEG_INF] * (nb - 1) and int(last["n_tokens"].sum()) == 0, where
        assert bool((last["tokens"] == PAD).all()) and bool((last["frames"] == -1).all()) and int(last["n_committed"]) == 0 and int(last["n_new"]) == 0, where
        return
    want = ops.ctc_beam_decode(x.to(DEV).to(dtype)[None], V1 - 1, PAD, beams=W, token_topk=K, nbest=nb, return_frames=True, dtype=torch.int32)
    assert torch.equal(last["n_tokens"], want["n_tokens"][0]), where
    assert torch.equal(last["scores"].view(torch.int32), want["scores"][0].view(torch.int32)), where
    assert torch.equal(last["tokens"][:, :T], want["tokens"][0]) and bool((last["tokens"][:, T:] == PAD).all()), where
    assert torch.equal(last["frames"][:, :T], want["frames"][0]) and bool((last["frames"][:, T:] == -1).all()), where
    n = int(last["n_committed"])
    assert n == int(last["n_tokens"][0]) and torch.equal(last["committed"][:n], last["tokens"][0, :n]) and bool((last["committed"][n:] == PAD).all()), where
    assert torch.equal(last["committed_frames"][:n], last["frames"][0, :n]) and bool((last["committed_frames"][n:] == -1).all()), where


# ------------------------------------------------------------------------------------------------ 1. the schedule with everything in it
# a: walks exactly max_frames = 48, slot 2.  b: 17 frames, slot 0.  c: a session of zero frames, slot 1.  d: 25 frames in the slot c has left.
MAIN_LEN = dict(a=48, b=17, c=0, d=25)
MAIN_SLOT = dict(a=2, b=0, c=1, d=1)
MAIN = [[("open", "a"), ("open", "b"), ("open", "c"), ("a", 5, False, False), ("c", 0, False, False), ("b", 3, False, False)],      # three slots, three sizes, n = 0; slots 2, 1, 0
        [("b", 1, False, True), ("a", 7, False, False)],                                                                         # partial for one of two; c idle
        [("c", 0, True, False), ("a", 11, False, True), ("b", 0, False, False)],                                                  # a final with n = 0: zero frames in total
        [("open", "d"), ("d", 9, False, False), ("b", 13, True, False), ("a", 6, False, False)],                                  # a final beside feeds
        [("a", 19, True, False), ("d", 16, False, True)],                                                                         # a reaches max_frames
        [("d", 0, True, False)]]                                                                                                 # a step without any rows


@functools.lru_cache(maxsize=None)
def main_case(case, layout):
    """the sessions of MAIN and their oracles, computed once per (case, layout) and shared"""
    V1 = CASES[case][0]
    dtype = torch.bfloat16 if layout == "bf16" else torch.float32
    xs = {k: _logits(100 + i + V1, n, V1) for i, (k, n) in enumerate(MAIN_LEN.items())}
    assert sum(p[0] for p in pieces_of(MAIN, "a")) == M and all(sum(p[0] for p in pieces_of(MAIN, k)) == n for k, n in MAIN_LEN.items())
    want = {k: run_alone(xs[k], pieces_of(MAIN, k), case, dtype) for k in xs}
    return xs, want, dtype


@pytest.mark.parametrize("case,layout", [("small", "fp32"), ("small", "bf16"), ("small", "strided"), ("wide", "fp32"), ("wide", "bf16"), ("one", "fp32")])
def test_every_session_of_a_mixed_schedule_equals_its_stream_of_one(case, layout):
    xs, want, dtype = main_case(case, layout)
    sessions = {k: (xs[k], MAIN_SLOT[k]) for k in xs}
    bp = new_pool(case)
    got, _ = run_pool(bp, sessions, MAIN, dtype, strided=layout == "strided")
    for k in xs:
        same(got[k], want[k], f"{case} {layout} session {k}")
        same_as_one_shot(got[k][-1], xs[k], case, dtype, f"{case} {layout} session {k}")
    assert bp.walked == [17, 25, 48] and bp.is_open == [False] * 3
    if case == "small":                                                    # not vacuous: the beam is full, hypotheses differ, something is committed before the end
        last = got["a"][-1]
        assert int((last["scores"] > NEG_INF).sum()) == 4 and int(last["n_tokens"][0]) > 2
        assert any(0 < int(s["n_committed"]) for s in got["a"][:-1])
    # the same pool again — every slot reused — and a fresh one: the same bits (no float atomics, no dependence on what a slot held before)
    again, _ = run_pool(bp, sessions, MAIN, dtype, strided=layout == "strided")
    fresh, _ = run_pool(new_pool(case), sessions, MAIN, dtype, strided=layout == "strided")
    for k in xs:
        same(again[k], got[k], f"{case} {layout} session {k}, the pool reused")
        same(fresh[k], got[k], f"{case} {layout} session {k}, a second pool")


def test_result_does_not_depend_on_slot_index_or_record_order():
    xs, want, dtype = main_case("small", "fp32")
    other = dict(a=0, b=1, c=2, d=2)                                       # other slots, and every step's records reversed
    steps = [[e for e in step if e[0] == "open"] + [e for e in reversed(step) if e[0] != "open"] for step in MAIN]
    got, _ = run_pool(new_pool("small"), {k: (xs[k], other[k]) for k in xs}, steps, dtype)
    for k in xs:
        same(got[k], want[k], f"session {k} in slot {other[k]}")


# ------------------------------------------------------------------------------------------------ 2. a slot reused, its neighbour mid-session; an idle slot
def test_reopened_slot_and_its_neighbour_equal_their_runs_alone():
    """e finishes 40 frames in slot 1, f (25 frames, other logits over the same few classes: the same (parent, token) pairs recur) is opened there; g is mid-session in
    slot 2 across that reset.  A reset that left e's node table behind would hand f nodes of e's arena numbering; one that zeroed more than slot 1 would lose g's."""
    steps = [[("open", "e"), ("open", "g"), ("e", 20, False, False), ("g", 10, False, False)],
             [("e", 20, True, False), ("g", 5, False, True)],
             [("open", "f"), ("f", 12, False, True), ("g", 9, False, False)],
             [("g", 6, True, False), ("f", 13, True, False)]]
    V1 = CASES["small"][0]
    xs = dict(e=_logits(31, 40, V1), f=_logits(32, 25, V1), g=_logits(33, 30, V1))
    slots = dict(e=1, f=1, g=2)
    bp = new_pool("small")
    got, _ = run_pool(bp, {k: (xs[k], slots[k]) for k in xs}, steps, torch.float32)
    for k in xs:
        same(got[k], run_alone(xs[k], pieces_of(steps, k), "small", torch.float32), f"session {k}")
        same_as_one_shot(got[k][-1], xs[k], "small", torch.float32, f"session {k}")
    assert int(got["e"][-1]["n_committed"]) > 0 and int(got["f"][0]["n_committed"]) < int(got["e"][-1]["n_committed"])      # f started from a cleared row
    assert bool((got["f"][0]["committed"][int(got["f"][0]["n_committed"]):] == PAD).all())


def test_idle_slot_is_left_alone():
    V1 = CASES["small"][0]
    xs = dict(h=torch.from_numpy(R.peaky(41, 30, V1, V1 - 1)), i=_logits(42, 20, V1), j=_logits(43, 12, V1))      # h: a planted alignment, two tokens committed after 14 frames
    slots = dict(h=0, i=1, j=2)
    sessions = {k: (xs[k], slots[k]) for k in xs}
    bp = new_pool("small")
    first = [[("open", "h"), ("open", "i"), ("open", "j"), ("h", 14, False, False), ("i", 4, False, False)]]
    others = [[("i", 8, False, True), ("j", 5, False, False)], [("j", 7, True, False)], [("i", 8, True, False)]]
    got, out = run_pool(bp, sessions, first, torch.float32)
    torch.cuda.synchronize()
    n_state = bp.state_bytes
    before = {k: out[k][0].clone() for k in COMMITTED}
    assert int(before["n_committed"]) > 0                                  # there is something to lose
    nodes, words = 1 + M * 4, 2
    while words < 2 * nodes:
        words <<= 1
    head, arena = SLOTS * (64 + 7 * 64 * 4), (16 * SLOTS * nodes + 15) // 16 * 16
    mine = lambda: torch.cat([bp._state[:64], bp._state[SLOTS * 64:SLOTS * 64 + 1792], bp._state[head:head + 16 * nodes],
                              bp._state[head + arena:head + arena + 8 * words]]).clone()          # slot 0's header, beam, arena and node table
    assert n_state == head + arena + 8 * SLOTS * words
    state0 = mine()
    pos = {"h": 14, "i": 4, "j": 0}
    rest = {k: [] for k in xs}
    for step in others:                                                    # (run_pool starts every session at row 0: continue by hand)
        recs, rows, at = [], [], 0
        for name, n, final, partial in step:
            recs.append((slots[name], at, n, final, partial))
            rows.append(xs[name][pos[name]:pos[name] + n]); pos[name] += n; at += n
        o = bp.step(torch.cat(rows).to(DEV), recs)
        for name, n, final, partial in step:
            rest[name].append(_snap(o, slots[name], o["rows"].get(slots[name])))
        for k in COMMITTED:
            assert torch.equal(o[k][0], before[k]), k                     # its committed row and counts: bit-equal
        assert torch.equal(mine(), state0)                                 # and its state
    o = bp.step(xs["h"][14:].to(DEV), [(0, 0, 16, True, False)])
    got["h"].append(_snap(o, 0, 0))
    same(got["h"], run_alone(xs["h"], [(14, False, False), (16, True, False)], "small", torch.float32), "the idle session")
    same(got["i"] + rest["i"], run_alone(xs["i"], [(4, False, False), (8, False, True), (8, True, False)], "small", torch.float32), "session i")
    same(rest["j"], run_alone(xs["j"], [(5, False, False), (7, True, False)], "small", torch.float32), "session j")


# ------------------------------------------------------------------------------------------------ 3. the float64 restatement
def test_pool_sessions_match_the_float64_restatement():
    """tests/ctc_beam_stream_ref.py on planted alignments whose every cut the float64 search certifies by 1e-3 (tests/ctc_beam_ref.min_margin): then fp32 takes the same
    decisions, so tokens, entry frames and — after every call — the committed prefix are equal; scores within 1e-3, the bar of test_gpu_stream_beam_ops at this length."""
    V1, W, K, nb = CASES["small"]
    T = 40
    kept = [s for s in range(24) if R.min_margin(R.beam_search(R.peaky(s, T, V1, V1 - 1), V1 - 1, W, min(W, V1 - 1), nbest=W)) >= 1e-3][:3]
    assert len(kept) == 3, kept
    xs = [torch.from_numpy(R.peaky(s, T, V1, V1 - 1)) for s in kept]
    bp = new_pool("small")
    refs = [S.BeamStream(V1 - 1, W, min(W, V1 - 1)) for _ in kept]
    for s in range(3):
        bp.open(s)
    sizes = [5, 8, 3]                                                       # each session in pieces of its own size
    pos = [0, 0, 0]
    while min(pos) < T:
        recs, rows, at = [], [], 0
        for s in (2, 0, 1):
            if pos[s] >= T:
                continue
            n = min(sizes[s], T - pos[s])
            final = pos[s] + n == T
            refs[s].feed(xs[s][pos[s]:pos[s] + n].numpy(), final=final)
            recs.append((s, at, n, final, False)); rows.append(xs[s][pos[s]:pos[s] + n]); pos[s] += n; at += n
        o = bp.step(torch.cat(rows).to(DEV), recs)
        for slot, _, _, final, _ in recs:
            n = int(o["n_committed"][slot])
            assert tuple(o["committed"][slot, :n].tolist()) == tuple(refs[slot].committed) and o["committed_frames"][slot, :n].tolist() == list(refs[slot].committed_frames)
            if final:
                row = o["rows"][slot]
                for r, (labels, score, frames) in enumerate(refs[slot].hyps(nb)):
                    k = int(o["n_tokens"][row, r])
                    print(f"seed {kept[slot]} rank {r}: {k} tokens, device {float(o['scores'][row, r]):.6f} float64 {score:.6f}")
                    assert tuple(o["tokens"][row, r, :k].tolist()) == tuple(labels) and o["frames"][row, r, :k].tolist() == list(frames), (slot, r)
                    assert abs(float(o["scores"][row, r]) - score) <= 1e-3, (slot, r)
