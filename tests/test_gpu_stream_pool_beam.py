"""GPU: the CTC prefix beam search on the session pool end to end (engine.stream_pool(...).with_beams; csrc/ctc_beam_pool.hip behind stream_pool.hip).  A session's
"beam" must equal — torch.equal — that of `engine.stream(1, C, Lmax, beams=)` fed the same pieces at every step, and at its end ops.ctc_beam_decode of the session's
own concatenated pool logits; everything the pool returned before stays what the pool without beams returns."""
import pytest
import torch

from helpers import seeded_state_dict, synth_feats
from huggingface_asr_amd import ops, shapes
from test_gpu_audio_stream import same
from test_gpu_stream import TINY_CAUSAL, _engine
from test_gpu_stream_pool import CF, LENGTHS, W, schedule

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LMAX, BEAMS, NBEST = 64, 8, 4
PLAIN = ("logits", "ids", "n_ids", "best", "n_out", "total", "final")
COMMITTED = ("committed", "committed_frames", "n_committed", "n_new")
NBEST_KEYS = ("tokens", "n_tokens", "scores", "frames")


def _copy(d):
    return {k: _copy(v) if isinstance(v, dict) else (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in d.items()}


def drive(pool, sessions, partial=None):
    """test_gpu_stream_pool.run_pool's protocol (whole chunks while more than one chunk is left, then the rest as the tail; start / after / idle), keeping every step's
    dict.  partial: {session: the indices of ITS calls that ask for the n-best}.  -> per session the copied step dicts, per step {session: n_out}"""
    st = [dict(s, pos=0, sid=None, done=False, calls=[]) for s in sessions]
    trace, t = [], 0
    while not all(s["done"] for s in st):
        for s in st:
            if s["sid"] is None and not s["done"] and (s.get("start") == t or (s.get("after") is not None and st[s["after"]]["done"])):
                s["sid"] = pool.open()
        feed, finish, who, ask = {}, {}, {}, set()
        for i, s in enumerate(st):
            if s["sid"] is None or s["done"] or t in s.get("idle", ()):
                continue
            left = s["n"] - s["pos"]
            (feed if left > W else finish)[s["sid"]] = s["x"][s["pos"]: s["pos"] + min(left, W)].to(DEV)
            who[s["sid"]] = i
            if partial and len(s["calls"]) in partial.get(i, ()):
                ask.add(s["sid"])
        out = pool.step(feed, finish, partial=ask) if ask else pool.step(feed, finish)
        assert set(out) == set(who)
        for sid, o in out.items():
            s = st[who[sid]]
            if pool.beam is not None:
                assert set(o["beam"]) == set(COMMITTED + (NBEST_KEYS if (o["final"] or sid in ask) else ())), (who[sid], sorted(o["beam"]))
            s["calls"].append(_copy(o))
            s["pos"] += W if sid in feed else s["n"] - s["pos"]
            s["done"] = o["final"]
        trace.append({who[sid]: o["n_out"] for sid, o in out.items()})
        t += 1
        assert t < 1000
    return [s["calls"] for s in st], trace


def alone(eng, x, n, partial=()):
    """the oracle: engine.stream(1, CF, LMAX, beams=) fed the same pieces -> the "beam" of every call, a stream's row taken out"""
    st = eng.stream(1, CF, LMAX, beams=BEAMS, nbest=NBEST)
    calls, pos = [], 0
    while True:
        left = n - pos
        piece = x[None, pos:pos + min(left, W)].to(DEV)
        o = st.feed(piece, partial=len(calls) in partial) if left > W else st.finish(piece)
        calls.append({k: v[0].clone() for k, v in o["beam"].items()})
        pos += min(left, W)
        if left <= W:
            return calls


def same_beam(got_calls, want, what):
    assert len(got_calls) == len(want), what
    for j, (o, w) in enumerate(zip(got_calls, want)):
        g = o["beam"]
        assert set(g) == set(w), (what, j, sorted(g), sorted(w))
        for k in g:
            a, b = (g[k].view(torch.int32), w[k].view(torch.int32)) if k == "scores" else (g[k], w[k])
            assert a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b), f"{what}, call {j}: {k} differs"


def same_as_one_shot(calls, eng, what):
    """the last call's n-best against ops.ctc_beam_decode of the session's own concatenated logits; the committed prefix's life over the calls"""
    x = torch.cat([o["logits"] for o in calls])
    T, b = x.shape[0], calls[-1]["beam"]
    want = ops.ctc_beam_decode(x[None], eng.cfg["vocab_size"], -1, beams=BEAMS, nbest=NBEST, return_frames=True, dtype=torch.int32)
    assert torch.equal(b["n_tokens"], want["n_tokens"][0]) and torch.equal(b["scores"].view(torch.int32), want["scores"][0].view(torch.int32)), what
    assert b["tokens"].shape == (NBEST, LMAX) and b["tokens"].dtype == torch.int32 and torch.equal(b["tokens"][:, :T], want["tokens"][0]), what
    assert torch.equal(b["frames"][:, :T], want["frames"][0]) and bool((b["tokens"][:, T:] == -1).all()) and bool((b["frames"][:, T:] == -1).all()), what
    counts = [int(o["beam"]["n_committed"]) for o in calls]
    assert counts == sorted(counts) and sum(int(o["beam"]["n_new"]) for o in calls) == counts[-1], (what, counts)          # monotone; the n_new sum to it
    n = counts[-1]
    assert n == int(b["n_tokens"][0]) > 0 and torch.equal(b["committed"][:n], b["tokens"][0, :n]) and bool(torch.isfinite(b["scores"][:1]).all()), what
    assert torch.equal(b["committed_frames"][:n], b["frames"][0, :n]) and bool((b["committed"][n:] == -1).all()), what
    for o in calls:                                                        # whatever was committed stayed: a prefix of the final hypothesis
        k = int(o["beam"]["n_committed"])
        assert torch.equal(o["beam"]["committed"][:k], b["tokens"][0, :k]), what


@pytest.fixture(scope="module")
def four():
    sd = seeded_state_dict(TINY_CAUSAL, 44)
    x, _ = synth_feats(44, 4, 250, LENGTHS)
    eng = _engine(TINY_CAUSAL, sd)
    return dict(eng=eng, x=x, ref=[alone(eng, x[b], n) for b, n in enumerate(LENGTHS)])


# ------------------------------------------------------------------ four utterances over three slots
def test_four_sessions_on_three_slots(four):
    eng, x = four["eng"], four["x"]
    got, trace = drive(eng.stream_pool(3, CF, LMAX).with_beams(BEAMS, nbest=NBEST), schedule(x))
    plain, plain_trace = drive(eng.stream_pool(3, CF, LMAX), schedule(x))
    assert trace == plain_trace and [s for s in trace if s.get(1, 0) > CF] == [{0: 0, 1: 16, 2: 0}]        # with the flush beside two feeds in it
    for b in range(4):
        assert len(got[b]) == len(plain[b])
        for j, (o, p) in enumerate(zip(got[b], plain[b])):                 # every key the pool had: untouched
            assert set(o) == set(PLAIN) | {"beam"} and set(p) == set(PLAIN)
            same({k: o[k] for k in PLAIN}, p, f"session {b} step {j}")
        same_beam(got[b], four["ref"][b], f"session {b}")
        same_as_one_shot(got[b], eng, f"session {b}")
    print("n_committed per call:", [[int(o["beam"]["n_committed"]) for o in got[b]] for b in range(4)])


def test_one_slot_flushes_while_two_feed(four):
    """session 1 takes its 13-frame tail — 16 frames of logits for its beam, and its end — in the step where sessions 0 and 2 emit nothing: records of n = 16 with
    final beside two of n = 0"""
    eng, x = four["eng"], four["x"]
    sess = [dict(x=x[0], n=143, start=0), dict(x=x[1], n=61, start=0), dict(x=x[2], n=250, start=0)]
    got, trace = drive(eng.stream_pool(3, CF, LMAX).with_beams(BEAMS, nbest=NBEST), sess)
    assert trace[3] == {0: 0, 1: 16, 2: 0}
    assert [int(got[b][3]["beam"]["n_new"]) for b in (0, 2)] == [0, 0] and int(got[1][3]["beam"]["n_new"]) == int(got[1][3]["beam"]["n_committed"]) > 0
    for b in range(3):
        same_beam(got[b], four["ref"][b], f"session {b}")
        same_as_one_shot(got[b], eng, f"session {b}")


def test_partial_for_one_slot_only(four):
    eng, x = four["eng"], four["x"]
    sess = [dict(x=x[0], n=143, start=0), dict(x=x[2], n=250, start=0)]
    asks = {1: {3, 9}}                                                     # session 1's calls 3 and 9 (drive checks that nobody else's dict gains the n-best)
    got, _ = drive(eng.stream_pool(3, CF, LMAX).with_beams(BEAMS, nbest=NBEST), sess, partial=asks)
    same_beam(got[0], four["ref"][0], "session 0")
    same_beam(got[1], alone(eng, x[2], 250, partial=asks[1]), "session 1")
    assert "tokens" in got[1][3]["beam"] and "tokens" not in got[0][3]["beam"] and "tokens" not in got[1][4]["beam"]
    pool = eng.stream_pool(2, CF, LMAX).with_beams(BEAMS)
    sid = pool.open()
    out = pool.step(feed={sid: x[0, :W].to(DEV)}, partial=True)[sid]       # True: every named slot; nothing emitted yet: the empty hypothesis so far
    assert out["n_out"] == 0 and out["beam"]["scores"].tolist() == [0.0] and int(out["beam"]["n_tokens"][0]) == 0
    with pytest.raises(RuntimeError, match="with_beams"):
        pool.with_beams(4)
    torch.cuda.synchronize()


# ------------------------------------------------------------------ audio in; the model surface
def test_model_audio_pool_with_beams_equals_model_stream_pool_on_extracted_features():
    import numpy as np

    from helpers import load_golden
    from huggingface_asr_amd import fbank as FB
    from huggingface_asr_amd import synth
    from huggingface_asr_amd.configuration_ebranchformer import Wav2Vec2EBranchformerConfig
    from huggingface_asr_amd.feature_extraction import CustomFeatureExtractor
    from huggingface_asr_amd.modeling_ebranchformer import Wav2Vec2EBranchformerForCTC
    from huggingface_asr_amd.streaming import audio_pieces
    g = load_golden("fbank")
    torch.manual_seed(0)
    model = Wav2Vec2EBranchformerForCTC(Wav2Vec2EBranchformerConfig(**dict(shapes.TINY, is_causal=True))).to(DEV).eval()
    fe = CustomFeatureExtractor(feature_size=80, norm_type="global", global_means=np.asarray(g["global_means"], np.float32).tolist(),
                                global_stds=np.asarray(g["global_stds"], np.float32).tolist())
    wave, sizes = torch.from_numpy(synth.waveforms(31, 2, 20000)).to(DEV)[1], [2999, 6000, 1, 7000, 4000]
    ap = model.audio_pool(fe, 2, CF, 48).with_beams(BEAMS)
    ap.open()                                                              # slot 0 stays idle
    sid = ap.open()
    x, _ = fe.extract_on_device(wave[None], default_transform=False)
    fp = model.stream_pool(2, CF, 48).with_beams(BEAMS)
    fp.open()
    fid = fp.open()
    pos = n = steps_run = 0
    news = []
    for i, m in enumerate(sizes):
        last = i == len(sizes) - 1
        ask = i == 1                                                       # the push that runs two steps: partial goes to both
        got = ap.push(**{"finish" if last else "audio": {sid: wave[pos:pos + m]}}, partial={sid} if ask else False)[sid]
        steps = audio_pieces(n, m, fp.n_feat[fid], CF, finish=last)
        assert len(got) == len(steps)
        for o, (lo, hi, fin) in zip(got, steps):
            want = fp.step(**{"finish" if fin else "feed": {fid: x[0, lo:hi]}}, partial=ask)[fid]
            assert "beam" in o and ("tokens" in o["beam"]) == (ask or fin)
            same({k: v for k, v in o.items() if k != "beam"}, {k: v for k, v in want.items() if k != "beam"}, f"push {i}")
            g, w = o["beam"], want["beam"]                                 # the push has run all its steps by now: the committed rows are views and have grown since
            k = int(w["n_committed"])
            assert set(g) == set(w) and int(g["n_committed"]) == k and int(g["n_new"]) == int(w["n_new"]), f"push {i}"
            assert torch.equal(g["committed"][:k], w["committed"][:k]) and torch.equal(g["committed_frames"][:k], w["committed_frames"][:k]), f"push {i}"
            same({k: g[k] for k in g if k in NBEST_KEYS}, {k: w[k] for k in w if k in NBEST_KEYS}, f"push {i} n-best")
            steps_run += 1
        news += [int(o["beam"]["n_new"]) for o in got]                  # read after the push returned: every step's own count survives the later steps
        pos += m
        n += m
    assert got[-1]["final"] and got[-1]["total"] == (FB.num_frames(20000) + 3) // 4 and steps_run > len(sizes)
    assert int(got[-1]["beam"]["n_committed"]) == int(got[-1]["beam"]["n_tokens"][0]) == sum(news) > 0


def test_model_pool_with_beams_equals_engine_pool():
    from huggingface_asr_amd.configuration_ebranchformer import Wav2Vec2EBranchformerConfig
    from huggingface_asr_amd.engine import cfg_from_hf
    from huggingface_asr_amd.modeling_ebranchformer import Wav2Vec2EBranchformerForCTC
    torch.manual_seed(0)
    model = Wav2Vec2EBranchformerForCTC(Wav2Vec2EBranchformerConfig(**dict(shapes.TINY, is_causal=True))).to(DEV).eval()
    x, _ = synth_feats(45, 2, 100, [100, 57])
    sess = [dict(x=x[0], n=100, start=0), dict(x=x[1], n=57, start=2)]
    a, _ = drive(model.stream_pool(2, CF, 32).with_beams(BEAMS, nbest=NBEST, token_topk=6), sess)
    eng = _engine(cfg_from_hf(model.config), {k: v for k, v in model.state_dict().items()})
    b, _ = drive(eng.stream_pool(2, CF, 32).with_beams(BEAMS, nbest=NBEST, token_topk=6), sess)
    for s in range(2):
        assert len(a[s]) == len(b[s])
        for j, (o, p) in enumerate(zip(a[s], b[s])):
            same(o, p, f"session {s} step {j}")
        assert "tokens" in a[s][-1]["beam"]
