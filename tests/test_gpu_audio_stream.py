"""GPU: streaming from audio end to end (engine.audio_stream / engine.audio_pool / the model-level calls; csrc/fbank_stream.hip in front of stream.hip / stream_pool.hip).
Audio pushed in irregular pieces must give — torch.equal — the logits, ids and beam results of the feature-fed stream (`engine.stream`, `engine.stream_pool`) given
`fbank_gpu`'s features of the WHOLE clip in the pieces `streaming.audio_pieces` names: the streamed features are the one-shot extractor's bit for bit, and the steps
are the same steps."""
import numpy as np
import pytest
import torch

from helpers import load_golden, seeded_state_dict
from huggingface_asr_amd import fbank as FB
from huggingface_asr_amd import shapes, synth
from huggingface_asr_amd.streaming import audio_pieces
from test_gpu_stream import TINY_CAUSAL, _engine

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CF = 4
LMAX = 48                                               # 24 000 samples = 148 feature frames = 37 encoder frames


@pytest.fixture(scope="module")
def rig():
    g = load_golden("fbank")
    stats = dict(normalize="global", global_means=np.asarray(g["global_means"], np.float32), global_stds=np.asarray(g["global_stds"], np.float32))
    tb = FB.FbankTables(80)
    w = torch.from_numpy(synth.waveforms(31, 3, 24000)).to(DEV)
    eng = _engine(TINY_CAUSAL, seeded_state_dict(TINY_CAUSAL, 46))
    dev_stats = dict(normalize="global", global_means=torch.from_numpy(stats["global_means"]).to(DEV), global_stds=torch.from_numpy(stats["global_stds"]).to(DEV))
    feats = lambda wave: FB.fbank_gpu(wave[None], tb, **dev_stats)[0][0]               # the one-shot extractor on a whole clip
    return dict(eng=eng, w=w, stats=stats, feats=feats)


def same(a, b, what):
    """two step dicts (or nested beam dicts): every tensor torch.equal, every count equal"""
    assert set(a) == set(b), what
    for k in a:
        if isinstance(a[k], dict):
            same(a[k], b[k], f"{what}.{k}")
        elif isinstance(a[k], torch.Tensor):
            assert a[k].shape == b[k].shape and torch.equal(a[k], b[k]), f"{what}: {k} differs"
        else:
            assert a[k] == b[k], f"{what}: {k} {a[k]} != {b[k]}"


# ------------------------------------------------------------------ lock-step
PUSHES = [0, 1, 159, 2700, 160, 161, 6000, 399, 400, 401, 2000, 1, 5000, 2619]           # 20 001 samples; the 6000 runs two steps, most run none
TAIL, TAIL_LENGTHS = 3000, [3000, 1201]                                                  # ends 1799 samples = 11 frames apart: less than a chunk of 16


def lock_step_reference(rig, **kw):
    eng, w = rig["eng"], rig["w"]
    ends = [sum(PUSHES) + n for n in TAIL_LENGTHS]
    f = [rig["feats"](w[b, :ends[b]]) for b in range(2)]
    T = max(x.shape[0] for x in f)
    x = torch.stack([torch.cat([v, torch.zeros((T - v.shape[0], 80), device=DEV)]) for v in f])
    st = eng.stream(2, CF, LMAX, **kw)
    outs, n = [], 0
    for m in PUSHES:
        outs.append([st.feed(x[:, lo:hi]) for lo, hi, _ in audio_pieces(n, m, st.n_feat, CF)])
        n += m
    steps = audio_pieces(n, TAIL_LENGTHS, st.n_feat, CF, finish=True)
    last = [st.feed(x[:, lo:hi]) for lo, hi, _ in steps[:-1]]
    lo, his, _ = steps[-1]
    last.append(st.finish(x[:, lo:max(his)], [h - lo for h in his]))
    return outs + [last]


def lock_step_audio(rig, **kw):
    w = rig["w"][:2]
    st = rig["eng"].audio_stream(2, CF, LMAX, **rig["stats"], **kw)
    outs, pos = [], 0
    for i, m in enumerate(PUSHES):
        piece = w[:, pos:pos + m]
        outs.append(st.push(piece.cpu() if i % 3 == 2 else piece))                       # host tensors now and then
        pos += m
    outs.append(st.finish(w[:, pos:pos + TAIL], TAIL_LENGTHS))
    return outs


def test_lock_step_equals_the_feature_fed_stream(rig):
    got, want = lock_step_audio(rig), lock_step_reference(rig)
    assert [len(o) for o in got] == [len(o) for o in want]
    assert 0 in [len(o) for o in got[:-1]] and 2 in [len(o) for o in got[:-1]]          # pushes without a step, a push with two
    for i, (a, b) in enumerate(zip(got, want)):
        for j, (x, y) in enumerate(zip(a, b)):
            same(x, y, f"call {i} step {j}")
    assert got[-1][-1]["totals"].tolist() == [(FB.num_frames(sum(PUSHES) + n) + 3) // 4 for n in TAIL_LENGTHS]
    again = lock_step_audio(rig)                                                         # a second run is bit-identical
    for a, b in zip(got, again):
        for x, y in zip(a, b):
            same(x, y, "second run")


def test_lock_step_with_beams(rig):
    got, want = lock_step_audio(rig, beams=4, nbest=2), lock_step_reference(rig, beams=4, nbest=2)
    assert "beam" in got[-1][-1] and [len(o) for o in got] == [len(o) for o in want]
    for i, (a, b) in enumerate(zip(got, want)):
        for j, (x, y) in enumerate(zip(a, b)):
            same(x, y, f"call {i} step {j}")


def test_lock_step_refuses_ends_more_than_a_chunk_apart(rig):
    st = rig["eng"].audio_stream(2, CF, LMAX, **rig["stats"])
    w = rig["w"][:2]
    first = st.push(w[:, :3000])
    state = st.fb._state.clone()
    with pytest.raises(ValueError, match="pool"):
        st.finish(w[:, 3000:9000], [6000, 500])                                           # 54 and 20 frames, 16 fed: the longest feeds two more chunks, the shortest holds 4 frames
    torch.cuda.synchronize()
    assert st.n == 3000 and st.fb.n == [3000, 3000] and torch.equal(st.fb._state, state) and not st.stream.finished      # nothing was pushed, nothing ran
    ref = rig["eng"].audio_stream(2, CF, LMAX, **rig["stats"])
    same(ref.push(w[:, :3000])[0], first[0], "first chunk")
    for a, b in zip(st.finish(w[:, 3000:9000], [6000, 5000]), ref.finish(w[:, 3000:9000], [6000, 5000])):      # and the stream goes on as if never asked
        same(a, b, "after the refusal")


def test_finish_without_a_tail_runs_the_same_steps(rig):
    """6000 samples = 36 frames: pushed whole then finished empty, or 5000 pushed and 1000 with the finish — chunk, chunk, a tail of 4 either way; the pool likewise"""
    w = rig["w"][:2]
    a = rig["eng"].audio_stream(2, CF, LMAX, **rig["stats"])
    b = rig["eng"].audio_stream(2, CF, LMAX, **rig["stats"])
    got = a.push(w[:, :6000]) + a.finish()
    want = b.push(w[:, :5000]) + b.finish(w[:, 5000:6000])
    assert [o["n_out"] for o in got] == [o["n_out"] for o in want] and len(got) == 3
    for x, y in zip(got, want):
        same(x, y, "finish without a tail")
    pool = rig["eng"].audio_pool(2, CF, LMAX, **rig["stats"])
    s0, s1 = pool.open(), pool.open()
    first = pool.push(audio={s0: w[0, :6000], s1: w[1, :5000].cpu()})
    last = pool.push(finish={s0: None, s1: w[1, 5000:6000]})
    assert [len(first[s0]), len(first[s1]), len(last[s0]), len(last[s1])] == [2, 1, 1, 2]
    for sid, sess in ((s0, dict(clip=0, n=6000, sizes=[6000, 0])), (s1, dict(clip=1, n=6000, sizes=[5000, 1000]))):
        assert torch.equal(torch.cat([o["logits"] for o in first[sid] + last[sid]]), feature_fed(rig, sess)[0])


# ------------------------------------------------------------------ pool
SESSIONS = [dict(clip=0, n=24000, sizes=[700, 5200, 1, 0, 2600, 6001, 399, 3000, 2559, 3540]),
            dict(clip=1, n=9003, sizes=[3000, 161, 400, 5442]),
            dict(clip=2, n=17003, sizes=[6000, 159, 160, 2684, 8000])]


def run_audio_pool(pool, rig, dummies=0):
    """sessions 0 and 1 open at once, session 2 when session 1 has finished (its slot); per call every open session pushes its next piece, the last one as finish
    -> per session (logits, ids, slot), the step counts of every push"""
    for _ in range(dummies):
        pool.open()
    st = [dict(s, i=0, pos=0, sid=None, logits=[], ids=[], done=False) for s in SESSIONS]
    counts = []
    while not all(s["done"] for s in st):
        for k, s in enumerate(st):
            if s["sid"] is None and not s["done"] and (k < 2 or st[1]["done"]):
                s["sid"] = pool.open()
        audio, finish, who = {}, {}, {}
        for k, s in enumerate(st):
            if s["sid"] is None or s["done"]:
                continue
            m = s["sizes"][s["i"]]
            piece = rig["w"][s["clip"], s["pos"]:s["pos"] + m]
            (finish if s["i"] == len(s["sizes"]) - 1 else audio)[s["sid"]] = piece.cpu() if (k + s["i"]) % 4 == 3 else piece
            who[s["sid"]] = k
            s["pos"] += m
            s["i"] += 1
        out = pool.push(audio=audio, finish=finish)
        assert set(out) == set(who)
        for sid, steps in out.items():
            s = st[who[sid]]
            counts.append(len(steps))
            for o in steps:
                k = int(o["n_ids"])
                s["logits"].append(o["logits"].clone())
                s["ids"] += o["ids"][:k].tolist()
            if sid in finish:
                assert steps and steps[-1]["final"] and steps[-1]["total"] == (FB.num_frames(s["n"]) + 3) // 4
                s["done"], s["slot"] = True, sid
                s["sid"] = None
    return [(torch.cat(s["logits"]), s["ids"], s["slot"]) for s in st], counts


def feature_fed(rig, s):
    """engine.stream(1, ...) given the clip's one-shot features in the pieces audio_pieces names for the session's pushes"""
    x = rig["feats"](rig["w"][s["clip"], :s["n"]])[None]
    st = rig["eng"].stream(1, CF, LMAX)
    logits, ids, n = [], [], 0
    for i, m in enumerate(s["sizes"]):
        for lo, hi, fin in audio_pieces(n, m, st.n_feat, CF, finish=i == len(s["sizes"]) - 1):
            o = st.finish(x[:, lo:hi]) if fin else st.feed(x[:, lo:hi])
            logits.append(o["logits"][0])
            ids += o["ids"][0, :int(o["n_ids"][0])].tolist()
        n += m
    return torch.cat(logits), ids


def test_pool_sessions_equal_the_feature_fed_stream_of_one(rig):
    assert all(sum(s["sizes"]) == s["n"] for s in SESSIONS)
    got, counts = run_audio_pool(rig["eng"].audio_pool(2, CF, LMAX, **rig["stats"]), rig)
    assert [g[2] for g in got] == [0, 1, 1] and 0 in counts and 2 in counts             # a reused slot; pushes without a step and with two
    for k, s in enumerate(SESSIONS):
        want = feature_fed(rig, s)
        assert got[k][0].shape == want[0].shape == ((FB.num_frames(s["n"]) + 3) // 4, rig["eng"].cfg["vocab_size"] + 1)
        assert torch.equal(got[k][0], want[0]), f"session {k}: differs from the feature-fed stream by {float((got[k][0] - want[0]).abs().max())}"
        assert got[k][1] == want[1]
    other, _ = run_audio_pool(rig["eng"].audio_pool(3, CF, LMAX, **rig["stats"]), rig, dummies=1)      # an idle session holds slot 0: every session in another slot
    assert [g[2] for g in other] == [1, 2, 2]
    for k in range(3):
        assert torch.equal(other[k][0], got[k][0]) and other[k][1] == got[k][1], f"session {k} in another slot"


# ------------------------------------------------------------------ model level
def test_model_audio_pool_equals_model_stream_pool_on_extracted_features(rig):
    from huggingface_asr_amd.configuration_ebranchformer import Wav2Vec2EBranchformerConfig
    from huggingface_asr_amd.feature_extraction import CustomFeatureExtractor
    from huggingface_asr_amd.modeling_ebranchformer import Wav2Vec2EBranchformerForCTC
    torch.manual_seed(0)
    model = Wav2Vec2EBranchformerForCTC(Wav2Vec2EBranchformerConfig(**dict(shapes.TINY, is_causal=True))).to(DEV).eval()
    fe = CustomFeatureExtractor(feature_size=80, norm_type="global", global_means=rig["stats"]["global_means"].tolist(), global_stds=rig["stats"]["global_stds"].tolist())
    with pytest.raises(NotImplementedError, match="whole utterance"):
        model.audio_pool(CustomFeatureExtractor(feature_size=80, norm_type="utterance"), 2, CF, LMAX)
    wave, sizes = rig["w"][1, :20000], [2999, 6000, 1, 7000, 4000]
    ap = model.audio_pool(fe, 2, CF, LMAX)
    assert ap.seconds(25) == 1.0
    ap.open()                                                                            # slot 0 stays idle
    sid = ap.open()
    x, _ = fe.extract_on_device(wave[None], default_transform=False)
    fp = model.stream_pool(2, CF, LMAX)
    fp.open()
    fid = fp.open()
    pos = n = 0
    for i, m in enumerate(sizes):
        last = i == len(sizes) - 1
        got = ap.push(**{"finish" if last else "audio": {sid: wave[pos:pos + m]}})[sid]
        steps = audio_pieces(n, m, fp.n_feat[fid], CF, finish=last)
        assert len(got) == len(steps)
        for o, (lo, hi, fin) in zip(got, steps):
            want = fp.step(**{"finish" if fin else "feed": {fid: x[0, lo:hi]}})[fid]
            same(o, want, f"push {i}")
        pos += m
        n += m
    assert got[-1]["final"] and got[-1]["total"] == (FB.num_frames(20000) + 3) // 4
