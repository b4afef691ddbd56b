"""GPU: contextual biasing of the CTC prefix beam search on a stream and on the session pool (csrc/ctc_beam_bias_stream.hip, csrc/ctc_beam_bias_pool.hip): a biased
stream after every call against the biased one-shot search of the logits so far, a biased pool against biased streams of batch 1, an unbiased pool beside it unchanged,
and the engine and model surfaces against each other — all bit for bit."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import ctc_beam_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T, V1, W, K = 40, 40, 8, 8
BLANK = V1 - 1
NBEST_KEYS = ("tokens", "n_tokens", "scores", "frames", "credit")


def bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def logits_and_context(B, seed, w=1.5):
    from huggingface_asr_amd.ctc_bias import CtcBias
    x = np.stack([R.peaky(seed + b, T, V1, BLANK) for b in range(B)])
    g = R.greedy(x[0], BLANK)
    rng = np.random.default_rng(seed)
    phrases = [list(g[1:4]), list(g[5:7])] + [[int(t) for t in rng.integers(0, BLANK, size=int(rng.integers(1, 4)))] for _ in range(6)]
    return torch.from_numpy(x).to(DEV), CtcBias([p for p in phrases if p], w, V1, BLANK)


# ------------------------------------------------------------------------------------------------ 1. a biased stream against the biased one-shot search
@pytest.mark.parametrize("cuts", [((8, 8), (16, 16), (16, 16), (40, 33)), ((0, 0), (1, 1), (1, 1), (25, 25), (40, 40)), ((13, 13), (13, 13), (39, 30), (40, 30))],
                         ids=["ragged-end", "zero-and-single-frames", "repeat-and-ragged"])
def test_stream_equals_the_one_shot_search_after_every_call(cuts):
    """cuts: per call the frames (stream 0, stream 1) delivered so far; a call carries max(new) rows and n_valid = the new frames of each stream"""
    from huggingface_asr_amd import ops
    x, ctx = logits_and_context(2, 700)
    st = ops.CtcBeamStream(2, T, beams=W, token_topk=K, nbest=W, blank=BLANK, pad_id=-1, dtype=torch.int32, return_frames=True, bias=ctx)
    for rnd in range(2):                                                   # the second round after reset(): the carried (s, n) start again at the root
        done = [0, 0]
        for j, upto in enumerate(cuts):
            new = [u - d for u, d in zip(upto, done)]
            rows = max(new)
            piece = torch.zeros((2, rows, V1), device=DEV)
            for b in range(2):
                piece[b, :new[b]] = x[b, done[b]:upto[b]]
            final = j == len(cuts) - 1
            out = st.feed(piece, new, final=final, partial=True)
            done = list(upto)
            lens = torch.tensor(done, dtype=torch.int32, device=DEV)
            want = ops.ctc_beam_decode(x[:, :max(max(done), 1)].contiguous(), BLANK, -1, lens, beams=W, token_topk=K, nbest=W, return_frames=True, dtype=torch.int32,
                                       bias=ctx)
            m = want["tokens"].shape[2]
            for k in NBEST_KEYS:
                got = out[k][:, :, :m] if k in ("tokens", "frames") else out[k]
                assert torch.equal(bits(got), bits(want[k])), (rnd, j, k)
            assert bool((out["tokens"][:, :, m:] == -1).all())
            for b in range(2):                                             # the committed prefix: the longest common prefix of the whole beam (nbest = beams)
                n = out["n_tokens"][b].tolist()
                hyps = [out["tokens"][b, r, :n[r]].tolist() for r in range(W) if r == 0 or torch.isfinite(out["scores"][b, r])]
                lcp = 0
                while all(len(h) > lcp for h in hyps) and len({h[lcp] for h in hyps}) == 1:
                    lcp += 1
                k = int(out["n_committed"][b])
                assert k == (n[0] if final else lcp), (rnd, j, b)
                assert out["committed"][b, :k].tolist() == hyps[0][:k] and bool((out["committed"][b, k:] == -1).all())
        assert int(out["credit"].max()) >= 2
        st.reset()


# ------------------------------------------------------------------------------------------------ 2. a biased pool against biased streams of batch 1
def test_pool_sessions_equal_streams_of_batch_1_and_an_unbiased_pool_is_unchanged():
    from huggingface_asr_amd import ops
    x, ctx = logits_and_context(3, 800)
    lengths, step = [40, 21, 30], 8
    kw = dict(beams=W, token_topk=K, nbest=4, blank=BLANK, pad_id=-1, dtype=torch.int32, return_frames=True)
    # session 0 on slot 0 from step 0, idle at step 2; session 1 on slot 1 from step 1; session 2 re-uses slot 1 once session 1 has ended
    plan = []                                                              # per step [(session, lo, hi, final)]
    pos, started, t = [0, 0, 0], [0, 1, None], 0
    while any(p < n for p, n in zip(pos, lengths)):
        if started[2] is None and pos[1] >= lengths[1]:
            started[2] = t
        now = []
        for s in range(3):
            if started[s] is None or t < started[s] or pos[s] >= lengths[s] or (s == 0 and t == 2):
                continue
            hi = min(pos[s] + step, lengths[s])
            now.append((s, pos[s], hi, hi == lengths[s]))
            pos[s] = hi
        plan.append(now)
        t += 1
    assert any(len(p) == 1 for p in plan) and any(len(p) == 2 for p in plan)

    def run_pool(bias):
        pool = ops.CtcBeamPool(2, T, bias=bias, **kw)
        slot_of, calls = {}, {0: [], 1: [], 2: []}
        for now in plan:
            recs, rows, r0 = [], [], 0
            for s, lo, hi, fin in now:
                if s not in slot_of:
                    slot_of[s] = 0 if s == 0 else 1
                    pool.open(slot_of[s])
                recs.append((slot_of[s], r0, hi - lo, fin, True))
                rows.append(x[s, lo:hi])
                r0 += hi - lo
            out = pool.step(torch.cat(rows), recs)
            for s, lo, hi, fin in now:
                sl, row = slot_of[s], out["rows"][slot_of[s]]
                call = {k: out[k][sl].clone() for k in ("committed", "committed_frames", "n_committed", "n_new")}
                call.update({k: out[k][row].clone() for k in NBEST_KEYS if k in out})
                calls[s].append(call)
        return calls

    def run_alone(bias, s):
        st = ops.CtcBeamStream(1, T, bias=bias, **kw)
        calls = []
        for now in plan:
            for s2, lo, hi, fin in now:
                if s2 == s:
                    out = st.feed(x[s:s + 1, lo:hi], final=fin, partial=True)
                    calls.append({k: v[0].clone() for k, v in out.items()})
        return calls
    for bias in (ctx, None):
        got = run_pool(bias)
        for s in range(3):
            want = run_alone(bias, s)
            assert len(got[s]) == len(want) > 0
            for j, (g, w) in enumerate(zip(got[s], want)):
                assert set(g) == set(w) and ("credit" in g) == (bias is not None), (s, j, sorted(g), sorted(w))
                for k in g:
                    assert torch.equal(bits(g[k]), bits(w[k])), (bias is not None, s, j, k)
        if bias is not None:
            assert int(got[0][-1]["credit"].max()) >= 2                    # session 0 holds a phrase: the context is at work


# ------------------------------------------------------------------------------------------------ 3. the engine and the model
def test_engine_and_model_surfaces_agree_with_each_other_and_with_the_one_shot_call():
    from helpers import load_golden
    from huggingface_asr_amd import ops, shapes, synth
    from huggingface_asr_amd.configuration_ebranchformer import Wav2Vec2EBranchformerConfig
    from huggingface_asr_amd.feature_extraction import CustomFeatureExtractor
    from huggingface_asr_amd.modeling_ebranchformer import Wav2Vec2EBranchformerForCTC
    CF, LMAX, BEAMS, NB = 4, 48, 4, 2
    g = load_golden("fbank")
    torch.manual_seed(0)
    model = Wav2Vec2EBranchformerForCTC(Wav2Vec2EBranchformerConfig(**dict(shapes.TINY, is_causal=True))).to(DEV).eval()
    fe = CustomFeatureExtractor(feature_size=80, norm_type="global", global_means=np.asarray(g["global_means"], np.float32).tolist(),
                                global_stds=np.asarray(g["global_stds"], np.float32).tolist())
    wave = torch.from_numpy(synth.waveforms(31, 2, 20000)).to(DEV)[1]
    x, _ = fe.extract_on_device(wave[None], default_transform=False)
    V, Wf = model.config.vocab_size, 4 * CF

    def through_stream(st):
        pos, logits = 0, []
        while x.shape[1] - pos > Wf:
            logits.append(st.feed(x[:, pos:pos + Wf])["logits"])
            pos += Wf
        o = st.finish(x[:, pos:])
        return {k: v[0] for k, v in o["beam"].items()}, torch.cat(logits + [o["logits"]], dim=1)[0]

    def through_pool(pool):
        pool.open()                                                        # slot 0 stays idle
        sid, pos = pool.open(), 0
        while x.shape[1] - pos > Wf:
            pool.step(feed={sid: x[0, pos:pos + Wf]})
            pos += Wf
        return pool.step(finish={sid: x[0, pos:]})[sid]["beam"]
    plain, _ = through_stream(model.stream(1, CF, LMAX, beams=BEAMS, nbest=NB))
    best = plain["tokens"][0, :int(plain["n_tokens"][0])].tolist()
    assert len(best) >= 1 and "credit" not in plain
    ctx = model.bias_context([best[:2], [(best[0] + 1) % V, best[0]], [best[-1]]], 2.0)
    kw = dict(beams=BEAMS, nbest=NB, bias=ctx)
    ref, logits = through_stream(model.stream(1, CF, LMAX, **kw))
    n = logits.shape[0]
    others = {"engine.stream": through_stream(model._get_engine(torch.device(DEV)).stream(1, CF, LMAX, **kw))[0],
              "model.stream_pool": through_pool(model.stream_pool(2, CF, LMAX).with_beams(BEAMS, nbest=NB, bias=ctx)),
              "engine.stream_pool": through_pool(model._get_engine(torch.device(DEV)).stream_pool(2, CF, LMAX).with_beams(BEAMS, nbest=NB, bias=ctx))}
    ap = model.audio_pool(fe, 2, CF, LMAX).with_beams(BEAMS, nbest=NB, bias=ctx)
    ap.open()
    sid = ap.open()
    others["model.audio_pool"] = ap.push(finish={sid: wave})[sid][-1]["beam"]
    others["model.audio_stream"] = {k: v[0] for k, v in model.audio_stream(fe, 1, CF, LMAX, **kw).finish(wave[None])[-1]["beam"].items()}
    for name, b in others.items():
        assert set(b) == set(ref) and "credit" in b, (name, sorted(b))
        for k in NBEST_KEYS + ("n_committed",):
            assert torch.equal(bits(b[k]), bits(ref[k])), (name, k)
        kc = int(ref["n_committed"])
        assert torch.equal(b["committed"][:kc], ref["committed"][:kc]), name
    want = ops.ctc_beam_decode(logits[None], V, -1, beams=BEAMS, nbest=NB, return_frames=True, dtype=torch.int32, bias=ctx)
    for k in NBEST_KEYS:
        got = ref[k][:, :n] if k in ("tokens", "frames") else ref[k]
        assert torch.equal(bits(got), bits(want[k][0])), k
    for r in range(NB):
        assert int(ref["credit"][r]) == ctx.credit(ref["tokens"][r, :int(ref["n_tokens"][r])].tolist())
    assert int(ref["credit"].max()) >= 1
    # model.transcribe(beams=, bias=): the engine's dict, with the credits of its own hypotheses
    if model.config.pad_token_id is None:
        model.config.pad_token_id = 0
    tr = model.transcribe(x, None, beams=BEAMS, nbest=NB, bias=ctx)
    assert tr["nbest_credit"].shape == (1, NB) and torch.equal(tr["credit"], tr["nbest_credit"][:, 0])
    for r in range(NB):
        assert int(tr["nbest_credit"][0, r]) == ctx.credit(tr["nbest_tokens"][0, r, :int(tr["nbest_n"][0, r])].tolist())
    assert isinstance(model.transcribe(x, None), tuple)                    # the defaults: today's result
