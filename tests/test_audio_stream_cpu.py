"""The host side of streaming from audio (huggingface_asr_amd/fbank.py FbankStream, streaming.py audio_pieces / AudioStream / AudioPool; csrc/fbank_stream.hip states the
semantics): the carry / FIFO arithmetic against `fbank_numpy` of the whole clip, `audio_pieces` against a brute-force simulation, the refusals before any launch and the
host-only C query.  No GPU here."""
import random

import numpy as np
import pytest
import torch

from audio_stream_ref import RefStream, brute_pieces
from huggingface_asr_amd import fbank as FB
from huggingface_asr_amd import shapes, synth
from huggingface_asr_amd.engine import EBranchformerEngine
from huggingface_asr_amd.streaming import audio_pieces, extractor_settings, seconds

CAUSAL = dict(shapes.TINY, is_causal=True)
EDGES = [0, 1, 159, 160, 161, 399, 400, 401]          # piece sizes around the hop and the frame


def _engine(cfg, **kw):
    return EBranchformerEngine(cfg, device="cpu", **kw)


@pytest.fixture(scope="module")
def built():
    from huggingface_asr_amd.csrc import build as B
    return B.build()


@pytest.fixture(scope="module")
def tables():
    return FB.FbankTables(80)


def random_pieces(rng, total):
    """sizes that sum to `total`: the edge sizes, each at least once, between random ones"""
    sizes = list(EDGES)
    left = total - sum(sizes)
    while left > 0:
        n = min(left, rng.choice([rng.randrange(0, 50), rng.randrange(100, 700), rng.randrange(700, 4000)]))
        sizes.append(n)
        left -= n
    rng.shuffle(sizes)
    return sizes


# ------------------------------------------------------------------ frames and carry
def test_every_total_and_cut_pair_gives_the_whole_clips_frames(tables):
    """every total N in 0 .. 1400 cut at every pair of points of a grid around the frame and hop edges: the frames streamed are those of the whole clip, bit for bit"""
    wave = synth.waveforms(7, 1, 1400)[0]
    whole = FB.fbank_numpy(wave, tables)                                  # (7, 80): a prefix's frames are a prefix of these
    memo = {}

    def frame_fn(fr):                                                     # fbank_numpy of the frame's own 400 samples, once per distinct frame
        key = fr.tobytes()
        if key not in memo:
            memo[key] = FB.fbank_numpy(fr, tables)[0]
        return memo[key]

    grid = [0, 1, 159, 160, 161, 399, 400, 401, 559, 560, 561, 720, 1000, 1399]
    cases = 0
    for N in range(0, 1401):
        cuts = [c for c in grid if c <= N]
        for i, a in enumerate(cuts):
            for b in cuts[i:]:
                s = RefStream(tables, frame_fn=frame_fn)
                got = [s.push(wave[:a]), s.push(wave[a:b]), s.push(wave[b:N])]
                T = FB.num_frames(N)
                assert sum(got) == T == len(s.fifo) and s.max_carry <= 399
                assert s.carry.size == N - (FB.HOP * T if T else 0)
                assert np.array_equal(s.pop(T), whole[:T]), (N, a, b)
                cases += 1
    assert cases > 50000 and len(memo) == 7                               # only the clip's own seven frames were ever formed


def test_random_splits_of_a_clip_give_its_frames(tables):
    wave = synth.waveforms(8, 1, 24000)[0]
    whole = FB.fbank_numpy(wave, tables)
    assert whole.shape == (148, 80)
    means, stds = synth.normal(8, "means", (80,), 1.0), np.abs(synth.normal(8, "stds", (80,), 1.0)) + 0.5
    whole_g = ((whole - means) / stds).astype(np.float32)
    rng = random.Random(5)
    for trial in range(4):
        sizes = random_pieces(rng, 24000)
        assert set(EDGES) <= set(sizes) and sum(sizes) == 24000
        s, g = RefStream(tables), RefStream(tables, "global", means, stds)
        pos, got = 0, []
        for n in sizes:
            s.push(wave[pos: pos + n])
            g.push((wave[pos: pos + n]))
            pos += n
            assert s.max_carry <= 399 and (s.n < 400 or s.carry.size >= 240)
            if trial % 2:                                                 # popped as they come, or all at the end
                got.append(s.pop(len(s.fifo)))
        got.append(s.pop(len(s.fifo)))
        assert np.array_equal(np.concatenate(got), whole)
        assert np.array_equal(g.pop(148), whole_g)


def test_int16_pieces_are_their_float_samples(tables):
    pcm = (synth.waveforms(9, 1, 3000)[0] * 32768.0).clip(-32768, 32767).astype(np.int16)
    a, b = RefStream(tables), RefStream(tables)
    a.push(pcm[:700]); a.push(pcm[700:])
    b.push(pcm.astype(np.float32) / np.float32(32768.0))
    fa = a.pop(17)
    assert np.array_equal(fa, b.pop(17)) and np.array_equal(fa, FB.fbank_numpy(pcm.astype(np.float32) / np.float32(32768.0), tables))


# ------------------------------------------------------------------ audio_pieces
@pytest.mark.parametrize("C", [1, 4, 16])
def test_pieces_equal_the_brute_force_simulation(C):
    W = 4 * C
    rng = random.Random(C)
    exact = zero = 0
    for trial in range(300):
        # totals that make the frame count an exact multiple of 4 C, sessions shorter than a frame (R = 0), and random ones
        kind = trial % 3
        if kind == 0:
            total = 400 + 160 * (W * rng.randrange(1, 5) - 1) + rng.randrange(0, 160)
            assert FB.num_frames(total) % W == 0
        elif kind == 1:
            total = rng.randrange(0, 400)
        else:
            total = rng.randrange(0, 160 * W * 5)
        pushes, left = [], total
        while left > 0:
            n = min(left, rng.choice(EDGES + [rng.randrange(0, 2 * 160 * W + 500)]))
            pushes.append(n)
            left -= n
        if rng.random() < 0.5 or not pushes:
            pushes.append(0)                                              # a finish without a tail
        want = brute_pieces(pushes, C)
        n = fed = 0
        for i, m in enumerate(pushes):
            steps = audio_pieces(n, m, fed, C, finish=i == len(pushes) - 1)
            assert steps == want[i], (pushes, i)
            n += m
            fed = steps[-1][1] if steps else fed
        T = FB.num_frames(total)
        assert fed == T and want[-1][-1][2]
        tail = want[-1][-1][1] - want[-1][-1][0]
        assert 0 <= tail <= W and (tail > 0) == (T > sum(hi - lo for call in want for lo, hi, f in call if not f))
        exact += T > 0 and T % W == 0 and tail == W
        zero += T == 0 and want[-1] == [(0, 0, True)]
    assert exact > 5 and zero > 50, (exact, zero)


def test_pieces_of_a_push_do_not_depend_on_how_it_is_cut():
    """k = max(0, ceil(R / 4C) - 1): a finish holds back 1 .. 4C frames for its last step however many arrive with it"""
    assert audio_pieces(0, 400 + 160 * 31, 0, 4, finish=True) == [(0, 16, False), (16, 32, True)]          # 32 frames: one chunk, then a full tail
    assert audio_pieces(0, 400 + 160 * 31, 0, 4) == [(0, 16, False), (16, 32, False)]
    assert audio_pieces(400 + 160 * 31, 0, 32, 4, finish=True) == [(32, 32, True)]                         # R = 0
    assert audio_pieces(0, 399, 0, 4, finish=True) == [(0, 0, True)]
    assert audio_pieces(5000, 1, 16, 4) == []
    with pytest.raises(ValueError, match="whole chunks"):
        audio_pieces(5000, 0, 15, 4)


def test_lock_step_streams_must_end_inside_one_call():
    n = lambda frames: 400 + 160 * (frames - 1)
    assert audio_pieces(0, [n(20), n(17)], 0, 4, finish=True) == [(0, 16, False), (16, [20, 17], True)]
    assert audio_pieces(0, [n(32), n(16)], 0, 4, finish=True) == [(0, 16, False), (16, [32, 16], True)]    # the shortest has the chunk, its tail is empty
    assert audio_pieces(n(16), [0, 0], 16, 4, finish=True) == [(16, [16, 16], True)]
    with pytest.raises(ValueError, match="pool"):
        audio_pieces(0, [n(33), n(31)], 0, 4, finish=True)            # the longest feeds two chunks, the shortest holds 31 frames
    with pytest.raises(ValueError, match="pool"):
        audio_pieces(0, [n(17), 0], 0, 4, finish=True)
    with pytest.raises(ValueError, match="finishing"):
        audio_pieces(0, [n(17), n(17)], 0, 4)
    assert seconds(25) == 1.0


# ------------------------------------------------------------------ refusals, before any launch
def test_refusals():
    with pytest.raises(NotImplementedError, match="whole utterance"):
        _engine(CAUSAL).audio_pool(2, 4, 100, normalize="utterance")
    with pytest.raises(NotImplementedError, match="whole utterance"):
        _engine(CAUSAL).audio_stream(2, 4, 100, normalize="utterance")
    with pytest.raises(ValueError, match="causal"):
        _engine(dict(shapes.TINY)).audio_pool(2, 4, 100)
    with pytest.raises(ValueError, match="causal"):
        _engine(dict(shapes.TINY)).audio_stream(2, 4, 100)
    with pytest.raises(NotImplementedError, match="fp32"):
        _engine(CAUSAL, precision="fp32").audio_stream(2, 4, 100)
    with pytest.raises(NotImplementedError, match="beams"):
        _engine(CAUSAL).audio_pool(2, 4, 100, beams=4)
    with pytest.raises(ValueError, match="global_means"):
        _engine(CAUSAL).audio_pool(2, 4, 100, normalize="global")
    with pytest.raises(ValueError, match="feature_size"):
        _engine(CAUSAL).audio_pool(2, 4, 100, normalize="global", global_means=np.zeros(40), global_stds=np.ones(40))
    with pytest.raises(ValueError, match="feature_size"):
        _engine(CAUSAL).audio_stream(2, 4, 100, tables=FB.FbankTables(40))
    pool = _engine(CAUSAL).audio_pool(2, 4, 100)
    sid = pool.open()
    with pytest.raises(ValueError, match="float32"):
        pool.push(audio={sid: torch.zeros(100, dtype=torch.float64)})
    with pytest.raises(ValueError, match="one dtype"):
        pool.push(audio={sid: torch.zeros(100), pool.open(): torch.zeros(100, dtype=torch.int16)})
    with pytest.raises(ValueError, match="both"):
        pool.push(audio={sid: torch.zeros(100)}, finish={sid: None})
    with pytest.raises(RuntimeError, match="no open session"):
        _engine(CAUSAL).audio_pool(2, 4, 100).push(audio={0: torch.zeros(100)})
    with pytest.raises(RuntimeError, match="max_frames"):
        pool.push(audio={sid: torch.zeros(160 * 4 * 101 + 400)})
    with pytest.raises(RuntimeError, match="GPU"):
        pool.push(audio={sid: torch.zeros(1000)})                        # valid, but there is no CPU path
    st = _engine(CAUSAL).audio_stream(2, 4, 100)
    with pytest.raises(ValueError, match="float32"):
        st.push(torch.zeros(2, 100, dtype=torch.int32))
    with pytest.raises(ValueError, match="same n"):
        st.push(torch.zeros(3, 100))
    with pytest.raises(ValueError, match="pool"):
        st.finish(torch.zeros(2, 160 * 40), [160 * 40, 400])              # ends more than a chunk apart: refused before anything is pushed
    assert st.n == 0 and st.fb.n == [0, 0]


def test_extractor_settings_and_the_model_surface():
    from huggingface_asr_amd.configuration_ebranchformer import Wav2Vec2EBranchformerConfig
    from huggingface_asr_amd.feature_extraction import CustomFeatureExtractor
    from huggingface_asr_amd.modeling_ebranchformer import Wav2Vec2EBranchformerForCTC
    utt = CustomFeatureExtractor(feature_size=80, norm_type="utterance")
    with pytest.raises(NotImplementedError, match="whole utterance"):
        extractor_settings(utt, 80)
    assert extractor_settings(CustomFeatureExtractor(feature_size=80, norm_type="utterance", do_ceptral_normalize=False), 80)["normalize"] is None
    glob = CustomFeatureExtractor(feature_size=80, norm_type="global", global_means=[0.5] * 80, global_stds=[2.0] * 80)
    s = extractor_settings(glob, 80)
    assert s["normalize"] == "global" and list(s["global_stds"]) == [2.0] * 80 and s["tables"].num_mel == 80
    with pytest.raises(ValueError, match="feature_size"):
        extractor_settings(CustomFeatureExtractor(feature_size=40, norm_type="global", global_means=[0.0] * 40, global_stds=[1.0] * 40), 80)
    m = Wav2Vec2EBranchformerForCTC(Wav2Vec2EBranchformerConfig(**CAUSAL)).train()
    with pytest.raises(RuntimeError, match="eval"):
        m.audio_pool(glob, 2, 4, 100)
    with pytest.raises(NotImplementedError, match="whole utterance"):
        m.eval().audio_pool(utt, 2, 4, 100)
    with pytest.raises(NotImplementedError, match="whole utterance"):
        m.audio_stream(utt, 2, 4, 100)
    with pytest.raises(RuntimeError, match="GPU"):
        m.audio_pool(glob, 2, 4, 100)
    with pytest.raises(RuntimeError, match="GPU"):
        m.audio_stream(glob, 2, 4, 100)


# ------------------------------------------------------------------ the ring and the C side's host-only query
def test_state_bytes_and_ring_size(built, tables):
    from huggingface_asr_amd import _lib
    fb = FB.FbankStream(5, 16, 1000, tables, device="cpu")
    assert fb.R == 16 + 7                                                  # 4 C + ceil(1000 / 160)
    assert fb.state_bytes() == 5 * (2 * 400 + fb.R * 80) * 4               # [carry (S, 2, 400) | fifo (S, R, nmel)] fp32
    L = _lib.lib()
    assert L.mi_fbank_stream_state_bytes(1, 1, 1) == (800 + 1) * 4
    assert L.mi_fbank_stream_state_bytes(16, 64 + 32, 127) == 16 * (800 + 96 * 127) * 4
    for bad in [(0, 8, 80), (2, 0, 80), (2, 8, 0), (2, 8, 128)]:
        assert L.mi_fbank_stream_state_bytes(*bad) == 0
    assert [FB.frames_added(n) for n in (0, 1, 160, 161, 1000)] == [0, 1, 1, 2, 7]
    for n_prev in range(0, 900, 7):                                        # frames_added bounds what a push completes, whatever came before
        for n in (1, 159, 160, 161, 1000):
            assert FB.num_frames(n_prev + n) - FB.num_frames(n_prev) <= FB.frames_added(n)
    with pytest.raises(ValueError, match="slot"):
        fb.open(5)
    with pytest.raises(RuntimeError, match="GPU"):
        fb.push({0: torch.zeros(100)})
    with pytest.raises(RuntimeError, match="ring"):
        fb.push({0: torch.zeros(400 + 160 * 30)})                         # 31 frames into a ring of 23, refused before the state is touched
