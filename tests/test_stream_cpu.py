"""CPU: the streaming recurrences (tests/stream_ref.py: per-layer frontiers, histories, flush) reproduce the full-utterance forward of the oracle in float64, the
step plan keeps its invariants, every refusal of the public interface happens before any launch, and the state size is host arithmetic.

1e-9 is a cap far above float64 summation-order noise at these magnitudes (logits of order 1, sums of at most a few thousand terms: ~1e-13), so only a wrong
recurrence exceeds it."""
import ctypes as C

import pytest
import torch

from helpers import case_inputs, load_golden, seeded_state_dict, synth_feats
from huggingface_asr_amd import shapes
from huggingface_asr_amd.engine import EBranchformerEngine
from huggingface_asr_amd.streaming import causal_out_frames, frontiers, plan
from oracle import ebranchformer_ref as R
from stream_ref import RefStream, stream_utterances

TOL = 1e-9
CAUSAL = dict(shapes.TINY, is_causal=True)


@pytest.fixture
def f64():
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    yield
    torch.set_default_dtype(old)


def _full(sd, cfg, x):
    with torch.no_grad():
        return R.ctc_head(sd, R.encoder_forward(sd, cfg, x[None]))[0]


def _check(sd, cfg, x, lengths, C):
    sd = {k: v.double() for k, v in sd.items()}
    x = x.double()
    with torch.no_grad():
        got, rec = stream_utterances(sd, cfg, x, lengths, C)
    worst = 0.0
    for b, n in enumerate(lengths):
        want = _full(sd, cfg, x[b, :n])
        assert got[b].shape == want.shape == (causal_out_frames(n), cfg["vocab_size"] + 1), (got[b].shape, want.shape)
        worst = max(worst, float((got[b] - want).abs().max()))
    assert worst < TOL, worst
    return rec


@pytest.mark.parametrize("C", [1, 4, 16, 40])
def test_golden_weights_both_lengths(f64, C):
    """tiny_causal at the golden's two lengths (160 and 97 frames; 97 = 4 * 24 + 1 ends in a tail of one frame), each utterance as a stream of its own"""
    cfg = dict(CAUSAL, ctc_zero_infinity=True, ctc_loss_reduction="mean")
    g = load_golden("tiny_causal")
    sd, x, am, _ = case_inputs(g, cfg)
    for b, n in enumerate(int(v) for v in g["lengths"]):
        _check(sd, cfg, x[b: b + 1], [n], C)


VARIANTS = [
    ("rotary", dict(position_embeddings_type="rotary")),
    ("merge3", dict(merge_conv_kernel=3)),
    ("merge1", dict(merge_conv_kernel=1)),
    ("nomacaron", dict(use_macaron_ff=False)),
    ("csgu_linear_gelu", dict(csgu_use_linear_after_conv=True, csgu_activation="gelu")),
]


@pytest.mark.parametrize("name,kw", VARIANTS, ids=[v[0] for v in VARIANTS])
@pytest.mark.parametrize("C", [1, 4, 16, 40])
def test_variants(f64, name, kw, C):
    cfg = dict(CAUSAL, **kw)
    sd = seeded_state_dict(cfg, 31)
    x, _ = synth_feats(31, 1, 160, [160])
    _check(sd, cfg, x, [160], C)


@pytest.mark.parametrize("tail", [1, 2, 3])
@pytest.mark.parametrize("C", [1, 4])
def test_short_tails(f64, C, tail):
    """`finish` with 1, 2 and 3 feature frames: out_frames(4k + 1 .. 3) = k + 1"""
    sd = seeded_state_dict(CAUSAL, 32)
    n = 16 * 8 + tail
    x, _ = synth_feats(32, 1, n, [n])
    _check(sd, CAUSAL, x, [n], C)


def test_ragged_finish_batch(f64):
    """two streams in lock-step that end inside the last call at different frames: each equals its utterance alone"""
    sd = seeded_state_dict(CAUSAL, 33)
    x, _ = synth_feats(33, 2, 141, [141, 131])
    _check(sd, CAUSAL, x, [141, 131], 4)


def test_reset_restarts(f64):
    sd = {k: v.double() for k, v in seeded_state_dict(CAUSAL, 34).items()}
    x = synth_feats(34, 1, 64, [64])[0].double()
    st = RefStream(sd, CAUSAL, 1, 16, 40)
    with torch.no_grad():
        a = st.step(x, finish=True)[0]
        st.reset()
        b = st.step(x, finish=True)[0]
    assert torch.equal(a, b)


# ------------------------------------------------------------------ plan
@pytest.mark.parametrize("L,r", [(2, 15), (12, 15), (12, 1), (3, 0)])
@pytest.mark.parametrize("C", [1, 4, 16, 40])
@pytest.mark.parametrize("n", [0, 1, 3, 97, 160, 1000])
def test_plan_invariants(n, C, L, r):
    W = 4 * C
    emitted = [0] * (L + 1)
    prev = [0] * (L + 1)
    pos = 0
    steps = []
    while n - pos > W:
        steps.append((pos + W, False, pos))
        pos += W
    steps.append((n, True, pos))
    for n_now, fin, n_prev in steps:
        rows = plan(n_now, C, L, r, fin, n_prev=n_prev)
        assert len(rows) == L + 1
        a0 = rows[0][1]
        assert a0 == causal_out_frames(n_now)
        for l, (lo, hi) in enumerate(rows):
            assert lo == prev[l] and hi >= lo, "frontiers never decrease and a step starts where the last one ended"
            if l > 0 and hi > lo and not fin:
                assert a0 > l * r, "layer l - 1 emits nothing before a_0 > l r"
            if l > 0 and fin:
                assert hi - lo <= C + l * r, "finish emits at most C + (l + 1) r rows at layer l"
            if l > 0 and not fin:
                assert hi - lo <= C
            emitted[l] += hi - lo
            prev[l] = hi
        if not fin:
            assert plan(n_now, C, L, r, False) == rows        # n_prev defaults to a whole chunk
    assert emitted == [causal_out_frames(n)] * (L + 1), "every layer emits every frame exactly once"
    assert frontiers(n, L, r, True) == [causal_out_frames(n)] * (L + 1)


def test_plan_refuses_partial_chunks():
    with pytest.raises(ValueError):
        plan(30, 4, 2, 15, False, n_prev=16)          # 14 frames are not a chunk
    with pytest.raises(ValueError):
        plan(40, 4, 2, 15, True, n_prev=16)           # a tail longer than a chunk
    with pytest.raises(ValueError):
        plan(20, 4, 2, 15, True, n_prev=10)           # finish after a partial chunk


# ------------------------------------------------------------------ refusals, before any launch (no GPU here)
def _engine(cfg, **kw):
    return EBranchformerEngine(cfg, device="cpu", **kw)


def test_refuses_non_causal():
    with pytest.raises(ValueError, match="causal"):
        _engine(dict(shapes.TINY)).stream(1, 4, 100)


def test_refuses_fp32_and_the_finetuning_head():
    with pytest.raises(NotImplementedError, match="fp32"):
        _engine(CAUSAL, precision="fp32").stream(1, 4, 100)
    with pytest.raises(NotImplementedError, match="mixing"):
        _engine(dict(CAUSAL, finetune_with_layer_mixing=True)).stream(1, 4, 100)
    with pytest.raises(NotImplementedError, match="additional"):
        _engine(dict(CAUSAL, finetune_with_additional_layer=True)).stream(1, 4, 100)


def test_refuses_bad_calls():
    st = _engine(CAUSAL).stream(2, 4, 6)
    with pytest.raises(ValueError, match="chunk"):
        st.feed(torch.zeros(2, 15, 80))               # not 4 * C frames
    with pytest.raises(ValueError, match="chunk"):
        st.feed(torch.zeros(1, 16, 80))               # not the stream batch
    with pytest.raises(ValueError, match="tail"):
        st.finish(torch.zeros(2, 17, 80))             # a tail longer than a chunk
    st.n_feat = 16                                    # as after one chunk: 4 frames; the next chunk would make 8 > max_frames = 6
    with pytest.raises(RuntimeError, match="max_frames"):
        st.feed(torch.zeros(2, 16, 80))
    st.finished = True                                # as after finish()
    with pytest.raises(RuntimeError, match="finished"):
        st.feed(torch.zeros(2, 16, 80))
    with pytest.raises(RuntimeError, match="finished"):
        st.finish()


def test_model_stream_refuses_non_causal_and_training():
    from huggingface_asr_amd.configuration_ebranchformer import Wav2Vec2EBranchformerConfig
    from huggingface_asr_amd.modeling_ebranchformer import Wav2Vec2EBranchformerForCTC
    m = Wav2Vec2EBranchformerForCTC(Wav2Vec2EBranchformerConfig(**dict(shapes.TINY, is_causal=True))).train()
    with pytest.raises(RuntimeError, match="eval"):
        m.stream(1, 4, 100)
    with pytest.raises(RuntimeError, match="GPU"):
        m.eval().stream(1, 4, 100)


# ------------------------------------------------------------------ state size: host arithmetic, linear in max_frames
@pytest.fixture(scope="module")
def built():
    from huggingface_asr_amd.csrc import build as B
    return B.build()


def test_state_bytes_on_cpu(built):
    from huggingface_asr_amd import _lib
    eng = _engine(dict(shapes.SMALL, is_causal=True))
    n = [eng.stream(2, 16, m).state_bytes() for m in (1000, 2000, 3000)]
    assert n[0] > 0 and n[2] - n[1] == n[1] - n[0] > 0, n
    B, L, d = 2, 12, 256
    kv, posp = B * L * 1000 * 2 * d * 2, L * 1000 * d * 2                 # what 1000 more frames cost: K | V rows of every layer and stream, the projected distances
    assert n[1] - n[0] == kv + posp, (n[1] - n[0], kv + posp)
    cs = _engine(dict(shapes.SMALL))._config_struct(2, 64, 80)            # not causal: no state
    assert _lib.lib().mi_ebf_stream_state_bytes(C.byref(cs), 16, 1000) == 0
