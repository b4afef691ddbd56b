"""GPU, end to end: causal E-Branchformer + CTC models fed piece by piece through EncoderStream (mi_ebf_stream_step) against the utterance's full forward.

The streamed path stores bf16 exactly where Fwd::plain_layer does, so it is held to the bars the full forward meets in tests/test_gpu_encoder.py: against the
bf16-modelled oracle of the utterance ALONE max < 0.03 / mean < 0.003, against the reference's fp32 golden max < 0.06 / mean < 0.009.  The gap to engine.forward
(other kernels for attention and the convs, the same rounding points) is reported in every message."""
import numpy as np
import pytest
import torch

from helpers import case_inputs, load_golden, seeded_state_dict, synth_feats
from huggingface_asr_amd import shapes
from huggingface_asr_amd.streaming import causal_out_frames, plan
from oracle import ebranchformer_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TINY_CAUSAL = dict(shapes.TINY, is_causal=True, ctc_zero_infinity=True, ctc_loss_reduction="mean")


def _engine(cfg, sd):
    from huggingface_asr_amd.engine import EBranchformerEngine
    eng = EBranchformerEngine(cfg, DEV)
    eng.load_state_dict(sd)
    return eng


def run_stream(st, x, lengths, check_plan=True):
    """feed utterances x (B, T, F) with `lengths` valid frames through the EncoderStream `st`: whole chunks while every stream has more than one left, then finish.
    -> per stream (logits (n_b, V+1) cpu, ids list), per-call n_out"""
    B, W = x.shape[0], 4 * st.C
    lengths = [int(v) for v in lengths]
    assert max(lengths) - (min(lengths) - 1) // W * W <= W, "every stream must end inside the last call"
    logits, ids, n_outs = [[] for _ in range(B)], [[] for _ in range(B)], []
    pos = 0

    def take(out, valid):
        n_ids = out["n_ids"].cpu()
        for b in range(B):
            logits[b].append(out["logits"][b, : valid[b]].float().cpu())
            ids[b] += out["ids"][b, : int(n_ids[b])].cpu().tolist()
        n_outs.append(out["n_out"])

    while min(lengths) - pos > W:
        out = st.feed(x[:, pos:pos + W].to(DEV))
        if check_plan:
            assert out["n_out"] == (lambda r: r[1] - r[0])(plan(pos + W, st.C, st.L, st.r, False)[-1])
        pos += W
        take(out, [out["n_out"]] * B)
    n = max(lengths) - pos
    out = st.finish(x[:, pos:pos + n].to(DEV), [v - pos for v in lengths])
    if check_plan:
        assert out["n_out"] == (lambda r: r[1] - r[0])(plan(pos + n, st.C, st.L, st.r, True, n_prev=pos)[-1])
    assert out["totals"].tolist() == [causal_out_frames(v) for v in lengths]
    take(out, [int(v) for v in out["n_valid"]])
    torch.cuda.synchronize()
    res = [(torch.cat(l, 0), i) for l, i in zip(logits, ids)]
    for (lg, _), v in zip(res, lengths):
        assert lg.shape[0] == causal_out_frames(v)
    return res, n_outs


def _oracle_alone(sd, cfg, x, n):
    with torch.no_grad():
        return R.ctc_head(sd, R.encoder_forward(sd, cfg, x[None, :n], None, q=R.bf16_round), q=R.bf16_round)[0].numpy()


def _forward_alone(eng, x, n):
    return eng.forward(x[None, :n].to(DEV), None)["logits"][0].float().cpu().numpy()


def _gap(a, b):
    d = np.abs(a - b)
    return float(d.max()), float(d.mean())


# ------------------------------------------------------------------ tiny_causal: the golden's two utterances
@pytest.fixture(scope="module")
def tiny():
    g = load_golden("tiny_causal")
    sd, x, am, _ = case_inputs(g, TINY_CAUSAL)
    lengths = [int(v) for v in g["lengths"]]
    eng = _engine(TINY_CAUSAL, sd)
    return dict(g=g, sd=sd, x=x, lengths=lengths, eng=eng, oracle=[_oracle_alone(sd, TINY_CAUSAL, x[b], n) for b, n in enumerate(lengths)],
                full=[_forward_alone(eng, x[b], n) for b, n in enumerate(lengths)])


def _check_tiny(t, b, got, where):
    o, f = _gap(got, t["oracle"][b]), _gap(got, t["full"][b])
    msg = f"{where} utterance {b}: vs oracle max {o[0]:.4f} mean {o[1]:.5f}; vs engine.forward max {f[0]:.4f} mean {f[1]:.5f}"
    print(msg)
    assert o[0] < 0.03 and o[1] < 0.003, msg
    if b == 0:                                          # the golden's unpadded row
        r = _gap(got, t["g"]["logits"][0])
        assert r[0] < 0.06 and r[1] < 0.009, msg + f"; vs reference max {r[0]:.4f} mean {r[1]:.5f}"


@pytest.mark.parametrize("C", [4, 16, 40])
def test_tiny_causal_each_utterance(tiny, C):
    for b, n in enumerate(tiny["lengths"]):
        res, _ = run_stream(tiny["eng"].stream(1, C, 48), tiny["x"][b:b + 1], [n])
        _check_tiny(tiny, b, res[0][0].numpy(), f"C={C}")


def test_tiny_causal_ragged_finish(tiny):
    """both utterances as one stream batch whose streams end inside the last call at frames 160 and 97"""
    res, _ = run_stream(tiny["eng"].stream(2, 40, 40), tiny["x"], tiny["lengths"])
    for b in range(2):
        _check_tiny(tiny, b, res[b][0].numpy(), "ragged C=40")


# ------------------------------------------------------------------ small_causal: 180 frames of lookahead, 12 layers, head size 64
def test_small_causal_row0():
    cfg = dict(shapes.SMALL, is_causal=True, ctc_zero_infinity=True, ctc_loss_reduction="mean")
    g = load_golden("small_causal")
    sd, x, am, _ = case_inputs(g, cfg)
    eng = _engine(cfg, sd)
    res, n_outs = run_stream(eng.stream(1, 32, 256), x[:1], [1000])
    logits = res[0][0].numpy()
    assert logits.shape == (250, 5001)
    d1, d2 = _gap(logits[::25, :64], g["logits_slice"][0]), _gap(logits[:, -1], g["logits_blank"][0])
    f = _gap(logits, _forward_alone(eng, x[0], 1000))
    msg = f"slice max {d1[0]:.4f} mean {d1[1]:.5f}; blank max {d2[0]:.4f} mean {d2[1]:.5f}; vs engine.forward max {f[0]:.4f} mean {f[1]:.5f}; n_out per call {n_outs}"
    print(msg)
    assert max(d1[0], d2[0]) < 0.06 and max(d1[1], d2[1]) < 0.009, msg


# ------------------------------------------------------------------ base size, rotary, head size 128
def test_base_causal_rotary_vs_forward():
    """Base size (16 layers, d 512), rotary, head size 128, 400 frames, C = 16 against engine.forward of the utterance alone at max < 0.03 / mean < 0.003.
    Without a relative term the step runs the full forward's own attention kernel over the K/V cache (mi_attention_qkv_bf16 with Tk != T), so every sum is the full
    forward's: measured gap exactly 0.  (Two bf16 paths that differ in ONE fp32 summation order end up about 0.0034 apart in the mean at this depth — a rounding
    that flips spreads through the bf16 stores of the next layers —, which is what mi_attention_chunk_bf16 measured here, 0.0227 / 0.00341, before the step used
    the full kernel; with relative positions, where the full kernel takes no cache, small_causal measures 0.0202 / 0.00310 against engine.forward.)"""
    from huggingface_asr_amd import synth
    cfg = dict(shapes.BASE, is_causal=True, position_embeddings_type="rotary")
    sd = {k: torch.from_numpy(v) for k, v in synth.state_dict_numpy(shapes.param_shapes(cfg), 41).items()}
    x, _ = synth_feats(41, 1, 400, [400])
    eng = _engine(cfg, sd)
    res, n_outs = run_stream(eng.stream(1, 16, 128), x, [400])
    f = _gap(res[0][0].numpy(), _forward_alone(eng, x[0], 400))
    msg = f"vs engine.forward max {f[0]:.4f} mean {f[1]:.5f}; n_out per call {n_outs}"
    print(msg)
    assert f[0] < 0.03 and f[1] < 0.003, msg


# ------------------------------------------------------------------ the other layer forms, against the oracle
@pytest.mark.parametrize("name,kw", [("merge3", dict(merge_conv_kernel=3)), ("csgu_linear", dict(csgu_use_linear_after_conv=True, csgu_activation="gelu")),
                                     ("rotary_nomacaron", dict(position_embeddings_type="rotary", use_macaron_ff=False)),
                                     # head size 64 without a relative term: the step runs the full forward's attention kernel over the cache
                                     ("rotary_hd64", dict(position_embeddings_type="rotary", hidden_size=128, num_attention_heads=2, intermediate_size=256)),
                                     ("nopos_hd64", dict(position_embeddings_type=None, hidden_size=128, num_attention_heads=2, intermediate_size=256))],
                         ids=["merge3", "csgu_linear", "rotary_nomacaron", "rotary_hd64", "nopos_hd64"])
def test_tiny_variants_vs_oracle(name, kw):
    cfg = dict(TINY_CAUSAL, **kw)
    sd = seeded_state_dict(cfg, 43)
    x, _ = synth_feats(43, 1, 150, [150])
    eng = _engine(cfg, sd)
    res, _ = run_stream(eng.stream(1, 4, 40), x, [150])
    got = res[0][0].numpy()
    o, f = _gap(got, _oracle_alone(sd, cfg, x[0], 150)), _gap(got, _forward_alone(eng, x[0], 150))
    msg = f"{name}: vs oracle max {o[0]:.4f} mean {o[1]:.5f}; vs engine.forward max {f[0]:.4f} mean {f[1]:.5f}"
    print(msg)
    assert o[0] < 0.03 and o[1] < 0.003, msg


# ------------------------------------------------------------------ exact properties
@pytest.fixture(scope="module")
def batch3():
    sd = seeded_state_dict(TINY_CAUSAL, 44)
    x, _ = synth_feats(44, 3, 143, [143, 141, 131])
    return dict(eng=_engine(TINY_CAUSAL, sd), x=x, lengths=[143, 141, 131])


def test_bit_identical_runs_reset_and_batch_independence(batch3):
    eng, x, lengths = batch3["eng"], batch3["x"], batch3["lengths"]
    st = eng.stream(3, 4, 40)
    a, n_a = run_stream(st, x, lengths)
    with pytest.raises(RuntimeError, match="finished"):
        st.feed(x[:, :16].to(DEV))
    st.reset()
    b, n_b = run_stream(st, x, lengths)                     # reset(), the same audio: the same bits
    c, _ = run_stream(eng.stream(3, 4, 40), x, lengths)     # a second stream batch: the same bits
    assert n_a == n_b
    for s in range(3):
        assert torch.equal(a[s][0], b[s][0]) and torch.equal(a[s][0], c[s][0]) and a[s][1] == b[s][1] == c[s][1]
        alone, _ = run_stream(eng.stream(1, 4, 40), x[s:s + 1], [lengths[s]])
        assert torch.equal(a[s][0], alone[0][0]), f"stream {s} of the batch differs from the same stream alone: {float((a[s][0] - alone[0][0]).abs().max())}"
        assert a[s][1] == alone[0][1]


def test_streamed_ids_equal_greedy_decode_of_the_streamed_logits(batch3):
    from huggingface_asr_amd import ops
    eng, x, lengths = batch3["eng"], batch3["x"], batch3["lengths"]
    res, _ = run_stream(eng.stream(3, 4, 40), x, lengths)
    for lg, ids in res:
        want = ops.ctc_greedy_decode(lg[None].to(DEV), eng.cfg["vocab_size"], -1)
        assert ids == want["tokens"][0, : int(want["n_tokens"][0])].cpu().tolist()


def test_refusals_on_the_device(batch3):
    eng, x = batch3["eng"], batch3["x"]
    st = eng.stream(3, 4, 6)
    st.feed(x[:, :16].to(DEV))
    with pytest.raises(RuntimeError, match="max_frames"):
        st.feed(x[:, 16:32].to(DEV))                        # 8 frames > max_frames = 6
    with pytest.raises(ValueError, match="chunk"):
        st.feed(x[:, :15].to(DEV))


def test_step_refuses_bad_plans(tiny):
    """the plan check the lock-step step shares with the pool's records, from the lock-step side: six malformed `rows` (L = 2, r = 15, C = 2, max_frames = 40; each
    breaks one rule) return MI_ERR_ARG before any launch — the state stays bit for bit — and the same six as one pool record fail mi_ebf_stream_slots_table (host only)"""
    import ctypes as C
    from huggingface_asr_amd import _lib
    eng = tiny["eng"]
    st = eng.stream(1, 2, 40)
    st.feed(tiny["x"][:1, :8].to(DEV))                      # one good step: rows (0, 2), (0, 0), (0, 0)
    cs, lib = st._config(), _lib.lib()
    feats = torch.zeros((1, 8, 80), device=DEV)
    lbuf, ints = torch.zeros((32, cs.logits_ld), device=DEV), torch.zeros((3, 32), dtype=torch.int32, device=DEV)
    ends = torch.tensor([4], dtype=torch.int32, device=DEV)
    bad = [([(4, 2), (0, 0), (0, 0)], False),               # a frontier that decreases
           ([(2, 5), (0, 0), (0, 0)], False),               # hi - lo > C at entry 0
           ([(39, 41), (24, 26), (9, 11)], False),          # hi past max_frames
           ([(2, 4), (0, 1), (0, 0)], False),               # a layer emitting more than a_l - r without ends
           ([(2, 4), (0, 4), (0, 3)], True),                # hi != the previous hi with ends
           ([(-1, 1), (0, 0), (0, 0)], False)]              # a negative lo
    good = plan(16, 2, st.L, st.r, False)
    assert (st.L, st.r) == (2, 15) and good == [(2, 4), (0, 0), (0, 0)]

    def table(rows, fin):
        rec = torch.tensor([0, rows[0][1] if fin else -1] + [v for lo, hi in rows for v in (lo, hi, 0)], dtype=torch.int32)
        return lib.mi_ebf_stream_slots_table(C.byref(cs), 2, 40, rec.data_ptr(), 1, None, 0)

    assert table(good, False) > 0                           # the same call takes a plan that is one
    torch.cuda.synchronize()
    before = st._state.clone()
    for rows, fin in bad:
        flat = (C.c_int * 6)(*[v for lo_hi in rows for v in lo_hi])
        rc = lib.mi_ebf_stream_step(C.byref(cs), eng._table, 2, 40, None if st._pos is None else st._pos.data_ptr(), st._state.data_ptr(), st._state.numel(), feats.data_ptr(),
                                    flat, ends.data_ptr() if fin else None, lbuf.data_ptr(), ints[0].data_ptr(), ints[1].data_ptr(), ints[2].data_ptr(),
                                    torch.cuda.current_stream().cuda_stream)
        assert rc == _lib.ERR_ARG, (rows, fin, rc)
        assert table(rows, fin) == _lib.ERR_ARG, (rows, fin)
    torch.cuda.synchronize()
    assert torch.equal(st._state, before)                   # nothing was launched


def test_model_stream_equals_engine_stream():
    from huggingface_asr_amd.configuration_ebranchformer import Wav2Vec2EBranchformerConfig
    from huggingface_asr_amd.engine import cfg_from_hf
    from huggingface_asr_amd.modeling_ebranchformer import Wav2Vec2EBranchformerForCTC
    torch.manual_seed(0)
    model = Wav2Vec2EBranchformerForCTC(Wav2Vec2EBranchformerConfig(**dict(shapes.TINY, is_causal=True))).to(DEV).eval()
    x, _ = synth_feats(45, 2, 100, [100, 97])
    a, _ = run_stream(model.stream(2, 8, 32), x, [100, 97])
    eng = _engine(cfg_from_hf(model.config), {k: v for k, v in model.state_dict().items()})
    b, _ = run_stream(eng.stream(2, 8, 32), x, [100, 97])
    for s in range(2):
        assert torch.equal(a[s][0], b[s][0]) and a[s][1] == b[s][1]
