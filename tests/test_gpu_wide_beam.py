"""GPU: device beam search at the widths the reference's evaluation recipes use (recipes_v0.0.1/librispeech_aed/decoding/*_beam_decode.sh: --num_beams=60
--max_length=512) —
  1. mi_beam_step_wide (csrc/beam_step_wide.hip) follows the pinned loop oracle/generate_ref.beam_search over whole decodes, candidate for candidate;
  2. ... also once the id buffers are past what mi_beam_step stages in LDS;
  3. ... and at small widths it gives mi_beam_step_lm's bits;
  4. the token step with the hypotheses of an utterance sharing its cross-attention K/V (`GPT2DecoderEngine.step(beams=W)`, mi_decoder_step_beams);
  5. `decoder.generate` reaches the device loop for these requests and returns what `generate_stepwise` returns.
The cases of 1-2 are built (and checked for what they must exercise) on the CPU: tests/wide_beam_cases.py, tests/test_wide_beam_cpu.py."""
import numpy as np
import pytest
import torch

import gen_model as GM
import wide_beam_cases as C
from helpers import AED_JCFG, gen_case_inputs
from huggingface_asr_amd import shapes

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ENC = dict(shapes.TINY, ctc_zero_infinity=True, ctc_loss_reduction="mean")


# ---------------------------------------------------------------------------------------------------------------- 1-3. the kernel
def _state(B, W, pad, Lmax):
    ids = torch.full((B * W, Lmax), pad, dtype=torch.long, device=DEV)
    ids[:, 0] = C.START
    bs = torch.zeros(B, W)
    bs[:, 1:] = -1e9
    return dict(ids=ids, bs=bs.view(-1).contiguous().to(DEV), done=torch.zeros(B, dtype=torch.int32, device=DEV), nfin=torch.zeros(B, dtype=torch.int32, device=DEV),
                fs=torch.zeros(B, W, dtype=torch.float32, device=DEV), fl=torch.zeros(B, W, dtype=torch.int32, device=DEV),
                ft=torch.full((B, W, Lmax), pad, dtype=torch.long, device=DEV))


def _padded(t, V):
    buf = torch.zeros(t.shape[0], (V + 7) // 8 * 8)
    buf[:, :V] = t
    return buf.to(DEV)[:, :V]


def _step(entry, st, inputs, B, W, V, cur, max_length, lp, es):
    """one launch of `entry` (mi_beam_step_wide or mi_beam_step_lm: the same arguments) on the device state `st` -> (new_tok, beam_idx, top_s, top_i)"""
    from huggingface_asr_amd import _lib
    from huggingface_asr_amd.decoder import _ES_MODE, _step_denoms
    lg, lse, ctc, lm, lm_lse = inputs
    logits, lse = _padded(lg, V), lse.to(DEV)
    ctc = ctc.to(DEV) if ctc is not None else None
    lm = _padded(lm, V) if lm is not None else None
    lm_lse = lm_lse.to(DEV) if lm_lse is not None else None
    n, Lmax, pad = B * W, st["ids"].shape[1], V - 1
    new_tok, beam_idx = torch.empty(n, dtype=torch.long, device=DEV), torch.empty(n, dtype=torch.long, device=DEV)
    top_s, top_i = torch.empty(B, 2 * W, device=DEV), torch.empty(B, 2 * W, dtype=torch.int32, device=DEV)
    denom, heur = _step_denoms(cur, max_length, lp, es)
    _lib.check(getattr(_lib.lib(), entry)(
        logits.data_ptr(), logits.stride(0), lse.data_ptr(), ctc.data_ptr() if ctc is not None else None, float(1 - C.W_CTC), float(C.W_CTC), int(ctc is not None), pad,
        C.EOS, B, W, V, cur, max_length, Lmax, denom, heur, _ES_MODE[es], st["ids"].data_ptr(), st["bs"].data_ptr(), new_tok.data_ptr(), beam_idx.data_ptr(),
        st["done"].data_ptr(), st["nfin"].data_ptr(), st["fs"].data_ptr(), st["fl"].data_ptr(), st["ft"].data_ptr(), top_s.data_ptr(), top_i.data_ptr(), None,
        lm.data_ptr() if lm is not None else None, lm.stride(0) if lm is not None else 0, lm_lse.data_ptr() if lm_lse is not None else None, float(C.W_LM),
        torch.cuda.current_stream().cuda_stream), entry)
    return new_tok, beam_idx, top_s, top_i


def _follow(case, B, W, V, lp, es, candidates=True):
    """the whole decode of `case` through mi_beam_step_wide; asserts against the oracle's run of the same case: the step at which every utterance closes, each open
    utterance's 2W candidates (values and indices) at every step, and the kept hypotheses, their scores and their order"""
    pad, max_length = case["pad"], case["max_length"]
    st = _state(B, W, pad, max_length + 1)
    tops = []
    for t, inputs in enumerate(case["steps"]):
        was_done = st["done"].clone()
        _, _, top_s, top_i = _step("mi_beam_step_wide", st, inputs, B, W, V, t + 1, max_length, lp, es)
        tops.append((top_s, top_i, was_done))
    seq, scores = case["oracle"]
    tr = case["trace"]
    fs, fl, ft, nf = st["fs"].cpu().numpy(), st["fl"].cpu().numpy(), st["ft"].cpu().numpy(), st["nfin"].cpu().numpy()
    assert (nf == W).all() and bool(st["done"].cpu().all())         # every utterance ends with W kept hypotheses (max_length closes the rest)
    for t, (ts, ti, was_done) in enumerate(tops):
        was_done = was_done.cpu().bool().numpy()
        if t >= case["calls"]:
            assert was_done.all(), t                                 # the oracle stopped: every utterance was closed
            continue
        assert (tr["open"][t] == ~was_done).all(), (t, tr["open"][t], was_done)      # the kernel closes an utterance exactly when the pinned rules freeze it
        if candidates:
            ov, oi = tr["cands"][t]
            ts, ti = ts.cpu().numpy(), ti.cpu().numpy().astype(np.int64)
            for b in np.nonzero(~was_done)[0]:
                assert ti[b].tolist() == oi[b].tolist() and ts[b].tolist() == ov[b].tolist(), (t, b, ts[b], ti[b], ov[b], oi[b])
    for b in range(B):
        for k in range(W):
            want = seq[b * W + k]
            n_tok = int(fl[b, k])
            assert ft[b, k, :n_tok].tolist() == want[:n_tok].tolist() and (want[n_tok:] == pad).all() and (ft[b, k, n_tok:] == pad).all(), (b, k, ft[b, k], want)
            assert fs[b, k] == scores[b * W + k], (b, k, fs[b, k], scores[b * W + k])


@pytest.mark.parametrize("B,W,V,with_ctc,with_lm,lp,es", C.FOLLOW)
def test_wide_beam_step_follows_the_pinned_loop(B, W, V, with_ctc, with_lm, lp, es):
    """mi_beam_step_wide over a whole decode (max_length 11) against oracle/generate_ref.beam_search on the same processed scores (the kernel's arithmetic restated on
    the host, one rounding per operation): for every utterance still open each step's 2W candidate values and indices, the step at which every utterance closes, the kept
    hypotheses, their scores and their order — for equality.  (2, 17, 51): the first width past mi_beam_step's, 2W < V; (1, 64, 51): 2W > V, a row contributes its V
    candidates; (2, 60, 5001): the recipe's, 300 060 candidates per utterance."""
    torch.set_num_threads(8)
    case = C.build(B, W, V, with_ctc, with_lm, lp, es)
    assert case["eos_closed"] > 0 and case["calls"] >= 3
    _follow(case, B, W, V, lp, es)


@pytest.mark.parametrize("B,W,V,with_ctc,with_lm", C.TIES)
def test_wide_beam_step_ranks_ties_in_index_order(B, W, V, with_ctc, with_lm):
    """every stream on a coarse grid: groups of equal values inside the top 2W, the index decides (the index digits of the kernel's keys)"""
    torch.set_num_threads(8)
    case = C.build(B, W, V, with_ctc, with_lm, 1.0, False, "ties")
    tied = case["tied"]
    assert tied > 0 and case["eos_closed"] > 0, tied
    _follow(case, B, W, V, 1.0, False)


@pytest.mark.parametrize("B,W,V,with_ctc,with_lm", C.MINUS_INF)
def test_wide_beam_step_ranks_minus_inf_in_index_order(B, W, V, with_ctc, with_lm):
    """utterances with fewer than 2W finite candidates: the rest of their top 2W are -inf candidates, ranked by index — whole rows of equal keys in stage one, more than
    2W of them in the merge"""
    torch.set_num_threads(8)
    case = C.build(B, W, V, with_ctc, with_lm, 1.0, False, "minus_inf")
    few = case["few"]
    assert few > 0 and case["eos_closed"] > 0, few
    _follow(case, B, W, V, 1.0, False)


def test_wide_beam_step_with_ids_past_the_old_lds_limit():
    """B = 2, W = 60, V = 51, max_length = 140: from cur_len = 64 on W * (cur_len + Lmax) * 8 exceeds the 96 KiB mi_beam_step stages its id buffers in.  The
    end-of-sequence logit is held at -5 until step 125 and lifted by 3 from there on, so beams re-order and hypotheses close while the buffers are past that limit.  Final
    sequences and scores against the pinned loop, for equality (and the step at which every utterance closes)."""
    torch.set_num_threads(8)
    L = C.LONG
    B, W, V, ml = L["B"], L["W"], L["V"], L["max_length"]
    case = C.build(B, W, V, True, False, 1.0, False, "", ml, L["late"])
    first_past = next(c for c in range(1, ml) if W * (c + ml + 1) * 8 > C.OLD_LDS)
    assert first_past < 70 and case["calls"] > L["late"] and sum(case["reorder"][first_past:]) > 20
    seq = case["oracle"][0]
    assert int(((seq == C.EOS).any(1) & (np.argmax(seq == C.EOS, 1) >= L["late"])).sum()) > 0          # hypotheses closed by EOS late in the decode
    _follow(case, B, W, V, 1.0, False, candidates=False)


@pytest.mark.parametrize("with_lm", [True, False])
@pytest.mark.parametrize("B,W,V", [(2, 5, 51), (1, 16, 300), (1, 4, 9001)])
def test_wide_beam_step_at_small_widths_is_mi_beam_step_lm(B, W, V, with_lm):
    """the same decode through both entries: every output of every step and the whole device state after it, bit for bit.  (1, 4, 9001): a row longer than the 8192 keys
    stage one keeps in LDS — its values are recomputed in every pass of the select."""
    case = C.build(B, W, V, True, with_lm, 1.0, False)
    pad, ml = case["pad"], case["max_length"]
    sa, sb = _state(B, W, pad, ml + 1), _state(B, W, pad, ml + 1)

    def bits(t):
        return t.view(torch.int32) if t.dtype == torch.float32 else t
    for t, inputs in enumerate(case["steps"]):
        ra = _step("mi_beam_step_lm", sa, inputs, B, W, V, t + 1, ml, 1.0, False)
        rb = _step("mi_beam_step_wide", sb, inputs, B, W, V, t + 1, ml, 1.0, False)
        for x, y in zip(ra, rb):
            assert torch.equal(bits(x), bits(y)), t
        for k in sa:
            assert torch.equal(bits(sa[k]), bits(sb[k])), (t, k)
    assert bool(sa["done"].cpu().all())


# ---------------------------------------------------------------------------------------------------------------- 4. shared cross K/V in the token step
ENC_LENS = (37, 21)
STEPS, REORDER_AT = 6, 3


def _dec_engine(sd, dec_cfg):
    from huggingface_asr_amd.decoder import GPT2DecoderEngine
    eng = GPT2DecoderEngine(dec_cfg, DEV)
    eng.load_state_dict(sd, "decoder.")
    return eng


def _tok(u, r):
    return C.START if u == 0 else 7 + (u * (5 + 3 * r) + 11 * r) % 40


def _run_steps(eng, enc, lens, W, shared):
    """6 token steps of len(lens) utterances x W hypotheses with one cache re-ordering -> (logits (rows, 6, V) on the CPU, the rows' token histories)"""
    B, T2, d = enc.shape
    n = B * W
    if shared:
        kvs, key_len, beams = eng.cross_kv(enc.reshape(B * T2, d).to(DEV, torch.bfloat16)), lens.to(DEV), W
    else:
        kvs, key_len, beams = eng.cross_kv(enc.repeat_interleave(W, 0).reshape(n * T2, d).to(DEV, torch.bfloat16)), lens.repeat_interleave(W).to(DEV), 1
    cache = eng.init_cache(n, STEPS + 1)
    hist = torch.zeros(n, 0, dtype=torch.long)
    out = []
    for u in range(STEPS):
        if u == REORDER_AT:
            sel = torch.tensor([b * W + (r + 1) % W if r != 2 else b * W for b in range(B) for r in range(W)])       # a rotation within the utterance, one row repeated
            eng.reorder_cache(cache, sel.to(DEV))
            hist = hist.index_select(0, sel)
        tok = torch.tensor([[_tok(u, r % W + 3 * (r // W))] for r in range(n)])
        hist = torch.cat([hist, tok], 1)
        out.append(eng.step(tok.to(DEV), cache, kvs, T2, key_len, beams=beams).float().cpu())
    return torch.stack(out, 1), hist


@pytest.mark.parametrize("W", [5, 9, 60])
def test_token_step_with_beams_sharing_their_cross_kv(W):
    """`step(..., beams=W)` on un-replicated cross tables, two utterances of 37 and 21 encoder frames, 2W rows (10, 18, 120: the launch-per-op path), 6 steps with one cache
    re-ordering: logits against the oracle's teacher-forced decoder (oracle/aed_ref.py, bf16 storage model) and against the replicated call, both within the bound
    tests/test_gpu_decode_long.py holds every form of the step to; utterance 0 run alone gives its rows' logits bit for bit.
    Whether the shared and the replicated call come out bit-equal is printed (run with -s), not required: the two run different shapes of the same attention kernel
    (`beams` queries per batch against one).  Not recorded here yet: the test has not been run on an MI355X."""
    from oracle import aed_ref as A
    from test_gpu_decode_long import _compare
    torch.set_num_threads(8)
    _, sd, _, _, dec_cfg = gen_case_inputs("gen_tiny")
    sd = {k: v for k, v in sd.items() if k.startswith("decoder.")}
    eng = _dec_engine(sd, dec_cfg)
    B, T2, d = len(ENC_LENS), max(ENC_LENS), dec_cfg["n_embd"]
    enc = A.E.bf16_round(torch.randn(B, T2, d, generator=torch.Generator().manual_seed(37)))
    lens = torch.tensor(ENC_LENS, dtype=torch.int32)
    assert B * W > 8
    got, hist = _run_steps(eng, enc, lens, W, shared=True)
    rep, hist_r = _run_steps(eng, enc, lens, W, shared=False)
    assert torch.equal(hist, hist_r)
    mask = (torch.arange(T2)[None] < lens[:, None].long()).repeat_interleave(W, 0)
    pre, post = hist[:, :REORDER_AT], hist                               # a row's history before the re-ordering is its source row's: two teacher-forced passes
    sel = torch.tensor([b * W + (r + 1) % W if r != 2 else b * W for b in range(B) for r in range(W)])
    with torch.no_grad():
        _, lg_post = A.decoder_forward(sd, "decoder.", dec_cfg, post, enc.repeat_interleave(W, 0), mask, None, A.E.bf16_round)
        pre_rows = torch.tensor([[_tok(u, r % W + 3 * (r // W)) for u in range(REORDER_AT)] for r in range(B * W)])
        _, lg_pre = A.decoder_forward(sd, "decoder.", dec_cfg, pre_rows, enc.repeat_interleave(W, 0), mask, None, A.E.bf16_round)
    assert torch.equal(pre_rows.index_select(0, sel), pre)
    want = torch.cat([lg_pre.float(), lg_post[:, REORDER_AT:].float()], 1)
    worst = _compare(got, want, B * W)
    worst_r = _compare(rep, want, B * W)
    print(f"W = {W}: shared vs oracle {worst:.4f}, replicated vs oracle {worst_r:.4f}, shared == replicated bit for bit: {torch.equal(got, rep)}, "
          f"max |shared - replicated| {float((got - rep).abs().max()):.2e}")
    _compare(got, rep, B * W)
    alone, _ = _run_steps(eng, enc[:1], lens[:1], W, shared=True)     # utterance 0 without the other one (W = 5: 5 rows, still the launch-per-op path with beams > 1)
    assert torch.equal(alone, got[:W])


# ---------------------------------------------------------------------------------------------------------------- 5. end to end
def _joint(sd, dec_cfg):
    from huggingface_asr_amd.decoder import JointAEDEngine
    eng = JointAEDEngine(ENC, dec_cfg, AED_JCFG, DEV)
    eng.load_state_dict(sd)
    return eng


def _both_loops(name, W, max_length, ctc_weight, lm=False):
    from huggingface_asr_amd.decoder import beam_loop_route, generate, generate_stepwise, lm_engine_for
    _, sd, x, am, dec_cfg = gen_case_inputs(name)
    eng = _joint(sd, dec_cfg)
    fl = am.sum(-1).to(DEV, torch.int32)
    kw = dict(num_beams=W, max_length=max_length, ctc_weight=ctc_weight, eos_token_id=GM.EOS)
    if lm:
        import lm_model as LM
        kw.update(lm=lm_engine_for(LM.tiny_lm(), DEV), lm_weight=LM.LM_WEIGHT)
    stats = {}
    a = generate(eng, x.to(DEV), fl, stats=stats, **kw)
    b = generate_stepwise(eng, x.to(DEV), fl, **kw)
    assert stats.get("steps", 0) >= 1 and stats["route"] == beam_loop_route(W, GM.V, max_length) == "device_wide", stats      # only the device loop fills it
    assert stats["kv_beams"] == W                                    # 2W rows > 8: the hypotheses share their utterance's cross K/V
    assert len(a) == len(b) == x.shape[0]
    for u in range(len(a)):
        assert len(a[u]["hypotheses"]) == W
        assert a[u]["hypotheses"] == b[u]["hypotheses"], (u, a[u]["hypotheses"][:3], b[u]["hypotheses"][:3])
    return a


@pytest.mark.parametrize("ctc_weight", [0.0, 0.3])
@pytest.mark.parametrize("W", [20, 60])
def test_generate_runs_wide_beams_on_the_device(W, ctc_weight):
    """`decoder.generate` against `decoder.generate_stepwise` on the tiny joint model, two ragged utterances, max_length 12: hypotheses, scores and order equal; the
    request runs the device loop (it fills `stats`) with mi_beam_step_wide"""
    _both_loops("gen_tiny", W, 12, ctc_weight)


def test_generate_runs_wide_beams_with_a_language_model():
    _both_loops("gen_tiny", 20, 12, 0.3, lm=True)


def test_generate_runs_sixty_beams_to_max_length_140():
    """id buffers past mi_beam_step's LDS staging (fixed sinusoidal positions: the table grows to the cache)"""
    out = _both_loops("gen_tiny_fixedpos", 60, 140, 0.3)
    assert max(len(t) for h in out for _, t in h["hypotheses"]) > 12


def test_model_generate_with_twenty_beams_returns_the_engine_sequences():
    from test_surface_cpu import _joint_model
    from huggingface_asr_amd.decoder import generate
    _, sd, x, am, dec_cfg = gen_case_inputs("gen_tiny")
    model = _joint_model(False)
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not missing and not unexpected
    model = model.to(DEV).eval()
    W, ml = 20, 12
    from huggingface_asr_amd.decoding import GenerationConfigCustom
    gen_config = GenerationConfigCustom(bos_token_id=GM.START, pad_token_id=GM.PAD, decoder_start_token_id=GM.START, length_penalty=1.0, early_stopping=False,
                                        eos_token_id=GM.EOS, max_length=ml, num_beams=W, ctc_weight=0.3, ctc_margin=0, lm_weight=0, lm_model=None, space_token_id=-1,
                                        apply_eos_space_trick=False, eos_space_trick_weight=1.0)
    model.generation_config = gen_config
    gen_config.num_return_sequences, gen_config.return_dict_in_generate, gen_config.output_scores = W, True, True
    out = model.generate(generation_config=gen_config, input_values=x.to(DEV), attention_mask=am.to(DEV))
    assert out.sequences.shape[0] == x.shape[0] * W
    stats = {}
    ref = generate(model._get_engine(DEV), x.to(DEV), am.sum(-1).to(DEV, torch.int32), num_beams=W, max_length=ml, ctc_weight=0.3, eos_token_id=GM.EOS, stats=stats)
    assert stats["route"] == "device_wide"
    for b in range(x.shape[0]):
        for k in range(W):
            s, toks = ref[b]["hypotheses"][k]
            row = out.sequences[b * W + k].tolist()
            assert row[: len(toks)] == toks and all(v == GM.PAD for v in row[len(toks):])
            assert float(out.sequences_scores[b * W + k]) == pytest.approx(s, abs=1e-6)
