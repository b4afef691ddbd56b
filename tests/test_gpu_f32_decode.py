"""GPU: the fp32 inference mode of the joint model (decoder.py / modeling_joint.py `precision="fp32"`, csrc/decoder_f32.hip) against the fp32 CPU oracle and the
reference's own fixtures — SURVEY §7 tier (i), "fp32-mode kernels vs fp32 oracle: max |dlogit| <= 1e-3", for the decoder step, the joint forward and decoding.

  * token-step logits of the tiny decoder (learned and fixed positions): 12 steps at 1, 3 and 2 x 5 rows with a cache re-ordering in the middle, against
    oracle.aed_ref.decoder_forward over the same prefixes (teacher-forced recomputation: no cache to get wrong), max |dlogit| <= 1e-3; `step` against `step_py`
    within 1e-5 of the logit scale; a 4-token prompt step against four single steps, same bar;
  * one step at DeCRED_base size (tests/config5_model.py), 1 and 5 hypotheses, same bar;
  * the teacher-forced JointAEDEngine(precision="fp32").forward on the aed_tiny fixtures, held to the bars tests/test_oracle_golden.py holds the fp32 CPU oracle to
    for the same fixtures (encoder logits / states 2e-4, logits 3e-4, the three losses 1e-4 relative);
  * generate on the gen_tiny fixtures, every setting of gen_model.SETTINGS: all 22 utterance decodes, every kept hypothesis, token for token the reference's, the
    sequence scores within 1e-3 (a twelfth of the fixtures' smallest decision margin, 0.012) — no decode may be left out;
  * generate_stepwise equals generate; the model-level switch.
Every comparison prints its observed figure (pytest -s): `F32DEC <what> ...`."""
import numpy as np
import pytest
import torch

import gen_model as GM
from helpers import AED_JCFG, TINY_DEC, aed_case_inputs, gen_case_inputs, load_golden
from huggingface_asr_amd import shapes
from oracle import aed_ref as A

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ENC = dict(shapes.TINY, ctc_zero_infinity=True, ctc_loss_reduction="mean")
BAR = 1e-3          # SURVEY §7 tier (i)


def _dec_engine(sd, cfg, precision="fp32"):
    from huggingface_asr_amd.decoder import GPT2DecoderEngine
    eng = GPT2DecoderEngine(cfg, DEV, precision=precision)
    eng.load_state_dict(sd)
    return eng


def _joint(sd, dec_cfg, precision="fp32"):
    from huggingface_asr_amd.decoder import JointAEDEngine
    eng = JointAEDEngine(ENC, dec_cfg, AED_JCFG, DEV, precision=precision)
    eng.load_state_dict(sd)
    return eng


def _oracle_last(sd, cfg, ids, enc, lens, W):
    """logits of EVERY position of the prefixes `ids` (rows, n), row r of utterance r // W attending to enc[r // W, :lens[r // W]]"""
    mask = (torch.arange(enc.shape[1])[None] < lens[:, None].long()).repeat_interleave(W, 0)
    with torch.no_grad():
        return A.decoder_forward(sd, "decoder.", cfg, ids, enc.repeat_interleave(W, 0), mask, None)[1]


@pytest.mark.parametrize("nu,W", [(1, 1), (3, 1), (2, 5)], ids=["B1", "B3", "B2xW5"])
@pytest.mark.parametrize("name,fixed", [("aed_tiny", False), ("aed_tiny_fixedpos", True)])
def test_token_step_logits_against_the_fp32_oracle(name, fixed, nu, W):
    sd, _, _, _ = aed_case_inputs(load_golden(name))
    cfg = dict(TINY_DEC, pos_emb_fixed=fixed)
    d, V, steps, T, Lmax = cfg["n_embd"], cfg["vocab_size"], 12, 37, 16
    rows = nu * W
    gen = torch.Generator().manual_seed(7 * rows + int(fixed))
    enc = torch.randn(nu, T, d, generator=gen)
    lens = torch.tensor([T, 20, 33][:nu], dtype=torch.int32)
    ids = torch.randint(0, V, (rows, steps), generator=gen)
    eng = _dec_engine(sd, cfg)
    kvs = eng.cross_kv(enc.to(DEV).view(nu * T, d))
    assert all(t.dtype == torch.float32 and t.shape == (nu * T, 2 * d) for t in kvs)
    ca, cb = eng.init_cache(rows, Lmax), eng.init_cache(rows, Lmax)
    assert ca["k"][0].dtype == torch.float32 and float(ca["k"][0].abs().max()) == 0.0
    ld = lens.to(DEV)
    hist = ids.clone()                                                # the prefix every row holds NOW (re-ordering copies prefixes between rows)
    got, snap = [], {}
    worst_py = scale = 0.0
    for t in range(steps):
        if t == 6 and W > 1:                                          # beam re-ordering inside every utterance, hypotheses duplicated and dropped
            idx = torch.tensor([u * W + k for u in range(nu) for k in (1, 1, 0, 4, 2)])
            snap[6] = hist[:, :6].clone()
            hist[:, :6] = hist[idx, :6]
            eng.reorder_cache(ca, idx)
            eng.reorder_cache(cb, idx)
        tok = hist[:, t:t + 1].to(DEV)
        la = eng.step(tok, ca, kvs, T, ld, beams=W)
        lb = eng.step_py(tok, cb, kvs, T, ld, beams=W)
        scale = max(scale, float(la.abs().max()))
        worst_py = max(worst_py, float((la - lb).abs().max()))
        got.append(la.cpu())
    assert ca["past"] == cb["past"] == steps
    # the oracle over the prefixes as they were when each step ran
    worst = 0.0
    first = 6 if 6 in snap else 0
    if first:
        want = _oracle_last(sd, cfg, snap[6], enc, lens, W)
        worst = max(float((got[t] - want[:, t]).abs().max()) for t in range(first))
    want = _oracle_last(sd, cfg, hist, enc, lens, W)
    worst = max([worst] + [float((got[t] - want[:, t]).abs().max()) for t in range(first, steps)])
    print(f"F32DEC step {name} rows={nu}x{W} max|dlogit|={worst:.3e} (bar {BAR:.0e}) step-vs-step_py={worst_py:.3e} logit scale={scale:.2f}")
    assert worst <= BAR
    assert worst_py <= 1e-5 * scale
    # a 4-token prompt step returns the last position's logits: the four single steps' fourth
    cp = eng.init_cache(rows, Lmax)
    first_ids = (snap[6] if first else hist)[:, :4].contiguous().to(DEV)
    lp = eng.step(first_ids, cp, kvs, T, ld, beams=W)
    dp = float((lp.cpu() - got[3]).abs().max())
    print(f"F32DEC prompt step {name} rows={nu}x{W} U=4 vs four steps max|dlogit|={dp:.3e}")
    assert cp["past"] == 4 and dp <= BAR
    # ... and leaves the cache the single steps left: the fifth step agrees too
    l5 = eng.step((snap[6] if first else hist)[:, 4:5].contiguous().to(DEV), cp, kvs, T, ld, beams=W)
    assert float((l5.cpu() - got[4]).abs().max()) <= BAR


def test_step_above_64_rows_runs_the_tiled_gemm():
    """70 rows: past the rows-streaming linear's 64, the step's linears are mi_gemm_f32 (gelu_new in its epilogue) and the cache append a launch of its own"""
    sd, _, _, _ = aed_case_inputs(load_golden("aed_tiny"))
    cfg = dict(TINY_DEC)
    d, V, T, nu, W = cfg["n_embd"], cfg["vocab_size"], 19, 14, 5
    gen = torch.Generator().manual_seed(70)
    enc = torch.randn(nu, T, d, generator=gen)
    lens = torch.randint(1, T + 1, (nu,), generator=gen).to(torch.int32)
    ids = torch.randint(0, V, (nu * W, 4), generator=gen)
    eng = _dec_engine(sd, cfg)
    kvs = eng.cross_kv(enc.to(DEV).view(nu * T, d))
    cache = eng.init_cache(nu * W, 6)
    want = _oracle_last(sd, cfg, ids, enc, lens, W)
    worst = 0.0
    for t0, t1 in ((0, 2), (2, 3), (3, 4)):                           # a two-token prompt, then single steps
        got = eng.step(ids[:, t0:t1].contiguous().to(DEV), cache, kvs, T, lens.to(DEV), beams=W).cpu()
        worst = max(worst, float((got - want[:, t1 - 1]).abs().max()))
    print(f"F32DEC step aed_tiny rows={nu}x{W} (tiled GEMM route) max|dlogit|={worst:.3e} (bar {BAR:.0e})")
    assert worst <= BAR


@pytest.mark.parametrize("W", [1, 5])
def test_one_step_at_decred_base_size(W, monkeypatch):
    import config5_model as C5
    monkeypatch.setattr(C5.shapes, "param_shapes", lambda cfg: {})   # the decoder's seeded weights alone (the base encoder's take ten seconds to draw and are not read here)
    sd = C5.state_dict(0)
    cfg, d, T = C5.DEC_CFG, C5.D, 61
    gen = torch.Generator().manual_seed(W)
    enc = torch.randn(1, T, d, generator=gen)
    lens = torch.tensor([55], dtype=torch.int32)
    ids = torch.randint(C5.ACTIVE, C5.ACTIVE + C5.NACT, (W, 4), generator=gen)
    eng = _dec_engine(sd, cfg)
    kvs = eng.cross_kv(enc.to(DEV).view(T, d))
    cache = eng.init_cache(W, 8)
    eng.step(ids[:, :3].contiguous().to(DEV), cache, kvs, T, lens.to(DEV), beams=W)
    got = eng.step(ids[:, 3:4].contiguous().to(DEV), cache, kvs, T, lens.to(DEV), beams=W).cpu()
    want = _oracle_last(sd, cfg, ids, enc, lens, W)[:, -1]
    err = float((got - want).abs().max())
    print(f"F32DEC step DeCRED_base rows={W} max|dlogit|={err:.3e} (bar {BAR:.0e}) logit scale={float(want.abs().max()):.2f}")
    assert got.shape == (W, C5.V) and err <= BAR


@pytest.mark.parametrize("name,fixed", [("aed_tiny", False), ("aed_tiny_fixedpos", True)])
def test_teacher_forced_joint_forward_against_the_reference_fixture(name, fixed):
    g = load_golden(name)
    sd, x, am, lab = aed_case_inputs(g)
    eng = _joint(sd, dict(TINY_DEC, pos_emb_fixed=fixed))
    with torch.no_grad():
        out = eng.forward(x.to(DEV), am.sum(-1).to(DEV, torch.int32), lab.to(DEV))
    assert out["logits"].dtype == out["encoder_hidden"].dtype == out["encoder_logits"].dtype == torch.float32
    B, T2 = g["encoder_hidden"].shape[:2]
    fig = {"encoder_logits": (out["encoder_logits"], 2e-4), "encoder_hidden": (out["encoder_hidden"].view(B, T2, -1), 2e-4), "logits": (out["logits"], 3e-4)}
    line = []
    for k, (t, bar) in fig.items():
        err = float(np.abs(t.cpu().numpy() - g[k]).max())
        line.append(f"{k}={err:.2e}/{bar:.0e}")
        assert err <= bar, (k, err)
    for k in ("loss", "enc_loss", "dec_loss"):
        rel = abs(float(out[k]) - float(g[k])) / abs(float(g[k]))
        line.append(f"{k} rel={rel:.2e}/1e-04")
        assert rel < 1e-4, (k, rel)
    print(f"F32DEC forward {name} " + " ".join(line))


def _assert_fixture_rows(g, key, W, got, tol):
    """every kept hypothesis of every utterance is the fixture's row, token for token, the score within tol -> largest score difference"""
    want = g[key + "/sequences"]
    worst = 0.0
    for b, h in enumerate(got):
        assert len(h["hypotheses"]) == W, (key, b)
        for k, (s, toks) in enumerate(h["hypotheses"]):
            row = want[b * W + k]
            assert toks == row[: len(toks)].tolist() and (row[len(toks):] == GM.PAD).all(), (key, b, k, toks, row)
            if W > 1:
                ds = abs(s - float(g[key + "/sequences_scores"][b * W + k]))
                worst = max(worst, ds)
                assert ds <= tol, (key, b, k, s, ds)
    return worst


@pytest.mark.parametrize("name", list(GM.CASES))
def test_generate_is_the_reference_generate_token_for_token(name):
    from huggingface_asr_amd.decoder import generate
    g, sd, x, am, dec_cfg = gen_case_inputs(name)
    eng = _joint(sd, dec_cfg)
    fl = am.sum(-1).to(DEV, torch.int32)
    decodes, worst = 0, 0.0
    for W, lp, es, ml in GM.SETTINGS:
        stats = {}
        got = generate(eng, x.to(DEV), fl, num_beams=W, max_length=ml, ctc_weight=0.3, length_penalty=lp, early_stopping=es, eos_token_id=GM.EOS, stats=stats)
        assert stats["kv_beams"] == W                                 # the shared layout, whatever the row count
        worst = max(worst, _assert_fixture_rows(g, GM.setting_key(W, lp, es, ml), W, got, BAR))
        decodes += len(got)
    print(f"F32DEC generate {name}: {decodes} of {decodes} utterance decodes equal the reference's token for token; max |dscore|={worst:.3e} (bar {BAR:.0e})")
    assert decodes == 22


@pytest.mark.parametrize("W", [1, 3, 5])
def test_generate_stepwise_equals_generate(W):
    from huggingface_asr_amd.decoder import generate, generate_stepwise
    g, sd, x, am, dec_cfg = gen_case_inputs("gen_tiny")
    eng = _joint(sd, dec_cfg)
    fl = am.sum(-1).to(DEV, torch.int32)
    kw = dict(num_beams=W, max_length=14, ctc_weight=0.3, eos_token_id=GM.EOS)
    a, b = generate(eng, x.to(DEV), fl, **kw), generate_stepwise(eng, x.to(DEV), fl, **kw)
    assert [h["hypotheses"] for h in a] == [h["hypotheses"] for h in b]
    # the eos / space trick decodes through the host loop with the fp32 step, unchanged
    space = a[0]["tokens"][2]
    t = dict(kw, space_token_id=space, apply_eos_space_trick=True, eos_space_trick_weight=0.5)
    assert [h["hypotheses"] for h in generate(eng, x.to(DEV), fl, **t)] == [h["hypotheses"] for h in generate_stepwise(eng, x.to(DEV), fl, **t)]


def test_model_level_switch():
    """config.hip_precision = "fp32": model.generate gives the fixture's rows; "bf16" rebuilds the engine; the default model's step logits keep their bits around it"""
    from test_surface_cpu import _joint_model
    from huggingface_asr_amd.decoding import GenerationConfigCustom
    g, sd, x, am, dec_cfg = gen_case_inputs("gen_tiny")
    model = _joint_model(False)
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not missing and not unexpected
    model = model.to(DEV).eval()
    W, lp, es, ml = 5, 1.0, False, 14
    model.generation_config = GenerationConfigCustom(bos_token_id=GM.START, pad_token_id=GM.PAD, decoder_start_token_id=GM.START, length_penalty=lp, early_stopping=es,
                                                     eos_token_id=GM.EOS, max_length=ml, num_beams=W, ctc_weight=0.3, ctc_margin=0, lm_weight=0, lm_model=None,
                                                     space_token_id=-1, apply_eos_space_trick=False, eos_space_trick_weight=1.0)
    gc = model.generation_config
    gc.num_return_sequences, gc.return_dict_in_generate, gc.output_scores = W, True, True

    def default_step_logits():
        eng = model._get_engine(DEV)
        assert eng.precision == "bf16"
        _, enc_bf, T2, key_len = eng.encode(x.to(DEV), am.sum(-1).to(DEV, torch.int32))
        kvs = eng.dec.cross_kv(enc_bf)
        cache = eng.dec.init_cache(x.shape[0], 4)
        return eng.dec.step(torch.full((x.shape[0], 1), GM.START, device=DEV), cache, kvs, T2, key_len).clone()
    before = default_step_logits()
    bf16_engine = model._engine
    model.config.hip_precision = "fp32"
    out = model.generate(input_values=x.to(DEV), attention_mask=am.to(DEV))
    assert model._engine is not bf16_engine and model._engine.precision == "fp32"
    key = GM.setting_key(W, lp, es, ml)
    want, want_sc = g[key + "/sequences"], g[key + "/sequences_scores"]
    seq = out.sequences.cpu().numpy()
    assert seq.shape[0] == want.shape[0] and (seq == want[:, : seq.shape[1]]).all() and (want[:, seq.shape[1]:] == GM.PAD).all()
    dsc = float(np.abs(out.sequences_scores.cpu().numpy() - want_sc).max())
    print(f"F32DEC model.generate hip_precision=fp32 max |dscore|={dsc:.3e}")
    assert dsc <= BAR
    with torch.no_grad():                                             # the eval forward runs in the mode too
        lab = torch.tensor([[5, 6, 7], [8, 9, -100]], device=DEV)
        o32 = model(input_values=x.to(DEV), attention_mask=am.to(DEV), labels=lab)
    assert o32.logits.dtype == torch.float32 and model._engine.precision == "fp32" and bool(torch.isfinite(o32.loss))
    model.config.hip_precision = "bf16"
    after = default_step_logits()
    assert model._engine.precision == "bf16" and model._engine is not bf16_engine
    assert torch.equal(before, after)
