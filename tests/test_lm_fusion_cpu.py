"""CPU: shallow-fusion LM rescoring (reference src/decoding/shallow_fussion.py, appended behind the CTC processor by
src/models/ctc_encoder_plus_autoregressive_decoder.py:398-403) — the oracle loop with the LM term against the reference's OWN generate() (fixture
tests/golden/gen_tiny_lm.npz, written by tests/golden/make_gen_lm.py), the packed layout of transformers' `GPT2LMHeadModel`, and what the drop-in `generate()` checks
about the LM before it touches a device."""
import numpy as np
import pytest
import torch

import gen_model as GM
import lm_model as LM
from helpers import AED_JCFG, gen_case_inputs, load_golden
from huggingface_asr_amd import shapes
from oracle import generate_ref as G

ENC = dict(shapes.TINY, ctc_zero_infinity=True, ctc_loss_reduction="mean")


def test_oracle_loop_with_the_lm_term_reproduces_the_reference_generate():
    """`generate_ref` with the score function wrapped as fn(ids) + float32(w) * log_softmax(LM(ids))[:, -1] (the LM: transformers' GPT2LMHeadModel, CPU, fp32) returns the
    fixture's sequences token for token, beam scores within 1e-5 — greedy and beams, with the CTC processor and without it (ctc_weight 0: raw logits for greedy)."""
    torch.set_num_threads(8)
    _, sd, x, am, dec_cfg = gen_case_inputs("gen_tiny")
    g = load_golden("gen_tiny_lm")
    lm = LM.tiny_lm()
    assert int(g["lm_seed"]) == LM.SEED and float(g["lm_weight"]) == LM.LM_WEIGHT
    psum = float(sum(float(p.double().sum()) for p in lm.parameters()))
    assert abs(psum - float(g["lm_param_sum"])) < 1e-6 * max(1.0, abs(psum)), "the LM's weights drifted from the fixture"
    base = load_golden("gen_tiny")
    for W, lp, es, ml, cw in LM.SETTINGS:
        key = LM.setting_key(W, lp, es, ml, cw)
        want = g[key + "/sequences"]
        fn, B = G.joint_score_fn(sd, ENC, dec_cfg, AED_JCFG, x, am, W, cw)
        fn = LM.with_lm(fn, lm, LM.LM_WEIGHT)
        if W == 1:
            seq = G.greedy(fn, B, max_length=ml, eos=GM.EOS, pad=GM.PAD, start=GM.START)
        else:
            seq, sc = G.beam_search(fn, B, W, GM.V, max_length=ml, eos=GM.EOS, pad=GM.PAD, start=GM.START, length_penalty=lp, early_stopping=es)
            assert np.abs(sc - g[key + "/sequences_scores"]).max() < 1e-5, key
        assert seq.shape == want.shape and (seq == want).all(), (key, seq, want)
        if cw == 0.3:                                           # the LM matters: the fixture differs from the one without it
            plain = base[GM.setting_key(W, lp, es, ml) + "/sequences"]
            L = max(plain.shape[1], want.shape[1])
            pad_to = lambda a: np.pad(a, ((0, 0), (0, L - a.shape[1])), constant_values=GM.PAD)
            assert (pad_to(plain) != pad_to(want)).any(), key


@pytest.mark.parametrize("tie", [True, False])
def test_lm_map_covers_the_gpt2_lm_head_model(tie):
    """`packing._lm_map` reads exactly the parameters of transformers' GPT2LMHeadModel (tied head: the token embedding only), packs Conv1D weights transposed, and its
    export functions give the reference tensors back."""
    from huggingface_asr_amd.decoder import lm_cfg_dict
    from huggingface_asr_amd.packing import _lm_map, lm_specs, mapped_fp32, packed
    lm = LM.random_lm(3, 128, 2, 2, 51, npos=16, tie=tie)
    names = {n for n, _ in lm.named_parameters()}
    assert ("lm_head.weight" in names) == (not tie)
    c = dict(lm_cfg_dict(lm.config), tie_word_embeddings=tie)
    m = _lm_map(c)
    keys = [k for r in m.values() for k, _ in r.pieces]
    assert sorted(keys) == sorted(names)
    sd = lm.state_dict()
    specs = lm_specs(c)
    assert [s.name for s in specs] == list(m)
    P = {s.name: t for s, t in packed(specs, m, mapped_fp32(m, sd, "cpu"))}
    assert P["h0.wqkv"].shape == (3 * 128, 128) and torch.equal(P["h0.wqkv"], sd["transformer.h.0.attn.c_attn.weight"].t())
    assert P["h1.wpr"].shape == (128, 4 * 128) and torch.equal(P["h1.wpr"], sd["transformer.h.1.mlp.c_proj.weight"].t())
    assert P["wpe"].shape == (16, 128)
    for name, r in m.items():
        for key, back in r.pieces:
            assert torch.equal(back(P[name]), sd[key]), key


def _cpu_model():
    from test_surface_cpu import _joint_model
    from huggingface_asr_amd.decoding import GenerationConfigCustom
    m = _joint_model(False).eval()
    m.generation_config = GenerationConfigCustom(pad_token_id=50, eos_token_id=1, decoder_start_token_id=2, num_beams=3, max_length=8, ctc_weight=0.3)
    return m


def test_generate_with_a_language_model_reaches_the_device_check():
    """`lm_weight` > 0 with a GPT2LMHeadModel is a valid request: on CPU inputs it gets as far as the "inputs must be on the GPU" error (no fallback) — as a keyword
    argument and inside the passed configuration, which is left holding the SAME module (no deep copy of the LM per call)."""
    import copy
    m = _cpu_model()
    x = torch.zeros(1, 200, 80)
    lm = LM.tiny_lm()
    with pytest.raises(RuntimeError, match="GPU"):
        m.generate(input_values=x, lm_weight=0.5, lm_model=lm)
    g = copy.copy(m.generation_config)
    g.lm_weight, g.lm_model = 0.5, lm
    with pytest.raises(RuntimeError, match="GPU"):
        m.generate(input_values=x, generation_config=g)
    assert g.lm_model is lm
    assert "_hfasr_lm_engine" not in lm.__dict__               # nothing was built for a request that never reached the device
    g.lm_weight = 0                                            # the weight gates: an LM with weight 0 is not looked at
    g.lm_model = torch.nn.Linear(2, 2)
    with pytest.raises(RuntimeError, match="GPU"):
        m.generate(input_values=x, generation_config=g)


def test_generate_refuses_language_models_it_cannot_run():
    m = _cpu_model()
    x = torch.zeros(1, 200, 80)
    with pytest.raises(NotImplementedError, match="lm_model"):
        m.generate(input_values=x, lm_weight=0.5)
    with pytest.raises(NotImplementedError, match="Linear"):
        m.generate(input_values=x, lm_weight=0.5, lm_model=torch.nn.Linear(2, 2))
    with pytest.raises(NotImplementedError, match="training"):
        m.generate(input_values=x, lm_weight=0.5, lm_model=LM.tiny_lm().train())
    with pytest.raises(ValueError, match="vocabulary"):
        m.generate(input_values=x, lm_weight=0.5, lm_model=LM.random_lm(3, 128, 1, 2, 37))
    with pytest.raises(ValueError, match="n_positions"):
        m.generate(input_values=x, lm_weight=0.5, lm_model=LM.random_lm(3, 128, 1, 2, 51, npos=6))     # max_length 8 feeds positions 0 .. 6
    for bad in (dict(n_head=4), dict(activation_function="relu"), dict(scale_attn_by_inverse_layer_idx=True), dict(reorder_and_upcast_attn=True),
                dict(add_cross_attention=True)):
        from transformers import GPT2Config, GPT2LMHeadModel
        lm = GPT2LMHeadModel(GPT2Config(**dict(dict(vocab_size=51, n_embd=128, n_layer=1, n_head=2, n_positions=16), **bad))).eval()
        with pytest.raises(NotImplementedError):
            m.generate(input_values=x, lm_weight=0.5, lm_model=lm)


def test_lm_engine_refuses_in_its_constructor():
    """head size not 64 / 128, another activation, the attention variants and cross-attention: refused by `GPT2LMEngine(cfg)` itself, before any device call"""
    from huggingface_asr_amd.decoder import GPT2LMEngine
    ok = dict(vocab_size=51, n_embd=128, n_layer=1, n_head=2, n_positions=16, activation_function="gelu_new")
    GPT2LMEngine(ok, "cpu")
    for bad in (dict(n_head=4), dict(activation_function="gelu"), dict(scale_attn_by_inverse_layer_idx=True), dict(reorder_and_upcast_attn=True),
                dict(add_cross_attention=True), dict(n_inner=256)):
        with pytest.raises(NotImplementedError):
            GPT2LMEngine(dict(ok, **bad), "cpu")


def test_new_entry_is_declared_and_bound():
    from huggingface_asr_amd import _lib
    assert len(_lib.SIGNATURES["mi_beam_step_lm"]) == len(_lib.SIGNATURES["mi_beam_step"]) + 4
    assert hasattr(_lib.lib(), "mi_beam_step_lm")
