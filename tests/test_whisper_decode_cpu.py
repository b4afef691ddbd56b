"""CPU: the host side of Whisper decoding on the HIP path — the packing of a transformers `WhisperDecoder` state dict into the token step's table, the suppression
vectors, what `hip_generate` refuses before it touches a device, and the two new `mi_gpt2_config` fields."""
import pytest
import torch

from huggingface_asr_amd import packing

CFG = dict(d_model=128, decoder_layers=2, decoder_attention_heads=2, decoder_ffn_dim=512, vocab_size=120, max_target_positions=40, activation_function="gelu",
           scale_embedding=False)


def _hf_model(**over):
    from transformers import WhisperConfig, WhisperForConditionalGeneration
    kw = dict(d_model=128, encoder_layers=1, decoder_layers=2, encoder_attention_heads=2, decoder_attention_heads=2, encoder_ffn_dim=256, decoder_ffn_dim=512,
              num_mel_bins=80, max_source_positions=100, max_target_positions=40, vocab_size=120, pad_token_id=0, bos_token_id=1, eos_token_id=2,
              decoder_start_token_id=1, suppress_tokens=None, begin_suppress_tokens=None)
    kw.update(over)
    torch.manual_seed(0)
    return WhisperForConditionalGeneration(WhisperConfig(**kw)).eval()


def test_packing_of_a_transformers_decoder_state_dict():
    dec = _hf_model().model.decoder
    sd = dec.state_dict()
    d, V = 128, 120
    m = packing._whisper_dec_map(CFG)
    specs = packing.whisper_decoder_specs(CFG)
    P = {s.name: t for s, t in packing.packed(specs, m, packing.mapped_fp32(m, sd, "cpu"))}
    want = {"wte": (V, d), "wpe": (40, d), "lnf_g": (d,), "lnf_b": (d,)}
    for l in range(2):
        p = f"h{l}."
        want.update({p + "ln1_g": (d,), p + "ln1_b": (d,), p + "wqkv": (3 * d, d), p + "bqkv": (3 * d,), p + "wo": (d, d), p + "bo": (d,), p + "lnc_g": (d,), p + "lnc_b": (d,),
                     p + "wq": (d, d), p + "bq": (d,), p + "wkv": (2 * d, d), p + "bkv": (2 * d,), p + "wco": (d, d), p + "bco": (d,), p + "ln2_g": (d,), p + "ln2_b": (d,),
                     p + "wfc": (4 * d, d), p + "bfc": (4 * d,), p + "wpr": (d, 4 * d), p + "bpr": (d,)})
    assert {k: tuple(v.shape) for k, v in P.items()} == want
    assert len(specs) == 4 + 2 * 20                                                 # the step's 18 per layer + the cross K/V pair, which cross_kv() reads
    for l in range(2):
        r = f"layers.{l}."
        assert torch.equal(P[f"h{l}.wqkv"], torch.cat([sd[r + f"self_attn.{n}_proj.weight"] for n in "qkv"], 0))
        assert torch.equal(P[f"h{l}.bqkv"][:d], sd[r + "self_attn.q_proj.bias"]) and torch.equal(P[f"h{l}.bqkv"][2 * d:], sd[r + "self_attn.v_proj.bias"])
        assert float(P[f"h{l}.bqkv"][d:2 * d].abs().max()) == 0.0                   # k_proj has no bias
        assert torch.equal(P[f"h{l}.wkv"], torch.cat([sd[r + "encoder_attn.k_proj.weight"], sd[r + "encoder_attn.v_proj.weight"]], 0))
        assert float(P[f"h{l}.bkv"][:d].abs().max()) == 0.0 and torch.equal(P[f"h{l}.bkv"][d:], sd[r + "encoder_attn.v_proj.bias"])
        assert torch.equal(P[f"h{l}.wfc"], sd[r + "fc1.weight"]) and torch.equal(P[f"h{l}.wpr"], sd[r + "fc2.weight"])
        assert torch.equal(P[f"h{l}.ln2_g"], sd[r + "final_layer_norm.weight"]) and torch.equal(P[f"h{l}.lnc_b"], sd[r + "encoder_attn_layer_norm.bias"])
    assert torch.equal(P["wte"], sd["embed_tokens.weight"]) and torch.equal(P["wpe"], sd["embed_positions.weight"])
    # the engine: the tied head is the bf16 image of embed_tokens, the table has 5 + 18 L pointers
    from huggingface_asr_amd.whisper import WhisperDecoderEngine
    eng = WhisperDecoderEngine(CFG, "cpu")
    eng.load_state_dict(sd)
    assert eng.w["lm_head"].dtype == torch.bfloat16 and torch.equal(eng.w["lm_head"], sd["embed_tokens.weight"].to(torch.bfloat16))
    assert eng.w["wte"].dtype == torch.float32 and len(eng._wtable) == 5 + 18 * 2 and eng.w["scale"] == 1.0
    assert eng.w["layers"][1]["wqkv"].dtype == torch.bfloat16 and eng.w["layers"][1]["bqkv"].dtype == torch.float32
    assert (eng._gcfg.act, eng._gcfg.d, eng._gcfg.H, eng._gcfg.L, eng._gcfg.V) == (1, 128, 2, 2, 120)
    eng2 = WhisperDecoderEngine(dict(CFG, scale_embedding=True), "cpu")
    eng2.load_state_dict(sd)
    assert abs(eng2.w["scale"] - 128 ** 0.5) < 1e-6
    bad = {k: v for k, v in sd.items() if k != "layers.1.encoder_attn.k_proj.weight"}
    with pytest.raises(KeyError, match="encoder_attn.k_proj.weight"):
        WhisperDecoderEngine(CFG, "cpu").load_state_dict(bad)
    with pytest.raises(ValueError, match="max_target_positions"):
        eng.ensure_positions(41)
    eng.ensure_positions(40)


def test_engine_refuses_shapes_the_step_does_not_run():
    from huggingface_asr_amd.whisper import WhisperDecoderEngine
    with pytest.raises(NotImplementedError, match="head size"):
        WhisperDecoderEngine(dict(CFG, decoder_attention_heads=1), "cpu")
    with pytest.raises(NotImplementedError, match="decoder_ffn_dim"):
        WhisperDecoderEngine(dict(CFG, decoder_ffn_dim=256), "cpu")
    with pytest.raises(NotImplementedError, match="activation"):
        WhisperDecoderEngine(dict(CFG, activation_function="relu"), "cpu")


def test_suppression_vectors():
    every, first = packing.suppression_vectors(10, [1, 7], [0, 3])
    ninf = float("-inf")
    assert every.dtype == torch.float32 and every.tolist() == [0, ninf, 0, 0, 0, 0, 0, ninf, 0, 0]
    assert first.tolist() == [ninf, ninf, 0, ninf, 0, 0, 0, ninf, 0, 0]              # the begin-only ids 0 and 3 sit in the first vector only
    assert packing.suppression_vectors(10) == (None, None)
    every, first = packing.suppression_vectors(10, None, [9])
    assert every is None and first.tolist() == [0] * 9 + [ninf]
    every, first = packing.suppression_vectors(10, [2], None)
    assert torch.equal(every, first) and every[2] == ninf
    for bad in ([10], [-1], [3, 99]):
        with pytest.raises(ValueError):
            packing.suppression_vectors(10, bad, None)
        with pytest.raises(ValueError):
            packing.suppression_vectors(10, None, bad)


def test_hip_generate_refuses_before_any_device_call():
    from huggingface_asr_amd.whisper import hip_generate
    m = _hf_model()
    x = torch.zeros(1, 80, 200)
    for kw in (dict(num_beams=2), dict(do_sample=True), dict(return_timestamps=True), dict(language="en"), dict(task="translate"), dict(logits_processor=[lambda i, s: s]),
               dict(stopping_criteria=[lambda i, s: False])):
        with pytest.raises(NotImplementedError):
            hip_generate(m, x, max_new_tokens=4, **kw)
    with pytest.raises(NotImplementedError, match="input features"):
        hip_generate(m, torch.zeros(80, 150), max_new_tokens=4)
    with pytest.raises(NotImplementedError, match="input features"):
        hip_generate(m, torch.zeros(1, 80, 3000), max_new_tokens=4)
    with pytest.raises(ValueError, match="max_target_positions"):
        hip_generate(m, x, decoder_input_ids=torch.ones(1, 3, dtype=torch.long), max_new_tokens=38)
    with pytest.raises(RuntimeError, match="GPU"):
        hip_generate(m, x, max_new_tokens=4)
    assert "_hfasr_engine" not in m.model.decoder.__dict__ and "_hfasr_engine" not in m.model.encoder.__dict__     # nothing was built on the way


def test_step_config_carries_the_new_fields_and_gpt2_keeps_its_own():
    from huggingface_asr_amd import _lib
    from huggingface_asr_amd.decoder import GPT2DecoderEngine
    names = [n for n, _ in _lib.Gpt2Config._fields_]
    assert names == ["d", "H", "L", "V", "eps", "step_form", "act"]
    c = _lib.Gpt2Config(d=1, H=1, L=1, V=1, eps=1e-5, step_form=2, act=1)
    assert (c.step_form, c.act) == (2, 1)
    for f in ("mi_decoder_step", "mi_linear_rows", "mi_linear_rows_workspace_bytes", "mi_greedy_advance"):
        assert f in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["mi_decoder_step"]) == len(_lib.SIGNATURES["mi_gpt2_step"]) + 1
    import gen_model as GM
    from helpers import gen_case_inputs
    g, sd, x, am, dec_cfg = gen_case_inputs("gen_tiny")
    eng = GPT2DecoderEngine(dec_cfg, "cpu")
    eng.load_state_dict(sd, "decoder.")
    assert (eng._gcfg.act, eng._gcfg.step_form) == (0, 0)
