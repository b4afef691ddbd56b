"""CPU: the host side of the fp32 inference mode of the joint model (decoder.py `precision="fp32"`, modeling_joint.py `hip_precision`; csrc/decoder_f32.hip): packed
dtypes, refusals, workspace queries, argument checks and the precision resolution all run without a GPU — nothing here launches a kernel.  (That the new header symbols
are exported with the binding's argument counts is tests/test_abi_cpu.py's test_header_symbols_exported.)"""
import ctypes as C

import pytest
import torch

from helpers import AED_JCFG, TINY_DEC, aed_case_inputs, load_golden
from huggingface_asr_amd import shapes

ENC = dict(shapes.TINY, ctc_zero_infinity=True, ctc_loss_reduction="mean")


@pytest.fixture(scope="module")
def lib():
    from huggingface_asr_amd import _lib
    from huggingface_asr_amd.csrc import build as B
    B.build()
    return _lib.lib()


@pytest.mark.parametrize("name,fixed", [("aed_tiny", False), ("aed_tiny_fixedpos", True)])
def test_fp32_engine_packs_every_tensor_in_fp32_in_the_default_engines_slots(name, fixed):
    from huggingface_asr_amd.decoder import GPT2DecoderEngine
    sd, _, _, _ = aed_case_inputs(load_golden(name))
    cfg = dict(TINY_DEC, pos_emb_fixed=fixed)
    a, b = GPT2DecoderEngine(cfg, "cpu"), GPT2DecoderEngine(cfg, "cpu", precision="fp32")
    assert a.precision == "bf16" and b.precision == "fp32"
    a.load_state_dict(sd); b.load_state_dict(sd)
    L = cfg["n_layer"]
    assert len(a._wtable) == len(b._wtable) == 5 + 18 * L
    mats = ("wqkv", "wo", "wq", "wkv", "wco", "wfc", "wpr")

    def flat(w):
        out = {"wte": w["wte"], "pos": w["pos"], "lnf_g": w["lnf"][0], "lnf_b": w["lnf"][1], "lm_head": w["lm_head"]}
        out.update({f"head{k}": t for k, t in enumerate(w["heads"])})
        for l, lw in enumerate(w["layers"]):
            for n, t in lw.items():
                if isinstance(t, tuple):
                    out[f"h{l}.{n}_g"], out[f"h{l}.{n}_b"] = t
                else:
                    out[f"h{l}.{n}"] = t
        return out
    fa, fb = flat(a.w), flat(b.w)
    assert fa.keys() == fb.keys() and len(fa) == 5 + 1 + 20 * L
    seen = 0
    for n in fa:
        is_mat = n.rpartition(".")[2] in mats or n == "lm_head" or n.startswith("head")
        assert fa[n].dtype == (torch.bfloat16 if is_mat else torch.float32), n           # the default engine's dtypes are what they were
        assert fb[n].dtype == torch.float32 and fb[n].shape == fa[n].shape, n
        assert torch.equal(fa[n], fb[n].to(fa[n].dtype)), n
        seen += int(is_mat)
    assert seen == 2 + 7 * L
    # a tied head is the embedding itself: one tensor, slot 4 = slot 0
    tied = {k: v for k, v in sd.items() if k != "decoder.lm_head.weight"}
    t = GPT2DecoderEngine(dict(cfg, tie_word_embeddings=True), "cpu", precision="fp32")
    t.load_state_dict(tied)
    assert t.w["lm_head"] is t.w["wte"] and t._wtable[4] == t._wtable[0]


def test_unknown_precision_is_a_value_error():
    from huggingface_asr_amd.decoder import GPT2DecoderEngine, GPT2LMEngine, JointAEDEngine
    from huggingface_asr_amd.whisper import WhisperDecoderEngine
    with pytest.raises(ValueError, match="precision"):
        GPT2DecoderEngine(dict(TINY_DEC), "cpu", precision="fp16")
    with pytest.raises(ValueError, match="precision"):
        JointAEDEngine(ENC, dict(TINY_DEC), AED_JCFG, "cpu", precision="fp16")
    with pytest.raises(ValueError, match="precision"):
        GPT2LMEngine(dict(vocab_size=51, n_embd=128, n_layer=1, n_head=2), "cpu", precision="fp16")
    with pytest.raises(ValueError, match="precision"):
        WhisperDecoderEngine(dict(d_model=128, decoder_attention_heads=2, decoder_layers=1, vocab_size=51, max_target_positions=16), "cpu", precision="fp16")


def test_fp32_refuses_what_it_does_not_cover():
    from huggingface_asr_amd.decoder import GPT2DecoderEngine, GPT2LMEngine, JointAEDEngine, generate, generate_stepwise
    from huggingface_asr_amd.whisper import WhisperDecoderEngine
    with pytest.raises(NotImplementedError, match="mixing"):
        GPT2DecoderEngine(dict(TINY_DEC, mixing_mode="scalar"), "cpu", precision="fp32")
    with pytest.raises(NotImplementedError, match="average_logits"):
        GPT2DecoderEngine(dict(TINY_DEC, average_logits=True), "cpu", precision="fp32")
    GPT2DecoderEngine(dict(TINY_DEC, mixing_mode="scalar"), "cpu")                        # the default mode still takes them
    GPT2DecoderEngine(dict(TINY_DEC, average_logits=True), "cpu")
    lm_cfg = dict(vocab_size=51, n_embd=128, n_layer=1, n_head=2, n_positions=64)
    with pytest.raises(NotImplementedError, match="shallow fusion"):
        GPT2LMEngine(lm_cfg, "cpu", precision="fp32")
    wcfg = dict(d_model=128, decoder_attention_heads=2, decoder_layers=1, vocab_size=51, max_target_positions=16)
    with pytest.raises(NotImplementedError, match="Whisper"):
        WhisperDecoderEngine(wcfg, "cpu", precision="fp32")
    WhisperDecoderEngine(wcfg, "cpu")
    # shallow fusion with an fp32 joint engine: refused on the host, before the device is touched (neither engine holds weights)
    joint = JointAEDEngine(ENC, dict(TINY_DEC), AED_JCFG, "cpu", precision="fp32")
    assert joint.enc.precision == joint.dec.precision == joint.precision == "fp32"
    lm = GPT2LMEngine(lm_cfg, "cpu")
    x = torch.zeros(1, 100, 80)
    for fn in (generate, generate_stepwise):
        with pytest.raises(NotImplementedError, match="shallow fusion"):
            fn(joint, x, None, num_beams=2, max_length=8, lm=lm, lm_weight=0.5)
    # what the fp32 encoder refuses keeps raising from the joint constructor
    with pytest.raises(NotImplementedError, match="gated"):
        JointAEDEngine(dict(ENC, context_awareness_type="gated"), dict(TINY_DEC), AED_JCFG, "cpu", precision="fp32")
    JointAEDEngine(dict(ENC, context_awareness_type="gated"), dict(TINY_DEC), AED_JCFG, "cpu")


def _gcfg(d, H, L=2, V=51):
    from huggingface_asr_amd import _lib
    return _lib.Gpt2Config(d=d, H=H, L=L, V=V, eps=1e-5)


def test_step_workspace_grows_with_rows_and_prompt_length(lib):
    ws = lambda B, U: int(lib.mi_decoder_step_f32_workspace_bytes(C.byref(_gcfg(768, 12, 6, 5000)), B, U))
    assert 0 < ws(1, 1) < ws(5, 1) < ws(50, 1) < ws(64, 1)
    assert 0 < ws(65, 1) < ws(100, 1) < ws(200, 1)                    # (above 64 rows the linears are mi_gemm_f32: no K-split partials in the workspace)
    assert ws(1, 1) < ws(1, 4) < ws(1, 16)
    assert ws(2, 4) > ws(2, 1) and ws(8, 1) > ws(2, 1)
    assert ws(0, 1) == 0 and ws(1, 0) == 0
    # the rows kernel's K-split partials: none where N alone fills the chip, (ksplit, M, N) floats where it does not
    assert int(lib.mi_linear_rows_f32_workspace_bytes(5, 50000, 768)) == 0
    n = int(lib.mi_linear_rows_f32_workspace_bytes(5, 768, 768))
    assert n > 0 and n % (5 * 768 * 4) == 0
    assert int(lib.mi_linear_rows_f32_workspace_bytes(10, 768, 768)) == 2 * n            # the plan does not depend on M


def test_unsupported_shapes_return_minus_three_before_any_launch(lib):
    # no pointer below is ever dereferenced
    assert lib.mi_linear_rows_f32(None, 0, None, 0, None, 0, None, 0, 0, None, None, 0, 0, 0, 0, 1, 8, 6, None, 0, None) == -3        # K % 4 != 0
    assert lib.mi_linear_rows_f32(None, 0, None, 0, None, 0, None, 0, 0, None, None, 0, 0, 0, 0, 1, 8, 130, None, 0, None) == -3
    assert lib.mi_linear_rows_f32(None, 8, None, 8, None, 0, None, 8, 0, None, None, 0, 0, 0, 0, 1, 8, 8, None, 0, None) == -1         # a supported shape: null operands
    assert lib.mi_linear_rows_f32(None, 8, None, 8, None, 0, None, 8, 0, None, None, 0, 0, 0, 0, 65, 8, 8, None, 0, None) == -1        # more than 64 rows
    step = lambda cfg: lib.mi_decoder_step_f32(C.byref(cfg), None, None, 1, 1, 1, 0, 8, None, None, None, 10, None, 1.0, None, None, 0, None, 64, None)
    assert step(_gcfg(64, 2)) == -3                                   # head size 32
    assert step(_gcfg(512, 2)) == -3                                  # head size 256
    assert step(_gcfg(128, 2)) == -1                                  # head size 64: the null tables
    assert lib.mi_attention_general_f32(None, 0, None, 0, None, 0, None, None, 0, 1, 1, 1, 1, 0, 2, 32, 1.0, 0, None) == -3


def test_joint_model_precision_resolution_order_and_training_refusal(monkeypatch):
    """config.hip_precision, then HFASR_PRECISION, then "bf16"; the engine follows the value; the training forward refuses fp32"""
    from test_surface_cpu import _joint_model
    model = _joint_model(False)
    monkeypatch.delenv("HFASR_PRECISION", raising=False)
    assert model._precision() == "bf16"
    assert model._get_engine("cpu").precision == "bf16"
    monkeypatch.setenv("HFASR_PRECISION", "fp32")
    assert model._precision() == "fp32"
    eng = model._get_engine("cpu")
    assert eng.precision == eng.enc.precision == eng.dec.precision == "fp32"
    assert eng.dec.w["layers"][0]["wqkv"].dtype == torch.float32 and eng.proj[0].dtype == torch.float32
    model.config.hip_precision = "bf16"                               # the config wins over the environment
    assert model._precision() == "bf16"
    eng2 = model._get_engine("cpu")
    assert eng2 is not eng and eng2.precision == "bf16" and eng2.dec.w["layers"][0]["wqkv"].dtype == eng2.proj[0].dtype == torch.bfloat16      # a changed value rebuilds the engine
    model.config.hip_precision = None
    assert model._precision() == "fp32"
    model.train()
    with pytest.raises(NotImplementedError, match="fp32"):
        model(input_values=torch.zeros(1, 100, 80), labels=torch.zeros(1, 3, dtype=torch.long))
    monkeypatch.setenv("HFASR_PRECISION", "fp8")
    with pytest.raises(ValueError, match="precision"):
        model._get_engine("cpu")
