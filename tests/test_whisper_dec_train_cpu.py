"""CPU: the opt-in binding of Whisper decoder training — where a `WhisperDecoder.forward` call is routed (`whisper.decoder_route`, a pure function of the raw keyword
arguments), what `install_whisper` replaces with and without its switches, how the environment switches reach it, and that CPU tensors run transformers' own forward."""
import types

import pytest
import torch


def _cfg(**kw):
    return types.SimpleNamespace(**dict(dict(dropout=0.0, attention_dropout=0.0, activation_dropout=0.0, output_attentions=False, output_hidden_states=False), **kw))


GPU, CPU = types.SimpleNamespace(is_cuda=True), types.SimpleNamespace(is_cuda=False)


def _route(training=True, cfg=None, **kw):
    from huggingface_asr_amd.whisper import decoder_route
    return decoder_route(dict(dict(input_ids=GPU, encoder_hidden_states=GPU), **kw), training=training, cfg=cfg or _cfg())


def test_routing_predicate():
    assert _route() == ("hip", None)
    assert _route(use_cache=None) == ("hip", None) and _route(use_cache=False) == ("hip", None)
    assert _route(training=False) == ("hip", None)
    assert _route(output_attentions=False, output_hidden_states=None, attention_mask=None) == ("hip", None)
    assert _route(num_items_in_batch=12, return_dict=True) == ("hip", None)          # what Trainer adds; nothing reads it
    assert _route(return_dict=False)[0] == "stock"
    # cached calls (everything `generate` does): transformers' forward, silently
    assert _route(use_cache=True) == ("stock", None)
    assert _route(past_key_values=object()) == ("stock", None)
    assert _route(past_key_values=object(), use_cache=True, attention_mask=GPU, cfg=_cfg(dropout=0.1)) == ("stock", None)
    # cache-less calls the HIP path does not cover: transformers' forward, with a reason
    for kw in (dict(input_ids=None, inputs_embeds=GPU), dict(inputs_embeds=GPU), dict(encoder_hidden_states=None), dict(attention_mask=GPU), dict(position_ids=GPU),
               dict(output_attentions=True), dict(output_hidden_states=True), dict(cfg=_cfg(output_attentions=True)), dict(cfg=_cfg(output_hidden_states=True)),
               dict(input_ids=CPU), dict(encoder_hidden_states=CPU), dict(cache_position=GPU),
               dict(cfg=_cfg(dropout=0.1)), dict(cfg=_cfg(attention_dropout=0.1)), dict(cfg=_cfg(activation_dropout=0.1))):
        where, why = _route(**kw)
        assert where == "stock" and why, kw
    assert "dropout" in _route(cfg=_cfg(dropout=0.1))[1] and "CPU" in _route(input_ids=CPU)[1]
    assert _route(training=False, cfg=_cfg(dropout=0.1)) == ("hip", None)            # dropout is inactive outside training


@pytest.fixture
def whisper_classes():
    """transformers' three Whisper classes with whatever `forward` they have now, put back afterwards (attributes the install adds included)"""
    from transformers.models.whisper import modeling_whisper as MW
    classes = (MW.WhisperEncoder, MW.WhisperDecoder, MW.WhisperForConditionalGeneration)
    before = [(c, c.forward, c.__dict__.get("_hfasr_reference_forward")) for c in classes]
    yield MW
    for c, fwd, ref in before:
        c.forward = fwd
        if ref is None:
            if "_hfasr_reference_forward" in c.__dict__:
                del c._hfasr_reference_forward
        else:
            c._hfasr_reference_forward = ref


def test_install_without_arguments_leaves_decoder_and_model_untouched(whisper_classes):
    MW = whisper_classes
    from huggingface_asr_amd.whisper import hip_whisper_encoder_forward, install_whisper
    dec, lm = MW.WhisperDecoder.forward, MW.WhisperForConditionalGeneration.forward
    install_whisper()
    assert MW.WhisperEncoder.forward is hip_whisper_encoder_forward
    assert MW.WhisperDecoder.forward is dec and MW.WhisperForConditionalGeneration.forward is lm


def test_install_decoder_is_idempotent_and_keeps_the_reference(whisper_classes):
    MW = whisper_classes
    from huggingface_asr_amd.whisper import hip_whisper_decoder_forward, hip_whisper_lm_forward, install_whisper
    dec, lm = MW.WhisperDecoder.forward, MW.WhisperForConditionalGeneration.forward
    install_whisper(decoder=True)
    install_whisper(decoder=True)
    assert MW.WhisperDecoder.forward is hip_whisper_decoder_forward and MW.WhisperDecoder._hfasr_reference_forward is dec
    assert MW.WhisperForConditionalGeneration.forward is lm
    install_whisper(fused_loss=True)                                # implies the decoder; the decoder's reference stays the original
    install_whisper(fused_loss=True)
    assert MW.WhisperDecoder._hfasr_reference_forward is dec
    assert MW.WhisperForConditionalGeneration.forward is hip_whisper_lm_forward and MW.WhisperForConditionalGeneration._hfasr_reference_forward is lm


def test_fused_loss_alone_installs_the_decoder_too(whisper_classes):
    MW = whisper_classes
    from huggingface_asr_amd.whisper import hip_whisper_decoder_forward, install_whisper
    if getattr(MW.WhisperDecoder.forward, "_hfasr_hip", False):
        MW.WhisperDecoder.forward = MW.WhisperDecoder._hfasr_reference_forward
    install_whisper(fused_loss=True)
    assert MW.WhisperDecoder.forward is hip_whisper_decoder_forward


@pytest.mark.parametrize("env,want", [({}, (False, False)), ({"HFASR_WHISPER_DECODER": "1"}, (True, False)), ({"HFASR_WHISPER_FUSED_LOSS": "1"}, (False, True)),
                                      ({"HFASR_WHISPER_DECODER": "1", "HFASR_WHISPER_FUSED_LOSS": "1"}, (True, True)), ({"HFASR_WHISPER_DECODER": "0"}, (False, False))])
def test_environment_switches_reach_install_whisper(monkeypatch, env, want):
    """`bind.install()` ends in `bind_all()` (the reference's trainers call it again themselves), which reads the switches"""
    import inspect

    from huggingface_asr_amd import bind, whisper
    seen = []
    monkeypatch.setattr(whisper, "install_whisper", lambda decoder=False, fused_loss=False: seen.append((decoder, fused_loss)))
    for k in ("HFASR_WHISPER_DECODER", "HFASR_WHISPER_FUSED_LOSS"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    bind.bind_all()
    assert seen == [want]
    assert inspect.getsource(bind.install).rstrip().endswith("bind_all()")


def _tiny():
    from transformers import WhisperConfig
    return WhisperConfig(d_model=128, encoder_layers=1, decoder_layers=1, encoder_attention_heads=2, decoder_attention_heads=2, encoder_ffn_dim=256, decoder_ffn_dim=512,
                         num_mel_bins=80, max_source_positions=16, max_target_positions=16, vocab_size=50, pad_token_id=0, bos_token_id=1, eos_token_id=2,
                         decoder_start_token_id=1, suppress_tokens=None, begin_suppress_tokens=None)


def test_cpu_tensors_run_transformers_forward(whisper_classes, monkeypatch):
    MW = whisper_classes
    from huggingface_asr_amd import whisper
    monkeypatch.delenv("HFASR_WHISPER_STRICT", raising=False)
    torch.manual_seed(0)
    dec = MW.WhisperDecoder(_tiny()).eval()
    ids, enc = torch.randint(0, 50, (2, 5)), torch.randn(2, 16, 128)
    with torch.no_grad():
        want = dec(input_ids=ids, encoder_hidden_states=enc, use_cache=False).last_hidden_state
    whisper.install_whisper(decoder=True, fused_loss=True)
    whisper._stock_decoder_forward.said.clear()
    with pytest.warns(UserWarning, match="CPU tensors"), torch.no_grad():
        got = dec(input_ids=ids, encoder_hidden_states=enc)
    assert torch.equal(got.last_hidden_state, want)
    monkeypatch.setenv("HFASR_WHISPER_STRICT", "1")
    with pytest.raises(NotImplementedError, match="CPU tensors"):
        dec(input_ids=ids, encoder_hidden_states=enc)
    with torch.no_grad():                                            # a cached call stays silent and allowed under STRICT
        dec(input_ids=ids, encoder_hidden_states=enc, use_cache=True)
    # the language-model wrapper: CPU labels decline the fused loss, the original forward returns logits
    monkeypatch.delenv("HFASR_WHISPER_STRICT", raising=False)
    model = MW.WhisperForConditionalGeneration(_tiny()).train()
    labels = torch.randint(3, 50, (2, 5))
    assert whisper.fused_loss_route(model, dict(input_features=torch.randn(2, 80, 32), labels=labels)) is False
    MW.WhisperEncoder.forward = MW.WhisperEncoder._hfasr_reference_forward if getattr(MW.WhisperEncoder.forward, "_hfasr_hip", False) else MW.WhisperEncoder.forward
    out = model(input_features=torch.randn(2, 80, 32), labels=labels)
    assert out.logits is not None and out.logits.shape == (2, 5, 50) and bool(torch.isfinite(out.loss))
