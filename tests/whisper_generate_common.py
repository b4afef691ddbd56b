"""Shared by tests/test_whisper_generate_cpu.py and tests/test_gpu_whisper_generate.py: the tiny multilingual Whisper model of both, its inputs, and the undo of
`install_whisper(generate=True)`."""
import numpy as np
import torch

from huggingface_asr_amd import synth

LANG_TO_ID = {"<|en|>": 100, "<|de|>": 101, "<|fr|>": 102, "<|es|>": 103}
TASK_TO_ID = {"transcribe": 104, "translate": 105}
NO_TIMESTAMPS = 109                         # ten timestamp tokens: 110 .. 119
SEED = 31


def fill(module, seed):
    """the module's state dict re-drawn from synth.uniform: matrices +-sqrt(3 / fan_in), embeddings and biases +-0.1, LayerNorm weights 1 +- 0.1"""
    sd = {}
    for k, v in module.state_dict().items():
        shape = tuple(v.shape)
        if "layer_norm" in k:
            t = synth.uniform(seed, k, shape, -0.1, 0.1) + (1.0 if k.endswith("weight") else 0.0)
        elif "embed_" in k or k.endswith("bias"):
            t = synth.uniform(seed, k, shape, -0.1, 0.1)
        else:
            a = float(np.sqrt(3.0 / int(np.prod(shape[1:]))))
            t = synth.uniform(seed, k, shape, -a, a)
        sd[k] = torch.from_numpy(t.astype(np.float32))
    module.load_state_dict(sd, strict=True)


def tiny_model(seed=SEED, **gen):
    """d 128, 2 + 2 layers, 2 heads, 100 source positions, 40 target positions, V 120, eos 2, start 1; a multilingual generation config on four languages, two tasks and
    ten timestamp tokens"""
    from transformers import WhisperConfig, WhisperForConditionalGeneration
    cfg = WhisperConfig(d_model=128, encoder_layers=2, decoder_layers=2, encoder_attention_heads=2, decoder_attention_heads=2, encoder_ffn_dim=256, decoder_ffn_dim=512,
                        num_mel_bins=80, max_source_positions=100, max_target_positions=40, vocab_size=120, pad_token_id=0, bos_token_id=1, eos_token_id=2,
                        decoder_start_token_id=1, suppress_tokens=None, begin_suppress_tokens=None)
    torch.manual_seed(0)
    model = WhisperForConditionalGeneration(cfg)
    fill(model.model, seed)
    model = model.eval()
    gc = model.generation_config
    gc.eos_token_id, gc.pad_token_id, gc.decoder_start_token_id = 2, 0, 1
    gc.lang_to_id, gc.task_to_id, gc.no_timestamps_token_id, gc.is_multilingual = dict(LANG_TO_ID), dict(TASK_TO_ID), NO_TIMESTAMPS, True
    gc.suppress_tokens, gc.begin_suppress_tokens = [5, 17], [2, 9]
    for k, v in gen.items():
        setattr(gc, k, v)
    return model


def features(B, tag="gen_feats"):
    return torch.from_numpy(synth.normal(SEED, tag, (B, 80, 200), 0.5))


def restore_generate():
    """undo `install_whisper(generate=True)`: other test modules assert that a default binding leaves `generate` transformers' own (the class inherits it)"""
    from transformers.models.whisper import modeling_whisper as MW
    cls = MW.WhisperForConditionalGeneration
    for name in ("generate", "_hfasr_reference_generate"):
        if name in cls.__dict__:
            delattr(cls, name)
