"""Drop-in `Wav2Vec2EBranchformerForCTC` whose forward runs on the HIP engine.

Mirrors the reference class surface (src/models/encoders/e_branchformer.py:408-496): same constructor, same
state-dict keys (huggingface_asr_amd/shapes.py), same forward signature / `CausalLMOutput`, same ValueError for
out-of-vocabulary labels, `freeze_encoder()`, `_get_feat_extract_output_lengths` (the UN-padded outer formula the
reference inherits from Wav2Vec2ForCTC) and `_get_feature_vector_attention_mask`.  The nn.Modules below only HOLD the
parameters (for state_dict / optimizers / checkpoint averaging); no tensor op of the forward goes through them.

Eval mode / no_grad: the inference engine (engine.py).  Training mode with labels: forward AND backward run on the HIP trainer
(train.py) behind a torch.autograd bridge (autograd_bridge.py), so `loss.backward()` fills ordinary `.grad`s for HF Trainer's
optimizer; dropout, LayerDrop, in-model SpecAugment (counter-based masks) and causal (streaming) encoders are supported; configurations the HIP training
step does not cover raise NotImplementedError rather than silently falling back to PyTorch."""
from __future__ import annotations

import os
from typing import NamedTuple, Optional, Tuple, Union

import torch
from torch import nn
from transformers import PreTrainedModel
from transformers.modeling_outputs import CausalLMOutput

from . import ops
from .configuration_ebranchformer import Wav2Vec2EBranchformerConfig
from .engine import EBranchformerEngine, cfg_from_hf


def _dropout_seed() -> int:
    """dropout-mask seed of the HIP training step: torch's seed (set by HF Trainer's set_seed) offset by the data-parallel rank"""
    rank = torch.distributed.get_rank() if torch.distributed.is_available() and torch.distributed.is_initialized() else 0
    return (torch.initial_seed() + 7919 * rank) & 0xFFFFFFFF


class CTCAlignment(NamedTuple):
    """what `Wav2Vec2EBranchformerForCTC.align` returns (frames are encoder output frames)"""
    path: torch.Tensor
    score: torch.Tensor
    start: torch.Tensor
    end: torch.Tensor
    token_lp: torch.Tensor
    n_tokens: torch.Tensor


class _Holder(nn.Module):
    """parameter container; calling it is a bug"""

    def forward(self, *a, **k):  # pragma: no cover
        raise RuntimeError("parameter holder: the forward pass runs in the HIP engine")


def _ln(d):
    return nn.LayerNorm(d)


class _FFN(_Holder):
    def __init__(self, d, i):
        super().__init__()
        self.intermediate_dense = nn.Linear(d, i)
        self.output_dense = nn.Linear(i, d)


class _SelfAttn(_Holder):
    def __init__(self, cfg):
        super().__init__()
        d, H = cfg.hidden_size, cfg.num_attention_heads
        self.linear_q, self.linear_k, self.linear_v, self.linear_out = (nn.Linear(d, d) for _ in range(4))
        if cfg.position_embeddings_type == "relative":
            self.linear_pos = nn.Linear(d, d, bias=False)
            self.pos_bias_u = nn.Parameter(torch.zeros(H, d // H))
            self.pos_bias_v = nn.Parameter(torch.zeros(H, d // H))


class _CSGU(_Holder):
    def __init__(self, cfg):
        super().__init__()
        c = cfg.intermediate_size // 2
        self.norm = _ln(c)
        self.conv = nn.Conv1d(c, c, cfg.csgu_kernel_size, 1, (cfg.csgu_kernel_size - 1) // 2, groups=c)
        if cfg.csgu_use_linear_after_conv:
            self.linear = nn.Linear(c, c)


class _CgMLP(_Holder):
    def __init__(self, cfg):
        super().__init__()
        self.channel_proj1 = nn.Sequential(nn.Linear(cfg.hidden_size, cfg.intermediate_size), nn.GELU())
        self.csgu = _CSGU(cfg)
        self.channel_proj2 = nn.Linear(cfg.intermediate_size // 2, cfg.hidden_size)


class _Layer(_Holder):
    def __init__(self, cfg):
        super().__init__()
        d = cfg.hidden_size
        if cfg.use_macaron_ff:
            self.ff1 = nn.Sequential(_ln(d), _FFN(d, cfg.intermediate_size))
        self.self_attn_layer_norm = _ln(d)
        self.self_attn = _SelfAttn(cfg)
        self.cgMLP = _CgMLP(cfg)
        self.cgMLP_layer_norm = _ln(d)
        self.merge_proj = nn.Linear(2 * d, d)
        self.depthwise_conv_fusion = nn.Conv1d(2 * d, 2 * d, cfg.merge_conv_kernel, 1, (cfg.merge_conv_kernel - 1) // 2, groups=2 * d)
        self.final_layer_norm = _ln(d)
        if cfg.use_macaron_ff:
            self.ff2 = nn.Sequential(_ln(d), _FFN(d, cfg.intermediate_size))


class _Gated(_Holder):      # GatedConv2d / GatedConv2dShared (extractors.py:23-54): .conv and .gate; the shared gate is a (4k, k) / stride (4s, s) / padding (4p, p) conv
    def __init__(self, cin, cout, k, s, p, share):
        super().__init__()
        self.conv = nn.Conv2d(cin, cout, (k, k), stride=(s, s), padding=p)
        self.gate = nn.Conv2d(cin, cout, (k * share, k), stride=(s * share, s), padding=(p * share, p))


class _ConvWrap(_Holder):   # ContextAwareConv2d: the extra ".conv" level of the non-causal key (extractors.py:57-65)
    def __init__(self, cin, cout, k, s, p=1, mode=0):
        super().__init__()
        # the reference's dict lookup: "gated" / "gated_shared" select a gate, anything else (None, the recipes' `shared_gated`, ...) is the plain nn.Conv2d
        self.conv = _Gated(cin, cout, k, s, p, 4 if mode == 2 else 1) if mode else nn.Conv2d(cin, cout, k, stride=s)


class _FeatureExtractor(_Holder):
    def __init__(self, cfg):
        super().__init__()
        from .shapes import context_mode, conv_freq_out
        blocks, cin = [], 1
        mode = context_mode(dict(is_causal=cfg.is_causal, context_awareness_type=getattr(cfg, "context_awareness_type", None)))
        for c, k, s, p in zip(cfg.conv_dim, cfg.conv_kernel, cfg.conv_stride, cfg.conv_padding):
            conv = nn.Conv2d(cin, c, k, stride=s) if cfg.is_causal else _ConvWrap(cin, c, k, s, p, mode)
            blocks.append(nn.Sequential(conv, nn.GELU()))
            cin = c
        self.conv = nn.Sequential(*blocks)
        fo = conv_freq_out(cfg.num_fbanks, cfg.conv_kernel, cfg.conv_stride, cfg.conv_padding)
        self.out = nn.Linear(cfg.conv_dim[-1] * fo, cfg.hidden_size)


class _FeatureProjection(_Holder):
    def __init__(self, cfg):
        super().__init__()
        self.layer_norm = nn.LayerNorm(cfg.hidden_size, eps=cfg.layer_norm_eps)
        self.projection = nn.Linear(cfg.hidden_size, cfg.hidden_size)


class _RotaryBuf(_Holder):
    def __init__(self, cfg):
        super().__init__()
        hd = cfg.hidden_size // cfg.num_attention_heads
        self.register_buffer("inv_freq", 1.0 / (cfg.rotary_embedding_base ** (torch.arange(0, hd, 2, dtype=torch.int64).float() / hd)))


class _Encoder(_Holder):
    def __init__(self, cfg):
        super().__init__()
        if cfg.position_embeddings_type == "rotary":
            self.embed_positions = _RotaryBuf(cfg)       # persistent `inv_freq` buffer is part of the reference state dict
        self.layer_norm = nn.LayerNorm(cfg.hidden_size, eps=cfg.layer_norm_eps)
        self.layers = nn.ModuleList([_Layer(cfg) for _ in range(cfg.num_hidden_layers)])


class _Wav2Vec2(_Holder):
    def __init__(self, cfg):
        super().__init__()
        self.feature_extractor = _FeatureExtractor(cfg)
        self.feature_projection = _FeatureProjection(cfg)
        if cfg.mask_time_prob > 0.0 or cfg.mask_feature_prob > 0.0:
            self.masked_spec_embed = nn.Parameter(torch.Tensor(cfg.hidden_size).uniform_())
        self.encoder = _Encoder(cfg)


class Wav2Vec2EBranchformerForCTC(PreTrainedModel):
    config_class = Wav2Vec2EBranchformerConfig
    base_model_prefix = "wav2vec2"
    main_input_name = "input_values"
    supports_gradient_checkpointing = False

    def __init__(self, config: Wav2Vec2EBranchformerConfig):
        super().__init__(config)
        self.wav2vec2 = _Wav2Vec2(config)
        self.lm_head = nn.Linear(config.hidden_size, config.vocab_size)
        self.blank_projection = nn.Linear(config.hidden_size, 1)
        self._engine: Optional[EBranchformerEngine] = None
        self._engine_key = None
        from .autograd_bridge import detach_state_dict_views
        self._register_state_dict_hook(detach_state_dict_views)      # adopted parameters (views of the trainer's flat store) leave state_dict() / save_pretrained() as private copies
        self.post_init()

    def _init_weights(self, module):
        std = getattr(self.config, "initializer_range", 0.02)
        if isinstance(module, (nn.Linear, nn.Conv1d, nn.Conv2d)):
            nn.init.normal_(module.weight, mean=0.0, std=std) if isinstance(module, nn.Linear) else nn.init.kaiming_normal_(module.weight)
            if module.bias is not None:
                nn.init.zeros_(module.bias)
        elif isinstance(module, nn.LayerNorm):
            nn.init.ones_(module.weight); nn.init.zeros_(module.bias)

    # ---- surface used by the reference's trainers / collators
    def freeze_encoder(self):
        for p in self.wav2vec2.encoder.parameters():
            p.requires_grad = False

    def freeze_feature_encoder(self):
        for p in self.wav2vec2.feature_extractor.parameters():
            p.requires_grad = False

    def get_output_embeddings(self):
        return None

    def _get_feat_extract_output_lengths(self, input_lengths, add_adapter=None):
        """Wav2Vec2ForCTC's UN-padded formula (quirk of SURVEY.md §8a row 8'): floor((L - k)/s) + 1 per conv."""
        for k, s in zip(self.config.conv_kernel, self.config.conv_stride):
            input_lengths = torch.div(input_lengths - k, s, rounding_mode="floor") + 1 if torch.is_tensor(input_lengths) \
                else (input_lengths - k) // s + 1
        return input_lengths

    def _get_feature_vector_attention_mask(self, feature_vector_length: int, attention_mask: torch.LongTensor, add_adapter=None):
        lens = self._get_feat_extract_output_lengths(attention_mask.sum(-1)).to(torch.long)
        return torch.arange(feature_vector_length, device=attention_mask.device)[None, :] < lens[:, None]

    # ---- engine plumbing
    def _param_list(self):
        """cached flat list of the parameters (walking the module tree per forward costs more than the check it feeds); parameters are never
        added or removed after construction"""
        pl = self.__dict__.get("_plist")
        if pl is None:
            pl = list(self.parameters())
            self.__dict__["_plist"] = pl
        return pl

    def _weights_version(self):
        return sum(p._version for p in self._param_list())

    def _precision(self) -> str:
        """numeric mode of the HIP inference engine: `config.hip_precision`, else the environment variable HFASR_PRECISION, else "bf16" ("fp32": engine.py)"""
        return getattr(self.config, "hip_precision", None) or os.environ.get("HFASR_PRECISION") or "bf16"

    def _get_engine(self, device) -> EBranchformerEngine:
        prec = self._precision()
        if self._engine is None or self._engine.device != torch.device(device) or self._engine.precision != prec:
            self._engine = EBranchformerEngine(cfg_from_hf(self.config), device, precision=prec)
            self._engine_key = None
        pl = self._param_list()
        from .autograd_bridge import bridge_generation
        key = (self._weights_version(), bridge_generation(self), pl[0].data_ptr(), pl[-1].data_ptr(), pl[len(pl) // 2].data_ptr())
        if key != self._engine_key:
            self._engine.load_state_dict({k: v for k, v in self.state_dict().items()})
            self._engine_key = key
        return self._engine

    def _get_trainer(self, device):
        from .train import EncoderCTCTrainer
        if getattr(self, "_trainer", None) is None or self._trainer.device != torch.device(device):
            self._trainer = EncoderCTCTrainer(cfg_from_hf(self.config), device, dp_sync=False, seed=_dropout_seed())      # optimizer / all-reduce stay with the caller (HF Trainer)
        return self._trainer

    def _training_forward(self, input_values, attention_mask, labels, output_hidden_states, return_dict):
        """training step through the HIP trainer; gradients reach the nn.Parameters via autograd_bridge.HipStep."""
        from .autograd_bridge import run_training_forward
        if labels is None:
            raise NotImplementedError("HIP training forward needs `labels` (the CTC loss is the only differentiable output of this head)")
        chk = getattr(self, "_label_check", None)
        if chk is None:
            from .autograd_bridge import LabelRangeCheck
            chk = LabelRangeCheck(self.config.vocab_size, "vocab_size")
            object.__setattr__(self, "_label_check", chk)
        chk.submit(labels)                                 # the reference's range check (e_branchformer.py:461-462) without its per-step host sync
        labels = labels.clamp(max=self.config.vocab_size - 1)   # a bad batch is reported one forward later: until then its labels must stay inside the logits row
        tr = self._get_trainer(input_values.device)
        feat_len = attention_mask.sum(-1).to(torch.int32) if attention_mask is not None else None

        def step(t):
            t.store.zero_grad()
            return t.forward_backward(input_values, feat_len, labels.to(input_values.device), keep_hidden=bool(output_hidden_states))
        loss, out = run_training_forward(self, tr, step)
        hidden_states = (out["last_hidden"],) if output_hidden_states else None
        if not return_dict:
            return (loss, out["logits"]) + ((hidden_states,) if hidden_states is not None else ())
        return CausalLMOutput(loss=loss, logits=out["logits"], hidden_states=hidden_states, attentions=None)

    def bias_context(self, phrases, weight: float, tokenizer=None):
        """A phrase list for contextual biasing of the CTC prefix beam search (ctc_bias.CtcBias; DESIGN.md §4 'Contextual biasing') over this model's classes, blank =
        config.vocab_size: `phrases` are lists of token ids, taken as they are, or strings, which go through `tokenizer(text, add_special_tokens=False).input_ids`;
        `weight` is in log-probability units per credited token.  Pure host work; pass the result as bias= to transcribe / stream / audio_stream (with beams=) or to
        stream_pool(...).with_beams(W, bias=) / audio_pool(...).with_beams(W, bias=)."""
        from .ctc_bias import CtcBias
        ids = []
        for ph in phrases:
            if isinstance(ph, str):
                if tokenizer is None:
                    raise ValueError("bias_context: a phrase given as text needs tokenizer=")
                ph = tokenizer(ph, add_special_tokens=False).input_ids
            ids.append(list(ph))
        return CtcBias(ids, weight, self.config.vocab_size + 1, self.config.vocab_size)

    def transcribe(self, input_values: torch.Tensor, attention_mask: Optional[torch.Tensor] = None, span: str = "valid", *, beams=None, token_topk=None, nbest=1, bias=None):
        """CTC greedy transcription on the device (eval mode only): -> (tokens (B, T') int64 = each utterance's token ids then config.pad_token_id, n_tokens (B) int32).
        span "valid" cuts every utterance at its un-padded output length (the lengths the CTC loss is trained with); "all" counts every frame, which is what the
        reference's ctc_greedy_decode does with this model's logits.  Runs engine.transcribe: with `model._get_engine(device).head_argmax` on (the default), the head's argmax comes out of its GEMM and no logits tensor is produced; otherwise the head
        GEMM fills an fp32 scratch and one argmax pass reads it (the same ids).
        beams=W (with token_topk, nbest, and bias = a `bias_context`): the CTC prefix beam search instead, -> engine.transcribe's dict (tokens, n_tokens, nbest_tokens,
        nbest_n, scores[, credit, nbest_credit], inner_len, outer_len); token_topk, nbest and bias without beams are refused (ValueError)."""
        if span not in ("valid", "all"):
            raise ValueError(f"transcribe: span must be 'valid' or 'all', got {span!r}")
        if beams is None and (token_topk is not None or nbest != 1 or bias is not None):
            raise ValueError("transcribe: token_topk, nbest and bias belong to beams=")
        if self.training:
            raise RuntimeError("transcribe() is an inference call: put the model in eval mode first (model.eval())")
        if not input_values.is_cuda:
            raise RuntimeError("Wav2Vec2EBranchformerForCTC (HIP): inputs must be on the GPU; there is no CPU fallback")
        pad = self.config.pad_token_id
        if pad is None:
            raise ValueError("transcribe: config.pad_token_id is not set")
        eng = self._get_engine(input_values.device)
        feat_len = attention_mask.sum(-1).to(torch.int32) if attention_mask is not None else None
        if beams is not None:
            return eng.transcribe(input_values, feat_len, span=span, pad_id=int(pad), beams=beams, token_topk=token_topk, nbest=nbest, bias=bias)
        out = eng.transcribe(input_values, feat_len, span=span, pad_id=int(pad))
        return out["tokens"], out["n_tokens"]

    def align(self, input_values: torch.Tensor, attention_mask: Optional[torch.Tensor] = None, labels: Optional[torch.Tensor] = None, span: str = "valid"):
        """CTC forced alignment on the device (eval mode only): the best frame-level alignment of each transcript in `labels` (B, U) int64, padded with any negative
        value as the collator pads them (-100), to its utterance.  -> CTCAlignment(path (B, T') int32 = the class of every frame on the best path (blank =
        config.vocab_size), -1 past the utterance; score (B) fp32 = the path's log-probability; start, end (B, U) int32 = token u occupies frames [start, end), -1 past
        the transcript; token_lp (B, U) fp32 = the token's summed log-probability over its frames; n_tokens (B) int32).  A transcript that does not fit its utterance
        (more tokens, counting one extra frame between equal neighbours, than frames) gets score -inf and -1 everywhere.  span as in transcribe().
        Frames are encoder output frames: one frame is prod(config.conv_stride) feature frames (4 with the two stride-2 convs of the shipped configs); converting to
        seconds needs the feature extractor's hop, which the model does not know."""
        if span not in ("valid", "all"):
            raise ValueError(f"align: span must be 'valid' or 'all', got {span!r}")
        if self.training:
            raise RuntimeError("align() is an inference call: put the model in eval mode first (model.eval())")
        if not input_values.is_cuda:
            raise RuntimeError("Wav2Vec2EBranchformerForCTC (HIP): inputs must be on the GPU; there is no CPU fallback")
        if labels is None or labels.dtype != torch.int64 or labels.dim() != 2 or labels.shape[0] != input_values.shape[0]:
            raise ValueError(f"align: labels must be ({input_values.shape[0]}, U) int64 (negative entries are padding)")
        eng = self._get_engine(input_values.device)
        feat_len = attention_mask.sum(-1).to(torch.int32) if attention_mask is not None else None
        out = eng.align(input_values, feat_len, labels.to(input_values.device), span=span)
        return CTCAlignment(path=out["path"], score=out["score"], start=out["start"], end=out["end"], token_lp=out["token_lp"], n_tokens=out["tgt_len"])

    def stream(self, batch: int, chunk_frames: int, max_frames: int, device=None, *, beams=None, token_topk=None, nbest=1, bias=None):
        """Streaming inference of a causal model (config.is_causal; eval mode only): -> streaming.EncoderStream over this model's weights — `feed` whole chunks of
        4 * chunk_frames feature frames for `batch` streams in lock-step, `finish` the rest; the concatenated logits are forward()'s of each utterance alone, the ids its
        greedy transcription.  A frame becomes final num_hidden_layers * (merge_conv_kernel - 1) / 2 frames late (DESIGN.md §4 'Streaming').  beams / token_topk /
        nbest / bias: the prefix beam search on the stream and its contextual biasing (a `bias_context`), as EBranchformerEngine.stream takes them."""
        if self.training:
            raise RuntimeError("stream() is an inference call: put the model in eval mode first (model.eval())")
        dev = device if device is not None else next(self.parameters()).device
        if torch.device(dev).type != "cuda":
            raise RuntimeError("Wav2Vec2EBranchformerForCTC (HIP): the model must be on the GPU; there is no CPU fallback")
        return self._get_engine(dev).stream(batch, chunk_frames, max_frames, beams=beams, token_topk=token_topk, nbest=nbest, bias=bias)

    def stream_pool(self, slots: int, chunk_frames: int, max_frames: int, device=None, *, beams=None):
        """Streaming inference for sessions that start, idle and end on their own (eval mode only): -> streaming.StreamPool over this model's weights, as
        EBranchformerEngine.stream_pool describes it (DESIGN.md §4 'Session pool'); `.with_beams(W, token_topk=None, nbest=1, bias=None)` on it adds the CTC prefix beam search per
        slot ('Beam search on the pool'), with bias = a `bias_context` its contextual biasing, one context for the pool."""
        if self.training:
            raise RuntimeError("stream_pool() is an inference call: put the model in eval mode first (model.eval())")
        dev = device if device is not None else next(self.parameters()).device
        if torch.device(dev).type != "cuda":
            raise RuntimeError("Wav2Vec2EBranchformerForCTC (HIP): the model must be on the GPU; there is no CPU fallback")
        return self._get_engine(dev).stream_pool(slots, chunk_frames, max_frames, beams=beams)

    def _audio_engine(self, feature_extractor, device, what):
        from .streaming import extractor_settings
        if self.training:
            raise RuntimeError(f"{what} is an inference call: put the model in eval mode first (model.eval())")
        settings = extractor_settings(feature_extractor, self.config.num_fbanks)        # the refusals that need no device
        dev = device if device is not None else next(self.parameters()).device
        if torch.device(dev).type != "cuda":
            raise RuntimeError("Wav2Vec2EBranchformerForCTC (HIP): the model must be on the GPU; there is no CPU fallback")
        return self._get_engine(dev), settings

    def audio_stream(self, feature_extractor, batch: int, chunk_frames: int, max_frames: int, device=None, *, beams=None, token_topk=None, nbest=1, max_push_samples=None,
                     bias=None):
        """`stream` fed audio (eval mode only): -> streaming.AudioStream.  feature_size, norm_type and the global statistics are read from the project's
        `CustomFeatureExtractor`; an extractor with utterance CMVN is refused (NotImplementedError: it needs the whole utterance), one whose feature_size is not
        config.num_fbanks too (ValueError).  The streamed features are those of `feature_extractor.extract_on_device(wave, default_transform=False)`.  bias as `stream`."""
        eng, settings = self._audio_engine(feature_extractor, device, "audio_stream()")
        return eng.audio_stream(batch, chunk_frames, max_frames, beams=beams, token_topk=token_topk, nbest=nbest, max_push_samples=max_push_samples, bias=bias, **settings)

    def audio_pool(self, feature_extractor, slots: int, chunk_frames: int, max_frames: int, device=None, *, beams=None, max_push_samples=None):
        """`stream_pool` fed audio (eval mode only): -> streaming.AudioPool; the extractor is read as `audio_stream` reads it.  `.with_beams(W, ..., bias=)` as on `stream_pool`."""
        eng, settings = self._audio_engine(feature_extractor, device, "audio_pool()")
        return eng.audio_pool(slots, chunk_frames, max_frames, beams=beams, max_push_samples=max_push_samples, **settings)

    def forward(
        self,
        input_values: Optional[torch.Tensor],
        attention_mask: Optional[torch.Tensor] = None,
        output_attentions: Optional[bool] = None,
        output_hidden_states: Optional[bool] = None,
        return_dict: Optional[bool] = None,
        labels: Optional[torch.Tensor] = None,
        **kwargs,
    ) -> Union[Tuple, CausalLMOutput]:
        return_dict = return_dict if return_dict is not None else getattr(self.config, "return_dict", True)
        if output_attentions:
            raise NotImplementedError("attention probabilities are never materialised by the fused HIP attention kernel")
        if not input_values.is_cuda:
            raise RuntimeError("Wav2Vec2EBranchformerForCTC (HIP): inputs must be on the GPU; there is no CPU fallback")
        if self.training and torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            if self._precision() == "fp32":
                raise NotImplementedError("hip_precision='fp32' is an inference mode: the HIP trainer is bf16-only (call model.eval(), or train with the default precision)")
            return self._training_forward(input_values, attention_mask, labels, output_hidden_states, return_dict)
        eng = self._get_engine(input_values.device)
        feat_len = attention_mask.sum(-1).to(torch.int32) if attention_mask is not None else None
        out = eng.forward(input_values, feat_len, want_hidden=True, want_all_hidden=bool(output_hidden_states))
        logits = out["logits"]
        loss = None
        if labels is not None:
            if getattr(self, "_label_check", None) is not None:
                self._label_check.flush()                   # a bad TRAINING batch still pending: report it now
            if labels.max() >= self.config.vocab_size:      # same check / same sync point as e_branchformer.py:461-462
                raise ValueError(f"Label values must be <= vocab_size: {self.config.vocab_size}")
            loss, _, _ = ops.ctc_loss(logits, labels.to(logits.device), out["outer_len"],
                                      reduction=self.config.ctc_loss_reduction, zero_infinity=self.config.ctc_zero_infinity, lse=out.get("lse"))
        hidden_states = out["hidden_states"] if output_hidden_states else None          # L + 1 tensors, as HF (tf:685-713)
        if not return_dict:
            output = (logits,) + ((hidden_states,) if hidden_states is not None else ())
            return ((loss,) + output) if loss is not None else output
        return CausalLMOutput(loss=loss, logits=logits, hidden_states=hidden_states, attentions=None)
