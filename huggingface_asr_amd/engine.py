"""Host driver of the HIP encoder: packs weights into the slot table of `mi_ebf_forward`, owns the
workspace / position tables, and launches the whole-encoder C call on the current stream.

The packed layouts themselves (and the reference state-dict names they come from) are defined once, in
packing.py, for this engine and the trainers alike; `load_state_dict` casts them into the slot table and
adds what only the forward kernels want: the V row views, the gated conv2's block interleave, ln_fold.
"""
from __future__ import annotations

import ctypes as C
import os

import torch

from . import _lib, ops
from .packing import _enc_map, encoder_specs, mapped_fp32, packed, relative_position_table, rotary_tables
from .shapes import GATE_SHARE, context_mode

G = dict(CONV1_W=0, CONV1_B=1, CONV2_W=2, CONV2_B=3, FEOUT_W=4, FEOUT_B=5, FP_LN_G=6, FP_LN_B=7, FP_W=8, FP_B=9,
         ENC_LN_G=10, ENC_LN_B=11, HEAD_W=12, HEAD_B=13, MIX_W=14, GATE1_W=15, GATE1_B=16, GATE2_W=17, GATE2_B=18)
LS = {n: i for i, n in enumerate(
    ["FF1_LN_G", "FF1_LN_B", "FF1_W1", "FF1_B1", "FF1_W2", "FF1_B2",
     "ATT_LN_G", "ATT_LN_B", "ATT_WQK", "ATT_BQK", "ATT_WV", "ATT_BV", "ATT_WO", "ATT_BO", "ATT_WPOS", "ATT_U", "ATT_V",
     "MLP_LN_G", "MLP_LN_B", "MLP_W1", "MLP_B1", "CSGU_LN_G", "CSGU_LN_B", "CSGU_W", "CSGU_B", "MLP_W2", "MLP_B2",
     "MRG_DW_W", "MRG_DW_B", "MRG_W", "MRG_B", "FIN_LN_G", "FIN_LN_B",
     "FF2_LN_G", "FF2_LN_B", "FF2_W1", "FF2_B1", "FF2_W2", "FF2_B2", "CSGU_LIN_W", "CSGU_LIN_B",
     # ln_fold (csrc/gemm_args.hpp): W' = bf16(W diag(gamma)), colsum(W') fp32, W beta + b fp32 of the four LayerNorm -> Linear pairs
     "FF1_WF", "FF1_SF", "FF1_CF", "QKV_WF", "QKV_SF", "QKV_CF", "MLP_WF", "MLP_SF", "MLP_CF", "FF2_WF", "FF2_SF", "FF2_CF"])}
SLOT_RENAME = {"att_wqkv": "ATT_WQK", "att_bqkv": "ATT_BQK"}      # every other slot is named like its packed parameter (packing.encoder_specs), upper-cased
# the bias that completes a LayerNorm -> Linear pair of ln_fold -> (slot prefix, weight, LayerNorm gamma, beta); the pair's other three precede it in the walk
FOLDS = {"ff1_b1": ("FF1", "ff1_w1", "ff1_ln_g", "ff1_ln_b"), "att_bqkv": ("QKV", "att_wqkv", "att_ln_g", "att_ln_b"),
         "mlp_b1": ("MLP", "mlp_w1", "mlp_ln_g", "mlp_ln_b"), "ff2_b1": ("FF2", "ff2_w1", "ff2_ln_g", "ff2_ln_b")}
ACT = {"identity": 0, "gelu": 1, "relu": 2, "silu": 3, "swish": 3}
POS = {None: 0, "none": 0, "relative": 1, "rotary": 2}
PRECISIONS = ("bf16", "fp32")


def cfg_from_hf(config) -> dict:
    """plain dict view of a (our or the reference's) Wav2Vec2EBranchformerConfig."""
    g = lambda k, d=None: getattr(config, k, d)
    return dict(hidden_size=g("hidden_size"), num_hidden_layers=g("num_hidden_layers"), num_attention_heads=g("num_attention_heads"),
                intermediate_size=g("intermediate_size"), conv_dim=list(g("conv_dim")), conv_kernel=list(g("conv_kernel")),
                conv_stride=list(g("conv_stride")), conv_padding=list(g("conv_padding", [1] * len(g("conv_kernel")))),
                vocab_size=g("vocab_size"), num_fbanks=g("num_fbanks", 80), context_awareness_type=g("context_awareness_type", None),
                position_embeddings_type=g("position_embeddings_type", "relative"), rotary_embedding_base=g("rotary_embedding_base", 10000),
                csgu_kernel_size=g("csgu_kernel_size", 31), merge_conv_kernel=g("merge_conv_kernel", 31),
                csgu_activation=g("csgu_activation", "identity"), csgu_use_linear_after_conv=g("csgu_use_linear_after_conv", False),
                use_macaron_ff=g("use_macaron_ff", True), is_causal=g("is_causal", False), layer_norm_eps=g("layer_norm_eps", 1e-5),
                hidden_act=g("hidden_act", "gelu"), feat_extract_activation=g("feat_extract_activation", "gelu"),
                mask_time_prob=g("mask_time_prob", 0.05), mask_feature_prob=g("mask_feature_prob", 0.0),
                ctc_loss_reduction=g("ctc_loss_reduction", "sum"), ctc_zero_infinity=g("ctc_zero_infinity", False),
                # training-mode randomness (dropout sites, in-model SpecAugment, LayerDrop: train.py)
                hidden_dropout=g("hidden_dropout", 0.0), activation_dropout=g("activation_dropout", 0.0), attention_dropout=g("attention_dropout", 0.0),
                final_dropout=g("final_dropout", 0.0), feat_proj_dropout=g("feat_proj_dropout", 0.0), layerdrop=g("layerdrop", 0.0),
                csgu_conv_dropout=g("csgu_conv_dropout", 0.0), apply_spec_augment=g("apply_spec_augment", False),
                mask_time_length=g("mask_time_length", 10), mask_time_min_masks=g("mask_time_min_masks", 2),
                mask_feature_length=g("mask_feature_length", 10), mask_feature_min_masks=g("mask_feature_min_masks", 0),
                # CTC fine-tuning head of a BEST-RQ encoder (bestrq.py:155-205)
                finetune_with_additional_layer=bool(g("finetune_with_additional_layer", False)),
                finetune_with_layer_mixing=bool(g("finetune_with_layer_mixing", False)))


class EBranchformerEngine:
    """Forward engine for Wav2Vec2EBranchformerForCTC (eval-mode semantics of e_branchformer.py:422-496).

    precision "bf16" (default): bf16 operands and activations between kernels, fp32 accumulation — the reference's `--bf16` recipes.
    precision "fp32": no value is rounded to bf16 anywhere between the features and the logits (mi_ebf_forward_f32: fp32 weights, f32-input MFMA GEMMs, fp32 attention
    scores; DESIGN.md §4 'fp32 inference mode') — what the reference's decode recipes compute.  Plain encoder + CTC head only: the gated front ends, the BEST-RQ
    fine-tuning head, want_all_hidden, ForwardPipeline lanes, HFASR_BRANCH_OVERLAP=1 and a forced ln_fold raise NotImplementedError, on the host."""

    def __init__(self, cfg: dict, device="cuda:0", logits_dtype=torch.float32, precision="bf16"):
        if precision not in PRECISIONS:
            raise ValueError(f"EBranchformerEngine: precision must be one of {PRECISIONS}, got {precision!r}")
        self.precision = precision
        self.cfg = dict(cfg)
        self.device = torch.device(device)
        self.logits_dtype = logits_dtype
        # experimental (HFASR_BRANCH_OVERLAP=1): attention and cgMLP branches of a layer on two streams, +1-2 % on the base model.
        # Off by default: two kernels of different streams sharing a CU is what DESIGN.md 'Concurrent kernels' is about.
        self.branch_overlap = os.environ.get("HFASR_BRANCH_OVERLAP", "0") == "1"
        c = self.cfg
        # CTC fine-tuning head of a BEST-RQ encoder (bestrq.py:239-274): weighted mix of all hidden states and / or one more layer before the head
        self.extra = int(bool(c.get("finetune_with_additional_layer", False)))
        self.mix = int(bool(c.get("finetune_with_layer_mixing", False)))
        if len(c["conv_dim"]) != 2 or len(set(c["conv_kernel"])) != 1 or len(set(c["conv_stride"])) != 1 or len(set(c["conv_padding"])) != 1:
            raise NotImplementedError("HIP path supports the 2-layer Conv2d sub-sampling with equal kernel/stride/padding")
        if c.get("hidden_act", "gelu") != "gelu" or c.get("feat_extract_activation", "gelu") != "gelu":
            raise NotImplementedError("HIP path implements the erf-GELU activations of the reference configs")
        if c.get("csgu_activation", "identity") not in ACT:
            raise NotImplementedError(f"csgu_activation {c['csgu_activation']}")
        # context-aware Conv2d front end (extractors.py:57-65): 1 "gated", 2 "gated_shared", 0 for None AND any other string (the reference's dict lookup
        # falls back to nn.Conv2d, e.g. for the recipes' `shared_gated`); conv and gate filters of a gated layer 2 are packed in blocks of `gate_blk` channels
        self.ctx_mode = context_mode(c)
        self.gate_blk = (32 if c["conv_dim"][1] % 32 == 0 else c["conv_dim"][1]) if self.ctx_mode == 1 else 0
        # LayerNorm folded into the GEMMs around it (mi_ebf_config.ln_fold): None = automatic (when the shapes qualify and the batch fills the 256x256 tiles),
        # True / False force it (tests; HFASR_LN_FOLD=0/1 sets the default)
        env = os.environ.get("HFASR_LN_FOLD")
        self.ln_fold = None if env is None else env == "1"
        # throughput mode (mi_ebf_config.wide_tiles; pipeline.ForwardPipeline sets it): the N = d GEMMs on 256 x 256 tiles — for several steps in flight, not for one alone
        self.wide_tiles = False
        self.head_lse = False                     # True: fp32 logits come with their row log-sum-exp out of the head GEMM's epilogue (`out["lse"]`, mi_ebf_forward_lse). Built for VERDICT r3
                                                  # item 7 and measured to buy nothing (the epilogue costs what the separate pass does): off by default, bench.py --head-lse
        self.head_argmax = True                   # transcribe(): True = the per-frame argmax comes out of the head GEMM's epilogue and no logits are written (mi_gemm_argmax_bf16);
                                                  # False = head GEMM into an fp32 scratch + one argmax pass over it.  Same ids either way.  On: measured 4.577 against 4.602 ms per step,
                                                  # base encoder at 32 x 10 s, leg spread 0.003 ms (profiles/r06_a; DESIGN §4 'Greedy transcription')
        self.weights = {}
        self._table = None
        self._ws = {}
        self._pos = {}
        self._posp = {}
        self.weights_version = 0
        if precision == "fp32":
            self._refuse_fp32_options(logits_dtype)

    def _refuse_fp32_options(self, logits_dtype=torch.float32):
        """what precision="fp32" does not cover, named and refused on the host before the device is touched"""
        no = lambda what: NotImplementedError(f"precision='fp32' does not cover {what}: use the default precision='bf16'")
        if self.ctx_mode:
            raise no(f"the gated front ends (context_awareness_type={self.cfg.get('context_awareness_type')!r})")
        if self.extra or self.mix:
            raise no("the BEST-RQ fine-tuning head (finetune_with_additional_layer / finetune_with_layer_mixing)")
        if self.branch_overlap:
            raise no("HFASR_BRANCH_OVERLAP=1")
        if self.ln_fold:
            raise no("a forced ln_fold (HFASR_LN_FOLD=1 / engine.ln_fold = True)")
        if self.wide_tiles:
            raise no("wide_tiles (ForwardPipeline's throughput mode)")
        if logits_dtype != torch.float32:
            raise ValueError("precision='fp32' produces fp32 logits: logits_dtype must be torch.float32")

    # ------------------------------------------------------------------ weights
    def load_state_dict(self, sd: dict):
        """sd: reference-named tensors (any device/dtype); packs them on `self.device`: every packed parameter of packing.encoder_specs into the slot of its
        name (`l3.ff1_ln_g` -> layer 3, FF1_LN_G), matrices in bf16, the rest in fp32, plus the three things only the forward kernels want (below).
        precision="fp32": the same slots, every one of them fp32 (matrices included), no fold tensors."""
        c, dev = self.cfg, self.device
        d, C2 = c["hidden_size"], c["conv_dim"][1]
        m = _enc_map(c)
        slots = [None] * (_lib.GLOBAL_SLOTS + (c["num_hidden_layers"] + self.extra) * _lib.LAYER_SLOTS)
        f32 = self.precision == "fp32"
        fold = self._fold_shapes_ok() and not f32
        layer = {}                                   # fp32 packed tensors of the layer being walked, by short name (ln_fold reads them)
        for s, t in packed(encoder_specs(c), m, mapped_fp32(m, sd, dev)):
            if s.name == "masked_spec_embed":        # SpecAugment's fill vector: training only
                continue
            l, _, n = s.name.rpartition(".")         # ("l3", ".", "ff1_ln_g") or ("", "", "feout_w")
            base, names = (_lib.GLOBAL_SLOTS + int(l[1:]) * _lib.LAYER_SLOTS, LS) if l else (0, G)
            if self.ctx_mode == 1 and n in ("conv2_w", "conv2_b"):
                # packed: conv rows then gate rows; the one implicit GEMM's epilogue wants [conv blk ; gate blk] per 2*blk rows (gemm_8p.hip GATED / mi_gated_act_bf16)
                t = t.reshape(2, C2 // self.gate_blk, self.gate_blk, -1).transpose(0, 1).reshape(s.shape)
            w = t.to(torch.bfloat16).contiguous() if (s.mat and not f32) else t.contiguous()
            slots[base + names[SLOT_RENAME.get(n, n.upper())]] = w
            if n in ("att_wqkv", "att_bqkv"):        # the V-only GEMM reads row views of the packed [Wq; Wk; Wv]
                slots[base + LS["ATT_WV" if s.mat else "ATT_BV"]] = w[2 * d:]
            if fold:
                layer[n] = t
                if n in FOLDS:                       # LN(x) W^T + b = rstd (x W'^T) - rstd mu colsum(W') + (W beta + b)
                    tag, wn, gn, bn = FOLDS[n]
                    wf = (layer[wn] * layer[gn][None, :]).to(torch.bfloat16).contiguous()
                    slots[base + LS[tag + "_WF"]] = wf
                    slots[base + LS[tag + "_SF"]] = wf.float().sum(-1).contiguous()
                    slots[base + LS[tag + "_CF"]] = ((layer[wn] * layer[bn][None, :]).sum(-1) + t).contiguous()      # (element-wise + row sum: no vendor BLAS call even at load time)
        self._keep = [t for t in slots if t is not None]
        self._slots = slots
        self._table = (C.c_void_p * len(slots))(*[(t.data_ptr() if t is not None else None) for t in slots])
        self._posp_valid = {}
        self.weights_version += 1

    def share_weights_from(self, other: "EBranchformerEngine") -> None:
        """Adopt `other`'s packed weight table (the same device tensors: bf16 weights, fold tensors, biases) instead of packing a state dict again — the lane engines of a
        `ForwardPipeline` differ in workspace and position cache only (four lanes held four copies of the weights and ran the load-time packing four times)."""
        if self.precision == "fp32" or other.precision == "fp32":
            raise NotImplementedError("precision='fp32' does not cover ForwardPipeline lanes (share_weights_from): use the default precision='bf16'")
        if other._table is None or other.device != self.device:
            raise ValueError("share_weights_from: the source engine must have its weights loaded on the same device")
        self._keep, self._slots, self._table = other._keep, other._slots, other._table
        self.weights = other.weights
        self._posp_valid = {}
        self.weights_version += 1

    def _fold_shapes_ok(self) -> bool:
        """shapes the folded-LayerNorm GEMM kernels take (csrc/gemm_8p.hip: 256-wide consumer tiles, 128-wide producers with <= 16 statistics pairs per row) and the
        layer forms the folded driver covers (csrc/encoder.hip)"""
        c = self.cfg
        d, I, H = c["hidden_size"], c["intermediate_size"], c["num_attention_heads"]
        return (d in (256, 512) and I % 256 == 0 and I >= 320 and (d // H) in (64, 128) and c.get("use_macaron_ff", True) and not self.extra and not self.mix
                and c.get("position_embeddings_type", "relative") != "rotary" and not c.get("csgu_use_linear_after_conv", False))

    def _use_fold(self, B: int, T2: int) -> bool:
        if self.precision == "fp32":
            self._refuse_fp32_options()                   # ln_fold / wide_tiles / branch_overlap set after construction
            return False
        if not self._fold_shapes_ok() or self.ln_fold is False or self.branch_overlap:
            return False
        return True if self.ln_fold else B * T2 >= 2048          # below that the 256x256 tiles cannot fill the chip: the small-problem kernels + LayerNorm kernels are faster

    # ------------------------------------------------------------------ tables / workspace
    def out_frames(self, T: int) -> int:
        c = self.cfg
        k, s, p = c["conv_kernel"][0], c["conv_stride"][0], c["conv_padding"][0]
        for _ in range(2):
            T = (T + 2 * p - k) // s + 1
        return T

    def _check_shared_gate(self, T: int):
        """GatedConv2dShared.forward (extractors.py:49-54) views the conv output as (B, C, -1, 4, F) and multiplies by gate.unsqueeze(3): both conv layers' time axes must
        be divisible by 4 and a quarter of them must equal the gate conv's output length — the reference raises a RuntimeError from `view` / broadcasting otherwise."""
        c = self.cfg
        k, s, p = c["conv_kernel"][0], c["conv_stride"][0], c["conv_padding"][0]
        for _ in range(2):
            To = (T + 2 * p - k) // s + 1
            Tg = (T + 2 * p * GATE_SHARE - k * GATE_SHARE) // (s * GATE_SHARE) + 1
            if To % GATE_SHARE or To // GATE_SHARE != Tg:
                raise RuntimeError(f"gated_shared front end: a conv layer maps {T} frames to {To} and its gate to {Tg}; the reference's view(B, C, -1, {GATE_SHARE}, F) * gate "
                                   f"needs {To} divisible by {GATE_SHARE} and {To} // {GATE_SHARE} == {Tg} (extractors.py:49-54) — pad the batch to a multiple of 16 frames")
            T = To

    def _pos_table(self, T2: int):
        c = self.cfg
        ptype = c.get("position_embeddings_type", "relative")
        key = (ptype, T2)
        if key in self._pos:
            return self._pos[key]
        d, H = c["hidden_size"], c["num_attention_heads"]
        if ptype == "relative":              # the sinusoid table in the precision of the GEMM that projects it
            t = relative_position_table(T2, d).to(self.device).to(torch.float32 if self.precision == "fp32" else torch.bfloat16).contiguous()
        elif ptype == "rotary":   # one buffer: [cos.flat ; sin.flat]
            cos, sin = rotary_tables(T2, d // H, c.get("rotary_embedding_base", 10000))
            t = torch.cat([cos.reshape(-1), sin.reshape(-1)]).to(self.device).contiguous()
        else:
            t = None
        self._pos[key] = t
        return t

    def _config_struct(self, B, T, F, slot=0):
        c = self.cfg
        fold = int(self._use_fold(B, self.out_frames(T)))
        return _lib.EbfConfig(ln_fold=fold, wide_tiles=int(bool(self.wide_tiles) and bool(fold)), B=B, T=T, F=F, d=c["hidden_size"], H=c["num_attention_heads"], I=c["intermediate_size"],
                              L=c["num_hidden_layers"], V=c["vocab_size"], C1=c["conv_dim"][0], C2=c["conv_dim"][1],
                              K=c["conv_kernel"][0], stride=c["conv_stride"][0], pad=c["conv_padding"][0],
                              is_causal=int(c.get("is_causal", False)), pos_type=POS[c.get("position_embeddings_type", "relative")],
                              csgu_kernel=c.get("csgu_kernel_size", 31), merge_kernel=c.get("merge_conv_kernel", 31),
                              csgu_act=ACT[c.get("csgu_activation", "identity")], use_macaron=int(c.get("use_macaron_ff", True)),
                              ln_eps=float(c.get("layer_norm_eps", 1e-5)), logits_f32=int(self.logits_dtype == torch.float32),
                              logits_ld=(c["vocab_size"] + 1 + 7) // 8 * 8,
                              branch_overlap=int(self.branch_overlap and slot == 0), extra_layers=self.extra, layer_mixing=self.mix,
                              csgu_linear=int(bool(c.get("csgu_use_linear_after_conv", False))), context_mode=self.ctx_mode, gate_blk=self.gate_blk)

    def _workspace(self, cs, slot=0):
        key = (cs.B, cs.T, cs.F, cs.ln_fold, cs.wide_tiles)
        if self._ws.get("key") != key:
            self._ws = {"key": key}                                                        # keep one shape resident
        if slot not in self._ws:
            nbytes = (_lib.lib().mi_ebf_f32_workspace_bytes if self.precision == "fp32" else _lib.lib().mi_ebf_workspace_bytes)(C.byref(cs))
            self._ws[slot] = torch.zeros(nbytes, dtype=torch.uint8, device=self.device)
        return self._ws[slot]

    def _head_fusable(self) -> bool:
        """the head shapes mi_gemm_argmax_bf16 takes (the 256 x 256 kernel: K = hidden size a multiple of 64, at least two K tiles); others run GEMM + argmax pass"""
        d = self.cfg["hidden_size"]
        return d % 64 == 0 and d >= 128

    # ------------------------------------------------------------------ forward
    def _prepare(self, feats, slot):
        """what every whole-encoder call needs: the config struct, the slot's workspace and the position tables for this batch shape"""
        if self._table is None:
            raise RuntimeError("EBranchformerEngine: load_state_dict() first")
        if not feats.is_cuda:
            raise RuntimeError("EBranchformerEngine.forward needs device tensors (no CPU fallback)")
        if self.precision == "fp32" and slot != 0:
            raise NotImplementedError("precision='fp32' does not cover ForwardPipeline lanes (slot != 0): use the default precision='bf16'")
        feats = feats.to(torch.float32).contiguous()
        B, T, F = feats.shape
        c = self.cfg
        cs = self._config_struct(B, T, F, slot)
        T2 = self.out_frames(T)
        if T2 <= 0:
            raise ValueError("input too short for the conv sub-sampling")
        if self.ctx_mode == 2:
            self._check_shared_gate(T)
        d = c["hidden_size"]
        ws = self._workspace(cs, slot)
        pos = self._pos_table(T2)
        posp, compute = None, 0
        if cs.pos_type == 1:
            if T2 not in self._posp:
                self._posp = {T2: torch.empty((c["num_hidden_layers"] + self.extra, 2 * T2 - 1, d), dtype=torch.float32 if self.precision == "fp32" else torch.bfloat16,
                                              device=self.device)}
                self._posp_valid = {}
            posp = self._posp[T2]
            compute = 0 if self._posp_valid.get(T2) == self.weights_version else 1
            if compute and slot != 0:
                raise RuntimeError("multi-stream use: run one forward on slot 0 first (it fills the shared position-projection cache)")
            self._posp_valid[T2] = self.weights_version
        return feats, cs, T2, ws, pos, posp, compute

    def transcribe(self, feats: torch.Tensor, feat_lengths: torch.Tensor | None = None, *, span="valid", pad_id=0, slot=0, want_hidden=False, return_frames=False,
                   dtype=torch.int64, beams=None, token_topk=None, nbest=1, bias=None):
        """CTC transcription on the device, greedy or (with `beams`) by prefix beam search.
        beams=None: feats (B,T,F) -> dict(tokens (B,T2) `dtype` = the token ids then pad_id, n_tokens (B) int32, best (B,T2) int32 = the
        per-frame classes, inner_len, outer_len[, frames (B,T2) int32 = the frame each token starts at, then -1][, last_hidden]).  Blank = the last class.
        span "valid": frames beyond outer_len (the lengths the CTC loss is trained with) are cut; "all": every frame counts, as in the reference's ctc_greedy_decode.
        With `head_argmax` on (the default; and a head that fits the fused kernel) no logits tensor is allocated; `slot` as in forward().
        beams=W (1..64): the forward with fp32-or-`logits_dtype` logits, then ops.ctc_beam_decode over them with the same lengths (W hypotheses, the `token_topk` best
        classes per frame, None = min(W, V)): tokens / n_tokens[/ frames] are the best hypothesis' (tokens (B,T2)), and the dict gains nbest_tokens (B,nbest,T2),
        nbest_n (B,nbest), scores (B,nbest) fp32[, nbest_frames (B,nbest,T2)]; no `best`.
        precision="fp32": the fp32 head GEMM writes its logits into a scratch, mi_row_argmax reads it and mi_ctc_collapse follows; `head_argmax` / `head_lse` are
        ignored in this mode (there is no fused fp32 head).  beams=W runs ops.ctc_beam_decode over the fp32 logits as above.
        bias (a ctc_bias.CtcBias for this model's V + 1 classes, blank V; needs beams): contextual biasing of that search (csrc/ctc_beam_bias.hip): the dict gains
        credit (B) int32, the best hypothesis' credited tokens, and nbest_credit (B,nbest)."""
        if span not in ("valid", "all"):
            raise ValueError(f"transcribe: span must be 'valid' or 'all', got {span!r}")
        self._check_bias("transcribe", bias, beams)
        if beams is not None:
            fwd = self.forward(feats, feat_lengths, want_hidden=want_hidden, want_logits=True, slot=slot)
            bo = ops.ctc_beam_decode(fwd["logits"], self.cfg["vocab_size"], pad_id, fwd["outer_len"] if span == "valid" else None, beams=beams, token_topk=token_topk,
                                     nbest=nbest, return_frames=return_frames, dtype=dtype, bias=bias)
            out = dict(tokens=bo["tokens"][:, 0], n_tokens=bo["n_tokens"][:, 0], nbest_tokens=bo["tokens"], nbest_n=bo["n_tokens"], scores=bo["scores"],
                       inner_len=fwd["inner_len"], outer_len=fwd["outer_len"])
            if bias is not None:
                out.update(credit=bo["credit"][:, 0], nbest_credit=bo["credit"])
            if return_frames:
                out.update(frames=bo["frames"][:, 0], nbest_frames=bo["frames"])
            if want_hidden:
                out["last_hidden"] = fwd["last_hidden"]
            return out
        if self.precision == "fp32":
            fwd = self.forward(feats, feat_lengths, want_hidden=want_hidden, want_logits=True, slot=slot)
            best = ops.row_argmax(fwd["logits"].flatten(0, 1)).view(fwd["logits"].shape[:2])
            out = ops.ctc_collapse(best, self.cfg["vocab_size"], pad_id, fwd["outer_len"] if span == "valid" else None, return_frames=return_frames, dtype=dtype)
            out.update(best=best, inner_len=fwd["inner_len"], outer_len=fwd["outer_len"])
            if want_hidden:
                out["last_hidden"] = fwd["last_hidden"]
            return out
        feats, cs, T2, ws, pos, posp, compute = self._prepare(feats, slot)
        B, c = feats.shape[0], self.cfg
        d, V1, L = c["hidden_size"], c["vocab_size"] + 1, _lib.lib()
        hidden = torch.empty((B, T2, d), dtype=torch.float32, device=self.device) if want_hidden else None
        lens = torch.empty((2, B), dtype=torch.int32, device=self.device)
        best = torch.empty((B, T2), dtype=torch.int32, device=self.device)
        if feat_lengths is not None:
            feat_lengths = feat_lengths.to(device=self.device, dtype=torch.int32).contiguous()
        p = lambda t: None if t is None else t.data_ptr()
        cs.logits_f32 = 1                               # the head's scratch, when one is needed, is fp32 whatever `logits_dtype` says: both head forms then take the argmax of the same fp32 values
        fused = bool(self.head_argmax) and self._head_fusable()
        aws = torch.empty((int(L.mi_gemm_argmax_workspace_floats(B * T2, V1)),), dtype=torch.float32, device=self.device) if fused else None
        scratch = None if fused else torch.empty((B * T2, cs.logits_ld), dtype=torch.float32, device=self.device)
        call = lambda: L.mi_ebf_forward_greedy(C.byref(cs), self._table, feats.data_ptr(), p(feat_lengths), p(pos), p(posp), compute, ws.data_ptr(), ws.numel(), p(hidden),
                                               best.data_ptr(), p(aws), p(scratch), lens[0].data_ptr(), lens[1].data_ptr(), torch.cuda.current_stream().cuda_stream)
        rc = call()
        if rc == _lib.ERR_UNSUPPORTED and scratch is None:      # the fused entry refused for a reason _head_fusable does not restate: lend the scratch and run again, never raise
            scratch = torch.empty((B * T2, cs.logits_ld), dtype=torch.float32, device=self.device)
            rc = call()
        _lib.check(rc, "mi_ebf_forward_greedy")
        out = ops.ctc_collapse(best, V1 - 1, pad_id, lens[1] if span == "valid" else None, return_frames=return_frames, dtype=dtype)
        out.update(best=best, inner_len=lens[0], outer_len=lens[1])
        if want_hidden:
            out["last_hidden"] = hidden
        return out

    def _check_bias(self, what, bias, beams):
        """bias= on the host, before any launch: it needs beams, is a ctc_bias.CtcBias, and was built for this model's classes and blank"""
        if bias is None:
            return
        from .ctc_bias import CtcBias
        if not isinstance(bias, CtcBias):
            raise TypeError(f"{what}: bias is a ctc_bias.CtcBias (model.bias_context builds one), got {type(bias).__name__}")
        if beams is None:
            raise ValueError(f"{what}: bias= biases the prefix beam search: it needs beams=")
        V = self.cfg["vocab_size"]
        if bias.vocab != V + 1 or bias.blank != V:
            raise ValueError(f"{what}: the bias context was built for vocab {bias.vocab}, blank {bias.blank}; this model has {V + 1} classes, blank {V}")

    def align(self, feats: torch.Tensor, feat_lengths: torch.Tensor | None, labels: torch.Tensor, *, span="valid", slot=0):
        """CTC forced alignment of `labels` (B, U) int64 (negative entries are padding) to feats (B,T,F): the forward that yields fp32-or-`logits_dtype` logits — with
        their row log-sum-exp out of the head's epilogue where `head_lse` is on, else (and in precision="fp32") by ops.row_lse — then ops.ctc_align over them.
        -> ops.ctc_align's dict (path (B,T2) int32, score (B), tgt_len (B), start / end (B,U) int32, token_lp (B,U); frames are encoder output frames, blank = the last
        class) plus inner_len, outer_len.  span "valid": frames beyond outer_len do not count (the lengths the CTC loss is trained with); "all": every frame does.
        `slot` and the lanes of a ForwardPipeline as in forward()."""
        if span not in ("valid", "all"):
            raise ValueError(f"align: span must be 'valid' or 'all', got {span!r}")
        if not isinstance(labels, torch.Tensor) or labels.dtype != torch.int64 or labels.dim() != 2 or labels.shape[0] != feats.shape[0]:
            raise ValueError(f"align: labels must be ({feats.shape[0]}, U) int64")
        fwd = self.forward(feats, feat_lengths, want_hidden=False, want_logits=True, slot=slot)
        out = ops.ctc_align(fwd["logits"], labels.to(self.device), fwd["outer_len"] if span == "valid" else None, blank=self.cfg["vocab_size"], lse=fwd["lse"])
        out.update(inner_len=fwd["inner_len"], outer_len=fwd["outer_len"])
        return out

    def stream(self, batch: int, chunk_frames: int, max_frames: int, *, beams=None, token_topk=None, nbest=1, bias=None):
        """Streaming inference of a causal model (bf16): -> streaming.EncoderStream for `batch` streams advanced in lock-step, `chunk_frames` encoder frames (4x as many
        feature frames) per `feed`, K/V caches of `max_frames` encoder frames.  Fed an utterance piece by piece it returns forward()'s logits of that utterance alone, each
        frame num_hidden_layers * (merge_conv_kernel - 1) / 2 frames late (csrc/stream.hip; DESIGN.md §4 'Streaming').  Refused before any launch: a non-causal config
        (ValueError); precision="fp32", layer mixing, an additional layer (NotImplementedError).
        beams=W (1..64): the stream also walks the prefix beam search of transcribe(beams=) over the frames it emits (ops.CtcBeamStream, csrc/ctc_beam_stream.hip): `feed`
        and `finish` gain a "beam" entry — the committed tokens after every step, the `nbest` hypotheses at `finish` (and per step with feed(..., partial=True)) —, bit
        for bit what ops.ctc_beam_decode gives on the concatenated logits.  Without beams nothing is allocated and no launch is added.
        bias (a ctc_bias.CtcBias; needs beams): contextual biasing of that search, as transcribe(beams=, bias=); the "beam" dicts gain credit beside the n-best."""
        from .streaming import EncoderStream
        self._check_bias("stream", bias, beams)
        return EncoderStream(self, batch, chunk_frames, max_frames, beams=beams, token_topk=token_topk, nbest=nbest, bias=bias)

    def stream_pool(self, slots: int, chunk_frames: int, max_frames: int, *, beams=None):
        """Streaming inference for sessions that start, idle and end on their own: -> streaming.StreamPool of `slots` slots over one state.  `open()` gives a free slot;
        `step(feed={slot: chunk}, finish={slot: tail})` advances the named slots — one set of launches over the rows of all of them —, leaves the others untouched and
        frees the finished ones.  A session's logits and ids are bit for bit those of `stream(1, chunk_frames, max_frames)` fed the same pieces, whatever the other slots
        do (csrc/stream_pool.hip; DESIGN.md §4 'Session pool').  `.with_beams(W, token_topk=None, nbest=1)` on the pool, before the first open(), adds the prefix beam
        search of `stream(beams=W)` per slot: every step dict gains "beam" (committed tokens per step; the n-best at finish or with step(..., partial=)), bit for bit
        what `stream(1, chunk_frames, max_frames, beams=W)` gives for the same pieces (csrc/ctc_beam_pool.hip; DESIGN.md §4 'Beam search on the pool').  Refusals as
        `stream`'s; the beams= keyword raises NotImplementedError and names `with_beams`."""
        from .streaming import StreamPool
        return StreamPool(self, slots, chunk_frames, max_frames, beams=beams)

    def audio_stream(self, batch: int, chunk_frames: int, max_frames: int, *, normalize=None, global_means=None, global_stds=None, beams=None, token_topk=None, nbest=1,
                     max_push_samples=None, tables=None, bias=None):
        """`stream` fed audio: -> streaming.AudioStream.  `push(samples (B, n))` takes fp32 samples in [-1, 1] or int16 PCM in pieces of any size, `finish(tail, lengths)`
        ends the streams; the stateful log-mel front end (csrc/fbank_stream.hip) gives, bit for bit, the features of fbank_gpu on the whole utterance with normalize=None
        or "global" (global_means / global_stds (F)), so the logits are those of `stream` fed these features in the pieces streaming.audio_pieces names.  Refusals as
        `stream`'s; normalize="utterance" raises NotImplementedError (utterance CMVN needs the whole utterance).  DESIGN.md §4 'Audio in'."""
        from .streaming import AudioStream
        self._check_bias("audio_stream", bias, beams)                      # bias= as on `stream`
        return AudioStream(self, batch, chunk_frames, max_frames, normalize=normalize, global_means=global_means, global_stds=global_stds, beams=beams,
                           token_topk=token_topk, nbest=nbest, max_push_samples=max_push_samples, tables=tables, bias=bias)

    def audio_pool(self, slots: int, chunk_frames: int, max_frames: int, *, normalize=None, global_means=None, global_stds=None, beams=None, max_push_samples=None,
                   tables=None):
        """`stream_pool` fed audio: -> streaming.AudioPool.  `open()` starts a session, `push(audio={sid: samples}, finish={sid: tail or None})` takes any sizes for
        any subset of the open slots and returns {sid: [the dicts of the steps the slot took]}.  `.with_beams(W, ...)` as on `stream_pool`; `push(..., partial=)` then asks
        for the n-best so far.  Refusals as `stream_pool`'s (the beams= keyword included) and `audio_stream`'s."""
        from .streaming import AudioPool
        return AudioPool(self, slots, chunk_frames, max_frames, normalize=normalize, global_means=global_means, global_stds=global_stds, beams=beams,
                         max_push_samples=max_push_samples, tables=tables)

    def forward(self, feats: torch.Tensor, feat_lengths: torch.Tensor | None = None, *, want_hidden=True, want_logits=True, slot=0, want_all_hidden=False):
        """feats (B,T,F) fp32 device tensor; feat_lengths (B) int32 (= attention_mask.sum(-1)) or None.
        Returns dict(logits (B,T2,V+1), last_hidden (B,T2,d) fp32, inner_len, outer_len int32 (B)); with want_all_hidden also
        hidden_states = the L+1 tensors HF returns for output_hidden_states (every layer's input, then the last hidden state).
        `slot` selects a private workspace: calls issued on different streams must use different slots.
        precision="fp32": the same dictionary out of mi_ebf_forward_f32 (logits fp32; `lse` None; want_all_hidden is not covered)."""
        if self.precision == "fp32" and want_all_hidden:
            raise NotImplementedError("precision='fp32' does not cover want_all_hidden (output_hidden_states): use the default precision='bf16'")
        feats, cs, T2, ws, pos, posp, compute = self._prepare(feats, slot)
        B, c = feats.shape[0], self.cfg
        d, V1 = c["hidden_size"], c["vocab_size"] + 1
        # rows padded to a multiple of 8 elements (16-B stores in the GEMM epilogue); callers get the (B,T2,V+1) view
        lbuf = torch.empty((B, T2, cs.logits_ld), dtype=self.logits_dtype, device=self.device) if want_logits else None
        logits = lbuf[..., :V1] if want_logits else None
        hidden = torch.empty((B, T2, d), dtype=torch.float32, device=self.device) if (want_hidden or want_all_hidden) else None
        hs = torch.empty((c["num_hidden_layers"] + 1, B, T2, d), dtype=torch.float32, device=self.device) if want_all_hidden else None
        lens = torch.empty((2, B), dtype=torch.int32, device=self.device)
        if feat_lengths is not None:
            feat_lengths = feat_lengths.to(device=self.device, dtype=torch.int32).contiguous()
        p = lambda t: None if t is None else t.data_ptr()
        if self.precision == "fp32":
            rc = _lib.lib().mi_ebf_forward_f32(C.byref(cs), self._table, feats.data_ptr(), p(feat_lengths), p(pos), p(posp), compute, ws.data_ptr(), ws.numel(),
                                               p(hidden), p(lbuf), lens[0].data_ptr(), lens[1].data_ptr(), torch.cuda.current_stream().cuda_stream)
            _lib.check(rc, "mi_ebf_forward_f32")
            return dict(logits=logits, last_hidden=hidden, inner_len=lens[0], outer_len=lens[1], lse=None)
        # fp32 logits come with their rows' log-sum-exp (B*T2) out of the head GEMM's epilogue: `ops.ctc_loss(..., lse=out["lse"])` then needs no pass of its own over them
        lse = lse_ws = None
        if want_logits and self.logits_dtype == torch.float32 and self.head_lse:
            lse = torch.empty((B * T2,), dtype=torch.float32, device=self.device)
            lse_ws = torch.empty((int(_lib.lib().mi_gemm_lse_workspace_floats(B * T2, V1)),), dtype=torch.float32, device=self.device)
        rc = _lib.lib().mi_ebf_forward_lse(C.byref(cs), self._table, feats.data_ptr(), p(feat_lengths), p(pos), p(posp), compute,
                                           ws.data_ptr(), ws.numel(), p(hidden), p(lbuf), lens[0].data_ptr(), lens[1].data_ptr(), p(hs), p(lse), p(lse_ws),
                                           torch.cuda.current_stream().cuda_stream)
        _lib.check(rc, "mi_ebf_forward")
        out = dict(logits=logits, last_hidden=hidden, inner_len=lens[0], outer_len=lens[1], lse=lse)
        if hs is not None:
            out["hidden_states"] = tuple(hs[i] for i in range(hs.shape[0]))
        return out
