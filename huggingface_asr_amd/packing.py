"""The packed weight layouts, once: what every parameter the kernels read looks like and how it relates to the reference's state dict.

Host-only (torch + shapes; nothing here loads the HIP library).  The trainers keep the packed tensors in a flat `train.ParamStore`, the forward
engines cast them into the slot tables of `mi_ebf_forward*` / `mi_gpt2_step`; both walk `*_specs()` and pack through `*_map()`, so a layout rule
lives in one place.  The layouts: nn.Linear weights as they are ((N, K) row-major IS K-contiguous, which is what the MFMA tiles read), [Wq; Wk; Wv]
in one matrix, lm_head + blank_projection concatenated with blank LAST (e_branchformer.py:456-457), conv2's weight re-ordered to
(Cout, (kh, kw, cin)), the columns of the front end's `out` Linear permuted from the reference's (c, f) flattening (extractors.py:112) to the
channels-last (f, c) activation layout, and transformers' Conv1D weights ((in, out)) transposed.  The position tables of the encoder, which
trainer and engine build from the same formulas, live here too.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from functools import partial
from typing import Callable, NamedTuple

import torch

from .shapes import GATE_SHARE, context_mode, conv_freq_out


@dataclass
class Spec:
    name: str
    shape: tuple
    mat: bool          # bf16 (N,K) GEMM operand -> also keeps the transposed bf16 copy
    decay: bool


class Ref(NamedTuple):
    """how one packed parameter relates to the reference's state dict: pack(sd) -> the packed tensor, pieces = [(reference key,
    unpack(packed) -> the reference tensor, a view where the layouts allow), ...]; optional: the keys may be missing from a reference
    state dict (pack then supplies the default) and are not exported when the last load lacked them"""
    pack: Callable
    pieces: list
    optional: bool = False


def _one(m, name, key, fwd=lambda t: t, bwd=lambda t: t):
    """map entry of a packed parameter that is ONE reference tensor: packed = fwd(sd[key]), reference = bwd(packed)"""
    m[name] = Ref(lambda sd: fwd(sd[key]), [(key, bwd)])


def mapped_fp32(ref_map: dict, sd: dict, device) -> dict:
    """the tensors of a reference state dict that `ref_map` reads, in fp32 on `device` (everything else in it is ignored)"""
    keys = {key for r in ref_map.values() for key, _ in r.pieces}
    return {k: v.detach().to(device, torch.float32) for k, v in sd.items() if k in keys and torch.is_tensor(v) and v.is_floating_point()}


def packed(specs, ref_map: dict, sd: dict):
    """(spec, its fp32 packed tensor in the spec's shape) for every spec, from what `mapped_fp32` returned; a key that a non-optional entry needs
    and the state dict lacks raises a KeyError naming it"""
    for s in specs:
        yield s, ref_map[s.name].pack(sd).reshape(s.shape)


# ====================================================================================================== encoder parameters
def encoder_specs(c: dict, head: bool = True) -> list[Spec]:
    d, I, L, V1 = c["hidden_size"], c["intermediate_size"], c["num_hidden_layers"], c["vocab_size"] + 1
    C1, C2 = c["conv_dim"]
    K = c["conv_kernel"][0]
    F2 = conv_freq_out(c.get("num_fbanks", 80), c["conv_kernel"], c["conv_stride"], c["conv_padding"])
    kc, km = c.get("csgu_kernel_size", 31), c.get("merge_conv_kernel", 31)
    rel = c.get("position_embeddings_type", "relative") == "relative"
    S = []
    mat = lambda n, *sh: S.append(Spec(n, tuple(sh), True, True))
    vec = lambda n, *sh, decay=False: S.append(Spec(n, tuple(sh), False, decay))
    vec("masked_spec_embed", d)     # SpecAugment fill vector: carried for state-dict parity, never receives a gradient on this path (torch skips it too)
    mode = context_mode(c)                                   # context-aware front end (extractors.py:23-65): 0 plain, 1 gated, 2 gated_shared
    gkh = K * (GATE_SHARE if mode == 2 else 1)               # the shared gate's kernel is (4K, K)
    vec("conv1_w", C1, K * K, decay=True); vec("conv1_b", C1)
    if mode:
        vec("gate1_w", C1, gkh * K, decay=True); vec("gate1_b", C1)
    if mode == 1:                                            # conv rows, then gate rows: ONE implicit GEMM forward, one dW / dX GEMM pair backward
        mat("conv2_w", 2 * C2, K * K * C1); vec("conv2_b", 2 * C2)
    else:
        mat("conv2_w", C2, K * K * C1); vec("conv2_b", C2)
    if mode == 2:
        mat("gate2_w", C2, gkh * K * C1); vec("gate2_b", C2)
    mat("feout_w", d, F2 * C2); vec("feout_b", d)
    vec("fp_ln_g", d); vec("fp_ln_b", d); mat("fp_w", d, d); vec("fp_b", d)
    for l in range(L + int(bool(c.get("finetune_with_additional_layer", False)))):     # layer L = the fine-tuning head's `additional_layer` (bestrq.py:199-200)
        p = f"l{l}."
        ffs = ("ff1", "ff2") if c.get("use_macaron_ff", True) else ()
        for ff in ffs[:1]:
            vec(p + ff + "_ln_g", d); vec(p + ff + "_ln_b", d); mat(p + ff + "_w1", I, d); vec(p + ff + "_b1", I); mat(p + ff + "_w2", d, I); vec(p + ff + "_b2", d)
        vec(p + "att_ln_g", d); vec(p + "att_ln_b", d)
        mat(p + "att_wqkv", 3 * d, d); vec(p + "att_bqkv", 3 * d); mat(p + "att_wo", d, d); vec(p + "att_bo", d)
        if rel:
            mat(p + "att_wpos", d, d); vec(p + "att_u", d); vec(p + "att_v", d)          # pos_bias_* : "bias" in the name -> no decay
        vec(p + "mlp_ln_g", d); vec(p + "mlp_ln_b", d); mat(p + "mlp_w1", I, d); vec(p + "mlp_b1", I)
        vec(p + "csgu_ln_g", I // 2); vec(p + "csgu_ln_b", I // 2); vec(p + "csgu_w", I // 2, kc, decay=True); vec(p + "csgu_b", I // 2)
        if c.get("csgu_use_linear_after_conv", False):
            mat(p + "csgu_lin_w", I // 2, I // 2); vec(p + "csgu_lin_b", I // 2)
        mat(p + "mlp_w2", d, I // 2); vec(p + "mlp_b2", d)
        vec(p + "mrg_dw_w", 2 * d, km, decay=True); vec(p + "mrg_dw_b", 2 * d); mat(p + "mrg_w", d, 2 * d); vec(p + "mrg_b", d)
        for ff in ffs[1:]:
            vec(p + ff + "_ln_g", d); vec(p + ff + "_ln_b", d); mat(p + ff + "_w1", I, d); vec(p + ff + "_b1", I); mat(p + ff + "_w2", d, I); vec(p + ff + "_b2", d)
        vec(p + "fin_ln_g", d); vec(p + "fin_ln_b", d)
    vec("enc_ln_g", d); vec("enc_ln_b", d)
    if c.get("finetune_with_layer_mixing", False):
        vec("mix_w", L + 1, decay=True)          # `per_layer_weights` (bestrq.py:202-205): a plain nn.Parameter, so weight decay applies
    if head:
        mat("head_w", V1, d); vec("head_b", V1)
    return S


def _enc_map(c: dict, head: bool = True):
    """packed name -> Ref (the encoder's packed layouts <-> the reference's state-dict names)"""
    d, L = c["hidden_size"], c["num_hidden_layers"]
    C1, C2 = c["conv_dim"]
    K = c["conv_kernel"][0]
    V = c["vocab_size"]
    F2 = conv_freq_out(c.get("num_fbanks", 80), c["conv_kernel"], c["conv_stride"], c["conv_padding"])
    kc, km = c.get("csgu_kernel_size", 31), c.get("merge_conv_kernel", 31)
    fe, fp = "wav2vec2.feature_extractor.", "wav2vec2.feature_projection."
    cw = "" if c.get("is_causal", False) else ".conv"
    m = {}
    one = partial(_one, m)
    # optional in the reference (present iff mask_time_prob > 0 or mask_feature_prob > 0): absent -> zeros, not exported
    m["masked_spec_embed"] = Ref(lambda sd: sd["wav2vec2.masked_spec_embed"] if "wav2vec2.masked_spec_embed" in sd else torch.zeros(d),
                                 [("wav2vec2.masked_spec_embed", lambda t: t)], optional=True)
    mode = context_mode(c)
    if mode:        # ContextAwareConv2d.conv is a Gated* module: keys ...conv.N.0.conv.{conv,gate}.{weight,bias} (extractors.py:23-54)
        gkh = K * (GATE_SHARE if mode == 2 else 1)
        c1, c2 = f"{fe}conv.0.0.conv.", f"{fe}conv.1.0.conv."
        cl = lambda t: t.permute(0, 2, 3, 1).reshape(t.shape[0], -1)                                  # (Cout, Cin, KH, KW) -> (Cout, (kh, kw, cin))
        uncl = lambda kh: (lambda t: t.reshape(C2, kh, K, C1).permute(0, 3, 1, 2))
        one("conv1_w", c1 + "conv.weight", lambda t: t.reshape(C1, K * K), lambda t: t.reshape(C1, 1, K, K))
        one("conv1_b", c1 + "conv.bias")
        one("gate1_w", c1 + "gate.weight", lambda t: t.reshape(C1, gkh * K), lambda t: t.reshape(C1, 1, gkh, K))
        one("gate1_b", c1 + "gate.bias")
        if mode == 1:
            m["conv2_w"] = Ref(lambda sd: torch.cat([cl(sd[c2 + "conv.weight"]), cl(sd[c2 + "gate.weight"])], 0),
                               [(c2 + "conv.weight", lambda t: uncl(K)(t[:C2])), (c2 + "gate.weight", lambda t: uncl(K)(t[C2:]))])
            m["conv2_b"] = Ref(lambda sd: torch.cat([sd[c2 + "conv.bias"], sd[c2 + "gate.bias"]], 0),
                               [(c2 + "conv.bias", lambda t: t[:C2]), (c2 + "gate.bias", lambda t: t[C2:])])
        else:
            one("conv2_w", c2 + "conv.weight", cl, uncl(K)); one("conv2_b", c2 + "conv.bias")
            one("gate2_w", c2 + "gate.weight", cl, uncl(gkh)); one("gate2_b", c2 + "gate.bias")
    else:
        one("conv1_w", f"{fe}conv.0.0{cw}.weight", lambda t: t.reshape(C1, K * K), lambda t: t.reshape(C1, 1, K, K))
        one("conv1_b", f"{fe}conv.0.0{cw}.bias")
        one("conv2_w", f"{fe}conv.1.0{cw}.weight", lambda t: t.permute(0, 2, 3, 1).reshape(C2, K * K * C1),
            lambda t: t.reshape(C2, K, K, C1).permute(0, 3, 1, 2))
        one("conv2_b", f"{fe}conv.1.0{cw}.bias")
    one("feout_w", fe + "out.weight", lambda t: t.reshape(d, C2, F2).permute(0, 2, 1).reshape(d, F2 * C2),
        lambda t: t.reshape(d, F2, C2).permute(0, 2, 1).reshape(d, C2 * F2))
    one("feout_b", fe + "out.bias")
    one("fp_ln_g", fp + "layer_norm.weight"); one("fp_ln_b", fp + "layer_norm.bias")
    one("fp_w", fp + "projection.weight"); one("fp_b", fp + "projection.bias")
    one("enc_ln_g", "wav2vec2.encoder.layer_norm.weight"); one("enc_ln_b", "wav2vec2.encoder.layer_norm.bias")
    if head:
        m["head_w"] = Ref(lambda sd: torch.cat([sd["lm_head.weight"], sd["blank_projection.weight"]], 0),
                          [("lm_head.weight", lambda t: t[:V]), ("blank_projection.weight", lambda t: t[V:])])
        m["head_b"] = Ref(lambda sd: torch.cat([sd["lm_head.bias"], sd["blank_projection.bias"]], 0),
                          [("lm_head.bias", lambda t: t[:V]), ("blank_projection.bias", lambda t: t[V:])])
    if c.get("finetune_with_layer_mixing", False):
        one("mix_w", "per_layer_weights")
    for l in range(L + int(bool(c.get("finetune_with_additional_layer", False)))):
        p, r = f"l{l}.", (f"wav2vec2.encoder.layers.{l}." if l < L else "additional_layer.")
        if c.get("use_macaron_ff", True):
            for ff in ("ff1", "ff2"):
                one(p + ff + "_ln_g", r + ff + ".0.weight"); one(p + ff + "_ln_b", r + ff + ".0.bias")
                one(p + ff + "_w1", r + ff + ".1.intermediate_dense.weight"); one(p + ff + "_b1", r + ff + ".1.intermediate_dense.bias")
                one(p + ff + "_w2", r + ff + ".1.output_dense.weight"); one(p + ff + "_b2", r + ff + ".1.output_dense.bias")
        one(p + "att_ln_g", r + "self_attn_layer_norm.weight"); one(p + "att_ln_b", r + "self_attn_layer_norm.bias")
        a = r + "self_attn."
        # [Wq; Wk; Wv] as one (3d, d) matrix: the fused QKV GEMM uses all rows, the Q/K-only and V-only GEMMs row views
        m[p + "att_wqkv"] = Ref(lambda sd, a=a: torch.cat([sd[a + f"linear_{n}.weight"] for n in "qkv"], 0),
                                [(a + f"linear_{n}.weight", (lambda t, i=i: t[i * d:(i + 1) * d])) for i, n in enumerate("qkv")])
        m[p + "att_bqkv"] = Ref(lambda sd, a=a: torch.cat([sd[a + f"linear_{n}.bias"] for n in "qkv"], 0),
                                [(a + f"linear_{n}.bias", (lambda t, i=i: t[i * d:(i + 1) * d])) for i, n in enumerate("qkv")])
        one(p + "att_wo", a + "linear_out.weight"); one(p + "att_bo", a + "linear_out.bias")
        if c.get("position_embeddings_type", "relative") == "relative":
            H = c["num_attention_heads"]
            one(p + "att_wpos", a + "linear_pos.weight")
            one(p + "att_u", a + "pos_bias_u", lambda t: t.reshape(d), lambda t: t.reshape(H, d // H))
            one(p + "att_v", a + "pos_bias_v", lambda t: t.reshape(d), lambda t: t.reshape(H, d // H))
        one(p + "mlp_ln_g", r + "cgMLP_layer_norm.weight"); one(p + "mlp_ln_b", r + "cgMLP_layer_norm.bias")
        g = r + "cgMLP."
        one(p + "mlp_w1", g + "channel_proj1.0.weight"); one(p + "mlp_b1", g + "channel_proj1.0.bias")
        one(p + "csgu_ln_g", g + "csgu.norm.weight"); one(p + "csgu_ln_b", g + "csgu.norm.bias")
        one(p + "csgu_w", g + "csgu.conv.weight", lambda t: t.reshape(-1, kc), lambda t: t.reshape(-1, 1, kc))
        one(p + "csgu_b", g + "csgu.conv.bias")
        if c.get("csgu_use_linear_after_conv", False):
            one(p + "csgu_lin_w", g + "csgu.linear.weight"); one(p + "csgu_lin_b", g + "csgu.linear.bias")
        one(p + "mlp_w2", g + "channel_proj2.weight"); one(p + "mlp_b2", g + "channel_proj2.bias")
        one(p + "mrg_dw_w", r + "depthwise_conv_fusion.weight", lambda t: t.reshape(-1, km), lambda t: t.reshape(-1, 1, km))
        one(p + "mrg_dw_b", r + "depthwise_conv_fusion.bias")
        one(p + "mrg_w", r + "merge_proj.weight"); one(p + "mrg_b", r + "merge_proj.bias")
        one(p + "fin_ln_g", r + "final_layer_norm.weight"); one(p + "fin_ln_b", r + "final_layer_norm.bias")
    return m


# ====================================================================================================== GPT-2 decoder parameters
def decoder_specs(c: dict, enc_dim: int, with_proj: bool) -> list[Spec]:
    d, L, V = c["n_embd"], c["n_layer"], c["vocab_size"]
    S = []
    mat = lambda n, *sh: S.append(Spec(n, tuple(sh), True, True))
    vec = lambda n, *sh, decay=False: S.append(Spec(n, tuple(sh), False, decay))
    if with_proj:
        mat("proj_w", d, enc_dim); vec("proj_b", d)
    mat("wte", V, d)                                       # fp32 master feeds the embedding gather, bf16 mirror a tied lm_head
    if not c.get("pos_emb_fixed", False):
        vec("wpe", c.get("n_positions", 1024), d, decay=True)
    for l in range(L):
        p = f"h{l}."
        vec(p + "ln1_g", d); vec(p + "ln1_b", d); mat(p + "wqkv", 3 * d, d); vec(p + "bqkv", 3 * d); mat(p + "wo", d, d); vec(p + "bo", d)
        vec(p + "lnc_g", d); vec(p + "lnc_b", d); mat(p + "wq", d, d); vec(p + "bq", d); mat(p + "wkv", 2 * d, d); vec(p + "bkv", 2 * d)
        mat(p + "wco", d, d); vec(p + "bco", d)
        vec(p + "ln2_g", d); vec(p + "ln2_b", d); mat(p + "wfc", 4 * d, d); vec(p + "bfc", 4 * d); mat(p + "wpr", d, 4 * d); vec(p + "bpr", d)
    vec("lnf_g", d); vec("lnf_b", d)
    if not c.get("tie_word_embeddings", False):
        mat("lm_head", V, d)
    for k in range(len(c.get("head_locations") or [])):
        mat(f"head{k}", V, d)
    H = len(c.get("head_locations") or []) + 1
    mode = c.get("mixing_mode")                            # GPT2LMMultiHeadModelMixing (multi_head_gpt2_mixing.py:39-51): fp32, folded into the head by `head_fold`
    if mode == "scalar":
        vec("mix", H, decay=True)
    elif mode == "linear":
        vec("mix", H, V, decay=True)
    elif mode == "full":
        vec("mix_w", V, H * V, decay=True); vec("mix_b", V)
    elif mode is not None:
        raise NotImplementedError(f"Mixing mode {mode} not implemented.")
    return S


def _dec_map(c: dict, with_proj: bool, prefix="decoder."):
    L = c["n_layer"]
    m = {}
    one = partial(_one, m)
    tr_in = lambda t: t.t().contiguous()                   # transformers Conv1D stores (in, out); the store keeps (out, in)
    tr = lambda t: t.t()                                   # export: a transposed VIEW (alias_views hands it to the nn.Parameter; state_dict() clones it contiguous)
    if with_proj:
        one("proj_w", "enc_to_dec_proj.weight"); one("proj_b", "enc_to_dec_proj.bias")
    t = prefix + "transformer."
    if c.get("pos_emb_fixed", False):
        one("wte", t + "wte.emb_layers.0.weight")
    else:
        one("wte", t + "wte.weight"); one("wpe", t + "wpe.weight")
    for l in range(L):
        p, r = f"h{l}.", f"{t}h.{l}."
        one(p + "ln1_g", r + "ln_1.weight"); one(p + "ln1_b", r + "ln_1.bias")
        one(p + "wqkv", r + "attn.c_attn.weight", tr_in, tr); one(p + "bqkv", r + "attn.c_attn.bias")
        one(p + "wo", r + "attn.c_proj.weight", tr_in, tr); one(p + "bo", r + "attn.c_proj.bias")
        one(p + "lnc_g", r + "ln_cross_attn.weight"); one(p + "lnc_b", r + "ln_cross_attn.bias")
        one(p + "wq", r + "crossattention.q_attn.weight", tr_in, tr); one(p + "bq", r + "crossattention.q_attn.bias")
        one(p + "wkv", r + "crossattention.c_attn.weight", tr_in, tr); one(p + "bkv", r + "crossattention.c_attn.bias")
        one(p + "wco", r + "crossattention.c_proj.weight", tr_in, tr); one(p + "bco", r + "crossattention.c_proj.bias")
        one(p + "ln2_g", r + "ln_2.weight"); one(p + "ln2_b", r + "ln_2.bias")
        one(p + "wfc", r + "mlp.c_fc.weight", tr_in, tr); one(p + "bfc", r + "mlp.c_fc.bias")
        one(p + "wpr", r + "mlp.c_proj.weight", tr_in, tr); one(p + "bpr", r + "mlp.c_proj.bias")
    one("lnf_g", t + "ln_f.weight"); one("lnf_b", t + "ln_f.bias")
    if not c.get("tie_word_embeddings", False):
        one("lm_head", prefix + "lm_head.weight")
    for k in range(len(c.get("head_locations") or [])):
        one(f"head{k}", f"{prefix}additional_lm_heads.{k}.weight")
    if c.get("mixing_mode") in ("scalar", "linear"):
        one("mix", prefix + "lm_mixing")
    elif c.get("mixing_mode") == "full":
        one("mix_w", prefix + "lm_mixing.weight"); one("mix_b", prefix + "lm_mixing.bias")
    return m


def head_taps(c: dict) -> list:
    """where the heads of a multi-head decoder read the stream, additional heads first, `lm_head` last — transformers' `hidden_states` index: 0 the embedding output,
    l the residual stream after l blocks (no LayerNorm), n_layer ln_f of the last block's output (multi_head_gpt2.py:143-148)"""
    L = c["n_layer"]
    locs = [int(l) for l in (c.get("head_locations") or [])]
    bad = [l for l in locs if not 0 <= l <= L]
    if bad:
        raise ValueError(f"head_locations {bad} outside [0, n_layer = {L}]")
    return locs + [L]


def mixes_heads(c: dict) -> bool:
    """does decoding read more than `lm_head`?  Every mixing mode, and `average_logits` with additional heads (multi_head_gpt2.py:129-136)"""
    return c.get("mixing_mode") is not None or (bool(c.get("average_logits", False)) and bool(c.get("head_locations")))


def head_fold(c: dict, heads: list, mix: dict):
    """Every way the reference forms decode-time logits from several heads is  logits = sum_h A_h hidden[loc_h] (+ b):  -> (the folded head [A_0 | ... | A_{H-1}] of shape
    (V, H d), b (V) or None), in the precision of its inputs (the engine passes fp32 and rounds the result to bf16 once).  `heads`: the H head matrices (V, d) in
    `head_taps` order; `mix`: "mix" (scalar (H,) / linear (H, V)) or "mix_w" (V, H V) + "mix_b" (V) of GPT2LMMultiHeadModelMixing:
      scalar / linear  logits = sum_h mix[h, v] head_h(.)            -> A_h = rows of W_h scaled by mix[h, v]          (multi_head_gpt2_mixing.py:111-121)
      full             logits = W_mix [head_0(.) | ...] + b_mix      -> A_h = W_mix[:, hV:(h+1)V] W_h, b = b_mix      (:101-110)
      average_logits   logits = sum_h head_weights[h] head_h(.)      -> A_h = head_weights[h] W_h                     (multi_head_gpt2.py:129-136)"""
    H, V = len(heads), heads[0].shape[0]
    mode = c.get("mixing_mode")
    if mode == "scalar":
        return torch.cat([mix["mix"][h] * heads[h] for h in range(H)], 1), None
    if mode == "linear":
        return torch.cat([mix["mix"][h][:, None] * heads[h] for h in range(H)], 1), None
    if mode == "full":
        return torch.cat([mix["mix_w"][:, h * V:(h + 1) * V] @ heads[h] for h in range(H)], 1), mix["mix_b"]
    if mode is not None:
        raise NotImplementedError(f"Mixing mode {mode} not implemented.")
    hw = list(c.get("head_weights") or [1.0])
    return torch.cat([float(hw[h]) * heads[h] for h in range(H)], 1), None


# ====================================================================================================== GPT-2 language model parameters (shallow fusion)
def lm_specs(c: dict) -> list[Spec]:
    """transformers' `GPT2LMHeadModel` without cross-attention — the external language model of shallow fusion (reference src/decoding/shallow_fussion.py; trained by
    src/trainers/train_clm.py) — in the names of `decoder_specs`: the same block minus its six cross parameters, learned positions, a tied or separate head."""
    d, L, V = c["n_embd"], c["n_layer"], c["vocab_size"]
    S = []
    mat = lambda n, *sh: S.append(Spec(n, tuple(sh), True, True))
    vec = lambda n, *sh, decay=False: S.append(Spec(n, tuple(sh), False, decay))
    mat("wte", V, d)
    vec("wpe", c.get("n_positions", 1024), d, decay=True)
    for l in range(L):
        p = f"h{l}."
        vec(p + "ln1_g", d); vec(p + "ln1_b", d); mat(p + "wqkv", 3 * d, d); vec(p + "bqkv", 3 * d); mat(p + "wo", d, d); vec(p + "bo", d)
        vec(p + "ln2_g", d); vec(p + "ln2_b", d); mat(p + "wfc", 4 * d, d); vec(p + "bfc", 4 * d); mat(p + "wpr", d, 4 * d); vec(p + "bpr", d)
    vec("lnf_g", d); vec("lnf_b", d)
    if not c.get("tie_word_embeddings", True):
        mat("lm_head", V, d)
    return S


def _lm_map(c: dict, prefix: str = ""):
    """packed name -> Ref for transformers' `GPT2LMHeadModel` state-dict names (Conv1D weights (in, out) transposed, as `_dec_map` does)"""
    m = {}
    one = partial(_one, m)
    tr_in = lambda t: t.t().contiguous()
    tr = lambda t: t.t()
    t = prefix + "transformer."
    one("wte", t + "wte.weight"); one("wpe", t + "wpe.weight")
    for l in range(c["n_layer"]):
        p, r = f"h{l}.", f"{t}h.{l}."
        one(p + "ln1_g", r + "ln_1.weight"); one(p + "ln1_b", r + "ln_1.bias")
        one(p + "wqkv", r + "attn.c_attn.weight", tr_in, tr); one(p + "bqkv", r + "attn.c_attn.bias")
        one(p + "wo", r + "attn.c_proj.weight", tr_in, tr); one(p + "bo", r + "attn.c_proj.bias")
        one(p + "ln2_g", r + "ln_2.weight"); one(p + "ln2_b", r + "ln_2.bias")
        one(p + "wfc", r + "mlp.c_fc.weight", tr_in, tr); one(p + "bfc", r + "mlp.c_fc.bias")
        one(p + "wpr", r + "mlp.c_proj.weight", tr_in, tr); one(p + "bpr", r + "mlp.c_proj.bias")
    one("lnf_g", t + "ln_f.weight"); one("lnf_b", t + "ln_f.bias")
    if not c.get("tie_word_embeddings", True):
        one("lm_head", prefix + "lm_head.weight")
    return m


# ====================================================================================================== Whisper decoder parameters
def _whisper_as_gpt2(c: dict) -> dict:
    """a transformers `WhisperConfig`'s decoder fields in the keys `decoder_specs` reads: learned positions, the token embedding tied as the head"""
    return dict(n_embd=c["d_model"], n_layer=c["decoder_layers"], n_head=c["decoder_attention_heads"], vocab_size=c["vocab_size"],
                n_positions=c["max_target_positions"], tie_word_embeddings=True)


def whisper_decoder_specs(c: dict) -> list[Spec]:
    """The Whisper decoder in the slots of the GPT-2 step (`decoder_specs`; the step's table is 5 globals + 18 per layer): the block is the same pre-LN block, with
    [Wq; Wk; Wv] as wqkv (K bias zero: k_proj has none), the cross [Wk; Wv] as wkv (K bias zero), fc1 / fc2 as wfc / wpr, embed_positions as wpe, no separate head."""
    return decoder_specs(_whisper_as_gpt2(c), c["d_model"], False)


def _whisper_dec_map(c: dict, prefix: str = ""):
    """packed name -> Ref for transformers' `WhisperDecoder` state-dict names"""
    d, L = c["d_model"], c["decoder_layers"]
    m = {}
    one = partial(_one, m)
    one("wte", prefix + "embed_tokens.weight"); one("wpe", prefix + "embed_positions.weight")
    for l in range(L):
        p, r = f"h{l}.", f"{prefix}layers.{l}."
        sa, ca = r + "self_attn.", r + "encoder_attn."
        one(p + "ln1_g", r + "self_attn_layer_norm.weight"); one(p + "ln1_b", r + "self_attn_layer_norm.bias")
        m[p + "wqkv"] = Ref(lambda sd, a=sa: torch.cat([sd[a + f"{n}_proj.weight"] for n in "qkv"], 0),
                            [(sa + f"{n}_proj.weight", (lambda t, i=i: t[i * d:(i + 1) * d])) for i, n in enumerate("qkv")])
        m[p + "bqkv"] = Ref(lambda sd, a=sa: torch.cat([sd[a + "q_proj.bias"], torch.zeros_like(sd[a + "q_proj.bias"]), sd[a + "v_proj.bias"]], 0),
                            [(sa + "q_proj.bias", lambda t: t[:d]), (sa + "v_proj.bias", lambda t: t[2 * d:])])
        one(p + "wo", sa + "out_proj.weight"); one(p + "bo", sa + "out_proj.bias")
        one(p + "lnc_g", r + "encoder_attn_layer_norm.weight"); one(p + "lnc_b", r + "encoder_attn_layer_norm.bias")
        one(p + "wq", ca + "q_proj.weight"); one(p + "bq", ca + "q_proj.bias")
        m[p + "wkv"] = Ref(lambda sd, a=ca: torch.cat([sd[a + "k_proj.weight"], sd[a + "v_proj.weight"]], 0),
                           [(ca + "k_proj.weight", lambda t: t[:d]), (ca + "v_proj.weight", lambda t: t[d:])])
        m[p + "bkv"] = Ref(lambda sd, a=ca: torch.cat([torch.zeros_like(sd[a + "v_proj.bias"]), sd[a + "v_proj.bias"]], 0), [(ca + "v_proj.bias", lambda t: t[d:])])
        one(p + "wco", ca + "out_proj.weight"); one(p + "bco", ca + "out_proj.bias")
        one(p + "ln2_g", r + "final_layer_norm.weight"); one(p + "ln2_b", r + "final_layer_norm.bias")
        one(p + "wfc", r + "fc1.weight"); one(p + "bfc", r + "fc1.bias")
        one(p + "wpr", r + "fc2.weight"); one(p + "bpr", r + "fc2.bias")
    one("lnf_g", prefix + "layer_norm.weight"); one("lnf_b", prefix + "layer_norm.bias")
    return m


def suppression_vectors(V: int, suppress_tokens=None, begin_suppress_tokens=None, device="cpu"):
    """(every step's, the first generated token's) fp32 (V) vectors added to the logits: -inf at a suppressed id, 0 elsewhere — transformers'
    SuppressTokensLogitsProcessor and, for the first generated token only, SuppressTokensAtBeginLogitsProcessor on top of it.  None where nothing is suppressed."""
    def vec(ids):
        ids = [int(i) for i in ids]
        bad = [i for i in ids if not 0 <= i < V]
        if bad:
            raise ValueError(f"suppressed token ids {bad} outside the vocabulary [0, {V})")
        v = torch.zeros(V, dtype=torch.float32)
        if ids:
            v[torch.tensor(ids, dtype=torch.long)] = float("-inf")
        return v.to(device)
    always, begin = list(suppress_tokens or []), list(begin_suppress_tokens or [])
    every = vec(always) if always else None
    first = vec(always + begin) if (always or begin) else None
    return every, first


# ====================================================================================================== encoder position tables
def relative_position_table(T2: int, d: int) -> torch.Tensor:
    """(2*T2-1, d) fp32 sinusoids of the relative positions T2-1 ... -(T2-1), one per row (tf wav2vec2_conformer :159-205)"""
    pos = torch.arange(T2 - 1, -T2, -1, dtype=torch.float32)[:, None]
    div = torch.exp(torch.arange(0, d, 2, dtype=torch.int64).float() * -(math.log(10000.0) / d))
    pe = torch.zeros(2 * T2 - 1, d)
    pe[:, 0::2] = torch.sin(pos * div)
    pe[:, 1::2] = torch.cos(pos * div)
    return pe


def rotary_tables(T2: int, hd: int, base=10000):
    """(cos, sin), each (T2, hd) fp32, of the rotary embedding of head size hd (tf :125-156)"""
    inv = 1.0 / (base ** (torch.arange(0, hd, 2, dtype=torch.int64).float() / hd))
    fr = torch.einsum("i,j->ij", torch.arange(T2).float(), inv)
    emb = torch.cat((fr, fr), dim=-1)
    return emb.cos(), emb.sin()
