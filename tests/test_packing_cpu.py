"""CPU tests of the one definition of the packed weight layouts (huggingface_asr_amd/packing.py): the forward engines' slot tables hold what the
trainers' flat store holds, the layout rules agree with formulas written out here on the reference's tensors, and the three things only the
forward kernels want (V row views, the gated conv2's block interleave, ln_fold) are what their kernels read.  The engines run on device "cpu",
where loading weights is plain torch; nothing here launches a kernel."""
import pytest
import torch

from helpers import TINY_DEC
from huggingface_asr_amd import _lib, packing, shapes, synth
from huggingface_asr_amd.decoder import GPT2DecoderEngine
from huggingface_asr_amd.engine import G, LS, EBranchformerEngine
from huggingface_asr_amd.train import ParamStore, _enc_map, encoder_specs
from huggingface_asr_amd.train_aed import _dec_map, decoder_specs

BF16, F32 = torch.bfloat16, torch.float32
FAMILIES = {"plain": {}, "rotary": {"position_embeddings_type": "rotary"}, "causal": {"is_causal": True},
            "gated": {"context_awareness_type": "gated", "conv_dim": [32, 64]}, "gated_shared": {"context_awareness_type": "gated_shared"},
            "no_macaron": {"use_macaron_ff": False}, "csgu_linear": {"csgu_use_linear_after_conv": True, "csgu_activation": "gelu"},
            "extra_layer_and_mixing": {"finetune_with_additional_layer": True, "finetune_with_layer_mixing": True},
            "fold": {"hidden_size": 256, "intermediate_size": 512}}
FOLD_SLOTS = [n for n in LS if n.endswith(("_WF", "_SF", "_CF"))]


def _loaded(extra):
    cfg = dict(shapes.TINY, **extra)
    sd = {k: torch.from_numpy(v) for k, v in synth.state_dict_numpy(shapes.param_shapes(cfg), 3).items()}
    eng = EBranchformerEngine(cfg, "cpu")
    eng.load_state_dict(sd)
    return cfg, sd, eng


def _slot(eng, name, layer=None):
    return eng._slots[G[name] if layer is None else _lib.GLOBAL_SLOTS + layer * _lib.LAYER_SLOTS + LS[name]]


def _slot_of_packed(name):
    """where the engine keeps a packed parameter: (slot name, layer or None)"""
    l, _, n = name.rpartition(".")
    return {"att_wqkv": "ATT_WQK", "att_bqkv": "ATT_BQK"}.get(n, n.upper()), (int(l[1:]) if l else None)


@pytest.mark.parametrize("family", list(FAMILIES))
def test_engine_slots_hold_the_trainer_stores_packed_parameters(family):
    cfg, sd, eng = _loaded(FAMILIES[family])
    store = ParamStore(encoder_specs(cfg), "cpu", _enc_map(cfg))
    store.pack(sd)
    d, n_layers = cfg["hidden_size"], cfg["num_hidden_layers"] + int(bool(cfg.get("finetune_with_additional_layer", False)))
    named = set()
    for s in store.specs.values():
        if s.name == "masked_spec_embed":               # training only: no slot
            continue
        sname, layer = _slot_of_packed(s.name)
        named.add((sname, layer))
        got = _slot(eng, sname, layer)
        assert got is not None and got.dtype == (BF16 if s.mat else F32) and got.is_contiguous() and got.shape == s.shape, s.name
        if family == "gated" and s.name in ("conv2_w", "conv2_b"):       # same rows in another order: checked row by row below
            continue
        assert torch.equal(got, store.p(s.name).to(got.dtype)), s.name
    # everything else that is filled: the V views and, where the shapes qualify, the fold slots; nothing unaccounted for
    filled = {(n, None) for n in G if _slot(eng, n) is not None} | {(n, l) for l in range(n_layers) for n in LS if _slot(eng, n, l) is not None}
    fold = {(n, l) for l in range(n_layers) for n in FOLD_SLOTS} if family == "fold" else set()
    assert filled - named == {(n, l) for l in range(n_layers) for n in ("ATT_WV", "ATT_BV")} | fold and named <= filled
    assert len(fold) == (24 if family == "fold" else 0)
    assert len(eng._table) == len(eng._slots) == _lib.GLOBAL_SLOTS + n_layers * _lib.LAYER_SLOTS
    assert [p is None for p in eng._table] == [t is None for t in eng._slots]
    # V-only GEMM operands: linear_v, as row VIEWS of the packed [Wq; Wk; Wv] (no second copy)
    for l in range(n_layers):
        r = (f"wav2vec2.encoder.layers.{l}." if l < cfg["num_hidden_layers"] else "additional_layer.") + "self_attn.linear_v."
        for v, qk, ref in (("ATT_WV", "ATT_WQK", sd[r + "weight"]), ("ATT_BV", "ATT_BQK", sd[r + "bias"])):
            tv, tqk = _slot(eng, v, l), _slot(eng, qk, l)
            assert torch.equal(tv, ref.to(tv.dtype)) and tv.is_contiguous()
            assert tv.untyped_storage().data_ptr() == tqk.untyped_storage().data_ptr() and tv.data_ptr() == tqk[2 * d:].data_ptr()


@pytest.mark.parametrize("family", ["plain", "causal"])
def test_layout_rules_against_the_reference_tensors(family):
    """the rules of packing.py's docstring, element by element on the reference's own tensors (independent of the map's code)"""
    cfg, sd, eng = _loaded(FAMILIES[family])
    d, V, (C1, C2), K = cfg["hidden_size"], cfg["vocab_size"], cfg["conv_dim"], cfg["conv_kernel"][0]
    cw = "" if family == "causal" else ".conv"
    fe = "wav2vec2.feature_extractor."
    w2, got = sd[f"{fe}conv.1.0{cw}.weight"], _slot(eng, "CONV2_W")
    for co, ci, kh, kw in ((0, 0, 0, 0), (5, 7, 1, 2), (C2 - 1, C1 - 1, K - 1, K - 1), (9, 30, 2, 0)):
        assert got[co, (kh * K + kw) * C1 + ci] == w2[co, ci, kh, kw].to(BF16)                 # (Cout, (kh, kw, cin))
    F2 = sd[fe + "out.weight"].shape[1] // C2
    wo, got = sd[fe + "out.weight"], _slot(eng, "FEOUT_W")
    for n, ch, f in ((0, 0, 0), (3, 5, 7), (d - 1, C2 - 1, F2 - 1), (11, 1, F2 - 2)):
        assert got[n, f * C2 + ch] == wo[n, ch * F2 + f].to(BF16)                              # (c, f) columns -> (f, c)
    hw, hb = _slot(eng, "HEAD_W"), _slot(eng, "HEAD_B")
    assert hw.shape == (V + 1, d) and torch.equal(hw[V], sd["blank_projection.weight"][0].to(BF16)) and torch.equal(hw[:V], sd["lm_head.weight"].to(BF16))
    assert hb[V] == sd["blank_projection.bias"][0] and torch.equal(hb[:V], sd["lm_head.bias"])    # blank LAST
    a = "wav2vec2.encoder.layers.1.self_attn."
    wqk = _slot(eng, "ATT_WQK", 1)
    assert all(torch.equal(wqk[i * d:(i + 1) * d], sd[a + f"linear_{n}.weight"].to(BF16)) for i, n in enumerate("qkv"))
    assert torch.equal(_slot(eng, "ATT_U", 1).reshape(-1), sd[a + "pos_bias_u"].reshape(-1))
    assert torch.equal(_slot(eng, "CSGU_W", 0), sd["wav2vec2.encoder.layers.0.cgMLP.csgu.conv.weight"][:, 0])       # depthwise taps (C, 1, k) -> (C, k)
    assert torch.equal(_slot(eng, "MRG_DW_W", 0), sd["wav2vec2.encoder.layers.0.depthwise_conv_fusion.weight"][:, 0])


def test_gated_conv2_rows_are_interleaved_in_blocks_for_the_gemm_epilogue():
    """mode "gated": ONE implicit GEMM computes conv and gate; its epilogue pairs row r of a 2*blk-row group with row r + blk, so the engine's rows are
    [conv channels of block j ; gate channels of block j] for j = 0 .. C2/blk - 1 (the trainer keeps all conv rows, then all gate rows).  C2 = 64 -> two blocks."""
    cfg, sd, eng = _loaded(FAMILIES["gated"])
    (C1, C2), K, blk = cfg["conv_dim"], cfg["conv_kernel"][0], eng.gate_blk
    assert blk == 32 and C2 // blk == 2
    c2 = "wav2vec2.feature_extractor.conv.1.0.conv."
    w, b = _slot(eng, "CONV2_W"), _slot(eng, "CONV2_B")
    assert w.shape == (2 * C2, K * K * C1) and b.shape == (2 * C2,)
    for ch in (0, 5, 31, 32, 40, 63):                   # output channel ch: its conv filter at row 2*blk*j + r, its gate filter blk rows below
        j, r = divmod(ch, blk)
        for part, row in (("conv", 2 * blk * j + r), ("gate", 2 * blk * j + blk + r)):
            ref = sd[c2 + part + ".weight"][ch]         # (Cin, KH, KW)
            assert torch.equal(w[row], ref.permute(1, 2, 0).reshape(-1).to(BF16)), (ch, part)
            assert b[row] == sd[c2 + part + ".bias"][ch], (ch, part)
    # layer 1 keeps conv and gate apart (fp32, a direct kernel): slots of their own
    assert torch.equal(_slot(eng, "GATE1_W"), sd["wav2vec2.feature_extractor.conv.0.0.conv.gate.weight"].reshape(C1, -1))


def test_fold_triple_is_the_layernorm_folded_into_its_linear():
    """ln_fold: LN(x) W^T + b = rstd (x W'^T) - rstd mu colsum(W') + (W beta + b) with W' = bf16(W diag(gamma)); the row sums are of the ROUNDED W' (that is
    what the GEMM multiplies).  Sums of n = 256 fp32 terms: compared with a float64 sum within n * 2^-24 * sum|terms|, the bound of any summation order."""
    cfg, sd, eng = _loaded(FAMILIES["fold"])
    d = cfg["hidden_size"]
    r = "wav2vec2.encoder.layers.1."
    cases = {"FF1": (sd[r + "ff1.1.intermediate_dense.weight"], sd[r + "ff1.1.intermediate_dense.bias"], sd[r + "ff1.0.weight"], sd[r + "ff1.0.bias"]),
             "MLP": (sd[r + "cgMLP.channel_proj1.0.weight"], sd[r + "cgMLP.channel_proj1.0.bias"], sd[r + "cgMLP_layer_norm.weight"], sd[r + "cgMLP_layer_norm.bias"]),
             "QKV": (torch.cat([sd[r + f"self_attn.linear_{n}.weight"] for n in "qkv"]), torch.cat([sd[r + f"self_attn.linear_{n}.bias"] for n in "qkv"]),
                     sd[r + "self_attn_layer_norm.weight"], sd[r + "self_attn_layer_norm.bias"])}
    for tag, (W, b, gamma, beta) in cases.items():
        wf, sf, cf = (_slot(eng, tag + s, 1) for s in ("_WF", "_SF", "_CF"))
        assert wf.dtype == BF16 and sf.dtype == F32 and cf.dtype == F32 and wf.shape == W.shape and sf.shape == cf.shape == b.shape
        for row in (0, 7, W.shape[0] - 1):
            want_w = (W[row] * gamma).to(BF16)
            assert torch.equal(wf[row], want_w), (tag, row)
            bound = d * 2.0 ** -24
            assert abs(sf[row].double() - want_w.double().sum()) <= bound * want_w.double().abs().sum(), (tag, row)
            terms = W[row].double() * beta.double()
            assert abs(cf[row].double() - (terms.sum() + b[row].double())) <= bound * (terms.abs().sum() + b[row].double().abs()) + 2.0 ** -24 * abs(cf[row].double()), (tag, row)


def test_a_missing_reference_key_is_named():
    cfg, sd, _ = _loaded({})
    key = "wav2vec2.encoder.layers.1.cgMLP.channel_proj2.bias"
    with pytest.raises(KeyError, match=key.replace(".", r"\.")):
        EBranchformerEngine(cfg, "cpu").load_state_dict({k: v for k, v in sd.items() if k != key})


def _decoder_state_dict(c, tie):
    g = torch.Generator().manual_seed(11)
    R = lambda *s: torch.randn(*s, generator=g)
    d, V = c["n_embd"], c["vocab_size"]
    t = "decoder.transformer."
    sd = {t + "ln_f.weight": R(d), t + "ln_f.bias": R(d), "decoder.additional_lm_heads.0.weight": R(V, d)}
    if c["pos_emb_fixed"]:
        sd[t + "wte.emb_layers.0.weight"] = wte = R(V, d)
    else:
        sd[t + "wte.weight"] = wte = R(V, d)
        sd[t + "wpe.weight"] = R(c["n_positions"], d)
    sd["decoder.lm_head.weight"] = wte if tie else R(V, d)
    for l in range(c["n_layer"]):
        r = f"{t}h.{l}."
        for n in ("ln_1", "ln_cross_attn", "ln_2"):
            sd[r + n + ".weight"] = R(d); sd[r + n + ".bias"] = R(d)
        for n, (i, o) in (("attn.c_attn", (d, 3 * d)), ("attn.c_proj", (d, d)), ("crossattention.q_attn", (d, d)), ("crossattention.c_attn", (d, 2 * d)),
                          ("crossattention.c_proj", (d, d)), ("mlp.c_fc", (d, 4 * d)), ("mlp.c_proj", (4 * d, d))):
            sd[r + n + ".weight"] = R(i, o); sd[r + n + ".bias"] = R(o)
    return sd


@pytest.mark.parametrize("fixed", [False, True])
@pytest.mark.parametrize("tie", [False, True])
def test_decoder_engine_holds_the_trainer_stores_packed_parameters(fixed, tie):
    c = dict(TINY_DEC, pos_emb_fixed=fixed, tie_word_embeddings=tie)
    d, L = c["n_embd"], c["n_layer"]
    sd = _decoder_state_dict(c, tie)
    eng = GPT2DecoderEngine(c, "cpu")
    eng.load_state_dict(sd, "decoder.")
    store = ParamStore(decoder_specs(c, d, False), "cpu", _dec_map(c, False))
    store.pack(sd)
    w = eng.w
    got = {"wte": w["wte"], "lnf_g": w["lnf"][0], "lnf_b": w["lnf"][1], "head0": w["heads"][0]}
    if not fixed:
        got["wpe"] = w["pos"]
    if not tie:
        got["lm_head"] = w["lm_head"]
    for l, lw in enumerate(w["layers"]):
        got.update({f"h{l}.{n}": t for n, t in lw.items() if torch.is_tensor(t)})
        got.update({f"h{l}.{n}_{s}": lw[n][i] for n in ("ln1", "lnc", "ln2") for i, s in enumerate("gb")})
    assert set(got) == set(store.order)                  # every packed parameter has its place in the engine
    for name, t in got.items():
        s = store.specs[name]
        assert t.dtype == (BF16 if s.mat and name != "wte" else F32) and t.is_contiguous() and t.shape == s.shape, name      # wte feeds the fp32 embedding gather
        assert torch.equal(t, store.p(name).to(t.dtype)), name
    # against the reference's tensors: Conv1D keeps (in, out), the GEMM reads (out, in) rows; a tied head is the token embedding in bf16
    r = "decoder.transformer.h.2."
    for n, key in (("wqkv", "attn.c_attn"), ("wkv", "crossattention.c_attn"), ("wpr", "mlp.c_proj")):
        W = sd[r + key + ".weight"]
        assert w["layers"][2][n].shape == (W.shape[1], W.shape[0]) and w["layers"][2][n][5, 3] == W[3, 5].to(BF16)
    assert torch.equal(w["lm_head"], sd["decoder.lm_head.weight"].to(BF16)) and w["lm_head"].dtype == BF16
    assert w["scale"] == (d ** 0.5 if fixed else 1.0) and w["pos"].shape[1] == d
    # pointer table of the C step: 5 globals, then 18 per layer, in the documented order
    lw = w["layers"][1]
    want = [w["wte"], w["pos"], w["lnf"][0], w["lnf"][1], w["lm_head"]]
    assert list(eng._wtable)[:5] == [t.data_ptr() for t in want] and len(eng._wtable) == 5 + 18 * L
    order = [lw["ln1"][0], lw["ln1"][1], lw["wqkv"], lw["bqkv"], lw["wo"], lw["bo"], lw["lnc"][0], lw["lnc"][1], lw["wq"], lw["bq"],
             lw["wco"], lw["bco"], lw["ln2"][0], lw["ln2"][1], lw["wfc"], lw["bfc"], lw["wpr"], lw["bpr"]]
    assert list(eng._wtable)[5 + 18:5 + 36] == [t.data_ptr() for t in order]
    key = "decoder.transformer.h.1.mlp.c_fc.bias"
    with pytest.raises(KeyError, match=key.replace(".", r"\.")):
        GPT2DecoderEngine(c, "cpu").load_state_dict({k: v for k, v in sd.items() if k != key})


def test_encoder_position_tables():
    """one formula, two arrangements: the engine reads [cos.flat ; sin.flat] in one fp32 buffer and the relative table in bf16"""
    T2, d, H = 9, 64, 4
    rel = packing.relative_position_table(T2, d)
    assert rel.shape == (2 * T2 - 1, d) and not rel[T2 - 1, 0::2].any() and bool((rel[T2 - 1, 1::2] == 1).all())     # the middle row is relative position 0
    assert torch.equal(rel[0, 0::2], -rel[-1, 0::2]) and torch.equal(rel[0, 1::2], rel[-1, 1::2])                      # rows run from +(T2-1) down to -(T2-1)
    torch.testing.assert_close(rel[T2 - 2, :2], torch.stack([torch.tensor(1.0).sin(), torch.tensor(1.0).cos()]))          # position +1, frequency 1: (sin 1, cos 1)
    cos, sin = packing.rotary_tables(T2, d // H, 10000)
    assert cos.shape == sin.shape == (T2, d // H) and torch.equal(cos[:, :d // H // 2], cos[:, d // H // 2:])
    torch.testing.assert_close(cos * cos + sin * sin, torch.ones(T2, d // H))
    torch.testing.assert_close(sin[3, 0], torch.tensor(3.0).sin())
    eng = EBranchformerEngine(dict(shapes.TINY), "cpu")
    t = eng._pos_table(T2)
    assert t.dtype == BF16 and torch.equal(t, rel.to(BF16)) and eng._pos_table(T2) is t
    eng = EBranchformerEngine(dict(shapes.TINY, position_embeddings_type="rotary"), "cpu")
    assert torch.equal(eng._pos_table(T2), torch.cat([cos.reshape(-1), sin.reshape(-1)]))
