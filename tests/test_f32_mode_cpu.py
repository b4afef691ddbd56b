"""CPU: the host side of the fp32 inference mode (engine.py `precision="fp32"`, modeling_ebranchformer.py `hip_precision`): the workspace queries, the
argument checks and the refusals all run without a GPU — nothing here launches a kernel.  (That the new header symbols are exported with the binding's argument
counts is tests/test_abi_cpu.py's test_header_symbols_exported.)"""
import ctypes as C

import pytest
import torch

from huggingface_asr_amd import shapes

SCORES_BOUND = 64 << 20          # MI_ATTENTION_F32_SCORES_BYTES (include/hfasr_hip.h; DESIGN.md §4 'fp32 inference mode')


@pytest.fixture(scope="module")
def lib():
    from huggingface_asr_amd import _lib
    from huggingface_asr_amd.csrc import build as B
    B.build()
    return _lib.lib()


def _engine(cfg=None, **kw):
    from huggingface_asr_amd.engine import EBranchformerEngine
    return EBranchformerEngine(dict(shapes.BASE if cfg is None else cfg), "cpu", **kw)


def test_fp32_workspace_grows_with_batch_and_its_scores_stay_bounded(lib):
    eng = _engine(precision="fp32")
    ws = lambda B, T: int(lib.mi_ebf_f32_workspace_bytes(C.byref(eng._config_struct(B, T, 80))))
    att = lambda B, T: int(lib.mi_attention_f32_workspace_bytes(B, eng.out_frames(T), 4, 128, 1))
    assert 0 < ws(1, 1000) < ws(8, 1000) < ws(32, 1000)
    # the scores: bounded by the documented constant whatever B and T' are, although the un-chunked product B*H*T'*(3T'-1) floats is far above it
    for B, T in ((32, 1000), (96, 2000), (32, 8000), (4, 40000)):
        T2 = eng.out_frames(T)
        assert att(B, T) <= SCORES_BOUND < B * 4 * T2 * (3 * T2 - 1) * 4, (B, T)
    # ... so past the bound the workspace grows with the activations alone: doubling T' doubles it (the scores term would quadruple)
    assert att(32, 8000) == att(32, 16000) == SCORES_BOUND
    a, b = ws(32, 8000), ws(32, 16000)
    assert 1.9 < (b - SCORES_BOUND) / (a - SCORES_BOUND) < 2.1
    # a small problem takes what it needs, not the bound
    assert att(2, 200) == 2 * 50 * (2 * 512 + 4 * (52 + 100)) * 4
    # the bf16 query is untouched and the fp32 one refuses what the mode does not cover
    assert int(lib.mi_ebf_workspace_bytes(C.byref(_engine()._config_struct(32, 1000, 80)))) > 400e6
    cs = eng._config_struct(2, 200, 80)
    for field in ("context_mode", "layer_mixing", "extra_layers", "ln_fold", "wide_tiles", "branch_overlap"):
        setattr(cs, field, 1)
        assert int(lib.mi_ebf_f32_workspace_bytes(C.byref(cs))) == 0, field
        # the forward refuses before anything is launched: no pointer below is ever dereferenced
        assert lib.mi_ebf_forward_f32(C.byref(cs), 8, 8, None, None, None, 0, 8, 1 << 40, None, None, None, None, None) == -3, field
        setattr(cs, field, 0)


def test_unknown_precision_is_a_value_error():
    with pytest.raises(ValueError, match="precision"):
        _engine(precision="fp16")
    assert _engine().precision == "bf16" and _engine(precision="fp32").precision == "fp32"


@pytest.mark.parametrize("kw,word", [(dict(context_awareness_type="gated"), "gated"), (dict(context_awareness_type="gated_shared"), "gated"),
                                     (dict(finetune_with_additional_layer=True), "fine-tuning"), (dict(finetune_with_layer_mixing=True), "fine-tuning")])
def test_fp32_refuses_uncovered_configurations(kw, word):
    with pytest.raises(NotImplementedError, match=word):
        _engine(dict(shapes.TINY, **kw), precision="fp32")
    _engine(dict(shapes.TINY, **kw))                               # the default mode still takes them


def test_fp32_refuses_uncovered_switches(monkeypatch):
    from huggingface_asr_amd.pipeline import ForwardPipeline
    monkeypatch.setenv("HFASR_BRANCH_OVERLAP", "1")
    with pytest.raises(NotImplementedError, match="HFASR_BRANCH_OVERLAP"):
        _engine(precision="fp32")
    monkeypatch.delenv("HFASR_BRANCH_OVERLAP")
    monkeypatch.setenv("HFASR_LN_FOLD", "1")
    with pytest.raises(NotImplementedError, match="ln_fold"):
        _engine(precision="fp32")
    monkeypatch.setenv("HFASR_LN_FOLD", "0")
    eng = _engine(precision="fp32")                                # forcing it OFF is what this mode does anyway
    eng.ln_fold = True                                             # ... and forcing it on after construction is caught where the config struct is built
    with pytest.raises(NotImplementedError, match="ln_fold"):
        eng._config_struct(2, 200, 80)
    monkeypatch.delenv("HFASR_LN_FOLD")
    with pytest.raises(NotImplementedError, match="lanes"):
        ForwardPipeline(dict(shapes.TINY), "cpu", {}, lanes=2, precision="fp32")
    with pytest.raises(NotImplementedError, match="lanes"):
        _engine(precision="fp32").share_weights_from(_engine())
    with pytest.raises(NotImplementedError, match="want_all_hidden"):
        _engine(precision="fp32").forward(torch.zeros(1, 200, 80), want_all_hidden=True)
    with pytest.raises(ValueError, match="logits_dtype"):
        _engine(precision="fp32", logits_dtype=torch.bfloat16)


def test_packed_slot_dtypes():
    """the default engine's slot dtypes are what they were (matrices bf16, the rest fp32, fold tensors present); the fp32 engine fills the same slots, all fp32, no folds"""
    import numpy as np
    from huggingface_asr_amd import synth
    from huggingface_asr_amd.engine import LS
    from huggingface_asr_amd.packing import encoder_specs
    cfg = dict(shapes.TINY, hidden_size=256, num_attention_heads=4, intermediate_size=512)      # a shape the LayerNorm fold takes
    sd = {k: torch.from_numpy(v) for k, v in synth.state_dict_numpy(shapes.param_shapes(cfg), 3).items()}
    a, b = _engine(cfg), _engine(cfg, precision="fp32")
    a.load_state_dict(sd); b.load_state_dict(sd)
    mats = {s.name.rpartition(".")[2] for s in encoder_specs(cfg) if s.mat}
    from huggingface_asr_amd import _lib
    from huggingface_asr_amd.engine import G
    names = {v: k for k, v in G.items()}
    lnames = {v: k for k, v in LS.items()}
    fold = {i for n, i in LS.items() if n[-3:] in ("_WF", "_SF", "_CF")}
    seen_bf16 = 0
    for i, (ta, tb) in enumerate(zip(a._slots, b._slots)):
        li = (i - _lib.GLOBAL_SLOTS) % _lib.LAYER_SLOTS if i >= _lib.GLOBAL_SLOTS else None
        if li in fold:
            assert ta is not None and tb is None, i               # fold tensors: the bf16 mode's alone
            assert ta.dtype == (torch.bfloat16 if lnames[li].endswith("_WF") else torch.float32)
            continue
        assert (ta is None) == (tb is None), i
        if ta is None:
            continue
        name = (names[i] if li is None else lnames[li]).lower()
        is_mat = name in mats or name in ("att_wqk", "att_wv")
        assert ta.dtype == (torch.bfloat16 if is_mat else torch.float32), name
        assert tb.dtype == torch.float32 and tb.shape == ta.shape, name
        seen_bf16 += int(is_mat)
        if not is_mat:
            assert torch.equal(ta, tb), name
        else:
            assert torch.equal(ta, tb.to(torch.bfloat16)), name
    assert seen_bf16 > 10
    assert np.isfinite(float(b._slots[G["HEAD_W"]].sum()))
    # the fp32 position table is the un-rounded sinusoid table
    from huggingface_asr_amd.packing import relative_position_table
    assert b._pos_table(50).dtype == torch.float32 and torch.equal(b._pos_table(50), relative_position_table(50, 256))
    assert a._pos_table(50).dtype == torch.bfloat16


def test_model_precision_resolution_order(monkeypatch):
    """config.hip_precision, then HFASR_PRECISION, then "bf16"; the engine follows the value"""
    from huggingface_asr_amd.configuration_ebranchformer import Wav2Vec2EBranchformerConfig
    from huggingface_asr_amd.modeling_ebranchformer import Wav2Vec2EBranchformerForCTC
    base = dict(shapes.TINY); base.pop("num_fbanks")
    model = Wav2Vec2EBranchformerForCTC(Wav2Vec2EBranchformerConfig(**base))
    monkeypatch.delenv("HFASR_PRECISION", raising=False)
    assert model._precision() == "bf16"
    monkeypatch.setenv("HFASR_PRECISION", "fp32")
    assert model._precision() == "fp32"
    assert model._get_engine("cpu").precision == "fp32"
    model.config.hip_precision = "bf16"                           # the config wins over the environment
    assert model._precision() == "bf16"
    assert model._get_engine("cpu").precision == "bf16"           # ... and a changed value rebuilds the engine
    model.config.hip_precision = None
    assert model._precision() == "fp32"
    monkeypatch.setenv("HFASR_PRECISION", "fp8")
    with pytest.raises(ValueError, match="precision"):
        model._get_engine("cpu")
