"""CPU: the DeCRED head-mixing surface (reference src/models/decoders/multi_head_gpt2_mixing.py) — configuration and parameter holder with the reference's keys and
initial values, the registrations, the decoder swap of `instantiate_aed_model` (src/utilities/model_utils.py:205-218), the load-time fold of the mixing parameters into
one multi-tap head (packing.head_fold) against an fp64 evaluation of the reference's formula, and the new C entry.  No GPU calls."""
import os
import re

import pytest
import torch

import mix_ref as MR
from huggingface_asr_amd.bind import bind_all
from huggingface_asr_amd.modeling_joint import (GPT2LMMultiHeadModel, GPT2LMMultiHeadModelMixing, GPT2MultiHeadConfig, GPT2MultiHeadMixingConfig,
                                                JointCTCAttentionEncoderDecoder, _dec_cfg_dict)
from huggingface_asr_amd.packing import head_fold, head_taps, mixes_heads
from test_surface_cpu import _joint_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V, D, H = 51, 128, 2


def _mix_cfg(mode, **kw):
    return GPT2MultiHeadMixingConfig(vocab_size=V, n_embd=D, n_layer=3, n_head=2, n_positions=64, head_locations=[1], head_weights=[0.4, 0.6], mixing_mode=mode,
                                     add_cross_attention=True, **kw)


def test_config_defaults_and_model_type():
    c = GPT2MultiHeadMixingConfig()
    assert c.model_type == "gpt2-multi-head-mixing" and c.mixing_mode == "full" and c.head_locations is None and c.average_logits is False
    assert GPT2MultiHeadMixingConfig.from_dict(_mix_cfg("scalar").to_dict()).mixing_mode == "scalar"


@pytest.mark.parametrize("mode", MR.MODES)
def test_state_dict_keys_shapes_and_initial_values(mode):
    """multi_head_gpt2_mixing.py:39-51: the plain multi-head decoder's keys plus `lm_mixing` ((H,) / (H, V), filled with 1 / H) or `lm_mixing.weight` (V, H V) =
    eye(V) repeated H times * 0.5 with a zero `lm_mixing.bias`"""
    m = GPT2LMMultiHeadModelMixing(_mix_cfg(mode))
    plain = GPT2LMMultiHeadModel(GPT2MultiHeadConfig(vocab_size=V, n_embd=D, n_layer=3, n_head=2, n_positions=64, head_locations=[1], head_weights=[0.4, 0.6],
                                                     add_cross_attention=True))
    extra = {k: v for k, v in m.state_dict().items() if k not in plain.state_dict()}
    assert {k: tuple(v.shape) for k, v in m.state_dict().items() if k in plain.state_dict()} == {k: tuple(v.shape) for k, v in plain.state_dict().items()}
    if mode == "full":
        assert {k: tuple(v.shape) for k, v in extra.items()} == {"lm_mixing.weight": (V, H * V), "lm_mixing.bias": (V,)}
        assert torch.equal(extra["lm_mixing.weight"], torch.eye(V).repeat(1, H) * 0.5) and not extra["lm_mixing.bias"].any()
    else:
        assert {k: tuple(v.shape) for k, v in extra.items()} == {"lm_mixing": (H,) if mode == "scalar" else (H, V)}
        assert torch.equal(extra["lm_mixing"], torch.full_like(extra["lm_mixing"], 1 / H))
    assert all(p.requires_grad for n, p in m.named_parameters() if n.startswith("lm_mixing"))
    with pytest.raises(RuntimeError):
        m(torch.zeros(1, 2, dtype=torch.long))                       # a parameter holder: the tensor work runs inside the joint model


def test_unknown_mode_raises_as_the_reference_does():
    with pytest.raises(NotImplementedError, match="Mixing mode bogus not implemented"):
        GPT2LMMultiHeadModelMixing(_mix_cfg("bogus"))


def test_registrations_resolve_to_the_hip_classes(tmp_path):
    from transformers import AutoConfig, AutoModelForSpeechSeq2Seq
    from huggingface_asr_amd import bind
    bind_all()
    assert type(AutoConfig.for_model("gpt2-multi-head-mixing")) is GPT2MultiHeadMixingConfig
    names = bind.REBIND["models.decoders.multi_head_gpt2_mixing"]
    assert names == {"GPT2MultiHeadMixingConfig": GPT2MultiHeadMixingConfig, "GPT2LMMultiHeadModelMixing": GPT2LMMultiHeadModelMixing}
    src = open(os.path.join(ROOT, "huggingface_asr_amd", "bind.py")).read()
    assert "CustomModelForCausalLM.register(GPT2MultiHeadMixingConfig, GPT2LMMultiHeadModelMixing" in src
    # a saved mixing checkpoint loads as what it is
    model = _swap(_joint_model(False), "linear")
    with torch.no_grad():
        model.decoder.lm_mixing.add_(torch.arange(H * V).view(H, V) * 1e-3)
    model.save_pretrained(tmp_path / "m")
    again = AutoModelForSpeechSeq2Seq.from_pretrained(tmp_path / "m")
    assert type(again) is JointCTCAttentionEncoderDecoder and type(again.decoder) is GPT2LMMultiHeadModelMixing and again.config.decoder.mixing_mode == "linear"
    assert torch.equal(again.decoder.lm_mixing, model.decoder.lm_mixing)


def _swap(model, mode):
    """the statements of model_utils.py:205-217 (there `CustomModelForCausalLM.from_config(new_config)`, which `bind.install()` registers the HIP class with)"""
    assert isinstance(model.decoder, GPT2LMMultiHeadModel)
    old_config = model.decoder.config
    new_config = GPT2MultiHeadMixingConfig(**old_config.to_dict(), mixing_mode=mode)
    new_decoder = GPT2LMMultiHeadModelMixing(new_config)
    new_decoder.load_state_dict(model.decoder.state_dict(), strict=False)
    model.decoder = new_decoder
    for name, param in model.named_parameters():
        if "lm_mixing" not in name:
            param.requires_grad = False
    return model


@pytest.mark.parametrize("mode", MR.MODES)
def test_decoder_swap_gives_a_hip_joint_model_with_only_the_mix_trainable(mode):
    model = _joint_model(False)
    before = {k: v.clone() for k, v in model.decoder.state_dict().items()}
    model = _swap(model, mode)
    assert type(model) is JointCTCAttentionEncoderDecoder and type(model.decoder) is GPT2LMMultiHeadModelMixing
    assert sorted(n for n, p in model.named_parameters() if p.requires_grad) == sorted("decoder." + k for k in model.decoder.state_dict() if k.startswith("lm_mixing"))
    for k, v in before.items():
        assert torch.equal(model.decoder.state_dict()[k], v), k
    # the joint configuration and the engine's decoder configuration follow the decoder that is there now
    assert model.config.decoder is model.decoder.config
    dc = _dec_cfg_dict(model.decoder.config)
    assert dc["mixing_mode"] == mode and dc["head_locations"] == [1] and dc["lsm_factor"] == 0.1
    assert _dec_cfg_dict(_joint_model(False).decoder.config)["mixing_mode"] is None
    with pytest.raises(TypeError, match="no PyTorch fallback"):
        model.decoder = torch.nn.Linear(2, 2)
    # the training-mode forward: `linear` / `scalar` train on the device (CPU tensors are refused, no fallback), `full` and any other trainable parameter are refused by name
    model.train()
    batch = dict(input_values=torch.zeros(1, 100, 80), labels=torch.zeros(1, 3, dtype=torch.long))
    if mode == "full":
        with pytest.raises(NotImplementedError, match="`full` mixing mode"):
            model(**batch)
    else:
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            model(**batch)
    model.encoder.lm_head.weight.requires_grad_(True)
    with pytest.raises(NotImplementedError, match="model_utils.py:214-217"):
        model(**batch)


def test_tap_rule():
    assert head_taps(dict(n_layer=3, head_locations=[1])) == [1, 3] and head_taps(dict(n_layer=3, head_locations=[0, 3])) == [0, 3, 3]
    assert head_taps(dict(n_layer=3)) == [3]
    with pytest.raises(ValueError):
        head_taps(dict(n_layer=3, head_locations=[4]))
    assert not mixes_heads(dict(head_locations=[1])) and not mixes_heads(dict(average_logits=True)) and mixes_heads(dict(average_logits=True, head_locations=[1]))
    assert mixes_heads(dict(mixing_mode="scalar"))


@pytest.mark.parametrize("mode", [*MR.MODES, None])
@pytest.mark.parametrize("locs", [[1], [0, 3], [3]])
def test_fold_against_the_reference_formula_in_fp64(locs, mode):
    """logits = sum_h A_h hidden[loc_h] (+ b): the folded matrix applied to the concatenated taps against the reference's expression on the per-head logits, both in fp64
    (agreement to rounding: the fold only re-associates), then folded in fp32 and rounded to bf16 once, as the engine does: the error of ONE bf16 rounding of each
    matrix entry, 2^-9 relative per product term"""
    Hn = len(locs) + 1
    cfg, heads, mix, hidden = MR.fold_case(Hn, locs, mode)
    taps = head_taps(cfg)
    want = MR.mix_logits([hidden[t] @ h.T for t, h in zip(taps, heads)], cfg, mix)
    cat = torch.cat([hidden[t] for t in taps], -1)
    fold, bias = head_fold(cfg, heads, mix)
    assert fold.shape == (51, Hn * 16) and (bias is not None) == (mode == "full")
    got = cat @ fold.T + (bias if bias is not None else 0)
    assert float((got - want).abs().max()) < 1e-12
    f32, b32 = head_fold(cfg, [h.float() for h in heads], {k: v.float() for k, v in mix.items()})
    fb = f32.to(torch.bfloat16).double()
    got = cat @ fb.T + (b32.double() if b32 is not None else 0)
    bound = 2.0 ** -9 * (cat.abs() @ fold.abs().T) + 1e-5
    assert bool(((got - want).abs() <= bound).all()), float(((got - want).abs() - bound).max())


def test_engine_folds_at_every_load():
    """the decoder engine keeps the folded head (V, H d) bf16, the fp32 bias of mode `full` and the tap list, and folds again when it is loaded again"""
    from huggingface_asr_amd.decoder import GPT2DecoderEngine
    model = _swap(_joint_model(False), "full")
    eng = GPT2DecoderEngine(_dec_cfg_dict(model.decoder.config), "cpu")
    eng.load_state_dict(dict(model.state_dict()))
    w = eng.w
    assert w["taps"] == [1, 3] and w["head_fold"].shape == (V, H * D) and w["head_fold"].dtype == torch.bfloat16 and w["head_bias"].dtype == torch.float32
    sd = model.state_dict()
    # the initial `full` mix is 0.5 * (head_0 + lm_head): each block of the fold is half its head
    assert torch.equal(w["head_fold"][:, :D], (0.5 * sd["decoder.additional_lm_heads.0.weight"]).to(torch.bfloat16))
    assert torch.equal(w["head_fold"][:, D:], (0.5 * sd["decoder.lm_head.weight"]).to(torch.bfloat16))
    with torch.no_grad():
        model.decoder.lm_mixing.bias.fill_(0.25)
    eng.load_state_dict(dict(model.state_dict()))
    assert bool((eng.w["head_bias"] == 0.25).all())
    plain = GPT2DecoderEngine(_dec_cfg_dict(_joint_model(False).decoder.config), "cpu")
    plain.load_state_dict(dict(_joint_model(False).state_dict()))
    assert plain.w["taps"] is None and "head_fold" not in plain.w


def test_new_entries_are_declared_bound_and_built():
    from huggingface_asr_amd import _lib
    S = _lib.SIGNATURES
    assert len(S["mi_decoder_step_taps"]) == len(S["mi_decoder_step_beams"]) + 2          # the tap locations and their count
    assert len(S["mi_decoder_step_taps_workspace_bytes"]) == len(S["mi_gpt2_step_workspace_bytes"]) + 1
    header = open(os.path.join(ROOT, "include", "hfasr_hip.h")).read()
    assert re.search(r"\bint mi_decoder_step_taps\(", header) and re.search(r"\bsize_t mi_decoder_step_taps_workspace_bytes\(", header)
    for name in ("mi_decoder_step_taps", "mi_decoder_step_taps_workspace_bytes", "mi_decoder_step_beams", "mi_decoder_step", "mi_gpt2_step"):
        assert hasattr(_lib.lib(), name), name
    flat = lambda name: re.sub(r"\s+", " ", re.search(r"\bint " + name + r"\((.*?)\);", header, re.S).group(1))
    assert flat("mi_decoder_step_taps") == flat("mi_decoder_step_beams").replace("const float* head_bias, ", "const float* head_bias, const int* taps, int n_taps, ")
    c = _lib.Gpt2Config(d=128, H=2, L=3, V=51, eps=1e-5)
    L_ = _lib.lib()
    import ctypes as C
    assert L_.mi_decoder_step_taps_workspace_bytes(C.byref(c), 4, 1, 1) <= L_.mi_gpt2_step_workspace_bytes(C.byref(c), 4, 1)          # (no fused-form workspace: a taps call never takes that form)
    assert L_.mi_decoder_step_taps_workspace_bytes(C.byref(c), 4, 1, 3) > L_.mi_decoder_step_taps_workspace_bytes(C.byref(c), 4, 1, 1)


def test_restatement_reproduces_the_reference_fixture():
    """tests/golden/gen_tiny_mix.npz (tests/golden/make_gen_mix.py: the reference's own mixing decoder inside its joint model) against the fp32 restatement the GPU tests
    compare with: teacher-forced mixed logits at B = 2 with labels absent, `dec_loss` / `loss` at B = 1 (where the reference's loss is defined) and autograd's
    `d lm_mixing` there, greedy decode — so a GPU comparison with tests/mix_ref.py is a comparison with the reference"""
    import numpy as np
    from helpers import AED_JCFG, load_golden
    from huggingface_asr_amd import shapes
    from oracle import aed_ref as A
    from oracle import generate_ref as G
    import gen_model as GM
    torch.set_num_threads(8)
    g = load_golden("gen_tiny_mix")
    enc = dict(shapes.TINY, ctc_zero_infinity=True, ctc_loss_reduction="mean")
    lab = torch.from_numpy(g["labels"])
    for mode, avg in (("scalar", False), ("linear", False), ("full", False), (None, True)):
        tag = mode or "average"
        sd, x, am, dec_cfg = MR.mix_case_inputs(mode, avg)
        ids = torch.from_numpy(g[f"{tag}/ids"])
        esd = {k[len("encoder."):]: v for k, v in sd.items() if k.startswith("encoder.")}
        with torch.no_grad():
            hidden = A.E.encoder_forward(esd, enc, x, am, None)
            outer = A.E.conv_out_lengths_outer(am.sum(-1), enc).long()
            mask = torch.arange(hidden.shape[1])[None] < outer[:, None]
            enc_h = torch.nn.functional.linear(hidden, sd["enc_to_dec_proj.weight"], sd["enc_to_dec_proj.bias"]) if "enc_to_dec_proj.weight" in sd else hidden
            _, logits = MR.decoder_forward(sd, "decoder.", dec_cfg, ids, enc_h, mask)
        assert float((logits - torch.from_numpy(g[f"{tag}/logits"])).abs().max()) < 2e-3, tag
        with MR.patched():
            fn, nb = G.joint_score_fn(sd, enc, dec_cfg, AED_JCFG, x, am, 1, 0.3)
            seq = G.greedy(fn, nb, max_length=14, eos=GM.EOS, pad=GM.PAD, start=GM.START)
        want = g[f"{tag}/" + GM.setting_key(1, 1.0, False, 14) + "/sequences"]
        assert seq.shape == want.shape and (seq == want).all(), tag
        if mode is None:
            continue
        n = int(am[0].sum())
        leaf = {k: v.clone().requires_grad_("lm_mixing" in k) for k, v in sd.items()}
        with MR.patched():
            out = A.joint_forward(leaf, enc, dec_cfg, AED_JCFG, x[:1, :n], am[:1, :n], lab)
        for k in ("dec_loss", "loss", "enc_loss"):
            assert abs(float(out[k]) - float(g[f"{tag}/{k}"])) < 1e-4 * abs(float(g[f"{tag}/{k}"])), (tag, k, float(out[k]), float(g[f"{tag}/{k}"]))
        if mode in ("scalar", "linear"):
            out["dec_loss"].backward()
            got, ref = leaf["decoder.lm_mixing"].grad, torch.from_numpy(g[f"{tag}/dmix"])
            assert float((got - ref).abs().max()) < 1e-4 * float(ref.abs().max()), tag


def test_decoder_swap_through_the_launcher_on_the_reference_layout(tmp_path):
    """`python -m huggingface_asr_amd.launch <script>` on the stand-in of the reference's `src/` (tests/test_reference_route_cpu.py): a script that imports the names
    `model_utils.py` imports and runs the statements of its lines 205-217 receives the HIP classes — the mixing configuration by name from
    `models.decoders.multi_head_gpt2_mixing`, the decoder through the reference's `CustomModelForCausalLM` registry (resolved, not read from bind.py's text) — and ends with
    a HIP joint model whose only trainable parameters are `lm_mixing`."""
    import textwrap
    from test_reference_route_cpu import _reference_layout, _run
    src = _reference_layout(tmp_path / "src")
    script = tmp_path / "swap_like_model_utils.py"
    script.write_text(textwrap.dedent('''
        import sys
        from models.auto_wrappers import CustomModelForCausalLM
        from models.decoders.multi_head_gpt2 import GPT2LMMultiHeadModel
        from models.decoders.multi_head_gpt2_mixing import GPT2LMMultiHeadModelMixing, GPT2MultiHeadMixingConfig
        from utilities.bind import bind_all
        if __name__ == "__main__":
            bind_all()
            sys.path.insert(0, sys.argv[1])
            from test_surface_cpu import _joint_model
            model = _joint_model(False)
            if not isinstance(model.decoder, GPT2LMMultiHeadModel):
                raise ValueError("The model decoder must be an instance of GPT2LMMultiHeadModel")
            old_config = model.decoder.config
            new_config = GPT2MultiHeadMixingConfig(**old_config.to_dict(), mixing_mode=sys.argv[2])
            new_decoder = CustomModelForCausalLM.registry[type(new_config)](new_config)          # the stand-in registry's `from_config`
            new_decoder.load_state_dict(model.decoder.state_dict(), strict=False)
            model.decoder = new_decoder
            for name, param in model.named_parameters():
                if "lm_mixing" not in name:
                    param.requires_grad = False
            print("CLASSES", type(model).__module__, type(model.decoder).__module__, type(model.decoder).__name__, type(new_decoder) is GPT2LMMultiHeadModelMixing,
                  type(model.config.decoder).__module__)
            print("TRAINABLE", sorted(n for n, p in model.named_parameters() if p.requires_grad))
    '''))
    r = _run(["-m", "huggingface_asr_amd.launch", "--reference-src", src, str(script), os.path.join(ROOT, "tests"), "scalar"])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert "CLASSES huggingface_asr_amd.modeling_joint huggingface_asr_amd.modeling_joint GPT2LMMultiHeadModelMixing True huggingface_asr_amd.modeling_joint" in r.stdout
    assert "TRAINABLE ['decoder.lm_mixing']" in r.stdout
