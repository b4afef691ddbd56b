"""CPU: the reference's model-instantiation code lands on the HIP classes after `bind.install()`.

The reference's `src/utilities/model_utils.py` imports `JointCTCAttentionEncoderDecoder{,Config}` by name and builds them directly (:193, :199), so swapping
`bind_all` alone is not enough.  The reference's sources are not part of this repository, so these tests run on a stand-in `src/` tree written into a temporary
directory: the module paths and class names `bind.install()` rebinds (bind.REBIND), a `utilities/model_utils.py` that imports them by name as the reference's does,
`utilities/bind.py` and the `models/auto_wrappers.py` decoder registry.  The scenarios run in a subprocess (they edit sys.modules / the Auto registry)."""
import os
import subprocess
import sys
import textwrap

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

# what the stand-in model_utils imports by name (model_utils.py:30-33 and the classes it builds the CTC / decoder models from)
_MODEL_UTILS = textwrap.dedent('''
    from models.ctc_encoder_plus_autoregressive_decoder import JointCTCAttentionEncoderDecoder, JointCTCAttentionEncoderDecoderConfig
    from models.decoders.multi_head_gpt2 import GPT2LMMultiHeadModel, GPT2MultiHeadConfig
    from models.encoders.e_branchformer import Wav2Vec2EBranchformerForCTC
    from utilities.bind import bind_all


    def joint_class():
        return JointCTCAttentionEncoderDecoder          # a module global, read at call time
''')


def _reference_layout(root):
    """A stand-in for the reference's src/: every module of bind.REBIND with a placeholder class per rebound name, plus the modules install() reaches for."""
    from huggingface_asr_amd import bind
    files = {m: "".join(f"class {n}:\n    pass\n\n\n" for n in names) for m, names in bind.REBIND.items()}
    files["models.encoders.e_branchformer"] += "class Wav2Vec2EBranchformerForPreTraining:\n    pass\n"     # not built on the HIP path: stays reachable
    files["models.auto_wrappers"] = textwrap.dedent('''
        class CustomModelForCausalLM:
            registry = {}

            @classmethod
            def register(cls, config_class, model_class, exist_ok=False):
                cls.registry[config_class] = model_class
    ''')
    files["utilities.bind"] = "def bind_all():\n    raise RuntimeError('the reference bind_all ran')\n"
    files["utilities.model_utils"] = _MODEL_UTILS
    for mod, text in files.items():
        parts = mod.split(".")
        for i in range(1, len(parts)):
            pkg = os.path.join(root, *parts[:i])
            os.makedirs(pkg, exist_ok=True)
            open(os.path.join(pkg, "__init__.py"), "a").close()
        with open(os.path.join(root, *parts) + ".py", "w") as f:
            f.write(text)
    return str(root)


_INSTALL_SCRIPT = textwrap.dedent('''
    import importlib
    import sys
    sys.path.insert(0, sys.argv[1])
    from transformers import AutoModelForCTC, AutoModelForPreTraining, AutoModelForSpeechSeq2Seq
    from huggingface_asr_amd import bind
    from huggingface_asr_amd.configuration_ebranchformer import Wav2Vec2EBranchformerConfig
    from huggingface_asr_amd.modeling_ebranchformer import Wav2Vec2EBranchformerForCTC
    from huggingface_asr_amd.modeling_joint import GPT2LMMultiHeadModel, GPT2MultiHeadConfig, JointCTCAttentionEncoderDecoder, JointCTCAttentionEncoderDecoderConfig
    if sys.argv[2] == "import_first":      # what a trainer does: `from utilities.model_utils import ...` at module top, bind_all() later in main()
        import utilities.model_utils as MU
        assert MU.JointCTCAttentionEncoderDecoder is not JointCTCAttentionEncoderDecoder
        bind.install()
    else:                                  # what `python -m huggingface_asr_amd.launch` does: install() before the script is executed
        bind.install()
        import utilities.model_utils as MU
    for modname, names in bind.REBIND.items():
        mod = importlib.import_module(modname)
        for attr, ours in names.items():
            assert getattr(mod, attr) is ours, (modname, attr)
    assert MU.JointCTCAttentionEncoderDecoder is JointCTCAttentionEncoderDecoder and MU.joint_class() is JointCTCAttentionEncoderDecoder
    assert MU.JointCTCAttentionEncoderDecoderConfig is JointCTCAttentionEncoderDecoderConfig
    assert MU.GPT2LMMultiHeadModel is GPT2LMMultiHeadModel and MU.GPT2MultiHeadConfig is GPT2MultiHeadConfig
    assert MU.Wav2Vec2EBranchformerForCTC is Wav2Vec2EBranchformerForCTC
    import utilities.bind as RB
    assert RB.bind_all is bind.bind_all and MU.bind_all is bind.bind_all
    MU.bind_all()                          # what the trainers call (train_enc_dec_asr.py:39)
    import models.auto_wrappers as AW
    import models.encoders.e_branchformer as REB
    assert AW.CustomModelForCausalLM.registry[GPT2MultiHeadConfig] is GPT2LMMultiHeadModel
    assert AutoModelForSpeechSeq2Seq._model_mapping[JointCTCAttentionEncoderDecoderConfig] is JointCTCAttentionEncoderDecoder
    assert AutoModelForCTC._model_mapping[Wav2Vec2EBranchformerConfig] is Wav2Vec2EBranchformerForCTC
    assert AutoModelForPreTraining._model_mapping[Wav2Vec2EBranchformerConfig] is REB.Wav2Vec2EBranchformerForPreTraining
    print("ALL OK")
''')


def _run(args, cwd=ROOT):
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1", PYTHONPATH=ROOT)
    return subprocess.run([sys.executable, *args], cwd=cwd, env=env, capture_output=True, text=True, timeout=600)


@pytest.mark.parametrize("order", ["import_first", "install_first"])
def test_install_rebinds_names_the_reference_layout_imports(tmp_path, order):
    src = _reference_layout(tmp_path / "src")
    r = _run(["-c", _INSTALL_SCRIPT, src, order])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "ALL OK" in r.stdout


def test_launcher_runs_a_script_on_the_hip_classes(tmp_path):
    """`python -m huggingface_asr_amd.launch <script>`: the script's own `from ... import` lines receive the HIP classes and our bind_all."""
    src = _reference_layout(tmp_path / "src")
    script = tmp_path / "trainer_like.py"
    script.write_text(textwrap.dedent('''
        import sys
        from utilities.bind import bind_all
        from models.ctc_encoder_plus_autoregressive_decoder import JointCTCAttentionEncoderDecoder, JointCTCAttentionEncoderDecoderConfig
        from models.encoders.e_branchformer import Wav2Vec2EBranchformerForCTC
        from models.decoders.multi_head_gpt2 import GPT2LMMultiHeadModel
        if __name__ == "__main__":
            bind_all()
            from transformers import AutoModelForSpeechSeq2Seq
            print("ARGV", sys.argv[1:])
            print("CLASSES", JointCTCAttentionEncoderDecoder.__module__, Wav2Vec2EBranchformerForCTC.__module__, GPT2LMMultiHeadModel.__module__, bind_all.__module__)
            print("AUTO", AutoModelForSpeechSeq2Seq._model_mapping[JointCTCAttentionEncoderDecoderConfig].__module__)
    '''))
    r = _run(["-m", "huggingface_asr_amd.launch", "--reference-src", src, str(script), "--flag=1"])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert "ARGV ['--flag=1']" in r.stdout
    assert "CLASSES huggingface_asr_amd.modeling_joint huggingface_asr_amd.modeling_ebranchformer huggingface_asr_amd.modeling_joint huggingface_asr_amd.bind" in r.stdout
    assert "AUTO huggingface_asr_amd.modeling_joint" in r.stdout


def test_from_encoder_decoder_pretrained_kwarg_routing(tmp_path):
    """no reference needed: encoder_/decoder_ prefixes go to the sub-configs, the rest to the joint config (reference :138-235)"""
    from huggingface_asr_amd import shapes
    from huggingface_asr_amd.bind import bind_all
    from huggingface_asr_amd.configuration_ebranchformer import Wav2Vec2EBranchformerConfig
    from huggingface_asr_amd.modeling_ebranchformer import Wav2Vec2EBranchformerForCTC
    from huggingface_asr_amd.modeling_joint import GPT2LMMultiHeadModel, GPT2MultiHeadConfig, JointCTCAttentionEncoderDecoder
    bind_all()
    base = dict(shapes.TINY); base.pop("num_fbanks")
    enc = Wav2Vec2EBranchformerForCTC(Wav2Vec2EBranchformerConfig(**base))
    dec = GPT2LMMultiHeadModel(GPT2MultiHeadConfig(vocab_size=base["vocab_size"], n_embd=32, n_layer=1, n_head=2, n_positions=32, lsm_factor=0.0, pos_emb_fixed=False,
                                                   add_cross_attention=True, is_decoder=True))
    enc.save_pretrained(tmp_path / "e"); dec.save_pretrained(tmp_path / "d")
    m = JointCTCAttentionEncoderDecoder.from_encoder_decoder_pretrained(str(tmp_path / "e"), str(tmp_path / "d"), encoder_layerdrop=0.0, decoder_lsm_factor=0.2,
                                                                        ctc_weight=0.25, decoder_start_token_id=1, pad_token_id=3)
    assert m.config.ctc_weight == 0.25 and m.config.decoder_start_token_id == 1 and m.config.pad_token_id == 3
    assert m.config.decoder.lsm_factor == 0.2 and m.lsm_factor == 0.2 and m.config.encoder.layerdrop == 0.0
    assert m.enc_loss_weight == 0.25 and abs(m.dec_loss_weight - 0.75) < 1e-12
    assert hasattr(m, "enc_to_dec_proj")                      # 64 -> 32
    with pytest.raises(ValueError):
        JointCTCAttentionEncoderDecoder.from_encoder_decoder_pretrained(None, str(tmp_path / "d"))
    with pytest.raises(TypeError):                            # a torch decoder is refused: no silent PyTorch fallback
        from transformers import GPT2Config, GPT2LMHeadModel
        JointCTCAttentionEncoderDecoder(encoder=enc, decoder=GPT2LMHeadModel(GPT2Config(n_layer=1, n_embd=32, n_head=2, vocab_size=50)))
