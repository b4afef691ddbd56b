"""CPU: the semantics of CTC greedy transcription and the Python surfaces around the device kernels (csrc/ctc_decode.hip).

tests/golden/ctc_greedy.npz holds seeded logits and what the reference's ctc_greedy_decode (src/utilities/eval_utils.py:37-43) returned for them
(tests/golden/make_ctc_greedy.py); tests/ctc_greedy_ref.py is our restatement, which the GPU tests hold the kernels to."""
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import ctc_greedy_ref as R  # noqa: E402

CASES = ["random", "blank_dominated", "all_blank_row", "single_token_row", "exact_ties", "blank_not_last"]


load_case = R.load_case


def test_fixture_holds_the_cases(golden_dir):
    d = np.load(os.path.join(golden_dir, "ctc_greedy.npz"))
    assert sorted({k.split(".")[0] for k in d.files} - {"meta"}) == sorted(CASES) == R.CASES and d["meta"].shape == (len(CASES), 2)
    x, blank, _, ids = load_case(golden_dir, "all_blank_row")
    assert (ids[1] == 1).all() and (ids[0] != 1).any()                    # one utterance decodes to nothing but padding
    x, blank, _, ids = load_case(golden_dir, "single_token_row")
    assert ids[0, 0] == 17 and (ids[0, 1:] == 0).all()
    x, blank, _, _ = load_case(golden_dir, "exact_ties")
    assert torch.equal(x[..., 7], x[..., 30]) and torch.equal(x[..., 12], x[..., blank])
    assert load_case(golden_dir, "blank_not_last")[1] != x.shape[-1] - 1


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_the_reference(golden_dir, name):
    x, blank, pad, ids = load_case(golden_dir, name)
    r = R.greedy(x, blank, pad)
    assert np.array_equal(r["tokens"], ids)
    for b in range(x.shape[0]):                                           # frames: where each kept token starts
        n = r["n_tokens"][b]
        assert (ids[b, n:] == pad).all() and (r["best"][b, r["frames"][b, :n]] != blank).all()
        assert np.array_equal(r["best"][b, r["frames"][b, :n]], r["tokens"][b, :n]) and (r["frames"][b, n:] == -1).all()
        assert (np.diff(r["frames"][b, :n]) > 0).all()


def test_restatement_lengths_cut_frames():
    best = np.array([[3, 3, 9, 3, 3, 4, 9, 4], [9, 9, 9, 9, 9, 9, 9, 9], [1, 2, 3, 4, 5, 6, 7, 8]])
    tok, n, fr = R.collapse(best, blank=9, pad_id=-7, lengths=[5, 8, 0])
    assert tok.tolist() == [[3, 3] + [-7] * 6, [-7] * 8, [-7] * 8] and n.tolist() == [2, 0, 0]
    assert fr[0].tolist() == [0, 3] + [-1] * 6
    tok, n, _ = R.collapse(best, blank=9, pad_id=-7)
    assert tok[0].tolist() == [3, 3, 4, 4, -7, -7, -7, -7] and n.tolist() == [4, 0, 8]


def test_argmax_rules_of_the_restatement():
    x = torch.tensor([[[1.0, 5.0, 5.0, 2.0], [float("-inf")] * 4, [1.0, float("nan"), 7.0, float("nan")], [float("inf"), 1.0, float("nan"), 0.0]]])
    assert R.argmax_frames(x).tolist() == [[1, 0, 1, 2]]


def test_cpu_tensors_are_refused():
    from huggingface_asr_amd import decoding, ops
    x = torch.zeros(1, 4, 5)
    with pytest.raises(RuntimeError, match="device tensor"):
        decoding.ctc_greedy_decode(x, 4, 0)
    with pytest.raises(RuntimeError):
        ops.ctc_greedy_decode(x, 4, 0)
    with pytest.raises(RuntimeError):
        ops.row_argmax(x[0])


def test_transcribe_argument_errors():
    from huggingface_asr_amd import shapes
    from huggingface_asr_amd.configuration_ebranchformer import Wav2Vec2EBranchformerConfig
    from huggingface_asr_amd.engine import EBranchformerEngine
    from huggingface_asr_amd.modeling_ebranchformer import Wav2Vec2EBranchformerForCTC
    base = dict(shapes.TINY); base.pop("num_fbanks")
    model = Wav2Vec2EBranchformerForCTC(Wav2Vec2EBranchformerConfig(**base))
    x = torch.zeros(1, 100, 80)
    model.eval()
    with pytest.raises(ValueError, match="span"):
        model.transcribe(x, span="outer")
    model.train()
    with pytest.raises(RuntimeError, match="eval"):
        model.transcribe(x)
    model.eval()
    with pytest.raises(RuntimeError, match="GPU"):                         # a CPU tensor, as in forward()
        model.transcribe(x)
    eng = EBranchformerEngine(dict(shapes.TINY), "cpu")
    with pytest.raises(ValueError, match="span"):
        eng.transcribe(x, span="inner")


# ---------------------------------------------------------------- bind.install() also swaps the reference's ctc_greedy_decode
_EVAL_UTILS = "def ctc_greedy_decode(logits, blank, pad_token_id):\n    raise RuntimeError('the reference ctc_greedy_decode ran')\n\n\ndef compute_metrics_ctc(*a):\n    return {}\n"
_TRAINER = textwrap.dedent('''
    from utilities.eval_utils import compute_metrics_ctc, ctc_greedy_decode


    def preprocess():
        return ctc_greedy_decode                 # a module global, read at call time (train_ctc_asr.py:83)
''')


def _reference_layout(root):
    """a stand-in for the reference's src/ (its sources are not part of this repository): what install() reaches for, plus utilities/eval_utils.py with a placeholder
    function and a trainer-shaped module importing it by name"""
    from huggingface_asr_amd import bind
    files = {m: "".join(f"class {n}:\n    pass\n\n\n" for n in names) for m, names in bind.REBIND.items()}
    files["models.auto_wrappers"] = "class CustomModelForCausalLM:\n    registry = {}\n\n    @classmethod\n    def register(cls, c, m, exist_ok=False):\n        cls.registry[c] = m\n"
    files["utilities.bind"] = "def bind_all():\n    raise RuntimeError('the reference bind_all ran')\n"
    files["utilities.eval_utils"] = _EVAL_UTILS
    files["trainers.train_ctc_like"] = _TRAINER
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
    import sys
    sys.path.insert(0, sys.argv[1])
    from huggingface_asr_amd import bind, decoding
    if sys.argv[2] == "import_first":
        import trainers.train_ctc_like as TR
        from utilities.eval_utils import ctc_greedy_decode       # held by __main__ under its own name, as a trainer run as a script holds it
        assert TR.ctc_greedy_decode is not decoding.ctc_greedy_decode
        bind.install()
        assert ctc_greedy_decode is decoding.ctc_greedy_decode, "__main__ keeps the reference function"
    else:
        bind.install()
        import trainers.train_ctc_like as TR
    import utilities.eval_utils as EU
    assert EU.ctc_greedy_decode is decoding.ctc_greedy_decode
    assert TR.ctc_greedy_decode is decoding.ctc_greedy_decode and TR.preprocess() is decoding.ctc_greedy_decode
    assert TR.compute_metrics_ctc is EU.compute_metrics_ctc and EU.compute_metrics_ctc.__module__ == "utilities.eval_utils"      # nothing else is touched
    assert "utilities.eval_utils" not in bind.REBIND
    bind.install()                                               # idempotent
    assert TR.ctc_greedy_decode is decoding.ctc_greedy_decode
    print("ALL OK")
''')


@pytest.mark.parametrize("order", ["import_first", "install_first"])
def test_install_rebinds_ctc_greedy_decode(tmp_path, order):
    src = _reference_layout(tmp_path / "src")
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1", PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-c", _INSTALL_SCRIPT, src, order], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "ALL OK" in r.stdout


def test_install_skips_an_eval_utils_that_cannot_be_imported(tmp_path):
    src = _reference_layout(tmp_path / "src")
    with open(os.path.join(src, "utilities", "eval_utils.py"), "w") as f:
        f.write("import a_package_that_is_not_installed_anywhere\n")
    code = "import sys; sys.path.insert(0, sys.argv[1]); from huggingface_asr_amd import bind; bind.install(); print('ALL OK')"
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1", PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-c", code, src], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ALL OK" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
