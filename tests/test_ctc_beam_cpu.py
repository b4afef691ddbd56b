"""CPU: CTC prefix beam search — the float64 restatement (tests/ctc_beam_ref.py) against the enumeration of every alignment, that the search finds better answers than
the greedy collapse, what the Python surfaces refuse on the host, the opt-in binding, and the budgets of the two kernels of csrc/ctc_beam.hip in the built code object."""
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import ctc_beam_ref as R  # noqa: E402
from test_ctc_decode_cpu import _reference_layout  # noqa: E402

SMALL = [(1, 3), (2, 3), (5, 3), (3, 4)]
DRAWS = 30


def small_logits(T, V1, seed):
    return np.random.default_rng(1000 * T + 100 * V1 + seed).standard_normal((T, V1)).astype(np.float32)


@pytest.mark.parametrize("T,V1", SMALL)
def test_restatement_equals_the_enumeration(T, V1):
    blank = V1 - 1
    for seed in range(DRAWS):
        x = small_logits(T, V1, seed)
        lp = R.log_softmax(x)
        want = R.brute_force(lp, blank)[:8]
        got = R.beam_search(x, blank, 64, V1 - 1, nbest=8)["hyps"]
        assert [h[0] for h in got] == [w[0] for w in want], (T, V1, seed)
        for (labels, score, frames), (_, exact) in zip(got, want):
            assert abs(score - exact) <= 1e-9 and abs(score - R.ctc_logp(lp, labels, blank)) <= 1e-9, (T, V1, seed, labels)
            assert len(frames) == len(labels) and all(a < b for a, b in zip(frames, frames[1:])) and all(0 <= f < T for f in frames)


def test_enumeration_and_forward_recursion_agree_and_sum_to_one():
    x = small_logits(5, 3, 99)
    lp = R.log_softmax(x)
    every = R.brute_force(lp, 2)
    assert abs(sum(np.exp(s) for _, s in every) - 1.0) < 1e-12
    for labels, s in every:
        assert abs(R.ctc_logp(lp, labels, 2) - s) < 1e-9
    assert R.ctc_logp(lp, (0, 0, 0, 0), 2) == float("-inf")               # needs 7 frames
    assert R.beam_search(x, 2, 4, nbest=2, length=0)["hyps"] == [((), 0.0, [])]


def test_beam_answers_differ_from_greedy_and_are_better():
    better = 0
    for T, V1 in SMALL[2:]:
        for seed in range(DRAWS):
            x = small_logits(T, V1, seed)
            lp = R.log_softmax(x)
            best = R.beam_search(x, V1 - 1, 64, V1 - 1)["hyps"][0][0]
            g = R.greedy(x, V1 - 1)
            if best != g:
                assert R.ctc_logp(lp, best, V1 - 1) > R.ctc_logp(lp, g, V1 - 1)
                better += 1
    assert better >= 5, better


def test_margins_see_a_narrow_cut():
    x = np.zeros((2, 4), dtype=np.float32)
    x[0] = [1.0, 0.5, 0.5 - 1e-4, 0.0]                                     # blank 3: the token cut at K = 2 is 1e-4 wide
    x[1] = [3.0, 2.0, 1.0, 0.0]
    r = R.beam_search(x, 3, 2, 2, nbest=2)
    assert abs(r["margins"]["token_cut"] - 1e-4) < 1e-6 and r["margins"]["beam_cut"] < float("inf") and len(r["margins"]["final"]) == 1
    assert R.token_cut([0.0, 2.0, 2.0, 9.0], 3, 2)[0] == [1, 2]            # equal values: the lower class first; the blank never


def test_host_side_refusals():
    from huggingface_asr_amd import decoding, ops

    class Tok:
        pad_token_id = 0
    x = torch.zeros(2, 6, 5)
    with pytest.raises(RuntimeError):
        ops.ctc_beam_decode(x, 4, 0, beams=4)
    with pytest.raises(RuntimeError, match="device tensor"):
        decoding.ctc_beam_decode(x, None, Tok(), 5)
    with pytest.raises(RuntimeError):
        ops.ctc_beam_cut(x, 4, 2)
    for kw in (dict(beams=0), dict(beams=65), dict(beams=4, nbest=5), dict(beams=4, nbest=0), dict(beams=4, token_topk=0), dict(beams=4, token_topk=65)):
        with pytest.raises(ValueError):
            ops.ctc_beam_decode(x, 4, 0, **kw)
    with pytest.raises(TypeError):
        ops.ctc_beam_decode(x[0], 4, 0, beams=4)                           # not 3-D
    with pytest.raises(TypeError):
        decoding.ctc_beam_decode(x[0], None, Tok(), 5)
    with pytest.raises(TypeError):
        ops.ctc_beam_decode(x, 4, 0, beams=4.0)
    with pytest.raises(TypeError):
        ops.ctc_beam_decode(x, 4, 0, beams=4, dtype=torch.int16)
    with pytest.raises(TypeError):
        ops.ctc_beam_decode(x, 4, 0)                                       # beams is required


def test_c_entries_refuse_bad_arguments_before_any_launch():
    """MI_ERR_ARG comes back from argument checks alone: no device is needed (and none is here)"""
    from huggingface_asr_amd import _lib
    L = _lib.lib()
    buf = (_lib.C.c_char * 4096)()
    p = _lib.C.addressof(buf)
    cut = lambda V1, blank, K: L.mi_ctc_beam_cut(p, 8, 64, 0, 1, 4, V1, None, blank, K, p, p, p, p, None)
    walk = lambda V1, blank, W, K, nbest: L.mi_ctc_beam_walk(p, 8, 64, 0, 1, 4, V1, None, blank, 0, W, K, nbest, p, p, p, p, p, 1 << 30, p, 1, p, p, None, None)
    for args in ((1, 0, 1), (5, 5, 2), (5, -1, 2), (5, 4, 0), (5, 4, 65)):
        assert cut(*args) == _lib.ERR_ARG, args
    for args in ((1, 0, 1, 1, 1), (5, 5, 4, 2, 1), (5, 4, 0, 2, 1), (5, 4, 65, 2, 1), (5, 4, 4, 0, 1), (5, 4, 4, 65, 1), (5, 4, 4, 2, 5), (5, 4, 4, 2, 0)):
        assert walk(*args) == _lib.ERR_ARG, args
    assert L.mi_ctc_beam_workspace_bytes(32, 250, 64) >= 32 * (1 + 250 * 64) * 24
    assert L.mi_ctc_beam_workspace_bytes(1, 250, 65) == 0 and L.mi_ctc_beam_workspace_bytes(1, 250, 0) == 0


def test_transcribe_with_beams_refuses_on_the_host():
    from huggingface_asr_amd import shapes
    from huggingface_asr_amd.engine import EBranchformerEngine
    eng = EBranchformerEngine(dict(shapes.TINY), "cpu")
    with pytest.raises(ValueError, match="span"):
        eng.transcribe(torch.zeros(1, 100, 80), span="inner", beams=4)
    with pytest.raises(RuntimeError):                                      # no weights, a CPU tensor: as without beams
        eng.transcribe(torch.zeros(1, 100, 80), beams=4)


# ---------------------------------------------------------------- bind.install() swaps ctc_beam_decode only on request
_EVAL_UTILS = ("def ctc_greedy_decode(logits, blank, pad_token_id):\n    raise RuntimeError('the reference ctc_greedy_decode ran')\n\n\n"
               "def ctc_beam_decode(logits, _, tokenizer, beam_size):\n    raise RuntimeError('the reference ctc_beam_decode ran')\n")
_INSTALL_SCRIPT = '''
import sys
sys.path.insert(0, sys.argv[1])
from huggingface_asr_amd import bind, decoding
from utilities.eval_utils import ctc_beam_decode, ctc_greedy_decode      # held by __main__ under their own names, as a trainer run as a script holds them
import utilities.eval_utils as EU
ref = EU.ctc_beam_decode
bind.install()
assert EU.ctc_greedy_decode is decoding.ctc_greedy_decode and ctc_greedy_decode is decoding.ctc_greedy_decode
if sys.argv[2] == "on":
    assert EU.ctc_beam_decode is decoding.ctc_beam_decode, "the defining module keeps the reference function"
    assert ctc_beam_decode is decoding.ctc_beam_decode, "__main__ keeps the reference function"
else:
    assert EU.ctc_beam_decode is ref and ctc_beam_decode is ref and ref.__module__ == "utilities.eval_utils"
assert "ctc_beam_decode" not in bind.REBIND_FUNCTIONS["utilities.eval_utils"]
bind.install()                                                           # idempotent
assert (EU.ctc_beam_decode is decoding.ctc_beam_decode) == (sys.argv[2] == "on")
print("ALL OK")
'''


@pytest.mark.parametrize("switch", ["off", "on", "other_value"])
def test_install_rebinds_ctc_beam_decode_only_on_request(tmp_path, switch):
    src = _reference_layout(tmp_path / "src")
    with open(os.path.join(src, "utilities", "eval_utils.py"), "w") as f:
        f.write(_EVAL_UTILS)
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1", PYTHONPATH=ROOT)
    env.pop("HFASR_CTC_BEAM", None)
    if switch != "off":
        env["HFASR_CTC_BEAM"] = "1" if switch == "on" else "0"
    r = subprocess.run([sys.executable, "-c", _INSTALL_SCRIPT, src, "on" if switch == "on" else "off"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "ALL OK" in r.stdout


# ---------------------------------------------------------------- the built kernels
def test_new_kernels_use_no_scratch_and_the_lds_their_header_states():
    from huggingface_asr_amd import _lib
    _lib.lib()
    header = open(os.path.join(ROOT, "huggingface_asr_amd", "csrc", "ctc_beam.hip")).read()
    stated = {k: int(re.search(r"//\s+" + k + r"\s.*?(\d+) B of LDS", header).group(1)) for k in ("ctc_cut_kernel", "ctc_walk_kernel")}
    assert stated == {"ctc_cut_kernel": 34352, "ctc_walk_kernel": 44576}
    so = os.path.join(ROOT, "huggingface_asr_amd", "libhfasr_hip.so")
    llvm = "/opt/rocm/lib/llvm/bin"
    found = {}
    magic = b"__CLANG_OFFLOAD_BUNDLE__"
    with tempfile.TemporaryDirectory() as td:
        fb, co = os.path.join(td, "lib.fatbin"), os.path.join(td, "lib.co")
        subprocess.run([os.path.join(llvm, "llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", so, fb], check=True)
        blob = open(fb, "rb").read()                                       # one bundle per translation unit, back to back
        starts = [m.start() for m in re.finditer(re.escape(magic), blob)]
        for lo, hi in zip(starts, starts[1:] + [len(blob)]):
            if b"ctc_walk_kernel" not in blob[lo:hi]:
                continue
            with open(fb, "wb") as f:
                f.write(blob[lo:hi])
            subprocess.run([os.path.join(llvm, "clang-offload-bundler"), "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--input={fb}",
                            f"--output={co}"], check=True)
            notes = subprocess.run([os.path.join(llvm, "llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout
            for block in notes.split("- .agpr_count")[1:]:
                name = re.search(r"\.name:\s+(\S*(ctc_cut_kernel|ctc_walk_kernel)\S*)", block)
                if name:
                    num = lambda key: int(re.search(r"\." + key + r":\s+(\d+)", block).group(1))
                    found[name.group(1)] = (name.group(2), num("private_segment_fixed_size"), num("group_segment_fixed_size"), num("vgpr_count"))
    assert len(found) == 4, sorted(found)                                  # fp32 and bf16 rows; int32 and int64 tokens
    for name, (kind, scratch, lds, vgprs) in found.items():
        assert scratch == 0, (name, scratch)
        assert lds == stated[kind] and vgprs <= 128, (name, lds, vgprs)
