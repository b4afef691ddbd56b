"""CPU: the CTC prefix beam search on a stream — the suspended float64 restatement (tests/ctc_beam_stream_ref.py) against the one-shot one (tests/ctc_beam_ref.py) for
every way of splitting the frames into calls, the committed prefix's properties, the state-size formula, the declarations, what the Python surfaces refuse on the
host, and the budget of csrc/ctc_beam_stream.hip's kernel in the built code object."""
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
import ctc_beam_stream_ref as S  # noqa: E402

ENUMERABLE = [(5, 3), (6, 4)]


def _logits(T, V1, seed):
    return np.random.default_rng(5000 + 100 * T + 10 * V1 + seed).standard_normal((T, V1)).astype(np.float32)


def _plain(hyps):
    return [(labels, score, list(frames)) for labels, score, frames in hyps]


# ---------------------------------------------------------------- the suspended restatement
@pytest.mark.parametrize("T,V1", ENUMERABLE)
@pytest.mark.parametrize("W", [2, 64])                                     # a beam that prunes at every frame, and one that never does
def test_suspended_restatement_equals_the_one_shot_one_for_every_composition(T, V1, W):
    """after EVERY call of EVERY composition: the same hypotheses in the same order (ranks), the same float64 scores, the same entry frames"""
    comps = S.compositions(T)
    assert len(comps) == sum(1 + len(c) + 1 for c in comps if 0 not in c) and [T] in comps and [1] * T in comps and [0, T] in comps
    for seed in range(3):
        x = _logits(T, V1, seed)
        want = [_plain(R.beam_search(x[:n], V1 - 1, W, V1 - 1, nbest=W, length=n)["hyps"]) for n in range(T + 1)]
        for parts in comps:
            st, t = S.BeamStream(V1 - 1, W, V1 - 1), 0
            for j, n in enumerate(parts):
                st.feed(x[t:t + n], final=j == len(parts) - 1)
                t += n
                assert _plain(st.hyps()) == want[t], (seed, parts, j)
            assert t == T and st.committed == want[T][0][0] and st.committed_frames == want[T][0][2]


def test_zero_frames_in_total_is_the_empty_hypothesis_with_score_zero():
    st = S.BeamStream(2, 4)
    assert st.feed(np.zeros((0, 3)), final=True) == 0
    assert st.hyps() == [((), 0.0, [])] and st.committed == ()


# ---------------------------------------------------------------- the committed prefix
def _committed_trace(x, blank, W, K, parts):
    st, t, trace = S.BeamStream(blank, W, K), 0, []
    for j, n in enumerate(parts):
        new = st.feed(x[t:t + n], final=j == len(parts) - 1)
        t += n
        trace.append(dict(new=new, committed=st.committed, frames=list(st.committed_frames), best=st.hyps(1)[0], every=[h[0] for h in st.hyps()]))
    return trace


def _check_trace(trace):
    for j, now in enumerate(trace):
        before = trace[j - 1]["committed"] if j else ()
        assert now["committed"][:len(before)] == before and now["new"] == len(now["committed"]) - len(before)       # append-only, monotone
        if j < len(trace) - 1:
            assert now["committed"] == S.lcp(now["every"])
        for later in trace[j:]:
            assert later["best"][0][:len(now["committed"])] == now["committed"]                                    # a prefix of every later best hypothesis
            assert later["best"][2][:len(now["frames"])] == now["frames"]
    assert trace[-1]["committed"] == trace[-1]["best"][0] and trace[-1]["frames"] == trace[-1]["best"][2]           # after final: the best hypothesis


def test_committed_prefix_is_monotone_a_prefix_of_every_later_best_and_the_best_after_final():
    for T, V1 in ENUMERABLE:
        for seed in range(6):
            for W in (2, 3):
                _check_trace(_committed_trace(_logits(T, V1, seed), V1 - 1, W, V1 - 1, [1] * T))
                _check_trace(_committed_trace(_logits(T, V1, seed), V1 - 1, W, V1 - 1, [2, 0, T - 2]))
    for seed in range(4):
        _check_trace(_committed_trace(R.peaky(20 + seed, 32, 12, 11), 11, 8, 8, S.chunks(32, 5)))


def test_planted_case_commits_in_steps_and_lags_the_best_hypothesis():
    """the inputs of the GPU committed-prefix test: so that it cannot pass vacuously, the committed prefix here is, at some non-final call, neither empty nor whole,
    and at some call shorter than the best hypothesis"""
    c = S.PLANTED
    trace = _committed_trace(S.planted_logits(), c["V1"] - 1, c["W"], c["K"], S.chunks(c["T"], c["chunk"]))
    _check_trace(trace)
    final_len = len(trace[-1]["committed"])
    assert any(0 < len(t["committed"]) < final_len for t in trace[:-1])
    assert any(len(t["committed"]) < len(t["best"][0]) for t in trace)
    assert len({len(t["committed"]) for t in trace}) >= 4                  # it grows in several steps
    assert S.lcp([]) == () and S.lcp([(1, 2, 3), (1, 2), (1, 2, 4)]) == (1, 2) and S.lcp([(1,), (2,)]) == ()


# ---------------------------------------------------------------- the C entries without a device
def _table_words(T, W):
    h = 2
    while h < 2 * (1 + T * W):
        h <<= 1
    return h


def test_state_bytes_match_the_documented_formula_and_need_no_device():
    from huggingface_asr_amd import _lib
    f = _lib.lib().mi_ctc_beam_stream_state_bytes
    align16 = lambda v: (v + 15) // 16 * 16
    for B, M, W in ((1, 1, 1), (3, 48, 4), (2, 1040, 64), (32, 1500, 10), (7, 333, 5)):
        assert f(B, M, W) == B * (64 + 7 * 64 * 4) + align16(16 * B * (1 + M * W)) + 8 * B * _table_words(M, W), (B, M, W)
    assert f(1, 65535, 64) > 0 and f(1, 65536, 64) == 0                    # max_frames W < 2^22 - 2
    for bad in ((0, 10, 4), (1, 0, 4), (1, 10, 0), (1, 10, 65), (-1, 10, 4)):
        assert f(*bad) == 0, bad


def test_c_entries_refuse_bad_arguments_before_any_launch():
    from huggingface_asr_amd import _lib
    L = _lib.lib()
    buf = (_lib.C.c_char * 8192)()
    p = (_lib.C.addressof(buf) + 15) // 16 * 16

    def walk(V1=5, blank=4, W=4, K=2, nbest=1, T=4, M=8, final=0, state=p, nbytes=1 << 30, tokens=p, frames=None, logits=p, committed=p):
        return L.mi_ctc_beam_stream_walk(logits, 8, 64, 0, 1, T, V1, None, blank, 0, W, K, nbest, p, p, p, p, state, nbytes, M, final, committed, p, p, p, tokens, 1, p, p,
                                         frames, None)
    for kw in (dict(V1=1, blank=0), dict(blank=5), dict(blank=-1), dict(W=0), dict(W=65), dict(K=0), dict(K=65), dict(nbest=5), dict(nbest=0), dict(T=-1), dict(M=0),
               dict(final=2), dict(state=None), dict(state=p + 4), dict(nbytes=64), dict(committed=None), dict(logits=None), dict(tokens=None, final=1),
               dict(tokens=None, frames=p)):
        assert walk(**kw) == _lib.ERR_ARG, kw
    assert walk(M=1 << 20, W=64) == _lib.ERR_UNSUPPORTED
    assert L.mi_ctc_beam_stream_reset(None, 1 << 30, 1, 8, 4, None) == _lib.ERR_ARG
    assert L.mi_ctc_beam_stream_reset(p, 64, 1, 8, 4, None) == _lib.ERR_ARG
    assert L.mi_ctc_beam_stream_reset(p, 1 << 30, 1, 8, 65, None) == _lib.ERR_ARG
    assert L.mi_ctc_beam_stream_reset(p, 1 << 30, 1, 1 << 20, 64, None) == _lib.ERR_UNSUPPORTED


def test_header_and_signatures_agree():
    from huggingface_asr_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hfasr_hip.h")).read(), flags=re.S)
    kinds = {"size_t": _lib.sz, "int": _lib.i32, "long": _lib.i64}
    for name, ret in (("mi_ctc_beam_stream_state_bytes", "size_t"), ("mi_ctc_beam_stream_reset", "int"), ("mi_ctc_beam_stream_walk", "int")):
        m = re.search(r"\b" + ret + r"\s+" + name + r"\s*\(([^;]*?)\)\s*;", header, flags=re.S)
        assert m, name
        want = []
        for arg in m.group(1).split(","):
            words = arg.replace("*", " * ").split()
            want.append(_lib.vp if "*" in words or words[0] == "mi_stream_t" else kinds[[w for w in words if w != "const"][0]])
        assert _lib.SIGNATURES[name] == want, name
        assert getattr(_lib.lib(), name).restype is kinds[ret]
    src = open(os.path.join(ROOT, "huggingface_asr_amd", "csrc", "build.py")).read()
    assert '"ctc_beam_stream.hip"' in src


# ---------------------------------------------------------------- what Python refuses on the host
def test_constructor_refusals():
    from huggingface_asr_amd import ops
    ok = dict(beams=4, blank=4, pad_id=0)
    for kw in (dict(beams=0), dict(beams=65), dict(nbest=5), dict(nbest=0), dict(token_topk=0), dict(token_topk=65), dict(blank=-1)):
        with pytest.raises(ValueError):
            ops.CtcBeamStream(2, 16, **dict(ok, **kw))
    for args in ((0, 16), (2, 0)):
        with pytest.raises(ValueError):
            ops.CtcBeamStream(*args, **ok)
    with pytest.raises(ValueError, match="node table"):
        ops.CtcBeamStream(1, 65536, beams=64, blank=4, pad_id=0)
    for kw in (dict(beams=4.0), dict(beams=True), dict(nbest=1.0), dict(token_topk=2.0), dict(dtype=torch.int16)):
        with pytest.raises(TypeError):
            ops.CtcBeamStream(2, 16, **dict(ok, **kw))
    with pytest.raises(TypeError):
        ops.CtcBeamStream(2, 16, blank=4, pad_id=0)                        # beams is required


def test_feed_refusals_come_before_any_launch():
    """on CPU tensors: whatever is wrong with a call is reported before the device is asked for anything, and the host count of frames does not move"""
    from huggingface_asr_amd import ops
    st = ops.CtcBeamStream(2, 16, beams=4, blank=4, pad_id=0)
    x = torch.zeros(2, 6, 5)
    for bad in (x[0], x.double(), x.long(), "x"):
        with pytest.raises(TypeError):
            st.feed(bad)
    for bad in (torch.zeros(3, 6, 5), torch.zeros(2, 6, 4), torch.zeros(2, 6, 1)):      # another batch; the blank outside; one class
        with pytest.raises(ValueError):
            st.feed(bad)
    with pytest.raises(ValueError, match="n_valid"):
        st.feed(x, [1, 2, 3])
    with pytest.raises(RuntimeError, match="max_frames"):
        st.feed(torch.zeros(2, 17, 5))
    with pytest.raises(RuntimeError, match="device"):                      # a good call, on the CPU: there is no fallback
        st.feed(x)
    assert st.walked == 0 and st._state is None
    st.walked = 12                                                         # as after 12 frames
    with pytest.raises(RuntimeError, match="max_frames"):
        st.feed(x)
    st.finished = True                                                     # as after final=True
    with pytest.raises(RuntimeError, match="finished"):
        st.feed(x[:, :1])
    st.reset()
    assert st.walked == 0 and not st.finished


def test_engine_stream_refusals_and_no_state_without_beams():
    from huggingface_asr_amd import shapes
    from huggingface_asr_amd.engine import EBranchformerEngine
    eng = EBranchformerEngine(dict(shapes.TINY, is_causal=True), "cpu")
    assert eng.stream(2, 4, 40).beam is None
    st = eng.stream(2, 4, 40, beams=8, nbest=4, token_topk=6)
    assert (st.beam.beams, st.beam.nbest, st.beam.token_topk, st.beam.max_frames, st.beam.B, st.beam._state) == (8, 4, 6, 40, 2, None)
    for kw in (dict(beams=0), dict(beams=65), dict(beams=4, nbest=5), dict(beams=4, token_topk=65), dict(nbest=2), dict(token_topk=4)):
        with pytest.raises(ValueError):
            eng.stream(2, 4, 40, **kw)
    with pytest.raises(TypeError):
        eng.stream(2, 4, 40, beams=4.0)
    with pytest.raises(ValueError, match="beams="):
        eng.stream(2, 4, 40).feed(torch.zeros(2, 16, 80), partial=True)


# ---------------------------------------------------------------- the built kernel
def test_stream_kernel_uses_no_scratch_the_lds_its_header_states_and_at_most_128_vgprs():
    from huggingface_asr_amd import _lib
    _lib.lib()
    header = open(os.path.join(ROOT, "huggingface_asr_amd", "csrc", "ctc_beam_stream.hip")).read()
    stated = int(re.search(r"//\s+ctc_stream_beam_kernel\s.*?(\d+) B of LDS", header).group(1))
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
            if b"ctc_stream_beam_kernel" not in blob[lo:hi]:
                continue
            with open(fb, "wb") as f:
                f.write(blob[lo:hi])
            subprocess.run([os.path.join(llvm, "clang-offload-bundler"), "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--input={fb}",
                            f"--output={co}"], check=True)
            notes = subprocess.run([os.path.join(llvm, "llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout
            for block in notes.split("- .agpr_count")[1:]:
                name = re.search(r"\.name:\s+(\S*ctc_stream_beam_kernel\S*)", block)
                if name:
                    num = lambda key: int(re.search(r"\." + key + r":\s+(\d+)", block).group(1))
                    found[name.group(1)] = (num("private_segment_fixed_size"), num("group_segment_fixed_size"), num("vgpr_count"))
                assert not re.search(r"\.name:\s+\S*(ctc_walk_kernel|ctc_cut_kernel)", block)      # the one-shot kernels live in their own translation unit
    assert len(found) == 2, sorted(found)                                  # int32 and int64 tokens
    for name, (scratch, lds, vgprs) in found.items():
        assert scratch == 0 and lds == stated and vgprs <= 128, (name, scratch, lds, vgprs)
