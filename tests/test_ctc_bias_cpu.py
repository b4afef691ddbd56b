"""CPU: contextual biasing of the CTC prefix beam search — ctc_bias.CtcBias' compiled tables against the credit's definition (tests/ctc_bias_ref.py), the float64 biased
restatement against the enumeration of every label sequence, that a zero weight is the unbiased search, that the bias changes an answer, what the surfaces refuse on
the host, the state's size, the header, the budgets of the three kernels in the built code object, and the certification of the seeds the device test runs."""
import itertools
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
import ctc_bias_ref as BR  # noqa: E402
from huggingface_asr_amd.ctc_bias import CtcBias  # noqa: E402

SMALL = [(1, 3), (2, 3), (5, 3), (3, 4)]                                   # the exhaustive shapes of test_ctc_beam_cpu.py: at most 63 prefixes, nothing is pruned at W = 64
TABLE = [[0, 1], [1], [0, 1, 0, 0]]                                        # the issue's worked example
LISTS = [TABLE,
         [[0], [0, 1]],                                                    # nested
         [[0, 1, 2], [1, 2]],                                              # a phrase that is a suffix of another
         [[0, 1, 0, 2, 1, 0]],                                             # one long phrase
         [[2, 2], [2, 0, 2], [1]],
         [[0, 0, 1], [0, 1, 1], [1, 0]],
         []]


def small_logits(T, V1, seed):
    return np.random.default_rng(1000 * T + 100 * V1 + seed).standard_normal((T, V1)).astype(np.float32)


# ---------------------------------------------------------------- the credit
def test_the_worked_example():
    ctx = CtcBias(TABLE, 1.0, 4, 3)
    for seq, n in (([0], 1), ([0, 1], 2), ([0, 1, 0], 3), ([0, 1, 0, 0], 4), ([0, 1, 0, 1], 3), ([1, 1], 2), ([0, 0, 1], 2), ([1, 0, 1, 1], 4)):
        assert BR.credit(TABLE, seq) == n and ctx.credit(seq) == n, seq


@pytest.mark.parametrize("phrases", LISTS, ids=[str(i) for i in range(len(LISTS))])
def test_compiled_tables_give_the_definitions_credit(phrases):
    ctx = CtcBias(phrases, 0.5, 4, 3)
    for n in range(8):
        for seq in itertools.product(range(3), repeat=n):
            got = ctx.credit(seq)
            assert got == BR.credit(phrases, seq), (phrases, seq)
            assert 0 <= got <= n


def test_packed_tables():
    for phrases, V1, blank in ((TABLE, 4, 3), ([[5, 6], [6, 5, 5]], 7, 2), ([[0, 3]], 5, 4), ([], 4, 3)):
        ctx = CtcBias(phrases + phrases[:1], 1.0, V1, blank)               # a duplicate counts once
        assert ctx.phrases == tuple(tuple(p) for p in phrases)
        S, A1 = ctx.tab.shape
        assert (S, A1) == (ctx.S, ctx.A1) and ctx.tab.dtype == np.int32 and ctx.col.dtype == np.int32 and ctx.col.shape == (V1,)
        assert A1 == len({t for p in phrases for t in p}) + 1 and S == len({tuple(p[:i]) for p in phrases for i in range(len(p) + 1)} | {()})
        nxt, dn = ctx.tab & 0xFFFF, ctx.tab >> 16
        assert nxt.min() >= 0 and nxt.max() < S
        assert np.array_equal(((dn.astype(np.int64) & 0xFFFF) << 16 | nxt).astype(np.uint32).view(np.int32), ctx.tab)      # dn round-trips through 16 bits
        used = {t for p in phrases for t in p}
        for t in range(V1):
            assert (ctx.col[t] == 0) == (t not in used), t                 # column 0: every token in no phrase (the blank, and class V1 - 1 when it is not the blank)
        assert sorted(ctx.col[sorted(used)].tolist()) == list(range(1, A1))
    assert CtcBias([[5, 6]], 1.0, 7, 2).col[6] == 1 + 1 and CtcBias([[5]], 1.0, 7, 2).col[6] == 0
    assert CtcBias([], -3.0, 4, 3).tab.tolist() == [[0]]


# ---------------------------------------------------------------- the search
@pytest.mark.parametrize("w", [0.5, 2.0, -1.0])
@pytest.mark.parametrize("T,V1", SMALL)
def test_restatement_equals_the_biased_enumeration(T, V1, w):
    blank = V1 - 1
    for seed in range(10):
        phrases = LISTS[seed % 6]
        phrases = [p for p in phrases if max(p) < blank]
        x = small_logits(T, V1, seed)
        want = BR.enumerate_all(x, blank, phrases, w)[:8]
        got = BR.beam_search(x, blank, 64, V1 - 1, nbest=8, phrases=phrases, w=w)["hyps"]
        assert [h[0] for h in got] == [e[0] for e in want], (T, V1, seed, w)
        for (labels, score, frames, n), (_, exact, n_exact) in zip(got, want):
            assert abs(score - exact) <= 1e-9 and n == n_exact == BR.credit(phrases, labels), (T, V1, seed, labels)
            assert len(frames) == len(labels)


def test_zero_weight_and_empty_list_are_the_unbiased_restatement():
    for T, V1, W, K in ((5, 3, 64, 2), (3, 4, 64, 3), (24, 12, 4, 4)):
        for seed in range(6):
            x = small_logits(T, V1, seed) if T < 24 else R.peaky(seed, T, V1, V1 - 1)
            plain = R.beam_search(x, V1 - 1, W, K, nbest=4)
            for phrases, w in ((TABLE[:2], 0.0), ([], 1.5)):
                got = BR.beam_search(x, V1 - 1, W, K, nbest=4, phrases=phrases, w=w)
                assert [h[:3] for h in got["hyps"]] == plain["hyps"]       # labels, scores and frames, exactly
                assert got["margins"] == plain["margins"]


def test_the_bias_changes_the_answer():
    """two frames, classes (a, b, blank), p(a) = 0.47, p(b) = 0.29: the unbiased best is (a) and does not hold the phrase (b); with weight 2 the best is (b)"""
    x = np.log(np.array([[0.50, 0.30, 0.20], [0.10, 0.10, 0.80]], dtype=np.float64)).astype(np.float32)
    plain = R.beam_search(x, 2, 8, 2, nbest=2)["hyps"]
    got = BR.beam_search(x, 2, 8, 2, nbest=2, phrases=[[1]], w=2.0)["hyps"]
    assert plain[0][0] == (0,) and 1 not in plain[0][0]
    assert got[0][0] == (1,) and got[0][3] == 1
    assert got[0][1] < plain[0][1]                                         # `scores` stay CTC log-probabilities: the boosted answer is the less probable one
    assert abs(got[0][1] - R.ctc_logp(R.log_softmax(x), (1,), 2)) < 1e-12


def test_suspended_form_equals_the_one_shot_one():
    x, blank, phrases = BR.cert_case(BR.CERT_SEEDS[0])
    whole = BR.beam_search(x, blank, 8, 8, nbest=4, phrases=phrases, w=0.5)
    for cuts in ((48,), (0, 7, 7, 30, 48), (1, 2, 3, 48)):
        s = BR.BiasedSearch(blank, 8, 8, 4, phrases, 0.5)
        lo, seen = 0, ()
        for hi in cuts:
            s.walk(x[lo:hi])
            lo = hi
            c = s.committed()
            assert c[:len(seen)] == seen                                   # the committed prefix only grows
            seen = c
        assert s.hyps() == whole["hyps"] and s.margins() == whole["margins"]


def test_the_device_tests_seeds_are_certified():
    """the float64 restatement's smallest decision margin on every draw the GPU certified case runs: an fp32 search must then take the same decisions"""
    assert len(BR.CERT_SEEDS) >= 3
    changed = 0
    for seed in BR.CERT_SEEDS:
        x, blank, phrases = BR.cert_case(seed)
        plain = R.beam_search(x, blank, BR.CERT_W, BR.CERT_K, nbest=BR.CERT_NBEST)
        for w in BR.CERT_WEIGHTS:
            r = BR.beam_search(x, blank, BR.CERT_W, BR.CERT_K, nbest=BR.CERT_NBEST, phrases=phrases, w=w)
            assert BR.min_margin(r) >= BR.CERT_MARGIN, (seed, w, BR.min_margin(r))
            assert float(np.float32(w)) * 64 == w * 64                     # dyadic: w n is exact in fp32
            changed += [h[0] for h in r["hyps"]] != [h[0] for h in plain["hyps"]]
    assert changed >= 2, changed                                           # the certified draws are ones the bias acts on


# ---------------------------------------------------------------- what is refused on the host
def test_context_refusals():
    ok = dict(weight=1.0, vocab=10, blank=9)
    for phrases in ([[]], [[1], []], [[9]], [[10]], [[-1]], [[1, 2, 9]]):
        with pytest.raises(ValueError):
            CtcBias(phrases, **ok)
    for w in (float("nan"), float("inf"), -float("inf"), 100.5, -101):
        with pytest.raises(ValueError):
            CtcBias([[1]], w, 10, 9)
    assert CtcBias([[1]], -100, 10, 9).weight == -100.0 and CtcBias([], 1.0, 10, 9).S == 1
    with pytest.raises(ValueError):
        CtcBias([[1]], 1.0, 10, 10)                                        # the blank outside the classes
    with pytest.raises(TypeError):
        CtcBias([[1.5]], **ok)
    with pytest.raises(ValueError, match="states"):                        # S <= 4096
        CtcBias([[i] + [1] * 63 for i in range(66)], 1.0, 100, 99)
    with pytest.raises(ValueError, match="distinct"):                      # A1 <= 1024
        CtcBias([[i] for i in range(1024)], 1.0, 2000, 1999)
    with pytest.raises(ValueError, match="words"):                         # S A1 <= 2^20
        CtcBias([[i, (i + 1) % 600, (i + 2) % 600, (i + 3) % 600] for i in range(600)], 1.0, 700, 699)
    at = CtcBias(BR.phrases_4096(), 1.0, 100, 99)                           # exactly at the limit
    assert at.S == 4096 and len(at.phrases) == 64 and all(len(p) == 64 for p in at.phrases)
    assert CtcBias([[i] for i in range(1023)], 1.0, 1100, 1099).tab.shape == (1024, 1024)


def test_ops_refusals_come_before_any_launch():
    from huggingface_asr_amd import ops
    x = torch.zeros(2, 6, 5)
    ctx, other_vocab, other_blank = CtcBias([[1, 2]], 1.0, 5, 4), CtcBias([[1, 2]], 1.0, 6, 4), CtcBias([[1, 2]], 1.0, 5, 0)
    for bad in ("ctx", [[1, 2]], (ctx.col, ctx.tab)):
        with pytest.raises(TypeError, match="CtcBias"):
            ops.ctc_beam_decode(x, 4, 0, beams=4, bias=bad)
        with pytest.raises(TypeError, match="CtcBias"):
            ops.CtcBeamStream(2, 16, beams=4, blank=4, pad_id=0, bias=bad)
        with pytest.raises(TypeError, match="CtcBias"):
            ops.CtcBeamPool(2, 16, beams=4, blank=4, pad_id=0, bias=bad)
    for bad in (other_vocab, other_blank):
        with pytest.raises(ValueError, match="bias context"):
            ops.ctc_beam_decode(x, 4, 0, beams=4, bias=bad)
    with pytest.raises(TypeError):
        ops.ctc_beam_decode(x, 4, 0, bias=ctx)                             # beams is required
    with pytest.raises(ValueError, match="bias context"):
        ops.CtcBeamStream(2, 16, beams=4, blank=4, pad_id=0, bias=other_blank)
    with pytest.raises(ValueError, match="bias context"):
        ops.CtcBeamPool(2, 16, beams=4, blank=4, pad_id=0, bias=other_blank)
    st = ops.CtcBeamStream(2, 16, beams=4, blank=4, pad_id=0, bias=other_vocab)
    with pytest.raises(ValueError, match="bias context"):
        st.feed(x)
    bp = ops.CtcBeamPool(2, 16, beams=4, blank=4, pad_id=0, bias=other_vocab)
    bp.open(0)
    with pytest.raises(ValueError, match="bias context"):
        bp.step(x[0], [(0, 0, 6, False, False)])
    with pytest.raises(RuntimeError, match="device"):                      # a good call, on the CPU: there is no fallback
        ops.ctc_beam_decode(x, 4, 0, beams=4, bias=ctx)
    good = ops.CtcBeamStream(2, 16, beams=4, blank=4, pad_id=0, bias=ctx)
    with pytest.raises(RuntimeError, match="device"):
        good.feed(x)
    assert good.walked == 0 and good._state is None and st._state is None and bp._state is None


def test_engine_and_model_refusals():
    from huggingface_asr_amd import shapes
    from huggingface_asr_amd.engine import EBranchformerEngine
    cfg = dict(shapes.TINY, is_causal=True)
    V = cfg["vocab_size"]
    eng = EBranchformerEngine(cfg, "cpu")
    ctx, other = CtcBias([[1, 2]], 1.0, V + 1, V), CtcBias([[1, 2]], 1.0, V + 2, V + 1)
    feats = torch.zeros(1, 100, 80)
    with pytest.raises(ValueError, match="beams"):
        eng.transcribe(feats, bias=ctx)
    with pytest.raises(ValueError, match="bias context"):
        eng.transcribe(feats, beams=4, bias=other)
    with pytest.raises(TypeError, match="CtcBias"):
        eng.transcribe(feats, beams=4, bias=[[1, 2]])
    with pytest.raises(ValueError, match="beams"):
        eng.stream(2, 4, 40, bias=ctx)
    with pytest.raises(ValueError, match="bias context"):
        eng.stream(2, 4, 40, beams=4, bias=other)
    with pytest.raises(TypeError, match="CtcBias"):
        eng.stream_pool(2, 4, 40).with_beams(4, bias="x")
    with pytest.raises(ValueError, match="bias context"):
        eng.stream_pool(2, 4, 40).with_beams(4, bias=other)
    assert eng.stream(2, 4, 40, beams=4, bias=ctx).beam.bias is ctx and eng.stream(2, 4, 40, beams=4).beam.bias is None
    assert eng.stream_pool(2, 4, 40).with_beams(4, bias=ctx).beam.bias is ctx


def test_model_bias_context_takes_ids_and_text():
    from huggingface_asr_amd.modeling_ebranchformer import Wav2Vec2EBranchformerForCTC as M

    class Cfg:
        vocab_size = 20

    class Tok:
        def __call__(self, text, add_special_tokens=True):
            assert add_special_tokens is False

            class Enc:
                input_ids = [ord(c) - 97 for c in text]
            return Enc

    class Stub:
        config = Cfg
    ctx = M.bias_context(Stub(), [[3, 4], "abc", [3, 4]], 1.5, tokenizer=Tok())
    assert ctx.phrases == ((3, 4), (0, 1, 2)) and (ctx.vocab, ctx.blank, ctx.weight) == (21, 20, 1.5)
    with pytest.raises(ValueError, match="tokenizer"):
        M.bias_context(Stub(), ["abc"], 1.5)
    with pytest.raises(ValueError):
        M.bias_context(Stub(), [[20]], 1.5)                                # the blank


# ---------------------------------------------------------------- the C ABI without a device
def _table_words(M, W):
    h = 2
    while h < 2 * (1 + M * W):
        h <<= 1
    return h


def test_state_bytes_match_the_documented_formula_and_the_unbiased_value_is_unchanged():
    from huggingface_asr_amd import _lib
    f, plain = _lib.lib().mi_ctc_beam_bias_stream_state_bytes, _lib.lib().mi_ctc_beam_stream_state_bytes
    align16 = lambda v: (v + 15) // 16 * 16
    for B, M, W in ((1, 1, 1), (3, 48, 4), (2, 1040, 64), (32, 1500, 10), (7, 333, 5)):
        unbiased = B * (64 + 7 * 64 * 4) + align16(16 * B * (1 + M * W)) + 8 * B * _table_words(M, W)
        assert plain(B, M, W) == unbiased and f(B, M, W) == unbiased + B * 2 * 64 * 4, (B, M, W)
    for bad in ((0, 10, 4), (1, 0, 4), (1, 10, 0), (1, 10, 65), (1, 65536, 64)):
        assert f(*bad) == 0, bad


def test_c_entries_refuse_bad_arguments_before_any_launch():
    from huggingface_asr_amd import _lib
    L = _lib.lib()
    buf = (_lib.C.c_char * 8192)()
    p = (_lib.C.addressof(buf) + 15) // 16 * 16
    nan, inf = float("nan"), float("inf")
    bias_bad = (dict(col=None), dict(tab=None), dict(S=0), dict(S=4097), dict(A1=0), dict(A1=1025), dict(S=2048, A1=1024), dict(w=nan), dict(w=inf), dict(w=-inf),
                dict(credit=None))

    def walk(V1=5, blank=4, W=4, K=2, nbest=1, col=p, tab=p, S=3, A1=2, w=1.0, credit=p):
        return L.mi_ctc_beam_walk_bias(p, 8, 64, 0, 1, 4, V1, None, blank, 0, W, K, nbest, p, p, p, p, p, 1 << 30, p, 1, p, p, None, col, tab, S, A1, w, credit, None)

    def stream(V1=5, blank=4, W=4, K=2, nbest=1, T=4, M=8, final=0, state=p, nbytes=1 << 30, tokens=p, col=p, tab=p, S=3, A1=2, w=1.0, credit=p):
        return L.mi_ctc_beam_bias_stream_walk(p, 8, 64, 0, 1, T, V1, None, blank, 0, W, K, nbest, p, p, p, p, state, nbytes, M, final, p, p, p, p, tokens, 1, p, p, None,
                                              col, tab, S, A1, w, credit, None)
    rec = (_lib.C.c_int * 5)(0, 0, 4, 0, 0)

    def slots(V1=5, blank=4, W=4, K=2, nbest=1, M=8, state=p, nbytes=1 << 30, records=rec, col=p, tab=p, S=3, A1=2, w=1.0, credit=p):
        return L.mi_ctc_beam_bias_stream_walk_slots(p, 8, 0, 4, V1, blank, 0, W, K, nbest, p, p, p, p, state, nbytes, 2, M, records, 1, p, p, p, p, p, p, 1, p, p, None, 1,
                                                    col, tab, S, A1, w, credit, None)
    for fn in (walk, stream, slots):
        for kw in bias_bad + (dict(V1=1, blank=0), dict(blank=5), dict(W=0), dict(W=65), dict(K=65), dict(nbest=5)):
            assert fn(**kw) == _lib.ERR_ARG, (fn.__name__, kw)
    for kw in (dict(final=2), dict(state=None), dict(state=p + 4), dict(M=0), dict(tokens=None, final=1)):
        assert stream(**kw) == _lib.ERR_ARG, kw
    unbiased = L.mi_ctc_beam_stream_state_bytes(1, 8, 4)
    assert stream(nbytes=unbiased) == _lib.ERR_ARG and slots(nbytes=L.mi_ctc_beam_stream_state_bytes(2, 8, 4)) == _lib.ERR_ARG      # an unbiased state is too small
    assert slots(records=(_lib.C.c_int * 5)(2, 0, 4, 0, 0)) == _lib.ERR_ARG and slots(records=(_lib.C.c_int * 5)(0, 2, 4, 0, 0)) == _lib.ERR_ARG
    assert stream(M=1 << 20, W=64) == _lib.ERR_UNSUPPORTED
    assert L.mi_ctc_beam_bias_stream_reset(None, 1 << 30, 1, 8, 4, None) == _lib.ERR_ARG
    assert L.mi_ctc_beam_bias_stream_reset(p, unbiased, 1, 8, 4, None) == _lib.ERR_ARG
    assert L.mi_ctc_beam_bias_stream_reset(p, 1 << 30, 1, 8, 65, None) == _lib.ERR_ARG
    assert L.mi_ctc_beam_bias_stream_reset_slot(p, 1 << 30, 2, 8, 4, 2, None) == _lib.ERR_ARG
    assert L.mi_ctc_beam_bias_stream_reset_slot(p, L.mi_ctc_beam_stream_state_bytes(2, 8, 4), 2, 8, 4, 0, None) == _lib.ERR_ARG


NAMES = (("mi_ctc_beam_walk_bias", "int"), ("mi_ctc_beam_bias_stream_state_bytes", "size_t"), ("mi_ctc_beam_bias_stream_reset", "int"),
         ("mi_ctc_beam_bias_stream_walk", "int"), ("mi_ctc_beam_bias_stream_reset_slot", "int"), ("mi_ctc_beam_bias_stream_walk_slots", "int"))


def test_header_signatures_and_exported_symbols_agree():
    from huggingface_asr_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hfasr_hip.h")).read(), flags=re.S)
    kinds = {"size_t": _lib.sz, "int": _lib.i32, "long": _lib.i64, "float": _lib.f32}
    so = os.path.join(ROOT, "huggingface_asr_amd", "libhfasr_hip.so")
    _lib.lib()
    exported = _lib.C.CDLL(so)                                             # a handle of its own: a symbol is looked up in the library, not in _lib's table
    unbiased = {"mi_ctc_beam_walk_bias": "mi_ctc_beam_walk", "mi_ctc_beam_bias_stream_walk": "mi_ctc_beam_stream_walk",
                "mi_ctc_beam_bias_stream_walk_slots": "mi_ctc_beam_stream_walk_slots", "mi_ctc_beam_bias_stream_reset": "mi_ctc_beam_stream_reset",
                "mi_ctc_beam_bias_stream_reset_slot": "mi_ctc_beam_stream_reset_slot", "mi_ctc_beam_bias_stream_state_bytes": "mi_ctc_beam_stream_state_bytes"}
    for name, ret in NAMES:
        m = re.search(r"\b" + ret + r"\s+" + name + r"\s*\(([^;]*?)\)\s*;", header, flags=re.S)
        assert m, name
        want = []
        for arg in m.group(1).split(","):
            words = arg.replace("*", " * ").split()
            want.append(_lib.vp if "*" in words or words[0] == "mi_stream_t" else kinds[[w for w in words if w != "const"][0]])
        assert _lib.SIGNATURES[name] == want, name
        assert getattr(_lib.lib(), name).restype is kinds[ret]
        assert getattr(exported, name, None) is not None, name
        plain = _lib.SIGNATURES[unbiased[name]]
        if name.endswith(("walk_bias", "_walk", "_walk_slots")):           # the counterpart's arguments, then col, tab, S, A1, weight, credit, and the stream last
            assert want == plain[:-1] + [_lib.vp, _lib.vp, _lib.i32, _lib.i32, _lib.f32, _lib.vp, _lib.vp], name
        else:
            assert want == plain, name
    src = open(os.path.join(ROOT, "huggingface_asr_amd", "csrc", "build.py")).read()
    for tu in ("ctc_beam_bias.hip", "ctc_beam_bias_stream.hip", "ctc_beam_bias_pool.hip"):
        assert f'"{tu}"' in src


# ---------------------------------------------------------------- the built kernels
def test_bias_kernels_use_no_scratch_the_lds_their_headers_state_and_at_most_128_vgprs():
    from huggingface_asr_amd import _lib
    _lib.lib()
    kernels = {"ctc_bias_walk": "ctc_beam_bias.hip", "ctc_bias_stream_beam": "ctc_beam_bias_stream.hip", "ctc_bias_pool_beam": "ctc_beam_bias_pool.hip"}
    stated = {}
    for k, tu in kernels.items():
        header = open(os.path.join(ROOT, "huggingface_asr_amd", "csrc", tu)).read()
        stated[k] = int(re.search(r"//\s+" + k + r"\s.*?(\d+) B of LDS", header).group(1))
    assert set(stated.values()) == {44576 + 2 * 2 * 64 * 4}                # the unbiased walk's LDS and (s, n) in both beams
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
            if b"ctc_bias_" not in blob[lo:hi]:
                continue
            with open(fb, "wb") as f:
                f.write(blob[lo:hi])
            subprocess.run([os.path.join(llvm, "clang-offload-bundler"), "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--input={fb}",
                            f"--output={co}"], check=True)
            notes = subprocess.run([os.path.join(llvm, "llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout
            for block in notes.split("- .agpr_count")[1:]:
                name = re.search(r"\.name:\s+(\S*(ctc_bias_walk|ctc_bias_stream_beam|ctc_bias_pool_beam)\S*)", block)
                if name:
                    num = lambda key: int(re.search(r"\." + key + r":\s+(\d+)", block).group(1))
                    found[name.group(1)] = (name.group(2), num("private_segment_fixed_size"), num("group_segment_fixed_size"), num("vgpr_count"))
                # the names the unbiased budget tests count by must not occur in the biased translation units
                assert not re.search(r"\.name:\s+\S*(ctc_walk_kernel|ctc_cut_kernel|ctc_stream_beam_kernel|ctc_pool_beam_kernel)", block)
    assert len(found) == 6, sorted(found)                                  # three kernels; int32 and int64 tokens
    for name, (kind, scratch, lds, vgprs) in found.items():
        assert scratch == 0 and lds == stated[kind] and vgprs <= 128, (name, scratch, lds, vgprs)
