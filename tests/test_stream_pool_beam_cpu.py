"""CPU: the CTC prefix beam search on the session pool — what `with_beams` and `ops.CtcBeamPool` refuse on the host, the records a step hands to the walk, the
declarations of the two per-slot entries, what they refuse before any launch, and the budget of csrc/ctc_beam_pool.hip's kernel in the built code object."""
import os
import re
import subprocess
import tempfile

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _engine():
    from huggingface_asr_amd import shapes
    from huggingface_asr_amd.engine import EBranchformerEngine
    return EBranchformerEngine(dict(shapes.TINY, is_causal=True), "cpu")


# ---------------------------------------------------------------- with_beams
def test_with_beams_refusals_and_no_state_before_a_device_step():
    eng = _engine()
    assert eng.stream_pool(2, 4, 40).beam is None
    pool = eng.stream_pool(2, 4, 40)
    assert pool.with_beams(8, nbest=4, token_topk=6) is pool
    b = pool.beam
    assert (b.beams, b.nbest, b.token_topk, b.max_frames, b.S, b._state, b.blank, b.pad_id, b.dtype) == (8, 4, 6, 40, 2, None, eng.cfg["vocab_size"], -1, torch.int32)
    for args, kw in (((0,), {}), ((65,), {}), ((4,), dict(nbest=5)), ((4,), dict(nbest=0)), ((4,), dict(token_topk=65)), ((4,), dict(token_topk=0))):
        with pytest.raises(ValueError):
            eng.stream_pool(2, 4, 40).with_beams(*args, **kw)
    for args, kw in (((4.0,), {}), ((True,), {}), ((None,), {}), ((4,), dict(nbest=1.0)), ((4,), dict(token_topk=2.0))):
        with pytest.raises(TypeError):
            eng.stream_pool(2, 4, 40).with_beams(*args, **kw)
    assert eng.stream_pool(1, 4, 8192).with_beams(64).beam.state_bytes > 0                 # the pool's max_frames <= 8192 stays below the node-table limit (CtcBeamPool's test)
    with pytest.raises(ValueError, match="with_beams"):
        eng.stream_pool(2, 4, 40).step(partial=True)                       # partial without the beam search
    with pytest.raises(TypeError):
        pool.step(partial=3)
    with pytest.raises(ValueError):
        pool.step(partial={2})                                             # a slot the pool does not have
    assert pool.step(partial={1}) == {}                                    # nothing named: nothing runs


def test_with_beams_needs_a_pool_without_open_sessions():
    pool = _engine().stream_pool(2, 4, 40)
    sid = pool.open()
    with pytest.raises(RuntimeError, match="open"):
        pool.with_beams(4)
    assert pool.beam is None
    pool = _engine().stream_pool(2, 4, 40).with_beams(4)
    sid = pool.open()                                                      # opens the slot's beam too
    assert pool.beam.is_open == [True, False] and pool.beam.walked == [0, 0] and sid == 0
    with pytest.raises(RuntimeError, match="open"):
        pool.with_beams(8)
    assert pool.beam.beams == 4
    ap = _engine().audio_pool(2, 4, 40)
    assert ap.with_beams(4, nbest=2) is ap and ap.pool.beam.nbest == 2
    ap.open()
    with pytest.raises(RuntimeError, match="open"):
        ap.with_beams(4)


def test_the_constructor_keyword_still_raises_and_names_the_method():
    eng = _engine()
    with pytest.raises(NotImplementedError, match="with_beams"):
        eng.stream_pool(2, 4, 40, beams=4)
    with pytest.raises(NotImplementedError, match="with_beams"):
        eng.audio_pool(2, 4, 40, beams=4)


# ---------------------------------------------------------------- the C entries without a device
def test_header_and_signatures_agree_for_the_slot_entries():
    from huggingface_asr_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hfasr_hip.h")).read(), flags=re.S)
    kinds = {"size_t": _lib.sz, "int": _lib.i32, "long": _lib.i64}
    for name in ("mi_ctc_beam_stream_reset_slot", "mi_ctc_beam_stream_walk_slots"):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", header, flags=re.S)
        assert m, name
        want = []
        for arg in m.group(1).split(","):
            words = arg.replace("*", " * ").split()
            want.append(_lib.vp if "*" in words or words[0] == "mi_stream_t" else kinds[[w for w in words if w != "const"][0]])
        assert _lib.SIGNATURES[name] == want, name
        assert getattr(_lib.lib(), name).restype is _lib.i32
    src = open(os.path.join(ROOT, "huggingface_asr_amd", "csrc", "build.py")).read()
    assert '"ctc_beam_pool.hip"' in src


def test_slot_entries_refuse_bad_arguments_before_any_launch():
    from huggingface_asr_amd import _lib
    L = _lib.lib()
    buf = (_lib.C.c_char * 8192)()
    p = (_lib.C.addressof(buf) + 15) // 16 * 16

    def walk(records=((0, 0, 4, 0, -1),), V1=5, blank=4, W=4, K=2, nbest=1, rows=8, M=8, S=3, R=1, state=p, nbytes=1 << 30, tokens=p, frames=None, logits=p, committed=p,
             dev=p, host=True, dtype=0, tdtype=1, A=None):
        rec = (_lib.C.c_int * (5 * len(records)))(*[v for r in records for v in r])
        return L.mi_ctc_beam_stream_walk_slots(logits, 8, dtype, rows, V1, blank, 0, W, K, nbest, p, p, p, p, state, nbytes, S, M, rec if host else None,
                                               len(records) if A is None else A, dev, committed, p, p, p, tokens, tdtype, p, p, frames, R, None)
    for kw in (dict(V1=1, blank=0), dict(blank=5), dict(blank=-1), dict(W=0), dict(W=65), dict(K=0), dict(K=65), dict(nbest=5), dict(nbest=0), dict(rows=-1), dict(M=0),
               dict(state=None), dict(state=p + 4), dict(nbytes=64), dict(committed=None), dict(logits=None), dict(tokens=None), dict(tokens=None, R=0, frames=p),
               dict(dtype=2), dict(tdtype=2), dict(S=0), dict(dev=None), dict(host=False), dict(A=0), dict(R=-1), dict(R=2),
               dict(records=((3, 0, 4, 0, -1),)), dict(records=((-1, 0, 4, 0, -1),)),                   # a slot out of range
               dict(records=((1, 0, 2, 0, -1), (1, 2, 2, 0, -1))),                                      # ... named twice
               dict(records=((0, 6, 4, 0, -1),)), dict(records=((0, -1, 4, 0, -1),)), dict(records=((0, 0, -1, 0, -1),)), dict(records=((0, 9, 0, 0, -1),)),
               dict(records=((0, 0, 4, 0, 1),)), dict(records=((0, 0, 4, 0, -2),)),                     # out outside [-1, R)
               dict(records=((0, 0, 4, 0, 1), (1, 4, 4, 0, 1)), R=2),                                       # ... used twice
               dict(records=((0, 0, 4, 1, -1),)), dict(records=((0, 0, 4, 2, 0),)),                     # final without out; final outside {0, 1}
               dict(records=((0, 0, 1, 0, -1), (1, 1, 1, 0, -1), (2, 2, 1, 0, -1), (0, 3, 1, 0, -1)))):  # more records than slots
        assert walk(**kw) == _lib.ERR_ARG, kw
    assert walk(M=1 << 20, W=64) == _lib.ERR_UNSUPPORTED                   # (so the defaults pass every check before this one: the cases above fail for their own reason)
    assert walk(V1=(1 << 20) + 1, blank=4) == _lib.ERR_UNSUPPORTED
    reset = L.mi_ctc_beam_stream_reset_slot
    assert reset(None, 1 << 30, 3, 8, 4, 0, None) == _lib.ERR_ARG
    assert reset(p, 64, 3, 8, 4, 0, None) == _lib.ERR_ARG
    assert reset(p + 4, 1 << 30, 3, 8, 4, 0, None) == _lib.ERR_ARG
    assert reset(p, 1 << 30, 3, 8, 65, 0, None) == _lib.ERR_ARG
    assert reset(p, 1 << 30, 3, 8, 4, 3, None) == _lib.ERR_ARG
    assert reset(p, 1 << 30, 3, 8, 4, -1, None) == _lib.ERR_ARG
    assert reset(p, 1 << 30, 0, 8, 4, 0, None) == _lib.ERR_ARG
    assert reset(p, 1 << 30, 1, 1 << 20, 64, 0, None) == _lib.ERR_UNSUPPORTED


# ---------------------------------------------------------------- the records of a step
def test_pool_records_on_a_hand_written_schedule():
    """TINY: L = 2 layers, r = 15: a slot emits nothing until its front end has passed the lookahead of 30 frames, a finishing slot flushes everything.  The beam's
    record of a slot is (its offset, its count) in the step's compact logits — the last (lo, hi, off) of pool_table's record."""
    from huggingface_asr_amd.streaming import pool_table
    C, L, r = 4, 2, 15
    # slot 2 has had 128 feature frames (32 encoder frames: 2 emitted) and feeds a chunk; slot 0 has had 48 and finishes with 13 more; slot 1 feeds its first chunk
    acts = [(0, 48, 13, True), (1, 0, 16, False), (2, 128, 16, False)]
    records, totals = pool_table(acts, C, L, r)
    rows = [(rec[-1], rec[-2] - rec[-3]) for rec in records]
    assert rows == [(0, 16), (16, 0), (16, 4)] and totals[-1] == 20
    from huggingface_asr_amd import ops
    bp = ops.CtcBeamPool(3, 40, beams=4, blank=4, pad_id=-1)
    for s in range(3):
        bp.open(s)
    bp.walked = [0, 0, 2]
    recs, outs = bp.records([(a[0], off, n, a[3], a[0] == 2) for a, (off, n) in zip(acts, rows)], totals[-1])
    assert recs == [[0, 0, 16, 1, 0], [1, 16, 0, 0, -1], [2, 16, 4, 0, 1]] and outs == {0: 0, 2: 1}
    assert bp.walked == [0, 0, 2] and bp.is_open == [True] * 3             # building records moves nothing
    recs, outs = bp.records([(2, 16, 4, False, False), (0, 0, 16, False, True)], 20)      # any order; the n-best rows follow the record order
    assert recs == [[2, 16, 4, 0, -1], [0, 0, 16, 0, 0]] and outs == {0: 0}


def test_beam_pool_constructor_refusals():
    from huggingface_asr_amd import ops
    ok = dict(beams=4, blank=4, pad_id=0)
    for kw in (dict(beams=0), dict(beams=65), dict(nbest=5), dict(nbest=0), dict(token_topk=0), dict(token_topk=65), dict(blank=-1)):
        with pytest.raises(ValueError):
            ops.CtcBeamPool(2, 16, **dict(ok, **kw))
    for args in ((0, 16), (2, 0)):
        with pytest.raises(ValueError):
            ops.CtcBeamPool(*args, **ok)
    with pytest.raises(ValueError, match="node table"):
        ops.CtcBeamPool(1, 65536, beams=64, blank=4, pad_id=0)
    for kw in (dict(beams=4.0), dict(beams=True), dict(nbest=1.0), dict(token_topk=2.0), dict(dtype=torch.int16)):
        with pytest.raises(TypeError):
            ops.CtcBeamPool(2, 16, **dict(ok, **kw))
    with pytest.raises(TypeError):
        ops.CtcBeamPool(2, 16, blank=4, pad_id=0)                          # beams is required
    for what in ("CtcBeamStream", "CtcBeamPool"):                          # one table, one wording
        with pytest.raises(ValueError, match=what + ": beams must be in 1..64, got 65"):
            getattr(ops, what)(2, 16, **dict(ok, beams=65))


def test_beam_pool_step_refusals_come_before_any_launch():
    """on CPU tensors: whatever is wrong with a step is reported before the device is asked for anything, and the host counts do not move"""
    from huggingface_asr_amd import ops
    bp = ops.CtcBeamPool(3, 16, beams=4, blank=4, pad_id=0)
    x = torch.zeros(12, 5)
    with pytest.raises(RuntimeError, match="open"):
        bp.step(x, [(0, 0, 4, False, False)])                              # never opened
    for s in (0, 1):
        bp.open(s)
    for bad in (3, -1, True, 1.0):
        with pytest.raises(ValueError):
            bp.open(bad)
    with pytest.raises(ValueError, match="no records"):
        bp.step(x, [])
    for bad in (x[None], x.double(), x.long(), "x"):
        with pytest.raises(TypeError):
            bp.step(bad, [(0, 0, 4, False, False)])
    for bad in (torch.zeros(12, 4), torch.zeros(12, 1)):                   # the blank outside; one class
        with pytest.raises(ValueError):
            bp.step(bad, [(0, 0, 4, False, False)])
    for recs in ([(0, 0, 4, False, False), (0, 4, 4, False, False)], [(0, 10, 4, False, False)], [(0, -1, 4, False, False)], [(0, 0, -1, False, False)], [(0, 0, 4, False)]):
        with pytest.raises(ValueError):
            bp.step(x, recs)
    with pytest.raises(TypeError):
        bp.step(x, [(0, 0, 4.0, False, False)])
    for slot in (2, 3, -1):                                                # not open; outside
        with pytest.raises(RuntimeError, match="open"):
            bp.step(x, [(slot, 0, 4, False, False)])
    with pytest.raises(RuntimeError, match="max_frames"):
        bp.step(torch.zeros(17, 5), [(0, 0, 17, False, False)])
    with pytest.raises(RuntimeError, match="device"):                      # a good step, on the CPU: there is no fallback
        bp.step(x, [(0, 0, 4, False, False), (1, 4, 8, True, False)])
    assert bp.walked == [0, 0, 0] and bp.is_open == [True, True, False] and bp._state is None
    bp.walked[0] = 13                                                      # as after 13 frames
    with pytest.raises(RuntimeError, match="max_frames"):
        bp.step(x, [(0, 0, 4, False, False)])
    bp.is_open[1] = False                                                  # as after its final record
    with pytest.raises(RuntimeError, match="open"):
        bp.step(x, [(1, 0, 1, False, False)])
    bp.open(0)
    assert bp.walked == [0, 0, 0] and bp.is_open == [True, False, False]


# ---------------------------------------------------------------- the built kernel
def test_pool_kernel_uses_no_scratch_the_lds_its_header_states_and_at_most_128_vgprs():
    from huggingface_asr_amd import _lib
    _lib.lib()
    header = open(os.path.join(ROOT, "huggingface_asr_amd", "csrc", "ctc_beam_pool.hip")).read()
    stated = int(re.search(r"//\s+ctc_pool_beam_kernel\s.*?(\d+) B of LDS", header).group(1))
    lockstep = open(os.path.join(ROOT, "huggingface_asr_amd", "csrc", "ctc_beam_stream.hip")).read()
    assert stated == int(re.search(r"//\s+ctc_stream_beam_kernel\s.*?(\d+) B of LDS", lockstep).group(1))       # the same LDS as the lock-step kernel
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
            if b"ctc_pool_beam_kernel" not in blob[lo:hi]:
                continue
            with open(fb, "wb") as f:
                f.write(blob[lo:hi])
            subprocess.run([os.path.join(llvm, "clang-offload-bundler"), "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--input={fb}",
                            f"--output={co}"], check=True)
            notes = subprocess.run([os.path.join(llvm, "llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout
            for block in notes.split("- .agpr_count")[1:]:
                name = re.search(r"\.name:\s+(\S*ctc_pool_beam_kernel\S*)", block)
                if name:
                    num = lambda key: int(re.search(r"\." + key + r":\s+(\d+)", block).group(1))
                    found[name.group(1)] = (num("private_segment_fixed_size"), num("group_segment_fixed_size"), num("vgpr_count"))
                assert not re.search(r"\.name:\s+\S*(ctc_walk_kernel|ctc_cut_kernel|ctc_stream_beam_kernel)", block)      # those live in their own translation units
    assert len(found) == 2, sorted(found)                                  # int32 and int64 tokens
    for name, (scratch, lds, vgprs) in found.items():
        assert scratch == 0 and lds == stated and vgprs <= 128, (name, scratch, lds, vgprs)
