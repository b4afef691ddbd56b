"""The host side of the streaming session pool (huggingface_asr_amd/streaming.py StreamPool / pool_table; csrc/stream_pool.hip states the semantics): per-slot row
ranges, compact offsets and slot bookkeeping over a random schedule, the refusals before any launch, and the host-only C queries.  No GPU here."""
import ctypes as C
import random

import pytest
import torch

from huggingface_asr_amd import shapes
from huggingface_asr_amd.engine import EBranchformerEngine
from huggingface_asr_amd.streaming import causal_out_frames, plan, pool_table

CAUSAL = dict(shapes.TINY, is_causal=True)


def _engine(cfg, **kw):
    return EBranchformerEngine(cfg, device="cpu", **kw)


@pytest.fixture(scope="module")
def built():
    from huggingface_asr_amd.csrc import build as B
    return B.build()


# ------------------------------------------------------------------ a random schedule: open, feed, idle, finish with tails 0 .. 4C, reuse
@pytest.mark.parametrize("r", [1, 15])
def test_random_schedule_rows_offsets_and_reuse(built, r):
    from huggingface_asr_amd import _lib
    S, Cf, L = 4, 4, 2
    W = 4 * Cf
    pool = _engine(dict(CAUSAL, merge_conv_kernel=2 * r + 1)).stream_pool(S, Cf, 400)
    assert (pool.L, pool.r) == (L, r)
    cs = pool._config()
    rng = random.Random(100 + r)
    hist = {}                                            # slot -> feature frames its session has had (our own count, not the pool's)
    chunk = torch.zeros(W, 80)
    finishes = reuses = idles = 0
    freed = set()
    for step in range(300):
        if len(hist) < S and rng.random() < 0.35:
            sid = pool.open()
            assert sid not in hist and pool.n_feat[sid] == 0 and pool.total[sid] == 0          # a freed slot restarts at zero
            reuses += sid in freed
            hist[sid] = 0
        feed, finish = {}, {}
        for sid in sorted(hist):
            u = rng.random()
            if u < 0.2:
                idles += 1
            elif u < 0.3 or hist[sid] + W > 4 * 300:
                t = rng.choice([0, 1, 2, 3, W - 1, W, rng.randrange(W + 1)])
                finish[sid] = None if t == 0 and rng.random() < 0.5 else torch.zeros(t, 80)
            else:
                feed[sid] = chunk
        acts = pool.actions(feed, finish)
        assert [a[0] for a in acts] == sorted(set(feed) | set(finish))
        if not acts:
            assert pool.step(feed, finish) == {}
            continue
        records, totals = pool_table([a[:4] for a in acts], Cf, L, r)
        sums = [0] * (L + 1)
        for (sid, n_prev, n, fin, _), rec in zip(acts, records):
            assert n_prev == hist[sid] and n == (W if sid in feed else (0 if finish[sid] is None else finish[sid].shape[0]))
            own = plan(n_prev + n, Cf, L, r, fin, n_prev=n_prev)                               # the slot's rows are plan() of its own history
            assert rec[0] == sid and rec[1] == (causal_out_frames(n_prev + n) if fin else -1)
            for l, (lo, hi) in enumerate(own):
                assert rec[2 + 3 * l: 5 + 3 * l] == [lo, hi, sums[l]]                         # compact offsets are the prefix sums
                sums[l] += hi - lo
            if fin:
                assert all(hi == causal_out_frames(n_prev + n) for _, hi in own)               # its own end, not a batch maximum
        assert sums == totals and max(totals) <= S * (Cf + L * r)
        # the C side accepts exactly these records and sizes the device table from them
        rec_t = torch.tensor(records, dtype=torch.int32)
        words = _lib.lib().mi_ebf_stream_slots_table(C.byref(cs), Cf, 400, rec_t.data_ptr(), len(acts), None, 0)
        assert words > 0 and words % len(acts) == 0
        table = torch.full((words,), -7, dtype=torch.int32)
        assert _lib.lib().mi_ebf_stream_slots_table(C.byref(cs), Cf, 400, rec_t.data_ptr(), len(acts), table.data_ptr(), words) == words
        assert int((table == -7).sum()) == 0                                                   # every word written
        assert _lib.lib().mi_ebf_stream_slots_table(C.byref(cs), Cf, 400, rec_t.data_ptr(), len(acts), table.data_ptr(), words - 1) == _lib.ERR_ARG
        res = pool._advance(acts, records)
        for (sid, n_prev, n, fin, _), rec in zip(acts, records):
            hist[sid] = n_prev + n
            assert res[sid] == (rec[-2] - rec[-3], pool.total[sid], fin) and pool.n_feat[sid] == hist[sid]
            if fin:
                assert pool.total[sid] == causal_out_frames(hist[sid]) and not pool.is_open[sid]
                del hist[sid]
                freed.add(sid)
                finishes += 1
    assert finishes > 10 and reuses > 5 and idles > 20, (finishes, reuses, idles)


def test_table_sections_of_one_step(built):
    """the expansion of two records, read back word for word: the K | V append at the slot's own p, the pending ring's modulus, the merge conv's end"""
    from huggingface_asr_amd import _lib
    Cf, L, r, S = 4, 2, 15, 3
    pool = _engine(CAUSAL).stream_pool(S, Cf, 400)
    cs = pool._config()
    records, totals = pool_table([(2, 160, 16, False), (0, 32, 5, True)], Cf, L, r)
    rec_t = torch.tensor(records, dtype=torch.int32)
    words = _lib.lib().mi_ebf_stream_slots_table(C.byref(cs), Cf, 400, rec_t.data_ptr(), 2, None, 0)
    t = torch.zeros(words, dtype=torch.int32)
    assert _lib.lib().mi_ebf_stream_slots_table(C.byref(cs), Cf, 400, rec_t.data_ptr(), 2, t.data_ptr(), words) == words
    t = t.tolist()
    A, N = 2, Cf + L * r
    assert words == A * (6 * 7 + L * 44 + 3)
    assert t[0:14] == [2, 0, 0, 0, 0, 0, 2, 0, 0, 0, 1, 0, 0, 2]                              # history rows of slots 2 and 0 in front of entries 0 and 1
    assert t[5 * 14: 6 * 14] == [0, 0, 0, 0, 0, 0, 4, 1, 0, 0, 0, 4, 0, 2]                     # 4 and 2 new frames, compact
    lay0 = A * 42
    assert t[lay0 + 14: lay0 + 28] == [0, 0, 0, 2, 40, 0, 4, 0, 4, 0, 0, 8, 0, 2]              # K | V rows at p = 40 of slot 2 and p = 8 of slot 0
    assert t[lay0: lay0 + 7] == [0, 0, 0, 2, 40, r + N, 4]                                     # the pending ring wraps at r + N
    att = lay0 + 3 * 14
    assert t[att: att + 8] == [0, 4, 44, 2, 4, 2, 10, 0]                                       # (first query, n_q, n_k, slot)
    mrg = att + 8 + 16
    assert t[mrg + 7] == 0x7FFFFFFF and t[mrg + 15] == 10                                      # only the finishing slot has an end: its own
    assert t[mrg + 8: mrg + 15] == [0, 4, records[1][7], 8, 2, 0, 10]                          # slot 0 flushes rows 0 .. 10 of layer 0's output
    assert t[-6:] == [2, 0, records[0][-2] - records[0][-3], 0, records[1][-1], 10]


# ------------------------------------------------------------------ refusals, before any launch
def test_refuses_what_stream_refuses():
    with pytest.raises(ValueError, match="causal"):
        _engine(dict(shapes.TINY)).stream_pool(2, 4, 100)
    with pytest.raises(NotImplementedError, match="fp32"):
        _engine(CAUSAL, precision="fp32").stream_pool(2, 4, 100)
    with pytest.raises(NotImplementedError, match="mixing"):
        _engine(dict(CAUSAL, finetune_with_layer_mixing=True)).stream_pool(2, 4, 100)
    with pytest.raises(NotImplementedError, match="additional"):
        _engine(dict(CAUSAL, finetune_with_additional_layer=True)).stream_pool(2, 4, 100)
    with pytest.raises(NotImplementedError, match="head size"):
        _engine(dict(CAUSAL, num_attention_heads=2)).stream_pool(2, 4, 100)
    with pytest.raises(NotImplementedError, match="3 x 3"):
        _engine(dict(CAUSAL, conv_kernel=[5, 5], conv_padding=[2, 2])).stream_pool(2, 4, 100)
    with pytest.raises(ValueError, match="max_frames"):
        _engine(CAUSAL).stream_pool(2, 4, 8193)
    with pytest.raises(ValueError, match="slots"):
        _engine(CAUSAL).stream_pool(0, 4, 100)
    with pytest.raises(NotImplementedError, match="beams"):
        _engine(CAUSAL).stream_pool(2, 4, 100, beams=4)


def test_refuses_bad_calls():
    pool = _engine(CAUSAL).stream_pool(2, 4, 6)
    a, b = pool.open(), pool.open()
    assert (a, b) == (0, 1)
    with pytest.raises(RuntimeError, match="slots"):
        pool.open()                                               # a full pool
    with pytest.raises(ValueError, match="chunk"):
        pool.step(feed={a: torch.zeros(15, 80)})                  # not 4 * C frames
    with pytest.raises(ValueError, match="chunk"):
        pool.step(feed={a: torch.zeros(1, 16, 80)})               # a batch is not a chunk
    with pytest.raises(ValueError, match="tail"):
        pool.step(finish={a: torch.zeros(17, 80)})                # a tail longer than 4 C
    with pytest.raises(ValueError, match="both"):
        pool.step(feed={a: torch.zeros(16, 80)}, finish={a: None})
    with pytest.raises(RuntimeError, match="no open session"):
        pool.step(feed={5: torch.zeros(16, 80)})                  # no such slot
    pool.n_feat[a] = 16                                           # as after one chunk: 4 frames; the next chunk would make 8 > max_frames = 6
    with pytest.raises(RuntimeError, match="max_frames"):
        pool.step(feed={a: torch.zeros(16, 80)})
    pool.is_open[b] = False                                       # as after its finish
    with pytest.raises(RuntimeError, match="no open session"):
        pool.step(feed={b: torch.zeros(16, 80)})                  # feeding a finished (free) slot
    with pytest.raises(RuntimeError, match="no open session"):
        pool.step(finish={b: None})
    assert pool.open() == b                                       # ... which open() hands out again
    with pytest.raises(RuntimeError, match="device"):
        pool.step(finish={b: None})                               # valid, but there is no CPU path


def test_model_surface_refuses_training_and_cpu():
    from huggingface_asr_amd.configuration_ebranchformer import Wav2Vec2EBranchformerConfig
    from huggingface_asr_amd.modeling_ebranchformer import Wav2Vec2EBranchformerForCTC
    m = Wav2Vec2EBranchformerForCTC(Wav2Vec2EBranchformerConfig(**CAUSAL)).train()
    with pytest.raises(RuntimeError, match="eval"):
        m.stream_pool(2, 4, 100)
    with pytest.raises(RuntimeError, match="GPU"):
        m.eval().stream_pool(2, 4, 100)


# ------------------------------------------------------------------ the C side's host-only queries and checks
def test_state_bytes_and_pieces_on_cpu(built):
    from huggingface_asr_amd import _lib
    eng = _engine(dict(shapes.SMALL, is_causal=True))
    pool = eng.stream_pool(3, 16, 1000)
    assert pool.state_bytes() == eng.stream(3, 16, 1000).state_bytes() > 0                     # the lock-step state of B = slots serves the pool
    cs = pool._config()
    n = _lib.lib().mi_ebf_stream_slot_pieces(C.byref(cs), 16, 1000, None, 0)
    L, d, I = 12, 256, shapes.SMALL["intermediate_size"]
    assert n == 3 + 5 * L
    out = (C.c_long * (2 * n))()
    assert _lib.lib().mi_ebf_stream_slot_pieces(C.byref(cs), 16, 1000, out, n) == n
    assert _lib.lib().mi_ebf_stream_slot_pieces(C.byref(cs), 16, 1000, out, n - 1) == _lib.ERR_ARG
    off, size = list(out[0::2]), list(out[1::2])
    assert size[0] == 2 * 80 * 4 and size[2] == 4 and size[3] == 1000 * 2 * d * 2
    r = (shapes.SMALL.get("merge_conv_kernel", 31) - 1) // 2
    assert size[6] == 2 * r * 2 * d * 2 and size[7] == (r + 16 + L * r) * d * 4
    for k in range(n - 1):                                                                     # pieces in order, the slots' slices inside their piece
        assert off[k] + 3 * size[k] <= off[k + 1]
    assert off[-1] + 3 * size[-1] <= pool.state_bytes()


def test_records_refused_on_the_host(built):
    from huggingface_asr_amd import _lib
    Cf, L, r = 4, 2, 15
    pool = _engine(CAUSAL).stream_pool(3, Cf, 40)
    cs = pool._config()

    def rc(records, A=None):
        t = torch.tensor(records, dtype=torch.int32)
        return _lib.lib().mi_ebf_stream_slots_table(C.byref(cs), Cf, 40, t.data_ptr(), len(records) if A is None else A, None, 0)

    good, _ = pool_table([(0, 32, 16, False), (2, 0, 16, False)], Cf, L, r)
    assert rc(good) > 0
    bad = [list(x) for x in good]; bad[0][2], bad[0][3] = good[0][3], good[0][2]               # frontiers that decrease
    assert rc(bad) == _lib.ERR_ARG
    bad = [list(x) for x in good]; bad[1][0] = 0                                               # a slot named twice
    assert rc(bad) == _lib.ERR_ARG
    bad = [list(x) for x in good]; bad[1][0] = 3                                               # no such slot
    assert rc(bad) == _lib.ERR_ARG
    bad = [list(x) for x in good]; bad[1][4] = 1                                               # an offset that is not the prefix sum
    assert rc(bad) == _lib.ERR_ARG
    far, _ = pool_table([(1, 160, 16, False)], Cf, L, r)                                       # 44 frames > max_frames = 40
    assert rc(far) == _lib.ERR_ARG
    assert rc(good, A=4) == _lib.ERR_ARG                                                       # more records than slots
    fin, _ = pool_table([(1, 32, 5, True)], Cf, L, r)
    assert rc(fin) > 0
    bad = [list(x) for x in fin]; bad[0][1] += 1                                               # an end that is not the slot's own
    assert rc(bad) == _lib.ERR_ARG
