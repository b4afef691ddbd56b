"""GPU: the per-slot kernels of csrc/stream_pool.hip, each against its lock-step entry point of csrc/stream.hip called once per slot with B = 1 on the same data —
bit for bit: both run one body (csrc/stream_common.hpp).  Every case holds a slot with zero rows between two live ones, and the slot order is permuted, so that a
compact row offset is never the slot index times anything."""
import ctypes as C

import pytest
import torch

from huggingface_asr_amd import shapes

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF16 = torch.bfloat16


def _rand(shape, seed, dtype=BF16, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dtype).to(DEV).contiguous()


# ------------------------------------------------------------------------------------------------ chunk attention
# (n_q, n_k) per active slot: a fresh slot (n_k = n_q), n_q around the four queries of a block, n_k at the 32-key tile edges, one slot past 1024 keys (LDS beyond 64 KiB)
ATTN_SLOTS = [(4, 4), (0, 10), (1, 32), (3, 33), (5, 64), (4, 65), (3, 1030), (5, 5)]
ATTN_ORDER = [5, 2, 7, 0, 3, 6, 1, 4]          # the state slot of each entry
LMAX = 1040


@pytest.mark.parametrize("ref", [1, 2, 3])
@pytest.mark.parametrize("rel", [False, True], ids=["plain", "rel"])
@pytest.mark.parametrize("hd", [16, 64])
def test_attention_slots_equal_the_lockstep_kernel_per_slot(hd, rel, ref):
    from huggingface_asr_amd import ops
    H = 2
    d = H * hd
    S = len(ATTN_SLOTS)
    cache = _rand((S, LMAX, 2 * d), 1)
    k, v = cache[..., :d], cache[..., d:]
    total = sum(n for n, _ in ATTN_SLOTS)
    q = _rand((total, d), 2)
    pos = _rand((LMAX, d), 3) if rel else None
    u = _rand((d,), 4, torch.float32, 0.5) if rel else None
    vb = _rand((d,), 5, torch.float32, 0.5) if rel else None
    entries, off = [], 0
    for (n_q, n_k), slot in zip(ATTN_SLOTS, ATTN_ORDER):
        entries.append((off, n_q, n_k, slot))
        off += n_q
    got = ops.attention_chunk_slots(q, k, v, entries, H, pos=pos, bias_u=u, bias_v=vb, ref=ref)
    for off, n_q, n_k, slot in entries:
        if n_q == 0:
            continue
        want = ops.attention_chunk(q[off:off + n_q][None], k[slot:slot + 1], v[slot:slot + 1], n_k, H, pos=pos, bias_u=u, bias_v=vb, ref=ref)[0]
        assert torch.equal(got[off:off + n_q], want), (n_q, n_k, slot, float((got[off:off + n_q].float() - want.float()).abs().max()))
    torch.cuda.synchronize()


def test_attention_slots_refuse():
    from huggingface_asr_amd import ops
    cache = _rand((2, 40, 64), 1)
    k, v, q = cache[..., :32], cache[..., 32:], _rand((4, 32), 2)
    with pytest.raises(RuntimeError, match="invalid argument"):
        ops.attention_chunk_slots(q, k, v, [(0, 4, 3, 0)], 2)             # fewer keys than queries
    with pytest.raises(RuntimeError, match="invalid argument"):
        ops.attention_chunk_slots(q, k, v, [(0, 4, 41, 0)], 2)            # past the cache
    with pytest.raises(RuntimeError, match="invalid argument"):
        ops.attention_chunk_slots(q, k, v, [(0, 2, 8, 0), (3, 2, 8, 1)], 2)      # not compact
    with pytest.raises(RuntimeError, match="invalid argument"):
        ops.attention_chunk_slots(q, k, v, [(0, 4, 8, 2)], 2)             # no such slot


# ------------------------------------------------------------------------------------------------ stateful depthwise conv
# per active slot (p, n_new, o0, n_out, end): p = 0; a call whose rows wrap the ring (p % Hr + n_new > Hr); zero rows; n_new > Hr; (merge) the flush: no new rows, an end
CSGU_K, CSGU_DIL = 5, 2                       # left = Hr = 8
CSGU_SLOTS = [(0, 3, 0, 3, None), (6, 5, 6, 5, None), (4, 0, 4, 0, None), (13, 11, 13, 11, None)]
MERGE_K = 5                                   # r = left = 2, Hr = 4
MERGE_SLOTS = [(0, 3, 0, 1, None), (6, 5, 4, 5, None), (4, 0, 2, 0, None), (13, 11, 11, 11, None), (9, 0, 7, 2, 9)]
DW_ORDER = [3, 0, 4, 1, 2]


@pytest.mark.parametrize("mode", ["csgu", "merge", "conv"])
@pytest.mark.parametrize("Cc", [64, 72])
def test_dwconv_slots_equal_the_lockstep_kernel_per_slot(Cc, mode):
    from huggingface_asr_amd import ops
    merge = mode == "merge"
    slots = MERGE_SLOTS if merge else CSGU_SLOTS
    K, dil = (MERGE_K, 1) if merge else (CSGU_K, CSGU_DIL)
    left = (K - 1) // 2 if merge else (K - 1) * dil
    Hr = 2 * left if merge else left
    S = 5
    n_in, n_out = sum(s[1] for s in slots), sum(s[3] for s in slots)
    x = _rand((n_in, Cc), 11)
    w, bias = _rand((Cc, K), 12, torch.float32, 0.3), _rand((Cc,), 13, torch.float32, 0.3)
    ring0 = _rand((S, Hr, Cc), 14)
    kw = {}
    rs0 = None
    if not merge:
        rs0 = _rand((S, (Cc + 63) // 64, Hr, 2), 15, torch.float32).abs() + 0.5
        kw = dict(stats=_rand((n_in, 2), 16, torch.float32).abs() + 0.5, gamma=_rand((Cc,), 17, torch.float32), beta=_rand((Cc,), 18, torch.float32))
    mul = _rand((n_out, Cc), 19) if mode == "csgu" else None
    entries, io, oo = [], 0, 0
    for (p, n_new, o0, n_o, end), slot in zip(slots, DW_ORDER):
        entries.append((slot, io, oo, p, n_new, o0, n_o, ops.NO_END if end is None else end))
        io += n_new
        oo += n_o
    ring, rs = ring0.clone(), None if rs0 is None else rs0.clone()
    got = ops.dwconv_stream_slots(x, w, bias, ring, entries, n_out, mode=mode, K=K, dil=dil, left=left, ring_stats=rs, mul=mul, act=1 if mode == "csgu" else 0, **kw)
    ring_w, rs_w = ring0.clone(), None if rs0 is None else rs0.clone()
    for slot, io, oo, p, n_new, o0, n_o, end in entries:
        if n_new == 0 and n_o == 0:
            continue
        kw1 = {} if merge else dict(stats=kw["stats"][io:io + n_new], gamma=kw["gamma"], beta=kw["beta"], ring_stats=rs_w[slot:slot + 1])
        want = ops.dwconv_stream(x[io:io + n_new][None], w, bias, ring_w[slot:slot + 1], mode=mode, p=p, K=K, dil=dil, left=left, o0=o0, n_out=n_o,
                                 mul=None if mul is None else mul[oo:oo + n_o][None], end=None if end == ops.NO_END else torch.tensor([end]),
                                 act=1 if mode == "csgu" else 0, **kw1)[0]
        assert torch.equal(got[oo:oo + n_o], want), (slot, p, n_new, o0, n_o)
    assert torch.equal(ring, ring_w)                                     # every slot's ring advanced as its own stream's; the idle slot's untouched
    assert torch.equal(ring[DW_ORDER[2]], ring0[DW_ORDER[2]])
    if rs is not None:
        assert torch.equal(rs, rs_w)
    torch.cuda.synchronize()


def test_dwconv_slots_refuse_windows_outside_the_history():
    from huggingface_asr_amd import ops
    x, w, ring = _rand((4, 64), 1), _rand((64, 5), 2, torch.float32), _rand((2, 4, 64), 3)
    ok = (1, 0, 0, 6, 4, 4, 4, ops.NO_END)
    ops.dwconv_stream_slots(x, w, None, ring, [ok], 4, mode="merge", K=5, left=2)
    for bad in [(1, 0, 0, 6, 4, 3, 4, ops.NO_END),          # reads row 1 < p - Hr = 2
                (1, 0, 0, 6, 4, 5, 4, ops.NO_END),          # reads row 10 > p + n_new - 1 without an end
                (2, 0, 0, 6, 4, 4, 4, ops.NO_END)]:         # no such slot
        with pytest.raises(RuntimeError, match="invalid argument"):
            ops.dwconv_stream_slots(x, w, None, ring, [bad], 4, mode="merge", K=5, left=2)
    ops.dwconv_stream_slots(x, w, None, ring, [(1, 0, 0, 10, 4, 9, 5, 14)], 5, mode="merge", K=5, left=2)      # with an end, past the fed rows
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ row copies
def test_copy_rows_slots_wraps_and_indirection():
    from huggingface_asr_amd import ops
    src = torch.arange(3 * 6 * 5, dtype=torch.float32, device=DEV).reshape(3, 6, 5)
    dst = torch.full((4, 7, 5), -1.0, device=DEV)
    entries = [(2, 4, 6, 0, 1, 0, 4),           # wrap on the source side: rows 4, 5, 0, 1 of slot 2
               (1, 0, 0, 1, 0, 0, 0),           # no rows
               (0, 1, 0, 3, 5, 7, 4),           # wrap on the destination side: rows 5, 6, 0, 1 of slot 3
               (1, 0, 0, 2, 2, 0, 3)]           # slot 1 -> slot 2: the slot indices are an indirection, in no order
    want = dst.clone()
    want[0, 1:5] = src[2, [4, 5, 0, 1]]
    want[3, [5, 6, 0, 1]] = src[0, 1:5]
    want[2, 2:5] = src[1, 0:3]
    ops.copy_rows_slots(src, dst, entries)
    assert torch.equal(dst, want)
    narrow = torch.full((4, 7, 5), -1.0, device=DEV)
    ops.copy_rows_slots(src, narrow, entries[:1], W=3)                   # a row's first W words only
    assert torch.equal(narrow[0, 1:5, :3], src[2, [4, 5, 0, 1], :3]) and bool((narrow[0, 1:5, 3:] == -1).all())
    for bad in [(3, 0, 0, 0, 0, 0, 1), (0, 5, 0, 0, 0, 0, 2), (0, 0, 0, 0, 6, 0, 2), (0, 0, 7, 0, 0, 0, 1), (0, 0, 0, 0, 0, 7, 8)]:
        with pytest.raises(RuntimeError, match="invalid argument"):
            ops.copy_rows_slots(src, dst, [bad])


# ------------------------------------------------------------------------------------------------ rotary
def test_rotary_slots_positions():
    from huggingface_asr_amd import ops
    from huggingface_asr_amd.packing import rotary_tables
    H, hd, tmax = 2, 16, 4100
    cos, sin = (t.to(DEV).contiguous() for t in rotary_tables(tmax, hd, 10000))
    x = _rand((10, H * hd), 21)
    entries = [(0, 3, 0), (3, 0, 11), (3, 5, 7), (8, 2, 4095)]
    got = ops.rotary_slots(x, cos, sin, entries, H)
    for off, n, p in entries:
        if n:
            want = ops.rotary(x[off:off + n], cos[p:], sin[p:], n, H)   # the lock-step call: a table that starts at p, position = row % n
            assert torch.equal(got[off:off + n], want), p
    with pytest.raises(RuntimeError, match="invalid argument"):
        ops.rotary_slots(x, cos, sin, [(0, 2, tmax - 1)], H)              # past the table


# ------------------------------------------------------------------------------------------------ collapse
def test_collapse_slots_carried_classes():
    from huggingface_asr_amd import ops
    blank = 50
    g = torch.Generator().manual_seed(31)
    long = torch.randint(47, 51, (70,), generator=g)                     # few classes: many repeats and blanks, more than one ballot of 64
    best = torch.cat([torch.tensor([5, 5, 3, blank, 3]), long]).to(torch.int32).to(DEV)
    prev = torch.tensor([9, -1, 5], dtype=torch.int32, device=DEV)
    entries = [(2, 0, 5),                       # the first frame repeats the carried class 5
               (0, 5, 0),                       # no frames: the carried class 9 must survive
               (1, 5, 70)]
    want_prev = prev.clone()
    ids, n = ops.ctc_collapse_slots(best, blank, prev, entries)
    for (slot, off, cnt), k in zip(entries, range(3)):
        if cnt == 0:
            assert int(n[k]) == 0
            continue
        w_ids, w_n = ops.ctc_collapse_stream(best[off:off + cnt][None], blank, want_prev[slot:slot + 1])
        assert torch.equal(ids[off:off + cnt], w_ids[0]) and int(n[k]) == int(w_n[0])
    assert ids[:5].tolist() == [3, 3, -1, -1, -1] and int(n[0]) == 2
    assert torch.equal(prev, want_prev) and prev.tolist() == [9, int(long[-1]), 3]
    with pytest.raises(RuntimeError, match="invalid argument"):
        ops.ctc_collapse_slots(best, blank, prev, [(1, 0, 5), (1, 5, 5)])          # one carried class, two entries


# ------------------------------------------------------------------------------------------------ per-slot reset
def test_reset_slot_touches_one_slot_only():
    from helpers import seeded_state_dict, synth_feats
    from huggingface_asr_amd import _lib
    from huggingface_asr_amd.engine import EBranchformerEngine
    cfg = dict(shapes.TINY, is_causal=True)
    eng = EBranchformerEngine(cfg, DEV)
    eng.load_state_dict(seeded_state_dict(cfg, 44))
    x, _ = synth_feats(44, 3, 160, [160, 160, 160])
    pool = eng.stream_pool(3, 4, 64)
    sids = [pool.open() for _ in range(3)]
    for t in range(10):                                                  # 40 frames: every ring has wrapped, every cache and history holds data
        pool.step(feed={s: x[s, 16 * t:16 * t + 16].to(DEV) for s in sids})
    cs = pool._config()
    n = _lib.lib().mi_ebf_stream_slot_pieces(C.byref(cs), 4, 64, None, 0)
    out = (C.c_long * (2 * n))()
    assert _lib.lib().mi_ebf_stream_slot_pieces(C.byref(cs), 4, 64, out, n) == n
    before = pool._state.clone()
    fresh_pool = eng.stream_pool(3, 4, 64)
    fresh_pool._ensure_state()
    fresh = fresh_pool._state
    rc = _lib.lib().mi_ebf_stream_reset_slot(C.byref(cs), 4, 64, pool._state.data_ptr(), pool._state.numel(), 1, torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    after = pool._state
    touched = torch.zeros_like(before, dtype=torch.bool)
    for k in range(n):
        off, size = out[2 * k], out[2 * k + 1]
        for s in (0, 2):
            assert torch.equal(after[off + s * size: off + (s + 1) * size], before[off + s * size: off + (s + 1) * size]), (k, s)
        assert not torch.equal(before[off + size: off + 2 * size], fresh[off + size: off + 2 * size]), f"piece {k} of slot 1 was never written: the test shows nothing"
        assert torch.equal(after[off + size: off + 2 * size], fresh[off + size: off + 2 * size]), k
        touched[off + size: off + 2 * size] = True
    assert torch.equal(after[~touched], before[~touched])                # and nothing else anywhere in the state
    assert _lib.lib().mi_ebf_stream_reset_slot(C.byref(cs), 4, 64, pool._state.data_ptr(), pool._state.numel(), 3, torch.cuda.current_stream().cuda_stream) == _lib.ERR_ARG
