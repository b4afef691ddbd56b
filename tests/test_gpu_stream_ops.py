"""GPU: the three kernels of csrc/stream.hip on their own.

Stateful depthwise conv: integer operands (dwconv_ref.int_inputs' ranges: every sum exact in any order), so the output concatenated over ANY partition of the
sequence into calls must EQUAL the reference — calls of one row, calls longer than the history, the whole sequence in one call, sequences of >= 3 rings so the ring
wraps, ragged ends at the flush.  Chunk attention: a float64 restatement on the same bf16 operands under the bound of tests/attention_cases.py (d_tolerance), exact
selector cases, and the chunked walk against mi_attention_qkv_bf16(causal=1).  Streaming collapse: Python groupby over the concatenation."""
import itertools
import math

import pytest
import torch

import attention_cases as AC
import dwconv_ref as DR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF16 = torch.bfloat16
F64 = torch.float64


def _dev(x, dtype):
    return x.to(dtype).to(DEV).contiguous()


def _parts(T, sizes):
    out, pos = [], 0
    for s in itertools.cycle(sizes):
        if pos >= T:
            return out
        out.append(min(s, T - pos))
        pos += out[-1]


# ------------------------------------------------------------------------------------------------ stateful conv, CSGU / conv-only
CSGU_K, CSGU_DIL = 31, 15
CSGU_REACH = (CSGU_K - 1) * CSGU_DIL          # 450 rows of history
CSGU_T = 1400                                 # > 3 rings
CSGU_PARTS = {"ones-then-mixed": [1, 1, 1, 7, 451, 64, 1, 449, 450], "longer-than-history": [700, 451], "whole": [CSGU_T]}


@pytest.fixture(scope="module")
def csgu_ref():
    out = {}
    for C in (64, 1024):
        case = DR.Case(f"stream-csgu-C{C}", "csgu", 2, CSGU_T, C, CSGU_K, CSGU_REACH, CSGU_DIL, "contig")
        inp = DR.int_inputs(case)
        g = torch.Generator().manual_seed(C)
        inp["stats"][:, 0] = torch.randint(-1, 2, (case.B * case.T,), generator=g).to(F64)       # a mean per row: the ring must carry the statistics too
        a = (inp["u"], inp["stats"], inp["gamma"], inp["beta"], inp["w"], inp["bias"])
        out[C] = (case, inp, DR.csgu_fwd(*a, case.B, case.T, case.pad, case.dil, 0, gated=True), DR.csgu_fwd(*a, case.B, case.T, case.pad, case.dil, 0, gated=False))
    return out


@pytest.mark.parametrize("mode", ["csgu", "conv"])
@pytest.mark.parametrize("part", list(CSGU_PARTS))
@pytest.mark.parametrize("C", [64, 1024])
def test_csgu_stream_equals_reference(csgu_ref, C, part, mode):
    from huggingface_asr_amd import ops
    case, inp, want_g, want_c = csgu_ref[C]
    B, T = case.B, case.T
    u = _dev(inp["u"].view(B, T, 2 * C), BF16)
    stats = _dev(inp["stats"].view(B, T, 2), torch.float32)
    gamma, beta, w, bias = (_dev(inp[k], torch.float32) for k in ("gamma", "beta", "w", "bias"))
    ring = torch.zeros(B, CSGU_REACH, C, dtype=BF16, device=DEV)
    rstats = torch.zeros(B, (C + 63) // 64, CSGU_REACH, 2, dtype=torch.float32, device=DEV)
    outs, p = [], 0
    for n in _parts(T, CSGU_PARTS[part]):
        chunk = u[:, p:p + n].contiguous()
        outs.append(ops.dwconv_stream(chunk[..., C:], w, bias, ring, mode=mode, p=p, K=CSGU_K, dil=CSGU_DIL, left=CSGU_REACH, o0=p, n_out=n, ring_stats=rstats,
                                      stats=stats[:, p:p + n].contiguous(), gamma=gamma, beta=beta, mul=chunk[..., :C] if mode == "csgu" else None))
        p += n
    got = torch.cat(outs, 1).double().cpu()
    want = (want_g if mode == "csgu" else want_c).view(B, T, C)
    assert torch.equal(got, want), float((got - want).abs().max())


# ------------------------------------------------------------------------------------------------ stateful conv, MERGE with lookahead and ragged ends
MERGE_T = 200
MERGE_ENDS = [200, 173]
MERGE_PARTS = {"ones-then-mixed": [1, 1, 1, 5, 64, 31, 1, 30, 2], "longer-than-history": [90, 64], "whole": [MERGE_T]}


@pytest.fixture(scope="module")
def merge_ref():
    out = {}
    for K, C in itertools.product((31, 3), (128, 1024)):
        case = DR.Case(f"stream-merge-K{K}-C{C}", "merge", 2, MERGE_T, C, K, (K - 1) // 2, 1, "contig")
        inp = DR.int_inputs(case)
        m = inp["m"].view(2, MERGE_T, C)
        # each stream alone, cut at its end; and uncut
        want = {tuple(ends): [DR.merge_fwd(m[b, :n], inp["w"], inp["bias"], 1, n, case.pad) for b, n in enumerate(ends)] for ends in (MERGE_ENDS, [MERGE_T, MERGE_T])}
        out[K, C] = (case, inp, want)
    return out


@pytest.mark.parametrize("flush", ["with-last-rows", "own-call"])
@pytest.mark.parametrize("part", list(MERGE_PARTS))
@pytest.mark.parametrize("K,C", [(31, 128), (31, 1024), (3, 128), (3, 1024)])
def test_merge_stream_equals_reference(merge_ref, K, C, part, flush):
    from huggingface_asr_amd import ops
    case, inp, want = merge_ref[K, C]
    B, T, r = case.B, case.T, (K - 1) // 2
    # a stream ends inside the LAST call that brings rows: ragged ends go with the flush that has rows; a flush of its own (no new rows) ends every stream where the rows end
    ends = MERGE_ENDS if flush == "with-last-rows" else [T, T]
    want = want[tuple(ends)]
    m = _dev(inp["m"].view(B, T, C), BF16)          # stream 1's rows beyond its end are fed as they are (non-zero): `end` must mask them
    w, bias = _dev(inp["w"], torch.float32), _dev(inp["bias"], torch.float32)
    ring = torch.zeros(B, 2 * r, C, dtype=BF16, device=DEV)
    end = torch.tensor(ends, dtype=torch.int32, device=DEV)
    parts = _parts(T, MERGE_PARTS[part])
    outs, p, emitted = [], 0, 0
    for i, n in enumerate(parts):
        last = i + 1 == len(parts) and flush == "with-last-rows"
        hi = p + n
        o1 = hi if last else max(0, hi - r)
        outs.append(ops.dwconv_stream(m[:, p:hi].contiguous(), w, bias, ring, mode="merge", p=p, K=K, left=r, o0=emitted, n_out=o1 - emitted, end=end if last else None))
        p, emitted = hi, o1
    if flush == "own-call":
        outs.append(ops.dwconv_stream(m[:, T:T], w, bias, ring, mode="merge", p=T, K=K, left=r, o0=emitted, n_out=T - emitted, end=end))
    got = torch.cat(outs, 1).double().cpu()
    assert got.shape[1] == T
    for b, n in enumerate(ends):
        assert torch.equal(got[b, :n], want[b]), (b, float((got[b, :n] - want[b]).abs().max()))


def test_dwconv_stream_refuses_windows_outside_its_history():
    from huggingface_asr_amd import ops
    x = torch.zeros(1, 4, 64, dtype=BF16, device=DEV)
    w, ring = torch.zeros(64, 3, device=DEV), torch.zeros(1, 2, 64, dtype=BF16, device=DEV)
    with pytest.raises(RuntimeError, match="invalid argument"):
        ops.dwconv_stream(x, w, None, ring, mode="merge", p=10, K=3, left=1, o0=8, n_out=2)        # row 7 left the 2-row history
    with pytest.raises(RuntimeError, match="invalid argument"):
        ops.dwconv_stream(x, w, None, ring, mode="merge", p=10, K=3, left=1, o0=10, n_out=4)       # row 14 is not fed yet and this is no flush


# ------------------------------------------------------------------------------------------------ chunk attention
def _attn_ref(q, k, v, n_k, H, pos=None, u=None, vb=None, scale=None):
    """float64 on the same bf16 operands: q (B, n_q, d), k / v (B, >= n_k, d), pos (>= n_k, d) by distance"""
    B, n_q, d = q.shape
    hd = d // H
    scale = 1.0 / math.sqrt(hd) if scale is None else scale
    qh = q.double().view(B, n_q, H, hd).transpose(1, 2)
    kh = k[:, :n_k].double().reshape(B, n_k, H, hd).transpose(1, 2)
    vh = v[:, :n_k].double().reshape(B, n_k, H, hd).transpose(1, 2)
    i = torch.arange(n_k - n_q, n_k)[:, None]
    j = torch.arange(n_k)[None, :]
    if pos is not None:
        qu = (qh.float() + u.view(1, H, 1, hd)).to(BF16).double()         # the kernel's A operands: bf16(q + u), bf16(q + v)
        qv = (qh.float() + vb.view(1, H, 1, hd)).to(BF16).double()
        ph = pos[:n_k].double().reshape(n_k, H, hd).transpose(0, 1)
        bd = torch.gather(qv @ ph.transpose(-2, -1)[None], 3, (i - j).clamp(min=0)[None, None].expand(B, H, n_q, n_k))
        s = (qu @ kh.transpose(-2, -1) + bd) * scale
    else:
        s = (qh @ kh.transpose(-2, -1)) * scale
    s = s.masked_fill((j > i)[None, None], float("-inf"))
    return (torch.softmax(s, -1) @ vh).transpose(1, 2).reshape(B, n_q, d)


# (keys in the cache before the call, new rows): an empty cache, the 32 / 128 / 1500 edges, n_q in {1, 16, 195}, more new rows than cached ones
ATTN_SHAPES = [(0, 1), (0, 16), (0, 195), (31, 2), (127, 2), (1499, 1), (100, 16), (50, 195), (1305, 195)]


@pytest.mark.parametrize("rel", [False, True], ids=["plain", "rel"])
@pytest.mark.parametrize("hd", [16, 64, 128])
@pytest.mark.parametrize("before,n_q", ATTN_SHAPES)
def test_attention_chunk_vs_float64(before, n_q, hd, rel):
    _attention_vs_float64(before, n_q, hd, rel, 0)


@pytest.mark.parametrize("ref", [1, 2, 3])
@pytest.mark.parametrize("before,n_q", [(0, 16), (31, 2), (1305, 195)])
def test_attention_chunk_vs_float64_with_the_full_kernels_references(before, n_q, ref):
    """the rounding of the probabilities follows another kernel's walk over 32-key tiles: the same quotient, the same bound"""
    _attention_vs_float64(before, n_q, 64, True, ref)


def _attention_vs_float64(before, n_q, hd, rel, ref):
    from huggingface_asr_amd import ops
    B, H, Lmax = 2, 2, 1504
    d, n_k = H * hd, before + n_q
    g = torch.Generator().manual_seed(before * 1000 + n_q + hd)
    rn = lambda *s: torch.randn(*s, generator=g)
    q, kv = rn(B, n_q, d).to(BF16), rn(B, Lmax, 2 * d).to(BF16)
    pos, u, vb = (rn(Lmax, d).to(BF16), 0.5 * rn(d), 0.5 * rn(d)) if rel else (None, None, None)
    dv = lambda t: None if t is None else t.to(DEV)
    kvd = kv.to(DEV)
    got = ops.attention_chunk(q.to(DEV), kvd[..., :d], kvd[..., d:], n_k, H, pos=dv(pos), bias_u=dv(u), bias_v=dv(vb), ref=ref).double().cpu()
    want = _attn_ref(q, kv[..., :d], kv[..., d:], n_k, H, pos, u, vb)
    err = AC.d_normalised_error(got, want)
    assert float(err.max()) <= AC.D_C, float(err.max())


@pytest.mark.parametrize("ref", [0, 1, 2, 3])
@pytest.mark.parametrize("rel", [False, True], ids=["content", "position"])
@pytest.mark.parametrize("hd", [16, 64, 128])
@pytest.mark.parametrize("where", ["distance0", "first-row", "farthest"])
def test_attention_chunk_selects_exactly(where, hd, rel, ref):
    """one allowed key outweighs every other by >= 128 in the exponent's argument (scale 1; q = 16, the winner's entry >= 8 above the others), so with the maximum
    subtracted exp of the rest is exactly 0 in fp32 and the output must EQUAL that key's value row.  In the content / distance-0 case every later row of the chunk
    carries a larger key: it would win if the causal mask let it through."""
    from huggingface_asr_amd import ops
    B, H, before, n_q, Lmax = 2, 2, 70, 9, 96
    d, n_k = H * hd, before + n_q
    g = torch.Generator().manual_seed(hd + 7 * rel)
    ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g).float()
    v = ri(-8, 8, B, Lmax, d)
    q = torch.zeros(B, n_q, d)
    k = torch.zeros(B, Lmax, d)
    pos = torch.zeros(Lmax, d)
    win = torch.zeros(B, H, n_q, dtype=torch.long)
    checked = torch.ones(n_q, dtype=torch.bool)
    for h in range(H):
        c0 = h * hd + (h % hd)                                  # the one column of the head that carries the score
        q[:, :, c0] = 16.0
        for i in range(n_q):
            ia = before + i
            win[:, h, i] = {"distance0": ia, "first-row": 0, "farthest": 0}[where]
        if rel:                                                 # the position term selects a distance; the content term is small noise
            k[:, :, c0] = ri(-1, 1, B, Lmax)
            if where == "distance0":
                pos[0, c0] = 16.0
            else:                                               # distance n_k - 1 exists for the last query only (its key is the cache's first row)
                pos[n_k - 1, c0] = 16.0
                checked[: n_q - 1] = False
        else:
            k[:, :, c0] = ri(-1, 1, B, Lmax)
            if where == "distance0":                            # the chunk's keys grow by 8 per row (16 * 8 = 128 in the exponent): every LATER row of the chunk would win if unmasked
                for i in range(n_q):
                    k[:, before + i, c0] = 16.0 + 8.0 * i
            else:
                k[:, 0, c0] = 16.0
    zeros = torch.zeros(d)
    kv = torch.cat([k, v], -1).to(BF16).to(DEV)
    got = ops.attention_chunk(q.to(BF16).to(DEV), kv[..., :d], kv[..., d:], n_k, H, pos=pos.to(BF16).to(DEV) if rel else None, bias_u=zeros.to(DEV) if rel else None,
                              bias_v=zeros.to(DEV) if rel else None, scale=1.0, ref=ref).float().cpu()
    for b, h, i in itertools.product(range(B), range(H), range(n_q)):
        if not checked[i]:
            continue
        want = v[b, win[b, h, i], h * hd:(h + 1) * hd]
        assert torch.equal(got[b, i, h * hd:(h + 1) * hd], want), (b, h, i)


def test_attention_chunk_walk_matches_the_full_causal_kernel():
    """a sequence fed in chunks of 16 rows against mi_attention_qkv_bf16(causal=1) on the same q, k, v and projected positions: twice the bound of the float64 test"""
    from huggingface_asr_amd import ops
    B, H, hd, T, C = 2, 2, 64, 160, 16
    d = H * hd
    g = torch.Generator().manual_seed(5)
    rn = lambda *s: torch.randn(*s, generator=g)
    qkv = rn(B * T, 3 * d).to(BF16).to(DEV)
    table = rn(2 * T - 1, d).to(BF16).to(DEV)                    # row T - 1 - (i - j)
    u, vb = (0.5 * rn(d)).to(DEV), (0.5 * rn(d)).to(DEV)
    full = ops.attention_qkv(qkv, B, T, H, pos=table, bias_u=u, bias_v=vb, causal=True).view(B, T, d)
    dist = table[:T].flip(0).contiguous()                        # row k = distance k
    x = qkv.view(B, T, 3 * d)
    cache = x[..., d:].contiguous()                              # the walk appends nothing: rows beyond n_k are never read
    # ref 2: head size 64 with relative positions runs the four-wave kernel in the full forward
    outs = [ops.attention_chunk(x[:, p:p + C, :d], cache[..., :d], cache[..., d:], p + C, H, pos=dist, bias_u=u, bias_v=vb, ref=2) for p in range(0, T, C)]
    got = torch.cat(outs, 1)
    err = AC.d_normalised_error(got.cpu(), full.cpu())
    assert float(err.max()) <= 2 * AC.D_C, float(err.max())


def test_attention_chunk_refuses():
    from huggingface_asr_amd import ops
    q = torch.zeros(1, 4, 64, dtype=BF16, device=DEV)
    kv = torch.zeros(1, 16, 128, dtype=BF16, device=DEV)
    with pytest.raises(RuntimeError, match="invalid argument"):
        ops.attention_chunk(q, kv[..., :64], kv[..., 64:], 3, 2)             # fewer keys than new rows
    with pytest.raises(RuntimeError, match="unsupported"):
        ops.attention_chunk(q, kv[..., :64], kv[..., 64:], 8, 8)             # head size 8


# ------------------------------------------------------------------------------------------------ streaming collapse
@pytest.mark.parametrize("sizes", [[1], [1, 2, 3, 70, 64, 65], [500]], ids=["ones", "mixed", "whole"])
def test_collapse_stream_equals_groupby(sizes):
    from huggingface_asr_amd import ops
    B, T, blank = 3, 500, 5
    g = torch.Generator().manual_seed(3)
    best = torch.randint(3, 6, (B, T), generator=g).int()          # three classes, one of them blank: many repeats across every boundary
    ends = [500, 431, 0]
    prev = torch.full((B,), -1, dtype=torch.int32, device=DEV)
    got = [[] for _ in range(B)]
    p = 0
    for n in _parts(T, sizes):
        ids, cnt = ops.ctc_collapse_stream(best[:, p:p + n].to(DEV), blank, prev, n_valid=torch.tensor(ends), offset=p)
        ids, cnt = ids.cpu(), cnt.cpu()
        for b in range(B):
            got[b] += ids[b, : int(cnt[b])].tolist()
            assert (ids[b, int(cnt[b]):] == -1).all()
        p += n
    for b in range(B):
        want = [k for k, _ in itertools.groupby(best[b, : ends[b]].tolist()) if k != blank]
        assert got[b] == want, b
