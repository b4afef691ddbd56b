"""The two new operators of the fp32 decoder step (huggingface_asr_amd/csrc/decoder_f32.hip; wrappers in huggingface_asr_amd/ops_f32.py) against float64 references
on the host.

  a. mi_linear_rows_f32 against a float64 host product, with the bound tests/test_gpu_f32_ops.py holds mi_gemm_f32 to, computed here in float64 per element:
         (K + 8) * 2**-24 * (sum_k |a_k w_k| + |bias| + |resid|)
     Every product enters an fma un-rounded and K - 1 additions (in whatever order: lanes of a chunk, the four waves of a block, the K slices of a split launch) plus
     bias and residual round once each: the first-order gamma_n bound holds for any summation order.  Shapes: 1 <= M <= 64 around the 32-row tile, N around the 32- and
     128-row block edges and one wide enough for the one-tile-per-wave decomposition, K from one 16-byte piece to a split over K with a ragged last chunk.  Without /
     with bias, plain / accumulated into what is there, gelu_new (bound x max |gelu_new'| = 1.13, + E = 2 x max |torch's fp32 tanh-GELU on the device - float64|: two
     independent fp32 tanh implementations); two runs give the same bits; the output is a view inside a NaN-filled buffer whose padding must stay NaN, the operands
     views beside finite junk that a read past K would pull into every sum; row m of the 64-row call equals the 1-row call on that row, bit for bit.
  b. its K / V-cache append: rows past + u of both caches, nothing else.
  c. mi_attention_general_f32 against the same attention in float64.  Allowance per case: 16 x max |CPU torch fp32 - float64| on the same inputs (the rule of
     tests/test_gpu_f32_ops.py: torch's own fp32 is the reference's noise).  Cached causal steps with a batch stride beyond the keys in use, cross-attention with key
     lengths (0 valid keys included: uniform over all Tk, as mi_attention_f32 documents), and hypotheses sharing one table per utterance (`beams`), which must give the
     bits of the replicated tables.
Every test prints its figures (pytest -s): `F32DEC <what> <case> ...`."""
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F32, F64 = torch.float32, torch.float64
U = 2.0 ** -24
MS = (1, 5, 31, 32, 33, 64)
NK = [(N, K) for N in (1, 33, 51, 130, 5001) for K in (4, 36, 132, 2048)] + [(24500, 36)]      # the last: >= 192 blocks of 128 weight rows, one tile per wave


def _ops():
    from huggingface_asr_amd import ops_f32
    return ops_f32


def _rand(gen, *shape, scale=1.0):
    """uniform in [-scale, scale), float64 holding fp32-representable values"""
    return ((torch.rand(*shape, generator=gen, dtype=F64) * 2 - 1) * scale).float().double()


def _strided(t, ld, fill):
    buf = torch.full((t.shape[0] + 1, ld), fill, dtype=F32, device=DEV)
    buf[: t.shape[0], : t.shape[1]] = t.to(DEV)
    return buf[: t.shape[0], : t.shape[1]]


@functools.lru_cache(maxsize=2)
def _linear_inputs(N, K):
    """64 rows once per (N, K): a row's result depends on that row alone, so every M reads the first M rows of the same reference"""
    gen = torch.Generator().manual_seed(10 * N + K)
    x, w = _rand(gen, 64, K), _rand(gen, N, K)
    bias, resid = _rand(gen, N), _rand(gen, 64, N, scale=2.0)
    return x, w, bias, resid, x @ w.T, x.abs() @ w.abs().T


def _run_linear(O, xv, wv, bias, resid, M, N, act="none"):
    """-> the (M, N) result inside a NaN-filled buffer, checked for writes outside it"""
    buf = torch.full((M + 1, N + 4), float("nan"), dtype=F32, device=DEV)
    out = buf[:M, :N]
    if resid is not None:
        out.copy_(resid[:M])
    O.linear_rows(xv[:M], wv, bias, out, act=act, accumulate=resid is not None)
    torch.cuda.synchronize()
    assert torch.isnan(buf[:M, N:]).all() and torch.isnan(buf[M]).all(), "the linear wrote outside its output"
    return out.cpu()


@pytest.mark.parametrize("N,K", NK, ids=[f"{n}x{k}" for n, k in NK])
def test_linear_rows_f32_against_float64(N, K):
    O = _ops()
    x, w, bias, resid, prod, mag = _linear_inputs(N, K)
    xv, wv = _strided(x.float(), K + 4, 7.0), _strided(w.float(), K + 8, 7.0)
    bd, rd = bias.float().to(DEV), resid.float().to(DEV)
    gelu64 = lambda t: 0.5 * t * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (t + 0.044715 * t ** 3)))
    # gelu_new over pre-activations of a few units (both tails of the function): x scaled so that the K-term sums have a spread of ~3
    sc = min(4.0, 9.0 / math.sqrt(K))
    xg = (x * sc).float().double()
    xgv = _strided(xg.float(), K + 4, 7.0)
    pre, gmag = xg @ w.T + bias[None], xg.abs() @ w.abs().T + bias.abs()[None]
    E = 2 * float((torch.nn.functional.gelu(pre.float().to(DEV), approximate="tanh").cpu().double() - gelu64(pre.float().double())).abs().max())
    worst = worst_g = 0.0
    for M in MS:
        for use_bias in (False, True):
            for acc in (False, True):
                want = prod[:M] + (bias[None] if use_bias else 0.0) + (resid[:M] if acc else 0.0)
                bound = (K + 8) * U * (mag[:M] + (bias.abs()[None] if use_bias else 0.0) + (resid[:M].abs() if acc else 0.0))
                got = [_run_linear(O, xv, wv, bd if use_bias else None, rd if acc else None, M, N) for _ in range(2)]
                assert torch.equal(got[0], got[1]), "two runs differ"
                assert torch.isfinite(got[0]).all()
                err = (got[0].double() - want).abs()
                worst = max(worst, float((err / bound).max()))
                assert bool((err <= bound).all()), (M, use_bias, acc, float((err / bound).max()))
        gbound = 1.13 * (K + 8) * U * gmag[:M] + E
        got = [_run_linear(O, xgv, wv, bd, None, M, N, act="gelu_new") for _ in range(2)]
        assert torch.equal(got[0], got[1])
        gerr = (got[0].double() - gelu64(pre[:M])).abs()
        worst_g = max(worst_g, float((gerr / gbound).max()))
        assert bool((gerr <= gbound).all()), (M, "gelu_new", float((gerr / gbound).max()))
    # a row's result is a function of that row alone, whatever M is
    full = _run_linear(O, xv, wv, bd, None, 64, N)
    for m in (0, 31, 32, 63):
        one = _run_linear(O, xv[m:m + 1], wv, bd, None, 1, N)
        assert torch.equal(one[0], full[m]), ("row", m)
    ksplit = O.linear_rows_workspace_bytes(1, N, K) // (4 * N)
    print(f"F32DEC linear_rows N={N} K={K} ksplit={max(ksplit, 1)} worst err/bound={worst:.3f} gelu_new err/bound={worst_g:.3f}")


@pytest.mark.parametrize("K,dkv", [(36, 44), (2048, 4)], ids=["one_launch", "split_k"])
def test_linear_rows_f32_cache_append(K, dkv):
    """the QKV linear of the step: columns [dkv, 3 dkv) of row b U + u land at row past + u of sequence b in both caches; every other cache row keeps its bits"""
    O = _ops()
    B, Un, past, Lmax = 3, 2, 3, 7
    M, N = B * Un, 3 * dkv
    gen = torch.Generator().manual_seed(K)
    x, w, bias = _rand(gen, M, K).float().to(DEV), _rand(gen, N, K).float().to(DEV), _rand(gen, N).float().to(DEV)
    assert (O.linear_rows_workspace_bytes(M, N, K) > 0) == (K == 2048)
    kc, vc = torch.full((B, Lmax, dkv), 5.0, device=DEV), torch.full((B, Lmax, dkv), 6.0, device=DEV)
    out = O.linear_rows(x, w, bias, kcache=kc, vcache=vc, U=Un, past=past)
    plain = O.linear_rows(x, w, bias)
    assert torch.equal(out, plain)
    o = out.view(B, Un, N)
    assert torch.equal(kc[:, past:past + Un], o[..., dkv:2 * dkv]) and torch.equal(vc[:, past:past + Un], o[..., 2 * dkv:])
    keep = [r for r in range(Lmax) if not past <= r < past + Un]
    assert bool((kc[:, keep] == 5.0).all()) and bool((vc[:, keep] == 6.0).all())


# ----------------------------------------------------------------------------------------------------------------- attention
def _attn_ref(q, k, v, B, Tq, Tk, H, lengths, causal, beams, dtype):
    """q (B*Tq, d), k / v (B / beams, Tk, d), lengths (B / beams) or None -> (B*Tq, d) in `dtype` on the CPU"""
    d = q.shape[1]
    hd = d // H
    q, k, v = q.to(dtype).view(B, Tq, H, hd), k.to(dtype), v.to(dtype)
    ut = torch.arange(B) // beams
    kh, vh = k[ut].view(B, Tk, H, hd), v[ut].view(B, Tk, H, hd)
    s = torch.einsum("bihc,bjhc->bhij", q, kh) / math.sqrt(hd)
    j = torch.arange(Tk)
    valid = torch.ones(B, 1, Tq, Tk, dtype=torch.bool)
    if lengths is not None:
        valid = valid & (j[None, None, None, :] < lengths[ut][:, None, None, None])
    if causal:
        valid = valid & (j[None, None, None, :] <= (torch.arange(Tq)[None, None, :, None] + Tk - Tq))
    valid = valid.expand(B, H, Tq, Tk)
    pr = torch.softmax(s.masked_fill(~valid, float("-inf")), -1)
    none = ~valid.any(-1, keepdim=True)
    pr = torch.where(none, torch.full_like(pr, 1.0 / Tk), torch.nan_to_num(pr, nan=0.0))
    return torch.einsum("bhij,bjhc->bihc", pr, vh).reshape(B * Tq, d)


ATT_SHAPES = [(H, hd, Tq, Tk) for H, hd in ((2, 64), (1, 128)) for Tq in (1, 3) for Tk in (1, 31, 33, 65, 130)]


def _check_attn(tag, got, q, k, v, B, Tq, Tk, H, lengths, causal, beams):
    want = _attn_ref(q, k, v, B, Tq, Tk, H, lengths, causal, beams, F64)
    noise = float((_attn_ref(q, k, v, B, Tq, Tk, H, lengths, causal, beams, F32).double() - want).abs().max())
    err = float((got.cpu().double() - want).abs().max())
    print(f"F32DEC attention {tag} err={err:.3e} allow={16 * noise:.3e} ratio={err / noise if noise else 0.0:.2f}")
    assert torch.isfinite(got).all() and err <= 16 * noise, (tag, err, noise)


@pytest.mark.parametrize("H,hd,Tq,Tk", ATT_SHAPES, ids=[f"H{h}x{c}_Tq{a}_Tk{b}" for h, c, a, b in ATT_SHAPES])
def test_attention_general_f32_against_float64(H, hd, Tq, Tk):
    O = _ops()
    d = H * hd
    gen = torch.Generator().manual_seed(1000 * hd + 10 * Tk + Tq)
    # cached, causal with offset Tk - Tq, the caches' batch stride beyond the keys in use; the unused cache rows hold NaN: a key past the valid set is never read
    if Tk >= Tq:
        B, Lmax = 2, Tk + 3
        q, k, v = _rand(gen, B * Tq, d, scale=2.0), _rand(gen, B, Tk, d, scale=2.0), _rand(gen, B, Tk, d)
        kc, vc = (torch.full((B, Lmax, d), float("nan"), dtype=F32, device=DEV) for _ in range(2))
        kc[:, :Tk], vc[:, :Tk] = k.float().to(DEV), v.float().to(DEV)
        qkv = _strided(q.float(), 3 * d, 7.0)                          # q as the first block of a wider row, as in the step
        got = [O.attention_general(qkv, kc.view(B * Lmax, d), vc.view(B * Lmax, d), B, Tq, Tk, H, causal=True, kv_bstride=Lmax * d) for _ in range(2)]
        assert torch.equal(got[0], got[1])
        _check_attn("cached", got[0], q, k, v, B, Tq, Tk, H, None, True, 1)
    # cross-attention with key lengths, one table per utterance shared by `beams` hypotheses
    for beams in (1, 3):
        nu = 3
        B = nu * beams
        q, k, v = _rand(gen, B * Tq, d, scale=2.0), _rand(gen, nu, Tk, d, scale=2.0), _rand(gen, nu, Tk, d)
        lengths = torch.tensor([1, Tk - 1, Tk], dtype=torch.int32)
        kv = torch.cat([k, v], -1).float().to(DEV).view(nu * Tk, 2 * d)                     # [K | V] rows, the step's cross tables
        qd = q.float().to(DEV)
        got = O.attention_general(qd, kv[:, :d], kv[:, d:], B, Tq, Tk, H, lengths=lengths.to(DEV), beams=beams)
        _check_attn(f"cross beams={beams}", got, q, k, v, B, Tq, Tk, H, lengths, False, beams)
        nolen = O.attention_general(qd, kv[:, :d], kv[:, d:], B, Tq, Tk, H, beams=beams)
        _check_attn(f"cross beams={beams} no lengths", nolen, q, k, v, B, Tq, Tk, H, None, False, beams)
        if beams > 1:                                                  # the replicated tables give the same bits
            kv_rep = kv.view(nu, Tk, 2 * d).repeat_interleave(beams, 0).reshape(B * Tk, 2 * d).contiguous()
            rep = O.attention_general(qd, kv_rep[:, :d], kv_rep[:, d:], B, Tq, Tk, H, lengths=lengths.repeat_interleave(beams).to(DEV))
            assert torch.equal(rep, got)


def test_new_operators_refuse_bad_arguments():
    O = _ops()
    x, w = torch.zeros((4, 8), device=DEV), torch.zeros((4, 8), device=DEV)
    with pytest.raises(ValueError):
        O.linear_rows(x, torch.zeros((4, 12), device=DEV))
    with pytest.raises(TypeError):
        O.linear_rows(x.bfloat16(), w)
    with pytest.raises(RuntimeError, match="unsupported"):
        O.linear_rows(torch.zeros((4, 6), device=DEV), torch.zeros((4, 6), device=DEV))       # K % 4 != 0
    with pytest.raises(RuntimeError, match="invalid argument"):
        O.linear_rows(torch.zeros((65, 8), device=DEV), w)                                      # more than 64 rows
    q = torch.zeros((2, 64), device=DEV)
    with pytest.raises(RuntimeError, match="unsupported"):
        O.attention_general(q, q, q, 2, 1, 1, 2)                                                 # head size 32
    with pytest.raises(RuntimeError, match="invalid argument"):
        O.attention_general(q, q, q, 2, 1, 1, 1, beams=3)                                        # 2 batches are no multiple of 3 hypotheses
