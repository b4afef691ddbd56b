"""Thin torch-tensor wrappers over the C ABI (one per entry point in include/hfasr_hip.h).

PyTorch is used for device memory and streams only; every op here runs a hand-written HIP kernel on
`torch.cuda.current_stream()`.  All tensors must be CUDA(HIP) tensors; there is no CPU path.
"""
from __future__ import annotations

import math

import torch

from . import _lib

BF16 = torch.bfloat16


def _p(t):
    return 0 if t is None else t.data_ptr()


_PINNED_STREAM = None          # set by `pinned_stream()`: the training step makes ~1100 C-ABI calls, and asking torch for the current stream costs ~5 us each


def _stream():
    return torch.cuda.current_stream().cuda_stream if _PINNED_STREAM is None else _PINNED_STREAM


class pinned_stream:
    """`with ops.pinned_stream():` — resolve torch's current stream ONCE for the body (a trainer step runs on one stream from start to end) instead of once per
    kernel launch.  Code inside that switches streams with `torch.cuda.stream(...)` must not rely on `_stream()` following it; nesting keeps the outer value."""

    def __enter__(self):
        global _PINNED_STREAM
        self.prev = _PINNED_STREAM
        if _PINNED_STREAM is None:
            _PINNED_STREAM = torch.cuda.current_stream().cuda_stream
        return self

    def __exit__(self, *exc):
        global _PINNED_STREAM
        _PINNED_STREAM = self.prev
        return False


def _req(t: torch.Tensor, dtype=None):
    if not t.is_cuda:
        raise RuntimeError("huggingface_asr_amd ops need device tensors (no CPU fallback)")
    if dtype is not None and t.dtype != dtype:
        raise TypeError(f"expected {dtype}, got {t.dtype}")
    return t


def gemm(a, w, bias=None, out=None, *, out_dtype=BF16, act="none", resid=None, alpha=1.0, bias_per_row=False,
         col_remap=None, variant=0):
    """out[M,N] = epi(a[M,K] @ w[N,K]^T); a/w bf16 (last dim contiguous).  `variant`: kernel selection of mi_gemm_bf16_v (tests / A-B tools; 0 = product dispatch)."""
    _req(a, BF16); _req(w, BF16)
    M, K = a.shape
    N = w.shape[0]
    if out is None:
        out = torch.empty((M, N), device=a.device, dtype=out_dtype)
    ct, ctp = col_remap if col_remap else (0, 0)
    rc = _lib.lib().mi_gemm_bf16_v(a.data_ptr(), a.stride(0), w.data_ptr(), w.stride(0), _p(bias),
                                   (2 if bias_per_row else 1) if bias is not None else 0,
                                   out.data_ptr(), out.stride(0), int(out.dtype == torch.float32),
                                   _p(resid), resid.stride(0) if resid is not None else 0, float(alpha),
                                   {"none": 0, "gelu": 1, "gelu_new": 2}[act], M, N, K, ct, ctp, int(variant), _stream())
    _lib.check(rc, "mi_gemm_bf16")
    return out


def conv2d_first_gelu(x, w, bias, stride=2, pad=1, causal=False):
    """x (B,T,F) f32, w (C,K*K) f32 -> channels-last (B,T1,F1,C) bf16 = gelu(conv)."""
    B, T, F = x.shape
    Cc, KK = w.shape
    K = int(round(math.sqrt(KK)))
    T1, F1 = (T + 2 * pad - K) // stride + 1, (F + 2 * pad - K) // stride + 1
    out = torch.empty((B, T1, F1, Cc), device=x.device, dtype=BF16)
    pl = 2 * pad if causal else pad
    rc = _lib.lib().mi_conv2d_first_gelu(x.data_ptr(), w.data_ptr(), bias.data_ptr(), out.data_ptr(), B, T, F, Cc, K,
                                         stride, pl, pl, T1, F1, _stream())
    _lib.check(rc, "mi_conv2d_first_gelu")
    return out


def conv2d_cl(x, w, bias, K=3, stride=2, pad=1, causal=False, act="gelu", variant=0):
    """x (B,T,F,Cin) bf16 channels-last, w (Cout, KH*KW*Cin) bf16 -> (B,T',F',Cout) bf16.  K / pad may be (time, freq) pairs
    (a Conv1d over time is K=(k,1), pad=(p,0) on an F=1 layout)."""
    B, T, F, Cin = x.shape
    Cout = w.shape[0]
    KH, KW = (K, K) if isinstance(K, int) else K
    pt, pf = (pad, pad) if isinstance(pad, int) else pad
    T1, F1 = (T + 2 * pt - KH) // stride + 1, (F + 2 * pf - KW) // stride + 1
    out = torch.empty((B, T1, F1, Cout), device=x.device, dtype=BF16)
    plt, plf = (2 * pt, 2 * pf) if causal else (pt, pf)
    rc = _lib.lib().mi_conv2d_cl_bf16_v(x.data_ptr(), w.data_ptr(), _p(bias), out.data_ptr(), B, T, F, Cin, Cout, KH, KW, stride,
                                        plt, plf, T1, F1, {"none": 0, "gelu": 1}[act], int(variant), _stream())
    _lib.check(rc, "mi_conv2d_cl_bf16")
    return out


def _geo_out(n, k, s, p):
    return (n + 2 * p - k) // s + 1


def conv2d_first_geo(x, w, bias, K=(3, 3), stride=(2, 2), pad=(1, 1), act="gelu"):
    """Conv2d(1 -> C) of general geometry: x (B,T,F) f32, w (C, KH*KW) f32 -> channels-last (B,T1,F1,C) bf16; act "gelu" or "none" (raw pre-activation)."""
    B, T, F = x.shape
    Cc = w.shape[0]
    (KH, KW), (st, sf), (pt, pf) = K, stride, pad
    T1, F1 = _geo_out(T, KH, st, pt), _geo_out(F, KW, sf, pf)
    out = torch.empty((B, T1, F1, Cc), device=x.device, dtype=BF16)
    _lib.check(_lib.lib().mi_conv2d_first_geo(x.data_ptr(), w.data_ptr(), bias.data_ptr(), out.data_ptr(), B, T, F, Cc, KH, KW, st, sf, pt, pf, T1, F1,
                                              {"none": 0, "gelu": 1}[act], _stream()), "mi_conv2d_first_geo")
    return out


def conv2d_first_gated_gelu(x, w, bias, gw, gbias, stride=2, pad=1):
    """GatedConv2d first layer fused (extractors.py:23-32): GELU((conv + b) * sigmoid(gate + bg)); 3x3 only."""
    B, T, F = x.shape
    Cc, KK = w.shape
    K = int(round(math.sqrt(KK)))
    T1, F1 = _geo_out(T, K, stride, pad), _geo_out(F, K, stride, pad)
    out = torch.empty((B, T1, F1, Cc), device=x.device, dtype=BF16)
    _lib.check(_lib.lib().mi_conv2d_first_gated_gelu(x.data_ptr(), w.data_ptr(), bias.data_ptr(), gw.data_ptr(), gbias.data_ptr(), out.data_ptr(), B, T, F, Cc, K,
                                                     stride, pad, pad, T1, F1, _stream()), "mi_conv2d_first_gated_gelu")
    return out


def conv2d_cl_geo(x, w, bias, K=(3, 3), stride=(2, 2), pad=(1, 1), act="gelu", gated=False):
    """conv2d_cl with (time, freq) kernel / stride / pad pairs; gated: w (2*Cout, K) / bias (2*Cout) interleaved [conv 32 ; gate 32] -> GELU(conv * sigmoid(gate))."""
    B, T, F, Cin = x.shape
    Cout = w.shape[0] // (2 if gated else 1)
    (KH, KW), (st, sf), (pt, pf) = K, stride, pad
    T1, F1 = _geo_out(T, KH, st, pt), _geo_out(F, KW, sf, pf)
    out = torch.empty((B, T1, F1, Cout), device=x.device, dtype=BF16)
    _lib.check(_lib.lib().mi_conv2d_cl_geo_bf16(x.data_ptr(), w.data_ptr(), _p(bias), out.data_ptr(), B, T, F, Cin, Cout, KH, KW, st, sf, pt, pf, T1, F1,
                                                {"none": 0, "gelu": 1}[act], int(gated), _stream()), "mi_conv2d_cl_geo_bf16")
    return out


def gated_act(z, g, B, T, Fq, C, share=1, blk=0, out=None):
    """GELU(z * sigmoid(g)) -> (B*T*Fq, C) bf16; z rows (b,t,f), g rows (b, t // share, f); blk > 0: z is g, columns interleaved [conv blk | gate blk]."""
    z2, g2 = z.reshape(-1, z.shape[-1]), g.reshape(-1, g.shape[-1])
    if out is None:
        out = torch.empty((B * T * Fq, C), device=z.device, dtype=BF16)
    _lib.check(_lib.lib().mi_gated_act_bf16(z2.data_ptr(), z2.stride(0), g2.data_ptr(), g2.stride(0), out.data_ptr(), out.stride(0), B, T, Fq, C, share, blk, _stream()),
               "mi_gated_act_bf16")
    return out


def gemm_lnfold(xb, wf, colsum, cbias, stats, npart, eps=1e-5, act="none", out=None):
    """act(LN(x) W^T + b) with the LayerNorm folded into the GEMM (csrc/gemm_args.hpp): xb = bf16(x) (M,K), wf = bf16(W diag(gamma)) (N,K), colsum = sum_k wf, cbias = W beta + b,
    stats (M,32) fp32 = per-row partial (sum, sumsq) pairs of x (npart pairs)."""
    M, K = xb.shape
    N = wf.shape[0]
    if out is None:
        out = torch.empty((M, N), device=xb.device, dtype=BF16)
    _lib.check(_lib.lib().mi_gemm_lnfold_bf16(xb.data_ptr(), xb.stride(0), wf.data_ptr(), wf.stride(0), colsum.data_ptr(), cbias.data_ptr(), stats.data_ptr(), int(npart), float(eps),
                                              out.data_ptr(), out.stride(0), {"none": 0, "gelu": 1}[act], M, N, K, _stream()), "mi_gemm_lnfold_bf16")
    return out


def gemm_resid_stats(a, w, bias, resid, alpha=1.0, wide=False, variant=None):
    """-> (C fp32 = resid + alpha (a W^T + b), C2 = bf16(C), stats (M,32) fp32 with one (sum, sumsq) pair per 32 columns of C — per 64 columns with `wide`,
    the 256 x 256 tile of the throughput mode (mi_ebf_config.wide_tiles))"""
    M, K = a.shape
    N = w.shape[0]
    c = torch.empty((M, N), device=a.device, dtype=torch.float32)
    c2 = torch.empty((M, N), device=a.device, dtype=BF16)
    st = torch.zeros((M, 32), device=a.device, dtype=torch.float32)
    _lib.check(_lib.lib().mi_gemm_resid_stats_f32_v(a.data_ptr(), a.stride(0), w.data_ptr(), w.stride(0), _p(bias), c.data_ptr(), c.stride(0), _p(resid), resid.stride(0) if resid is not None else 0,
                                                    float(alpha), c2.data_ptr(), c2.stride(0), st.data_ptr(), M, N, K, (40 if wide else 0) if variant is None else int(variant), _stream()), "mi_gemm_resid_stats_f32_v")
    return c, c2, st


def layernorm_fold(x, ln=None, eps=1e-5, lengths=None, T=1):
    """y = [LN](mask(x)) -> (y fp32, bf16(y), stats (M,32) with (sum, sumsq) of y in pair 0)"""
    M, d = x.shape
    g, b = ln if ln else (None, None)
    y = torch.empty_like(x)
    yb = torch.empty((M, d), device=x.device, dtype=BF16)
    st = torch.zeros((M, 32), device=x.device, dtype=torch.float32)
    _lib.check(_lib.lib().mi_layernorm_fold(x.data_ptr(), x.stride(0), _p(lengths), T, _p(g), _p(b), float(eps), y.data_ptr(), y.stride(0), yb.data_ptr(), yb.stride(0), st.data_ptr(),
                                            M, d, _stream()), "mi_layernorm_fold")
    return y, yb, st


def layernorm_chain(x, *, lengths=None, T=1, ln1=None, eps1=1e-5, store_y=None, lna=None, eps2=1e-5, outa=None,
                    outa32=None, lnb=None, outb=None):
    """see csrc/norm.hip; x (M,d) f32; ln* = (gamma, beta) f32."""
    M, d = x.shape
    g1, b1 = ln1 if ln1 else (None, None)
    ga, ba = lna if lna else (None, None)
    gb, bb = lnb if lnb else (None, None)
    rc = _lib.lib().mi_layernorm_chain(x.data_ptr(), x.stride(0), _p(lengths), T, _p(g1), _p(b1), eps1,
                                       _p(store_y), store_y.stride(0) if store_y is not None else 0,
                                       _p(ga), _p(ba), eps2, _p(outa), outa.stride(0) if outa is not None else 0,
                                       _p(outa32), outa32.stride(0) if outa32 is not None else 0,
                                       _p(gb), _p(bb), _p(outb), outb.stride(0) if outb is not None else 0, M, d, _stream())
    _lib.check(rc, "mi_layernorm_chain")


def rotary(x, cos, sin, T, H):
    M, d = x.shape
    out = torch.empty_like(x)
    rc = _lib.lib().mi_rotary_bf16(x.data_ptr(), x.stride(0), out.data_ptr(), out.stride(0), cos.data_ptr(), sin.data_ptr(),
                                   M, T, H, d // H, _stream())
    _lib.check(rc, "mi_rotary_bf16")
    return out


def attention(q, k, vt, Tp, B, T, H, *, pos=None, bias_u=None, bias_v=None, lengths=None, causal=False):
    """q,k (B*T, >=d) bf16 views; vt (d, B*Tp) bf16; pos (2T-1, d) bf16 or None -> ctx (B*T, d) bf16."""
    d = vt.shape[0]
    hd = d // H
    out = torch.empty((B * T, d), device=q.device, dtype=BF16)
    rc = _lib.lib().mi_attention_bf16(q.data_ptr(), q.stride(0), k.data_ptr(), k.stride(0), vt.data_ptr(), vt.stride(0), Tp,
                                      _p(pos), pos.stride(0) if pos is not None else 0, _p(bias_u), _p(bias_v), _p(lengths),
                                      out.data_ptr(), out.stride(0), B, T, H, hd, 1.0 / math.sqrt(hd), int(causal), _stream())
    _lib.check(rc, "mi_attention_bf16")
    return out


def attention_qkv(qkv, B, T, H, *, pos=None, bias_u=None, bias_v=None, lengths=None, causal=False, lse=None, drop=None, variant=0):
    """LDS-staged attention on a fused (B*T, 3d) bf16 projection [Q|K|V]; head size 64 or 128.
    lse: (B, H, T) fp32 that receives the rows' log-sum-exp (training forward; the backward's `ops_train.attn_bwd_probs` reads it).
    drop = (p, seed, stream_id): attention-probability dropout (with lse only)."""
    d = qkv.shape[1] // 3
    hd = d // H
    out = torch.empty((B * T, d), device=qkv.device, dtype=BF16)
    q, k, v = qkv[:, :d], qkv[:, d:2 * d], qkv[:, 2 * d:]
    operands = (q.data_ptr(), qkv.stride(0), k.data_ptr(), qkv.stride(0), v.data_ptr(), qkv.stride(0),
               _p(pos), pos.stride(0) if pos is not None else 0, _p(bias_u), _p(bias_v), _p(lengths), out.data_ptr(), out.stride(0))
    if lse is not None:
        dp, dseed, dsid = drop if drop is not None else (0.0, 0, 0)
        rc = _lib.lib().mi_attention_qkv_lse_bf16(*operands, lse.data_ptr(), B, T, H, hd, 1.0 / math.sqrt(hd), int(causal),
                                                  float(dp), int(dseed) & 0xFFFFFFFF, int(dsid) & 0xFFFFFFFF, _stream())
        _lib.check(rc, "mi_attention_qkv_lse_bf16")
        return out
    # variant != 0: measurement only (tools/attn_ab.py): 1 = the four-wave kernel of rounds 1-3, 2 = the eight-wave form
    rc = _lib.lib().mi_attention_qkv_bf16_v(*operands, B, T, 0, 0, H, hd, 1.0 / math.sqrt(hd), int(causal), int(variant), _stream())
    _lib.check(rc, "mi_attention_qkv_bf16_v")
    return out


def attention_general(q, k, v, B, Tq, Tk, H, *, lengths=None, causal=False, out=None, kv_bstride=0, variant=0):
    """q (B*Tq, .) / k, v (B*Tk, .) bf16 row views with head h at columns [h*hd, (h+1)*hd) -> context (B*Tq, d) bf16.
    Cross-attention (Tk = encoder frames, `lengths` = valid keys) and KV-cache steps (causal offset Tk - Tq).
    variant: as in `attention_qkv` (1 = the four-wave kernel, 2 = the eight-wave form; tests and measurements only)."""
    d = q.shape[1]
    hd = d // H
    if out is None:
        out = torch.empty((B * Tq, d), device=q.device, dtype=BF16)
    rc = _lib.lib().mi_attention_qkv_bf16_v(q.data_ptr(), q.stride(0), k.data_ptr(), k.stride(0), v.data_ptr(), v.stride(0),
                                            0, 0, 0, 0, _p(lengths), out.data_ptr(), out.stride(0), B, Tq, Tk, kv_bstride, H, hd,
                                            1.0 / math.sqrt(hd), int(causal), int(variant), _stream())
    _lib.check(rc, "mi_attention_qkv_bf16_v")
    return out


def row_stats(x, eps=1e-5):
    M, d = x.shape
    st = torch.empty((M, 2), device=x.device, dtype=torch.float32)
    rc = _lib.lib().mi_row_stats_bf16(x.data_ptr(), x.stride(0), d, eps, st.data_ptr(), M, _stream())
    _lib.check(rc, "mi_row_stats_bf16")
    return st


def csgu(u, gamma, beta, w, bias, B, T, *, pad_left=None, dilation=1, act=0, eps=1e-5, stats=None):
    """u (B*T, 2C) bf16 = [x_r | x_g] -> x_r * act(dwconv(LN(x_g)) + b)  (B*T, C) bf16.  stats: row_stats(u[:, C:], eps) when the caller already holds it."""
    M, C2 = u.shape
    Cc = C2 // 2
    K = w.shape[-1]
    st = row_stats(u[:, Cc:], eps) if stats is None else stats
    out = torch.empty((M, Cc), device=u.device, dtype=BF16)
    rc = _lib.lib().mi_csgu_bf16(u.data_ptr(), u.stride(0), st.data_ptr(), gamma.data_ptr(), beta.data_ptr(), w.data_ptr(),
                                 _p(bias), out.data_ptr(), out.stride(0), B, T, Cc, K,
                                 (K - 1) // 2 if pad_left is None else pad_left, dilation, act, _stream())
    _lib.check(rc, "mi_csgu_bf16")
    return out


def csgu_conv(u, stats, gamma, beta, w, bias, B, T, *, pad_left=None, dilation=1):
    """the CSGU conv alone (split form: csgu_use_linear_after_conv / non-identity activation on the training path): dwconv(LN(x_g)) + b  (B*T, C) bf16;
    stats = row_stats(u[:, C:])"""
    M, C2 = u.shape
    Cc = C2 // 2
    K = w.shape[-1]
    out = torch.empty((M, Cc), device=u.device, dtype=BF16)
    rc = _lib.lib().mi_csgu_conv_bf16(u.data_ptr(), u.stride(0), stats.data_ptr(), gamma.data_ptr(), beta.data_ptr(), w.data_ptr(), _p(bias),
                                      out.data_ptr(), out.stride(0), B, T, Cc, K, (K - 1) // 2 if pad_left is None else int(pad_left), int(dilation), _stream())
    _lib.check(rc, "mi_csgu_conv_bf16")
    return out


def gate_act_mul(r, g, act=0):
    """r * act(g) on (M, C) bf16 rows (r may be a column slice); act 0 identity, 1 gelu, 2 relu, 3 silu"""
    M, Cc = g.shape
    out = torch.empty((M, Cc), device=g.device, dtype=BF16)
    rc = _lib.lib().mi_gate_act_mul_bf16(r.data_ptr(), r.stride(0), g.data_ptr(), g.stride(0), out.data_ptr(), out.stride(0), M, Cc, int(act), _stream())
    _lib.check(rc, "mi_gate_act_mul_bf16")
    return out


def dwconv_residual(m, w, bias, B, T, pad_left=None):
    M, Cc = m.shape
    K = w.shape[-1]
    out = torch.empty_like(m)
    rc = _lib.lib().mi_dwconv_residual_bf16(m.data_ptr(), m.stride(0), w.data_ptr(), _p(bias), out.data_ptr(), out.stride(0),
                                            B, T, Cc, K, (K - 1) // 2 if pad_left is None else int(pad_left), _stream())
    _lib.check(rc, "mi_dwconv_residual_bf16")
    return out


def gemm_lse(a, w, bias, out):
    """the CTC head in one pass over its logits: out (M, ld >= N) fp32 [:, :N] = a W^T + b, N = w.shape[0], and -> lse (M) fp32 = the rows' log-sum-exp over those N
    columns, out of the GEMM's epilogue (mi_gemm_lse_f32); shapes outside that kernel: the GEMM followed by row_lse."""
    _req(a, BF16); _req(w, BF16)
    M, K = a.shape
    N = w.shape[0]
    L = _lib.lib()
    lse = torch.empty((M,), device=a.device, dtype=torch.float32)
    ws = torch.empty((int(L.mi_gemm_lse_workspace_floats(M, N)),), device=a.device, dtype=torch.float32)
    rc = L.mi_gemm_lse_f32(a.data_ptr(), a.stride(0), w.data_ptr(), w.stride(0), _p(bias), out.data_ptr(), out.stride(0), lse.data_ptr(), ws.data_ptr(), M, N, K, _stream())
    if rc == _lib.ERR_UNSUPPORTED:
        gemm(a, w, bias, out=out)
        return row_lse(out[:, :N])
    _lib.check(rc, "mi_gemm_lse_f32")
    return lse


def linear_rows(x, w, bias=None, *, act="none", out=None, out_dtype=BF16, accumulate=False, kv_cache=None, U=1, past=0):
    """y = act(x @ w^T + bias) for 1 <= M <= 64 rows (mi_linear_rows, csrc/linear_rows.hip: the weights are streamed once, spread over the chip by N and K; no float
    atomics, bit-reproducible, rows independent).  x (M, K), w (N, K) bf16, K % 8 == 0.  out fp32: y, or out += y with `accumulate` (the residual stream); out bf16: y, and
    with kv_cache = (k, v), each (B, Lmax, d) bf16 and N == 3 d, columns [d, 2d) / [2d, 3d) of row b U + u are also written to k / v at position past + u."""
    _req(x, BF16); _req(w, BF16)
    M, K = x.shape
    N = w.shape[0]
    if out is None:
        out = torch.empty((M, N), device=x.device, dtype=out_dtype)
    L = _lib.lib()
    nbytes = L.mi_linear_rows_workspace_bytes(M, N, K)
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=x.device)
    f32 = out.dtype == torch.float32
    kc, vc = kv_cache if kv_cache is not None else (None, None)
    rc = L.mi_linear_rows(x.data_ptr(), x.stride(0), w.data_ptr(), w.stride(0), _p(bias), {"none": 0, "gelu": 1, "gelu_new": 2}[act],
                          out.data_ptr() if f32 else None, out.stride(0) if f32 else 0, int(bool(accumulate)), None if f32 else out.data_ptr(), 0 if f32 else out.stride(0),
                          _p(kc), _p(vc), int(U), int(past), kc.shape[1] if kc is not None else 0, kc.shape[2] if kc is not None else 0, M, N, K,
                          ws.data_ptr(), nbytes, _stream())
    _lib.check(rc, "mi_linear_rows")
    return out


def row_lse(x):
    M, V = x.shape
    out = torch.empty((M,), device=x.device, dtype=torch.float32)
    rc = _lib.lib().mi_row_lse(x.data_ptr(), x.stride(0), 0 if x.dtype == torch.float32 else 1, V, out.data_ptr(), M, _stream())
    _lib.check(rc, "mi_row_lse")
    return out


def row_argmax(x):
    """x (M, V) f32|bf16 (last dim contiguous, any row stride) -> (M) int32 = torch.argmax(x, -1): lowest index among equal maxima, the first NaN beats every number,
    an all -inf row gives 0 (mi_row_argmax: one pass over x)."""
    _req(x)
    if x.dtype not in (torch.float32, BF16) or x.dim() != 2 or x.stride(1) != 1:
        raise TypeError("row_argmax: a 2-D fp32 / bf16 tensor with contiguous rows")
    M, V = x.shape
    out = torch.empty((M,), device=x.device, dtype=torch.int32)
    rc = _lib.lib().mi_row_argmax(x.data_ptr(), x.stride(0), 0 if x.dtype == torch.float32 else 1, V, out.data_ptr(), M, _stream())
    _lib.check(rc, "mi_row_argmax")
    return out


def whisper_timestamp_argmax(logits, ids, *, begin_index, cur_len, no_timestamps_token_id, eos_token_id, max_initial_timestamp_index=None, detect_from_logprob=True):
    """logits (B, V) fp32 (contiguous rows, any row stride), ids (B, Lmax) int64 -> (B) int32 = argmax(WhisperTimeStampLogitsProcessor(ids[:, :cur_len], logits)) of
    transformers, with `row_argmax`'s rules; ids[:, begin_index:cur_len] are the sampled tokens (mi_whisper_timestamp_argmax: one pass over logits)."""
    _req(logits, torch.float32); _req(ids, torch.long)
    if logits.dim() != 2 or logits.stride(1) != 1 or ids.dim() != 2 or ids.stride(1) != 1 or ids.shape[0] != logits.shape[0]:
        raise TypeError("whisper_timestamp_argmax: logits (B, V) fp32 and ids (B, Lmax) int64, both with contiguous rows")
    B, V = logits.shape
    if not 0 <= begin_index <= cur_len <= ids.shape[1]:
        raise ValueError(f"whisper_timestamp_argmax: need 0 <= begin_index ({begin_index}) <= cur_len ({cur_len}) <= {ids.shape[1]}")
    out = torch.empty((B,), device=logits.device, dtype=torch.int32)
    rc = _lib.lib().mi_whisper_timestamp_argmax(logits.data_ptr(), logits.stride(0), V, ids.data_ptr(), ids.stride(0), int(begin_index), int(cur_len),
                                                int(no_timestamps_token_id), int(eos_token_id), -1 if max_initial_timestamp_index is None else int(max_initial_timestamp_index),
                                                1 if detect_from_logprob else 0, out.data_ptr(), B, _stream())
    _lib.check(rc, "mi_whisper_timestamp_argmax")
    return out


def whisper_beam_scores(logits, ids, *, begin_index, cur_len, suppress=None, no_timestamps_token_id=None, eos_token_id=0, max_initial_timestamp_index=None,
                        detect_from_logprob=True):
    """One beam-search step's scores under Whisper's rules, for `mi_beam_step*` (which form logit - lse themselves): logits (rows, V) fp32 (contiguous rows, any row stride,
    no head bias) are rewritten IN PLACE — -inf where `suppress` ((V) fp32 of 0 / -inf, or None) or transformers' `WhisperTimeStampLogitsProcessor(ids[:, :cur_len], .)`
    masks, every other value untouched — and the raw rows' log-sum-exp is returned: (rows) fp32, `row_lse`'s bits.  `no_timestamps_token_id` None: suppression only
    (mi_whisper_beam_scores: one launch, one block per row)."""
    _req(logits, torch.float32); _req(ids, torch.long)
    if logits.dim() != 2 or logits.stride(1) != 1 or ids.dim() != 2 or ids.stride(1) != 1 or ids.shape[0] != logits.shape[0]:
        raise TypeError("whisper_beam_scores: logits (rows, V) fp32 and ids (rows, Lmax) int64, both with contiguous rows")
    rows, V = logits.shape
    if not 0 <= begin_index <= cur_len <= ids.shape[1]:
        raise ValueError(f"whisper_beam_scores: need 0 <= begin_index ({begin_index}) <= cur_len ({cur_len}) <= {ids.shape[1]}")
    if suppress is not None:
        _req(suppress, torch.float32)
        if suppress.shape != (V,) or not suppress.is_contiguous():
            raise TypeError(f"whisper_beam_scores: suppress must be a contiguous ({V}) fp32 vector")
    out = torch.empty((rows,), device=logits.device, dtype=torch.float32)
    rc = _lib.lib().mi_whisper_beam_scores(logits.data_ptr(), logits.stride(0), V, ids.data_ptr(), ids.stride(0), int(begin_index), int(cur_len), _p(suppress),
                                           -1 if no_timestamps_token_id is None else int(no_timestamps_token_id), int(eos_token_id),
                                           -1 if max_initial_timestamp_index is None else int(max_initial_timestamp_index), 1 if detect_from_logprob else 0,
                                           out.data_ptr(), rows, _stream())
    _lib.check(rc, "mi_whisper_beam_scores")
    return out


def gemm_argmax(a, w, bias):
    """the CTC head without its logits: -> (M) int32 = argmax_n (a W^T + b)[m, n] out of the GEMM's epilogue (mi_gemm_argmax_bf16: no (M, N) tensor is written);
    shapes outside that kernel: the fp32 GEMM into a scratch followed by row_argmax."""
    _req(a, BF16); _req(w, BF16)
    M, K = a.shape
    N = w.shape[0]
    L = _lib.lib()
    best = torch.empty((M,), device=a.device, dtype=torch.int32)
    ws = torch.empty((int(L.mi_gemm_argmax_workspace_floats(M, N)),), device=a.device, dtype=torch.float32)
    rc = L.mi_gemm_argmax_bf16(a.data_ptr(), a.stride(0), w.data_ptr(), w.stride(0), _p(bias), best.data_ptr(), ws.data_ptr(), M, N, K, _stream())
    if rc == _lib.ERR_UNSUPPORTED:
        return row_argmax(gemm(a, w, bias, out_dtype=torch.float32))
    _lib.check(rc, "mi_gemm_argmax_bf16")
    return best


def gemm_ce(a, w, labels, *, return_target=False, bias=None):
    """the language-model head with its cross-entropy, without the logits: a (M, K), w (N, K) bf16, labels (M) int64 (negative = ignored, CrossEntropyLoss's ignore_index)
    -> (acc [sum of the valid rows' nll, their count] fp32, lse (M) fp32, nll (M) fp32 = lse - logit[label], exactly 0 on ignored rows) out of the GEMM's epilogue
    (mi_gemm_ce_f32: no (M, N) tensor is written).  Shapes outside that kernel: the fp32 GEMM into a scratch, row_lse and ce_label_smoothing(shift=0, eps=0).
    return_target: also the label's logit per row (M) fp32 (tests; undefined on ignored rows).  bias: (N) fp32 added to the logits (the folded multi-tap head's), or None."""
    _req(a, BF16); _req(w, BF16); _req(labels, torch.int64)
    M, K = a.shape
    N = w.shape[0]
    labels = labels.contiguous()
    L = _lib.lib()
    dev = a.device
    acc, lse, nll, tgt = (torch.empty((n,), device=dev, dtype=torch.float32) for n in (2, M, M, M))
    ws = torch.empty((int(L.mi_gemm_lse_workspace_floats(M, N)),), device=dev, dtype=torch.float32)
    rc = L.mi_gemm_ce_f32(a.data_ptr(), a.stride(0), w.data_ptr(), w.stride(0), _p(bias), labels.data_ptr(), acc.data_ptr(), lse.data_ptr(), nll.data_ptr(), tgt.data_ptr(),
                          ws.data_ptr(), M, N, K, _stream())
    if rc == _lib.ERR_UNSUPPORTED:
        logits = gemm(a, w, bias, out_dtype=torch.float32)
        lse = row_lse(logits)
        acc = torch.zeros((2,), device=dev, dtype=torch.float32)
        L_rc = L.mi_ce_label_smoothing(logits.data_ptr(), logits.stride(0), labels.data_ptr(), 1, M, 0, N, 0.0, acc.data_ptr(), nll.data_ptr(), _stream())
        _lib.check(L_rc, "mi_ce_label_smoothing")
        nll = torch.nan_to_num_(nll, nan=0.0)                           # the kernel marks ignored rows with NaN
        if return_target:
            tgt = logits.gather(1, labels.clamp(0, N - 1)[:, None])[:, 0]
    else:
        _lib.check(rc, "mi_gemm_ce_f32")
    return (acc, lse, nll, tgt) if return_target else (acc, lse, nll)


def rows_nll(logits, lse, labels):
    """logits (M, V) fp32 (contiguous rows, any row stride), lse (M) fp32 their log-sum-exp, labels (M) int64 -> nll (M) fp32 = lse - logits[m, labels[m]], exactly 0
    where labels[m] < 0 (or >= V): `gemm_ce`'s nll for the routes that materialise logits (mi_rows_nll_f32)."""
    _req(logits, torch.float32); _req(lse, torch.float32); _req(labels, torch.int64)
    if logits.dim() != 2 or logits.stride(1) != 1 or lse.shape != (logits.shape[0],) or labels.shape != (logits.shape[0],):
        raise TypeError("rows_nll: logits (M, V) fp32 with contiguous rows, lse (M) fp32, labels (M) int64")
    M, V = logits.shape
    lse, labels = lse.contiguous(), labels.contiguous()
    nll = torch.empty((M,), device=logits.device, dtype=torch.float32)
    rc = _lib.lib().mi_rows_nll_f32(logits.data_ptr(), logits.stride(0), lse.data_ptr(), labels.data_ptr(), V, nll.data_ptr(), M, _stream())
    _lib.check(rc, "mi_rows_nll_f32")
    return nll


def _nbest_tokens(tokens, what):
    if not isinstance(tokens, torch.Tensor) or tokens.dtype not in (torch.int32, torch.int64) or tokens.dim() != 3:
        raise TypeError(f"{what}: tokens must be (B, N, Tt) int32 / int64")
    _req(tokens)
    return tokens.contiguous()


def rescore_pack(tokens, n_tokens, ctc, *, vocab, U, start_id, eos_id, pad_id):
    """An n-best as the teacher-forced decoder's operands (mi_rescore_pack, csrc/rescore.hip): tokens (B, N, Tt) int32 | int64, n_tokens (B, N) int32, ctc (B, N) fp32
    -> dict(ids (B*N, U) int64 = [start, t_0 .. t_{k-1}, pad ..], labels (B*N, U) int64 = [t_0 .. t_{k-1}, eos, -100 ..], len (B*N) int32 = k + 1).  A hypothesis
    with a non-finite score, more than U - 1 tokens or a token outside [0, vocab) does not exist: ids = [start, pad ..], labels = -100, len = 0."""
    tokens = _nbest_tokens(tokens, "rescore_pack")
    B, N, Tt = tokens.shape
    _req(n_tokens, torch.int32); _req(ctc, torch.float32)
    if n_tokens.shape != (B, N) or ctc.shape != (B, N):
        raise ValueError(f"rescore_pack: n_tokens and ctc must be ({B}, {N})")
    if U < 1 or vocab < 1 or B < 1 or N < 1 or Tt < 1:
        raise ValueError(f"rescore_pack: B, N, Tt, vocab and U must be >= 1, got {B}, {N}, {Tt}, {vocab}, {U}")
    dev = tokens.device
    ids, labels = torch.empty((B * N, U), device=dev, dtype=torch.int64), torch.empty((B * N, U), device=dev, dtype=torch.int64)
    ln = torch.empty((B * N,), device=dev, dtype=torch.int32)
    rc = _lib.lib().mi_rescore_pack(tokens.data_ptr(), int(tokens.dtype == torch.int64), n_tokens.contiguous().data_ptr(), ctc.contiguous().data_ptr(), B, N, Tt, int(vocab),
                                    int(U), int(start_id), int(eos_id), int(pad_id), ids.data_ptr(), labels.data_ptr(), ln.data_ptr(), _stream())
    _lib.check(rc, "mi_rescore_pack")
    return dict(ids=ids, labels=labels, len=ln)


def rescore_select(nll, lens, ctc, denom, tokens, *, w_ctc, w_att, K, eos_id, pad_id, frames=None):
    """Rank the N <= 64 hypotheses of every utterance by the joint objective and gather the best K (mi_rescore_select, csrc/rescore.hip): nll (B*N*U) fp32 the decoder's
    per-position lse - logit[label], lens (B*N) int32, ctc (B, N) fp32, denom (U + 1) fp32 = l ** length_penalty from the host, tokens (B, N, Tt) the n-best, frames
    (B, N, Tt) int32 or None.  total = (w_ctc * ctc + w_att * att) / denom[len], att = -(the nll of positions u < len summed in ascending order); len = 0 and NaN count
    as -inf; descending total, equal totals by lower n.  -> dict(order (B, K) int32, total, att, ctc (B, K) fp32, token_lp (B, K, U) fp32 = -nll then 0, tokens (B, K, U)
    int64 = the tokens, eos, then pad, n_tokens (B, K) int32[, frames (B, K, U) int32 then -1]), best first."""
    tokens = _nbest_tokens(tokens, "rescore_select")
    B, N, Tt = tokens.shape
    _req(nll, torch.float32); _req(lens, torch.int32); _req(ctc, torch.float32); _req(denom, torch.float32)
    if not 1 <= N <= 64 or not 1 <= int(K) <= N:
        raise ValueError(f"rescore_select: 1 <= K <= N <= 64 required, got K = {K}, N = {N}")
    if nll.numel() % (B * N) or nll.numel() < B * N:
        raise ValueError(f"rescore_select: nll holds {nll.numel()} values for {B * N} hypotheses")
    U = nll.numel() // (B * N)
    if lens.numel() != B * N or ctc.numel() != B * N or denom.numel() != U + 1:
        raise ValueError(f"rescore_select: lens and ctc must hold {B * N} values and denom {U + 1}")
    K = int(K)
    dev = tokens.device
    if frames is not None:
        _req(frames, torch.int32)
        if frames.shape != tokens.shape:
            raise ValueError("rescore_select: frames must have the shape of tokens")
        frames = frames.contiguous()
    nll, lens, ctc, denom = nll.contiguous(), lens.contiguous(), ctc.contiguous(), denom.contiguous()
    order, out_n = torch.empty((B, K), device=dev, dtype=torch.int32), torch.empty((B, K), device=dev, dtype=torch.int32)
    total, att, ctc_o = (torch.empty((B, K), device=dev, dtype=torch.float32) for _ in range(3))
    tlp = torch.empty((B, K, U), device=dev, dtype=torch.float32)
    otok = torch.empty((B, K, U), device=dev, dtype=torch.int64)
    ofr = torch.empty((B, K, U), device=dev, dtype=torch.int32) if frames is not None else None
    rc = _lib.lib().mi_rescore_select(nll.data_ptr(), lens.data_ptr(), ctc.data_ptr(), denom.data_ptr(), float(w_ctc), float(w_att), B, N, U, K, tokens.data_ptr(),
                                      int(tokens.dtype == torch.int64), Tt, _p(frames), int(eos_id), int(pad_id), order.data_ptr(), total.data_ptr(), att.data_ptr(),
                                      ctc_o.data_ptr(), tlp.data_ptr(), otok.data_ptr(), out_n.data_ptr(), _p(ofr), _stream())
    _lib.check(rc, "mi_rescore_select")
    out = dict(order=order, total=total, att=att, ctc=ctc_o, token_lp=tlp, tokens=otok, n_tokens=out_n)
    if ofr is not None:
        out["frames"] = ofr
    return out


def _lengths_i32(lengths, B, device):
    if lengths is None:
        return None
    lengths = lengths.to(device=device, dtype=torch.int32).contiguous()
    if lengths.shape != (B,):
        raise ValueError(f"lengths: expected shape ({B},), got {tuple(lengths.shape)}")
    return lengths


def ctc_collapse(best, blank, pad_id, lengths=None, *, return_frames=False, dtype=torch.int64):
    """best (B, T) int32 per-frame classes -> dict(tokens (B, T) `dtype`, n_tokens (B) int32[, frames (B, T) int32]): frame t is kept iff t < n_b, best != blank and
    (t == 0 or best[t] != best[t-1]), n_b = lengths[b] or T; the kept ids in order, then pad_id (frames: where each kept token starts, then -1).  mi_ctc_collapse."""
    _req(best, torch.int32)
    if dtype not in (torch.int32, torch.int64):
        raise TypeError("ctc_collapse: token dtype int32 or int64")
    best = best.contiguous()
    B, T = best.shape
    lengths = _lengths_i32(lengths, B, best.device)
    tokens = torch.empty((B, T), device=best.device, dtype=dtype)
    n = torch.empty((B,), device=best.device, dtype=torch.int32)
    frames = torch.empty((B, T), device=best.device, dtype=torch.int32) if return_frames else None
    rc = _lib.lib().mi_ctc_collapse(best.data_ptr(), B, T, _p(lengths), int(blank), int(pad_id), tokens.data_ptr(), int(dtype == torch.int64), n.data_ptr(), _p(frames), _stream())
    _lib.check(rc, "mi_ctc_collapse")
    out = dict(tokens=tokens, n_tokens=n)
    if return_frames:
        out["frames"] = frames
    return out


def ctc_greedy_decode(logits, blank, pad_id, lengths=None, *, return_frames=False, dtype=torch.int64):
    """CTC greedy transcription of logits (B, T, V+1) f32|bf16 (last dim contiguous, any row / batch strides): per-frame argmax, repeats merged, blanks dropped.
    -> dict(tokens, n_tokens, best (B, T) int32[, frames]) as ctc_collapse; with lengths=None every frame counts (the reference's ctc_greedy_decode,
    src/utilities/eval_utils.py:37-43).  One pass over the logits + one block per utterance (mi_ctc_greedy)."""
    _req(logits)
    if logits.dtype not in (torch.float32, BF16) or logits.dim() != 3:
        raise TypeError("ctc_greedy_decode: (B, T, V+1) fp32 / bf16 logits")
    if logits.stride(2) != 1:
        logits = logits.contiguous()
    if dtype not in (torch.int32, torch.int64):
        raise TypeError("ctc_greedy_decode: token dtype int32 or int64")
    B, T, V1 = logits.shape
    lengths = _lengths_i32(lengths, B, logits.device)
    best = torch.empty((B, T), device=logits.device, dtype=torch.int32)
    tokens = torch.empty((B, T), device=logits.device, dtype=dtype)
    n = torch.empty((B,), device=logits.device, dtype=torch.int32)
    frames = torch.empty((B, T), device=logits.device, dtype=torch.int32) if return_frames else None
    rc = _lib.lib().mi_ctc_greedy(logits.data_ptr(), logits.stride(1), logits.stride(0), 0 if logits.dtype == torch.float32 else 1, B, T, V1, _p(lengths), int(blank), int(pad_id),
                                  best.data_ptr(), tokens.data_ptr(), int(dtype == torch.int64), n.data_ptr(), _p(frames), _stream())
    _lib.check(rc, "mi_ctc_greedy")
    out = dict(tokens=tokens, n_tokens=n, best=best)
    if return_frames:
        out["frames"] = frames
    return out


def _ctc_beam_logits(logits, blank, what):
    _req(logits)
    if logits.dtype not in (torch.float32, BF16) or logits.dim() != 3:
        raise TypeError(f"{what}: (B, T, V+1) fp32 / bf16 logits")
    if logits.shape[0] < 1 or logits.shape[1] < 1 or logits.shape[2] < 2:
        raise ValueError(f"{what}: at least one utterance, one frame and two classes, got {tuple(logits.shape)}")
    if not 0 <= int(blank) < logits.shape[2]:
        raise ValueError(f"{what}: blank {blank} outside [0, {logits.shape[2]})")
    return logits if logits.stride(2) == 1 else logits.contiguous()


def ctc_beam_cut(logits, blank, token_topk, lengths=None):
    """the first launch of ctc_beam_decode on its own (mi_ctc_beam_cut): logits (B, T, V+1) f32|bf16 -> dict(lse (B, T), lp_blank (B, T), lp (B, T, K) fp32,
    ids (B, T, K) int32): per frame t < n_b the row's log-sum-exp, the blank's log-probability and the min(K, V) non-blank classes with the largest logits, best first,
    equal values by lower class (entries past V: -inf / -1).  Rows past n_b are not written."""
    K = int(token_topk)
    if not 1 <= K <= 64:
        raise ValueError(f"ctc_beam_cut: token_topk must be in 1..64, got {token_topk}")
    logits = _ctc_beam_logits(logits, blank, "ctc_beam_cut")
    B, T, V1 = logits.shape
    dev = logits.device
    lengths = _lengths_i32(lengths, B, dev)
    lse, lpb = torch.empty((B, T), device=dev, dtype=torch.float32), torch.empty((B, T), device=dev, dtype=torch.float32)
    lp, ids = torch.empty((B, T, K), device=dev, dtype=torch.float32), torch.empty((B, T, K), device=dev, dtype=torch.int32)
    rc = _lib.lib().mi_ctc_beam_cut(logits.data_ptr(), logits.stride(1), logits.stride(0), 0 if logits.dtype == torch.float32 else 1, B, T, V1, _p(lengths), int(blank), K,
                                    lse.data_ptr(), lpb.data_ptr(), lp.data_ptr(), ids.data_ptr(), _stream())
    _lib.check(rc, "mi_ctc_beam_cut")
    return dict(lse=lse, lp_blank=lpb, lp=lp, ids=ids)


def _ctc_bias_type(what, bias):
    """bias=: None or a ctc_bias.CtcBias (TypeError otherwise)"""
    from .ctc_bias import CtcBias
    if bias is not None and not isinstance(bias, CtcBias):
        raise TypeError(f"{what}: bias is a ctc_bias.CtcBias or None, got {type(bias).__name__}")
    return bias


def _ctc_bias_fits(what, bias, V1, blank):
    """a context built for another vocabulary or blank is refused on the host, before anything touches the device"""
    if bias is not None and (bias.vocab != V1 or bias.blank != int(blank)):
        raise ValueError(f"{what}: the bias context was built for vocab {bias.vocab}, blank {bias.blank}; the logits have {V1} classes, blank {blank}")


def _ctc_bias_args(bias, dev):
    """the context arguments of a biased entry: bias_col, bias_tab, S, A1, weight"""
    col, tab = bias.to(dev)
    return col.data_ptr(), tab.data_ptr(), bias.S, bias.A1, bias.weight


def ctc_beam_decode(logits, blank, pad_id, lengths=None, *, beams, token_topk=None, nbest=1, return_frames=False, dtype=torch.int64, bias=None):
    """CTC prefix beam search (csrc/ctc_beam.hip states the semantics: the sum over alignments, not the flashlight decoder's max) of logits (B, T, V+1) f32|bf16
    (last dim contiguous, any row / batch strides) with `beams` <= 64 hypotheses per utterance over the `token_topk` <= 64 best non-blank classes of every frame
    (None: min(beams, V), as the reference passes beam_size_token = beam_size).  -> dict(tokens (B, nbest, T) `dtype` = each hypothesis' ids then pad_id, best first,
    n_tokens (B, nbest) int32, scores (B, nbest) fp32 = log of the summed alignment probability[, frames (B, nbest, T) int32 = the frame at which each token's prefix
    entered the beam, then -1]); hypotheses that do not exist: 0 tokens, score -inf.  lengths (B): frames that count per utterance (None: all).  Two launches.
    bias (a ctc_bias.CtcBias built for these V + 1 classes and this blank): contextual biasing, csrc/ctc_beam_bias.hip — hypotheses are selected and ranked by
    score + weight * credit, scores stay the CTC log-probabilities, and the dict gains credit (B, nbest) int32 (0 for hypotheses that do not exist)."""
    _ctc_bias_type("ctc_beam_decode", bias)
    if not isinstance(beams, int) or isinstance(beams, bool) or not isinstance(nbest, int) or isinstance(nbest, bool):
        raise TypeError("ctc_beam_decode: beams and nbest are ints")
    if token_topk is not None and (not isinstance(token_topk, int) or isinstance(token_topk, bool)):
        raise TypeError("ctc_beam_decode: token_topk is an int or None")
    if not 1 <= beams <= 64:
        raise ValueError(f"ctc_beam_decode: beams must be in 1..64, got {beams}")
    if not 1 <= nbest <= beams:
        raise ValueError(f"ctc_beam_decode: nbest must be in 1..beams, got {nbest} with {beams} beams")
    if token_topk is not None and not 1 <= token_topk <= 64:
        raise ValueError(f"ctc_beam_decode: token_topk must be in 1..64, got {token_topk}")
    if dtype not in (torch.int32, torch.int64):
        raise TypeError("ctc_beam_decode: token dtype int32 or int64")
    if not isinstance(logits, torch.Tensor) or logits.dim() != 3:
        raise TypeError("ctc_beam_decode: (B, T, V+1) fp32 / bf16 logits")
    _ctc_bias_fits("ctc_beam_decode", bias, logits.shape[2], blank)
    logits = _ctc_beam_logits(logits, blank, "ctc_beam_decode")
    B, T, V1 = logits.shape
    K = min(beams, V1 - 1) if token_topk is None else token_topk
    dev = logits.device
    lengths = _lengths_i32(lengths, B, dev)
    cut = ctc_beam_cut(logits, blank, K, lengths)
    L = _lib.lib()
    nbytes = int(L.mi_ctc_beam_workspace_bytes(B, T, beams))
    if nbytes == 0:
        raise ValueError(f"ctc_beam_decode: {T} frames x {beams} beams is beyond the node table (T * beams < 2^22 - 2)")
    ws = torch.empty((nbytes,), device=dev, dtype=torch.uint8)
    tokens = torch.empty((B, nbest, T), device=dev, dtype=dtype)
    n = torch.empty((B, nbest), device=dev, dtype=torch.int32)
    scores = torch.empty((B, nbest), device=dev, dtype=torch.float32)
    frames = torch.empty((B, nbest, T), device=dev, dtype=torch.int32) if return_frames else None
    args = (logits.data_ptr(), logits.stride(1), logits.stride(0), 0 if logits.dtype == torch.float32 else 1, B, T, V1, _p(lengths), int(blank), int(pad_id),
            beams, K, nbest, cut["lse"].data_ptr(), cut["lp_blank"].data_ptr(), cut["lp"].data_ptr(), cut["ids"].data_ptr(), ws.data_ptr(), nbytes,
            tokens.data_ptr(), int(dtype == torch.int64), n.data_ptr(), scores.data_ptr(), _p(frames))
    out = dict(tokens=tokens, n_tokens=n, scores=scores)
    if bias is None:
        _lib.check(L.mi_ctc_beam_walk(*args, _stream()), "mi_ctc_beam_walk")
    else:
        out["credit"] = torch.empty((B, nbest), device=dev, dtype=torch.int32)
        _lib.check(L.mi_ctc_beam_walk_bias(*args, *_ctc_bias_args(bias, dev), out["credit"].data_ptr(), _stream()), "mi_ctc_beam_walk_bias")
    if return_frames:
        out["frames"] = frames
    return out


def _beam_stream_args(what, count_name, count_noun, count, max_frames, beams, token_topk, nbest, blank, dtype):
    """the constructor checks of CtcBeamStream and CtcBeamPool: one table, one wording"""
    ints = lambda *v: all(isinstance(x, int) and not isinstance(x, bool) for x in v)
    if not ints(count, max_frames, beams, nbest, blank):
        raise TypeError(f"{what}: {count_name}, max_frames, beams, nbest and blank are ints")
    if token_topk is not None and not ints(token_topk):
        raise TypeError(f"{what}: token_topk is an int or None")
    if count < 1 or max_frames < 1:
        raise ValueError(f"{what}: at least one {count_noun} and one frame, got {count_name}={count}, max_frames={max_frames}")
    if not 1 <= beams <= 64:
        raise ValueError(f"{what}: beams must be in 1..64, got {beams}")
    if not 1 <= nbest <= beams:
        raise ValueError(f"{what}: nbest must be in 1..beams, got {nbest} with {beams} beams")
    if token_topk is not None and not 1 <= token_topk <= 64:
        raise ValueError(f"{what}: token_topk must be in 1..64, got {token_topk}")
    if blank < 0:
        raise ValueError(f"{what}: blank {blank} is negative")
    if dtype not in (torch.int32, torch.int64):
        raise TypeError(f"{what}: token dtype int32 or int64")


class CtcBeamStream:
    """CTC prefix beam search on a stream (csrc/ctc_beam_stream.hip states the semantics): ctc_beam_decode's walk for `batch` streams in lock-step, suspended between
    calls.  After every `feed` the beam is bit for bit the beam ctc_beam_decode holds after the same frames of the concatenated logits, however they were split.

        st = ops.CtcBeamStream(B, max_frames, beams=10, blank=V, pad_id=0)
        out = st.feed(logits)                      # (B, T_call, V+1) f32|bf16; T_call = 0 is allowed
        out = st.feed(logits, n_valid, final=True) # the last rows: n_valid (B) of them count per stream

    feed -> dict(committed (B, max_frames) int32, committed_frames (B, max_frames) int32, n_committed (B) int32, n_new (B) int32): the tokens every hypothesis of the beam
    begins with — they can no longer change —, the frame at which each entered the beam, how many there are and how many this call appended.  These four are the
    object's own buffers: the next call updates them in place.  With partial=True, and always with final=True, also tokens (B, nbest, max_frames) `dtype`, n_tokens,
    scores[, frames] as ctc_beam_decode returns them; after final=True committed[:n_committed] is hypothesis 0.  Without them a call does no backtrace.
    mi_ctc_beam_cut on the call's rows, then mi_ctc_beam_stream_walk: two launches, no host synchronisation.  The object counts T_call per call as the frames walked
    (an upper bound when n_valid is given: the counts stay on the device) and refuses, before any launch, a call that could pass max_frames.
    bias (a ctc_bias.CtcBias for the logits' V + 1 classes and this blank): contextual biasing as ctc_beam_decode(bias=) — csrc/ctc_beam_bias_stream.hip; the state
    grows by 512 B per stream, the walk is mi_ctc_beam_bias_stream_walk, and credit (B, nbest) int32 comes wherever the n-best do."""

    def __init__(self, batch, max_frames, *, beams, token_topk=None, nbest=1, blank, pad_id, dtype=torch.int64, return_frames=False, bias=None):
        _beam_stream_args("CtcBeamStream", "batch", "stream", batch, max_frames, beams, token_topk, nbest, blank, dtype)
        self.bias = _ctc_bias_type("CtcBeamStream", bias)
        if bias is not None and bias.blank != blank:
            raise ValueError(f"CtcBeamStream: the bias context was built for blank {bias.blank}, not {blank}")
        self.B, self.max_frames, self.beams, self.token_topk, self.nbest = batch, max_frames, beams, token_topk, nbest
        self.blank, self.pad_id, self.dtype, self.return_frames = blank, int(pad_id), dtype, bool(return_frames)
        self._fn = "mi_ctc_beam_stream" if bias is None else "mi_ctc_beam_bias_stream"      # the entries' common prefix: _state_bytes, _reset, _walk
        self.state_bytes = int(getattr(_lib.lib(), self._fn + "_state_bytes")(batch, max_frames, beams))
        if self.state_bytes == 0:
            raise ValueError(f"CtcBeamStream: {max_frames} frames x {beams} beams is beyond the node table (max_frames * beams < 2^22 - 2)")
        self.walked = 0                            # host upper bound of the frames any stream has walked
        self.finished = False
        self.V1 = None
        self._state = None

    def _allocate(self, dev):
        B, M = self.B, self.max_frames
        self._state = torch.empty((self.state_bytes,), device=dev, dtype=torch.uint8)
        self.committed = torch.empty((B, M), device=dev, dtype=torch.int32)
        self.committed_frames = torch.empty((B, M), device=dev, dtype=torch.int32)
        self.n_committed = torch.empty((B,), device=dev, dtype=torch.int32)
        self.n_new = torch.empty((B,), device=dev, dtype=torch.int32)
        self._reset_device()

    def _reset_device(self):
        rc = getattr(_lib.lib(), self._fn + "_reset")(self._state.data_ptr(), self.state_bytes, self.B, self.max_frames, self.beams, _stream())
        _lib.check(rc, self._fn + "_reset")
        self.committed.fill_(self.pad_id)
        self.committed_frames.fill_(-1)
        self.n_committed.zero_()
        self.n_new.zero_()

    def reset(self):
        """every stream back to its start: nothing walked, nothing committed"""
        self.walked = 0
        self.finished = False
        if self._state is not None:
            self._reset_device()

    def feed(self, logits, n_valid=None, *, final=False, partial=False):
        if self.finished:
            raise RuntimeError("CtcBeamStream.feed: the streams are finished (final=True was fed); reset() starts new ones")
        if not isinstance(logits, torch.Tensor) or logits.dim() != 3 or logits.dtype not in (torch.float32, BF16):
            raise TypeError("CtcBeamStream.feed: (B, T_call, V+1) fp32 / bf16 logits")
        B, T, V1 = logits.shape
        if B != self.B or V1 < 2 or self.blank >= V1 or (self.V1 is not None and V1 != self.V1):
            raise ValueError(f"CtcBeamStream.feed: logits of ({self.B}, T_call, {self.V1 or 'V+1'}) with blank {self.blank} inside, got {tuple(logits.shape)}")
        if n_valid is not None and not isinstance(n_valid, torch.Tensor):
            n_valid = torch.tensor([int(v) for v in n_valid], dtype=torch.int32)
        if n_valid is not None and tuple(n_valid.shape) != (B,):
            raise ValueError(f"CtcBeamStream.feed: n_valid: expected shape ({B},), got {tuple(n_valid.shape)}")
        _ctc_bias_fits("CtcBeamStream.feed", self.bias, V1, self.blank)
        if self.walked + T > self.max_frames:
            raise RuntimeError(f"CtcBeamStream.feed: {self.walked} + {T} frames exceed max_frames={self.max_frames}")
        _req(logits)
        dev = logits.device
        extra = ()
        if self.bias is not None:
            extra = _ctc_bias_args(self.bias, dev)
        if T and logits.stride(2) != 1:
            logits = logits.contiguous()
        K = min(self.beams, V1 - 1) if self.token_topk is None else self.token_topk
        n_valid = _lengths_i32(n_valid, B, dev)
        if self._state is None:
            self._allocate(dev)
        cut = ctc_beam_cut(logits, self.blank, K, n_valid) if T else dict(lse=None, lp_blank=None, lp=None, ids=None)
        want = bool(final or partial)
        nb, M = self.nbest, self.max_frames
        tokens = torch.empty((B, nb, M), device=dev, dtype=self.dtype) if want else None
        n = torch.empty((B, nb), device=dev, dtype=torch.int32) if want else None
        scores = torch.empty((B, nb), device=dev, dtype=torch.float32) if want else None
        frames = torch.empty((B, nb, M), device=dev, dtype=torch.int32) if want and self.return_frames else None
        credit = torch.empty((B, nb), device=dev, dtype=torch.int32) if want and self.bias is not None else None
        if self.bias is not None:
            extra = (*extra, _p(credit))
        rc = getattr(_lib.lib(), self._fn + "_walk")(logits.data_ptr() if T else None, logits.stride(1) if T else 0, logits.stride(0) if T else 0,
                                                     0 if logits.dtype == torch.float32 else 1, B, T, V1, _p(n_valid), self.blank, self.pad_id, self.beams, K, nb,
                                                     _p(cut["lse"]), _p(cut["lp_blank"]), _p(cut["lp"]), _p(cut["ids"]), self._state.data_ptr(), self.state_bytes, M,
                                                     int(bool(final)), self.committed.data_ptr(), self.committed_frames.data_ptr(), self.n_committed.data_ptr(),
                                                     self.n_new.data_ptr(), _p(tokens), int(self.dtype == torch.int64), _p(n), _p(scores), _p(frames), *extra, _stream())
        _lib.check(rc, self._fn + "_walk")
        self.V1 = V1
        self.walked += T
        self.finished = bool(final)
        out = dict(committed=self.committed, committed_frames=self.committed_frames, n_committed=self.n_committed, n_new=self.n_new)
        if want:
            out.update(tokens=tokens, n_tokens=n, scores=scores)
            if self.return_frames:
                out["frames"] = frames
            if credit is not None:
                out["credit"] = credit
        return out


class CtcBeamPool:
    """CTC prefix beam search on the slots of a session pool (csrc/ctc_beam_pool.hip states the semantics): CtcBeamStream's walk per slot, every slot a session with
    rows, an end and a start of its own.  A session's beam is bit for bit that of `CtcBeamStream(1, ...)` fed the same pieces, whatever the other slots do.

        bp = ops.CtcBeamPool(slots, max_frames, beams=10, blank=V, pad_id=0)
        bp.open(slot)                              # the slot back to a stream start; no other slot is touched
        out = bp.step(logits, [(slot, row0, n, final, partial), ...])      # logits (rows, V+1) f32|bf16: the step's compact rows; a record's rows are [row0, row0 + n)

    step -> dict(committed, committed_frames (slots, max_frames) int32, n_committed, n_new (slots) int32): the pool's own buffers, a row per slot, updated in place by
    the next call that names the slot and cleared by its next `open`.  For the records with final or partial also tokens (R, nbest, max_frames) `dtype`, n_tokens,
    scores (R, nbest)[, frames], compact in record order, and rows {slot: row}.  mi_ctc_beam_cut over the compact rows (skipped without rows), then
    mi_ctc_beam_stream_walk_slots: at most two launches, no host synchronisation.  `walked[slot]` counts a session's frames exactly (every row of a record is valid);
    a record that would pass max_frames, or names a slot that is not open or already final, is refused before any launch.
    bias (a ctc_bias.CtcBias): contextual biasing, one context per pool shared by all slots (csrc/ctc_beam_bias_pool.hip); credit (R, nbest) comes beside scores."""

    REC_WORDS = 5

    def __init__(self, slots, max_frames, *, beams, token_topk=None, nbest=1, blank, pad_id, dtype=torch.int64, return_frames=False, bias=None):
        _beam_stream_args("CtcBeamPool", "slots", "slot", slots, max_frames, beams, token_topk, nbest, blank, dtype)
        self.bias = _ctc_bias_type("CtcBeamPool", bias)                    # one context per pool, shared by all slots
        if bias is not None and bias.blank != blank:
            raise ValueError(f"CtcBeamPool: the bias context was built for blank {bias.blank}, not {blank}")
        self.S, self.max_frames, self.beams, self.token_topk, self.nbest = slots, max_frames, beams, token_topk, nbest
        self.blank, self.pad_id, self.dtype, self.return_frames = blank, int(pad_id), dtype, bool(return_frames)
        self._fn = "mi_ctc_beam_stream" if bias is None else "mi_ctc_beam_bias_stream"      # the entries' common prefix: _state_bytes, _reset, _reset_slot, _walk_slots
        self.state_bytes = int(getattr(_lib.lib(), self._fn + "_state_bytes")(slots, max_frames, beams))
        if self.state_bytes == 0:
            raise ValueError(f"CtcBeamPool: {max_frames} frames x {beams} beams is beyond the node table (max_frames * beams < 2^22 - 2)")
        self.walked = [0] * slots                  # frames the slot's session has walked
        self.is_open = [False] * slots             # opened and not yet final
        self.V1 = None
        self._state = None

    def _allocate(self, dev):
        """the state of all slots, every one at a stream start (a slot opened before this needs no reset of its own)"""
        S, M = self.S, self.max_frames
        self._state = torch.empty((self.state_bytes,), device=dev, dtype=torch.uint8)
        self.committed = torch.full((S, M), self.pad_id, device=dev, dtype=torch.int32)
        self.committed_frames = torch.full((S, M), -1, device=dev, dtype=torch.int32)
        self.n_committed = torch.zeros((S,), device=dev, dtype=torch.int32)
        self.n_new = torch.zeros((S,), device=dev, dtype=torch.int32)
        rc = getattr(_lib.lib(), self._fn + "_reset")(self._state.data_ptr(), self.state_bytes, S, M, self.beams, _stream())
        _lib.check(rc, self._fn + "_reset")

    def open(self, slot):
        """the slot back to a stream start: its beam state (mi_ctc_beam_stream_reset_slot: one launch and a memset of the slot's node table), its committed row to pad,
        committed_frames to -1, its counts to 0, walked[slot] = 0.  Before the first device step there is no state yet: it is then created with every slot at its start."""
        if not isinstance(slot, int) or isinstance(slot, bool) or not 0 <= slot < self.S:
            raise ValueError(f"CtcBeamPool.open: slot {slot!r} outside [0, {self.S})")
        if self._state is not None:
            rc = getattr(_lib.lib(), self._fn + "_reset_slot")(self._state.data_ptr(), self.state_bytes, self.S, self.max_frames, self.beams, slot, _stream())
            _lib.check(rc, self._fn + "_reset_slot")
            self.committed[slot].fill_(self.pad_id)
            self.committed_frames[slot].fill_(-1)
            self.n_committed[slot].zero_()
            self.n_new[slot].zero_()
        self.walked[slot] = 0
        self.is_open[slot] = True

    def records(self, records, rows):
        """the checked records of a step -> (A x [slot, row0, n, final, out], rows {slot: out} of the records with final or partial); host arithmetic, nothing moves"""
        recs, outs = [], {}
        for r in records:
            if len(r) != 5:
                raise ValueError(f"CtcBeamPool.step: a record is (slot, row0, n, final, partial), got {r!r}")
            slot, row0, n, final, partial = r
            if not all(isinstance(v, int) and not isinstance(v, bool) for v in (slot, row0, n)):
                raise TypeError(f"CtcBeamPool.step: slot, row0 and n are ints, got {r!r}")
            if not 0 <= slot < self.S or not self.is_open[slot]:
                raise RuntimeError(f"CtcBeamPool.step: slot {slot} holds no open beam (not opened, or already final): open() starts one")
            if slot in (q[0] for q in recs):
                raise ValueError(f"CtcBeamPool.step: slot {slot} is named twice")
            if row0 < 0 or n < 0 or row0 + n > rows:
                raise ValueError(f"CtcBeamPool.step: rows [{row0}, {row0} + {n}) of slot {slot} lie outside the {rows} rows of the logits")
            if self.walked[slot] + n > self.max_frames:
                raise RuntimeError(f"CtcBeamPool.step: {self.walked[slot]} + {n} frames of slot {slot} exceed max_frames={self.max_frames}")
            out = -1
            if final or partial:
                out = outs[slot] = len(outs)
            recs.append([slot, row0, n, int(bool(final)), out])
        if not recs:
            raise ValueError("CtcBeamPool.step: no records")
        return recs, outs

    def step(self, logits, records, *, records_dev=None):
        """records_dev: the checked records (`self.records`) as 5 A int32 on the device, when the caller has uploaded them with a transfer of its own (StreamPool: they
        ride behind the step's descriptor table); None: they are uploaded here from a pinned buffer."""
        if not isinstance(logits, torch.Tensor) or logits.dim() != 2 or logits.dtype not in (torch.float32, BF16):
            raise TypeError("CtcBeamPool.step: (rows, V+1) fp32 / bf16 logits")
        rows, V1 = logits.shape
        if V1 < 2 or self.blank >= V1 or (self.V1 is not None and V1 != self.V1):
            raise ValueError(f"CtcBeamPool.step: logits of (rows, {self.V1 or 'V+1'}) with blank {self.blank} inside, got {tuple(logits.shape)}")
        _ctc_bias_fits("CtcBeamPool.step", self.bias, V1, self.blank)
        recs, outs = self.records(records, rows)
        _req(logits)
        dev = logits.device
        extra = ()
        if self.bias is not None:
            extra = _ctc_bias_args(self.bias, dev)
        if rows and logits.stride(1) != 1:
            logits = logits.contiguous()
        A, R, nb, M = len(recs), len(outs), self.nbest, self.max_frames
        K = min(self.beams, V1 - 1) if self.token_topk is None else self.token_topk
        host = torch.tensor(recs, dtype=torch.int32).reshape(-1)
        if records_dev is None:
            pinned = torch.empty((A * self.REC_WORDS,), dtype=torch.int32, pin_memory=True)
            pinned.copy_(host)
            records_dev = pinned.to(dev, non_blocking=True)
        elif records_dev.dtype != torch.int32 or records_dev.numel() != A * self.REC_WORDS or not records_dev.is_cuda or not records_dev.is_contiguous():
            raise ValueError(f"CtcBeamPool.step: records_dev holds the {A} x {self.REC_WORDS} int32 of the records on the device")
        if self._state is None:
            self._allocate(dev)
        if rows:
            cut = ctc_beam_cut(logits.unsqueeze(0), self.blank, K)
            lse, lpb, lp, ids = cut["lse"], cut["lp_blank"], cut["lp"], cut["ids"]
        else:
            lse = lpb = lp = ids = None
        tokens = torch.empty((R, nb, M), device=dev, dtype=self.dtype) if R else None
        n = torch.empty((R, nb), device=dev, dtype=torch.int32) if R else None
        scores = torch.empty((R, nb), device=dev, dtype=torch.float32) if R else None
        frames = torch.empty((R, nb, M), device=dev, dtype=torch.int32) if R and self.return_frames else None
        credit = torch.empty((R, nb), device=dev, dtype=torch.int32) if R and self.bias is not None else None
        if self.bias is not None:
            extra = (*extra, _p(credit))
        rc = getattr(_lib.lib(), self._fn + "_walk_slots")(logits.data_ptr() if rows else None, logits.stride(0) if rows else 0, 0 if logits.dtype == torch.float32 else 1, rows,
                                                           V1, self.blank, self.pad_id, self.beams, K, nb, _p(lse), _p(lpb), _p(lp), _p(ids), self._state.data_ptr(),
                                                           self.state_bytes, self.S, M, host.data_ptr(), A, records_dev.data_ptr(), self.committed.data_ptr(),
                                                           self.committed_frames.data_ptr(), self.n_committed.data_ptr(), self.n_new.data_ptr(), _p(tokens),
                                                           int(self.dtype == torch.int64), _p(n), _p(scores), _p(frames), R, *extra, _stream())
        _lib.check(rc, self._fn + "_walk_slots")
        self.V1 = V1
        for slot, _, cnt, final, _ in recs:
            self.walked[slot] += cnt
            if final:
                self.is_open[slot] = False
        out = dict(committed=self.committed, committed_frames=self.committed_frames, n_committed=self.n_committed, n_new=self.n_new, rows=outs)
        if R:
            out.update(tokens=tokens, n_tokens=n, scores=scores)
            if self.return_frames:
                out["frames"] = frames
            if credit is not None:
                out["credit"] = credit
        return out


def ctc_loss(logits, labels, in_len, *, reduction="mean", zero_infinity=False, lse=None):
    """logits (B,T,V+1) f32|bf16 (blank = last class), labels (B,U) int64 (<0 = padding), in_len (B) int32.
    Returns (loss scalar tensor | per-utterance nll for reduction='none', nll (B), tgt_len (B))."""
    B, T, V1 = logits.shape
    labels = labels.contiguous()
    U = labels.shape[1]
    if lse is None:
        lse = row_lse(logits.reshape(B * T, V1))
    nll = torch.empty((B,), device=logits.device, dtype=torch.float32)
    tl = torch.empty((B,), device=logits.device, dtype=torch.int32)
    loss = torch.empty((1,), device=logits.device, dtype=torch.float32)
    rc = _lib.lib().mi_ctc_loss_fwd(logits.data_ptr(), logits.stride(0), logits.stride(1), 0 if logits.dtype == torch.float32 else 1,
                                    lse.data_ptr(), T, labels.data_ptr(), U, in_len.data_ptr(), V1 - 1, B,
                                    1 if reduction == "mean" else 0, int(zero_infinity), nll.data_ptr(), tl.data_ptr(),
                                    loss.data_ptr(), _stream())
    _lib.check(rc, "mi_ctc_loss_fwd")
    if reduction == "none":
        out = torch.where(torch.isinf(nll), torch.zeros_like(nll), nll) if zero_infinity else nll
        return out, nll, tl
    return loss[0], nll, tl


def _row_lse_3d(logits):
    """the rows' log-sum-exp of (B, T, V1) logits with contiguous rows and any (batch, row) strides -> (B*T) fp32, without copying them: mi_row_lse's bits"""
    B, T, V1 = logits.shape
    if B == 1 or logits.stride(0) == T * logits.stride(1):
        return row_lse(logits.as_strided((B * T, V1), (logits.stride(1), 1)))
    return torch.cat([row_lse(logits[b]) for b in range(B)])


def ctc_align(logits, labels, in_len=None, *, blank=None, lse=None, return_spans=True):
    """CTC forced alignment (csrc/ctc_align.hip states the exact semantics): the best path of each transcript through logits (B, T, V1) f32|bf16 (last dim contiguous,
    any row / batch strides).  labels (B, U) int64: a row's non-negative entries, in order, are its target (negatives are padding wherever they stand); in_len (B) int32:
    the frames that count (None: all T); blank: None = the last class; lse (B*T) fp32: the rows' log-sum-exp when the caller already holds it (None: ops.row_lse runs first).
    -> dict(path (B, T) int32 = the class of every counted frame on the best path, then -1; score (B) fp32 = its log-probability; tgt_len (B) int32[; start, end (B, U) int32:
    token u emits on frames [start, end), then -1; token_lp (B, U) fp32 = the token's summed log-probability over them, then 0]).  Utterances that cannot be aligned (fewer
    frames than the target needs, a label >= V1 or == blank): score -inf, path / start / end -1, token_lp 0.  One launch, one block per utterance, bit-identical run to run."""
    if not isinstance(logits, torch.Tensor) or logits.dtype not in (torch.float32, BF16):
        raise ValueError("ctc_align: logits must be an fp32 or bf16 tensor")
    if logits.dim() != 3 or logits.shape[0] < 1 or logits.shape[1] < 1 or logits.shape[2] < 2:
        raise ValueError(f"ctc_align: logits must be (B, T, V1) with at least one utterance, one frame and two classes, got {tuple(logits.shape)}")
    if logits.stride(2) != 1:
        raise ValueError("ctc_align: the last dimension of logits must be contiguous")
    B, T, V1 = logits.shape
    if not isinstance(labels, torch.Tensor) or labels.dtype != torch.int64 or labels.dim() != 2 or labels.shape[0] != B:
        raise ValueError(f"ctc_align: labels must be ({B}, U) int64")
    if in_len is not None and (not isinstance(in_len, torch.Tensor) or in_len.dtype != torch.int32 or in_len.shape != (B,)):
        raise ValueError(f"ctc_align: in_len must be ({B},) int32")
    if lse is not None and (not isinstance(lse, torch.Tensor) or lse.dtype != torch.float32 or lse.numel() != B * T):
        raise ValueError(f"ctc_align: lse must hold {B * T} fp32 values")
    blank = V1 - 1 if blank is None else int(blank)
    if not 0 <= blank < V1:
        raise ValueError(f"ctc_align: blank {blank} outside [0, {V1})")
    U = labels.shape[1]
    for t in (logits, labels, in_len, lse):
        if t is not None:
            _req(t)
    dev = logits.device
    labels = labels.contiguous()
    in_len = torch.full((B,), T, device=dev, dtype=torch.int32) if in_len is None else in_len.contiguous()
    lse = _row_lse_3d(logits) if lse is None else lse.contiguous()
    L = _lib.lib()
    nbytes = int(L.mi_ctc_align_workspace_bytes(B, T, U))
    ws = torch.empty((nbytes,), device=dev, dtype=torch.uint8) if nbytes else None
    path = torch.empty((B, T), device=dev, dtype=torch.int32)
    score = torch.empty((B,), device=dev, dtype=torch.float32)
    tl = torch.empty((B,), device=dev, dtype=torch.int32)
    start, end = (torch.empty((B, U), device=dev, dtype=torch.int32) for _ in range(2)) if return_spans else (None, None)
    tlp = torch.empty((B, U), device=dev, dtype=torch.float32) if return_spans else None
    rc = L.mi_ctc_align(logits.data_ptr(), logits.stride(0), logits.stride(1), 0 if logits.dtype == torch.float32 else 1, lse.data_ptr(), T, labels.data_ptr(), U,
                        in_len.data_ptr(), blank, V1, B, _p(ws), nbytes, path.data_ptr(), score.data_ptr(), tl.data_ptr(), _p(start), _p(end), _p(tlp), _stream())
    _lib.check(rc, "mi_ctc_align")
    out = dict(path=path, score=score, tgt_len=tl)
    if return_spans:
        out.update(start=start, end=end, token_lp=tlp)
    return out


def embed_tokens(ids, wte, pos, *, scale=1.0, pos_offset=0, U=None):
    """ids (B,U) int64 -> (B*U, d) fp32 = wte[ids]*scale + pos[pos_offset + u]."""
    ids = ids.contiguous()
    M = ids.numel()
    U = ids.shape[-1] if U is None else U
    V, d = wte.shape
    out = torch.empty((M, d), device=ids.device, dtype=torch.float32)
    rc = _lib.lib().mi_embed_tokens(ids.data_ptr(), wte.data_ptr(), float(scale), pos.data_ptr(), pos_offset, U, d, M, V, out.data_ptr(), _stream())
    _lib.check(rc, "mi_embed_tokens")
    return out


def ce_label_smoothing(logits, labels, *, shift=1, eps=0.0, return_acc=False):
    """mean over valid targets of the label-smoothed CE of logits[b,u] vs labels[b,u+shift] (ignore < 0). logits (B,U,V) fp32.
    return_acc: hand back the kernel's [sum, count] pair instead, undivided — what `ops_train.ce_label_smoothing_bwd` reads, and what a caller that wants the sum needs."""
    B, U, V = logits.shape
    labels = labels.contiguous()
    acc = torch.zeros((2,), device=logits.device, dtype=torch.float32)
    rows = torch.empty((B * (U - shift),), device=logits.device, dtype=torch.float32)       # per-row losses; summed by one block in a fixed order
    rc = _lib.lib().mi_ce_label_smoothing(logits.data_ptr(), logits.stride(1), labels.data_ptr(), B, U, shift, V, float(eps), acc.data_ptr(), rows.data_ptr(), _stream())
    _lib.check(rc, "mi_ce_label_smoothing")
    return acc if return_acc else acc[0] / acc[1]


def cast_bf16(x):
    """(M,d) fp32 -> bf16 (round to nearest even) on the HIP path."""
    M, d = x.shape
    out = torch.empty((M, d), device=x.device, dtype=BF16)
    rc = _lib.lib().mi_cast_f32_bf16(x.data_ptr(), x.stride(0), out.data_ptr(), out.stride(0), M, d, _stream())
    _lib.check(rc, "mi_cast_f32_bf16")
    return out


# ---------------------------------------------------------------------------------------------------- streaming inference (csrc/stream.hip)
def attention_chunk(q, k_cache, v_cache, n_k, H, *, pos=None, bias_u=None, bias_v=None, scale=None, ref=0):
    """q (B, n_q, d) bf16 = the new rows' queries; k_cache / v_cache (B, Lmax, d) bf16 row views of one cache (same strides) whose first n_k rows are keys, the new rows'
    own last; query i sees keys j <= n_k - n_q + i.  pos (>= n_k, d) bf16 = the projected sinusoid of distance i - j in row i - j, with bias_u / bias_v (d) fp32 (all
    three or none).  ref 0..3: whose key walk the bf16 rounding of the probabilities follows (0 the row maximum; 1 / 2 / 3 the full forward's kernels).
    -> (B, n_q, d) bf16.  mi_attention_chunk_bf16."""
    _req(q, BF16); _req(k_cache, BF16); _req(v_cache, BF16)
    B, n_q, d = q.shape
    q = q.contiguous()
    if k_cache.stride() != v_cache.stride() or k_cache.stride(2) != 1:
        raise ValueError("attention_chunk: k_cache and v_cache must be row views with equal strides")
    hd = d // H
    out = torch.empty((B, n_q, d), device=q.device, dtype=BF16)
    rc = _lib.lib().mi_attention_chunk_bf16(q.data_ptr(), d, k_cache.data_ptr(), k_cache.stride(1), v_cache.data_ptr(), v_cache.stride(1), k_cache.stride(0),
                                            _p(pos), 0 if pos is None else pos.stride(0), _p(bias_u), _p(bias_v), out.data_ptr(), d, B, n_q, int(n_k), H, hd,
                                            float(scale if scale is not None else 1.0 / math.sqrt(hd)), int(ref), _stream())
    _lib.check(rc, "mi_attention_chunk_bf16")
    return out


DWCONV_STREAM_MODES = {"csgu": 0, "merge": 1, "conv": 2}


def dwconv_stream(x, w, bias, ring, *, mode, p, K, dil=1, left, o0, n_out, ring_stats=None, stats=None, gamma=None, beta=None, mul=None, end=None, act=0):
    """Stateful depthwise conv over time (mi_dwconv_stream_bf16): x (B, n_new, C) bf16 (last dim contiguous, any row stride; batch b at row b * n_new) = rows
    [p, p + n_new); ring (B, Hr, C) bf16 = rows [p - Hr, p) at slot t % Hr, advanced in place (ring_stats (B, ceil(C/64), Hr, 2) fp32 with modes "csgu" / "conv");
    -> (B, n_out, C) bf16 = rows [o0, o0 + n_out).  mode "csgu": x_r * act(conv(LN(x_g)) + b) with stats (B * n_new, 2), gamma, beta, mul = x_r; "merge": x + conv(x)
    + b, rows >= end[b] zero (a stream ends among the rows of the call that carries `end`, or where they end: end[b] >= p); "conv": the conv of "csgu" alone."""
    _req(x, BF16); _req(ring, BF16)
    B, n_new, Cc = x.shape
    Hr = ring.shape[1]
    out = torch.empty((B, n_out, Cc), device=x.device, dtype=BF16)
    if end is not None:
        end = _lengths_i32(end, B, x.device)
    rc = _lib.lib().mi_dwconv_stream_bf16(x.data_ptr(), x.stride(1) if n_new else Cc, _p(mul), 0 if mul is None else mul.stride(1), _p(stats), _p(gamma), _p(beta), w.data_ptr(), _p(bias),
                                          ring.data_ptr() if Hr else 0, _p(ring_stats), _p(end), out.data_ptr(), Cc, B, Cc, int(K), int(dil), int(left), Hr, int(p), n_new,
                                          int(o0), int(n_out), DWCONV_STREAM_MODES[mode], int(act), _stream())
    _lib.check(rc, "mi_dwconv_stream_bf16")
    return out


def ctc_collapse_stream(best, blank, prev, n_valid=None, offset=0):
    """best (B, T) int32 per-frame classes of one call, prev (B) int32 = the class before its first frame (-1 at stream start; updated in place) -> (ids (B, T) int32 =
    the newly emitted tokens then -1, n_ids (B) int32).  Frames t < n_valid[b] - offset count (all T without n_valid).  mi_ctc_collapse_stream."""
    _req(best, torch.int32); _req(prev, torch.int32)
    best = best.contiguous()
    B, T = best.shape
    ids = torch.empty((B, T), device=best.device, dtype=torch.int32)
    n = torch.empty((B,), device=best.device, dtype=torch.int32)
    if n_valid is not None:
        n_valid = _lengths_i32(n_valid, B, best.device)
    rc = _lib.lib().mi_ctc_collapse_stream(best.data_ptr(), B, T, _p(n_valid), int(offset), int(blank), prev.data_ptr(), ids.data_ptr(), n.data_ptr(), _stream())
    _lib.check(rc, "mi_ctc_collapse_stream")
    return ids, n


# ---------------------------------------------------------------------------------------------------- streaming session pool: the per-slot forms (csrc/stream_pool.hip)
def slot_table(entries, width, device):
    """entries: rows of `width` ints, one per active slot -> (host, device) int32 tensors of the same words: the C entries check the first and hand the second to the kernel"""
    host = torch.tensor(entries, dtype=torch.int32).reshape(-1, width).contiguous()
    return host, host.to(device)


NO_END = 0x7FFFFFFF          # a dwconv entry's `end` of a slot that does not finish


def copy_rows_slots(src, dst, entries, W=None):
    """rows between (slots, rows, width) tensors of 4-byte elements (fp32 / int32; last dim contiguous), `dst` written in place.  entries: per active slot (src slot, src
    row, src modulus, dst slot, dst row, dst modulus, rows); a modulus of 0 does not wrap.  W: elements of a row copied (default: the narrower width).  mi_copy_rows_slots."""
    _req(src); _req(dst)
    if src.element_size() != 4 or dst.element_size() != 4 or src.dim() != 3 or dst.dim() != 3 or src.stride(2) != 1 or dst.stride(2) != 1:
        raise ValueError("copy_rows_slots: (slots, rows, width) tensors of 4-byte elements, last dim contiguous")
    W = min(src.shape[2], dst.shape[2]) if W is None else int(W)
    th, td = slot_table(entries, 7, src.device)
    rc = _lib.lib().mi_copy_rows_slots(src.data_ptr(), src.stride(0), src.stride(1), src.shape[0], src.shape[1], dst.data_ptr(), dst.stride(0), dst.stride(1), dst.shape[0],
                                       dst.shape[1], th.data_ptr(), td.data_ptr(), th.shape[0], W, _stream())
    _lib.check(rc, "mi_copy_rows_slots")
    return dst


def attention_chunk_slots(q, k_cache, v_cache, entries, H, *, pos=None, bias_u=None, bias_v=None, scale=None, ref=0):
    """attention_chunk per slot: q (sum n_q, d) bf16 compact; k_cache / v_cache (slots, Lmax, d) row views of one cache; entries: per active slot (first query row, n_q,
    n_k, slot), the first rows the prefix sums of n_q.  -> (sum n_q, d) bf16.  mi_attention_chunk_slots_bf16."""
    _req(q, BF16); _req(k_cache, BF16); _req(v_cache, BF16)
    q = q.contiguous()
    n, d = q.shape
    if k_cache.stride() != v_cache.stride() or k_cache.stride(2) != 1:
        raise ValueError("attention_chunk_slots: k_cache and v_cache must be row views with equal strides")
    hd = d // H
    out = torch.empty((n, d), device=q.device, dtype=BF16)
    th, td = slot_table(entries, 4, q.device)
    rc = _lib.lib().mi_attention_chunk_slots_bf16(q.data_ptr(), d, k_cache.data_ptr(), k_cache.stride(1), v_cache.data_ptr(), v_cache.stride(1), k_cache.stride(0),
                                                  k_cache.shape[0], k_cache.shape[1], _p(pos), 0 if pos is None else pos.stride(0), _p(bias_u), _p(bias_v), out.data_ptr(), d,
                                                  th.data_ptr(), td.data_ptr(), th.shape[0], H, hd, float(scale if scale is not None else 1.0 / math.sqrt(hd)), int(ref), _stream())
    _lib.check(rc, "mi_attention_chunk_slots_bf16")
    return out


def dwconv_stream_slots(x, w, bias, ring, entries, n_out_total, *, mode, K, dil=1, left, ring_stats=None, stats=None, gamma=None, beta=None, mul=None, act=0):
    """dwconv_stream per slot: x (sum n_new, C) bf16 compact (last dim contiguous, any row stride); ring (slots, Hr, C) advanced in place; entries: per active slot (slot,
    first in row, first out row, p, n_new, o0, n_out, end or NO_END).  -> (n_out_total, C) bf16 compact.  mi_dwconv_stream_slots_bf16."""
    _req(x, BF16); _req(ring, BF16)
    Cc = x.shape[1]
    Hr = ring.shape[1]
    out = torch.empty((n_out_total, Cc), device=x.device, dtype=BF16)
    th, td = slot_table(entries, 8, x.device)
    rc = _lib.lib().mi_dwconv_stream_slots_bf16(x.data_ptr(), x.stride(0), _p(mul), 0 if mul is None else mul.stride(0), _p(stats), _p(gamma), _p(beta), w.data_ptr(), _p(bias),
                                                ring.data_ptr() if Hr else 0, _p(ring_stats), ring.shape[0], out.data_ptr(), Cc, th.data_ptr(), td.data_ptr(), th.shape[0],
                                                Cc, int(K), int(dil), int(left), Hr, DWCONV_STREAM_MODES[mode], int(act), _stream())
    _lib.check(rc, "mi_dwconv_stream_slots_bf16")
    return out


def rotary_slots(x, cos, sin, entries, H):
    """rotary with per-slot positions: x (rows, d) bf16 compact; cos / sin (tmax, hd) fp32; entries: per active slot (first row, rows, p): row i of the slot stands at
    position p + i.  -> (rows, d) bf16 (rows no entry names are not written).  mi_rotary_slots_bf16."""
    _req(x, BF16)
    M, d = x.shape
    out = torch.zeros_like(x)
    th, td = slot_table(entries, 3, x.device)
    rc = _lib.lib().mi_rotary_slots_bf16(x.data_ptr(), x.stride(0), out.data_ptr(), out.stride(0), cos.data_ptr(), sin.data_ptr(), cos.shape[0], th.data_ptr(), td.data_ptr(),
                                         th.shape[0], H, d // H, _stream())
    _lib.check(rc, "mi_rotary_slots_bf16")
    return out


def ctc_collapse_slots(best, blank, prev, entries):
    """ctc_collapse_stream per slot: best (frames) int32 compact; prev (slots) int32 the carried classes, updated in place; entries: per active slot (slot, first frame,
    frames).  -> (ids (frames) int32: an entry's new tokens then -1 in its places, n_ids (entries) int32).  mi_ctc_collapse_slots."""
    _req(best, torch.int32); _req(prev, torch.int32)
    best = best.contiguous()
    th, td = slot_table(entries, 3, best.device)
    if best.numel() == 0:
        raise ValueError("ctc_collapse_slots: no frames")
    ids = torch.full((best.numel(),), -1, device=best.device, dtype=torch.int32)
    n = torch.empty((th.shape[0],), device=best.device, dtype=torch.int32)
    rc = _lib.lib().mi_ctc_collapse_slots(best.data_ptr(), int(blank), prev.data_ptr(), prev.numel(), ids.data_ptr(), n.data_ptr(), th.data_ptr(), td.data_ptr(),
                                          th.shape[0], _stream())
    _lib.check(rc, "mi_ctc_collapse_slots")
    return ids, n
