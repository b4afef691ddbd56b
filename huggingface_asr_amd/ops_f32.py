"""Torch-tensor wrappers over the fp32 entries of the C ABI (csrc/gemm_f32.hip, csrc/encoder_f32.hip, csrc/decoder_f32.hip): the operators of the `precision="fp32"`
inference mode, one by one.  The engine calls the whole-encoder entry (mi_ebf_forward_f32); these exist for the operator tests and for callers who want
one exact-fp32 piece.  Every tensor is an fp32 device tensor with a contiguous last dimension; there is no CPU path.
"""
from __future__ import annotations

import math

import torch

from . import _lib
from .ops import _p, _req, _stream

F32 = torch.float32
ACT = {"identity": 0, "none": 0, "gelu": 1, "relu": 2, "silu": 3, "swish": 3}
SCORES_BOUND = 64 << 20          # MI_ATTENTION_F32_SCORES_BYTES (include/hfasr_hip.h)


def _rows(t):
    _req(t, F32)
    if t.dim() != 2 or t.stride(1) != 1:
        raise TypeError("expected a 2-D fp32 tensor with contiguous rows")
    return t


def gemm(a, w, bias=None, out=None, *, act="none", resid=None, alpha=1.0):
    """out (M,N) = resid + alpha * act(a (M,K) @ w (N,K)^T + bias) on the f32-input MFMA; act "none" | "gelu" (exact erf) | "gelu_new" (exact tanh); resid may be `out`
    itself."""
    _rows(a); _rows(w)
    M, K = a.shape
    N = w.shape[0]
    if w.shape[1] != K:
        raise ValueError("gemm: a (M,K) and w (N,K) disagree on K")
    if out is None:
        out = torch.empty((M, N), device=a.device, dtype=F32)
    _rows(out)
    rc = _lib.lib().mi_gemm_f32(a.data_ptr(), a.stride(0), w.data_ptr(), w.stride(0), _p(bias), out.data_ptr(), out.stride(0),
                                _p(resid), resid.stride(0) if resid is not None else 0, float(alpha), {"none": 0, "gelu": 1, "gelu_new": 2}[act], M, N, K, _stream())
    _lib.check(rc, "mi_gemm_f32")
    return out


def layernorm(x, gamma, beta, eps=1e-5, *, lengths=None, T=1, x_out=None):
    """LayerNorm over the last dimension of x (M,d); lengths (B) int32 with row = b*T + t: frames t >= lengths[b] are zeroed first (x_out receives the zeroed rows)."""
    _rows(x)
    M, d = x.shape
    y = torch.empty((M, d), device=x.device, dtype=F32)
    rc = _lib.lib().mi_layernorm_f32(x.data_ptr(), x.stride(0), _p(lengths), int(T), _p(x_out), x_out.stride(0) if x_out is not None else 0,
                                     gamma.data_ptr(), beta.data_ptr(), float(eps), y.data_ptr(), y.stride(0), M, d, _stream())
    _lib.check(rc, "mi_layernorm_f32")
    return y


def rotary(x, cos, sin, T, H):
    _rows(x)
    M, d = x.shape
    y = torch.empty((M, d), device=x.device, dtype=F32)
    rc = _lib.lib().mi_rotary_f32(x.data_ptr(), x.stride(0), y.data_ptr(), y.stride(0), cos.data_ptr(), sin.data_ptr(), M, int(T), int(H), d // H, _stream())
    _lib.check(rc, "mi_rotary_f32")
    return y


def dwconv(x, w, bias, B, T, *, pad_left=None, dilation=1, gate=None, act="identity", residual=False):
    """depthwise Conv1d over time on x (B*T, C), w (C, K): plain, gated (gate * act(conv), the CSGU) or with the input added (the merge)."""
    _rows(x)
    C, K = w.shape
    if pad_left is None:
        pad_left = (K - 1) // 2
    y = torch.empty((B * T, C), device=x.device, dtype=F32)
    mode = 1 if gate is not None else (2 if residual else 0)
    rc = _lib.lib().mi_dwconv_f32(x.data_ptr(), x.stride(0), w.data_ptr(), _p(bias), _p(gate), gate.stride(0) if gate is not None else 0, y.data_ptr(), y.stride(0),
                                  B, T, C, K, int(pad_left), int(dilation), ACT[act], mode, _stream())
    _lib.check(rc, "mi_dwconv_f32")
    return y


def gate_act_mul(r, g, act="identity"):
    _rows(r); _rows(g)
    M, N = g.shape
    s = torch.empty((M, N), device=r.device, dtype=F32)
    rc = _lib.lib().mi_gate_act_mul_f32(r.data_ptr(), r.stride(0), g.data_ptr(), g.stride(0), s.data_ptr(), s.stride(0), M, N, ACT[act], _stream())
    _lib.check(rc, "mi_gate_act_mul_f32")
    return s


def csgu(h, gamma, beta, w, bias, B, T, *, causal=False, act="identity", lin_w=None, lin_b=None, eps=1e-5):
    """the CSGU of the cgMLP (e_branchformer.py:144-203) on h (B*T, I) = [x_r | x_g]: x_r * act(linear?(dwconv(LayerNorm(x_g)))) -> (B*T, I/2).
    causal: the reference's dilation quirk — dilation (K-1)/2, left padding (K-1) * dilation."""
    _rows(h)
    I = h.shape[1]
    K = w.shape[1]
    dil = (K - 1) // 2 if causal else 1
    pad = (K - 1) * dil if causal else (K - 1) // 2
    gn = layernorm(h[:, I // 2:], gamma, beta, eps)
    if lin_w is None:
        return dwconv(gn, w, bias, B, T, pad_left=pad, dilation=dil, gate=h[:, :I // 2], act=act)
    cv = dwconv(gn, w, bias, B, T, pad_left=pad, dilation=dil)
    return gate_act_mul(h[:, :I // 2], gemm(cv, lin_w, lin_b), act)


def conv2d_first_gelu(x, w, bias, K=3, stride=2, pad=1, causal=False):
    """x (B,T,F) -> GELU(Conv2d(1 -> C)) as (B,T1,F1,C) channels-last; w (C, K*K).  causal: all of the 2*pad padding on the left / top (CausalConv2d)."""
    _req(x, F32)
    B, T, Fq = x.shape
    C = w.shape[0]
    T1, F1 = (T + 2 * pad - K) // stride + 1, (Fq + 2 * pad - K) // stride + 1
    pl = 2 * pad if causal else pad
    out = torch.empty((B, T1, F1, C), device=x.device, dtype=F32)
    rc = _lib.lib().mi_conv2d_first_gelu_f32(x.contiguous().data_ptr(), w.data_ptr(), bias.data_ptr(), out.data_ptr(), B, T, Fq, C, K, stride, pl, pl, T1, F1, _stream())
    _lib.check(rc, "mi_conv2d_first_gelu_f32")
    return out


def conv2d_cl(x, w, bias, K=3, stride=2, pad=1, causal=False, act="gelu"):
    """x (B,T1,F1,Cin) channels-last -> (B,T2,F2,Cout); w (Cout, K*K*Cin) in (kh, kw, cin) order.  Implicit GEMM: no im2col buffer."""
    _req(x, F32)
    B, T1, F1, Cin = x.shape
    Cout = w.shape[0]
    T2, F2 = (T1 + 2 * pad - K) // stride + 1, (F1 + 2 * pad - K) // stride + 1
    pl = 2 * pad if causal else pad
    out = torch.empty((B, T2, F2, Cout), device=x.device, dtype=F32)
    rc = _lib.lib().mi_conv2d_cl_f32(x.contiguous().data_ptr(), w.data_ptr(), _p(bias), out.data_ptr(), B, T1, F1, Cin, Cout, K, stride, pl, pl, T2, F2,
                                     {"none": 0, "gelu": 1}[act], _stream())
    _lib.check(rc, "mi_conv2d_cl_f32")
    return out


def attention_workspace_bytes(B, T, H, hd, relative):
    return int(_lib.lib().mi_attention_f32_workspace_bytes(B, T, H, hd, int(bool(relative))))


def attention(q, k, v, B, T, H, *, pos=None, bias_u=None, bias_v=None, lengths=None, causal=False, workspace_bytes=None):
    """q, k, v (B*T, d) row views -> ctx (B*T, d): fp32 scores, softmax and P.V.  pos (2T-1, d) projected relative positions with bias_u / bias_v (d), or none of
    the three.  workspace_bytes: size of the scores workspace (default: mi_attention_f32_workspace_bytes, at most SCORES_BOUND) — a smaller one walks more chunks."""
    _rows(q); _rows(k); _rows(v)
    d = q.shape[1]
    hd = d // H
    nbytes = attention_workspace_bytes(B, T, H, hd, pos is not None) if workspace_bytes is None else int(workspace_bytes)
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=q.device)
    out = torch.empty((B * T, d), device=q.device, dtype=F32)
    rc = _lib.lib().mi_attention_f32(q.data_ptr(), q.stride(0), k.data_ptr(), k.stride(0), v.data_ptr(), v.stride(0), _p(pos), pos.stride(0) if pos is not None else 0,
                                     _p(bias_u), _p(bias_v), _p(lengths), out.data_ptr(), out.stride(0), B, T, H, hd, 1.0 / math.sqrt(hd), int(bool(causal)),
                                     ws.data_ptr(), nbytes, _stream())
    _lib.check(rc, "mi_attention_f32")
    return out


def linear_rows_workspace_bytes(M, N, K):
    return int(_lib.lib().mi_linear_rows_f32_workspace_bytes(M, N, K))


def linear_rows(x, w, bias=None, out=None, *, act="none", accumulate=False, kcache=None, vcache=None, U=1, past=0):
    """out (M,N) = act(x (M,K) @ w (N,K)^T + bias), or out += that (`accumulate`: the residual stream), for 1 <= M <= 64 rows with the weights streamed once
    (mi_linear_rows_f32); act "none" | "gelu_new".  kcache / vcache (B, Lmax, N/3) fp32: columns [N/3, N) of row b*U + u are also appended at row past + u."""
    _rows(x); _rows(w)
    M, K = x.shape
    N = w.shape[0]
    if w.shape[1] != K:
        raise ValueError("linear_rows: x (M,K) and w (N,K) disagree on K")
    if out is None:
        if accumulate:
            raise ValueError("linear_rows: accumulate needs `out`")
        out = torch.empty((M, N), device=x.device, dtype=F32)
    _rows(out)
    nbytes = linear_rows_workspace_bytes(M, N, K)
    ws = torch.empty((max(nbytes, 4),), dtype=torch.uint8, device=x.device)
    Lmax, dkv = (kcache.shape[1], kcache.shape[2]) if kcache is not None else (0, 0)
    rc = _lib.lib().mi_linear_rows_f32(x.data_ptr(), x.stride(0), w.data_ptr(), w.stride(0), _p(bias), {"none": 0, "gelu_new": 2}[act], out.data_ptr(), out.stride(0),
                                       int(bool(accumulate)), _p(kcache), _p(vcache), int(U), int(past), Lmax, dkv, M, N, K, ws.data_ptr(), nbytes, _stream())
    _lib.check(rc, "mi_linear_rows_f32")
    return out


def attention_general(q, k, v, B, Tq, Tk, H, *, lengths=None, causal=False, out=None, kv_bstride=0, beams=1):
    """`ops.attention_general` in fp32: q (B*Tq, .) / k, v row views with head h at columns [h*hd, (h+1)*hd) -> context (B*Tq, d) fp32.  Cross-attention (`lengths` =
    valid keys) and KV-cache steps (causal offset Tk - Tq, `kv_bstride` floats between the batches of a cache).  `beams`: the B batches are B / beams utterances whose
    hypotheses read ONE K / V table (and one `lengths` entry) each."""
    _rows(q); _rows(k); _rows(v)
    d = q.shape[1]
    hd = d // H
    if out is None:
        out = torch.empty((B * Tq, d), device=q.device, dtype=F32)
    rc = _lib.lib().mi_attention_general_f32(q.data_ptr(), q.stride(0), k.data_ptr(), k.stride(0), v.data_ptr(), v.stride(0), _p(lengths), out.data_ptr(), out.stride(0),
                                             B, int(beams), Tq, Tk, int(kv_bstride), H, hd, 1.0 / math.sqrt(hd), int(bool(causal)), _stream())
    _lib.check(rc, "mi_attention_general_f32")
    return out
