"""CPU references, case table and dispatch restatement for the depthwise-conv kernels (csrc/conv.hip: dwconv_time_kernel, dwconv31_kernel, gate_act_mul_kernel,
row_stats_kernel; csrc/conv_bwd.hip: dwconv_bwd_kernel, dwconv31_bwd_kernel, dwconv_bwd_dilated_kernel, gate_act_mul_bwd_kernel).  Plain torch, written from the
definitions, no GPU and none of the kernels' tiling:

    conv(x)[b, t, c] = bias[c] + sum_k w[c, k] x[b, t - pad + k dil, c]           x = 0 outside 0 <= t < T of ITS OWN utterance
    CSGU    s = x_r * act(conv(LN(x_g)))         LN(x)[row] = (x - mean[row]) rstd[row] gamma + beta with the GIVEN (mean, rstd)       gated=False: conv(LN(x_g)) alone
    MERGE   y = m + conv(m)
    backward (identity activation)   dyc = ds x_r (gated) | ds (split) | dy (merge)
        dr = ds conv        dgn[u] = sum_k w[k] dyc[u + pad - k dil]        dm = dy + conv^T(dy)        dw[c, k] = sum_{b,t} dyc[t] x[t - pad + k dil]        db = sum dyc

Every function takes `dtype`: float64 is the reference, float32 is the same formula evaluated in the kernels' accumulation precision — the difference of the two is what
the real-valued GPU tests size their additive bound from (tests/test_gpu_dwconv.py).

Integer inputs (`int_inputs`): x_g, taps, bias, beta, ds, dy in {-1, 0, 1}, gamma in {-1, 1}, x_r and m in {-2..2}, stats (0, 1).  Then |LN(x_g)| <= 2, |conv| <= 31 * 2 + 1,
every output is an integer below 256 in magnitude (exact in bf16) and every partial sum an integer below 2**24 (exact in fp32 in ANY order): the device result must
EQUAL the reference, so an index that is off by one row or one channel cannot hide under a rounding bound."""
from collections import namedtuple

import torch

F64 = torch.float64
F32 = torch.float32
BF16 = torch.bfloat16


# ---------------------------------------------------------------------------------------------------------------- the convolution and its two transposes
def _pad_time(x, B, T, lo, hi):
    """(B*T, C) -> (B, lo + T + hi, C) with zeros around every utterance"""
    C = x.shape[1]
    xp = torch.zeros(B, lo + T + hi, C, dtype=x.dtype)
    xp[:, lo:lo + T] = x.reshape(B, T, C)
    return xp


def conv(x, w, bias, B, T, pad_left, dilation=1):
    """x (B*T, C), w (C, K), bias (C) or None -> (B*T, C)"""
    C, K = w.shape
    reach = (K - 1) * dilation
    xp = _pad_time(x, B, T, pad_left, max(reach - pad_left, 0))          # xp[:, t + k dil] = x[t - pad + k dil]
    y = torch.zeros(B, T, C, dtype=x.dtype)
    if bias is not None:
        y = y + bias
    for k in range(K):
        y = y + w[:, k] * xp[:, k * dilation:k * dilation + T]
    return y.reshape(B * T, C)


def conv_transpose(d, w, B, T, pad_left, dilation=1):
    """gradient of conv w.r.t. its input: out[u] = sum_k w[k] d[u + pad - k dil]   (0 <= pad <= (K - 1) dil)"""
    C, K = w.shape
    reach = (K - 1) * dilation
    dp = _pad_time(d, B, T, reach - pad_left, pad_left)                  # dp[:, u + (K - 1 - k) dil] = d[u + pad - k dil]
    out = torch.zeros(B, T, C, dtype=d.dtype)
    for k in range(K):
        o = (K - 1 - k) * dilation
        out = out + w[:, k] * dp[:, o:o + T]
    return out.reshape(B * T, C)


def conv_wgrad(d, x, K, B, T, pad_left, dilation=1):
    """dw (C, K) = sum_{b,t} d[t] x[t - pad + k dil],  db (C) = sum d;  also S (C, K) = sum |d| |x| and Sb (C) = sum |d|, the magnitudes an fp32 summation bound needs"""
    C = x.shape[1]
    reach = (K - 1) * dilation
    xp = _pad_time(x, B, T, pad_left, max(reach - pad_left, 0))
    dv = d.reshape(B, T, C)
    dw = torch.zeros(C, K, dtype=x.dtype)
    S = torch.zeros(C, K, dtype=x.dtype)
    for k in range(K):
        xs = xp[:, k * dilation:k * dilation + T]
        dw[:, k] = (dv * xs).sum(dim=(0, 1))
        S[:, k] = (dv.abs() * xs.abs()).sum(dim=(0, 1))
    return dw, dv.sum(dim=(0, 1)), S, dv.abs().sum(dim=(0, 1))


# ---------------------------------------------------------------------------------------------------------------- activations
_RSQRT2 = 0.7071067811865476
_RSQRT2PI = 0.3989422804014327


def act_fn(v, act):
    """0 identity, 1 erf-GELU, 2 ReLU, 3 SiLU"""
    if act == 0:
        return v
    if act == 1:
        return 0.5 * v * (1.0 + torch.erf(v * _RSQRT2))
    if act == 2:
        return torch.clamp(v, min=0.0)
    if act == 3:
        return v / (1.0 + torch.exp(-v))
    raise ValueError(act)


def act_grad(v, act):
    if act == 0:
        return torch.ones_like(v)
    if act == 1:
        return 0.5 * (1.0 + torch.erf(v * _RSQRT2)) + v * _RSQRT2PI * torch.exp(-0.5 * v * v)
    if act == 2:
        return (v > 0).to(v.dtype)
    if act == 3:
        s = 1.0 / (1.0 + torch.exp(-v))
        return s * (1.0 + v * (1.0 - s))
    raise ValueError(act)


# The kernels' forward GELU (gelu_erf, csrc/common.hpp) is not erff but a fit, x / (1 + 2**(xc (c1 + c3 xc^2 + c5 xc^4))) with xc = clamp(x, -10, 10), documented
# there as within 2.6e-5 ABSOLUTE of the erf form.  `gelu_fit` restates that formula in fp64 so that the figure can be checked without a GPU
# (tests/test_dwconv_ref_cpu.py); GELU_FIT_ERR |x_r| — the activation's specified tolerance — is what the real-valued GPU tests add to the bound of x_r * gelu(.).
GELU_FIT_ERR = 2.6e-5
_GELU_FIT_C = (-2.30112135, -1.06775756e-1, 1.01426783e-3)


def gelu_fit(x):
    x = x.to(F64)
    xc = x.clamp(-10.0, 10.0)
    x2 = xc * xc
    out = x / (1.0 + torch.exp2(xc * (_GELU_FIT_C[0] + x2 * (_GELU_FIT_C[1] + x2 * _GELU_FIT_C[2]))))
    return torch.where(x < -10.0, torch.zeros_like(x), out)


def gate_act_mul(r, g, act, dtype=F64):
    return r.to(dtype) * act_fn(g.to(dtype), act)


def gate_act_mul_bwd(r, g, ds, act, dtype=F64):
    """s = r act(g):  dr = ds act(g),  dg = ds r act'(g)"""
    r, g, ds = r.to(dtype), g.to(dtype), ds.to(dtype)
    return ds * act_fn(g, act), ds * r * act_grad(g, act)


# ---------------------------------------------------------------------------------------------------------------- row statistics / LayerNorm with given statistics
def row_stats(x, eps, dtype=F64):
    """(M, d) -> (M, 2) = (mean, 1 / sqrt(biased variance + eps)), two-pass"""
    x = x.to(dtype)
    mean = x.mean(dim=1)
    var = ((x - mean[:, None]) ** 2).mean(dim=1)
    return torch.stack([mean, 1.0 / torch.sqrt(var + eps)], dim=1)


def ln_given(x, stats, gamma, beta):
    return (x - stats[:, :1]) * stats[:, 1:2] * gamma + beta


# ---------------------------------------------------------------------------------------------------------------- CSGU / merge, forward and backward
def csgu_fwd(u, stats, gamma, beta, w, bias, B, T, pad_left, dilation, act, gated=True, dtype=F64, parts=False):
    """u (B*T, 2C) = [x_r | x_g] -> x_r * act(conv(LN(x_g)) + b);  gated=False: the conv alone (act must be 0).  parts: also the conv output"""
    u, stats, gamma, beta, w = [t.to(dtype) for t in (u, stats, gamma, beta, w)]
    bias = None if bias is None else bias.to(dtype)
    C = u.shape[1] // 2
    cv = conv(ln_given(u[:, C:], stats, gamma, beta), w, bias, B, T, pad_left, dilation)
    out = u[:, :C] * act_fn(cv, act) if gated else cv
    return (out, cv) if parts else out


def merge_fwd(m, w, bias, B, T, pad_left, dtype=F64):
    m, w = m.to(dtype), w.to(dtype)
    return m + conv(m, w, None if bias is None else bias.to(dtype), B, T, pad_left, 1)


def csgu_bwd(u, stats, gamma, beta, w, bias, ds, B, T, pad_left, dilation, gated=True, dtype=F64):
    """-> dict(dr (None for the split form), dgn, dw, db, conv, dyc, S, Sb)"""
    u, stats, gamma, beta, w, ds = [t.to(dtype) for t in (u, stats, gamma, beta, w, ds)]
    bias = None if bias is None else bias.to(dtype)
    C, K = w.shape
    gn = ln_given(u[:, C:], stats, gamma, beta)
    cv = conv(gn, w, bias, B, T, pad_left, dilation)
    dyc = ds * u[:, :C] if gated else ds
    dw, db, S, Sb = conv_wgrad(dyc, gn, K, B, T, pad_left, dilation)
    return dict(dr=ds * cv if gated else None, dgn=conv_transpose(dyc, w, B, T, pad_left, dilation), dw=dw, db=db, conv=cv, dyc=dyc, S=S, Sb=Sb)


def merge_bwd(m, w, dy, B, T, pad_left, dilation=1, dtype=F64):
    """-> dict(dm, dw, db, dyc, S, Sb)"""
    m, w, dy = m.to(dtype), w.to(dtype), dy.to(dtype)
    dw, db, S, Sb = conv_wgrad(dy, m, w.shape[1], B, T, pad_left, dilation)
    return dict(dm=dy + conv_transpose(dy, w, B, T, pad_left, dilation), dw=dw, db=db, dyc=dy, S=S, Sb=Sb)


# ---------------------------------------------------------------------------------------------------------------- the cases
# op: "csgu" (gated: mi_csgu_bf16 / csgu_bwd), "split" (mi_csgu_conv_bf16 / csgu_bwd(dr=None)), "merge" (mi_dwconv_residual_bf16 / dwconv_residual_bwd)
# view: how the conv input (u for the CSGU forms, m for merge) lies in memory — "contig"; "slice64" = buf[:, 64:64 + W] of a wider buffer (16-B aligned, ld != W);
#       "off4" = buf[:, 4:4 + W] (the pointer is 8-B aligned only)
Case = namedtuple("Case", "name op B T C K pad dil view")

GUARD_COLS = 8          # every device output is big[g:g + M, 8:8 + C] of a (g + M + g, C + 16) buffer: 16 B in front of the rows, ld = C + 16
VIEW_OFF = {"contig": 0, "slice64": 64, "off4": 4}
VIEW_EXTRA = {"contig": 0, "slice64": 128, "off4": 8}


def _c(name, op, B, T, C, K=31, pad=None, dil=1, view="contig"):
    return Case(name, op, B, T, C, K, (K - 1) // 2 if pad is None else pad, dil, view)


def _cases():
    out = []
    # ---- fast form: K 31, pad 15, dilation 1, C % 64 == 0, aligned; T around the 15-row halo, the 31-row window and the 64-row tile
    for T, B, C in [(1, 2, 64), (15, 3, 64), (16, 2, 128), (31, 2, 64), (63, 2, 192), (64, 1, 64), (65, 2, 128), (150, 3, 64)]:
        out.append(_c(f"fast-csgu-T{T}", "csgu", B, T, C))
    for T, B, C in [(1, 2, 128), (15, 2, 64), (16, 3, 64), (31, 2, 192), (63, 2, 64), (64, 2, 128), (65, 1, 64), (150, 2, 192)]:
        out.append(_c(f"fast-merge-T{T}", "merge", B, T, C))
    out.append(_c("fast-csgu-slice", "csgu", 2, 150, 128, view="slice64"))
    out.append(_c("fast-merge-slice", "merge", 2, 65, 64, view="slice64"))
    # ---- generic form, same K 31 / pad 15: a partial last channel block, a channel count that is no multiple of 8, an unaligned view, the split gate
    out.append(_c("gen31-csgu-C72", "csgu", 2, 65, 72))
    out.append(_c("gen31-csgu-C96", "csgu", 2, 150, 96))
    out.append(_c("gen31-csgu-C72-T1", "csgu", 2, 1, 72))
    out.append(_c("gen31-merge-C72", "merge", 2, 64, 72))
    out.append(_c("gen31-merge-C96", "merge", 1, 65, 96))
    out.append(_c("gen31-merge-C100", "merge", 2, 65, 100))
    out.append(_c("gen31-merge-C100-T15", "merge", 3, 15, 100))
    out.append(_c("gen31-csgu-off4", "csgu", 2, 65, 64, view="off4"))
    out.append(_c("gen31-merge-off4", "merge", 2, 150, 128, view="off4"))
    out.append(_c("gen31-split-C64-T65", "split", 2, 65, 64))             # everything the fast form wants except the gate operand
    out.append(_c("gen31-split-C72", "split", 2, 150, 72))
    out.append(_c("gen31-split-off4", "split", 1, 64, 64, view="off4"))
    out.append(_c("gen31-split-slice", "split", 2, 16, 128, view="slice64"))
    # ---- generic form because of K: centred pad, C 64 / 72, T below a tile, one tile, one row more, two tiles and two rows
    for K, T, op, B, C in [
            (1, 5, "csgu", 2, 64), (1, 64, "merge", 2, 64), (1, 65, "split", 2, 64), (1, 130, "csgu", 2, 72),
            (3, 5, "merge", 2, 72), (3, 64, "split", 1, 72), (3, 65, "csgu", 2, 64), (3, 130, "merge", 2, 64),
            (7, 5, "split", 2, 64), (7, 64, "csgu", 2, 72), (7, 65, "merge", 2, 72), (7, 130, "split", 2, 72),
            (15, 5, "csgu", 2, 64), (15, 64, "merge", 2, 64), (15, 65, "split", 2, 64), (15, 130, "csgu", 2, 72)]:
        out.append(_c(f"genK{K}-{op}-T{T}", op, B, T, C, K=K))
    # ---- generic form, non-centred pad at dilation 1 (the causal conv of a K = 3 model has dilation (K - 1) // 2 = 1)
    out.append(_c("causalK3-csgu", "csgu", 2, 65, 64, K=3, pad=2))
    out.append(_c("causalK3-split", "split", 2, 64, 72, K=3, pad=2))
    out.append(_c("causalK3-merge", "merge", 2, 65, 72, K=3, pad=2))
    out.append(_c("causalK15-merge", "merge", 2, 130, 64, K=15, pad=14))
    # ---- dilated form: the causal CSGU (dilation 15, left pad 450) and a small dilated one; T below one tap step, below the reach, above it
    out.append(_c("dil15-csgu-T20", "csgu", 2, 20, 64, pad=450, dil=15))
    out.append(_c("dil15-csgu-T100", "csgu", 1, 100, 96, pad=450, dil=15))
    out.append(_c("dil15-csgu-T520", "csgu", 2, 520, 64, pad=450, dil=15))
    out.append(_c("dil15-split-T20", "split", 1, 20, 96, pad=450, dil=15))
    out.append(_c("dil15-split-T100", "split", 2, 100, 64, pad=450, dil=15))
    out.append(_c("dil15-split-T520", "split", 2, 520, 96, pad=450, dil=15))
    out.append(_c("dil3-csgu-K7", "csgu", 2, 70, 72, K=7, pad=18, dil=3))
    out.append(_c("dil3-split-K7", "split", 2, 70, 72, K=7, pad=18, dil=3))
    return out


CASES = _cases()
CASE_BY_NAME = {c.name: c for c in CASES}
assert len(CASE_BY_NAME) == len(CASES)

# one case per (backward form x op) for the real-valued tests
REAL_CASES = ["fast-csgu-T150", "fast-merge-T65", "gen31-csgu-C72", "gen31-split-C64-T65", "gen31-merge-C100", "dil15-csgu-T520", "dil3-split-K7"]
# fused activations 1 (GELU) and 3 (SiLU) of mi_csgu_bf16, on the fast and on the generic forward
REAL_ACT_CASES = ["fast-csgu-T65", "gen31-csgu-C96"]


def layout(case):
    """element offsets and leading dimensions of the device buffers the GPU tests build: dict(W, off_in, ld_in, ld_out, off_out).  Allocations are at least 16-B aligned
    and the guard rows in front of a view are a whole number of 16-B units whenever ld % 8 == 0, so a view is 16-B aligned iff (column offset * 2 bytes) % 16 == 0."""
    W = case.C if case.op == "merge" else 2 * case.C
    return dict(W=W, off_in=VIEW_OFF[case.view], ld_in=W + VIEW_EXTRA[case.view], ld_out=case.C + 2 * GUARD_COLS, off_out=GUARD_COLS)


def _al16(off_elems):
    return (off_elems * 2) % 16 == 0


def forms(case):
    """(forward kernel, backward kernel) a case reaches: the predicates of dw_launch (conv.hip) and dw_bwd_launch (conv_bwd.hip) restated on the test's buffer layout.
    forward: "fast" (dwconv31_kernel) | "generic" (dwconv_time_kernel);   backward: "dilated" | "fast" (dwconv31_bwd_kernel) | "generic" (dwconv_bwd_kernel)"""
    lay = layout(case)
    csgu = case.op != "merge"
    gate = case.op == "csgu"                                   # the gate operand x_r (forward `mul`, backward `r` / `dr`) is present
    in_off = lay["off_in"] + (case.C if csgu else 0)           # the conv input of the CSGU forms is the second half of u
    shape_ok = case.K == 31 and case.pad == 15 and case.C % 64 == 0 and not (csgu and not gate)
    in_ok = lay["ld_in"] % 8 == 0 and _al16(in_off) and (not csgu or _al16(lay["off_in"]))      # x_g (and x_r: same ld) of u
    out_ok = lay["ld_out"] % 8 == 0 and _al16(lay["off_out"])                                      # every output / gradient buffer of the tests has this layout
    dy_ok = case.C % 8 == 0                                    # ds / dy is a contiguous (M, C) tensor
    fwd = "fast" if shape_ok and case.dil == 1 and in_ok and out_ok else "generic"
    if case.dil > 1:
        bwd = "dilated"
    else:
        bwd = "fast" if shape_ok and in_ok and out_ok and dy_ok else "generic"
    return fwd, bwd


def edges(case):
    """the edge conditions a case exercises, as tags"""
    e = {f"T={case.T}", f"K={case.K}", f"B={case.B}"}
    if case.view == "slice64":
        e.add("slice")
    if case.view == "off4":
        e.add("unaligned")
    if case.C % 64:
        e.add("partial-channel-block")
    if case.C % 8:
        e.add("C%8")
    if case.dil == 1 and case.pad != (case.K - 1) // 2:
        e.add("non-centred-pad")
    if case.dil > 1 and (case.K - 1) * case.dil >= case.T:
        e.add("dead-taps")                                      # taps whose reach exceeds T: they never meet data, their gradient is exactly zero
    return e


def dead_taps(case):
    """tap k multiplies x[t - pad + k dil]; with the causal pad (K - 1) dil that is x[t - (K - 1 - k) dil]: inside the utterance for some t < T iff (K - 1 - k) dil < T"""
    return [k for k in range(case.K) if case.pad - k * case.dil >= case.T or -case.pad + k * case.dil >= case.T]


# ---------------------------------------------------------------------------------------------------------------- inputs
def _gen(case, salt):
    return torch.Generator().manual_seed(1000 * CASES.index(case) + salt if case in CASES else salt)


def _ri(g, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=g).to(F64)


def int_inputs(case):
    """fp64 tensors holding small integers (see the module docstring).  CSGU forms: u, stats, gamma, beta, w, bias, ds;  merge: m, w, bias, dy"""
    g = _gen(case, 1)
    M, C, K = case.B * case.T, case.C, case.K
    w, bias = _ri(g, -1, 1, C, K), _ri(g, -1, 1, C)
    if case.op == "merge":
        return dict(m=_ri(g, -2, 2, M, C), w=w, bias=bias, dy=_ri(g, -1, 1, M, C))
    u = torch.cat([_ri(g, -2, 2, M, C), _ri(g, -1, 1, M, C)], dim=1)
    stats = torch.stack([torch.zeros(M, dtype=F64), torch.ones(M, dtype=F64)], dim=1)
    return dict(u=u, stats=stats, gamma=_ri(g, 0, 1, C) * 2 - 1, beta=_ri(g, -1, 1, C), w=w, bias=bias, ds=_ri(g, -1, 1, M, C))


def real_inputs(case, eps=1e-5):
    """random inputs as the device sees them, held in fp64: activations rounded to bf16, parameters and statistics rounded to fp32 (statistics computed in fp64 from
    the rounded activations, then cast: the kernel and the reference get the same fp32 numbers)"""
    g = _gen(case, 2)
    M, C, K = case.B * case.T, case.C, case.K

    def rn(*shape, scale=1.0):
        return torch.randn(*shape, generator=g) * scale

    def b16(x):
        return x.to(BF16).to(F64)

    w, bias = (rn(C, K, scale=0.2)).to(F64), (0.1 * rn(C)).to(F64)
    if case.op == "merge":
        return dict(m=b16(rn(M, C)), w=w, bias=bias, dy=b16(rn(M, C)))
    u = b16(rn(M, 2 * C))
    stats = row_stats(u[:, C:], float(torch.tensor(eps, dtype=F32))).to(F32).to(F64)
    return dict(u=u, stats=stats, gamma=(1 + 0.1 * rn(C)).to(F64), beta=(0.1 * rn(C)).to(F64), w=w, bias=bias, ds=b16(rn(M, C)))


def reference(case, inp, act=0, dtype=F64):
    """everything the kernels of a case produce: forward outputs `fwd` (csgu: dict act -> out; split / merge: the one output) and the backward dict"""
    B, T = case.B, case.T
    if case.op == "merge":
        return dict(fwd=merge_fwd(inp["m"], inp["w"], inp["bias"], B, T, case.pad, dtype=dtype), bwd=merge_bwd(inp["m"], inp["w"], inp["dy"], B, T, case.pad, dtype=dtype))
    a = (inp["u"], inp["stats"], inp["gamma"], inp["beta"], inp["w"], inp["bias"])
    gated = case.op == "csgu"
    return dict(fwd=csgu_fwd(*a, B, T, case.pad, case.dil, act if gated else 0, gated=gated, dtype=dtype),
                bwd=csgu_bwd(*a, inp["ds"], B, T, case.pad, case.dil, gated=gated, dtype=dtype))


def additive_bound(ref32, ref64):
    """the `a` of |got - want| <= 2**-8 |want| + a for a bf16 output: 16 x the largest difference between the SAME reference evaluated in fp32 and in fp64 (the kernel sums
    in fp32, in another order, with fast erff / __expf: 16 is the margin for those), and never below 2**-18 max|want| (four fp32 roundings of the largest value)"""
    return max(16.0 * float((ref32.to(F64) - ref64).abs().max()), 2.0 ** -18 * float(ref64.abs().max()))


def sum_bound(N, S):
    """worst-case error of ANY fp32 summation order of N products whose magnitudes add up to S: N 2**-24 S  (a single dropped term is ~ S / N)"""
    return N * 2.0 ** -24 * S
