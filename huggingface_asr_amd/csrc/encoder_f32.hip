// precision = "fp32": the E-Branchformer encoder + CTC head with NO value rounded to bf16 between the input features and the logits.
// What the reference's decode recipes compute (they carry no --bf16), and the mode in which SURVEY.md §7's first acceptance tier — fp32 kernels against the
// fp32 oracle, max |dlogit| <= 1e-3 — is tested.  Opt-in (engine.py `precision="fp32"`); the bf16 path (encoder.hip) is untouched by anything here.
//
// This file: the fp32 forms of the non-GEMM operators (LayerNorm, rotary, depthwise convs / CSGU, conv #1), the attention with materialised fp32 scores,
// and the whole-encoder driver mi_ebf_forward_f32.  Every dense contraction — the Linears, the attention's three products, conv #2 as an implicit GEMM —
// is gemm_f32.hip's kernel on the f32-input matrix instruction.  None of it is tuned beyond "MFMA, LDS-tiled, no scratch": this mode is for agreement, not speed.
//
// Data layout in HBM (all fp32, row-major, rows = b*T2 + t): x residual stream, a0/a1/a2 LayerNorm outputs, h (M, I), qkv (M, 3d) = [Q | K | V], ctx, cat (M, 2d),
// act1 (B,T1,F1,C1) / act2 (B,T2,F2,C2) channels-last conv activations.
#include "common.hpp"
#include "gemm_f32.hpp"
#include "ebf_layout.hpp"

namespace {

// ------------------------------------------------------------------------------------------------ element-wise / row kernels
__device__ __forceinline__ float gelu_exact(float v) { return 0.5f * v * (1.0f + erff(v * 0.70710678118654752440f)); }
__device__ __forceinline__ float act_f32(float v, int act) {      // engine.py ACT: 0 identity, 1 gelu, 2 relu, 3 silu
    if (act == 1) return gelu_exact(v);
    if (act == 2) return v > 0.f ? v : 0.f;
    if (act == 3) return v / (1.0f + expf(-v));
    return v;
}

// LayerNorm, one wave per row, two passes for the statistics (mean, then the variance around it), all fp32.  mask_len: rows at t >= mask_len[b] are ZEROED first
// (tf:662-665) — their LayerNorm is beta — and xo (nullable, may alias x) receives the masked rows.
__global__ __launch_bounds__(256) void layernorm_f32_kernel(const float* x, long ldx, const int* __restrict__ mask_len, int T, float* xo, long ldxo,
                                                            const float* __restrict__ g, const float* __restrict__ b, float eps, float* y, long ldy, int M, int d) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    const float* xr = x + row * ldx;
    float* yr = y + row * ldy;
    if (mask_len && (int)(row % T) >= mask_len[row / T]) {
        for (int c = lane; c < d; c += 64) {
            if (xo) xo[row * ldxo + c] = 0.f;
            yr[c] = b[c];
        }
        return;
    }
    float s = 0.f;
    for (int c = lane; c < d; c += 64) s += xr[c];
    const float mean = wave_sum(s) / (float)d;
    float q = 0.f;
    for (int c = lane; c < d; c += 64) { const float t = xr[c] - mean; q = fmaf(t, t, q); }
    const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)d + eps);
    const bool copy = xo && xo + row * ldxo != xr;
    for (int c = lane; c < d; c += 64) {
        const float v = xr[c];
        if (copy) xo[row * ldxo + c] = v;
        yr[c] = (v - mean) * rstd * g[c] + b[c];
    }
}

// rotary embedding of the Q / K projections' INPUT, per head (tf:509-526): y = x cos + rotate_half(x) sin
__global__ void rotary_f32_kernel(const float* __restrict__ x, long ldx, float* __restrict__ y, long ldy, const float* __restrict__ cs, const float* __restrict__ sn,
                                  long total, int T, int d, int hd) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const long m = idx / d;
    const int c = (int)(idx - m * d), i = c % hd, t = (int)(m % T), half = hd / 2;
    const float v = x[m * ldx + c];
    const float r = i < half ? -x[m * ldx + c + half] : x[m * ldx + c - half];
    y[m * ldy + c] = v * cs[(long)t * hd + i] + r * sn[(long)t * hd + i];
}

// depthwise Conv1d over time on (B, T, C) rows: v[t, c] = bias[c] + sum_k w[c, k] x[t - pad + k * dil, c], zero outside [0, T), taps added in k order.
// mode 0: y = v;  1: y = gate * act(v) (the CSGU gate, e_branchformer.py:196-203);  2: y = x + v (the merge's residual, :297-299).
// A thread owns one channel and TT consecutive frames (the channel is the coalesced axis).
constexpr int DW_TT = 8;
__global__ __launch_bounds__(256) void dwconv_f32_kernel(const float* __restrict__ x, long ldx, const float* __restrict__ w, const float* __restrict__ bias,
                                                         const float* __restrict__ gate, long ldg, float* __restrict__ y, long ldy,
                                                         int T, int C, int K, int pad, int dil, int act, int mode) {
    const int c = blockIdx.y * 256 + threadIdx.x;
    if (c >= C) return;
    const int tblocks = (T + DW_TT - 1) / DW_TT;
    const int b = blockIdx.x / tblocks, t0 = (blockIdx.x - b * tblocks) * DW_TT;
    const float* xb = x + (long)b * T * ldx + c;
    const float* wc = w + (long)c * K;
    float acc[DW_TT];
    const float bv = bias ? bias[c] : 0.f;
#pragma unroll
    for (int j = 0; j < DW_TT; ++j) acc[j] = bv;
    if (dil == 1) {
        // sliding window: input frame t0 - pad + i feeds tap i - j of output j.  wr[j] = w[i - j]: one weight and one input load per step; taps outside [0, K) are
        // skipped, not multiplied by zero, so an output sums exactly its own K taps in k order (a non-finite frame reaches only the outputs whose window holds it)
        float wr[DW_TT];
#pragma unroll
        for (int j = 0; j < DW_TT; ++j) wr[j] = 0.f;
        for (int i = 0; i < K + DW_TT - 1; ++i) {
#pragma unroll
            for (int j = DW_TT - 1; j > 0; --j) wr[j] = wr[j - 1];
            wr[0] = i < K ? wc[i] : 0.f;
            const int t = t0 - pad + i;
            const float v = (t >= 0 && t < T) ? xb[(long)t * ldx] : 0.f;
#pragma unroll
            for (int j = 0; j < DW_TT; ++j) acc[j] = (i - j >= 0 && i - j < K) ? fmaf(wr[j], v, acc[j]) : acc[j];
        }
    } else {
        for (int k = 0; k < K; ++k) {
            const float wk = wc[k];
#pragma unroll
            for (int j = 0; j < DW_TT; ++j) {
                const int t = t0 + j - pad + k * dil;
                const float v = (t >= 0 && t < T) ? xb[(long)t * ldx] : 0.f;
                acc[j] = fmaf(wk, v, acc[j]);
            }
        }
    }
#pragma unroll
    for (int j = 0; j < DW_TT; ++j) {
        const int t = t0 + j;
        if (t >= T) break;
        const long row = (long)b * T + t;
        float v = acc[j];
        if (mode == 1) v = gate[row * ldg + c] * act_f32(v, act);
        else if (mode == 2) v = xb[(long)t * ldx] + v;
        y[row * ldy + c] = v;
    }
}

// s = r * act(g)   (csgu_use_linear_after_conv: the gate after the extra Linear)
__global__ void gate_act_mul_f32_kernel(const float* __restrict__ r, long ldr, const float* __restrict__ g, long ldg, float* __restrict__ s, long lds_, long total, int N, int act) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const long m = idx / N;
    const int c = (int)(idx - m * N);
    s[m * lds_ + c] = r[m * ldr + c] * act_f32(g[m * ldg + c], act);
}

// Conv2d #1 (1 -> C, K x K) + GELU over the (B, T, F) fp32 features -> channels-last (B, T1, F1, C) fp32 (extractors.py:71-96 layer 0, :111)
__global__ void conv2d_first_f32_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias, float* __restrict__ out,
                                        long total, int T, int F, int C, int K, int stride, int pt, int pf, int T1, int F1) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const int c = (int)(idx % C);
    long r = idx / C;
    const int f1 = (int)(r % F1); r /= F1;
    const int t1 = (int)(r % T1);
    const long b = r / T1;
    float acc = bias[c];
    for (int kh = 0; kh < K; ++kh) {
        const int t = t1 * stride - pt + kh;
        if (t < 0 || t >= T) continue;
        for (int kw = 0; kw < K; ++kw) {
            const int f = f1 * stride - pf + kw;
            if (f < 0 || f >= F) continue;
            acc = fmaf(w[(long)c * K * K + kh * K + kw], x[(b * T + t) * F + f], acc);
        }
    }
    out[idx] = gelu_exact(acc);
}

// ------------------------------------------------------------------------------------------------ attention
// (q + pos_bias_u), (q + pos_bias_v) of a chunk of query rows: out (nb, rows, d) each
__global__ void add_uv_f32_kernel(const float* __restrict__ q, long ldq, const float* __restrict__ u, const float* __restrict__ v, float* __restrict__ qu, float* __restrict__ qv,
                                  long total, int rows, int d, int T, int b0, int i0) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const long r = idx / d;
    const int c = (int)(idx - r * d), bl = (int)(r / rows), il = (int)(r - (long)bl * rows);
    const float x = q[((long)(b0 + bl) * T + i0 + il) * ldq + c];
    qu[idx] = x + u[c];
    qv[idx] = x + v[c];
}

// One wave per query row: score[j] = (ac[j] + bd[T-1-i+j]) * scale over the keys j < len (and j <= i when causal), softmax in fp32, probabilities written over ac;
// a key outside that set gets EXACTLY 0 (the reference adds finfo.min, which absorbs any finite score; exp(min - max) = 0).  A row with no key at all is uniform over
// all T keys, as the reference's all-equal row is.  bd (nullable): the un-shifted (q + v) p^T product, row stride ldb; the shift is the index map of SURVEY §7.
__global__ __launch_bounds__(256) void rel_softmax_f32_kernel(float* __restrict__ ac, long lda, const float* __restrict__ bd, long ldb, const int* __restrict__ lens,
                                                              int nrows_total, int rows, int H, int T, int b0, int i0, float scale, int causal) {
    const int lane = threadIdx.x & 63;
    const long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);          // ((bl * H + h) * rows + il)
    if (r >= nrows_total) return;
    const int il = (int)(r % rows), bl = (int)(r / ((long)rows * H));
    const int i = i0 + il;
    float* a = ac + r * lda;
    const float* p = bd ? bd + r * ldb + (T - 1 - i) : nullptr;
    int n = lens ? lens[b0 + bl] : T;
    n = n < 0 ? 0 : (n > T ? T : n);
    if (causal && n > i + 1) n = i + 1;
    if (n == 0) {
        const float uni = 1.0f / (float)T;
        for (int j = lane; j < T; j += 64) a[j] = uni;
        return;
    }
    float mx = -INFINITY;
    for (int j = lane; j < n; j += 64) {
        const float s = (a[j] + (p ? p[j] : 0.f)) * scale;
        a[j] = s;
        mx = fmaxf(mx, s);
    }
    mx = wave_max(mx);
    float sum = 0.f;
    for (int j = lane; j < n; j += 64) {
        const float e = expf(a[j] - mx);
        a[j] = e;
        sum += e;
    }
    sum = wave_sum(sum);
    for (int j = lane; j < T; j += 64) a[j] = j < n ? a[j] / sum : 0.f;
}

// ------------------------------------------------------------------------------------------------ launch helpers
inline unsigned grid1(long total) { return (unsigned)((total + 255) / 256); }

int gemm(const float* A, long lda, const float* W, long ldw, const float* bias, float* C, long ldc, const float* resid, long ldr, float alpha, int act,
         int M, int N, int K, hipStream_t st) {
    GemmF32Args a{};
    a.A = A; a.lda = lda; a.W = W; a.ldw = ldw; a.bias = bias; a.resid = resid; a.ldr = ldr; a.C = C; a.ldc = ldc;
    a.alpha = alpha; a.act = act; a.M = M; a.N = N; a.K = K; a.nz = 1; a.nh = 1;
    return gemm_f32_launch(a, st);
}

inline long pad4(long n) { return (n + 3) / 4 * 4; }
// floats of attention workspace per query row: (q+u | q+v) rows, and per head a score row and an un-shifted position row (both padded to 16 bytes)
inline long attn_row_floats(int T, int H, int hd, int rel) { return rel ? 2L * H * hd + (long)H * (pad4(T) + pad4(2L * T - 1)) : (long)H * pad4(T); }

}  // namespace

// ================================================================================================ C entries
extern "C" int mi_layernorm_f32(const float* x, long ldx, const int* lengths, int T, float* x_out, long ldxo, const float* gamma, const float* beta, float eps,
                                float* y, long ldy, int M, int d, hipStream_t st) {
    MI_ENTER();
    if (!x || !gamma || !beta || !y || M <= 0 || d <= 0 || T <= 0) return MI_ERR_ARG;
    hipLaunchKernelGGL(layernorm_f32_kernel, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, st, x, ldx, lengths, T, x_out, ldxo, gamma, beta, eps, y, ldy, M, d);
    MI_CHECK_LAUNCH();
    return MI_OK;
}

extern "C" int mi_rotary_f32(const float* x, long ldx, float* y, long ldy, const float* cos_t, const float* sin_t, int M, int T, int H, int hd, hipStream_t st) {
    MI_ENTER();
    if (!x || !y || !cos_t || !sin_t || M <= 0 || T <= 0 || H <= 0 || hd <= 0 || (hd & 1)) return MI_ERR_ARG;
    const long total = (long)M * H * hd;
    hipLaunchKernelGGL(rotary_f32_kernel, dim3(grid1(total)), dim3(256), 0, st, x, ldx, y, ldy, cos_t, sin_t, total, T, H * hd, hd);
    MI_CHECK_LAUNCH();
    return MI_OK;
}

extern "C" int mi_dwconv_f32(const float* x, long ldx, const float* w, const float* bias, const float* gate, long ldg, float* y, long ldy,
                             int B, int T, int C, int K, int pad_left, int dilation, int act, int mode, hipStream_t st) {
    MI_ENTER();
    if (!x || !w || !y || B <= 0 || T <= 0 || C <= 0 || K <= 0 || pad_left < 0 || dilation < 1 || mode < 0 || mode > 2 || act < 0 || act > 3 || (mode == 1 && !gate)) return MI_ERR_ARG;
    const long gx = (long)B * ((T + DW_TT - 1) / DW_TT);
    if (gx > 0x7fffffffL || (C + 255) / 256 > 65535) return MI_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(dwconv_f32_kernel, dim3((unsigned)gx, (unsigned)((C + 255) / 256)), dim3(256), 0, st, x, ldx, w, bias, gate, ldg, y, ldy, T, C, K, pad_left, dilation, act, mode);
    MI_CHECK_LAUNCH();
    return MI_OK;
}

extern "C" int mi_gate_act_mul_f32(const float* r, long ldr, const float* g, long ldg, float* s, long lds_, int M, int N, int act, hipStream_t st) {
    MI_ENTER();
    if (!r || !g || !s || M <= 0 || N <= 0 || act < 0 || act > 3) return MI_ERR_ARG;
    hipLaunchKernelGGL(gate_act_mul_f32_kernel, dim3(grid1((long)M * N)), dim3(256), 0, st, r, ldr, g, ldg, s, lds_, (long)M * N, N, act);
    MI_CHECK_LAUNCH();
    return MI_OK;
}

extern "C" int mi_conv2d_first_gelu_f32(const float* x, const float* w, const float* bias, float* out_cl, int B, int T, int F, int C, int K, int stride,
                                        int pad_t, int pad_f, int T1, int F1, hipStream_t st) {
    MI_ENTER();
    if (!x || !w || !bias || !out_cl || B <= 0 || T <= 0 || F <= 0 || C <= 0 || K <= 0 || stride <= 0 || T1 <= 0 || F1 <= 0) return MI_ERR_ARG;
    const long total = (long)B * T1 * F1 * C;
    hipLaunchKernelGGL(conv2d_first_f32_kernel, dim3(grid1(total)), dim3(256), 0, st, x, w, bias, out_cl, total, T, F, C, K, stride, pad_t, pad_f, T1, F1);
    MI_CHECK_LAUNCH();
    return MI_OK;
}

// Conv2d over a channels-last fp32 activation as an implicit GEMM: rows (b, t2, f2), K = (kh, kw, cin) gathered inside the GEMM's A load — no im2col buffer.
extern "C" int mi_conv2d_cl_f32(const float* in, const float* weight, const float* bias, float* out, int B, int Tin, int Fin, int Cin, int Cout, int K, int stride,
                                int pad_t, int pad_f, int Tout, int Fout, int act, hipStream_t st) {
    MI_ENTER();
    if (!in || !weight || !out || B <= 0 || Tin <= 0 || Fin <= 0 || Cin <= 0 || Cout <= 0 || K <= 0 || stride <= 0 || Tout <= 0 || Fout <= 0) return MI_ERR_ARG;
    const long M = (long)B * Tout * Fout;
    if (M > 0x7fffffffL || (long)K * K * Cin > 0x7fffffffL) return MI_ERR_UNSUPPORTED;
    GemmF32Args a{};
    a.A = in; a.W = weight; a.ldw = (long)K * K * Cin; a.bias = bias; a.C = out; a.ldc = Cout; a.alpha = 1.f; a.act = act;
    a.M = (int)M; a.N = Cout; a.K = K * K * Cin; a.nz = 1; a.nh = 1;
    a.conv = 1; a.T1 = Tin; a.F1 = Fin; a.C1 = Cin; a.KW = K; a.stride = stride; a.pt = pad_t; a.pf = pad_f; a.T2 = Tout; a.F2 = Fout;
    const int rc = gemm_f32_launch(a, st);
    if (rc != MI_OK) return rc;
    MI_CHECK_LAUNCH();
    return MI_OK;
}

// The scores of the fp32 attention live in workspace; it is walked in chunks of utterances (and, when one utterance alone is too large, of query rows) so that the
// workspace never exceeds MI_ATTENTION_F32_SCORES_BYTES, whatever B and T are.
extern "C" size_t mi_attention_f32_workspace_bytes(int B, int T, int H, int hd, int relative) {
    if (B <= 0 || T <= 0 || H <= 0 || hd <= 0) return 0;
    const size_t row = (size_t)attn_row_floats(T, H, hd, relative) * sizeof(float);
    const size_t all = row * (size_t)B * (size_t)T;
    const size_t cap = (size_t)MI_ATTENTION_F32_SCORES_BYTES;
    return all < cap ? all : (row > cap ? row : cap);
}

// ctx[b, i, h, :] = softmax_j(((q_i + u) . k_j + (q_i + v) . p[T-1-i+j]) * scale) v_j  — e_branchformer.py:74-141 / tf:528-565 with fp32 scores, softmax and P·V.
// q / k / v / out: (B*T, >= H*hd) fp32 row views, head h at columns [h*hd, (h+1)*hd).  posp (T'=T: (2T-1, H*hd) rows, row stride ldp) with u, v (H*hd), or all three
// null (rotary / no positions).  lengths (B) int32 or null.  workspace: >= one query row of mi_attention_f32_workspace_bytes' layout; more = fewer, larger chunks.
extern "C" int mi_attention_f32(const float* q, long ldq, const float* k, long ldk, const float* v, long ldv, const float* posp, long ldp, const float* bias_u,
                                const float* bias_v, const int* lengths, float* out, long ldo, int B, int T, int H, int hd, float scale, int causal,
                                void* workspace, size_t workspace_bytes, hipStream_t st) {
    MI_ENTER();
    if (!q || !k || !v || !out || !workspace || B <= 0 || T <= 0 || H <= 0 || hd <= 0) return MI_ERR_ARG;
    const int rel = posp != nullptr;
    if (rel != (bias_u != nullptr) || rel != (bias_v != nullptr)) return MI_ERR_ARG;
    const int d = H * hd;
    const long rowf = attn_row_floats(T, H, hd, rel);
    const long fit = (long)(workspace_bytes / sizeof(float)) / rowf;          // query rows (over all heads) the workspace holds
    if (fit < 1) return MI_ERR_ARG;
    int nb = 1, rows = T;
    if (fit >= T) { const long n = fit / T; nb = (int)(n < B ? n : B); } else rows = (int)fit;
    if ((long)nb * H > 65535) nb = 65535 / H;
    if (nb < 1) return MI_ERR_UNSUPPORTED;
    const long Ta = pad4(T), Pa = pad4(2L * T - 1), P = 2L * T - 1;
    float* ws = (float*)workspace;
    for (int b0 = 0; b0 < B; b0 += nb) {
        const int cb = B - b0 < nb ? B - b0 : nb;
        for (int i0 = 0; i0 < T; i0 += rows) {
            const int cr = T - i0 < rows ? T - i0 : rows;
            const long nq = (long)cb * cr;                        // query rows of this chunk
            float* qu = ws;                                       // (cb, cr, d)   relative only
            float* qv = qu + (rel ? nq * d : 0);
            float* ac = qv + (rel ? nq * d : 0);                  // (cb, H, cr, Ta): scores, then probabilities
            float* bd = ac + nq * H * Ta;                         // (cb, H, cr, Pa)   relative only
            GemmF32Args g{};
            g.alpha = 1.f; g.nz = cb * H; g.nh = H; g.M = cr; g.K = hd;
            g.W = k + (long)b0 * T * ldk; g.ldw = ldk; g.sWb = (long)T * ldk; g.sWh = hd;
            g.C = ac; g.ldc = Ta; g.sCb = (long)H * cr * Ta; g.sCh = (long)cr * Ta; g.N = T;
            if (rel) {
                const long total = nq * d;
                hipLaunchKernelGGL(add_uv_f32_kernel, dim3(grid1(total)), dim3(256), 0, st, q, ldq, bias_u, bias_v, qu, qv, total, cr, d, T, b0, i0);
                g.A = qu; g.lda = d; g.sAb = (long)cr * d; g.sAh = hd;
            } else {
                g.A = q + ((long)b0 * T + i0) * ldq; g.lda = ldq; g.sAb = (long)T * ldq; g.sAh = hd;
            }
            int rc = gemm_f32_launch(g, st);                      // ac = (q + u) k^T
            if (rc != MI_OK) return rc;
            if (rel) {
                g.A = qv;
                g.W = posp; g.ldw = ldp; g.sWb = 0; g.sWh = hd; g.N = (int)P;
                g.C = bd; g.ldc = Pa; g.sCb = (long)H * cr * Pa; g.sCh = (long)cr * Pa;
                rc = gemm_f32_launch(g, st);                      // bd = (q + v) p^T, un-shifted
                if (rc != MI_OK) return rc;
            }
            const long nrows = nq * H;
            hipLaunchKernelGGL(rel_softmax_f32_kernel, dim3((unsigned)((nrows + 3) / 4)), dim3(256), 0, st, ac, Ta, rel ? bd : nullptr, Pa, lengths,
                               (int)nrows, cr, H, T, b0, i0, scale, causal);
            GemmF32Args p{};                                      // ctx = P · V
            p.alpha = 1.f; p.nz = cb * H; p.nh = H; p.M = cr; p.N = hd; p.K = T;
            p.A = ac; p.lda = Ta; p.sAb = (long)H * cr * Ta; p.sAh = (long)cr * Ta;
            p.W = v + (long)b0 * T * ldv; p.ldw = ldv; p.sWb = (long)T * ldv; p.sWh = hd; p.w_kn = 1;
            p.C = out + ((long)b0 * T + i0) * ldo; p.ldc = ldo; p.sCb = (long)T * ldo; p.sCh = hd;
            rc = gemm_f32_launch(p, st);
            if (rc != MI_OK) return rc;
        }
    }
    MI_CHECK_LAUNCH();
    return MI_OK;
}

// ================================================================================================ whole-encoder driver
// Slot order and geometry: ebf_layout.hpp, shared with the bf16 driver; this mode reads the un-folded slots, all of them fp32.
namespace {

struct Ws {
    float *act1, *act2, *feo, *x, *a0, *a1, *a2, *a1r, *h, *qkv, *ctx, *cat, *m2, *gn, *s, *cv, *lin, *hid;
    int* lens;
    void* attn; size_t attn_bytes;
    size_t bytes;
};
Ws carve(const mi_ebf_config& c, const Dims& d, void* base) {
    Carver k{(char*)base, 0};
    auto take = [&](size_t floats) { return (float*)k.take(floats * 4); };
    Ws w;
    const size_t M = d.M, dd = c.d, I = c.I;
    w.act1 = take((size_t)c.B * d.T1 * d.F1 * c.C1);
    w.act2 = take((size_t)c.B * d.T2 * d.F2 * c.C2);
    w.feo = take(M * dd); w.x = take(M * dd); w.a0 = take(M * dd); w.a1 = take(M * dd); w.a2 = take(M * dd); w.a1r = take(M * dd);
    w.h = take(M * I); w.qkv = take(M * 3 * dd); w.ctx = take(M * dd); w.cat = take(M * 2 * dd); w.m2 = take(M * 2 * dd);
    w.gn = take(M * (I / 2)); w.s = take(M * (I / 2));
    w.cv = w.lin = nullptr;
    if (c.csgu_linear) { w.cv = take(M * (I / 2)); w.lin = take(M * (I / 2)); }
    w.hid = take(M * dd);
    w.lens = (int*)take((size_t)2 * c.B);
    w.attn_bytes = mi_attention_f32_workspace_bytes(c.B, d.T2, c.H, d.hd, c.pos_type == 1);
    w.attn = take((w.attn_bytes + 3) / 4);
    w.bytes = k.off;
    return w;
}

// what this mode does not cover (header: mi_ebf_forward_f32)
bool f32_unsupported(const mi_ebf_config& c) {
    return c.context_mode != 0 || c.layer_mixing || c.extra_layers || c.ln_fold || c.wide_tiles || c.branch_overlap;
}

constexpr float LEPS = 1e-5f;                  // nn.LayerNorm default: the layers use nn.LayerNorm(embed_dim) (e_branchformer.py:233-261)

// One fp32 forward, in the stages of the bf16 driver's un-folded branch (encoder.hip): front end, layer, exit
struct Fwd32 : Slots {
    const mi_ebf_config& c; const Dims D; const Ws w; hipStream_t st;
    const int* mask_len;                          // the inner lengths of a ragged batch, else null
    const float* pos_table; float* posp;          // header: mi_ebf_forward_f32
    const int M, d, I, T2, P;                     // P = 2*T2-1 relative positions
    Fwd32(const mi_ebf_config& c_, const Dims& D_, const Ws& w_, const void* const* weights, hipStream_t st_, const int* mask, const void* pos_table_, void* posp_)
        : Slots{weights}, c(c_), D(D_), w(w_), st(st_), mask_len(mask), pos_table((const float*)pos_table_), posp((float*)posp_), M(D_.M), d(c_.d), I(c_.I), T2(D_.T2),
          P(2 * D_.T2 - 1) {}
    int ln(const float* x, const int* mask, float* xo, const float* g, const float* b, float eps, float* y) const {
        return mi_layernorm_f32(x, d, mask, T2, xo, d, g, b, eps, y, d, M, d, st);
    }
    int first_norms(int l, const int* mask, float* xo) const;
    int front_end(const float* feats, int compute_posp) const;
    int layer(int l) const;
    int exit(int l, float* last_hidden, float* logits) const;
};

// the LayerNorm(s) in front of layer l: ff1's with macaron FFNs, else the two branch norms; mask / xo: as mi_layernorm_f32's, for the first of them
int Fwd32::first_norms(int l, const int* mask, float* xo) const {
    if (c.use_macaron) return ln(w.x, mask, xo, Lf(l, FF1_LN_G), Lf(l, FF1_LN_B), LEPS, w.a0);
    RUN(ln(w.x, mask, xo, Lf(l, ATT_LN_G), Lf(l, ATT_LN_B), LEPS, w.a1));
    return ln(w.x, nullptr, nullptr, Lf(l, MLP_LN_G), Lf(l, MLP_LN_B), LEPS, w.a2);
}

int Fwd32::front_end(const float* feats, int compute_posp) const {
    // --- Conv2d sub-sampling (extractors.py:110-113); causal: all padding on the left (CausalConv2d, streaming_modules.py:31-55)
    const int pl = c.is_causal ? 2 * c.pad : c.pad;
    RUN(mi_conv2d_first_gelu_f32(feats, Gf(G_CONV1_W), Gf(G_CONV1_B), w.act1, c.B, c.T, c.F, c.C1, c.K, c.stride, pl, pl, D.T1, D.F1, st));
    RUN(mi_conv2d_cl_f32(w.act1, Gf(G_CONV2_W), Gf(G_CONV2_B), w.act2, c.B, D.T1, D.F1, c.C1, c.C2, c.K, c.stride, pl, pl, D.T2, D.F2, 1, st));
    // (B,C,T',F') -> transpose -> flatten -> Linear: act2 is already (B*T', F'*C) with the weight columns permuted to match
    RUN(gemm(w.act2, (long)D.F2 * c.C2, Gf(G_FEOUT_W), (long)D.F2 * c.C2, Gf(G_FEOUT_B), w.feo, d, nullptr, 0, 1.f, 0, M, d, D.F2 * c.C2, st));
    // --- feature projection: LN -> Linear (extractors.py:130-131; tf:328-333)
    RUN(ln(w.feo, nullptr, nullptr, Gf(G_FP_LN_G), Gf(G_FP_LN_B), c.ln_eps, w.a0));
    RUN(gemm(w.a0, d, Gf(G_FP_W), d, Gf(G_FP_B), w.x, d, nullptr, 0, 1.f, 0, M, d, d, st));
    // --- zero padded frames once (tf:662-665) + first LayerNorm(s) of layer 0
    RUN(first_norms(0, mask_len, w.x));
    // --- relative positions: p_l = linear_pos_l(table) for every layer (batch independent; tf:531-536)
    if (c.pos_type == 1 && compute_posp)
        for (int l = 0; l < c.L; ++l)
            RUN(gemm(pos_table, d, Lf(l, ATT_WPOS), d, nullptr, posp + (size_t)l * P * d, d, nullptr, 0, 1.f, 0, P, d, d, st));
    return MI_OK;
}

// one layer, from its first LayerNorm's output to the residual stream in front of final_layer_norm
int Fwd32::layer(int l) const {
    const int kc = c.csgu_kernel, km = c.merge_kernel;
    if (c.use_macaron) {   // x += 0.5 * FFN(LN(x))   e_branchformer.py:271-273
        RUN(gemm(w.a0, d, Lf(l, FF1_W1), d, Lf(l, FF1_B1), w.h, I, nullptr, 0, 1.f, 1, M, I, d, st));
        RUN(gemm(w.h, I, Lf(l, FF1_W2), I, Lf(l, FF1_B2), w.x, d, w.x, d, 0.5f, 0, M, d, I, st));
        RUN(ln(w.x, nullptr, nullptr, Lf(l, ATT_LN_G), Lf(l, ATT_LN_B), LEPS, w.a1));
        RUN(ln(w.x, nullptr, nullptr, Lf(l, MLP_LN_G), Lf(l, MLP_LN_B), LEPS, w.a2));
    }
    // global branch (e_branchformer.py:281-288): [Q|K|V] projection (weights are packed [Wq;Wk;Wv]); rotary feeds Q,K from the rotated input only
    if (c.pos_type == 2) {
        RUN(mi_rotary_f32(w.a1, d, w.a1r, d, pos_table, pos_table ? pos_table + (size_t)T2 * D.hd : nullptr, M, T2, c.H, D.hd, st));      // [cos (T2, hd) | sin (T2, hd)]
        RUN(gemm(w.a1r, d, Lf(l, ATT_WQK), d, Lf(l, ATT_BQK), w.qkv, 3 * d, nullptr, 0, 1.f, 0, M, 2 * d, d, st));
        RUN(gemm(w.a1, d, Lf(l, ATT_WV), d, Lf(l, ATT_BV), w.qkv + 2 * d, 3 * d, nullptr, 0, 1.f, 0, M, d, d, st));
    } else {
        RUN(gemm(w.a1, d, Lf(l, ATT_WQK), d, Lf(l, ATT_BQK), w.qkv, 3 * d, nullptr, 0, 1.f, 0, M, 3 * d, d, st));
    }
    const bool rel = c.pos_type == 1;
    RUN(mi_attention_f32(w.qkv, 3 * d, w.qkv + d, 3 * d, w.qkv + 2 * d, 3 * d, rel ? posp + (size_t)l * P * d : nullptr, d,
                         rel ? Lf(l, ATT_U) : nullptr, rel ? Lf(l, ATT_V) : nullptr, mask_len, w.ctx, d,
                         c.B, T2, c.H, D.hd, 1.0f / sqrtf((float)D.hd), c.is_causal, w.attn, w.attn_bytes, st));
    RUN(gemm(w.ctx, d, Lf(l, ATT_WO), d, Lf(l, ATT_BO), w.cat, 2 * d, nullptr, 0, 1.f, 0, M, d, d, st));
    // local branch: cgMLP (e_branchformer.py:291-292, 184-222)
    RUN(gemm(w.a2, d, Lf(l, MLP_W1), d, Lf(l, MLP_B1), w.h, I, nullptr, 0, 1.f, 1, M, I, d, st));
    RUN(mi_layernorm_f32(w.h + I / 2, I, nullptr, T2, nullptr, 0, Lf(l, CSGU_LN_G), Lf(l, CSGU_LN_B), LEPS, w.gn, I / 2, M, I / 2, st));
    // quirk: the causal CSGU conv is dilated by (K-1)/2 (e_branchformer.py:153-160 passes it in the dilation slot)
    const int dil = c.is_causal ? (kc - 1) / 2 : 1;
    const int cpad = c.is_causal ? (kc - 1) * dil : (kc - 1) / 2;
    if (c.csgu_linear) {   // conv -> Linear -> act -> gate (e_branchformer.py:196-201)
        RUN(mi_dwconv_f32(w.gn, I / 2, Lf(l, CSGU_W), Lf(l, CSGU_B), nullptr, 0, w.cv, I / 2, c.B, T2, I / 2, kc, cpad, dil, 0, 0, st));
        RUN(gemm(w.cv, I / 2, Lf(l, CSGU_LIN_W), I / 2, Lf(l, CSGU_LIN_B), w.lin, I / 2, nullptr, 0, 1.f, 0, M, I / 2, I / 2, st));
        RUN(mi_gate_act_mul_f32(w.h, I, w.lin, I / 2, w.s, I / 2, M, I / 2, c.csgu_act, st));
    } else
        RUN(mi_dwconv_f32(w.gn, I / 2, Lf(l, CSGU_W), Lf(l, CSGU_B), w.h, I, w.s, I / 2, c.B, T2, I / 2, kc, cpad, dil, c.csgu_act, 1, st));
    RUN(gemm(w.s, I / 2, Lf(l, MLP_W2), I / 2, Lf(l, MLP_B2), w.cat + d, 2 * d, nullptr, 0, 1.f, 0, M, d, I / 2, st));
    // merge (e_branchformer.py:296-304)
    RUN(mi_dwconv_f32(w.cat, 2 * d, Lf(l, MRG_DW_W), Lf(l, MRG_DW_B), nullptr, 0, w.m2, 2 * d, c.B, T2, 2 * d, km, (km - 1) / 2, 1, 0, 2, st));
    RUN(gemm(w.m2, 2 * d, Lf(l, MRG_W), 2 * d, Lf(l, MRG_B), w.x, d, w.x, d, 1.0f, 0, M, d, 2 * d, st));
    if (c.use_macaron) {   // e_branchformer.py:307-309
        RUN(ln(w.x, nullptr, nullptr, Lf(l, FF2_LN_G), Lf(l, FF2_LN_B), LEPS, w.a0));
        RUN(gemm(w.a0, d, Lf(l, FF2_W1), d, Lf(l, FF2_B1), w.h, I, nullptr, 0, 1.f, 1, M, I, d, st));
        RUN(gemm(w.h, I, Lf(l, FF2_W2), I, Lf(l, FF2_B2), w.x, d, w.x, d, 0.5f, 0, M, d, I, st));
    }
    return MI_OK;
}

// final_layer_norm (:312), then the next consumer: layer l+1's first LayerNorm(s), or after the last layer encoder.layer_norm (tf:707) and the CTC head
int Fwd32::exit(int l, float* last_hidden, float* logits) const {
    if (l + 1 < c.L) {
        RUN(ln(w.x, nullptr, nullptr, Lf(l, FIN_LN_G), Lf(l, FIN_LN_B), LEPS, w.x));
        return first_norms(l + 1, nullptr, nullptr);
    }
    RUN(ln(w.x, nullptr, nullptr, Lf(l, FIN_LN_G), Lf(l, FIN_LN_B), LEPS, w.a0));
    float* lh = last_hidden ? last_hidden : w.hid;
    RUN(ln(w.a0, nullptr, nullptr, Gf(G_ENC_LN_G), Gf(G_ENC_LN_B), c.ln_eps, lh));
    if (!logits) return MI_OK;
    // CTC head: lm_head ⊕ blank_projection, blank LAST (e_branchformer.py:456-457)
    return gemm(lh, d, Gf(G_HEAD_W), d, Gf(G_HEAD_B), logits, c.logits_ld > 0 ? c.logits_ld : c.V + 1, nullptr, 0, 1.f, 0, M, c.V + 1, d, st);
}

}  // namespace

extern "C" size_t mi_ebf_f32_workspace_bytes(const mi_ebf_config* cfg) {
    return sizable(cfg) && !f32_unsupported(*cfg) ? carve(*cfg, dims(*cfg), nullptr).bytes : 0;
}

// pos_table: relative: (2*T2-1, d) FP32 sinusoid table; rotary: fp32 [cos (T2,hd) | sin (T2,hd)].  posp: (L, 2*T2-1, d) FP32.
extern "C" int mi_ebf_forward_f32(const mi_ebf_config* cfg, const void* const* weights, const float* feats, const int* feat_lengths, const void* pos_table, void* posp,
                                  int compute_posp, void* workspace, size_t workspace_bytes, float* last_hidden, float* logits, int* inner_len, int* outer_len,
                                  hipStream_t st) {
    if (!cfg) return MI_ERR_ARG;
    const mi_ebf_config& c = *cfg;
    if (f32_unsupported(c)) return MI_ERR_UNSUPPORTED;        // before anything touches the device
    MI_ENTER();
    if (!weights || !feats || !workspace) return MI_ERR_ARG;
    if (c.B <= 0 || c.T <= 0 || c.L <= 0 || c.H <= 0 || c.d % c.H || c.I % 2 || ((c.d / c.H) & 1) || c.pos_type < 0 || c.pos_type > 2) return MI_ERR_ARG;
    if (c.pos_type != 0 && !pos_table) return MI_ERR_ARG;
    if (c.pos_type == 1 && !posp) return MI_ERR_ARG;
    const Dims D = dims(c);
    if (D.T2 <= 0) return MI_ERR_ARG;
    const Ws w = carve(c, D, workspace);
    if (w.bytes > workspace_bytes) return MI_ERR_ARG;
    int* inner = inner_len ? inner_len : w.lens;
    int* outer = outer_len ? outer_len : w.lens + c.B;
    launch_subsampled_lengths(feat_lengths, c.T, c.B, c.K, c.stride, c.is_causal ? c.K - 1 : 2 * c.pad, 2, D.T2, inner, outer, st);
    const Fwd32 f(c, D, w, weights, st, feat_lengths ? inner : nullptr, pos_table, posp);
    RUN(f.front_end(feats, compute_posp));
    for (int l = 0; l < c.L; ++l) {
        RUN(f.layer(l));
        RUN(f.exit(l, last_hidden, logits));
    }
    MI_CHECK_LAUNCH();
    return MI_OK;
}
