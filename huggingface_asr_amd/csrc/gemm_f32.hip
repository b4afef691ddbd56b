// fp32 GEMM on the f32-input matrix instruction (v_mfma_f32_32x32x2_f32) — the dense contraction of the precision = "fp32" inference mode.
//
//   C (M, N) fp32 = resid + alpha * act(A (M, K) · W (N, K)^T + bias)          every operand fp32, nothing is rounded to a narrower format anywhere
//
// The instruction is bit-for-bit a k-ordered fmaf chain (one rounding per product, no wider internal accumulation), so an output element is
//   fma(a[K-1], w[K-1], ... fma(a[1], w[1], fma(a[0], w[0], 0)))
// whatever the tile it lands in: no split-K, no atomics, a result depends on its own row of A and its own row of W only, and two runs are bit-identical.
//
// Block: 256 threads = 4 waves on a 128 x 128 output tile (each wave 2 x 2 tiles of 32 x 32, 64 accumulator registers), K walked in steps of 16 through LDS
// ([row][16 + 1] floats per operand: the odd row stride spreads the 32 rows a half-wave reads over 32 banks).  The next K step's global loads are issued before the
// current one's MFMAs.  Edges: rows past M / N and columns past K are ZERO-FILLED in the loads (the 32x32x2 form consumes K in pairs: an odd K gets a zero
// partner; fma(0, 0, acc) = acc), stores are guarded.  Any M, N, K >= 1, any leading dimensions; 16-byte loads where pointers and strides allow, scalar ones otherwise.
#include "common.hpp"
#include "gemm_f32.hpp"
#include "../../include/hfasr_hip.h"

namespace {

constexpr int BM = 128, BN = 128, BK = 16, LD = BK + 1;

__device__ __forceinline__ float gelu_exact(float v) { return 0.5f * v * (1.0f + erff(v * 0.70710678118654752440f)); }
// GPT-2's gelu_new with the exact tanhf (the decoder MLP of the fp32 token step above 64 rows and of the teacher-forced forward)
__device__ __forceinline__ float gelu_new_exact(float v) { return 0.5f * v * (1.0f + tanhf(0.7978845608028654f * (v + 0.044715f * v * v * v))); }

struct RowSrc { const float* p; bool ok; int t0, f0; };

// eight consecutive k (k0 a multiple of 8) of one row of a (rows, K) operand with contiguous k
__device__ __forceinline__ void load_row8(const RowSrc& r, int k0, int K, bool vec, float* v) {
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = 0.f;
    if (!r.ok || k0 >= K) return;
    if (vec && k0 + 8 <= K) {
        const f32x4 x = *(const f32x4*)(r.p + k0), y = *(const f32x4*)(r.p + k0 + 4);
        v[0] = x[0]; v[1] = x[1]; v[2] = x[2]; v[3] = x[3]; v[4] = y[0]; v[5] = y[1]; v[6] = y[2]; v[7] = y[3];
        return;
    }
#pragma unroll
    for (int e = 0; e < 8; ++e)
        if (k0 + e < K) v[e] = r.p[k0 + e];
}

// the same for the implicit-GEMM Conv2d: k = (kh, kw, c), c fastest; r.p = the image of this row's batch element, (t0, f0) its window origin
__device__ __forceinline__ void load_conv8(const GemmF32Args& g, const RowSrc& r, int k0, bool vec, float* v) {
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = 0.f;
    if (!r.ok || k0 >= g.K) return;
    if (vec) {                                      // C1 % 8 == 0: the eight share (kh, kw); K = KH * KW * C1 is a multiple of 8 too
        const int kk = k0 / g.C1, c = k0 - kk * g.C1, kh = kk / g.KW, kw = kk - kh * g.KW;
        const int t = r.t0 + kh, f = r.f0 + kw;
        if (t < 0 || t >= g.T1 || f < 0 || f >= g.F1) return;
        const float* p = r.p + ((long)t * g.F1 + f) * g.C1 + c;
        const f32x4 x = *(const f32x4*)p, y = *(const f32x4*)(p + 4);
        v[0] = x[0]; v[1] = x[1]; v[2] = x[2]; v[3] = x[3]; v[4] = y[0]; v[5] = y[1]; v[6] = y[2]; v[7] = y[3];
        return;
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int k = k0 + e;
        if (k >= g.K) continue;
        const int kk = k / g.C1, c = k - kk * g.C1, kh = kk / g.KW, kw = kk - kh * g.KW;
        const int t = r.t0 + kh, f = r.f0 + kw;
        if (t >= 0 && t < g.T1 && f >= 0 && f < g.F1) v[e] = r.p[((long)t * g.F1 + f) * g.C1 + c];
    }
}

// eight consecutive n of row k of a (K, N) operand with contiguous n (the w_kn form)
__device__ __forceinline__ void load_kn8(const float* W, long ldw, int k, int K, int n, int N, bool vec, float* v) {
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = 0.f;
    if (k >= K || n >= N) return;
    const float* p = W + (long)k * ldw + n;
    if (vec && n + 8 <= N) {
        const f32x4 x = *(const f32x4*)p, y = *(const f32x4*)(p + 4);
        v[0] = x[0]; v[1] = x[1]; v[2] = x[2]; v[3] = x[3]; v[4] = y[0]; v[5] = y[1]; v[6] = y[2]; v[7] = y[3];
        return;
    }
#pragma unroll
    for (int e = 0; e < 8; ++e)
        if (n + e < N) v[e] = p[e];
}

__global__ __launch_bounds__(256) void gemm_f32_kernel(const GemmF32Args g, const int vecA, const int vecW) {
    __shared__ float As[BM * LD];
    __shared__ float Ws[BN * LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BN;
    const int z = blockIdx.z, zb = z / g.nh, zh = z - zb * g.nh;
    const float* A = g.A + zb * g.sAb + zh * g.sAh;
    const float* W = g.W + zb * g.sWb + zh * g.sWh;
    float* C = g.C + zb * g.sCb + zh * g.sCh;

    // what this thread brings in per K step: eight k of one A row; eight k of one W row, or (w_kn) eight n of one k
    const int lr = tid >> 1, lk = (tid & 1) * 8;
    RowSrc ra;
    {
        const int m = m0 + lr;
        ra.ok = m < g.M; ra.t0 = ra.f0 = 0; ra.p = A;
        if (ra.ok) {
            if (g.conv) {
                const int f2 = m % g.F2, bt = m / g.F2, t2 = bt % g.T2, b = bt / g.T2;
                ra.p = A + (long)b * g.T1 * g.F1 * g.C1;
                ra.t0 = t2 * g.stride - g.pt; ra.f0 = f2 * g.stride - g.pf;
            } else {
                ra.p = A + (long)m * g.lda;
            }
        }
    }
    RowSrc rw;
    rw.ok = !g.w_kn && n0 + lr < g.N; rw.t0 = rw.f0 = 0;
    rw.p = rw.ok ? W + (long)(n0 + lr) * g.ldw : W;
    const int kn_k = tid >> 4, kn_n = (tid & 15) * 8;

    float va[8], vw[8];
    auto fetch = [&](int kt) {
        if (g.conv) load_conv8(g, ra, kt * BK + lk, vecA != 0, va);
        else load_row8(ra, kt * BK + lk, g.K, vecA != 0, va);
        if (g.w_kn) load_kn8(W, g.ldw, kt * BK + kn_k, g.K, n0 + kn_n, g.N, vecW != 0, vw);
        else load_row8(rw, kt * BK + lk, g.K, vecW != 0, vw);
    };

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64, fr = lane & 31, fk = lane >> 5;
    const int nkt = (g.K + BK - 1) / BK;
    fetch(0);
    for (int kt = 0; kt < nkt; ++kt) {
#pragma unroll
        for (int e = 0; e < 8; ++e) As[lr * LD + lk + e] = va[e];
        if (g.w_kn) {
#pragma unroll
            for (int e = 0; e < 8; ++e) Ws[(kn_n + e) * LD + kn_k] = vw[e];
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) Ws[lr * LD + lk + e] = vw[e];
        }
        __syncthreads();
        if (kt + 1 < nkt) fetch(kt + 1);
#pragma unroll
        for (int kk = 0; kk < BK; kk += 2) {
            const float a0 = As[(wm + fr) * LD + kk + fk], a1 = As[(wm + 32 + fr) * LD + kk + fk];
            const float b0 = Ws[(wn + fr) * LD + kk + fk], b1 = Ws[(wn + 32 + fr) * LD + kk + fk];
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
        }
        __syncthreads();
    }

    // epilogue: C/D layout of the 32x32 forms: column = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int n = n0 + wn + j * 32 + fr;
        if (n >= g.N) continue;
        const float bv = g.bias ? g.bias[n] : 0.f;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = m0 + wm + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * fk;
                if (m >= g.M) continue;
                float v = acc[i][j][r] + bv;
                if (g.act == 1) v = gelu_exact(v);
                else if (g.act == 2) v = gelu_new_exact(v);
                v *= g.alpha;
                if (g.resid) v = g.resid[(long)m * g.ldr + n] + v;
                C[(long)m * g.ldc + n] = v;
            }
    }
}

bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

int gemm_f32_launch(const GemmF32Args& a, hipStream_t st) {
    if (!a.A || !a.W || !a.C || a.M < 1 || a.N < 1 || a.K < 1 || a.nz < 1 || a.nh < 1 || a.nz > 65535 || a.act < 0 || a.act > 2) return MI_ERR_ARG;
    if (a.resid && a.nz != 1) return MI_ERR_ARG;
    const long gy = (a.N + BN - 1) / BN;
    if (gy > 65535) return MI_ERR_UNSUPPORTED;
    int vecA, vecW;
    if (a.conv) {
        if (a.T1 < 1 || a.F1 < 1 || a.C1 < 1 || a.KW < 1 || a.stride < 1 || a.T2 < 1 || a.F2 < 1 || a.K % (a.C1 * a.KW) != 0) return MI_ERR_ARG;
        vecA = al16(a.A) && (a.C1 % 8) == 0;
    } else {
        if (a.lda < a.K) return MI_ERR_ARG;
        vecA = al16(a.A) && (a.lda % 4) == 0 && (a.sAb % 4) == 0 && (a.sAh % 4) == 0;
    }
    if (a.ldw < (a.w_kn ? a.N : a.K) || a.ldc < a.N || (a.resid && a.ldr < a.N)) return MI_ERR_ARG;
    vecW = al16(a.W) && (a.ldw % 4) == 0 && (a.sWb % 4) == 0 && (a.sWh % 4) == 0;
    hipLaunchKernelGGL(gemm_f32_kernel, dim3((unsigned)((a.M + BM - 1) / BM), (unsigned)gy, (unsigned)a.nz), dim3(256), 0, st, a, vecA, vecW);
    return MI_OK;
}

extern "C" int mi_gemm_f32(const float* A, long lda, const float* W, long ldw, const float* bias, float* C, long ldc, const float* resid, long ldr,
                           float alpha, int act, int M, int N, int K, hipStream_t stream) {
    MI_ENTER();
    GemmF32Args a{};
    a.A = A; a.lda = lda; a.W = W; a.ldw = ldw; a.bias = bias; a.resid = resid; a.ldr = ldr; a.C = C; a.ldc = ldc;
    a.alpha = alpha; a.act = act; a.M = M; a.N = N; a.K = K; a.nz = 1; a.nh = 1;
    const int rc = gemm_f32_launch(a, stream);
    if (rc != MI_OK) return rc;
    MI_CHECK_LAUNCH();
    return MI_OK;
}
