// Rows-streaming linear for decoding: y = act(x · W^T + b) (+ resid) for 1 <= M <= 64 rows, any N, K % 8 == 0.  W bf16 (N, K), x bf16 (M, K), fp32 accumulation.
//
// At these M a linear is a read of W: a 128-wide MFMA tile grid gives six blocks at N = 768 and the GEMV form (decoder_step.hip, skinny_linear_kernel) stops at 8 rows.
// Here W sits on the 32-row side of v_mfma_f32_32x32x16_bf16 and the M rows of x are the other operand, so every weight byte is read once per launch, straight into
// registers: K is walked in chunks of 64 (one 128-B line of a weight row); lane (row i, half h) of a wave fetches the four 16-B pieces of bytes [64 h, 64 h + 64) of its
// row's line, and MFMA p of the chunk contracts the k set {8 p + j} U {32 + 8 p + j}, j < 8 — a permutation of K inside the chunk, applied to both operands, which the
// sum does not see.  The x rows of a block's K range go through LDS in full lines (M x 512 or M x 256 elements per stage, row stride padded by 16 B) and are read back as
// ds_read_b128 fragments.
//
// Decomposition: the launch spreads by N and, where N alone leaves fewer blocks than CUs, by K.
//   KW = 4 (narrow N): a block owns 32 weight rows, its four waves take every fourth chunk of the block's K range and are summed through LDS in wave order.
//   KW = 1 (wide N, the vocabulary head): a block owns 128 weight rows, one 32-row tile per wave, every wave walks the whole K range.
// A split over K writes fp32 partials (ksplit, M, N) and a small second launch adds them in slice order and runs the epilogue: no float atomics, fixed order everywhere,
// so results are bit-reproducible, and a row's result is a function of that row alone (an MFMA output column reads one column of the x operand).
// Epilogue: bias, activation (0 none / 1 erf-GELU, the library's fit / 2 gelu_new), fp32 output (plain or added in place to what is there: the residual stream), or bf16
// output with the K/V-cache append of skinny_linear_kernel (same argument meaning).
#include "common.hpp"
#include "../../include/hfasr_hip.h"

namespace {

constexpr int LR_CHUNK = 64;           // k per chunk: one 128-B line of a weight row
constexpr int LR_RED_LD = 33;          // [part][m][33]: accumulator tiles through LDS, i (weight row) fastest: conflict-free both ways

struct LrArgs {
    const bf16_t* x; long ldx;
    const bf16_t* W; long ldw; const float* bias;
    float* out32; long ldo32; int accumulate;        // fp32 output: out32 = (accumulate ? out32 : 0) + v
    bf16_t* out16; long ldo16;                       // bf16 output
    bf16_t* kc; bf16_t* vc; int U, past, Lmax, dkv;  // optional (kc != null, bf16 output): columns [dkv, 2 dkv) / [2 dkv, 3 dkv) are ALSO appended to the K / V caches at row past + u
    float* part;                                     // (ksplit, M, N) fp32 when ksplit > 1
    int M, N, K, act, ksplit, cps;                   // cps: chunks per K slice
};

__device__ __forceinline__ void lr_emit(const LrArgs& p, int m, int n, float v) {
    v += p.bias ? p.bias[n] : 0.f;
    if (p.act == 1) v = gelu_erf(v);
    else if (p.act == 2) v = gelu_tanh(v);
    if (p.out32) {
        float* o = p.out32 + (long)m * p.ldo32 + n;
        *o = p.accumulate ? *o + v : v;
    } else {
        const bf16_t o = f2bf(v);
        p.out16[(long)m * p.ldo16 + n] = o;
        if (p.kc && n >= p.dkv) {
            const int b = m / p.U, u = m - b * p.U;
            const long row = ((long)b * p.Lmax + p.past + u) * p.dkv;
            if (n < 2 * p.dkv) p.kc[row + n - p.dkv] = o; else p.vc[row + n - 2 * p.dkv] = o;
        }
    }
}

// MT: 32-row tiles of x (1: M <= 32, 2: M <= 64).  KW: waves of a block along K (4) or along N (1).
template <int MT, int KW>
__global__ __launch_bounds__(256) void linear_rows_kernel(LrArgs p) {
    constexpr int SC = KW == 4 ? 8 : 4;              // chunks per stage
    constexpr int CPW = SC / KW;                     // chunks per wave and stage: 2 / 4
    constexpr int XS = SC * LR_CHUNK + 8;            // LDS row stride of x in elements (+16 B: the 32 rows of a fragment read land on different banks)
    constexpr int RB = KW == 4 ? 32 : 128;           // weight rows per block
    extern __shared__ __attribute__((aligned(16))) char smem[];
    bf16_t* xs = reinterpret_cast<bf16_t*>(smem);                                   // [M][XS]
    float* red = reinterpret_cast<float*>(smem);                                    // after the K walk: [4][32 MT][LR_RED_LD]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int li = lane & 31, lh = lane >> 5;
    const int n0 = blockIdx.x * RB;
    const int chunks = (p.K + LR_CHUNK - 1) / LR_CHUNK;
    const int c0 = blockIdx.y * p.cps;
    const int c1 = c0 + p.cps < chunks ? c0 + p.cps : chunks;
    const int kend = c1 * LR_CHUNK < p.K ? c1 * LR_CHUNK : p.K;                     // x is zero from here on: a chunk or piece past it contributes nothing
    int wrow = n0 + (KW == 4 ? 0 : wave * 32) + li;
    wrow = wrow < p.N ? wrow : p.N - 1;                                             // rows past N: a valid row's data, never stored
    const bf16_t* wp = p.W + (long)wrow * p.ldw;
    int xr[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) { const int m = t * 32 + li; xr[t] = (m < p.M ? m : 0) * XS + lh * 32; }

    f32x16 acc[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

    for (int cb = c0; cb < c1; cb += SC) {
        // this wave's weight pieces of the stage do not depend on x: requested first, consumed after the barrier (past the block's K range: the row's first piece again, which meets zeros of x)
        bf16x8 wv[CPW][4];
#pragma unroll
        for (int j = 0; j < CPW; ++j)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int k = (cb + (KW == 4 ? wave + 4 * j : j)) * LR_CHUNK + lh * 32 + q * 8;
                wv[j][q] = *reinterpret_cast<const bf16x8*>(wp + (k < kend ? k : 0));
            }
        if (cb != c0) __syncthreads();                                              // the previous stage's fragments are read
        const int kb = cb * LR_CHUNK;
        for (int i = threadIdx.x; i < p.M * SC * 8; i += 256) {
            const int m = i / (SC * 8), pc = i - m * (SC * 8);
            const int k = kb + pc * 8;
            bf16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
            if (k < kend) v = *reinterpret_cast<const bf16x8*>(p.x + (long)m * p.ldx + k);
            *reinterpret_cast<bf16x8*>(xs + m * XS + pc * 8) = v;
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < CPW; ++j) {
            const int cl = KW == 4 ? wave + 4 * j : j;                              // chunk of the stage
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int t = 0; t < MT; ++t) {
                    const bf16x8 xb = *reinterpret_cast<const bf16x8*>(xs + xr[t] + cl * LR_CHUNK + q * 8);
                    acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wv[j][q], xb, acc[t], 0, 0, 0);
                }
        }
    }
    __syncthreads();
    // accumulators -> LDS: C[i][m] sits in lane m + 32 h, register r, with i = 8 (r / 4) + 4 h + r % 4
#pragma unroll
    for (int t = 0; t < MT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r)
            red[(wave * 32 * MT + t * 32 + li) * LR_RED_LD + 8 * (r >> 2) + 4 * lh + (r & 3)] = acc[t][r];
    __syncthreads();
    for (int i = threadIdx.x; i < RB * p.M; i += 256) {
        const int m = i / RB, r = i - m * RB, n = n0 + r;
        if (n >= p.N) continue;
        float v;
        if (KW == 4) {
            const float* s = red + m * LR_RED_LD + r;
            v = ((s[0] + s[32 * MT * LR_RED_LD]) + s[2 * 32 * MT * LR_RED_LD]) + s[3 * 32 * MT * LR_RED_LD];      // waves in order
        } else {
            v = red[((r >> 5) * 32 * MT + m) * LR_RED_LD + (r & 31)];
        }
        if (p.ksplit > 1) p.part[((long)blockIdx.y * p.M + m) * p.N + n] = v;
        else lr_emit(p, m, n, v);
    }
}

// the K slices of a split launch, added in slice order, then the epilogue
__global__ __launch_bounds__(256) void linear_rows_combine_kernel(LrArgs p) {
    const long total = (long)p.M * p.N;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    float v = p.part[i];
    for (int s = 1; s < p.ksplit; ++s) v += p.part[(long)s * total + i];
    lr_emit(p, (int)(i / p.N), (int)(i % p.N), v);
}

struct LrPlan { int kw, ksplit, cps; };
// a function of (N, K) only: the K order of a row's sum does not change with the number of rows beside it
LrPlan lr_plan(int N, int K) {
    const int chunks = (K + LR_CHUNK - 1) / LR_CHUNK;
    LrPlan pl;
    pl.kw = cdiv(N, 128) >= 192 ? 1 : 4;
    const int tiles = pl.kw == 4 ? cdiv(N, 32) : cdiv(N, 128);
    int want = cdiv(256, tiles);                                // blocks ~ the CU count
    const int most = pl.kw == 4 ? (chunks / 4 > 0 ? chunks / 4 : 1) : chunks;          // KW = 4: at least one chunk per wave
    want = want < 1 ? 1 : (want > most ? most : want);
    pl.cps = want == 1 ? chunks : cdiv(chunks, want);
    if (pl.kw == 4 && want > 1) pl.cps = chunks / want / 4 * 4 > 4 ? chunks / want / 4 * 4 : 4;    // whole rounds of the four waves
    pl.ksplit = cdiv(chunks, pl.cps);
    return pl;
}

template <int MT, int KW>
int lr_launch(const LrArgs& a, hipStream_t st) {
    constexpr int SC = KW == 4 ? 8 : 4;
    const size_t xs = (size_t)a.M * (SC * LR_CHUNK + 8) * sizeof(bf16_t), red = (size_t)4 * 32 * MT * LR_RED_LD * sizeof(float);
    const size_t lds = xs > red ? xs : red;
    if (!ensure_dynamic_lds<0>((const void*)linear_rows_kernel<MT, KW>, 72 * 1024)) return MI_ERR_LAUNCH;
    hipLaunchKernelGGL((linear_rows_kernel<MT, KW>), dim3(cdiv(a.N, KW == 4 ? 32 : 128), a.ksplit), dim3(256), lds, st, a);
    return MI_OK;
}

}  // namespace

size_t linear_rows_workspace_floats(int M, int N, int K) {
    const LrPlan pl = lr_plan(N, K);
    return pl.ksplit > 1 ? (size_t)pl.ksplit * M * N : 0;
}

int linear_rows(const bf16_t* x, long ldx, const bf16_t* W, long ldw, const float* bias, int act, float* out32, long ldo32, int accumulate, bf16_t* out16, long ldo16,
                bf16_t* kc, bf16_t* vc, int U, int past, int Lmax, int dkv, int M, int N, int K, float* workspace, size_t workspace_floats, hipStream_t st) {
    if (M <= 0 || M > 64 || N <= 0 || K <= 0 || (K % 8) || (ldw % 8) || (ldx % 8) || ldw < K || ldx < K || act < 0 || act > 2) return MI_ERR_ARG;
    if ((out32 == nullptr) == (out16 == nullptr)) return MI_ERR_ARG;
    if (((uintptr_t)x | (uintptr_t)W) & 15) return MI_ERR_ARG;
    if (kc && (!out16 || !vc || U <= 0 || (M % U) || N != 3 * dkv || past < 0 || past + U > Lmax)) return MI_ERR_ARG;
    const LrPlan pl = lr_plan(N, K);
    LrArgs a{x, ldx, W, ldw, bias, out32, ldo32, accumulate, out16, ldo16, kc, vc, U, past, Lmax, dkv, workspace, M, N, K, act, pl.ksplit, pl.cps};
    if (pl.ksplit > 1 && (!workspace || workspace_floats < (size_t)pl.ksplit * M * N)) return MI_ERR_ARG;
    int rc;
    if (M <= 32) rc = pl.kw == 4 ? lr_launch<1, 4>(a, st) : lr_launch<1, 1>(a, st);
    else rc = pl.kw == 4 ? lr_launch<2, 4>(a, st) : lr_launch<2, 1>(a, st);
    if (rc != MI_OK) return rc;
    if (pl.ksplit > 1) hipLaunchKernelGGL(linear_rows_combine_kernel, dim3(cdiv((long)M * N, 256)), dim3(256), 0, st, a);
    return MI_OK;
}

extern "C" size_t mi_linear_rows_workspace_bytes(int M, int N, int K) { return linear_rows_workspace_floats(M, N, K) * sizeof(float); }

extern "C" int mi_linear_rows(const void* x, long ldx, const void* W, long ldw, const float* bias, int act, float* out32, long ldo32, int accumulate, void* out16,
                              long ldo16, void* kcache, void* vcache, int U, int past, int Lmax, int dkv, int M, int N, int K, void* workspace, size_t workspace_bytes,
                              hipStream_t st) {
    MI_ENTER();
    const int rc = linear_rows((const bf16_t*)x, ldx, (const bf16_t*)W, ldw, bias, act, out32, ldo32, accumulate, (bf16_t*)out16, ldo16, (bf16_t*)kcache, (bf16_t*)vcache,
                               U, past, Lmax, dkv, M, N, K, (float*)workspace, workspace_bytes / sizeof(float), st);
    if (rc != MI_OK) return rc;
    MI_CHECK_LAUNCH();
    return MI_OK;
}
