// precision = "fp32" for the joint model's decoder: the GPT-2 token step, its rows-streaming linear and its attention over cached / cross keys with NO value rounded to
// bf16 — what the reference's decode recipes (no --bf16) run per emitted token.  Opt-in (decoder.py `precision="fp32"`); the bf16 step (decoder_step.hip, linear_rows.hip)
// is untouched by anything here.
//
// Rows-streaming fp32 linear: y = act(x · W^T + b) (+ what is there) for 1 <= M <= 64 rows, any N, K % 4 == 0.  linear_rows.hip's decomposition carries over byte for
// byte with half the k per 128-byte line: W sits on the 32-row side of v_mfma_f32_32x32x2_f32, the M rows of x are the other operand, so every weight byte is read once
// per launch, straight into registers with 16-byte loads.  K is walked in chunks of 32 (one 128-B line of a weight row); lane (row i, half h) of a wave fetches the four
// 16-B pieces of bytes [64 h, 64 h + 64) of its row's line, and MFMA (q, e) of the chunk contracts the k pair {4 q + e, 16 + 4 q + e} — a permutation of K inside the
// chunk, applied to both operands.  The x rows of a block's K range go through LDS in full lines (row stride padded by 16 B) and come back as ds_read_b128 fragments.
//   KW = 4 (narrow N): a block owns 32 weight rows, its four waves take every fourth chunk of the block's K range and are summed through LDS in wave order.
//   KW = 1 (wide N):   a block owns 128 weight rows, one 32-row tile per wave, every wave walks the whole K range.
// Where N alone leaves fewer blocks than CUs the launch spreads over K as well: fp32 partials (ksplit, M, N), added in slice order by a second launch that runs the
// epilogue.  No float atomics and a fixed order everywhere: results are bit-reproducible; the plan is a function of (N, K) only and an MFMA output column reads one
// column of the x operand, so a row's result is a function of that row alone, whatever M is.
// Epilogue: bias, activation (0 none / 2 gelu_new with the exact tanhf), fp32 output (plain or added in place: the residual stream), and optionally columns
// [dkv, 3 dkv) appended to fp32 K / V caches (the argument meaning of the bf16 kernel).
//
// General fp32 attention: one block per (query row, head); fp32 scores of the row's valid keys in LDS, softmax with expf and a division by the sum, fp32 P · V.
// Step driver: mi_decoder_step_beams' argument meaning and pointer-table order with every slot fp32.
#include "common.hpp"
#include "gemm_f32.hpp"
#include "../../include/hfasr_hip.h"

namespace {

__device__ __forceinline__ float gelu_new_exact(float x) { return 0.5f * x * (1.0f + tanhf(0.7978845608028654f * (x + 0.044715f * x * x * x))); }

// ------------------------------------------------------------------------------------------------ rows-streaming linear
constexpr int LF_CHUNK = 32;           // k per chunk: one 128-B line of a weight row
constexpr int LF_RED_LD = 33;          // [part][m][33]: accumulator tiles through LDS, i (weight row) fastest

struct LfArgs {
    const float* x; long ldx;
    const float* W; long ldw; const float* bias;
    float* out; long ldo; int accumulate;           // out = (accumulate ? out : 0) + v
    float* kc; float* vc; int U, past, Lmax, dkv;   // optional (kc != null): columns [dkv, 2 dkv) / [2 dkv, 3 dkv) are ALSO appended to the K / V caches at row past + u
    float* part;                                    // (ksplit, M, N) fp32 when ksplit > 1
    int M, N, K, act, ksplit, cps;                  // cps: chunks per K slice
};

__device__ __forceinline__ void lf_emit(const LfArgs& p, int m, int n, float v) {
    v += p.bias ? p.bias[n] : 0.f;
    if (p.act == 2) v = gelu_new_exact(v);
    float* o = p.out + (long)m * p.ldo + n;
    v = p.accumulate ? *o + v : v;
    *o = v;
    if (p.kc && n >= p.dkv) {
        const int b = m / p.U, u = m - b * p.U;
        const long row = ((long)b * p.Lmax + p.past + u) * p.dkv;
        if (n < 2 * p.dkv) p.kc[row + n - p.dkv] = v; else p.vc[row + n - 2 * p.dkv] = v;
    }
}

// MT: 32-row tiles of x (1: M <= 32, 2: M <= 64).  KW: waves of a block along K (4) or along N (1).
template <int MT, int KW>
__global__ __launch_bounds__(256) void linear_rows_f32_kernel(LfArgs p) {
    constexpr int SC = KW == 4 ? 8 : 4;              // chunks per stage
    constexpr int CPW = SC / KW;                     // chunks per wave and stage: 2 / 4
    constexpr int XS = SC * LF_CHUNK + 4;            // LDS row stride of x in floats (+16 B: the 32 rows of a fragment read land on different banks)
    constexpr int RB = KW == 4 ? 32 : 128;           // weight rows per block
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* xs = reinterpret_cast<float*>(smem);                                     // [M][XS]
    float* red = reinterpret_cast<float*>(smem);                                    // after the K walk: [4][32 MT][LF_RED_LD]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int li = lane & 31, lh = lane >> 5;
    const int n0 = blockIdx.x * RB;
    const int chunks = (p.K + LF_CHUNK - 1) / LF_CHUNK;
    const int c0 = blockIdx.y * p.cps;
    const int c1 = c0 + p.cps < chunks ? c0 + p.cps : chunks;
    const int kend = c1 * LF_CHUNK < p.K ? c1 * LF_CHUNK : p.K;                     // x is zero from here on: a chunk or piece past it contributes nothing
    int wrow = n0 + (KW == 4 ? 0 : wave * 32) + li;
    wrow = wrow < p.N ? wrow : p.N - 1;                                             // rows past N: a valid row's data, never stored
    const float* wp = p.W + (long)wrow * p.ldw;
    int xr[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) { const int m = t * 32 + li; xr[t] = (m < p.M ? m : 0) * XS + lh * 16; }

    f32x16 acc[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

    for (int cb = c0; cb < c1; cb += SC) {
        // this wave's weight pieces of the stage do not depend on x: requested first, consumed after the barrier (past the block's K range: the row's first piece again, which meets zeros of x)
        f32x4 wv[CPW][4];
#pragma unroll
        for (int j = 0; j < CPW; ++j)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int k = (cb + (KW == 4 ? wave + 4 * j : j)) * LF_CHUNK + lh * 16 + q * 4;
                wv[j][q] = *reinterpret_cast<const f32x4*>(wp + (k < kend ? k : 0));
            }
        if (cb != c0) __syncthreads();                                              // the previous stage's fragments are read
        const int kb = cb * LF_CHUNK;
        for (int i = threadIdx.x; i < p.M * SC * 8; i += 256) {
            const int m = i / (SC * 8), pc = i - m * (SC * 8);
            const int k = kb + pc * 4;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (k < kend) v = *reinterpret_cast<const f32x4*>(p.x + (long)m * p.ldx + k);
            *reinterpret_cast<f32x4*>(xs + m * XS + pc * 4) = v;
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < CPW; ++j) {
            const int cl = KW == 4 ? wave + 4 * j : j;                              // chunk of the stage
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                f32x4 xb[MT];
#pragma unroll
                for (int t = 0; t < MT; ++t) xb[t] = *reinterpret_cast<const f32x4*>(xs + xr[t] + cl * LF_CHUNK + q * 4);
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int t = 0; t < MT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(wv[j][q][e], xb[t][e], acc[t], 0, 0, 0);
            }
        }
    }
    __syncthreads();
    // accumulators -> LDS: C[i][m] sits in lane m + 32 h, register r, with i = 8 (r / 4) + 4 h + r % 4
#pragma unroll
    for (int t = 0; t < MT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r)
            red[(wave * 32 * MT + t * 32 + li) * LF_RED_LD + 8 * (r >> 2) + 4 * lh + (r & 3)] = acc[t][r];
    __syncthreads();
    for (int i = threadIdx.x; i < RB * p.M; i += 256) {
        const int m = i / RB, r = i - m * RB, n = n0 + r;
        if (n >= p.N) continue;
        float v;
        if (KW == 4) {
            const float* s = red + m * LF_RED_LD + r;
            v = ((s[0] + s[32 * MT * LF_RED_LD]) + s[2 * 32 * MT * LF_RED_LD]) + s[3 * 32 * MT * LF_RED_LD];      // waves in order
        } else {
            v = red[((r >> 5) * 32 * MT + m) * LF_RED_LD + (r & 31)];
        }
        if (p.ksplit > 1) p.part[((long)blockIdx.y * p.M + m) * p.N + n] = v;
        else lf_emit(p, m, n, v);
    }
}

// the K slices of a split launch, added in slice order, then the epilogue
__global__ __launch_bounds__(256) void linear_rows_f32_combine_kernel(LfArgs p) {
    const long total = (long)p.M * p.N;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    float v = p.part[i];
    for (int s = 1; s < p.ksplit; ++s) v += p.part[(long)s * total + i];
    lf_emit(p, (int)(i / p.N), (int)(i % p.N), v);
}

struct LfPlan { int kw, ksplit, cps; };
// a function of (N, K) only: the K order of a row's sum does not change with the number of rows beside it
LfPlan lf_plan(int N, int K) {
    const int chunks = (K + LF_CHUNK - 1) / LF_CHUNK;
    LfPlan pl;
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
int lf_launch(const LfArgs& a, hipStream_t st) {
    constexpr int SC = KW == 4 ? 8 : 4;
    const size_t xs = (size_t)a.M * (SC * LF_CHUNK + 4) * sizeof(float), red = (size_t)4 * 32 * MT * LF_RED_LD * sizeof(float);
    const size_t lds = xs > red ? xs : red;
    if (!ensure_dynamic_lds<0>((const void*)linear_rows_f32_kernel<MT, KW>, 72 * 1024)) return MI_ERR_LAUNCH;
    hipLaunchKernelGGL((linear_rows_f32_kernel<MT, KW>), dim3(cdiv(a.N, KW == 4 ? 32 : 128), a.ksplit), dim3(256), lds, st, a);
    return MI_OK;
}

constexpr int ROWS_MAXM = 64;

size_t linear_rows_f32_workspace_floats(int M, int N, int K) {
    if (M <= 0 || N <= 0 || K <= 0) return 0;
    const LfPlan pl = lf_plan(N, K);
    return pl.ksplit > 1 ? (size_t)pl.ksplit * M * N : 0;
}

int linear_rows_f32(const float* x, long ldx, const float* W, long ldw, const float* bias, int act, float* out, long ldo, int accumulate,
                    float* kc, float* vc, int U, int past, int Lmax, int dkv, int M, int N, int K, float* workspace, size_t workspace_floats, hipStream_t st) {
    if (K > 0 && (K % 4)) return MI_ERR_UNSUPPORTED;                                // 16-byte pieces of a weight row
    if (M <= 0 || M > ROWS_MAXM || N <= 0 || K <= 0 || (ldw % 4) || (ldx % 4) || ldw < K || ldx < K || ldo < N || (act != 0 && act != 2)) return MI_ERR_ARG;
    if (!x || !W || !out || (((uintptr_t)x | (uintptr_t)W) & 15)) return MI_ERR_ARG;
    if (kc && (!vc || U <= 0 || (M % U) || N != 3 * dkv || past < 0 || past + U > Lmax)) return MI_ERR_ARG;
    const LfPlan pl = lf_plan(N, K);
    if ((long)cdiv(N, pl.kw == 4 ? 32 : 128) > 0x7fffffffL || pl.ksplit > 65535) return MI_ERR_UNSUPPORTED;
    LfArgs a{x, ldx, W, ldw, bias, out, ldo, accumulate, kc, vc, U, past, Lmax, dkv, workspace, M, N, K, act, pl.ksplit, pl.cps};
    if (pl.ksplit > 1 && (!workspace || workspace_floats < (size_t)pl.ksplit * M * N)) return MI_ERR_ARG;
    int rc;
    if (M <= 32) rc = pl.kw == 4 ? lf_launch<1, 4>(a, st) : lf_launch<1, 1>(a, st);
    else rc = pl.kw == 4 ? lf_launch<2, 4>(a, st) : lf_launch<2, 1>(a, st);
    if (rc != MI_OK) return rc;
    if (pl.ksplit > 1) hipLaunchKernelGGL(linear_rows_f32_combine_kernel, dim3(cdiv((long)M * N, 256)), dim3(256), 0, st, a);
    return MI_OK;
}

// ------------------------------------------------------------------------------------------------ attention over cached / cross keys
// One block per (query row, head).  LPK = HD / 4 lanes share a key (16-B pieces of its K and V rows), the block's 256 / LPK key slots split the keys.  The scores of the
// row's n valid keys live in LDS; max, exp (expf) and sum in fp32, each in a fixed order (a thread's keys in key order, the wave by DPP, the four waves in wave order);
// P · V per key slot in key order, the slots added in slot order.  A key outside the valid set is never read and contributes exactly 0.  A row with no key at all is
// uniform over all Tk keys, as mi_attention_f32 documents.
constexpr int AT_MAX_KEYS = 15 * 1024;          // scores of one query row in LDS: 60 KiB, + the reduction buffers

struct AtArgs {
    const float* q; long ldq; const float* k; long ldk; const float* v; long ldv; long kv_bstride;
    const int* lengths; float* out; long ldo;
    int Tq, Tk, H, beams, causal; float scale;
};

template <int HD>
__global__ __launch_bounds__(256) void attention_general_f32_kernel(AtArgs p) {
    constexpr int LPK = HD / 4, SLOTS = 256 / LPK;                    // lanes per key (16 / 32), key slots per block (16 / 8)
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* sc = reinterpret_cast<float*>(smem);                       // [Tk] scores, then probabilities
    float* red = sc + (p.Tk + 3) / 4 * 4;                             // [SLOTS][HD] partial contexts
    __shared__ float wred[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int slot = tid / LPK, c = tid % LPK;
    const long row = blockIdx.x;                                       // b * Tq + i
    const int h = blockIdx.y;
    const int b = (int)(row / p.Tq), i = (int)(row - (long)b * p.Tq);
    const int ut = b / p.beams;                                        // the utterance whose K / V table and length this hypothesis reads
    int n = p.lengths ? p.lengths[ut] : p.Tk;
    n = n < 0 ? 0 : (n > p.Tk ? p.Tk : n);
    if (p.causal) { const int lim = i + p.Tk - p.Tq + 1; n = n < lim ? n : (lim < 0 ? 0 : lim); }
    const float* kb = p.k + (long)ut * p.kv_bstride + h * HD + c * 4;
    const float* vb = p.v + (long)ut * p.kv_bstride + h * HD + c * 4;
    float inv = 1.f;
    if (n == 0) {                                                      // block-uniform
        n = p.Tk;
        for (int j = tid; j < n; j += 256) sc[j] = 1.0f / (float)p.Tk;
    } else {
        const f32x4 q4 = *reinterpret_cast<const f32x4*>(p.q + row * p.ldq + h * HD + c * 4);
        for (int j0 = 0; j0 < n; j0 += SLOTS) {                        // block-uniform trip count: the DPP steps below run with every lane active
            const int j = j0 + slot;
            const f32x4 k4 = *reinterpret_cast<const f32x4*>(kb + (long)(j < n ? j : 0) * p.ldk);
            float s = q4[0] * k4[0];
            s = fmaf(q4[1], k4[1], s); s = fmaf(q4[2], k4[2], s); s = fmaf(q4[3], k4[3], s);
            s += dpp_f32<0xB1, 0xF>(0.f, s);                           // the key's lanes: quad, half row, row of 16 [, the neighbouring row]
            s += dpp_f32<0x4E, 0xF>(0.f, s);
            s += dpp_f32<0x141, 0xF>(0.f, s);
            s += dpp_f32<0x140, 0xF>(0.f, s);
            if (LPK == 32) s += __shfl_xor(s, 16, 64);
            if (c == 0 && j < n) sc[j] = s * p.scale;
        }
        __syncthreads();
        float mx = -INFINITY;
        for (int j = tid; j < n; j += 256) mx = fmaxf(mx, sc[j]);
        mx = wave_max(mx);
        if (lane == 0) wred[wave] = mx;
        __syncthreads();
        mx = fmaxf(fmaxf(wred[0], wred[1]), fmaxf(wred[2], wred[3]));
        __syncthreads();
        float sum = 0.f;
        for (int j = tid; j < n; j += 256) { const float e = expf(sc[j] - mx); sc[j] = e; sum += e; }
        sum = wave_sum(sum);
        if (lane == 0) wred[wave] = sum;
        __syncthreads();
        inv = ((wred[0] + wred[1]) + wred[2]) + wred[3];
    }
    __syncthreads();
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int j = slot; j < n; j += SLOTS) {
        const float pr = sc[j] / inv;
        const f32x4 v4 = *reinterpret_cast<const f32x4*>(vb + (long)j * p.ldv);
        acc[0] = fmaf(pr, v4[0], acc[0]); acc[1] = fmaf(pr, v4[1], acc[1]); acc[2] = fmaf(pr, v4[2], acc[2]); acc[3] = fmaf(pr, v4[3], acc[3]);
    }
    *reinterpret_cast<f32x4*>(red + slot * HD + c * 4) = acc;
    __syncthreads();
    if (tid < HD) {
        float o = 0.f;
#pragma unroll
        for (int s = 0; s < SLOTS; ++s) o += red[s * HD + tid];
        p.out[row * p.ldo + h * HD + tid] = o;
    }
}

int attention_general_f32(const AtArgs& a, int B, int hd, hipStream_t st) {
    if (hd != 64 && hd != 128) return MI_ERR_UNSUPPORTED;
    if (a.Tk > AT_MAX_KEYS || (long)B * a.Tq > 0x7fffffffL || a.H > 65535) return MI_ERR_UNSUPPORTED;
    if (!a.q || !a.k || !a.v || !a.out || B <= 0 || a.Tq <= 0 || a.Tk <= 0 || a.H <= 0 || a.beams < 1 || (B % a.beams)) return MI_ERR_ARG;
    if ((a.ldq % 4) || (a.ldk % 4) || (a.ldv % 4) || (a.kv_bstride % 4) || (((uintptr_t)a.q | (uintptr_t)a.k | (uintptr_t)a.v) & 15)) return MI_ERR_ARG;
    const size_t lds = ((size_t)(a.Tk + 3) / 4 * 4 + 256 * 4) * sizeof(float);          // scores + [SLOTS][HD] = 1024 floats for both head sizes
    const dim3 grid((unsigned)((long)B * a.Tq), (unsigned)a.H);
    if (hd == 64) {
        if (!ensure_dynamic_lds<1>((const void*)attention_general_f32_kernel<64>, 64 * 1024)) return MI_ERR_LAUNCH;
        hipLaunchKernelGGL(attention_general_f32_kernel<64>, grid, dim3(256), lds, st, a);
    } else {
        if (!ensure_dynamic_lds<2>((const void*)attention_general_f32_kernel<128>, 64 * 1024)) return MI_ERR_LAUNCH;
        hipLaunchKernelGGL(attention_general_f32_kernel<128>, grid, dim3(256), lds, st, a);
    }
    return MI_OK;
}

// K / V rows of the new tokens -> cache[(b, past + u), :]   (the step above 64 rows, whose QKV linear is mi_gemm_f32)
__global__ __launch_bounds__(256) void kv_append_f32_kernel(const float* __restrict__ qkv, long ldq, float* __restrict__ kc, float* __restrict__ vc,
                                                             int B, int U, int past, int Lmax, int d) {
    const int d4 = d >> 2;
    const long total = (long)B * U * d4;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int c = (int)(i % d4);
        const long m = i / d4;
        const int b = (int)(m / U), u = (int)(m % U);
        const long dst = ((long)b * Lmax + past + u) * d + c * 4;
        *reinterpret_cast<f32x4*>(kc + dst) = *reinterpret_cast<const f32x4*>(qkv + m * ldq + d + c * 4);
        *reinterpret_cast<f32x4*>(vc + dst) = *reinterpret_cast<const f32x4*>(qkv + m * ldq + 2 * d + c * 4);
    }
}

// ------------------------------------------------------------------------------------------------ step driver
constexpr int MAX_LAYERS = 48;

struct Carver {
    char* base; size_t off;
    void* take(size_t bytes) { void* p = base ? base + off : nullptr; off += (bytes + 255) / 256 * 256; return p; }
};
struct StepWs { float *x, *a, *qkv, *ctx, *qq, *m, *hid, *part; size_t part_floats, bytes; };

// Which linears of the step stream their weights (linear_rows_f32_kernel) and which run as mi_gemm_f32's 128 x 128 tiles.  Measured per decoder shape at 1, 5 and 50 rows
// (tools/f32_decode_bench.py; the table is in DESIGN.md §4 'fp32 inference mode'): the rows kernel was 4 to 18 times faster at every one, so up to its 64 rows every
// shape streams and no shape is routed to the tiled GEMM; above 64 rows the rows kernel does not apply.  (The step checks d % 4 == 0, the kernel's one shape condition.)
bool rows_route(int M) { return M <= ROWS_MAXM; }

StepWs carve(const mi_gpt2_config& c, int M, int B, void* base) {
    Carver k{(char*)base, 0};
    StepWs w;
    const size_t d = (size_t)c.d;
    w.x = (float*)k.take((size_t)M * d * 4);
    w.a = (float*)k.take((size_t)M * d * 4);
    w.qkv = (float*)k.take((size_t)M * 3 * d * 4);
    w.ctx = (float*)k.take((size_t)M * d * 4);
    w.qq = (float*)k.take((size_t)M * d * 4);
    w.m = (float*)k.take((size_t)M * 4 * d * 4);
    w.hid = (float*)k.take((size_t)B * d * 4);
    w.part_floats = 0;
    const int shapes[5][3] = {{M, 3 * c.d, c.d}, {M, c.d, c.d}, {M, 4 * c.d, c.d}, {M, c.d, 4 * c.d}, {B, c.V, c.d}};
    for (auto& s : shapes)
        if (rows_route(s[0])) { const size_t f = linear_rows_f32_workspace_floats(s[0], s[1], s[2]); w.part_floats = f > w.part_floats ? f : w.part_floats; }
    w.part = (float*)k.take(w.part_floats * sizeof(float));
    w.bytes = k.off;
    return w;
}

bool step_cfg_ok(const mi_gpt2_config& c) { return c.d > 0 && c.H > 0 && c.L > 0 && c.L <= MAX_LAYERS && c.V > 0 && (c.d % c.H) == 0 && (c.d % 4) == 0; }

#define RUN(expr) do { int rc__ = (expr); if (rc__ != MI_OK) return rc__; } while (0)

}  // namespace

extern "C" size_t mi_linear_rows_f32_workspace_bytes(int M, int N, int K) { return linear_rows_f32_workspace_floats(M, N, K) * sizeof(float); }

extern "C" int mi_linear_rows_f32(const float* x, long ldx, const float* W, long ldw, const float* bias, int act, float* out, long ldo, int accumulate,
                                  float* kcache, float* vcache, int U, int past, int Lmax, int dkv, int M, int N, int K, void* workspace, size_t workspace_bytes,
                                  hipStream_t st) {
    MI_ENTER();
    const int rc = linear_rows_f32(x, ldx, W, ldw, bias, act, out, ldo, accumulate, kcache, vcache, U, past, Lmax, dkv, M, N, K, (float*)workspace,
                                   workspace_bytes / sizeof(float), st);
    if (rc != MI_OK) return rc;
    MI_CHECK_LAUNCH();
    return MI_OK;
}

extern "C" int mi_attention_general_f32(const float* q, long ldq, const float* k, long ldk, const float* v, long ldv, const int* lengths, float* out, long ldo,
                                        int B, int beams, int Tq, int Tk, long kv_bstride, int H, int hd, float scale, int causal, hipStream_t st) {
    MI_ENTER();
    AtArgs a{q, ldq, k, ldk, v, ldv, kv_bstride ? kv_bstride : (long)Tk * ldk, lengths, out, ldo, Tq, Tk, H, beams, causal, scale};
    if (ldk != ldv && !kv_bstride) return MI_ERR_ARG;                 // one batch stride serves both tables
    const int rc = attention_general_f32(a, B, hd, st);
    if (rc != MI_OK) return rc;
    MI_CHECK_LAUNCH();
    return MI_OK;
}

extern "C" size_t mi_decoder_step_f32_workspace_bytes(const mi_gpt2_config* cfg, int B, int U) {
    if (!cfg || !step_cfg_ok(*cfg) || B <= 0 || U <= 0) return 0;
    return carve(*cfg, B * U, B, nullptr).bytes;
}

// weights: [wte (V,d), pos (n_pos,d), lnf_g, lnf_b, lm_head (V,d)] then per layer the 18 pointers of mi_decoder_step_beams, every one fp32 (matrices (out, in)).
// kcache / vcache: L pointers to (B, Lmax, d) fp32; cross_kv: L pointers to (B / beams * T_enc, 2d) fp32 [K | V]; enc_len (B / beams) or null.
// logits (B, ld_logits) fp32 of the LAST new position (+ head_bias).  Appends the new tokens' K / V at rows [past, past + U).
extern "C" int mi_decoder_step_f32(const mi_gpt2_config* cfg, const void* const* weights, const long* ids_new, int B, int beams, int U, int past, int Lmax,
                                   void* const* kcache, void* const* vcache, const void* const* cross_kv, int T_enc, const int* enc_len,
                                   float emb_scale, const float* head_bias, void* workspace, size_t workspace_bytes, float* logits, long ld_logits, hipStream_t st) {
    MI_ENTER();
    if (!cfg) return MI_ERR_ARG;
    const mi_gpt2_config& c = *cfg;
    if (!step_cfg_ok(c) || c.act != 0) return MI_ERR_ARG;              // gelu_new: the GPT-2 block (the Whisper decoder has no fp32 mode)
    const int hd = c.d / c.H;
    if (hd != 64 && hd != 128) return MI_ERR_UNSUPPORTED;
    if (B <= 0 || U <= 0 || past < 0 || past + U > Lmax || beams < 1 || (B % beams) || T_enc <= 0 || ld_logits < c.V) return MI_ERR_ARG;
    if (!weights || !ids_new || !kcache || !vcache || !cross_kv || !workspace || !logits) return MI_ERR_ARG;
    if ((long)B * U > 0x7fffffffL / (4L * c.d) || T_enc > AT_MAX_KEYS || past + U > AT_MAX_KEYS) return MI_ERR_UNSUPPORTED;
    for (int i = 0; i < 5 + 18 * c.L; ++i) if (!weights[i]) return MI_ERR_ARG;
    for (int l = 0; l < c.L; ++l) if (!kcache[l] || !vcache[l] || !cross_kv[l]) return MI_ERR_ARG;
    const int M = B * U, d = c.d;
    StepWs w = carve(c, M, B, workspace);
    if (w.bytes > workspace_bytes) return MI_ERR_ARG;
    const float scale = 1.0f / sqrtf((float)hd);
    auto Gf = [&](int i) { return (const float*)weights[i]; };
    auto Lf = [&](int l, int i) { return (const float*)weights[5 + l * 18 + i]; };
    auto ln = [&](const float* x, long ldx, const float* g, const float* b, float* out, int rows) {
        return mi_layernorm_f32(x, ldx, nullptr, 1, nullptr, 0, g, b, c.eps, out, d, rows, d, st);
    };
    // y = act(in · W^T + bias): plain into `out`, or added to the stream in place; kc / vc: the QKV linear's cache append
    auto lin = [&](const float* in, long ldi, int rows, int K, const float* W, const float* bias, int N, int act, float* out, long ldo, int accumulate, float* kc, float* vc) {
        if (rows_route(rows))
            return linear_rows_f32(in, ldi, W, K, bias, act, out, ldo, accumulate, kc, vc, U, past, Lmax, d, rows, N, K, w.part, w.part_floats, st);
        RUN(mi_gemm_f32(in, ldi, W, K, bias, out, ldo, accumulate ? out : nullptr, ldo, 1.f, act, rows, N, K, st));
        if (kc) {
            const long total = (long)rows * (d / 4);
            hipLaunchKernelGGL(kv_append_f32_kernel, dim3((unsigned)((total + 255) / 256 < 1024 ? (total + 255) / 256 : 1024)), dim3(256), 0, st, out, ldo, kc, vc, B, U, past,
                               Lmax, d);
        }
        return MI_OK;
    };
    RUN(mi_embed_tokens(ids_new, Gf(0), emb_scale, Gf(1), past, U, d, M, c.V, w.x, st));
    for (int l = 0; l < c.L; ++l) {
        float* kc = (float*)kcache[l];
        float* vc = (float*)vcache[l];
        const float* ckv = (const float*)cross_kv[l];
        RUN(ln(w.x, d, Lf(l, 0), Lf(l, 1), w.a, M));
        RUN(lin(w.a, d, M, d, Lf(l, 2), Lf(l, 3), 3 * d, 0, w.qkv, 3 * d, 0, kc, vc));
        RUN(attention_general_f32(AtArgs{w.qkv, 3 * d, kc, d, vc, d, (long)Lmax * d, nullptr, w.ctx, d, U, past + U, c.H, 1, 1, scale}, B, hd, st));
        RUN(lin(w.ctx, d, M, d, Lf(l, 4), Lf(l, 5), d, 0, w.x, d, 1, nullptr, nullptr));
        RUN(ln(w.x, d, Lf(l, 6), Lf(l, 7), w.a, M));
        RUN(lin(w.a, d, M, d, Lf(l, 8), Lf(l, 9), d, 0, w.qq, d, 0, nullptr, nullptr));
        RUN(attention_general_f32(AtArgs{w.qq, d, ckv, 2 * d, ckv + d, 2 * d, (long)T_enc * 2 * d, enc_len, w.ctx, d, U, T_enc, c.H, beams, 0, scale}, B, hd, st));
        RUN(lin(w.ctx, d, M, d, Lf(l, 10), Lf(l, 11), d, 0, w.x, d, 1, nullptr, nullptr));
        RUN(ln(w.x, d, Lf(l, 12), Lf(l, 13), w.a, M));
        RUN(lin(w.a, d, M, d, Lf(l, 14), Lf(l, 15), 4 * d, 2, w.m, 4 * d, 0, nullptr, nullptr));
        RUN(lin(w.m, 4 * d, M, 4 * d, Lf(l, 16), Lf(l, 17), d, 0, w.x, d, 1, nullptr, nullptr));
    }
    // ln_f on the last new position of every sequence (rows b*U + U-1: a strided view), then the head
    RUN(ln(w.x + (size_t)(U - 1) * d, (long)U * d, Gf(2), Gf(3), w.hid, B));
    RUN(lin(w.hid, d, B, d, Gf(4), head_bias, c.V, 0, logits, ld_logits, 0, nullptr, nullptr));
    MI_CHECK_LAUNCH();
    return MI_OK;
}
