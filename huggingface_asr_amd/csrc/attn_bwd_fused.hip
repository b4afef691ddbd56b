// Attention backward with no score-sized tensor in HBM (Whisper encoder training, T' = 1500; DESIGN "Whisper encoder training").
//
// Self-attention on the fused (B*T, 3d) bf16 projection [Q|K|V], head size 64 / 128, optional key lengths (keys j >= lengths[b] masked, as
// attention_qkv does), no relative positions, no probability dropout.  P and dS are recomputed from Q, K and the forward's log-sum-exp
// (log2 domain: P = 2^(q·k scale log2e - lse), the convention of attention.hip) instead of being read back from (H, B, T, Ts) buffers:
//   delta_i = dO_i · O_i                                    (attn_fused_delta_kernel, one f32 per (b, h, i))
//   dS = P (dO V^T - delta) scale
//   dV = P^T dO, dK = dS^T Q       key-stationary walk (attn_fused_dkv_kernel): a wave owns 32 keys and their dK / dV accumulators
//   dQ = dS K                      query-stationary walk (attn_fused_dq_kernel): a wave owns 32 queries and their dQ accumulators
// Every output element is summed by one lane in a fixed order: no atomics, run-to-run bit-identical.
//
// MFMA layout (v_mfma_f32_32x32x16_bf16): A[i][k] from lane i + 32 (k / 8), element k % 8; B[k][j] from lane j + 32 (k / 8); C[i][j] in lane
// j + 32 hi, register r, with i = crow(r, hi) = (r & 3) + 8 (r >> 2) + 4 hi.  S and dP are computed with the walk's OWN index (key in the dK / dV
// walk, query in the dQ walk) on the lane, so registers 8 kb .. 8 kb + 7 of P / dS are directly the A operand of the next product's k-block kb,
// with the contraction index permuted: k-position 16 kb + 8 hi + e <-> row crow(8 kb + e, hi).  The B operand of that product (dO, Q or K of
// the tile, transposed) is staged in LDS in the same permuted order, so one 16-B read gives a lane its eight elements.
#include "common.hpp"

namespace {

struct FusedBwdArgs {
    const bf16_t* q; const bf16_t* k; const bf16_t* v; long ldqkv;      // head h at columns [h hd, (h+1) hd) of each view
    const bf16_t* ctx; long ldo; const bf16_t* dctx; long ldd;
    const float* lse;                                                    // (B, H, T) log2 domain
    const float* delta;                                                  // (B, H, T) workspace (written by the pre-pass)
    const int* lengths;
    bf16_t* dq; bf16_t* dk; bf16_t* dv; long ldg;                        // row views of the dQKV buffer
    int B, T, H;
    float scale;
};

__device__ __forceinline__ int crow(int r, int hi) { return (r & 3) + 8 * (r >> 2) + 4 * hi; }
// position of row q (0..31) in the permuted contraction order: the inverse of (16 kb + 8 hi + e) -> crow(8 kb + e, hi)
__device__ __forceinline__ int perm_pos(int q) {
    const int r = 4 * (q >> 3) + (q & 3), hi = (q >> 2) & 1;
    return 16 * (r >> 3) + 8 * hi + (r & 7);
}

__global__ __launch_bounds__(256) void attn_fused_delta_kernel(FusedBwdArgs p, int hd, float* delta) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;               // (b t, h)
    if (idx >= (long)p.B * p.T * p.H) return;
    const int h = (int)(idx % p.H);
    const long bt = idx / p.H;
    const int b = (int)(bt / p.T), t = (int)(bt % p.T);
    const bf16x8* o = reinterpret_cast<const bf16x8*>(p.ctx + bt * p.ldo + (long)h * hd);
    const bf16x8* g = reinterpret_cast<const bf16x8*>(p.dctx + bt * p.ldd + (long)h * hd);
    float s = 0.f;
    for (int c = 0; c < hd / 8; ++c) {
        const bf16x8 a = o[c], w = g[c];
#pragma unroll
        for (int e = 0; e < 8; ++e) s = fmaf(bf2f(a[e]), bf2f(w[e]), s);
    }
    delta[((long)b * p.H + h) * p.T + t] = s;
}

// stage 32 rows [r0, r0 + 32) of a head's (., HD) operand: row-major into `rm` (row stride HD + 8) and / or transposed in the permuted order into
// `tr` ([HD][40]); rows >= rend are zeros
template <int HD>
__device__ __forceinline__ void stage_tile(const bf16_t* base, long ld, int r0, int rend, bf16_t* rm, bf16_t* tr) {
    constexpr int C8 = HD / 8;
    for (int ch = threadIdx.x; ch < 32 * C8; ch += 256) {
        const int row = ch / C8, c8 = ch % C8;
        bf16x8 x = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
        if (r0 + row < rend) x = *reinterpret_cast<const bf16x8*>(base + (long)(r0 + row) * ld + c8 * 8);
        if (rm) *reinterpret_cast<bf16x8*>(rm + row * (HD + 8) + c8 * 8) = x;
        if (tr) {
            const int pp = perm_pos(row);
#pragma unroll
            for (int e = 0; e < 8; ++e) tr[(c8 * 8 + e) * 40 + pp] = x[e];
        }
    }
}

// one wave's 32 rows [r0, r0 + 32) of an operand as MFMA fragments (row = lane & 31, columns 16 ks + 8 hi + [0, 8)); rows >= rend are zeros
template <int HD>
__device__ __forceinline__ void load_frags(const bf16_t* base, long ld, int r0, int rend, bf16x8 (&f)[HD / 16]) {
    const int lane = threadIdx.x & 63, row = r0 + (lane & 31), hi = lane >> 5;
#pragma unroll
    for (int ks = 0; ks < HD / 16; ++ks)
        f[ks] = row < rend ? *reinterpret_cast<const bf16x8*>(base + (long)row * ld + ks * 16 + hi * 8) : bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
}

// dK, dV: a workgroup = 4 waves = 128 keys of one (b, h); each wave's 32 keys sit on the MFMA lanes, the workgroup walks all queries in tiles of 32
template <int HD>
__global__ __launch_bounds__(256) void attn_fused_dkv_kernel(FusedBwdArgs p) {
    constexpr int KS = HD / 16, NT = HD / 32;
    __shared__ __attribute__((aligned(16))) bf16_t sQ[32 * (HD + 8)];
    __shared__ __attribute__((aligned(16))) bf16_t sO[32 * (HD + 8)];      // dO rows
    __shared__ __attribute__((aligned(16))) bf16_t sQT[HD * 40];
    __shared__ __attribute__((aligned(16))) bf16_t sOT[HD * 40];
    __shared__ float sL[32], sD[32];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, hi = lane >> 5;
    const int h = blockIdx.y, b = blockIdx.z, T = p.T;
    const int len = p.lengths ? min(max(p.lengths[b], 0), T) : T;
    const int k0 = blockIdx.x * 128 + wave * 32;
    const long rb = (long)b * T;
    const bf16_t* qh = p.q + rb * p.ldqkv + h * HD;
    const bf16_t* oh = p.dctx + rb * p.ldd + h * HD;
    const float* lse = p.lse + ((long)b * p.H + h) * T;
    const float* del = p.delta + ((long)b * p.H + h) * T;
    const bool active = k0 < len;                                        // wave-uniform; keys >= len get zero gradients
    const float c2 = p.scale * 1.4426950408889634f;

    bf16x8 kf[KS], vf[KS];
    load_frags<HD>(p.k + rb * p.ldqkv + h * HD, p.ldqkv, k0, len, kf);
    load_frags<HD>(p.v + rb * p.ldqkv + h * HD, p.ldqkv, k0, len, vf);
    f32x16 dK[NT], dV[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int e = 0; e < 16; ++e) { dK[t][e] = 0.f; dV[t][e] = 0.f; }
    const int key = k0 + (lane & 31);
    const bool key_ok = key < len;

    const int nqt = blockIdx.x * 128 < len ? (T + 31) / 32 : 0;     // block-uniform: a workgroup of masked keys only writes its zeros
    for (int qt = 0; qt < nqt; ++qt) {
        const int q0 = qt * 32;
        __syncthreads();                                                 // the previous tile's reads are done
        stage_tile<HD>(qh, p.ldqkv, q0, T, sQ, sQT);
        stage_tile<HD>(oh, p.ldd, q0, T, sO, sOT);
        if (threadIdx.x < 32) {
            const int q = min(q0 + (int)threadIdx.x, T - 1);
            sL[threadIdx.x] = lse[q];
            sD[threadIdx.x] = del[q];
        }
        __syncthreads();
        if (!active) continue;
        f32x16 S, D;
#pragma unroll
        for (int e = 0; e < 16; ++e) { S[e] = 0.f; D[e] = 0.f; }
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const bf16x8 qa = *reinterpret_cast<const bf16x8*>(sQ + (lane & 31) * (HD + 8) + ks * 16 + hi * 8);
            const bf16x8 oa = *reinterpret_cast<const bf16x8*>(sO + (lane & 31) * (HD + 8) + ks * 16 + hi * 8);
            S = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qa, kf[ks], S, 0, 0, 0);
            D = __builtin_amdgcn_mfma_f32_32x32x16_bf16(oa, vf[ks], D, 0, 0, 0);
        }
        bf16x8 pa[2], da[2];
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int qi = crow(e, hi);
            const bool ok = key_ok && q0 + qi < T;
            const float pr = ok ? __builtin_amdgcn_exp2f(S[e] * c2 - sL[qi]) : 0.f;
            const float ds = ok ? pr * (D[e] - sD[qi]) * p.scale : 0.f;
            pa[e >> 3][e & 7] = f2bf(pr);
            da[e >> 3][e & 7] = f2bf(ds);
        }
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const int n = t * 32 + (lane & 31);
                const bf16x8 ob = *reinterpret_cast<const bf16x8*>(sOT + n * 40 + kb * 16 + hi * 8);
                const bf16x8 qb = *reinterpret_cast<const bf16x8*>(sQT + n * 40 + kb * 16 + hi * 8);
                dV[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(pa[kb], ob, dV[t], 0, 0, 0);
                dK[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(da[kb], qb, dK[t], 0, 0, 0);
            }
    }
    // C[key = crow(r, hi)][column = 32 t + lane & 31]: 32 lanes store one row's 64 consecutive bytes
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int kr = k0 + crow(e, hi);
            if (kr >= T) continue;
            const long o = (rb + kr) * p.ldg + h * HD + t * 32 + (lane & 31);
            p.dk[o] = f2bf(dK[t][e]);
            p.dv[o] = f2bf(dV[t][e]);
        }
}

// dQ: a workgroup = 4 waves = 128 queries of one (b, h); each wave's 32 queries sit on the MFMA lanes, the workgroup walks the valid keys in tiles of 32
template <int HD>
__global__ __launch_bounds__(256) void attn_fused_dq_kernel(FusedBwdArgs p) {
    constexpr int KS = HD / 16, NT = HD / 32;
    __shared__ __attribute__((aligned(16))) bf16_t sK[32 * (HD + 8)];
    __shared__ __attribute__((aligned(16))) bf16_t sV[32 * (HD + 8)];
    __shared__ __attribute__((aligned(16))) bf16_t sKT[HD * 40];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, hi = lane >> 5;
    const int h = blockIdx.y, b = blockIdx.z, T = p.T;
    const int len = p.lengths ? min(max(p.lengths[b], 0), T) : T;
    const int q0 = blockIdx.x * 128 + wave * 32;
    const long rb = (long)b * T;
    const bool active = q0 < T;
    const float c2 = p.scale * 1.4426950408889634f;

    bf16x8 qf[KS], of[KS];
    load_frags<HD>(p.q + rb * p.ldqkv + h * HD, p.ldqkv, q0, T, qf);
    load_frags<HD>(p.dctx + rb * p.ldd + h * HD, p.ldd, q0, T, of);
    const int qi = min(q0 + (lane & 31), T - 1);
    const float lse2 = p.lse[((long)b * p.H + h) * T + qi];
    const float dl = p.delta[((long)b * p.H + h) * T + qi];
    const bool q_ok = q0 + (lane & 31) < T;
    f32x16 dQ[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int e = 0; e < 16; ++e) dQ[t][e] = 0.f;

    const int nkt = (len + 31) / 32;
    for (int kt = 0; kt < nkt; ++kt) {
        const int j0 = kt * 32;
        __syncthreads();
        stage_tile<HD>(p.k + rb * p.ldqkv + h * HD, p.ldqkv, j0, len, sK, sKT);
        stage_tile<HD>(p.v + rb * p.ldqkv + h * HD, p.ldqkv, j0, len, sV, nullptr);
        __syncthreads();
        if (!active) continue;
        f32x16 S, D;
#pragma unroll
        for (int e = 0; e < 16; ++e) { S[e] = 0.f; D[e] = 0.f; }
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const bf16x8 ka = *reinterpret_cast<const bf16x8*>(sK + (lane & 31) * (HD + 8) + ks * 16 + hi * 8);
            const bf16x8 va = *reinterpret_cast<const bf16x8*>(sV + (lane & 31) * (HD + 8) + ks * 16 + hi * 8);
            S = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ka, qf[ks], S, 0, 0, 0);        // S^T[key][query]
            D = __builtin_amdgcn_mfma_f32_32x32x16_bf16(va, of[ks], D, 0, 0, 0);
        }
        bf16x8 da[2];
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const bool ok = q_ok && j0 + crow(e, hi) < len;
            const float pr = ok ? __builtin_amdgcn_exp2f(S[e] * c2 - lse2) : 0.f;
            da[e >> 3][e & 7] = f2bf(ok ? pr * (D[e] - dl) * p.scale : 0.f);
        }
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const bf16x8 kb8 = *reinterpret_cast<const bf16x8*>(sKT + (t * 32 + (lane & 31)) * 40 + kb * 16 + hi * 8);
                dQ[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(da[kb], kb8, dQ[t], 0, 0, 0);
            }
    }
    if (!active) return;
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int qr = q0 + crow(e, hi);
            if (qr >= T) continue;
            p.dq[(rb + qr) * p.ldg + h * HD + t * 32 + (lane & 31)] = f2bf(dQ[t][e]);
        }
}

template <int HD>
int launch_fused_bwd(const FusedBwdArgs& a, hipStream_t st) {
    const dim3 grid(cdiv(a.T, 128), a.H, a.B);
    hipLaunchKernelGGL(attn_fused_dkv_kernel<HD>, grid, dim3(256), 0, st, a);
    MI_CHECK_LAUNCH();
    hipLaunchKernelGGL(attn_fused_dq_kernel<HD>, grid, dim3(256), 0, st, a);
    MI_CHECK_LAUNCH();
    return MI_OK;
}

}  // namespace

// q / k / v: head h at columns [h hd, (h+1) hd) of (B*T, ldqkv) row views (the fused projection); ctx / dctx (B*T, ld) bf16; lse (B, H, T) from
// mi_attention_qkv_lse_bf16 (no positions, no dropout); dq / dk / dv: row views of a (B*T, ldg) bf16 buffer, every row < T of every head written.
// workspace: >= B T H * 4 bytes (the delta rows).
extern "C" int mi_attention_qkv_bwd_fused(const void* q, const void* k, const void* v, long ldqkv, const int* lengths,
                                          const void* ctx, long ldo, const void* dctx, long ldd, const float* lse,
                                          void* dq, void* dk, void* dv, long ldg, void* workspace, size_t ws_bytes,
                                          int B, int T, int H, int hd, float scale, hipStream_t st) {
    MI_ENTER();
    if (B <= 0 || T <= 0 || H <= 0 || !q || !k || !v || !ctx || !dctx || !lse || !dq || !dk || !dv || !workspace) return MI_ERR_ARG;
    if (hd != 64 && hd != 128) return MI_ERR_UNSUPPORTED;
    if (ws_bytes < (size_t)B * T * H * sizeof(float)) return MI_ERR_ARG;
    if ((ldqkv % 8) || (ldo % 8) || (ldd % 8) || ldg <= 0 || ldqkv < (long)H * hd || ldo < (long)H * hd || ldd < (long)H * hd || ldg < (long)H * hd) return MI_ERR_ARG;
    if (((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)ctx | (uintptr_t)dctx) & 15) return MI_ERR_ARG;
    FusedBwdArgs a{(const bf16_t*)q, (const bf16_t*)k, (const bf16_t*)v, ldqkv, (const bf16_t*)ctx, ldo, (const bf16_t*)dctx, ldd, lse,
                   (const float*)workspace, lengths, (bf16_t*)dq, (bf16_t*)dk, (bf16_t*)dv, ldg, B, T, H, scale};
    hipLaunchKernelGGL(attn_fused_delta_kernel, dim3(cdiv((long)B * T * H, 256)), dim3(256), 0, st, a, hd, (float*)workspace);
    MI_CHECK_LAUNCH();
    return hd == 64 ? launch_fused_bwd<64>(a, st) : launch_fused_bwd<128>(a, st);
}
