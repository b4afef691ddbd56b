// Mixing fine-tuning of the DeCRED decoder (reference src/models/decoders/multi_head_gpt2_mixing.py:111-131, modes `scalar` and `linear`; model_utils.py:205-217 freezes
// everything but `lm_mixing`): from the H per-head fp32 logit matrices L_h (M, ld) of the existing head GEMMs and the mixing parameter,
//   z[r, v] = sum_h mix[h, v] L_h[r, v]          (scalar: mix[h] for every v)
//   loss    = mean over the rows with a target of  lse_v(z[r, :]) - z[r, target_r]        (unsmoothed, labels shifted by one, ignore index < 0)
//   dmix[h, v] = sum_r dz[r, v] L_h[r, v],  dz = (softmax(z[r, :]) - onehot(target_r)) / N_valid       (scalar: summed over v as well)
// Neither z nor dz exists at full size: both kernels rebuild z[r, v] from the H logits they read anyway.  Only columns [0, V) enter the log-sum-exp; the padding columns
// [V, ld) are never read.  No float atomics: the forward sums the row losses in one block (a strided walk per thread, a fixed tree); the backward reduces rows in fixed chunks of MIX_ROWS (one
// partial (H, V) per chunk, a thread per column walking its chunk's rows in order), a second pass adds the partials in chunk order, and the scalar mode's sum over v is
// a strided walk plus a fixed tree — two runs give the same bits.
#include "common.hpp"
#include "../../include/hfasr_hip.h"

namespace {
constexpr int MIX_MAXH = 8, MIX_ROWS = 64, MIX_COLS = 256;

struct MixArgs {
    const float* lg; long ld, hs;          // head h, row r, column v at lg[h * hs + r * ld + v]
    const float* mix; int per_col;         // (H, V) when per_col, else (H)
    const long* labels; int B, U, V, H;
};

__device__ __forceinline__ long mix_target(const MixArgs& p, int r) {      // row r = b U + u predicts labels[b, u + 1]; the last position of a sequence has no target
    const int u = r % p.U;
    return u + 1 < p.U ? p.labels[r + 1] : -1;
}

__device__ __forceinline__ float mix_z(const MixArgs& p, const float* mh, int r, int v) {
    float z = 0.f;
    for (int h = 0; h < p.H; ++h) z = fmaf(p.per_col ? p.mix[(long)h * p.V + v] : mh[h], p.lg[(long)h * p.hs + (long)r * p.ld + v], z);
    return z;
}

// one wave per row: lse[r] and the row's loss (NaN: no target)
__global__ __launch_bounds__(256) void mix_ce_rows_kernel(MixArgs p, float* __restrict__ lse, float* __restrict__ row_loss, int M) {
    const int lane = threadIdx.x & 63, r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= M) return;                                                // wave-uniform
    float mh[MIX_MAXH];
    for (int h = 0; h < MIX_MAXH; ++h) mh[h] = (!p.per_col && h < p.H) ? p.mix[h] : 0.f;
    float mx = -INFINITY, s = 0.f;
    for (int v = lane; v < p.V; v += 64) {
        const float z = mix_z(p, mh, r, v);
        if (z > mx) { s = s * __expf(mx - z); mx = z; }
        s += __expf(z - mx);
    }
    const float gm = wave_max(mx);
    s = wave_sum(mx == -INFINITY ? 0.f : s * __expf(mx - gm));
    const float l = gm + __logf(s);
    if (lane == 0) {
        lse[r] = l;
        const long t = mix_target(p, r);
        row_loss[r] = (t >= 0 && t < p.V) ? l - mix_z(p, mh, r, (int)t) : __builtin_nanf("");
    }
}

// acc[0] = sum of the rows' losses, acc[1] = their count (one block: a strided walk per thread, then a fixed tree)
__global__ __launch_bounds__(256) void mix_ce_sum_kernel(const float* __restrict__ row_loss, int M, float* __restrict__ acc) {
    __shared__ float ss[256], sc[256];
    float s = 0.f, c = 0.f;
    for (int r = threadIdx.x; r < M; r += 256) { const float v = row_loss[r]; if (v == v) { s += v; c += 1.f; } }
    ss[threadIdx.x] = s; sc[threadIdx.x] = c;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (threadIdx.x < w) { ss[threadIdx.x] += ss[threadIdx.x + w]; sc[threadIdx.x] += sc[threadIdx.x + w]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) { acc[0] = ss[0]; acc[1] = sc[0]; }
}

// block (column tile, row chunk): thread = one column, the chunk's rows in order -> part[chunk][h][v]
__global__ __launch_bounds__(MIX_COLS) void mix_ce_bwd_kernel(MixArgs p, const float* __restrict__ lse, const float* __restrict__ acc, float* __restrict__ part, int M) {
    const int v = blockIdx.x * MIX_COLS + threadIdx.x;
    if (v >= p.V) return;
    float mh[MIX_MAXH], g[MIX_MAXH];
    for (int h = 0; h < MIX_MAXH; ++h) { mh[h] = (!p.per_col && h < p.H) ? p.mix[h] : 0.f; g[h] = 0.f; }
    const float inv = 1.f / acc[1];
    const int r0 = blockIdx.y * MIX_ROWS, r1 = r0 + MIX_ROWS < M ? r0 + MIX_ROWS : M;
    for (int r = r0; r < r1; ++r) {
        const long t = mix_target(p, r);
        if (t < 0 || t >= p.V) continue;                               // block-uniform
        const float dz = (__expf(mix_z(p, mh, r, v) - lse[r]) - (v == (int)t ? 1.f : 0.f)) * inv;
        for (int h = 0; h < p.H; ++h) g[h] = fmaf(dz, p.lg[(long)h * p.hs + (long)r * p.ld + v], g[h]);
    }
    for (int h = 0; h < p.H; ++h) part[((long)blockIdx.y * p.H + h) * p.V + v] = g[h];
}

// the chunks' partials in chunk order -> out[h][v]
__global__ __launch_bounds__(256) void mix_ce_chunks_kernel(const float* __restrict__ part, int chunks, long HV, float* __restrict__ out) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= HV) return;
    float s = part[i];
    for (int c = 1; c < chunks; ++c) s += part[(long)c * HV + i];
    out[i] = s;
}

// scalar mode: dmix[h] = sum_v lin[h][v] — a block per head, a strided walk per thread, a fixed tree
__global__ __launch_bounds__(256) void mix_ce_sumv_kernel(const float* __restrict__ lin, int V, float* __restrict__ out) {
    __shared__ float ss[256];
    float s = 0.f;
    for (int v = threadIdx.x; v < V; v += 256) s += lin[(long)blockIdx.x * V + v];
    ss[threadIdx.x] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (threadIdx.x < w) ss[threadIdx.x] += ss[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[blockIdx.x] = ss[0];
}

bool mix_args_ok(const MixArgs& p) {
    return p.lg && p.mix && p.labels && p.B > 0 && p.U > 1 && p.V > 0 && p.H >= 1 && p.H <= MIX_MAXH && p.ld >= p.V && p.hs >= (long)p.B * p.U * p.ld;
}
}  // namespace

extern "C" int mi_mix_ce_fwd(const float* logits, long ld, long head_stride, int H, const float* mix, int mix_per_col, const long* labels, int B, int U, int V,
                             float* lse, float* row_loss, float* acc, hipStream_t st) {
    MI_ENTER();
    const MixArgs p{logits, ld, head_stride, mix, mix_per_col, labels, B, U, V, H};
    if (!mix_args_ok(p) || !lse || !row_loss || !acc) return MI_ERR_ARG;
    const int M = B * U;
    hipLaunchKernelGGL(mix_ce_rows_kernel, dim3(cdiv(M, 4)), dim3(256), 0, st, p, lse, row_loss, M);
    hipLaunchKernelGGL(mix_ce_sum_kernel, dim3(1), dim3(256), 0, st, row_loss, M, acc);
    MI_CHECK_LAUNCH();
    return MI_OK;
}

// workspace of mi_mix_ce_bwd in floats: the chunks' partials, and the (H, V) sums the scalar mode reduces further
extern "C" size_t mi_mix_ce_bwd_workspace_floats(int M, int H, int V) { return ((size_t)cdiv(M, MIX_ROWS) + 1) * H * V; }

// lse, acc: what mi_mix_ce_fwd left for the same inputs.  dmix: (H, V) fp32 when mix_per_col, else (H)
extern "C" int mi_mix_ce_bwd(const float* logits, long ld, long head_stride, int H, const float* mix, int mix_per_col, const long* labels, int B, int U, int V,
                             const float* lse, const float* acc, float* workspace, size_t workspace_floats, float* dmix, hipStream_t st) {
    MI_ENTER();
    const MixArgs p{logits, ld, head_stride, mix, mix_per_col, labels, B, U, V, H};
    const int M = B * U, chunks = cdiv(M, MIX_ROWS);
    if (!mix_args_ok(p) || !lse || !acc || !workspace || !dmix || workspace_floats < mi_mix_ce_bwd_workspace_floats(M, H, V)) return MI_ERR_ARG;
    const long HV = (long)H * V;
    float* lin = mix_per_col ? dmix : workspace + (size_t)chunks * HV;
    hipLaunchKernelGGL(mix_ce_bwd_kernel, dim3(cdiv(V, MIX_COLS), chunks), dim3(MIX_COLS), 0, st, p, lse, acc, workspace, M);
    hipLaunchKernelGGL(mix_ce_chunks_kernel, dim3((unsigned)((HV + 255) / 256)), dim3(256), 0, st, workspace, chunks, HV, lin);
    if (!mix_per_col) hipLaunchKernelGGL(mix_ce_sumv_kernel, dim3(H), dim3(256), 0, st, lin, V, dmix);
    MI_CHECK_LAUNCH();
    return MI_OK;
}
