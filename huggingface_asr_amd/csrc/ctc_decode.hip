// CTC greedy transcription on gfx950: per-frame argmax over the classes, then the collapse (merge repeats, drop blanks) into padded token ids.
//
// Reference: ctc_greedy_decode (src/utilities/eval_utils.py:37-43, called from src/trainers/train_ctc_asr.py:77-85 with blank = len(vocab), the LAST class of
// e_branchformer.py:456-457): torch.argmax, then a Python groupby over the elements of a device tensor.  Here: one pass over the logits (row_argmax_kernel; the CTC
// engine needs not even that, its head GEMM leaves the argmax — mi_gemm_argmax_bf16) and one block per utterance for the collapse.  No atomics: the outputs are a
// deterministic function of the inputs.
#include "common.hpp"
#include "../../include/hfasr_hip.h"

namespace {

template <typename T> struct Vec16;
template <> struct Vec16<float> { typedef f32x4 type; static constexpr int N = 4; };
template <> struct Vec16<bf16_t> { typedef bf16x8 type; static constexpr int N = 8; };

// One wave per row, 4 rows per block; row m = (b, t) = (m / T, m % T) starts at x + b * ld_b + t * ld_t.  Whole 16-B vectors of the row where the row is 16-B aligned
// (four in flight per lane), the remaining columns one by one; every candidate is folded as a key of the shared order (common.hpp argmax_*).
template <typename T>
__global__ __launch_bounds__(256) void row_argmax_kernel(const T* __restrict__ x, long ld_t, long ld_b, int Tn, int V, int* __restrict__ best, int M) {
    typedef typename Vec16<T>::type vec_t;
    constexpr int VN = Vec16<T>::N;
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    const T* xr = x + (long)(row / Tn) * ld_b + (long)(row % Tn) * ld_t;
    amax_t k = ARGMAX_EMPTY;
    int done = 0;                                                   // columns covered by the vector loop
    if ((reinterpret_cast<uintptr_t>(xr) & 15) == 0) {
        const int nvec = V / VN;
        const vec_t* xv = reinterpret_cast<const vec_t*>(xr);
        int q = lane;
        for (; q + 3 * 64 < nvec; q += 4 * 64) {
            vec_t v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = xv[q + 64 * u];
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int e = 0; e < VN; ++e) k = argmax_max(k, argmax_key((float)v[u][e], (q + 64 * u) * VN + e));
        }
        for (; q < nvec; q += 64) {
            const vec_t v = xv[q];
#pragma unroll
            for (int e = 0; e < VN; ++e) k = argmax_max(k, argmax_key((float)v[e], q * VN + e));
        }
        done = nvec * VN;
    }
    for (int c = done + lane; c < V; c += 64) k = argmax_max(k, argmax_key((float)xr[c], c));
    const int w = wave_argmax(k);
    if (lane == 0) best[row] = w;
}

// One block (256 threads) per utterance.  Frame t is kept iff t < n, best[t] != blank and (t == 0 or best[t] != best[t - 1]); the kept ids go to tokens[0..count) in
// order, their frame indices to frames[0..count), the rest of both rows is pad_id / -1.  The block walks chunks of 1024 frames (four consecutive frames per thread):
// keep flags, a block-wide exclusive prefix sum (DPP-free shuffles inside a wave, the four wave totals through LDS), scatter; the count is carried from chunk to chunk,
// the id in front of a chunk is read back from `best` like any other predecessor.
constexpr int CC_ITEMS = 4, CC_CHUNK = 256 * CC_ITEMS;
template <typename TOK>
__global__ __launch_bounds__(256) void ctc_collapse_kernel(const int* __restrict__ best, int Tn, const int* __restrict__ lengths, int blank, long pad_id,
                                                           TOK* __restrict__ tokens, int* __restrict__ n_tokens, int* __restrict__ frames) {
    __shared__ int wtot[2][4];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int* bb = best + (long)b * Tn;
    TOK* tk = tokens + (long)b * Tn;
    int* fr = frames ? frames + (long)b * Tn : nullptr;
    const int n = lengths ? min(max(lengths[b], 0), Tn) : Tn;
    int count = 0, par = 0;
    for (int base = 0; base < n; base += CC_CHUNK, par ^= 1) {
        const int t0 = base + tid * CC_ITEMS;
        int id[CC_ITEMS];
        bool keep[CC_ITEMS];
        int prev = (t0 > 0 && t0 < n) ? bb[t0 - 1] : -1;
        int mine = 0;
#pragma unroll
        for (int e = 0; e < CC_ITEMS; ++e) {
            const int t = t0 + e;
            id[e] = t < n ? bb[t] : blank;
            keep[e] = t < n && id[e] != blank && (t == 0 || id[e] != prev);
            prev = id[e];
            mine += keep[e] ? 1 : 0;
        }
        int inc = mine;                                             // inclusive prefix sum over the wave
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int up = __shfl_up(inc, o, 64);
            if (lane >= o) inc += up;
        }
        if (lane == 63) wtot[par][wave] = inc;
        __syncthreads();                                            // (the other parity's totals are rewritten only after every wave has passed this barrier once more)
        int off = count + inc - mine;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const int tw = wtot[par][w];
            off += w < wave ? tw : 0;
            count += tw;
        }
#pragma unroll
        for (int e = 0; e < CC_ITEMS; ++e)
            if (keep[e]) {
                tk[off] = (TOK)id[e];
                if (fr) fr[off] = t0 + e;
                ++off;
            }
    }
    for (int t = count + tid; t < Tn; t += 256) {
        tk[t] = (TOK)pad_id;
        if (fr) fr[t] = -1;
    }
    if (tid == 0) n_tokens[b] = count;
}

int row_argmax_launch(const void* x, long ld_t, long ld_b, int Tn, int dtype, int V, int* best, int M, hipStream_t stream) {
    if (!x || !best || M <= 0 || V <= 0 || Tn <= 0) return MI_ERR_ARG;
    dim3 grid(cdiv(M, 4)), block(256);
    if (dtype == 0) hipLaunchKernelGGL(row_argmax_kernel<float>, grid, block, 0, stream, (const float*)x, ld_t, ld_b, Tn, V, best, M);
    else if (dtype == 1) hipLaunchKernelGGL(row_argmax_kernel<bf16_t>, grid, block, 0, stream, (const bf16_t*)x, ld_t, ld_b, Tn, V, best, M);
    else return MI_ERR_ARG;
    MI_CHECK_LAUNCH();
    return MI_OK;
}

}  // namespace

// best (M) int32 = argmax over the V1 columns of row m of x (row stride ld elements; dtype 0 fp32 / 1 bf16), torch.argmax's rules
extern "C" int mi_row_argmax(const void* x, long ld, int dtype, int V1, int* best, int M, hipStream_t stream) {
    MI_ENTER();
    return row_argmax_launch(x, ld, 0, M > 0 ? M : 1, dtype, V1, best, M, stream);
}

// best (B, T) int32 -> tokens (B, T) int32 (tokens_dtype 0) / int64 (1), n_tokens (B) int32, frames (B, T) int32 or null; lengths (B) int32 or null (every frame counts)
extern "C" int mi_ctc_collapse(const int* best, int B, int T, const int* lengths, int blank, long pad_id, void* tokens, int tokens_dtype, int* n_tokens, int* frames,
                               hipStream_t stream) {
    MI_ENTER();
    if (!best || !tokens || !n_tokens || B <= 0 || T <= 0) return MI_ERR_ARG;
    if ((const void*)best == (const void*)tokens) return MI_ERR_ARG;
    if (tokens_dtype == 0) hipLaunchKernelGGL(ctc_collapse_kernel<int>, dim3(B), dim3(256), 0, stream, best, T, lengths, blank, pad_id, (int*)tokens, n_tokens, frames);
    else if (tokens_dtype == 1) hipLaunchKernelGGL(ctc_collapse_kernel<long>, dim3(B), dim3(256), 0, stream, best, T, lengths, blank, pad_id, (long*)tokens, n_tokens, frames);
    else return MI_ERR_ARG;
    MI_CHECK_LAUNCH();
    return MI_OK;
}

// the two above over logits (B, T, V1) with element strides (ld_batch, ld_row); best (B, T) int32 is the caller's scratch (and a result: the per-frame classes)
extern "C" int mi_ctc_greedy(const void* logits, long ld_row, long ld_batch, int dtype, int B, int T, int V1, const int* lengths, int blank, long pad_id,
                             int* best, void* tokens, int tokens_dtype, int* n_tokens, int* frames, hipStream_t stream) {
    MI_ENTER();
    if (B <= 0 || T <= 0) return MI_ERR_ARG;
    const int rc = row_argmax_launch(logits, ld_row, ld_batch, T, dtype, V1, best, B * T, stream);
    if (rc != MI_OK) return rc;
    return mi_ctc_collapse(best, B, T, lengths, blank, pad_id, tokens, tokens_dtype, n_tokens, frames, stream);
}
