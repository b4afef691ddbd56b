// Two-pass joint decoding ("attention rescoring") on gfx950: the three small kernels around the teacher-forced decoder pass that scores a CTC n-best.
//
//   mi_rescore_pack    the n-best of the CTC prefix beam search (tokens, n_tokens, scores) -> the decoder's operands: ids = [start, t_0 .. t_{k-1}, pad ..],
//                      labels = [t_0 .. t_{k-1}, eos, -100 ..], len = k + 1; a hypothesis that does not exist (non-finite CTC score, k outside [0, U - 1] or past its
//                      token row, a token outside [0, V)) becomes ids = [start, pad ..], labels = -100, len = 0.  One block per hypothesis.
//   mi_rows_nll_f32    nll[m] = lse[m] - x[m, labels[m]] for the routes that materialise logits; exactly 0 for labels[m] < 0 (and for a label >= V, which
//                      mi_gemm_ce_f32 ignores as well).
//   mi_rescore_select  one block per utterance, N <= 64 hypotheses: att[n] = -(((nll[0] + nll[1]) + nll[2]) ...) over u < len[n] in ascending order,
//                      total[n] = (w_ctc * ctc[n] + w_att * att[n]) / denom[len[n]] — every multiply, the add and the divide rounded once (no FMA contraction: the
//                      kernel is compiled with fp contraction off), so a float32 restatement reproduces the bits (tests/rescore_ref.py select32).  len = 0 and NaN totals count as -inf;
//                      order: descending total, equal totals by lower n (each hypothesis counts the ones in front of it: a rank, no sort).  The best K are gathered,
//                      best first.  The joint beam search's objective at a closed hypothesis (decoder.py `generate`): at EOS the prefix scorer's value is the
//                      full-sequence CTC probability, denom[l] = l ** length_penalty is the host's table (decoder._step_denoms), so there is no pow on the device.
//
// This pass has no counterpart in the reference.  No atomics, fixed summation order: bit-identical run to run.  No per-thread arrays: no scratch.
#include "common.hpp"
#include "../../include/hfasr_hip.h"

namespace {

constexpr int RS_MAXN = 64;

template <typename TOK>
__global__ __launch_bounds__(256) void rescore_pack_kernel(const TOK* __restrict__ tokens, const int* __restrict__ n_tokens, const float* __restrict__ ctc, int Tt, int V,
                                                           int U, long start, long eos, long pad, long* __restrict__ ids, long* __restrict__ labels,
                                                           int* __restrict__ len) {
    const int r = blockIdx.x, tid = threadIdx.x;
    const TOK* tk = tokens + (long)r * Tt;
    const int k = n_tokens[r];
    const float c = ctc[r];
    int bad = !(fabsf(c) < INFINITY) || k < 0 || k > U - 1 || k > Tt;            // (a NaN score fails the comparison too)
    if (!bad)
        for (int u = tid; u < k; u += 256) {
            const long t = (long)tk[u];
            bad |= (t < 0 || t >= (long)V) ? 1 : 0;
        }
    bad = __syncthreads_or(bad);
    long* ir = ids + (long)r * U;
    long* lr = labels + (long)r * U;
    const int kk = bad ? -1 : k;                                                 // tokens that are copied; the label row closes with eos at position kk
    for (int u = tid; u < U; u += 256) {
        ir[u] = u == 0 ? start : (u <= kk ? (long)tk[u - 1] : pad);
        lr[u] = u < kk ? (long)tk[u] : (u == kk ? eos : -100L);
    }
    if (tid == 0) len[r] = bad ? 0 : k + 1;
}

__global__ __launch_bounds__(256) void rows_nll_kernel(const float* __restrict__ x, long ld, const float* __restrict__ lse, const long* __restrict__ labels, int V,
                                                       float* __restrict__ nll, int M) {
    const int m = blockIdx.x * 256 + threadIdx.x;
    if (m >= M) return;
    const long t = labels[m];
    nll[m] = (t < 0 || t >= (long)V) ? 0.f : lse[m] - x[(long)m * ld + t];
}

template <typename TOK>
__global__ __launch_bounds__(256) void rescore_select_kernel(const float* __restrict__ nll, const int* __restrict__ len, const float* __restrict__ ctc,
                                                             const float* __restrict__ denom, float w_ctc, float w_att, int N, int U, int K,
                                                             const TOK* __restrict__ tokens, int Tt, const int* __restrict__ frames, long eos, long pad,
                                                             int* __restrict__ order, float* __restrict__ total, float* __restrict__ att, float* __restrict__ ctc_out,
                                                             float* __restrict__ token_lp, long* __restrict__ out_tokens, int* __restrict__ out_n,
                                                             int* __restrict__ out_frames) {
#pragma clang fp contract(off)                                                   // every product and sum below is rounded on its own
    __shared__ float tot_s[RS_MAXN];
    __shared__ int ord_s[RS_MAXN], len_s[RS_MAXN];
    const int b = blockIdx.x, tid = threadIdx.x;
    float my_tot = -INFINITY, my_att = 0.f, my_ctc = 0.f;
    int my_len = 0;
    if (tid < N) {
        const long r = (long)b * N + tid;
        int l = len[r];
        l = (l < 0 || l > U || l - 1 > Tt) ? 0 : l;
        my_len = l;
        my_ctc = ctc[r];
        if (l > 0) {
            const float* p = nll + r * U;
            float s = p[0];
            for (int u = 1; u < l; ++u) s = s + p[u];
            my_att = -s;
            const float pc = w_ctc * my_ctc, pa = w_att * my_att;
            const float t = __fdiv_rn(pc + pa, denom[l]);
            my_tot = t != t ? -INFINITY : t;
        }
        tot_s[tid] = my_tot;
        len_s[tid] = my_len;
    }
    __syncthreads();
    if (tid < N) {
        int rank = 0;
        for (int m = 0; m < N; ++m) {
            const float o = tot_s[m];
            rank += (o > my_tot || (o == my_tot && m < tid)) ? 1 : 0;
        }
        if (rank < K) {
            const long o = (long)b * K + rank;
            ord_s[rank] = tid;
            order[o] = tid;
            total[o] = my_tot;
            att[o] = my_att;
            ctc_out[o] = my_ctc;
            out_n[o] = my_len > 0 ? my_len - 1 : 0;
        }
    }
    __syncthreads();
    for (int i = tid; i < K * U; i += 256) {
        const int k = i / U, u = i - k * U;
        const int n = ord_s[k], l = len_s[n], nt = l > 0 ? l - 1 : 0;           // a hypothesis that does not exist: no tokens, the closing eos
        const long r = (long)b * N + n, o = ((long)b * K + k) * U + u;
        token_lp[o] = u < l ? -nll[r * U + u] : 0.f;
        out_tokens[o] = u < nt ? (long)tokens[r * Tt + u] : (u == nt ? eos : pad);
        if (out_frames) out_frames[o] = u < nt ? frames[r * Tt + u] : -1;
    }
}

}  // namespace

extern "C" int mi_rescore_pack(const void* tokens, int tokens_dtype, const int* n_tokens, const float* ctc, int B, int N, int Tt, int V, int U, long start, long eos,
                               long pad, long* ids, long* labels, int* len, hipStream_t stream) {
    MI_ENTER();
    if (!tokens || !n_tokens || !ctc || !ids || !labels || !len) return MI_ERR_ARG;
    if (B < 1 || N < 1 || Tt < 1 || V < 1 || U < 1 || (long)B * N > 0x7FFFFFFFL) return MI_ERR_ARG;
    const dim3 grid((unsigned)(B * N)), block(256);
    if (tokens_dtype == 0) hipLaunchKernelGGL(rescore_pack_kernel<int>, grid, block, 0, stream, (const int*)tokens, n_tokens, ctc, Tt, V, U, start, eos, pad, ids, labels, len);
    else if (tokens_dtype == 1) hipLaunchKernelGGL(rescore_pack_kernel<long>, grid, block, 0, stream, (const long*)tokens, n_tokens, ctc, Tt, V, U, start, eos, pad, ids, labels, len);
    else return MI_ERR_ARG;
    MI_CHECK_LAUNCH();
    return MI_OK;
}

extern "C" int mi_rows_nll_f32(const float* x, long ld, const float* lse, const long* labels, int V, float* nll, int M, hipStream_t stream) {
    MI_ENTER();
    if (!x || !lse || !labels || !nll || M < 1 || V < 1 || ld < V) return MI_ERR_ARG;
    hipLaunchKernelGGL(rows_nll_kernel, dim3((unsigned)cdiv(M, 256)), dim3(256), 0, stream, x, ld, lse, labels, V, nll, M);
    MI_CHECK_LAUNCH();
    return MI_OK;
}

extern "C" int mi_rescore_select(const float* nll, const int* len, const float* ctc, const float* denom, float w_ctc, float w_att, int B, int N, int U, int K,
                                 const void* tokens, int tokens_dtype, int Tt, const int* frames, long eos, long pad, int* order, float* total, float* att,
                                 float* ctc_out, float* token_lp, long* out_tokens, int* out_n, int* out_frames, hipStream_t stream) {
    MI_ENTER();
    if (!nll || !len || !ctc || !denom || !tokens || !order || !total || !att || !ctc_out || !token_lp || !out_tokens || !out_n) return MI_ERR_ARG;
    if ((frames == nullptr) != (out_frames == nullptr)) return MI_ERR_ARG;
    if (B < 1 || N < 1 || N > RS_MAXN || K < 1 || K > N || U < 1 || Tt < 1) return MI_ERR_ARG;
    const dim3 grid((unsigned)B), block(256);
    if (tokens_dtype == 0)
        hipLaunchKernelGGL(rescore_select_kernel<int>, grid, block, 0, stream, nll, len, ctc, denom, w_ctc, w_att, N, U, K, (const int*)tokens, Tt, frames, eos, pad, order,
                           total, att, ctc_out, token_lp, out_tokens, out_n, out_frames);
    else if (tokens_dtype == 1)
        hipLaunchKernelGGL(rescore_select_kernel<long>, grid, block, 0, stream, nll, len, ctc, denom, w_ctc, w_att, N, U, K, (const long*)tokens, Tt, frames, eos, pad, order,
                           total, att, ctc_out, token_lp, out_tokens, out_n, out_frames);
    else return MI_ERR_ARG;
    MI_CHECK_LAUNCH();
    return MI_OK;
}
