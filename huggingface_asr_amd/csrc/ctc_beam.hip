// CTC prefix beam search on gfx950: the n best label sequences of a CTC model's logits, each scored with the SUM over all of its alignments that the beam kept.
//
// Reference: ctc_beam_decode (src/utilities/eval_utils.py:46-62, the CTC trainer's preprocess_logits_for_metrics when --generation_num_beams > 1,
// src/trainers/train_ctc_asr.py:77-85) hands log-softmax rows to torchaudio's flashlight lexicon-free decoder on the CPU.  This is deliberately NOT a clone of that
// decoder (which takes the max over alignments by default and treats a `sil` token specially): it is the textbook sum-over-alignments prefix search, whose answer can
// be enumerated exactly for small problems (tests/ctc_beam_ref.py).
//
// ---- Semantics (normative; DESIGN.md 'CTC prefix beam search' repeats them)
// Per utterance b: logits x[t, c], t < n_b, c < V1; n_b = lengths[b] clipped to [0, T], or T without lengths; `blank` any class; beam width 1 <= W <= 64; token cut
// 1 <= K <= 64.  a (+) b is logaddexp in fp32, max(a, b) + log1p(exp(min(a, b) - max(a, b))) and -inf when both are; lp[t, c] = x[t, c] - lse_t with lse_t over all
// V1 classes (an x of -inf gives lp = -inf).
//   Token cut   toks_t = the min(K, V1 - 1) non-blank classes of frame t with the largest logits, equal values by lower class index (argmax_key's order).
//   State       a hypothesis is a label prefix l with p_b (alignments ending in blank) and p_nb (ending in its last label); score = p_b (+) p_nb.
//               Start: {(): p_b = 0, p_nb = -inf}.
//   Frame step  for every kept l, tot = p_b (+) p_nb:
//                 p_b'(l)      (+)= tot + lp[t, blank]
//                 p_nb'(l)     (+)= p_nb + lp[t, last(l)]                       l not empty; whether or not last(l) is in toks_t
//                 p_nb'(l + c) (+)= (c == last(l) ? p_b : tot) + lp[t, c]       c in toks_t
//               A prefix reached as a survivor and as an extension of its parent is ONE hypothesis: p_nb' = (survivor term) (+) (extension term), p_b' has one term.
//   Selection   the W largest scores, never a score of -inf; equal scores: survivor before extension, then lower rank of the (parent) hypothesis in the beam, then
//               lower rank in toks_t.
//   Output      after frame n_b - 1 the nbest <= W best, best first: tokens (B, nbest, T) int32 | int64 padded with pad_id, n_tokens (B, nbest), scores (B, nbest)
//               fp32, frames (B, nbest, T) (optional): the frame at which each token's prefix first entered the beam, then -1.  Rows beyond the hypotheses that
//               exist: n_tokens 0, score -inf, pad / -1.  n_b = 0: the empty hypothesis, score 0.
//   No float atomics: two runs are bit-identical; an utterance's result does not depend on the rest of the batch.
//
// ---- Launch A, ctc_cut_kernel: one block (256 threads) per row (b, t), t < n_b; rows past n_b are skipped.  The row is read ONCE (16-B vectors where the row is 16-B
// aligned, four in flight per thread) into LDS as order-preserving 32-bit keys (V1 <= 8192; a longer row is re-read per pass instead); from LDS: the maximum, the sum
// of exponentials in a fixed order (lse), the radix select of radix_select.hpp over the non-blank classes for the K-th key, a rank sort of the K survivors.  Writes
// lse, lp[blank] and toks_t as (lp, class id) best first into (B, T, K) tables (entries past V1 - 1: -inf / -1).
//
// ---- Launch B, ctc_walk_kernel: one block per utterance walks its frames.  The beam (W x {p_b, p_nb, score, node, last token, parent node, length}, twice: this
// frame's and the next one's) lives in LDS with the frame's n (K + 1) <= 4160 candidate keys.  Candidate index = rank of the survivor, or W + rank * K + k for the
// extension of hypothesis `rank` by toks_t[k]: the key order is the tie rule above.  The merge goes through the trie: survivor j absorbs the extension (i, k) with
// node[i] == parent node of j and toks_t[k] == last(j), and that extension stops being a candidate.  Prefixes live in a per-utterance arena of (parent, token, frame,
// length) nodes in global memory, at most 1 + T W, appended only for selected new prefixes.  A prefix that left the beam can come back as an extension of its parent
// while one of its own children is still in the beam; so that it then merges with that child's line again, nodes are canonical: a selected new prefix first looks its
// (parent node, token) up in an open-addressing table in global memory (integer compare-and-swap; one 64-bit word per node, at most half full) and re-uses the node it
// had.  Every access to that table is an agent-scope atomic (they meet in the L2; a block's waves order them with the block's barriers).  The n-best are backtraced at the end of the same launch.  Every loop is bounded by T, W, K or the table size; no block waits on another.
//
// Budgets (hipcc --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage; tests/test_ctc_beam_cpu.py reads them from the built code object):
//   ctc_cut_kernel    256 threads, 56 VGPRs, 34352 B of LDS (32 KiB keys + histogram + survivors): four blocks share a CU's 160 KiB; no scratch
//   ctc_walk_kernel   256 threads (W (K + 1) <= 1024) or 1024, 65 VGPRs, 44576 B of LDS (32.5 KiB candidate keys, 4 KiB merge flags, the two beams); no scratch
#include "common.hpp"
#include "radix_select.hpp"
#include "ctc_walk_step.hpp"
#include "../../include/hfasr_hip.h"

namespace {

constexpr int CUT_THREADS = 256, CUT_VCACHE = 8192;

template <typename T> struct Vec16;
template <> struct Vec16<float> { typedef f32x4 type; static constexpr int N = 4; };
template <> struct Vec16<bf16_t> { typedef bf16x8 type; static constexpr int N = 8; };

__device__ __forceinline__ unsigned value_key(float v) { return (unsigned)(argmax_key(v, 0) >> 32); }      // ord_key with every NaN on top, the shared argmax order

struct CutArgs {
    const void* x; long ld_t, ld_b;
    int B, T, V1;
    const int* lengths;
    int blank, K;
    float* lse; float* lpb; float* cut_lp; int* cut_id;
};

// ---- launch A
template <typename T>
__global__ __launch_bounds__(CUT_THREADS) void ctc_cut_kernel(CutArgs p) {
    typedef typename Vec16<T>::type vec_t;
    constexpr int VN = Vec16<T>::N;
    __shared__ unsigned vals[CUT_VCACHE];
    __shared__ u64 surv[CB_MAXK];
    __shared__ int hist[256], ctl[4], taken;
    __shared__ unsigned wmax[4];
    __shared__ float wsum[4];
    const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = row / p.T, t = row - b * p.T;
    const int n = p.lengths ? min(max(p.lengths[b], 0), p.T) : p.T;
    if (t >= n) return;                                                // (block-uniform)
    const int V = p.V1, K = p.K, Kk = min(K, V - 1), blank = p.blank;
    const T* xr = (const T*)p.x + (long)b * p.ld_b + (long)t * p.ld_t;
    const bool cached = V <= CUT_VCACHE;
    if (tid == 0) taken = 0;

    // f(class, value key) for the classes this thread owns, from global memory
    auto from_row = [&](auto&& f) {
        int done = 0;
        if ((reinterpret_cast<uintptr_t>(xr) & 15) == 0) {
            const int nvec = V / VN;
            const vec_t* xv = reinterpret_cast<const vec_t*>(xr);
            for (int q0 = tid; q0 < nvec; q0 += 4 * CUT_THREADS) {
                vec_t v[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int q = q0 + u * CUT_THREADS;
                    v[u] = xv[q < nvec ? q : nvec - 1];
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int q = q0 + u * CUT_THREADS;
                    if (q < nvec)
#pragma unroll
                        for (int e = 0; e < VN; ++e) f(q * VN + e, value_key((float)v[u][e]));
                }
            }
            done = nvec * VN;
        }
        for (int c = done + tid; c < V; c += CUT_THREADS) f(c, value_key((float)xr[c]));
    };
    // the same from LDS once the row is there
    auto classes = [&](auto&& f) {
        if (cached) {
            for (int c = tid; c < V; c += CUT_THREADS) f(c, vals[c]);
        } else
            from_row(f);
    };

    unsigned mk = 0;                                                   // the row's maximum, as a key
    from_row([&](int c, unsigned k) {
        if (cached) vals[c] = k;
        mk = k > mk ? k : mk;
    });
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned other = (unsigned)__shfl_xor((int)mk, o, 64);
        mk = other > mk ? other : mk;
    }
    if (lane == 0) wmax[wave] = mk;
    __syncthreads();                                                   // (also publishes vals)
    mk = max(max(wmax[0], wmax[1]), max(wmax[2], wmax[3]));
    const float m = argmax_value((amax_t)mk << 32);
    float s = 0.f;
    classes([&](int, unsigned k) {
        const float v = argmax_value((amax_t)k << 32);
        s += v == NEG_INF ? 0.f : expf(v - m);
    });
    s = wave_sum(s);
    if (lane == 0) wsum[wave] = s;
    __syncthreads();
    const float lse = m + logf((wsum[0] + wsum[1]) + (wsum[2] + wsum[3]));

    auto each = [&](auto&& f) {
        classes([&](int c, unsigned k) {
            if (c != blank) f(cand_key(k, c));
        });
    };
    u64 thr = 0; int shift = 0;                                        // Kk == V - 1: every non-blank class
    if (Kk < V - 1) radix_select(each, Kk, hist, ctl, thr, shift);
    each([&](u64 key) {
        if ((key >> shift) >= thr) {
            const int slot = atomicAdd(&taken, 1);
            if (slot < CB_MAXK) surv[slot] = key;
        }
    });
    __syncthreads();
    float* olp = p.cut_lp + (long)row * K;
    int* oid = p.cut_id + (long)row * K;
    if (tid < Kk) {                                                    // best first: a survivor's rank is the number of larger keys
        const u64 my = surv[tid];
        int rank = 0;
        for (int j = 0; j < Kk; ++j) rank += surv[j] > my ? 1 : 0;
        olp[rank] = log_prob(argmax_value((amax_t)(unsigned)(my >> 24) << 32), lse);
        oid[rank] = key_index(my);
    } else if (tid < K) {
        olp[tid] = NEG_INF;
        oid[tid] = -1;
    }
    if (tid == 0) {
        p.lse[row] = lse;
        p.lpb[row] = log_prob(cached ? argmax_value((amax_t)vals[blank] << 32) : (float)xr[blank], lse);
    }
}

// ---- launch B
// the arguments (WalkArgs), the utterance's walk (walk_utterance), the frame step (walk_frame) and the backtrace (walk_backtrace) are ctc_walk_step.hpp's: the stream and
// pool kernels walk with the same step, and ctc_beam_bias.hip's ctc_bias_walk is this kernel with the bias policy
template <typename TOK>
__global__ __launch_bounds__(1024) void ctc_walk_kernel(WalkArgs p) {
    __shared__ WalkLds L;
    int n;
    walk_utterance<TOK>(L, p, NoBias{}, blockIdx.x, n);
}

}  // namespace

// bytes of mi_ctc_beam_walk's workspace: per utterance the node arena (1 + T W nodes of 16 B) and the node table; 0 for arguments the walk refuses
extern "C" size_t mi_ctc_beam_workspace_bytes(int B, int T, int W) {
    if (B <= 0 || T <= 0 || W < 1 || W > CB_MAXW || !walk_sizes_ok(T, W, 2)) return 0;
    return align16((size_t)B * (1 + (size_t)T * W) * sizeof(int4)) + (size_t)B * table_words(T, W) * sizeof(u64);
}

extern "C" int mi_ctc_beam_cut(const void* logits, long ld_row, long ld_batch, int dtype, int B, int T, int V1, const int* lengths, int blank, int K, float* lse,
                               float* lp_blank, float* cut_lp, int* cut_id, hipStream_t stream) {
    MI_ENTER();
    if (!logits || !lse || !lp_blank || !cut_lp || !cut_id || B <= 0 || T <= 0 || V1 < 2 || K < 1 || K > CB_MAXK || blank < 0 || blank >= V1 || (dtype != 0 && dtype != 1))
        return MI_ERR_ARG;
    if (V1 >= (1 << 24) || (long)B * T >= (1l << 31)) return MI_ERR_UNSUPPORTED;
    CutArgs a{logits, ld_row, ld_batch, B, T, V1, lengths, blank, K, lse, lp_blank, cut_lp, cut_id};
    if (dtype == 0) hipLaunchKernelGGL(ctc_cut_kernel<float>, dim3(B * T), dim3(CUT_THREADS), 0, stream, a);
    else hipLaunchKernelGGL(ctc_cut_kernel<bf16_t>, dim3(B * T), dim3(CUT_THREADS), 0, stream, a);
    MI_CHECK_LAUNCH();
    return MI_OK;
}

extern "C" int mi_ctc_beam_walk(const void* logits, long ld_row, long ld_batch, int dtype, int B, int T, int V1, const int* lengths, int blank, long pad_id, int W, int K,
                                int nbest, const float* lse, const float* lp_blank, const float* cut_lp, const int* cut_id, void* workspace, size_t workspace_bytes,
                                void* tokens, int tokens_dtype, int* n_tokens, float* scores, int* frames, hipStream_t stream) {
    MI_ENTER();
    WalkArgs a;
    dim3 block;
    const int rc = walk_prepare(logits, ld_row, ld_batch, dtype, B, T, V1, lengths, blank, pad_id, W, K, nbest, lse, lp_blank, cut_lp, cut_id, workspace, workspace_bytes,
                                mi_ctc_beam_workspace_bytes(B, T, W), tokens, tokens_dtype, n_tokens, scores, frames, a, block);
    if (rc != MI_OK) return rc;
    if (tokens_dtype == 0) hipLaunchKernelGGL(ctc_walk_kernel<int>, dim3(B), block, 0, stream, a);
    else hipLaunchKernelGGL(ctc_walk_kernel<long>, dim3(B), block, 0, stream, a);
    MI_CHECK_LAUNCH();
    return MI_OK;
}
