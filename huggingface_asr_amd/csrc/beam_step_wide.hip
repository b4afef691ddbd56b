// The beam-search step of csrc/beam_step.hip for the widths the reference's evaluation recipes decode with (recipes_v0.0.1/librispeech_aed/decoding/*_beam_decode.sh:
// --num_beams=60 --max_length=512; ebranchformer_english/decoding: 10 beams, max_length 512): W <= 64 beams, any W * V < 2^24, any max_length.  Same rules, same
// arithmetic, same arguments and outputs as mi_beam_step_lm (the header of beam_step.hip states them; oracle/generate_ref.beam_search pins them); what differs is how the
// top 2W are found and where the ids live.
//
// Selection, exact, in two launches.  A candidate among an utterance's top 2W is among its own row's top K = min(2W, V), so
//   beam_row_select_kernel   one block per (utterance, beam) row: the row's V values are computed ONCE (every load of a group of eight requested before the first is used),
//                            turned into order-preserving keys and kept in LDS; a radix select (8-bit digits, most significant first, a 256-bin LDS histogram per
//                            pass) finds the row's K-th key; the K keys at or above it go to a (B * W, K) table in global memory, unsorted.  The W * V * (1-3 streams)
//                            read of an utterance is spread over W blocks instead of one, and nothing is read twice (V > 8192: the values are recomputed per pass).
//   beam_merge_kernel        one block per utterance: the W * K <= 8192 keys sit in registers (eight per thread), the same radix select takes the top 2W, a rank
//                            sort of those <= 128 puts them best first; then the walk of beam_step.hip, unchanged.
// A key is 56 bits: the float's bits made monotone (-0 counts as +0, so the two zeros tie as they do for the comparison operators) above 2^24 - 1 - (candidate index):
// its unsigned order IS (value descending, index ascending), -inf candidates included, and no two candidates share a key — the select is exact, ties at the threshold
// are resolved by the index digits (three more passes, taken only when the value digits leave a tie), and the outcome does not depend on the order in which threads
// arrive: the histograms are integer counts, the survivors are sorted by key.  No float atomics.
//
// Ids and kept hypotheses.  beam_step.hip stages an utterance's (W, cur_len) ids and (W, Lmax) kept hypotheses in LDS: 492 KB at W = 60, max_length = 512.  Here they move
// in column chunks: 32 columns of all W rows are read into LDS, a barrier, the same 32 columns are written back permuted — in place, no second buffer, 32 KiB.  The kept
// hypotheses are staged only in a step that changes them.  The walk's arrays (stop flags, kept scores / lengths / sources) are LDS arrays, not per-thread ones.
//
// Budgets (hipcc --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage; tests/test_wide_beam_cpu.py reads them from the built code object):
//   beam_row_select_kernel   256 threads, 56 VGPRs (64 with the LM term), 33.0 KiB LDS (32 KiB keys + histogram): four blocks share a CU's 160 KiB; no scratch
//   beam_merge_kernel        1024 threads, 47 VGPRs, 38.3 KiB LDS: two blocks (all 2048 thread slots of a CU) fit; no scratch
#include <map>
#include <utility>

#include "common.hpp"
#include "radix_select.hpp"
#include "../../include/hfasr_hip.h"

namespace {

constexpr float LOGZERO = -10000000000.0f;
constexpr int WB_MAXW = 64, WB_MAXK = 2 * WB_MAXW;
constexpr int RS_THREADS = 256, RS_VCACHE = 8192, RS_UNROLL = 8;
constexpr int MG_THREADS = 1024, MG_CPT = WB_MAXW * WB_MAXK / MG_THREADS, MG_CH = 32;

struct WideArgs {                          // BeamArgs of beam_step.hip, then the table between the two launches
    const float* logits; long ldl;
    const float* lse;
    const float* ctc;
    float w_att, w_ctc;
    int mask_pad;
    int pad, eos, B, W, V, cur_len, max_length, Lmax;
    float denom, heur_denom;
    int early_stopping;
    long* ids;
    float* beam_scores;
    long* new_tok;
    long* beam_idx;
    int* done; int* nfin; float* fin_score; int* fin_len; long* fin_tok;
    float* top_s; int* top_i;
    int* done_out;
    const float* lm_logits; long ldlm;
    const float* lm_lse;
    float w_lm;
    u64* table; int K;                     // (B * W, K) keys of every row's K best candidates, K = min(2W, V)
};

// the host loop's arithmetic (cand_value of beam_step.hip), one rounding per operation: no multiply-add contraction
template <bool LM>
__device__ __forceinline__ float mix_value(const WideArgs& p, int tok, float lg, float ct, float lm, float lse, float lmlse, float bs) {
#pragma clang fp contract(off)
    float s = lg - lse;
    if (p.mask_pad && tok == p.pad) s = LOGZERO;
    if (p.ctc) {
        const float a = p.w_att * s, c = p.w_ctc * ct;
        s = a + c;
    }
    if (LM) {
        const float l = lm - lmlse;
        const float m = p.w_lm * l;
        s = s + m;
    }
    return s + bs;
}

// ---- stage one: a row's K best candidates
template <bool LM>
__global__ __launch_bounds__(RS_THREADS) void beam_row_select_kernel(WideArgs p) {
    __shared__ unsigned vals[RS_VCACHE];
    __shared__ int hist[256], ctl[4], taken;
    const int row = blockIdx.x, tid = threadIdx.x;
    const int b = row / p.W, beam = row - b * p.W;
    if (p.done[b]) return;                                             // (block-uniform) a closed utterance has no candidates
    const int V = p.V, K = p.K, e0 = beam * V;
    const float lse = p.lse[row], bs = p.beam_scores[row], lmlse = LM ? p.lm_lse[row] : 0.f;
    const float* lg = p.logits + (long)row * p.ldl;
    const float* ct = p.ctc ? p.ctc + (long)row * V : nullptr;
    const float* lm = LM ? p.lm_logits + (long)row * p.ldlm : nullptr;
    u64* out = p.table + (long)row * K;
    if (tid == 0) taken = 0;

    // f(token, key of its value) for the tokens tid, tid + 256, ...: eight at a time, their loads requested together (clamped addresses past the last token)
    auto values = [&](auto&& f) {
        for (int t0 = tid; t0 < V; t0 += RS_UNROLL * RS_THREADS) {
            float a[RS_UNROLL], c[RS_UNROLL], l[RS_UNROLL];
#pragma unroll
            for (int u = 0; u < RS_UNROLL; ++u) {
                const int t = t0 + u * RS_THREADS, tc = t < V ? t : V - 1;
                a[u] = lg[tc];
                c[u] = ct ? ct[tc] : 0.f;
                l[u] = LM ? lm[tc] : 0.f;
            }
#pragma unroll
            for (int u = 0; u < RS_UNROLL; ++u) {
                const int t = t0 + u * RS_THREADS;
                if (t < V) f(t, ord_key(mix_value<LM>(p, t, a[u], c[u], l[u], lse, lmlse, bs)));
            }
        }
    };
    if (K == V) {                                                      // 2W >= V: the whole row
        values([&](int t, unsigned hi) { out[t] = cand_key(hi, e0 + t); });
        return;
    }
    const bool cached = V <= RS_VCACHE;
    if (cached) values([&](int t, unsigned hi) { vals[t] = hi; });     // (radix_select's first barrier publishes them)
    auto each = [&](auto&& f) {
        if (cached) {
            for (int t = tid; t < V; t += RS_THREADS) f(cand_key(vals[t], e0 + t));
        } else
            values([&](int t, unsigned hi) { f(cand_key(hi, e0 + t)); });
    };
    u64 thr; int shift;
    radix_select(each, K, hist, ctl, thr, shift);
    each([&](u64 key) {
        if ((key >> shift) >= thr) {
            const int slot = atomicAdd(&taken, 1);
            if (slot < K) out[slot] = key;
        }
    });
}

// ---- stage two: an utterance's top 2W of its W rows' K, the walk, the moves
__global__ __launch_bounds__(MG_THREADS) void beam_merge_kernel(WideArgs p) {
    __shared__ long st_ids[WB_MAXW * MG_CH], st_fin[WB_MAXW * MG_CH];  // a chunk of MG_CH columns of the utterance's ids / kept hypotheses before the step
    __shared__ u64 surv[WB_MAXK];
    __shared__ float tops[WB_MAXK];
    __shared__ int topi[WB_MAXK], ttok[WB_MAXK], tbeam[WB_MAXK], hit[WB_MAXK];
    __shared__ float nbs[WB_MAXW], fs[WB_MAXW];
    __shared__ long nbt[WB_MAXW];
    __shared__ int nbb[WB_MAXW], fsrc[WB_MAXW], fl[WB_MAXW];
    __shared__ int hist[256], ctl[4], taken, nf_new, moved;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int W = p.W, V = p.V, K = p.K, R = 2 * W, n2 = W * K;        // n2 >= R: K >= 2
    const bool was_done = p.done[b] != 0;
    const bool at_max = p.cur_len + 1 >= p.max_length;
    if (tid < W) { fs[tid] = p.fin_score[(long)b * W + tid]; fl[tid] = p.fin_len[(long)b * W + tid]; }
    if (tid == 0) { taken = 0; nf_new = p.nfin[b]; moved = 0; }

    if (!was_done) {                                                   // (block-uniform)
        const u64* src = p.table + (long)b * n2;
        u64 keys[MG_CPT];
#pragma unroll
        for (int i = 0; i < MG_CPT; ++i) {
            const int idx = tid + i * MG_THREADS;
            keys[i] = src[idx < n2 ? idx : n2 - 1];
        }
        auto each = [&](auto&& f) {
#pragma unroll
            for (int i = 0; i < MG_CPT; ++i)
                if (tid + i * MG_THREADS < n2) f(keys[i]);
        };
        u64 thr; int shift;
        radix_select(each, R, hist, ctl, thr, shift);
        each([&](u64 key) {
            if ((key >> shift) >= thr) {
                const int slot = atomicAdd(&taken, 1);
                if (slot < R) surv[slot] = key;
            }
        });
        __syncthreads();
        if (tid < R) {                                                 // best first: a survivor's rank is the number of larger keys
            const u64 my = surv[tid];
            int rank = 0;
            for (int j = 0; j < R; ++j) rank += surv[j] > my ? 1 : 0;
            int e = key_index(my);
            e = e < W * V ? e : W * V - 1;                             // (never taken: the table holds indices of this utterance's candidates)
            const int bm = e / V, tk = e - bm * V;
            tops[rank] = ord_value((unsigned)(my >> 24));
            topi[rank] = e; ttok[rank] = tk; tbeam[rank] = bm;
            hit[rank] = (tk == p.eos || at_max) ? 1 : 0;
        }
    }
    __syncthreads();

    // ---- walk the candidates (one thread: at most 2W steps; the rules and the arithmetic of beam_step.hip, line for line)
    if (tid == 0) {
        for (int k = 0; k < W; ++k) { nbs[k] = 0.f; nbt[k] = was_done ? p.pad : 0; nbb[k] = 0; fsrc[k] = k; }
        if (!was_done) {
            // the W best candidates that did not stop run on; when fewer are left (max_length) the stopped ones follow, lowered by 1e9
            int k = 0;
            for (int r = 0; r < R && k < W; ++r)
                if (!hit[r]) { nbs[k] = tops[r]; nbt[k] = ttok[r]; nbb[k] = tbeam[r]; ++k; }
            for (int r = 0; r < R && k < W; ++r)
                if (hit[r]) { nbs[k] = tops[r] + -1.0e9f; nbt[k] = ttok[r]; nbb[k] = tbeam[r]; ++k; }
            // stopped candidates among the first W ranks compete with the kept hypotheses: best W, best first, an equal score behind the older one
            int nf = nf_new, mv = 0;
            for (int r = 0; r < W; ++r) {
                if (!hit[r]) continue;
                const float sc = tops[r] / p.denom;
                int pos = nf;
                while (pos > 0 && sc > fs[pos - 1]) --pos;
                if (pos >= W) continue;
                const int last = nf < W ? nf : W - 1;
                for (int i = last; i > pos; --i) { fs[i] = fs[i - 1]; fl[i] = fl[i - 1]; fsrc[i] = fsrc[i - 1]; }
                fs[pos] = sc; fl[pos] = p.cur_len + 1; fsrc[pos] = ~r;
                if (nf < W) ++nf;
                mv = 1;
            }
            nf_new = nf;
            moved = mv;
            p.nfin[b] = nf;
            // early-stop rule on the state after the step
            const float best = nbs[0] / p.heur_denom;
            const bool unsat = best > (nf == W ? fs[W - 1] : -1.0e9f);
            if (!unsat || (p.early_stopping == 1 && nf == W) || at_max) p.done[b] = 1;
        }
        if (p.done_out) p.done_out[b] = p.done[b];
    }
    __syncthreads();
    if (!was_done && tid < nf_new) { p.fin_score[(long)b * W + tid] = fs[tid]; p.fin_len[(long)b * W + tid] = fl[tid]; }
    if (p.top_s && tid < R) { p.top_s[(long)b * R + tid] = was_done ? 0.f : tops[tid]; p.top_i[(long)b * R + tid] = was_done ? 0 : topi[tid]; }

    // ---- ids follow their beams, kept hypotheses move to their new ranks: MG_CH columns at a time through LDS (old rows from the staged copy, a new hypothesis = its
    // beam's ids + the closing token)
    const bool mv = moved != 0;
    const int jend = mv ? p.Lmax : p.cur_len;
    for (int j0 = 0; j0 < jend; j0 += MG_CH) {
        for (int i = tid; i < W * MG_CH; i += MG_THREADS) {
            const int k = i / MG_CH, j = j0 + (i - k * MG_CH);
            if (j < p.cur_len) st_ids[i] = p.ids[((long)b * W + k) * p.Lmax + j];
            if (mv && j < p.Lmax) st_fin[i] = p.fin_tok[((long)b * W + k) * p.Lmax + j];
        }
        __syncthreads();
        for (int i = tid; i < W * MG_CH; i += MG_THREADS) {
            const int k = i / MG_CH, jj = i - k * MG_CH, j = j0 + jj;
            if (j < p.cur_len) p.ids[((long)b * W + k) * p.Lmax + j] = st_ids[nbb[k] * MG_CH + jj];
            if (mv && j < p.Lmax && k < nf_new) {
                const int s = fsrc[k];
                if (s != k) {
                    long v;
                    if (s >= 0) v = st_fin[s * MG_CH + jj];
                    else v = j < p.cur_len ? st_ids[tbeam[~s] * MG_CH + jj] : (j == p.cur_len ? (long)ttok[~s] : (long)p.pad);
                    p.fin_tok[((long)b * W + k) * p.Lmax + j] = v;
                }
            }
        }
        __syncthreads();
    }
    if (tid < W) {
        const long row = (long)b * W + tid;
        p.ids[row * p.Lmax + p.cur_len] = nbt[tid];
        p.new_tok[row] = nbt[tid];
        p.beam_idx[row] = (long)b * W + nbb[tid];
        p.beam_scores[row] = nbs[tid];
    }
}

// The (B * W, K) key table between the two launches: one buffer per (device, stream), grown when a call needs more, never shrunk (1 MB at B = 16, W = 64).  Calls on one
// stream are ordered, so they can share it; calls on different streams get different buffers.  Growing frees the old buffer, which waits for the device.
u64* wide_table(hipStream_t st, size_t bytes) {
    static std::mutex mu;
    static std::map<std::pair<int, hipStream_t>, std::pair<void*, size_t>> tab;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return nullptr;
    std::lock_guard<std::mutex> lk(mu);
    auto& e = tab[std::make_pair(dev, st)];
    if (e.second >= bytes) return (u64*)e.first;
    if (e.first) { (void)hipFree(e.first); e.first = nullptr; e.second = 0; }
    size_t want = (size_t)1 << 20;
    while (want < bytes) want <<= 1;
    void* ptr = nullptr;
    if (hipMalloc(&ptr, want) != hipSuccess) return nullptr;
    e.first = ptr; e.second = want;
    return (u64*)ptr;
}

}  // namespace

// mi_beam_step_lm's arguments, rules and outputs for W <= 64 and any max_length (no LDS limit on the id buffers); lm_logits == NULL: no LM term.  Two launches; the table
// between them is the library's own (a hipMalloc at the first call on a stream and when a later call needs a larger one: not inside a stream capture).
extern "C" int mi_beam_step_wide(const float* logits, long ldl, const float* lse, const float* ctc, float w_att, float w_ctc, int mask_pad, int pad, int eos, int B, int W,
                                 int V, int cur_len, int max_length, int Lmax, float denom, float heur_denom, int early_stopping, long* ids, float* beam_scores, long* new_tok,
                                 long* beam_idx, int* done, int* nfin, float* fin_score, int* fin_len, long* fin_tok, float* top_s, int* top_i, int* done_out,
                                 const float* lm_logits, long ld_lm, const float* lm_lse, float w_lm, hipStream_t stream) {
    MI_ENTER();
    if (!logits || !lse || !ids || !beam_scores || !new_tok || !beam_idx || !done || !nfin || !fin_score || !fin_len || !fin_tok) return MI_ERR_ARG;
    if (B <= 0 || W <= 0 || W > WB_MAXW || V <= 1 || ldl < V || (long)W * V >= (1l << 24) || cur_len <= 0 || cur_len >= Lmax || cur_len >= max_length || max_length > Lmax ||
        pad < 0 || pad >= V || !(denom > 0.f) || !(heur_denom > 0.f) || early_stopping < 0 || early_stopping > 2)
        return MI_ERR_ARG;
    if (lm_logits && (!lm_lse || ld_lm < V)) return MI_ERR_ARG;
    if ((top_s == nullptr) != (top_i == nullptr)) return MI_ERR_ARG;
    const int K = 2 * W < V ? 2 * W : V;
    u64* table = wide_table(stream, (size_t)B * W * K * sizeof(u64));
    if (!table) return MI_ERR_LAUNCH;
    WideArgs a{logits, ldl, lse, ctc, w_att, w_ctc, mask_pad, pad, eos, B, W, V, cur_len, max_length, Lmax, denom, heur_denom, early_stopping, ids, beam_scores, new_tok, beam_idx,
               done, nfin, fin_score, fin_len, fin_tok, top_s, top_i, done_out, lm_logits, ld_lm, lm_lse, w_lm, table, K};
    if (lm_logits) hipLaunchKernelGGL(beam_row_select_kernel<true>, dim3(B * W), dim3(RS_THREADS), 0, stream, a);
    else hipLaunchKernelGGL(beam_row_select_kernel<false>, dim3(B * W), dim3(RS_THREADS), 0, stream, a);
    hipLaunchKernelGGL(beam_merge_kernel, dim3(B), dim3(MG_THREADS), 0, stream, a);
    MI_CHECK_LAUNCH();
    return MI_OK;
}
