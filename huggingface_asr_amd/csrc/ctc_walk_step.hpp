// The frame step of the CTC prefix beam search, ONE definition for the kernels that walk frames with it: ctc_walk_kernel (ctc_beam.hip, a whole utterance per
// launch) and, through ctc_beam_stream_body.hpp, ctc_stream_beam_kernel (ctc_beam_stream.hip, the same walk suspended between launches) and ctc_pool_beam_kernel
// (ctc_beam_pool.hip, that per slot of a session pool).  ctc_beam.hip's header states the semantics; this file holds the state (Beam), the block's LDS (WalkLds), the
// step (walk_frame) and the backtrace of the n best (walk_backtrace).  All of them must take the same decisions and sum in the same order, bit for bit: whatever
// changes here changes all.  The same definitions, instantiated with the bias policy below, are the kernels of contextual biasing: ctc_bias_walk (ctc_beam_bias.hip,
// whose header states what the bias changes), ctc_bias_stream_beam (ctc_beam_bias_stream.hip) and ctc_bias_pool_beam (ctc_beam_bias_pool.hip).
#pragma once
#include "common.hpp"
#include "radix_select.hpp"

namespace {

constexpr int CB_MAXW = 64, CB_MAXK = 64, CB_MAXC = CB_MAXW * (CB_MAXK + 1);
constexpr unsigned KEY_NEG_INF = 0x007FFFFFu;                           // ord_key(-inf): a candidate counts iff its value key is above it
constexpr float NEG_INF = -__builtin_inff();

__device__ __forceinline__ float logaddexp_f(float a, float b) {
    const float m = fmaxf(a, b), d = fminf(a, b) - m;
    return m == NEG_INF ? m : m + log1pf(expf(d));
}
__device__ __forceinline__ float log_prob(float x, float lse) { return x == NEG_INF ? NEG_INF : x - lse; }

// a table word: (parent node + 1) in bits 63..42, the token in 41..22, the node in 21..0; 0 = empty
__device__ __forceinline__ u64 node_word(int parent, int token) { return ((u64)(unsigned)(parent + 1) << 42) | ((u64)(unsigned)token << 22); }
__device__ __forceinline__ unsigned node_hash(u64 w) {
    u64 z = (w >> 22) * 0x9E3779B97F4A7C15ull;
    return (unsigned)(z >> 32);
}

// ---- The bias policy, a compile-time parameter of the state, the LDS and the step.  NoBias is the search of ctc_beam.hip: nothing is carried, nothing is read,
// the code and the layout are the ones without a policy.  TrieBias is the contextual biasing of ctc_beam_bias.hip (its header states the semantics): a hypothesis
// carries the state s of its label prefix in the phrase automaton and its credit n, and is selected and ranked by score + w (float)n.
struct NoBias { static constexpr bool on = false; };
struct TrieBias {
    static constexpr bool on = true;
    const int* col; const int* tab;                                    // col (V1): a token's column; tab (S, A1): (dn << 16) | next per (state, column)
    int S, A1, V1; float w;
    int* sn;                                                           // a beam stream's carried (s, n): per stream 2 x CB_MAXW ints behind the unbiased state; else null
    int* credit;                                                       // out: n per hypothesis, a row of nbest beside every row of scores
};

// one token through the automaton: (s, tok) -> (next state, dn).  Whatever the tables hold, every index is clamped into them: tok into [0, V1), the column into [0, A1),
// s and next into [0, S); a malformed context gives a wrong credit, never an access outside the tables.
__device__ __forceinline__ void bias_step(const TrieBias& b, int s, int tok, int& next, int& dn) {
    const int c = min(max(b.col[min(max(tok, 0), b.V1 - 1)], 0), b.A1 - 1);
    const int word = b.tab[min(max(s, 0), b.S - 1) * b.A1 + c];
    next = min(word & 0xFFFF, b.S - 1);
    dn = word >> 16;
}
__device__ __forceinline__ float bias_value(const TrieBias& b, float v, int n) { return __fadd_rn(v, __fmul_rn(b.w, (float)n)); }      // one multiply, one add, never fused; -inf stays -inf: w is finite

template <bool ON> struct BeamBias {};                                  // (a base, so that it takes no room when it is empty)
template <> struct BeamBias<true> { int bs[CB_MAXW], bn[CB_MAXW]; };
template <class P> struct BeamT : BeamBias<P::on> {
    float pb[CB_MAXW], pnb[CB_MAXW], sc[CB_MAXW];
    int node[CB_MAXW], last[CB_MAXW], parent[CB_MAXW], len[CB_MAXW];
};
typedef BeamT<NoBias> Beam;

// the LDS of a walking block: 44576 B; 45600 B with TrieBias (the two beams carry s and n)
template <class P> struct WalkLdsT {
    u64 keys[CB_MAXC];
    unsigned dead_words[CB_MAXW * CB_MAXK / 4];                         // one byte per extension (i, k): it was folded into a survivor
    BeamT<P> beams[2];
    float tot[CB_MAXW], spb[CB_MAXW], spnb[CB_MAXW], ssc[CB_MAXW], tlp[CB_MAXK];
    int tcls[CB_MAXK], isnew[CB_MAXW], outlen[CB_MAXW];
    u64 surv[CB_MAXW];
    int hist[256], ctl[4], taken, n_next, n_nodes[2];
};
typedef WalkLdsT<NoBias> WalkLds;
static_assert(sizeof(Beam) == 7 * CB_MAXW * 4 && sizeof(WalkLds) == 44576 && sizeof(WalkLdsT<TrieBias>) == 45600, "the layouts the kernels' headers state");

// what a frame step reads besides the beam: the logits, the cut's tables, the utterance's arena and node table (H words, a power of two)
struct WalkIn {
    const void* x; int dtype;
    int W, K, Kk;
    const float* lse; const float* lpb; const float* cut_lp; const int* cut_id;
    int4* arena; long arena_stride;
    u64* table; unsigned H;
};

// One frame: L.beams[cur] (n hypotheses, node count L.n_nodes[cur]) -> L.beams[cur ^ 1], L.n_nodes[cur ^ 1]; returns the new n.  `row` indexes the cut's tables, `at0`
// is the element offset of the frame's logits row in q.x, `stamp` the frame index written into the nodes of new prefixes.  Every thread of the block calls it.
// With TrieBias an extension candidate steps its parent's (s, n) by its token — two dependent 4-byte loads from the L2-resident tables — for the value it is ranked by,
// and again when it is selected; its CTC score is recomputed, not recovered from the key, which then holds the biased value.
template <class P>
__device__ __forceinline__ int walk_frame(WalkLdsT<P>& L, const WalkIn& q, const P& bias, int cur, int n, long row, long at0, int stamp) {
    const int tid = threadIdx.x, nt = blockDim.x;
    unsigned char* dead = reinterpret_cast<unsigned char*>(L.dead_words);
    const int W = q.W, K = q.K, Kk = q.Kk;
    const unsigned H = q.H;
    int4* arena = q.arena;
    u64* table = q.table;
    const BeamT<P>& s = L.beams[cur];
    BeamT<P>& nx = L.beams[cur ^ 1];
    const float lpb = q.lpb[row], lse = q.lse[row];
    if (tid < Kk) { L.tlp[tid] = q.cut_lp[row * K + tid]; L.tcls[tid] = q.cut_id[row * K + tid]; }
    for (int i = tid; i < CB_MAXW * CB_MAXK / 4; i += nt) L.dead_words[i] = 0u;
    if (tid == 0) { L.taken = 0; L.n_next = 0; }
    if (tid < n) {                                                     // the survivor terms
        const float a = s.pb[tid], c = s.pnb[tid];
        const float tt = logaddexp_f(a, c);
        const int last = s.last[tid];
        float own = NEG_INF;
        if (last >= 0) {
            const long at = at0 + last;
            const float xv = q.dtype ? (float)((const bf16_t*)q.x)[at] : ((const float*)q.x)[at];
            own = c + log_prob(xv, lse);
        }
        L.tot[tid] = tt; L.spb[tid] = tt + lpb; L.spnb[tid] = own;
    }
    __syncthreads();
    if (tid < n) {                                                     // the merge: survivor tid absorbs the extension of its parent by its last token
        const int last = s.last[tid], par = s.parent[tid];
        float own = L.spnb[tid];
        if (last >= 0) {
            int pi = -1, pk = -1;
            for (int i = 0; i < n; ++i) pi = s.node[i] == par ? i : pi;
            for (int k = 0; k < Kk; ++k) pk = L.tcls[k] == last ? k : pk;
            if (pi >= 0 && pk >= 0) {
                own = logaddexp_f(own, (s.last[pi] == last ? s.pb[pi] : L.tot[pi]) + L.tlp[pk]);
                dead[pi * K + pk] = 1;
                L.spnb[tid] = own;
            }
        }
        L.ssc[tid] = logaddexp_f(L.spb[tid], own);
    }
    __syncthreads();
    const int ntot = n * (Kk + 1), kk = min(W, ntot);
    for (int e = tid; e < ntot; e += nt) {
        float v; int idx;
        if (e < n) {
            v = L.ssc[e]; idx = e;
            if constexpr (P::on) v = bias_value(bias, v, s.bn[e]);
        } else {
            const int qq = e - n, i = qq / Kk, k = qq - i * Kk;
            idx = W + i * K + k;
            v = dead[i * K + k] ? NEG_INF : (L.tcls[k] == s.last[i] ? s.pb[i] : L.tot[i]) + L.tlp[k];
            if constexpr (P::on) {
                int ns, dn;
                bias_step(bias, s.bs[i], L.tcls[k], ns, dn);
                v = bias_value(bias, v, s.bn[i] + dn);
            }
        }
        L.keys[e] = cand_key(ord_key(v), idx);
    }
    auto each = [&](auto&& f) {
        for (int e = tid; e < ntot; e += nt) f(L.keys[e]);
    };
    u64 thr; int shift;
    radix_select(each, kk, L.hist, L.ctl, thr, shift);                 // (its first barrier publishes the keys)
    each([&](u64 key) {
        if ((key >> shift) >= thr) {
            const int slot = atomicAdd(&L.taken, 1);
            if (slot < CB_MAXW) L.surv[slot] = key;
        }
    });
    __syncthreads();
    if (tid < kk) {                                                    // best first; a selected extension looks for the node its prefix had
        const u64 my = L.surv[tid];
        int rank = 0;
        for (int j = 0; j < kk; ++j) rank += L.surv[j] > my ? 1 : 0;
        const unsigned hi = (unsigned)(my >> 24);
        int fresh = 0;
        if (hi > KEY_NEG_INF) {
            float v = ord_value(hi);
            int idx = key_index(my);
            atomicAdd(&L.n_next, 1);
            if (idx < W) {
                idx = idx < n ? idx : 0;                               // (never taken)
                if constexpr (P::on) { v = L.ssc[idx]; nx.bs[rank] = s.bs[idx]; nx.bn[rank] = s.bn[idx]; }
                nx.pb[rank] = L.spb[idx]; nx.pnb[rank] = L.spnb[idx]; nx.sc[rank] = v;
                nx.node[rank] = s.node[idx]; nx.last[rank] = s.last[idx]; nx.parent[rank] = s.parent[idx]; nx.len[rank] = s.len[idx];
            } else {
                int i = (idx - W) / K, k = (idx - W) - i * K;
                i = i < n ? i : 0; k = k < Kk ? k : 0;                 // (never taken)
                const int tok = L.tcls[k], par = s.node[i];
                if constexpr (P::on) {
                    int ns, dn;
                    bias_step(bias, s.bs[i], tok, ns, dn);
                    v = (tok == s.last[i] ? s.pb[i] : L.tot[i]) + L.tlp[k];
                    nx.bs[rank] = ns; nx.bn[rank] = s.bn[i] + dn;
                }
                const u64 w = node_word(par, tok);
                int found = -1;
                unsigned h = node_hash(w);
                for (unsigned probe = 0; probe < H; ++probe, ++h) {
                    const u64 e = __hip_atomic_load(&table[h & (H - 1)], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if (e == 0ull) break;
                    if ((e >> 22) == (w >> 22)) { found = (int)(e & 0x3FFFFFull); break; }
                }
                fresh = found < 0 ? 1 : 0;
                nx.pb[rank] = NEG_INF; nx.pnb[rank] = v; nx.sc[rank] = v;
                nx.node[rank] = found; nx.last[rank] = tok; nx.parent[rank] = par; nx.len[rank] = s.len[i] + 1;
            }
        }
        L.isnew[rank] = fresh;
    }
    __syncthreads();
    const int nn = L.n_next, base = L.n_nodes[cur];
    if (tid < nn) {                                                    // new prefixes get the next node ids in rank order, and enter the table
        int off = 0;
        for (int r = 0; r < tid; ++r) off += L.isnew[r];
        if (L.isnew[tid]) {
            const int id = base + off, par = nx.parent[tid], tok = nx.last[tid];
            nx.node[tid] = id;
            arena[id < q.arena_stride ? id : 0] = make_int4(par, tok, stamp, nx.len[tid]);
            const u64 w = node_word(par, tok) | (u64)(unsigned)id;
            unsigned h = node_hash(w);
            for (unsigned probe = 0; probe < H; ++probe, ++h)
                if (atomicCAS(&table[h & (H - 1)], 0ull, w) == 0ull) break;
        }
        if (tid == nn - 1) L.n_nodes[cur ^ 1] = base + off + L.isnew[tid];
    }
    if (nn == 0 && tid == 0) L.n_nodes[cur ^ 1] = base;
    __syncthreads();
    return nn;
}

// The n best of beam s (n hypotheses), backtraced into rows [0, nbest) of tokens / frames (each `width` wide, n_tokens / scores one per row): a row's tokens then
// pad_id, frames then -1; rows that do not exist: 0 tokens, -inf.  Every thread of the block calls it.
template <typename TOK, class P>
__device__ __forceinline__ void walk_backtrace(WalkLdsT<P>& L, const BeamT<P>& s, int n, int nbest, int width, const int4* arena, long arena_stride, long pad_id, TOK* tokens,
                                               int* frames, int* n_tokens, float* scores) {
    const int tid = threadIdx.x, nt = blockDim.x;
    if (tid < nbest) {
        int len = 0;
        float sc = NEG_INF;
        if (tid < n) {
            len = min(s.len[tid], width);
            sc = s.sc[tid];
            int nd = s.node[tid];
            for (int pos = len - 1; pos >= 0 && nd > 0; --pos) {
                const int4 e = arena[nd < arena_stride ? nd : 0];
                tokens[(long)tid * width + pos] = (TOK)e.y;
                if (frames) frames[(long)tid * width + pos] = e.z;
                nd = e.x;
            }
        }
        L.outlen[tid] = len;
        n_tokens[tid] = len;
        scores[tid] = sc;
    }
    __syncthreads();
    for (long i = tid; i < (long)nbest * width; i += nt) {
        const int r = (int)(i / width), pos = (int)(i - (long)r * width);
        if (pos >= L.outlen[r]) {
            tokens[i] = (TOK)pad_id;
            if (frames) frames[i] = -1;
        }
    }
}

// the credit n of the n best of beam s into credit[0, nbest); rows that do not exist: 0
__device__ __forceinline__ void walk_credit(const BeamT<TrieBias>& s, int n, int nbest, int* credit) {
    const int tid = threadIdx.x;
    if (tid < nbest) credit[tid] = tid < n ? s.bn[tid] : 0;
}

// ---- a whole utterance per block: what the one-shot kernels (ctc_walk_kernel, ctc_bias_walk) take and run
struct WalkArgs {
    const void* x; long ld_t, ld_b; int dtype;
    int B, T, V1;
    const int* lengths;
    int blank; long pad_id;
    int W, K, nbest;
    const float* lse; const float* lpb; const float* cut_lp; const int* cut_id;
    int4* arena; long arena_stride;                                    // per utterance: 1 + T W nodes (parent, token, frame, length)
    u64* table; long table_stride;                                     // per utterance: the (parent node, token) -> node table
    void* tokens; int* n_tokens; float* scores; int* frames;
};

// utterance b from the start {(): p_b = 0, p_nb = -inf} through its n_b frames, then the n best backtraced -> the beam they stand in and its n.  Every thread of the
// block calls it.
template <typename TOK, class P>
__device__ __forceinline__ const BeamT<P>& walk_utterance(WalkLdsT<P>& L, const WalkArgs& p, const P& bias, int b, int& n_out) {
    const int tid = threadIdx.x, nt = blockDim.x;
    const int W = p.W, T = p.T, nbest = p.nbest;
    const int n_b = p.lengths ? min(max(p.lengths[b], 0), T) : T;
    int4* arena = p.arena + (long)b * p.arena_stride;
    u64* table = p.table + (long)b * p.table_stride;
    unsigned H = 2;                                                    // this utterance's table: a power of two >= 2 (1 + n_b W) words (<= table_stride)
    while (H < 2u * (1u + (unsigned)n_b * (unsigned)W)) H <<= 1;
    for (unsigned i = tid; i < H; i += nt) __hip_atomic_store(&table[i], 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (tid == 0) {
        BeamT<P>& s = L.beams[0];
        s.pb[0] = 0.f; s.pnb[0] = NEG_INF; s.sc[0] = 0.f; s.node[0] = 0; s.last[0] = -1; s.parent[0] = -1; s.len[0] = 0;
        if constexpr (P::on) { s.bs[0] = 0; s.bn[0] = 0; }             // the automaton's root, no credit
        arena[0] = make_int4(-1, -1, -1, 0);
        L.n_nodes[0] = 1;
    }
    __syncthreads();

    const WalkIn q{p.x, p.dtype, W, p.K, min(p.K, p.V1 - 1), p.lse, p.lpb, p.cut_lp, p.cut_id, arena, p.arena_stride, table, H};
    int n = 1, cur = 0;
    for (int t = 0; t < n_b && n > 0; ++t, cur ^= 1) n = walk_frame(L, q, bias, cur, n, (long)b * T + t, (long)b * p.ld_b + (long)t * p.ld_t, t);

    // ---- the n best, backtraced; rows that do not exist
    walk_backtrace<TOK>(L, L.beams[cur], n, nbest, T, arena, p.arena_stride, p.pad_id, (TOK*)p.tokens + (long)b * nbest * T,
                        p.frames ? p.frames + (long)b * nbest * T : nullptr, p.n_tokens + (long)b * nbest, p.scores + (long)b * nbest);
    n_out = n;
    return L.beams[cur];
}

inline size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }
inline long table_words(int T, int W) {
    long h = 2;
    while (h < 2 * (1 + (long)T * W)) h <<= 1;
    return h;
}
inline bool walk_sizes_ok(int T, int W, int V1) { return 1 + (long)T * W < (1l << 22) - 1 && V1 <= (1 << 20); }
inline dim3 walk_block(int W, int K, int V1) { return dim3(W * ((K < V1 - 1 ? K : V1 - 1) + 1) <= 1024 ? 256 : 1024); }

// the argument check of the one-shot entries (mi_ctc_beam_walk, mi_ctc_beam_walk_bias), then their kernel's arguments and block; `need` = mi_ctc_beam_workspace_bytes
inline int walk_prepare(const void* logits, long ld_row, long ld_batch, int dtype, int B, int T, int V1, const int* lengths, int blank, long pad_id, int W, int K, int nbest,
                        const float* lse, const float* lp_blank, const float* cut_lp, const int* cut_id, void* workspace, size_t workspace_bytes, size_t need, void* tokens,
                        int tokens_dtype, int* n_tokens, float* scores, int* frames, WalkArgs& a, dim3& block) {
    if (!logits || !lse || !lp_blank || !cut_lp || !cut_id || !workspace || !tokens || !n_tokens || !scores || B <= 0 || T <= 0 || V1 < 2 || W < 1 || W > CB_MAXW || K < 1 ||
        K > CB_MAXK || nbest < 1 || nbest > W || blank < 0 || blank >= V1 || (dtype != 0 && dtype != 1) || (tokens_dtype != 0 && tokens_dtype != 1))
        return MI_ERR_ARG;
    if (!walk_sizes_ok(T, W, V1)) return MI_ERR_UNSUPPORTED;
    if (workspace_bytes < need || (reinterpret_cast<uintptr_t>(workspace) & 15)) return MI_ERR_ARG;
    const long nodes = 1 + (long)T * W, words = table_words(T, W);
    a = WalkArgs{logits, ld_row, ld_batch, dtype, B, T, V1, lengths, blank, pad_id, W, K, nbest, lse, lp_blank, cut_lp, cut_id,
                 (int4*)workspace, nodes, (u64*)((char*)workspace + align16((size_t)B * nodes * sizeof(int4))), words, tokens, n_tokens, scores, frames};
    block = walk_block(W, K, V1);
    return MI_OK;
}

// the bias arguments of the biased entries: the tables, their limits (1 <= S <= 4096, 1 <= A1 <= 1024, S A1 <= 2^20), a finite weight
constexpr int BIAS_MAXS = 4096, BIAS_MAXA = 1024, BIAS_MAXWORDS = 1 << 20;
inline bool bias_args_ok(const int* col, const int* tab, int S, int A1, float w) {
    return col && tab && S >= 1 && S <= BIAS_MAXS && A1 >= 1 && A1 <= BIAS_MAXA && (long)S * A1 <= BIAS_MAXWORDS && __builtin_isfinite(w);
}

}  // namespace
