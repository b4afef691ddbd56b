// The frame step of the CTC prefix beam search, ONE definition for the kernels that walk frames with it: ctc_walk_kernel (ctc_beam.hip, a whole utterance per
// launch) and, through ctc_beam_stream_body.hpp, ctc_stream_beam_kernel (ctc_beam_stream.hip, the same walk suspended between launches) and ctc_pool_beam_kernel
// (ctc_beam_pool.hip, that per slot of a session pool).  ctc_beam.hip's header states the semantics; this file holds the state (Beam), the block's LDS (WalkLds), the
// step (walk_frame) and the backtrace of the n best (walk_backtrace).  All of them must take the same decisions and sum in the same order, bit for bit: whatever
// changes here changes all.
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

struct Beam {
    float pb[CB_MAXW], pnb[CB_MAXW], sc[CB_MAXW];
    int node[CB_MAXW], last[CB_MAXW], parent[CB_MAXW], len[CB_MAXW];
};

// the LDS of a walking block: 44576 B
struct WalkLds {
    u64 keys[CB_MAXC];
    unsigned dead_words[CB_MAXW * CB_MAXK / 4];                         // one byte per extension (i, k): it was folded into a survivor
    Beam beams[2];
    float tot[CB_MAXW], spb[CB_MAXW], spnb[CB_MAXW], ssc[CB_MAXW], tlp[CB_MAXK];
    int tcls[CB_MAXK], isnew[CB_MAXW], outlen[CB_MAXW];
    u64 surv[CB_MAXW];
    int hist[256], ctl[4], taken, n_next, n_nodes[2];
};

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
__device__ __forceinline__ int walk_frame(WalkLds& L, const WalkIn& q, int cur, int n, long row, long at0, int stamp) {
    const int tid = threadIdx.x, nt = blockDim.x;
    unsigned char* dead = reinterpret_cast<unsigned char*>(L.dead_words);
    const int W = q.W, K = q.K, Kk = q.Kk;
    const unsigned H = q.H;
    int4* arena = q.arena;
    u64* table = q.table;
    const Beam& s = L.beams[cur];
    Beam& nx = L.beams[cur ^ 1];
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
        if (e < n) { v = L.ssc[e]; idx = e; }
        else {
            const int qq = e - n, i = qq / Kk, k = qq - i * Kk;
            idx = W + i * K + k;
            v = dead[i * K + k] ? NEG_INF : (L.tcls[k] == s.last[i] ? s.pb[i] : L.tot[i]) + L.tlp[k];
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
            const float v = ord_value(hi);
            int idx = key_index(my);
            atomicAdd(&L.n_next, 1);
            if (idx < W) {
                idx = idx < n ? idx : 0;                               // (never taken)
                nx.pb[rank] = L.spb[idx]; nx.pnb[rank] = L.spnb[idx]; nx.sc[rank] = v;
                nx.node[rank] = s.node[idx]; nx.last[rank] = s.last[idx]; nx.parent[rank] = s.parent[idx]; nx.len[rank] = s.len[idx];
            } else {
                int i = (idx - W) / K, k = (idx - W) - i * K;
                i = i < n ? i : 0; k = k < Kk ? k : 0;                 // (never taken)
                const int tok = L.tcls[k], par = s.node[i];
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
template <typename TOK>
__device__ __forceinline__ void walk_backtrace(WalkLds& L, const Beam& s, int n, int nbest, int width, const int4* arena, long arena_stride, long pad_id, TOK* tokens,
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

inline size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }
inline long table_words(int T, int W) {
    long h = 2;
    while (h < 2 * (1 + (long)T * W)) h <<= 1;
    return h;
}
inline bool walk_sizes_ok(int T, int W, int V1) { return 1 + (long)T * W < (1l << 22) - 1 && V1 <= (1 << 20); }

}  // namespace
