// One call of a beam stream, ONE definition for the two kernels that run it: ctc_stream_beam_kernel (ctc_beam_stream.hip: B streams in lock-step, one T_call and one
// `final` for all) and ctc_pool_beam_kernel (ctc_beam_pool.hip: the slots of a session pool, each record with rows, `final` and backtrace request of its own).
// ctc_beam_stream.hip's header states what a beam stream is; this file holds the layout of its state (StreamState), what a call reads and writes besides it (StreamIo)
// and the call's body (stream_beam_call): load the beam, walk the call's frames with ctc_walk_step.hpp's frame step, append the committed prefix, spill the beam, and
// on request backtrace the n best.  Both kernels must give the same bits: whatever changes here changes both.
#pragma once
#include <vector>

#include "ctc_walk_step.hpp"

namespace {

constexpr int HDR_WORDS = 16;                                          // n, node count, frames walked, committed node, committed length; the rest is spare
enum { H_N = 0, H_NODES = 1, H_FRAMES = 2, H_CNODE = 3, H_CLEN = 4 };

// the state of B streams (or slots), stream-strided: [headers | beams | arenas | node tables]
struct StreamState {
    int* hdr; Beam* beam;                                              // per stream: HDR_WORDS words; one Beam
    int4* arena; long arena_stride;                                    // per stream: 1 + max_frames W nodes (parent, token, frame, length)
    u64* table; long table_stride;                                     // per stream: the (parent node, token) -> node table, all of it in use
    int max_frames;
};

// what a call reads and writes besides the state: the logits and the cut's tables of this call's rows, the committed buffers (one row per stream) and the n-best rows
struct StreamIo {
    const void* x; long ld_t; int dtype;
    int V1;
    long pad_id;
    int W, K, nbest;
    const float* lse; const float* lpb; const float* cut_lp; const int* cut_id;
    int* committed; int* committed_frames; int* n_committed; int* n_new;
    void* tokens; int* n_tokens; float* scores; int* frames;           // rows of nbest hypotheses, each max_frames wide; frames nullable
};

constexpr int BIAS_SN_WORDS = 2 * CB_MAXW;                             // a biased stream's carried (s, n): 64 + 64 ints, behind the unbiased state
inline size_t stream_head_bytes(int B) { return (size_t)B * (HDR_WORDS * sizeof(int) + sizeof(Beam)); }
inline StreamState stream_state_at(void* state, int B, int max_frames, int W) {
    char* base = (char*)state;
    const long nodes = 1 + (long)max_frames * W, words = table_words(max_frames, W);
    return StreamState{(int*)base, (Beam*)(base + (size_t)B * HDR_WORDS * sizeof(int)), (int4*)(base + stream_head_bytes(B)), nodes,
                       (u64*)(base + stream_head_bytes(B) + align16((size_t)B * nodes * sizeof(int4))), words, max_frames};
}

// stream b back to its start: {(): p_b = 0, p_nb = -inf}, one node (the root), nothing walked, nothing committed.  The node table is the caller's to zero.
__device__ __forceinline__ void stream_start(const StreamState& st, int b) {
    int* h = st.hdr + (long)b * HDR_WORDS;
    h[H_N] = 1; h[H_NODES] = 1; h[H_FRAMES] = 0; h[H_CNODE] = 0; h[H_CLEN] = 0;
    Beam& s = st.beam[b];
    s.pb[0] = 0.f; s.pnb[0] = NEG_INF; s.sc[0] = 0.f; s.node[0] = 0; s.last[0] = -1; s.parent[0] = -1; s.len[0] = 0;
    st.arena[(long)b * st.arena_stride] = make_int4(-1, -1, -1, 0);
}

// One call of stream b (its index into the state and into the committed buffers): walks rows [0, n_rows) of the call — frame t reads the cut's tables at row0 + t and the
// logits at element at0 + t ld_t —, clamped to the frames left below max_frames; `final` appends the rest of the best hypothesis; out >= 0: the n best are backtraced
// into row `out` of io.tokens / n_tokens / scores / frames, out < 0: no backtrace.  Every thread of the block calls it, with the same arguments.
// With TrieBias (ctc_beam_bias_stream.hip) the carried (s, n) of the beam travel with it, from and to bias.sn, and a backtrace also writes the credits.
template <typename TOK, class P>
__device__ __forceinline__ void stream_beam_call(WalkLdsT<P>& L, const StreamState& S, const StreamIo& p, const P& bias, int b, long at0, long row0, int n_rows, int final, int out) {
    const int tid = threadIdx.x;
    const int W = p.W, nbest = p.nbest, MF = S.max_frames;
    int* hdr = S.hdr + (long)b * HDR_WORDS;
    Beam* st = S.beam + b;
    int4* arena = S.arena + (long)b * S.arena_stride;
    u64* table = S.table + (long)b * S.table_stride;
    const int n0 = min(max(hdr[H_N], 0), W), t0 = min(max(hdr[H_FRAMES], 0), MF);
    const int cnode = hdr[H_CNODE], clen = min(max(hdr[H_CLEN], 0), MF);
    const int n_call = min(max(n_rows, 0), MF - t0);                   // never past the arena: 1 + max_frames W nodes

    // ---- the beam, into slot 0
    if (tid < CB_MAXW) {
        BeamT<P>& s = L.beams[0];
        s.pb[tid] = st->pb[tid]; s.pnb[tid] = st->pnb[tid]; s.sc[tid] = st->sc[tid];
        s.node[tid] = st->node[tid]; s.last[tid] = st->last[tid]; s.parent[tid] = st->parent[tid]; s.len[tid] = st->len[tid];
        if constexpr (P::on) { s.bs[tid] = bias.sn[(long)b * BIAS_SN_WORDS + tid]; s.bn[tid] = bias.sn[(long)b * BIAS_SN_WORDS + CB_MAXW + tid]; }
    }
    if (tid == 0) L.n_nodes[0] = hdr[H_NODES];
    __syncthreads();

    // ---- this call's frames
    const WalkIn q{p.x, p.dtype, W, p.K, min(p.K, p.V1 - 1), p.lse, p.lpb, p.cut_lp, p.cut_id, arena, S.arena_stride, table, (unsigned)S.table_stride};
    int n = n0, cur = 0;
    for (int t = 0; t < n_call && n > 0; ++t, cur ^= 1) n = walk_frame(L, q, bias, cur, n, row0 + t, at0 + (long)t * p.ld_t, t0 + t);
    const BeamT<P>& s = L.beams[cur];

    // ---- the committed prefix (wave 0; walk_frame's last barrier has published the beam and the nodes of this call)
    if (tid < 64) {
        int target = cnode, tlen = clen;                               // an empty beam commits nothing more
        if (n > 0) {
            if (final) {                                               // the rest of the best hypothesis
                target = s.node[0]; tlen = s.len[0];
            } else {
                const bool mine = tid < n;
                int nd = mine ? s.node[tid] : 0, len = mine ? s.len[tid] : 0x7FFFFFFF;
                int lo = len;
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) lo = min(lo, __shfl_xor(lo, o, 64));
                for (int d = len; mine && d > lo && nd > 0; --d) nd = arena[nd < S.arena_stride ? nd : 0].x;
                for (int d = lo; d > clen; --d) {                      // together, until every lane stands on the same node
                    const int first = __shfl(nd, 0, 64);
                    if (__ballot(mine && nd != first) == 0ull) break;
                    if (mine && nd > 0) nd = arena[nd < S.arena_stride ? nd : 0].x;
                    --lo;
                }
                target = __shfl(nd, 0, 64); tlen = lo;
            }
        }
        tlen = min(max(tlen, clen), MF);
        if (tid == 0) {
            int nd = target;
            for (int pos = tlen - 1; pos >= clen && nd > 0; --pos) {   // append positions clen .. tlen - 1
                const int4 e = arena[nd < S.arena_stride ? nd : 0];
                p.committed[(long)b * MF + pos] = e.y;
                p.committed_frames[(long)b * MF + pos] = e.z;
                nd = e.x;
            }
            p.n_committed[b] = tlen;
            p.n_new[b] = tlen - clen;
            hdr[H_N] = n; hdr[H_NODES] = L.n_nodes[cur]; hdr[H_FRAMES] = t0 + n_call; hdr[H_CNODE] = tlen > clen ? target : cnode; hdr[H_CLEN] = tlen;
        }
    }
    // ---- the beam, back
    if (tid < CB_MAXW) {
        st->pb[tid] = s.pb[tid]; st->pnb[tid] = s.pnb[tid]; st->sc[tid] = s.sc[tid];
        st->node[tid] = s.node[tid]; st->last[tid] = s.last[tid]; st->parent[tid] = s.parent[tid]; st->len[tid] = s.len[tid];
        if constexpr (P::on) { bias.sn[(long)b * BIAS_SN_WORDS + tid] = s.bs[tid]; bias.sn[(long)b * BIAS_SN_WORDS + CB_MAXW + tid] = s.bn[tid]; }
    }
    // ---- on request the n best, backtraced, in the one-shot entry's format (rows max_frames wide)
    if (out >= 0) {
        walk_backtrace<TOK>(L, s, n, nbest, MF, arena, S.arena_stride, p.pad_id, (TOK*)p.tokens + (long)out * nbest * MF,
                            p.frames ? p.frames + (long)out * nbest * MF : nullptr, p.n_tokens + (long)out * nbest, p.scores + (long)out * nbest);
        if constexpr (P::on) walk_credit(s, n, nbest, bias.credit + (long)out * nbest);
    }
}

inline bool stream_sizes_ok(int B, int max_frames, int W) { return B > 0 && max_frames > 0 && W >= 1 && W <= CB_MAXW && walk_sizes_ok(max_frames, W, 2); }
inline size_t stream_state_bytes(int B, int max_frames, int W) {
    if (!stream_sizes_ok(B, max_frames, W)) return 0;
    return stream_head_bytes(B) + align16((size_t)B * (1 + (size_t)max_frames * W) * sizeof(int4)) + (size_t)B * table_words(max_frames, W) * sizeof(u64);
}
// ... of biased streams: the same state, then per stream the carried (s, n), 2 x 64 ints
inline size_t bias_stream_state_bytes(int B, int max_frames, int W) {
    const size_t plain = stream_state_bytes(B, max_frames, W);
    return plain ? plain + (size_t)B * BIAS_SN_WORDS * sizeof(int) : 0;
}

// the argument check of the lock-step entries (mi_ctc_beam_stream_walk, mi_ctc_beam_bias_stream_walk), then the state's layout and the call's io; `need`: the state's bytes
inline int stream_prepare(const void* logits, long ld_row, int dtype, int B, int T_call, int V1, int blank, long pad_id, int W, int K, int nbest, const float* lse,
                          const float* lp_blank, const float* cut_lp, const int* cut_id, void* state, size_t state_bytes, size_t need, int max_frames, int final, int* committed,
                          int* committed_frames, int* n_committed, int* n_new, void* tokens, int tokens_dtype, int* n_tokens, float* scores, int* frames, StreamState& st,
                          StreamIo& io) {
    if (!state || !committed || !committed_frames || !n_committed || !n_new || B <= 0 || T_call < 0 || max_frames <= 0 || V1 < 2 || W < 1 || W > CB_MAXW || K < 1 ||
        K > CB_MAXK || nbest < 1 || nbest > W || blank < 0 || blank >= V1 || (dtype != 0 && dtype != 1) || (tokens_dtype != 0 && tokens_dtype != 1) ||
        (final != 0 && final != 1))
        return MI_ERR_ARG;
    if (T_call > 0 && (!logits || !lse || !lp_blank || !cut_lp || !cut_id)) return MI_ERR_ARG;
    if (tokens && (!n_tokens || !scores)) return MI_ERR_ARG;
    if (!tokens && (frames || final)) return MI_ERR_ARG;               // the final call always returns the n best
    if (!walk_sizes_ok(max_frames, W, V1)) return MI_ERR_UNSUPPORTED;
    if ((long)B * T_call >= (1l << 31)) return MI_ERR_UNSUPPORTED;
    if (state_bytes < need || (reinterpret_cast<uintptr_t>(state) & 15)) return MI_ERR_ARG;
    st = stream_state_at(state, B, max_frames, W);
    io = StreamIo{logits, ld_row, dtype, V1, pad_id, W, K, nbest, lse, lp_blank, cut_lp, cut_id, committed, committed_frames, n_committed, n_new, tokens, n_tokens, scores, frames};
    return MI_OK;
}

// ... and of the per-slot entries (mi_ctc_beam_stream_walk_slots, mi_ctc_beam_bias_stream_walk_slots): records of five ints [slot, row0, n, final, out]
constexpr int REC_WORDS = 5;
inline int pool_prepare(const void* logits, long ld_row, int dtype, int rows, int V1, int blank, long pad_id, int W, int K, int nbest, const float* lse, const float* lp_blank,
                        const float* cut_lp, const int* cut_id, void* state, size_t state_bytes, size_t need, int S, int max_frames, const int* records_host, int A,
                        const int* records_dev, int* committed, int* committed_frames, int* n_committed, int* n_new, void* tokens, int tokens_dtype, int* n_tokens,
                        float* scores, int* frames, int R, StreamState& st, StreamIo& io) {
    if (!state || !committed || !committed_frames || !n_committed || !n_new || !records_host || !records_dev || S <= 0 || A <= 0 || A > S || rows < 0 || R < 0 || R > A ||
        max_frames <= 0 || V1 < 2 || W < 1 || W > CB_MAXW || K < 1 || K > CB_MAXK || nbest < 1 || nbest > W || blank < 0 || blank >= V1 || (dtype != 0 && dtype != 1) ||
        (tokens_dtype != 0 && tokens_dtype != 1))
        return MI_ERR_ARG;
    if (rows > 0 && (!logits || !lse || !lp_blank || !cut_lp || !cut_id)) return MI_ERR_ARG;
    if (R > 0 && (!tokens || !n_tokens || !scores)) return MI_ERR_ARG;
    if (!tokens && frames) return MI_ERR_ARG;
    if (!walk_sizes_ok(max_frames, W, V1)) return MI_ERR_UNSUPPORTED;
    if (state_bytes < need || (reinterpret_cast<uintptr_t>(state) & 15)) return MI_ERR_ARG;
    std::vector<char> slot_seen(S, 0), out_seen(R, 0);
    for (int i = 0; i < A; ++i) {
        const int* r = records_host + (long)i * REC_WORDS;
        const int slot = r[0], row0 = r[1], n = r[2], final = r[3], out = r[4];
        if (slot < 0 || slot >= S || slot_seen[slot]) return MI_ERR_ARG;
        if (row0 < 0 || n < 0 || (long)row0 + n > rows) return MI_ERR_ARG;
        if ((final != 0 && final != 1) || out < -1 || out >= R || (final && out < 0)) return MI_ERR_ARG;
        if (out >= 0 && out_seen[out]) return MI_ERR_ARG;
        slot_seen[slot] = 1;
        if (out >= 0) out_seen[out] = 1;
    }
    st = stream_state_at(state, S, max_frames, W);
    io = StreamIo{logits, ld_row, dtype, V1, pad_id, W, K, nbest, lse, lp_blank, cut_lp, cut_id, committed, committed_frames, n_committed, n_new, tokens, n_tokens, scores, frames};
    return MI_OK;
}

// a pool kernel's record, read by every thread of its block: false for one the host check would have refused (block-uniform: the block ends before any barrier)
__device__ __forceinline__ bool pool_record(const int* records, int S, int rows, int R, int& slot, int& row0, int& n, int& final, int& out) {
    const int* rec = records + (long)blockIdx.x * REC_WORDS;
    slot = rec[0]; row0 = rec[1]; n = rec[2]; final = rec[3]; out = rec[4];
    return !(slot < 0 || slot >= S || row0 < 0 || n < 0 || (long)row0 + n > rows || out >= R);
}

}  // namespace
