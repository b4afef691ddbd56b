// One call of a beam stream, ONE definition for the two kernels that run it: ctc_stream_beam_kernel (ctc_beam_stream.hip: B streams in lock-step, one T_call and one
// `final` for all) and ctc_pool_beam_kernel (ctc_beam_pool.hip: the slots of a session pool, each record with rows, `final` and backtrace request of its own).
// ctc_beam_stream.hip's header states what a beam stream is; this file holds the layout of its state (StreamState), what a call reads and writes besides it (StreamIo)
// and the call's body (stream_beam_call): load the beam, walk the call's frames with ctc_walk_step.hpp's frame step, append the committed prefix, spill the beam, and
// on request backtrace the n best.  Both kernels must give the same bits: whatever changes here changes both.
#pragma once
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
template <typename TOK>
__device__ __forceinline__ void stream_beam_call(WalkLds& L, const StreamState& S, const StreamIo& p, int b, long at0, long row0, int n_rows, int final, int out) {
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
        Beam& s = L.beams[0];
        s.pb[tid] = st->pb[tid]; s.pnb[tid] = st->pnb[tid]; s.sc[tid] = st->sc[tid];
        s.node[tid] = st->node[tid]; s.last[tid] = st->last[tid]; s.parent[tid] = st->parent[tid]; s.len[tid] = st->len[tid];
    }
    if (tid == 0) L.n_nodes[0] = hdr[H_NODES];
    __syncthreads();

    // ---- this call's frames
    const WalkIn q{p.x, p.dtype, W, p.K, min(p.K, p.V1 - 1), p.lse, p.lpb, p.cut_lp, p.cut_id, arena, S.arena_stride, table, (unsigned)S.table_stride};
    int n = n0, cur = 0;
    for (int t = 0; t < n_call && n > 0; ++t, cur ^= 1) n = walk_frame(L, q, cur, n, row0 + t, at0 + (long)t * p.ld_t, t0 + t);
    const Beam& s = L.beams[cur];

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
    }
    // ---- on request the n best, backtraced, in the one-shot entry's format (rows max_frames wide)
    if (out >= 0)
        walk_backtrace<TOK>(L, s, n, nbest, MF, arena, S.arena_stride, p.pad_id, (TOK*)p.tokens + (long)out * nbest * MF,
                            p.frames ? p.frames + (long)out * nbest * MF : nullptr, p.n_tokens + (long)out * nbest, p.scores + (long)out * nbest);
}

inline bool stream_sizes_ok(int B, int max_frames, int W) { return B > 0 && max_frames > 0 && W >= 1 && W <= CB_MAXW && walk_sizes_ok(max_frames, W, 2); }

}  // namespace
