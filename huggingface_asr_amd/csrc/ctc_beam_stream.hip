// Streaming CTC prefix beam search on gfx950: the walk of ctc_beam.hip suspended between calls, with the prefix that can no longer change reported as committed.
//
// ---- Semantics (normative; DESIGN.md §4 'Streaming', 'Beam search on a stream' repeats them)
// Per stream, a *beam stream* is the walk of csrc/ctc_beam.hip ("Semantics", DESIGN §4 'CTC prefix beam search'), suspended between calls.
//   - It has the same token cut, state, frame step, selection and tie rules.  Nothing is approximated and nothing is re-ordered.
//   - Let a stream's frames be delivered over calls 1..k, n_j valid frames in call j, and let t_k = sum of n_j.  After call k the beam is exactly the beam the one-shot
//     walk holds after frame t_k - 1 of the concatenated logits.  This holds for p_b, p_nb, scores, prefixes, ranks and the `frames` stamps, which are global frame
//     indices.
//   - Node ids and the table size may differ from the one-shot walk.  No output depends on them.
//   Committed prefix.  stable_k is the longest common prefix of ALL hypotheses in the beam after call k.  It covers all n <= W of them, not only the nbest.
//   - stable_k is a prefix of stable_{k+1}.  Every member of the next beam is a survivor or an extension of a member of this one, hence a descendant of their common
//     ancestor in the trie.
//   - Tokens are appended to a per-stream, append-only `committed` buffer.  A parallel `committed_frames` buffer holds each token's entry frame.  `n_committed` counts
//     them.
//   - An empty beam (all scores -inf: the one-shot walk stops there too) commits nothing more.
//   - In the FINAL call (final = 1) the rest of the best hypothesis is appended after the last frame.  Then committed[:n_committed] equals the best hypothesis, and
//     committed_frames equals its `frames`.
//   - A stream with zero frames in total yields the empty hypothesis with score 0.
//   Outputs.  Every call returns n_committed (B) and the number of tokens newly appended, n_new (B); on request (tokens not null: `partial`, or always in the final
//   call) the nbest hypotheses in the one-shot entry's format: tokens (B, nbest, max_frames) int32 | int64 padded with pad_id, n_tokens, scores, and optional frames.
//   Non-existent rows are 0 tokens, -inf, pad / -1.  Without that request the call does no backtrace: its cost then does not grow with the utterance.
//   Guarantees kept from the one-shot kernel.  No float atomics.  Two runs are bit-identical.  A stream's result does not depend on the rest of the batch.  A call
//   with 0 valid frames for a stream leaves that stream's state untouched (the beam is written back as it was read).
//
// ---- Entries
//   mi_ctc_beam_stream_state_bytes(B, max_frames, W): host arithmetic, no device needed; 0 for refused arguments.  Per stream: a header of 16 words (beam count n,
//     node count, frames walked, the committed node and its length), the Beam record (7 x 64 words), the node arena (1 + max_frames W nodes of 16 B) and the node table
//     (table_words(max_frames, W) 64-bit words, the power of two >= 2 (1 + max_frames W)):
//       bytes = B (64 + 1792) + align16(16 B (1 + max_frames W)) + 8 B table_words(max_frames, W)
//   mi_ctc_beam_stream_reset: zeroes the state (the node table with it: the walk never clears it) and writes the start {(): p_b = 0, p_nb = -inf} of every stream.
//   mi_ctc_beam_stream_walk: the logits and mi_ctc_beam_cut's tables of THIS call's rows (B, T_call[, K]); n_valid (B, nullable) valid rows per stream, clamped to
//     [0, T_call] and to the frames left below max_frames, so the arena can never be overrun (the host refuses such a call first).  T_call = 0 is a call without
//     frames (the logits and tables may be null): it recomputes the counts and, with final = 1, closes the stream.
//   Limits: those of the one-shot walk with T = max_frames; max_frames W < 2^22 - 2, else MI_ERR_UNSUPPORTED; argument errors MI_ERR_ARG before any launch.
//   The per-slot form for a session pool — the same state with B = slots, every slot with rows, `final` and start of its own — is csrc/ctc_beam_pool.hip
//   (mi_ctc_beam_stream_reset_slot, mi_ctc_beam_stream_walk_slots); a call's body is ONE definition for both, ctc_beam_stream_body.hpp.
//
// ---- ctc_stream_beam_kernel: one block per stream, 256 threads when W (min(K, V1 - 1) + 1) <= 1024, else 1024, as the one-shot launch.  The body of a call
// is ctc_beam_stream_body.hpp's stream_beam_call, here with (b, b T, n_valid[b], final, b).  The beam is loaded from the state into LDS slot 0 (the ping-pong parity is not state), the call's frames are walked with ctc_walk_step.hpp's frame step — the one-shot kernel's own — and the
// beam is spilled back.  Table accesses stay agent-scope atomics; the kernel boundary orders them, the arena and the state between calls.  Committed prefix: wave 0,
// one lane per hypothesis; each lane climbs its chain to the minimum length, then all lanes climb together (ballot) until their nodes agree; lane 0 appends the tokens
// between the old committed node and the new one.  All hypotheses descend from the old committed node, so the work is bounded by the un-committed tail, not by the
// utterance.  Every loop is bounded by T_call, W, K, max_frames or the table size; no block waits on another.
//
// Budget (hipcc --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage; tests/test_stream_beam_cpu.py reads it from the built code object):
//   ctc_stream_beam_kernel   256 or 1024 threads, <= 128 VGPRs, 44576 B of LDS (the one-shot walk's: candidate keys, merge flags, the two beams); no scratch
#include "common.hpp"
#include "radix_select.hpp"
#include "ctc_beam_stream_body.hpp"
#include "../../include/hfasr_hip.h"

namespace {

struct StreamArgs {
    StreamState st; StreamIo io;
    long ld_b;
    int B, T;                                                          // T: the rows of this call
    const int* n_valid;
    int final;
};

__global__ __launch_bounds__(64) void ctc_stream_reset_kernel(StreamState st, int B) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b < B) stream_start(st, b);
}

template <typename TOK>
__global__ __launch_bounds__(1024) void ctc_stream_beam_kernel(StreamArgs p) {
    __shared__ WalkLds L;
    const int b = blockIdx.x, T = p.T;
    const int n_call = p.n_valid ? min(max(p.n_valid[b], 0), T) : T;
    stream_beam_call<TOK>(L, p.st, p.io, NoBias{}, b, (long)b * p.ld_b, (long)b * T, n_call, p.final, p.io.tokens ? b : -1);
}

}  // namespace

extern "C" size_t mi_ctc_beam_stream_state_bytes(int B, int max_frames, int W) {
    return stream_state_bytes(B, max_frames, W);
}

extern "C" int mi_ctc_beam_stream_reset(void* state, size_t state_bytes, int B, int max_frames, int W, hipStream_t stream) {
    MI_ENTER();
    if (!state || B <= 0 || max_frames <= 0 || W < 1 || W > CB_MAXW) return MI_ERR_ARG;
    if (!walk_sizes_ok(max_frames, W, 2)) return MI_ERR_UNSUPPORTED;
    const size_t need = mi_ctc_beam_stream_state_bytes(B, max_frames, W);
    if (state_bytes < need || (reinterpret_cast<uintptr_t>(state) & 15)) return MI_ERR_ARG;
    if (hipMemsetAsync(state, 0, need, stream) != hipSuccess) return MI_ERR_LAUNCH;
    hipLaunchKernelGGL(ctc_stream_reset_kernel, dim3((B + 63) / 64), dim3(64), 0, stream, stream_state_at(state, B, max_frames, W), B);
    MI_CHECK_LAUNCH();
    return MI_OK;
}

extern "C" int mi_ctc_beam_stream_walk(const void* logits, long ld_row, long ld_batch, int dtype, int B, int T_call, int V1, const int* n_valid, int blank, long pad_id,
                                       int W, int K, int nbest, const float* lse, const float* lp_blank, const float* cut_lp, const int* cut_id, void* state,
                                       size_t state_bytes, int max_frames, int final, int* committed, int* committed_frames, int* n_committed, int* n_new,
                                       void* tokens, int tokens_dtype, int* n_tokens, float* scores, int* frames, hipStream_t stream) {
    MI_ENTER();
    StreamArgs a{};
    const int rc = stream_prepare(logits, ld_row, dtype, B, T_call, V1, blank, pad_id, W, K, nbest, lse, lp_blank, cut_lp, cut_id, state, state_bytes,
                                  stream_state_bytes(B, max_frames, W), max_frames, final, committed, committed_frames, n_committed, n_new, tokens, tokens_dtype, n_tokens,
                                  scores, frames, a.st, a.io);
    if (rc != MI_OK) return rc;
    a.ld_b = ld_batch; a.B = B; a.T = T_call; a.n_valid = n_valid; a.final = final;
    const dim3 block = walk_block(W, K, V1);
    if (tokens_dtype == 0) hipLaunchKernelGGL(ctc_stream_beam_kernel<int>, dim3(B), block, 0, stream, a);
    else hipLaunchKernelGGL(ctc_stream_beam_kernel<long>, dim3(B), block, 0, stream, a);
    MI_CHECK_LAUNCH();
    return MI_OK;
}
