// CTC prefix beam search on the slots of a session pool, gfx950: the beam stream of ctc_beam_stream.hip per slot — each with its own rows, its own end and its own
// start.  ctc_beam_stream.hip's header stays normative for what a beam stream is; a call's body is its own (ctc_beam_stream_body.hpp), so a session's beam is bit for
// bit the beam of a lock-step stream of batch 1 fed the same pieces, and through it mi_ctc_beam_walk's on the concatenated logits.
//
// ---- Semantics
//   State.  That of the lock-step streams with B = S slots: the same layout, the same mi_ctc_beam_stream_state_bytes(S, max_frames, W).  It is slot-strided.
//   Records.  A call names A slots, each with a record of five ints [slot, row0, n, final, out]:
//     row0, n  the slot's rows in this step's compact logits (rows, V1) — row stride ld_row — and in mi_ctc_beam_cut's tables computed over those same compact rows
//              (one call with B = 1, T = rows, ld_batch = 0; skipped when rows = 0).  n = 0 is a call without frames.
//     final    1 closes the slot's stream: the rest of the best hypothesis is appended to the committed prefix.  final = 1 requires out >= 0.
//     out      >= 0: the row of the n-best outputs (tokens (R, nbest, max_frames), n_tokens / scores (R, nbest), frames) to backtrace into; -1: no backtrace.
//   - The frames already walked come from the slot's header.  n is clamped to the frames left below max_frames, so the arena can never be overrun (the host refuses such
//     a call first).
//   - n = 0 leaves the slot's beam as read; with final = 1 it closes the stream.  A session with zero frames in total gives the empty hypothesis with score 0.
//   - committed / committed_frames (S, max_frames) and n_committed / n_new (S) are indexed by slot.
//   - Nothing of a slot that no record names is read or written: not its state, its committed row or its counts.
//   - No float atomics.  Two runs are bit-identical.  A slot's result does not depend on the other records, on the record order or on its slot index.
//
// ---- Entries
//   mi_ctc_beam_stream_reset_slot: one slot back to a stream start on the caller's stream, no synchronisation: its header, start beam {(): p_b = 0, p_nb = -inf} and arena
//     root are written (one launch) and ITS node table is zeroed (one memset: the walk never clears it).  No other slot is touched.  The memset is
//     8 table_words(max_frames, W) bytes per open: 256 KiB at max_frames = 1500, W = 10; 2 MiB at W = 64.  The committed row and counts are the caller's to clear.
//   mi_ctc_beam_stream_walk_slots: the records come twice, as the pool's tables do: records_host is checked here, records_dev (the same 5 A ints on the device) is what
//     the kernel reads.  MI_ERR_ARG before any launch: a slot out of [0, S) or named twice; row0 / n negative or row0 + n > rows; final outside {0, 1}; out outside
//     [-1, R) or used twice; final without out; rows > 0 without logits or tables; R > 0 without tokens / n_tokens / scores; and whatever mi_ctc_beam_stream_walk
//     refuses.  MI_ERR_UNSUPPORTED as mi_ctc_beam_stream_walk.
//
// ---- ctc_pool_beam_kernel: one block per record, 256 threads when W (min(K, V1 - 1) + 1) <= 1024, else 1024, as the lock-step launch.  The block reads its record
// (block-uniform; a record the host check would have refused ends the block before its first barrier), then runs stream_beam_call with
// (slot, row0, n, final, out).  Blocks share nothing: every slot's header, beam, arena and table are its own, and a slot appears in one record.
//
// Budget (hipcc --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage; tests/test_stream_pool_beam_cpu.py reads it from the built code object):
//   ctc_pool_beam_kernel   256 or 1024 threads, <= 128 VGPRs, 44576 B of LDS (the lock-step kernel's); no scratch
#include "common.hpp"
#include "radix_select.hpp"
#include "ctc_beam_stream_body.hpp"
#include "../../include/hfasr_hip.h"

namespace {

struct PoolArgs {
    StreamState st; StreamIo io;
    const int* records;
    int S, rows, R;
};

__global__ __launch_bounds__(64) void ctc_pool_reset_slot_kernel(StreamState st, int slot) {
    const int tid = threadIdx.x;
    int* h = st.hdr + (long)slot * HDR_WORDS;
    Beam& s = st.beam[slot];
    if (tid < HDR_WORDS) h[tid] = 0;
    s.pb[tid] = 0.f; s.pnb[tid] = 0.f; s.sc[tid] = 0.f; s.node[tid] = 0; s.last[tid] = 0; s.parent[tid] = 0; s.len[tid] = 0;      // (as the whole-state reset leaves them)
    __syncthreads();
    if (tid == 0) stream_start(st, slot);
}

template <typename TOK>
__global__ __launch_bounds__(1024) void ctc_pool_beam_kernel(PoolArgs p) {
    __shared__ WalkLds L;
    int slot, row0, n, final, out;
    if (!pool_record(p.records, p.S, p.rows, p.R, slot, row0, n, final, out)) return;      // (the host has refused it: block-uniform, before any barrier)
    stream_beam_call<TOK>(L, p.st, p.io, NoBias{}, slot, (long)row0 * p.io.ld_t, row0, n, final != 0, out);
}

}  // namespace

extern "C" int mi_ctc_beam_stream_reset_slot(void* state, size_t state_bytes, int S, int max_frames, int W, int slot, hipStream_t stream) {
    MI_ENTER();
    if (!state || S <= 0 || max_frames <= 0 || W < 1 || W > CB_MAXW || slot < 0 || slot >= S) return MI_ERR_ARG;
    if (!walk_sizes_ok(max_frames, W, 2)) return MI_ERR_UNSUPPORTED;
    if (state_bytes < mi_ctc_beam_stream_state_bytes(S, max_frames, W) || (reinterpret_cast<uintptr_t>(state) & 15)) return MI_ERR_ARG;
    const StreamState st = stream_state_at(state, S, max_frames, W);
    if (hipMemsetAsync(st.table + (size_t)slot * st.table_stride, 0, (size_t)st.table_stride * sizeof(u64), stream) != hipSuccess) return MI_ERR_LAUNCH;
    hipLaunchKernelGGL(ctc_pool_reset_slot_kernel, dim3(1), dim3(CB_MAXW), 0, stream, st, slot);
    MI_CHECK_LAUNCH();
    return MI_OK;
}

extern "C" int mi_ctc_beam_stream_walk_slots(const void* logits, long ld_row, int dtype, int rows, int V1, int blank, long pad_id, int W, int K, int nbest, const float* lse,
                                             const float* lp_blank, const float* cut_lp, const int* cut_id, void* state, size_t state_bytes, int S, int max_frames,
                                             const int* records_host, int A, const int* records_dev, int* committed, int* committed_frames, int* n_committed, int* n_new,
                                             void* tokens, int tokens_dtype, int* n_tokens, float* scores, int* frames, int R, hipStream_t stream) {
    MI_ENTER();
    PoolArgs a{};
    const int rc = pool_prepare(logits, ld_row, dtype, rows, V1, blank, pad_id, W, K, nbest, lse, lp_blank, cut_lp, cut_id, state, state_bytes,
                                stream_state_bytes(S, max_frames, W), S, max_frames, records_host, A, records_dev, committed, committed_frames, n_committed, n_new, tokens,
                                tokens_dtype, n_tokens, scores, frames, R, a.st, a.io);
    if (rc != MI_OK) return rc;
    a.records = records_dev; a.S = S; a.rows = rows; a.R = R;
    const dim3 block = walk_block(W, K, V1);
    if (tokens_dtype == 0) hipLaunchKernelGGL(ctc_pool_beam_kernel<int>, dim3(A), block, 0, stream, a);
    else hipLaunchKernelGGL(ctc_pool_beam_kernel<long>, dim3(A), block, 0, stream, a);
    MI_CHECK_LAUNCH();
    return MI_OK;
}
