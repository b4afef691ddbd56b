// Contextual biasing on the slots of a session pool, gfx950: the per-slot beam stream of ctc_beam_pool.hip with the bias policy of ctc_beam_bias.hip; both headers stay
// normative.  One context per pool, shared by all slots.  A session's beam is bit for bit that of a biased lock-step stream of batch 1 (ctc_beam_bias_stream.hip) fed
// the same pieces with the same context, whatever the other slots do.
//
// ---- State.  mi_ctc_beam_bias_stream_state_bytes(S, max_frames, W), slot-strided: the unbiased state, then per slot the carried (s, n), 2 x 64 ints.
//
// ---- Entries
//   mi_ctc_beam_bias_stream_reset_slot: mi_ctc_beam_stream_reset_slot on the unbiased part, and the slot's carried (s, n) zeroed (a second memset, 512 B).  No other slot
//     is touched.
//   mi_ctc_beam_bias_stream_walk_slots: mi_ctc_beam_stream_walk_slots' arguments, then the context (bias_col (V1), bias_tab (S_bias, A1), S_bias, A1, weight) and
//     credit (R, nbest) int32, a row beside every row of scores; rows that do not exist hold 0.  MI_ERR_ARG before any launch: whatever mi_ctc_beam_stream_walk_slots
//     refuses, null tables, S_bias, A1 or their product outside 1..4096, 1..1024, <= 2^20, a weight that is not finite, R > 0 without credit.
//
// ---- ctc_bias_pool_beam: ctc_pool_beam_kernel with the policy: one block per record, the record read and checked the same way, then stream_beam_call.
//
// Budget (hipcc --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage; tests/test_ctc_bias_cpu.py reads it from the built code object):
//   ctc_bias_pool_beam   256 or 1024 threads, <= 128 VGPRs, 45600 B of LDS (ctc_bias_walk's); no scratch
#include "common.hpp"
#include "radix_select.hpp"
#include "ctc_beam_stream_body.hpp"
#include "../../include/hfasr_hip.h"

namespace {

struct BiasPoolArgs {
    StreamState st; StreamIo io;
    const int* records;
    int S, rows, R;
};

template <typename TOK>
__global__ __launch_bounds__(1024) void ctc_bias_pool_beam(BiasPoolArgs p, TrieBias bias) {
    __shared__ WalkLdsT<TrieBias> L;
    int slot, row0, n, final, out;
    if (!pool_record(p.records, p.S, p.rows, p.R, slot, row0, n, final, out)) return;      // (the host has refused it: block-uniform, before any barrier)
    stream_beam_call<TOK>(L, p.st, p.io, bias, slot, (long)row0 * p.io.ld_t, row0, n, final != 0, out);
}

}  // namespace

extern "C" int mi_ctc_beam_bias_stream_reset_slot(void* state, size_t state_bytes, int S, int max_frames, int W, int slot, hipStream_t stream) {
    MI_ENTER();
    const size_t plain = stream_state_bytes(S, max_frames, W);
    if (plain && state_bytes < bias_stream_state_bytes(S, max_frames, W)) return MI_ERR_ARG;
    const int rc = mi_ctc_beam_stream_reset_slot(state, state_bytes, S, max_frames, W, slot, stream);        // (refuses what is left to refuse)
    if (rc != MI_OK) return rc;
    if (hipMemsetAsync((char*)state + plain + (size_t)slot * BIAS_SN_WORDS * sizeof(int), 0, BIAS_SN_WORDS * sizeof(int), stream) != hipSuccess) return MI_ERR_LAUNCH;
    return MI_OK;
}

extern "C" int mi_ctc_beam_bias_stream_walk_slots(const void* logits, long ld_row, int dtype, int rows, int V1, int blank, long pad_id, int W, int K, int nbest,
                                                  const float* lse, const float* lp_blank, const float* cut_lp, const int* cut_id, void* state, size_t state_bytes, int S,
                                                  int max_frames, const int* records_host, int A, const int* records_dev, int* committed, int* committed_frames,
                                                  int* n_committed, int* n_new, void* tokens, int tokens_dtype, int* n_tokens, float* scores, int* frames, int R,
                                                  const int* bias_col, const int* bias_tab, int S_bias, int A1, float weight, int* credit, hipStream_t stream) {
    MI_ENTER();
    if (!bias_args_ok(bias_col, bias_tab, S_bias, A1, weight) || (R > 0 && !credit)) return MI_ERR_ARG;
    BiasPoolArgs a{};
    const int rc = pool_prepare(logits, ld_row, dtype, rows, V1, blank, pad_id, W, K, nbest, lse, lp_blank, cut_lp, cut_id, state, state_bytes,
                                bias_stream_state_bytes(S, max_frames, W), S, max_frames, records_host, A, records_dev, committed, committed_frames, n_committed, n_new,
                                tokens, tokens_dtype, n_tokens, scores, frames, R, a.st, a.io);
    if (rc != MI_OK) return rc;
    a.records = records_dev; a.S = S; a.rows = rows; a.R = R;
    const TrieBias bias{bias_col, bias_tab, S_bias, A1, V1, weight, (int*)((char*)state + stream_state_bytes(S, max_frames, W)), credit};
    const dim3 block = walk_block(W, K, V1);
    if (tokens_dtype == 0) hipLaunchKernelGGL(ctc_bias_pool_beam<int>, dim3(A), block, 0, stream, a, bias);
    else hipLaunchKernelGGL(ctc_bias_pool_beam<long>, dim3(A), block, 0, stream, a, bias);
    MI_CHECK_LAUNCH();
    return MI_OK;
}
