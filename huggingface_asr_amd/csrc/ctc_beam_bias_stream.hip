// Contextual biasing on a beam stream, gfx950: the beam stream of ctc_beam_stream.hip with the bias policy of ctc_beam_bias.hip.  Those two headers stay normative:
// what a beam stream is (the walk suspended between calls, the committed prefix, the outputs) and what the bias changes (the value a candidate is selected and ranked by,
// the credit).  After every call the beam is bit for bit the beam mi_ctc_beam_walk_bias holds after the same frames of the concatenated logits, with the same context.
//
// ---- State.  That of the unbiased streams, unchanged and at the same offsets, then per stream the carried (s, n) of its <= 64 hypotheses, 2 x 64 ints:
//       mi_ctc_beam_bias_stream_state_bytes(B, max_frames, W) = mi_ctc_beam_stream_state_bytes(B, max_frames, W) + 512 B
// Only a biased state grows; the context (tables and weight) is an argument of every walk, not state, and must be the same from a stream's start to its end.
//
// ---- Entries
//   mi_ctc_beam_bias_stream_reset: mi_ctc_beam_stream_reset on the unbiased part, and the carried (s, n) zeroed: every hypothesis at the automaton's root, no credit.
//   mi_ctc_beam_bias_stream_walk: mi_ctc_beam_stream_walk's arguments, then the context (bias_col (V1), bias_tab (S, A1), S, A1, weight) and credit (B, nbest) int32,
//     written wherever the n best are (tokens not null); rows that do not exist hold 0.  MI_ERR_ARG before any launch: whatever mi_ctc_beam_stream_walk refuses, null
//     tables, S, A1 or S A1 outside 1..4096, 1..1024, <= 2^20, a weight that is not finite, tokens without credit.
//
// ---- ctc_bias_stream_beam: ctc_stream_beam_kernel with the policy; a call's body is ctc_beam_stream_body.hpp's stream_beam_call, the one definition of all four
// stream and pool kernels.  The carried (s, n) are loaded and spilled with the beam.
//
// Budget (hipcc --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage; tests/test_ctc_bias_cpu.py reads it from the built code object):
//   ctc_bias_stream_beam   256 or 1024 threads, <= 128 VGPRs, 45600 B of LDS (ctc_bias_walk's); no scratch
#include "common.hpp"
#include "radix_select.hpp"
#include "ctc_beam_stream_body.hpp"
#include "../../include/hfasr_hip.h"

namespace {

struct BiasStreamArgs {
    StreamState st; StreamIo io;
    long ld_b;
    int B, T;                                                          // T: the rows of this call
    const int* n_valid;
    int final;
};

template <typename TOK>
__global__ __launch_bounds__(1024) void ctc_bias_stream_beam(BiasStreamArgs p, TrieBias bias) {
    __shared__ WalkLdsT<TrieBias> L;
    const int b = blockIdx.x, T = p.T;
    const int n_call = p.n_valid ? min(max(p.n_valid[b], 0), T) : T;
    stream_beam_call<TOK>(L, p.st, p.io, bias, b, (long)b * p.ld_b, (long)b * T, n_call, p.final, p.io.tokens ? b : -1);
}

}  // namespace

extern "C" size_t mi_ctc_beam_bias_stream_state_bytes(int B, int max_frames, int W) { return bias_stream_state_bytes(B, max_frames, W); }

extern "C" int mi_ctc_beam_bias_stream_reset(void* state, size_t state_bytes, int B, int max_frames, int W, hipStream_t stream) {
    MI_ENTER();
    const size_t plain = stream_state_bytes(B, max_frames, W), need = bias_stream_state_bytes(B, max_frames, W);
    if (plain && state_bytes < need) return MI_ERR_ARG;
    const int rc = mi_ctc_beam_stream_reset(state, state_bytes, B, max_frames, W, stream);                   // (refuses what is left to refuse)
    if (rc != MI_OK) return rc;
    if (hipMemsetAsync((char*)state + plain, 0, need - plain, stream) != hipSuccess) return MI_ERR_LAUNCH;
    return MI_OK;
}

extern "C" int mi_ctc_beam_bias_stream_walk(const void* logits, long ld_row, long ld_batch, int dtype, int B, int T_call, int V1, const int* n_valid, int blank, long pad_id,
                                            int W, int K, int nbest, const float* lse, const float* lp_blank, const float* cut_lp, const int* cut_id, void* state,
                                            size_t state_bytes, int max_frames, int final, int* committed, int* committed_frames, int* n_committed, int* n_new,
                                            void* tokens, int tokens_dtype, int* n_tokens, float* scores, int* frames, const int* bias_col, const int* bias_tab, int S,
                                            int A1, float weight, int* credit, hipStream_t stream) {
    MI_ENTER();
    if (!bias_args_ok(bias_col, bias_tab, S, A1, weight) || (tokens && !credit)) return MI_ERR_ARG;
    BiasStreamArgs a{};
    const int rc = stream_prepare(logits, ld_row, dtype, B, T_call, V1, blank, pad_id, W, K, nbest, lse, lp_blank, cut_lp, cut_id, state, state_bytes,
                                  bias_stream_state_bytes(B, max_frames, W), max_frames, final, committed, committed_frames, n_committed, n_new, tokens, tokens_dtype,
                                  n_tokens, scores, frames, a.st, a.io);
    if (rc != MI_OK) return rc;
    a.ld_b = ld_batch; a.B = B; a.T = T_call; a.n_valid = n_valid; a.final = final;
    const TrieBias bias{bias_col, bias_tab, S, A1, V1, weight, (int*)((char*)state + stream_state_bytes(B, max_frames, W)), credit};
    const dim3 block = walk_block(W, K, V1);
    if (tokens_dtype == 0) hipLaunchKernelGGL(ctc_bias_stream_beam<int>, dim3(B), block, 0, stream, a, bias);
    else hipLaunchKernelGGL(ctc_bias_stream_beam<long>, dim3(B), block, 0, stream, a, bias);
    MI_CHECK_LAUNCH();
    return MI_OK;
}
