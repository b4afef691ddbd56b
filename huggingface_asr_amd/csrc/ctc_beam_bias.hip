// Contextual biasing of the CTC prefix beam search on gfx950: the search of ctc_beam.hip with a phrase list ("hotwords") whose matches raise a hypothesis' rank.
//
// ---- Semantics (normative; DESIGN.md §4 'Contextual biasing' repeats them)
// Phrase list.  A bias context is a list of phrases and one weight w.
//   Phrase      a non-empty list of token ids, each in [0, V1) and not `blank`.  Duplicate phrases count once.
//   Weight      a finite fp32 value, in log-probability units per credited token.  A negative weight is allowed.
// Credit.  The credit n(l) of a label sequence l is an integer, defined by walking l through the phrase trie.  depth(s) is the depth of trie node s; fail(s) the
//   Aho-Corasick failure link, the deepest node whose string is a proper suffix of s's string; keep(s) the depth of the deepest phrase end on the path root -> s, s
//   included, 0 if there is none.  The walk state is (s, k) and starts at (root, 0).  For each token c:
//     1. if s has a child for c: s <- child(s, c), k unchanged;
//     2. otherwise, if keep(s) > 0: k <- k + keep(s), s <- root (the completed phrase stays, the tokens after it are given back);
//     3. otherwise: while s != root and s has no child for c, s <- fail(s) (nothing is kept);
//     4. after step 2 or 3: if s has a child for c, s <- child(s, c).
//   Then n(l) = k + depth(s).  A partial match earns a provisional credit of one per token, withdrawn when the match breaks; a phrase that occurs only as a suffix
//   of a longer partial match is not credited; 0 <= n(l) <= len(l).
// Search.  All of ctc_beam.hip's semantics stay (state, frame step, merge, tie rules).  One thing changes: the value a candidate is selected and ranked by.  Unbiased
//   it is score = p_b (+) p_nb; biased it is score + w (float)n(prefix): one fp32 multiply and one fp32 add, -inf stays -inf.  For an extension (i, k), n comes from
//   hypothesis i's carried (s, n) and the token; for a survivor it is the carried n.  The merge is unaffected: a survivor and the extension it absorbs are the same
//   prefix, so they have the same n.
// Outputs.  `scores` stays the CTC log-probability p_b (+) p_nb, not the biased value.  A new output credit (..., nbest) int32 holds n per hypothesis; rows that do not
//   exist hold 0.  The n-best order is the biased order.  The committed-prefix rule of the stream and pool forms is unchanged.  With w = 0, or with an empty phrase
//   list, every output equals the unbiased search's, bit for bit.
//
// ---- Tables (huggingface_asr_amd/ctc_bias.py compiles them).  n' - n depends on (s, c) alone, so the walk is a table: col (V1) int32 maps a token to its alphabet
// column, 0 = "in no phrase"; tab (S, A1) int32 holds per (state, column) the word (dn << 16) | next, dn = n' - n an int16, next < S; the root is state 0.
// 1 <= S <= 4096, 1 <= A1 <= 1024, S A1 <= 2^20 (4 MiB: L2-resident).  The kernel clamps what it reads — the token into [0, V1), the column into [0, A1), a state into
// [0, S) — so no table content can cause an access outside the tables: a malformed context gives a wrong answer, never a fault.
//
// ---- ctc_bias_walk: ctc_walk_kernel (ctc_beam.hip, launch B) with the bias policy of ctc_walk_step.hpp: the same utterance walk, frame step and backtrace, one
// definition for both.  A hypothesis carries two more ints (s, n) in both beams.  Per extension candidate the step reads col[tok] and tab[s A1 + col], two dependent
// 4-byte loads, for the value in its key, and again for the <= W selected ones, whose CTC score is recomputed (the key holds the biased value); there is no new barrier.
// Launch A, the cut, is mi_ctc_beam_cut as it is.  The stream and pool forms are ctc_beam_bias_stream.hip and ctc_beam_bias_pool.hip.
//
// Budget (hipcc --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage; tests/test_ctc_bias_cpu.py reads it from the built code object):
//   ctc_bias_walk   256 or 1024 threads, <= 128 VGPRs, 45600 B of LDS (the unbiased walk's 44576 B and 2 x 2 x 64 ints of carried (s, n)); no scratch
#include "common.hpp"
#include "radix_select.hpp"
#include "ctc_walk_step.hpp"
#include "../../include/hfasr_hip.h"

namespace {

template <typename TOK>
__global__ __launch_bounds__(1024) void ctc_bias_walk(WalkArgs p, TrieBias bias) {
    __shared__ WalkLdsT<TrieBias> L;
    int n;
    const BeamT<TrieBias>& s = walk_utterance<TOK>(L, p, bias, blockIdx.x, n);
    walk_credit(s, n, p.nbest, bias.credit + (long)blockIdx.x * p.nbest);
}

}  // namespace

extern "C" int mi_ctc_beam_walk_bias(const void* logits, long ld_row, long ld_batch, int dtype, int B, int T, int V1, const int* lengths, int blank, long pad_id, int W, int K,
                                     int nbest, const float* lse, const float* lp_blank, const float* cut_lp, const int* cut_id, void* workspace, size_t workspace_bytes,
                                     void* tokens, int tokens_dtype, int* n_tokens, float* scores, int* frames, const int* bias_col, const int* bias_tab, int S, int A1,
                                     float weight, int* credit, hipStream_t stream) {
    MI_ENTER();
    if (!bias_args_ok(bias_col, bias_tab, S, A1, weight) || !credit) return MI_ERR_ARG;
    WalkArgs a;
    dim3 block;
    const int rc = walk_prepare(logits, ld_row, ld_batch, dtype, B, T, V1, lengths, blank, pad_id, W, K, nbest, lse, lp_blank, cut_lp, cut_id, workspace, workspace_bytes,
                                mi_ctc_beam_workspace_bytes(B, T, W), tokens, tokens_dtype, n_tokens, scores, frames, a, block);
    if (rc != MI_OK) return rc;
    const TrieBias bias{bias_col, bias_tab, S, A1, V1, weight, nullptr, credit};
    if (tokens_dtype == 0) hipLaunchKernelGGL(ctc_bias_walk<int>, dim3(B), block, 0, stream, a, bias);
    else hipLaunchKernelGGL(ctc_bias_walk<long>, dim3(B), block, 0, stream, a, bias);
    MI_CHECK_LAUNCH();
    return MI_OK;
}
