// The stream step, written once: what mi_ebf_stream_step (stream.hip, B streams in lock-step) and mi_ebf_stream_step_slots (stream_pool.hip, the active slots of a
// pool) enqueue, staged as encoder.hip's forward is.  Everything row-wise — GEMMs, LayerNorms, row statistics, the gate, the head, the argmax — runs on "the rows of
// this step at entry l", compact, and does not know whose rows they are.  What knows where a stream stands goes through `Pos`, a policy resolved at compile time, one
// instance per translation unit: LockStep (stream.hip) answers with the batch-wide scalars of the step's plan, PerSlot (stream_pool.hip) with sections of the step's
// descriptor table.  streams(): the sequences the front end convolves; rows(l): the rows of all of them at entry l (l < L: layer l's input, L: the emitted rows);
// history_in_front / new_rows_behind / history_back: a conv's input [2 history rows | new rows] and its last two rows kept for the next step; first_frames: the
// first n_0 of the C projected frames -> x; pending_in / pending_out: the merge's residual rows into and out of the layer's ring; rotary, kv_append, attention,
// csgu_conv, merge_conv (AttnArgs / DwsArgs without the position fields), collapse.  The pool's bit-equality with a stream of one rests on this being one body.
#pragma once
#include "stream_common.hpp"

namespace {

static_assert(FF1_LN_G == 0 && FF2_LN_B - FF2_LN_G == FF1_LN_B && FF2_W1 - FF2_LN_G == FF1_W1 && FF2_B1 - FF2_LN_G == FF1_B1 && FF2_W2 - FF2_LN_G == FF1_W2 &&
              FF2_B2 - FF2_LN_G == FF1_B2, "Step::ffn walks the slots of either macaron FFN from its first");

template <class Pos>
struct Step : Slots {
    const mi_ebf_config& c; const Geo& g; LayerState ls[64]; const St s; const Pos& at; const void* pos_table; hipStream_t st;      // s: the state, carved
    const int C, d, I, L, Rp;                     // Rp: the pending-residual ring, rows [o0, a) always fit
    Step(const mi_ebf_config& c_, const Geo& g_, void* state, const void* const* weights, const Pos& at_, const void* pos_table_, hipStream_t st_)
        : Slots{weights}, c(c_), g(g_), s(carve_state(c_, g_, state, ls)), at(at_), pos_table(pos_table_), st(st_), C(g_.C), d(g_.d), I(g_.I), L(g_.L), Rp(g_.r + g_.N) {}

    // LayerNorm(s) of M rows.  mi_layernorm_chain reads its T argument only with a lengths mask (norm.hip), and there is none here: M stands in
    int ln(const float* x, int M, const float* g1, const float* b1, float* y32, const float* ga, const float* ba, float eps2, bf16_t* outa, const float* gb, const float* bb,
           bf16_t* outb) const {
        return mi_layernorm_chain(x, d, nullptr, M, g1, b1, g1 ? LEPS : 0.f, y32, y32 ? d : 0, ga, ba, eps2, outa, outa ? d : 0, nullptr, 0, gb, bb, outb, outb ? d : 0, M, d, st);
    }
    // a macaron FFN, f its first slot: x += 0.5 * FFN(LN(x))   e_branchformer.py:271-273, :307-309
    int ffn(int l, int f, float* x, int M) const {
        RUN(ln(x, M, nullptr, nullptr, nullptr, Lf(l, f + FF1_LN_G), Lf(l, f + FF1_LN_B), LEPS, s.a0, nullptr, nullptr, nullptr));
        RUN(mi_gemm_bf16(s.a0, d, Lw(l, f + FF1_W1), d, Lf(l, f + FF1_B1), 1, s.h, I, 0, nullptr, 0, 1.f, 1, M, I, d, 0, 0, st));
        return mi_gemm_bf16(s.h, I, Lw(l, f + FF1_W2), I, Lf(l, f + FF1_B2), 1, x, d, 1, x, d, 0.5f, 0, M, d, I, 0, 0, st);
    }

    // Both convs on [2 history rows | the new rows] of their input, no time padding: the history IS the left padding (zero at stream start).  Then the output Linear
    // and the feature projection on all C new frames; the first n_0 of them are frames of the utterance(s) and become x.
    int front_end(const float* feats) const {
        const int n = at.streams(), Mc = n * C;
        const int wF = g.F, wA = g.F1 * g.C1 / 2;                          // row widths in 4-byte words
        RUN(at.history_in_front(s.x_hist, s.featcat, 4 * C, wF));
        RUN(at.new_rows_behind(0, feats, s.featcat, 4 * C, wF));
        RUN(at.history_back(0, s.featcat, 4 * C, s.x_hist, wF));
        RUN(mi_conv2d_first_gelu(s.featcat, Gf(G_CONV1_W), Gf(G_CONV1_B), s.act1n, n, 4 * C + 2, g.F, g.C1, 3, 2, 0, 2, 2 * C, g.F1, st));
        RUN(at.history_in_front(s.c1_hist, s.act1c, 2 * C, wA));
        RUN(at.new_rows_behind(1, s.act1n, s.act1c, 2 * C, wA));
        RUN(at.history_back(1, s.act1c, 2 * C, s.c1_hist, wA));
        RUN(mi_conv2d_cl_bf16(s.act1c, Gw(G_CONV2_W), Gf(G_CONV2_B), s.act2, n, 2 * C + 2, g.F1, g.C1, g.C2, 3, 3, 2, 0, 2, C, g.F2, 1, st));
        RUN(mi_gemm_bf16(s.act2, (long)g.F2 * g.C2, Gw(G_FEOUT_W), (long)g.F2 * g.C2, Gf(G_FEOUT_B), 1, s.feo, d, 1, nullptr, 0, 1.f, 0, Mc, d, g.F2 * g.C2, 0, 0, st));
        RUN(mi_layernorm_chain(s.feo, d, nullptr, C, nullptr, nullptr, 0.f, nullptr, 0, Gf(G_FP_LN_G), Gf(G_FP_LN_B), c.ln_eps, s.a0, d, nullptr, 0, nullptr, nullptr, nullptr, 0, Mc, d, st));
        RUN(mi_gemm_bf16(s.a0, d, Gw(G_FP_W), d, Gf(G_FP_B), 1, s.fp, d, 1, nullptr, 0, 1.f, 0, Mc, d, d, 0, 0, st));
        return at.first_frames(s.fp, s.x, C, d);
    }

    // first LayerNorm(s) of the layer on its M input rows x (the previous layer's final_layer_norm output, or the feature projection); x is the merge's residual
    int layer_input(int l, int M) const {
        if (c.use_macaron) RUN(ffn(l, FF1_LN_G, s.x, M));
        RUN(ln(s.x, M, nullptr, nullptr, nullptr, Lf(l, ATT_LN_G), Lf(l, ATT_LN_B), LEPS, s.a1, Lf(l, MLP_LN_G), Lf(l, MLP_LN_B), s.a2));
        return at.pending_in(l, s.x, ls[l].pend, Rp, d);
    }

    // Q | K | V of the new rows, K | V appended to the cache, chunk attention over the cache, output projection -> cat[:, :d]
    int global_branch(int l, int M) const {
        if (c.pos_type == 2) {
            const float* cs = (const float*)pos_table;
            RUN(at.rotary(l, s.a1, s.a1r, d, cs, cs + (size_t)g.Lmax * g.hd, g.H, g.hd));
            RUN(mi_gemm_bf16(s.a1r, d, Lw(l, ATT_WQK), d, Lf(l, ATT_BQK), 1, s.qk, 3 * d, 0, nullptr, 0, 1.f, 0, M, 2 * d, d, 0, 0, st));
            RUN(mi_gemm_bf16(s.a1, d, Lw(l, ATT_WV), d, Lf(l, ATT_BV), 1, s.qk + 2 * d, 3 * d, 0, nullptr, 0, 1.f, 0, M, d, d, 0, 0, st));
        } else {
            RUN(mi_gemm_bf16(s.a1, d, Lw(l, ATT_WQK), d, Lf(l, ATT_BQK), 1, s.qk, 3 * d, 0, nullptr, 0, 1.f, 0, M, 3 * d, d, 0, 0, st));
        }
        RUN(at.kv_append(l, s.qk + d, ls[l].kv, g.Lmax, d));             // the [K | V] columns of the new rows: d words out of rows 3d/2 words apart
        const bf16_t* posp = c.pos_type == 1 ? s.posp + (size_t)l * g.Lmax * d : nullptr;
        // ref: the walk of the full forward's kernel for this shape (stream_common.hpp); n_q, n_k, nkp, ntp are the launcher's
        const AttnArgs a{s.qk, 3L * d, ls[l].kv, ls[l].kv + d, 2L * d, (long)g.Lmax * 2 * d, posp, d, posp ? Lf(l, ATT_U) : nullptr, posp ? Lf(l, ATT_V) : nullptr, s.ctx, d,
                         0, 0, g.H, 0, 0, g.hd == 16 ? 1 : ((g.hd == 64 && posp) ? 2 : 3), 1.0f / sqrtf((float)g.hd)};
        RUN(at.attention(l, a, g.hd));
        return mi_gemm_bf16(s.ctx, d, Lw(l, ATT_WO), d, Lf(l, ATT_BO), 1, s.cat, 2 * d, 0, nullptr, 0, 1.f, 0, M, d, d, 0, 0, st);
    }

    // cgMLP with the stateful CSGU conv -> cat[:, d:]; csgu_linear: conv -> Linear -> act -> gate (e_branchformer.py:196-201)
    int local_branch(int l, int M) const {
        const bool lin = c.csgu_linear;
        RUN(mi_gemm_bf16(s.a2, d, Lw(l, MLP_W1), d, Lf(l, MLP_B1), 1, s.h, I, 0, nullptr, 0, 1.f, 1, M, I, d, 0, 0, st));
        RUN(mi_row_stats_bf16(s.h + I / 2, I, I / 2, LEPS, s.stats, M, st));
        const DwsArgs cg{s.h + I / 2, I, lin ? nullptr : s.h, I, s.stats, Lf(l, CSGU_LN_G), Lf(l, CSGU_LN_B), Lf(l, CSGU_W), Lf(l, CSGU_B), ls[l].csgu, ls[l].csgu_stats, nullptr,
                         lin ? s.cv : s.s, I / 2, g.B, I / 2, g.Kc, g.dil, g.Hc, g.Hc, 0, 0, 0, 0, lin ? 2 : 0, lin ? 0 : c.csgu_act};
        RUN(at.csgu_conv(l, cg));
        if (lin) {
            RUN(mi_gemm_bf16(s.cv, I / 2, Lw(l, CSGU_LIN_W), I / 2, Lf(l, CSGU_LIN_B), 1, s.lin, I / 2, 0, nullptr, 0, 1.f, 0, M, I / 2, I / 2, 0, 0, st));
            RUN(mi_gate_act_mul_bf16(s.h, I, s.lin, I / 2, s.s, I / 2, M, I / 2, c.csgu_act, st));
        }
        return mi_gemm_bf16(s.s, I / 2, Lw(l, MLP_W2), I / 2, Lf(l, MLP_B2), 1, s.cat + d, 2 * d, 0, nullptr, 0, 1.f, 0, M, d, I / 2, 0, 0, st);
    }

    // merge: push the new cat rows, m2 = cat + dwconv(cat) for the rows whose lookahead is complete (all pending ones of a stream that finishes); for the Mo emitted
    // rows merge_proj adds the pending residual, then the second macaron FFN and the final LayerNorm(s) run
    int merge_exit(int l, int Mo) const {
        const DwsArgs mg{s.cat, 2L * d, nullptr, 0, nullptr, nullptr, nullptr, Lf(l, MRG_DW_W), Lf(l, MRG_DW_B), ls[l].cat, nullptr, nullptr, s.m2, 2L * d,
                         g.B, 2 * d, g.Km, 1, g.r, 2 * g.r, 0, 0, 0, 0, 1, 0};
        RUN(at.merge_conv(l, mg));
        if (Mo == 0) return MI_OK;
        RUN(at.pending_out(l, ls[l].pend, s.res, Rp, d));
        RUN(mi_gemm_bf16(s.m2, 2 * d, Lw(l, MRG_W), 2 * d, Lf(l, MRG_B), 1, s.xo, d, 1, s.res, d, 1.0f, 0, Mo, d, 2 * d, 0, 0, st));
        if (c.use_macaron) RUN(ffn(l, FF2_LN_G, s.xo, Mo));
        if (l + 1 < L)         // final_layer_norm (:312): the next layer's input rows; after the last layer chained with encoder.layer_norm -> the head's input
            return ln(s.xo, Mo, Lf(l, FIN_LN_G), Lf(l, FIN_LN_B), s.x, nullptr, nullptr, 0.f, nullptr, nullptr, nullptr, nullptr);
        return ln(s.xo, Mo, Lf(l, FIN_LN_G), Lf(l, FIN_LN_B), nullptr, Gf(G_ENC_LN_G), Gf(G_ENC_LN_B), c.ln_eps, s.hid, nullptr, nullptr, nullptr);
    }

    // CTC head, per-frame classes, collapse with the carried class
    int head(int Mo, float* logits, int* best, int* ids, int* n_ids) const {
        RUN(mi_gemm_bf16(s.hid, d, Gw(G_HEAD_W), d, Gf(G_HEAD_B), 1, logits, g.ldl, 1, nullptr, 0, 1.f, 0, Mo, g.V1, d, 0, 0, st));
        RUN(mi_row_argmax(logits, g.ldl, 0, g.V1, best, Mo, st));
        return at.collapse(best, c.V, s.prev, ids, n_ids);
    }

    // x holds layer l's new input rows of all streams, compact (rows(l), d); a layer with nothing to take and nothing to emit is skipped
    int run(const float* feats, float* logits, int* best, int* ids, int* n_ids) const {
        const int n_out = at.rows(L);
        if (n_out > 0 && (!logits || !best || !ids || !n_ids)) return MI_ERR_ARG;
        if ((g.F1 * g.C1) % 2) return MI_ERR_UNSUPPORTED;               // rows are copied as 4-byte words (d is even: a multiple of the head size)
        RUN(front_end(feats));
        for (int l = 0; l < L; ++l) {
            const int M = at.rows(l), Mo = at.rows(l + 1);
            if (M == 0 && Mo == 0) continue;
            if (M > 0) {
                RUN(layer_input(l, M));
                RUN(global_branch(l, M));
                RUN(local_branch(l, M));
            }
            RUN(merge_exit(l, Mo));
        }
        return n_out > 0 ? head(n_out, logits, best, ids, n_ids) : MI_OK;
    }
};

}  // namespace
