// The C-side contract of the whole-encoder drivers (encoder.hip: bf16, encoder_f32.hip: fp32), written once: the weight-table slot order, the geometry of the
// Conv2d sub-sampling, the workspace carver and the length launcher.  Internal: nothing here is exported.
#pragma once
#include "common.hpp"
#include "../../include/hfasr_hip.h"

// ---- weight-table slot order: the ABI between engine.py (G / LS; tests/test_encoder_layout_cpu.py ties them to these two lists) and both drivers.  Append only.
enum G { G_CONV1_W, G_CONV1_B, G_CONV2_W, G_CONV2_B, G_FEOUT_W, G_FEOUT_B, G_FP_LN_G, G_FP_LN_B, G_FP_W, G_FP_B,
         G_ENC_LN_G, G_ENC_LN_B, G_HEAD_W, G_HEAD_B, G_MIX_W /* per_layer_weights (L+1) f32, bestrq.py:202-205 */,
         G_GATE1_W, G_GATE1_B, G_GATE2_W, G_GATE2_B /* gate filters of the context-aware front ends (extractors.py:23-54) */ };
enum LS { FF1_LN_G, FF1_LN_B, FF1_W1, FF1_B1, FF1_W2, FF1_B2,
          ATT_LN_G, ATT_LN_B, ATT_WQK, ATT_BQK, ATT_WV, ATT_BV, ATT_WO, ATT_BO, ATT_WPOS, ATT_U, ATT_V,
          MLP_LN_G, MLP_LN_B, MLP_W1, MLP_B1, CSGU_LN_G, CSGU_LN_B, CSGU_W, CSGU_B, MLP_W2, MLP_B2,
          MRG_DW_W, MRG_DW_B, MRG_W, MRG_B, FIN_LN_G, FIN_LN_B,
          FF2_LN_G, FF2_LN_B, FF2_W1, FF2_B1, FF2_W2, FF2_B2, CSGU_LIN_W, CSGU_LIN_B,
          // ln_fold: W' = bf16(W diag(gamma)), its fp32 column sums, and W beta + b for the four LayerNorm -> Linear pairs of a layer (the fp32 driver reads none of them)
          FF1_WF, FF1_SF, FF1_CF, QKV_WF, QKV_SF, QKV_CF, MLP_WF, MLP_SF, MLP_CF, FF2_WF, FF2_SF, FF2_CF };
static_assert(G_GATE2_B < MI_EBF_GLOBAL_SLOTS && FF2_CF < MI_EBF_LAYER_SLOTS, "the slot lists must fit the table the header sizes");

// the slots of a table: globals first, then MI_EBF_LAYER_SLOTS per layer
struct Slots {
    const void* const* t;
    const void* Gw(int s) const { return t[s]; }
    const void* Lw(int l, int s) const { return t[MI_EBF_GLOBAL_SLOTS + l * MI_EBF_LAYER_SLOTS + s]; }
    const float* Gf(int s) const { return (const float*)Gw(s); }
    const float* Lf(int l, int s) const { return (const float*)Lw(l, s); }
};

// ---- geometry: two K x K / stride convs over (T, F); a causal stack has the same total padding, all of it on the left (streaming_modules.py:31-55)
struct Dims { int T1, F1, T2, F2, M, Tp, hd; };      // M = B * T2 rows; Tp = T2 padded to 32 (V^T's time axis); hd = head size

static inline int conv_out(int n, int k, int s, int pad_total) { return s > 0 ? (n + pad_total - k) / s + 1 : 0; }

static inline Dims dims(const mi_ebf_config& c) {
    Dims d;
    d.T1 = conv_out(c.T, c.K, c.stride, 2 * c.pad); d.F1 = conv_out(c.F, c.K, c.stride, 2 * c.pad);
    d.T2 = conv_out(d.T1, c.K, c.stride, 2 * c.pad); d.F2 = conv_out(d.F1, c.K, c.stride, 2 * c.pad);
    d.M = c.B * d.T2; d.Tp = (d.T2 + 31) / 32 * 32; d.hd = c.H > 0 ? c.d / c.H : 0;
    return d;
}
// what a workspace query needs before it carves (the forwards check the same fields, among others)
static inline bool sizable(const mi_ebf_config* c) { return c && c->B > 0 && c->H > 0 && dims(*c).T2 > 0; }

// workspace carver: consecutive 256-byte aligned pieces; base == nullptr only counts
struct Carver {
    char* base; size_t off;
    void* take(size_t bytes) { void* p = base ? base + off : nullptr; off += (bytes + 255) / 256 * 256; return p; }
};

// "conv #1 of the gated front end runs fused": mi_conv2d_first_gated_gelu's (conv.hip) condition, and the one under which the driver's workspace holds no raw conv / gate
// tensors for that layer
static inline bool conv1_gated_fused(int B, int T1, int F1, int C, int K) {
    return K == 3 && (C % 4) == 0 && C / 4 <= 256 && (long)B * T1 * F1 < (1L << 31) - 256L * 8192;
}

// frame counts behind `layers` sub-sampling convs for every utterance, one launch (encoder.hip): inner = min(the count with pad_total of padding per conv, tmax) — what the
// masks use (extractors.py:133-162) —, outer = the count without padding — what the CTC loss is given (_get_feat_extract_output_lengths; quirk of SURVEY.md §8a row 8').
// lengths == nullptr: every utterance has T frames.
__attribute__((visibility("hidden"))) void launch_subsampled_lengths(const int* lengths, int T, int B, int K, int stride, int pad_total, int layers, int tmax,
                                                                     int* inner, int* outer, hipStream_t st);

#define RUN(expr) do { int rc__ = (expr); if (rc__ != MI_OK) return rc__; } while (0)
