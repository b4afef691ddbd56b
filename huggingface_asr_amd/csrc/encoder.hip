// Whole-encoder driver: Wav2Vec2EBranchformerForCTC.forward in eval mode as one C call that enqueues
// every kernel of the path on the caller's stream (no allocation, no sync -> hipGraph-capturable).
//
// Reference call stack: e_branchformer.py:422-457 -> wav2vec2_conformer model forward
// (:1133-1195: conv sub-sampling, mask, feature projection) -> encoder loop (:651-717) with
// Wav2Vec2EBranchformerEncoderLayer.forward (e_branchformer.py:263-313) -> lm_head ⊕ blank_projection.
//
// Data layout in HBM (all row-major, rows = b*T2 + t):
//   x     fp32 (M, d)     residual stream (the reference's stream is fp32 under bf16 autocast too)
//   a0/a1/a2 bf16 (M, d)  LayerNorm outputs = GEMM A operands
//   h     bf16 (M, I)     FFN hidden / cgMLP channel_proj1 output [x_r | x_g]
//   qk    bf16 (M, 2d)    [Q | K] projections; vt bf16 (d, B*Tp) = V^T, key-contiguous, time padded to 32
//   cat   bf16 (M, 2d)    [attention branch | cgMLP branch]  (torch.cat at e_branchformer.py:296 is free)
//   act1  bf16 (B,T1,F1,C1), act2 bf16 (B,T2,F2,C2) channels-last conv activations
#include "ebf_layout.hpp"

namespace {

struct Ws {
    bf16_t *act1, *act2, *a0, *a1, *a2, *a1r, *h, *qk, *vt, *ctx, *cat, *m2, *s, *hid;
    bf16_t *cv, *lin;         // csgu_use_linear_after_conv: the CSGU conv output and the Linear's output
    bf16_t *z1, *g1, *z2, *g2;   // context-aware front ends: raw conv / gate outputs of the un-fused forms
    float *feo, *x, *stats, *lnst;   // lnst: ln_fold's per-row partial (sum, sumsq) records, 32 floats per row
    float *mixed, *lh, *sw;   // fine-tuning head: weighted sum of the hidden states, fp32 copy of the last one, softmax(per_layer_weights)
    int* lens;   // [inner(B) | outer(B)]
    size_t bytes;
};

Ws carve(const mi_ebf_config& c, const Dims& d, void* base) {
    Carver k{(char*)base, 0};
    auto bf = [&](size_t n) { return (bf16_t*)k.take(n * 2); };
    auto f32 = [&](size_t n) { return (float*)k.take(n * 4); };
    Ws w;
    const size_t M = d.M, dd = c.d, I = c.I, n1 = (size_t)c.B * d.T1 * d.F1 * c.C1, n2 = (size_t)c.B * d.T2 * d.F2 * c.C2;
    w.act1 = bf(n1); w.act2 = bf(n2);
    w.z1 = w.g1 = w.z2 = w.g2 = nullptr;
    if (c.context_mode == 1) {            // the un-fused fallbacks of GatedConv2d: layer 1 [conv | gate] as two tensors, layer 2 as one stacked (M2, 2*C2) GEMM output
        if (!conv1_gated_fused(c.B, d.T1, d.F1, c.C1, c.K)) { w.z1 = bf(n1); w.g1 = bf(n1); }
        w.z2 = bf(2 * n2);
    } else if (c.context_mode == 2) {     // GatedConv2dShared: the gate has a quarter of the conv's time steps
        w.z1 = bf(n1); w.g1 = bf((size_t)c.B * (d.T1 / 4 + 1) * d.F1 * c.C1);
        w.z2 = bf(n2); w.g2 = bf((size_t)c.B * (d.T2 / 4 + 1) * d.F2 * c.C2);
    }
    w.feo = f32(M * dd); w.x = f32(M * dd);
    w.a0 = bf(M * dd); w.a1 = bf(M * dd); w.a2 = bf(M * dd); w.a1r = bf(M * dd);
    w.h = bf(M * I);
    w.qk = bf(M * 3 * dd);      // [Q | K | V] (V columns used by the LDS-staged attention only)
    w.vt = bf(dd * c.B * d.Tp);
    w.ctx = bf(M * dd); w.cat = bf(M * 2 * dd); w.m2 = bf(M * 2 * dd); w.s = bf(M * (I / 2));
    w.cv = w.lin = nullptr;
    if (c.csgu_linear) { w.cv = bf(M * (I / 2)); w.lin = bf(M * (I / 2)); }
    w.hid = bf(M * dd);
    w.stats = f32(M * 2);
    w.lnst = c.ln_fold ? f32(M * 32) : nullptr;
    w.lens = (int*)k.take((size_t)2 * c.B * 4);
    w.mixed = w.lh = w.sw = nullptr;
    if (c.layer_mixing) { w.mixed = f32(M * dd); w.sw = f32((size_t)(c.L + 1)); }
    if (c.layer_mixing || c.extra_layers) w.lh = f32(M * dd);
    w.bytes = k.off;
    return w;
}

__device__ __forceinline__ int floor_div(int a, int d) { int q = a / d; if ((a % d) != 0 && ((a < 0) != (d < 0))) --q; return q; }      // torch.div(rounding_mode="floor")
__global__ void subsampled_lengths_kernel(const int* __restrict__ in, int T, int B, int K, int stride, int pad_total, int layers, int tmax,
                                          int* __restrict__ inner, int* __restrict__ outer) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    int li = in ? in[b] : T, lo = li;
    for (int i = 0; i < layers; ++i) { li = floor_div(li + pad_total - K, stride) + 1; lo = floor_div(lo - K, stride) + 1; }
    inner[b] = li < tmax ? li : tmax;
    outer[b] = lo;
}

// side stream + fork/join events of the experimental branch overlap (created on first use; one forward in flight at a time)
constexpr int MAX_OVL_LAYERS = 64;
hipStream_t g_side = nullptr;
hipEvent_t g_fork[MAX_OVL_LAYERS], g_join[MAX_OVL_LAYERS];      // one pair per layer: an event is never re-recorded while a wait on it may be pending
bool side_ready() {
    if (g_side) return true;
    if (hipStreamCreateWithFlags(&g_side, hipStreamNonBlocking) != hipSuccess) { g_side = nullptr; return false; }
    for (int i = 0; i < MAX_OVL_LAYERS; ++i)
        if (hipEventCreateWithFlags(&g_fork[i], hipEventDisableTiming) != hipSuccess || hipEventCreateWithFlags(&g_join[i], hipEventDisableTiming) != hipSuccess) {
            g_side = nullptr;
            return false;
        }
    return true;
}

constexpr float LEPS = 1e-5f;      // nn.LayerNorm default: the layers use nn.LayerNorm(embed_dim) (e_branchformer.py:233-261)

// One forward: the config, its geometry, the carved workspace, the weight table and the stream, and the stages of the launch sequence in the order ebf_forward_body runs them.
struct Fwd : Slots {
    const mi_ebf_config& c; const Dims D; const Ws w; hipStream_t st;
    const int* mask_len;                          // the inner lengths of a ragged batch, else null
    const void* pos_table; void* posp;            // header: mi_ebf_forward
    const int M, d, I, T2, P;                     // P = 2*T2-1 relative positions
    const int dil, cpad;                          // quirk: the causal CSGU conv is dilated by (K-1)/2 (e_branchformer.py:153-160 passes it in the dilation slot)
    const float scale;
    Fwd(const mi_ebf_config& c_, const Dims& D_, const Ws& w_, const void* const* weights, hipStream_t st_, const int* mask, const void* pos_table_, void* posp_)
        : Slots{weights}, c(c_), D(D_), w(w_), st(st_), mask_len(mask), pos_table(pos_table_), posp(posp_), M(D_.M), d(c_.d), I(c_.I), T2(D_.T2), P(2 * D_.T2 - 1),
          dil(c_.is_causal ? (c_.csgu_kernel - 1) / 2 : 1), cpad(c_.is_causal ? (c_.csgu_kernel - 1) * dil : (c_.csgu_kernel - 1) / 2), scale(1.0f / sqrtf((float)D_.hd)) {}

    const bf16_t* posp_of(int l) const { return c.pos_type == 1 ? (const bf16_t*)posp + (size_t)l * P * d : nullptr; }
    const float* pos_u(int l) const { return c.pos_type == 1 ? Lf(l, ATT_U) : nullptr; }
    const float* pos_v(int l) const { return c.pos_type == 1 ? Lf(l, ATT_V) : nullptr; }
    int keep_hidden(float* hidden_states, int l, const float* src) const {      // output_hidden_states entry l: a device-to-device copy on the same stream, only when asked for
        if (hidden_states && hipMemcpyAsync(hidden_states + (size_t)l * M * d, src, (size_t)M * d * sizeof(float), hipMemcpyDeviceToDevice, st) != hipSuccess) return MI_ERR_LAUNCH;
        return MI_OK;
    }
    int front_end(const float* feats) const;
    int enter_layer(const float* src, int l) const;
    int project_positions(int layers) const;
    int attention_qkv(int l) const;
    int local_gate(int l, hipStream_t sl) const;
    int merge_dwconv(int l) const;
    int plain_layer(int l, int Lt) const;
    int folded_layer(int l) const;
    int encoder_exit(int l, float* last_hidden) const;
    int ctc_head(void* logits, float* lse, float* lse_workspace, int* best, float* amax_workspace) const;
};

// Conv2d sub-sampling in its three context modes (extractors.py:110-113), the output Linear and the feature projection: x = the encoder's input rows
int Fwd::front_end(const float* feats) const {
    const int pl = c.is_causal ? 2 * c.pad : c.pad;
    if (c.context_mode < 0 || c.context_mode > 2 || (c.context_mode && c.is_causal)) return MI_ERR_ARG;      // the causal stack is CausalConv2d whatever the field says (extractors.py:74-81)
    if (c.context_mode == 0) {
        RUN(mi_conv2d_first_gelu(feats, Gf(G_CONV1_W), Gf(G_CONV1_B), w.act1, c.B, c.T, c.F, c.C1, c.K, c.stride, pl, pl, D.T1, D.F1, st));
        RUN(mi_conv2d_cl_bf16(w.act1, Gw(G_CONV2_W), Gf(G_CONV2_B), w.act2, c.B, D.T1, D.F1, c.C1, c.C2, c.K, c.K, c.stride, pl, pl,
                              D.T2, D.F2, 1, st));
    } else if (c.context_mode == 1) {
        // GatedConv2d (extractors.py:23-32): GELU(conv * sigmoid(gate)), both layers.  Layer 1: two filter banks in one VALU kernel; layer 2: conv and gate rows in ONE
        // implicit GEMM with the product in its epilogue.  Shapes the fused kernels do not take run raw convs + mi_gated_act_bf16.
        if (c.gate_blk <= 0 || (c.C2 % c.gate_blk) != 0) return MI_ERR_ARG;
        int rc = mi_conv2d_first_gated_gelu(feats, Gf(G_CONV1_W), Gf(G_CONV1_B), Gf(G_GATE1_W), Gf(G_GATE1_B), w.act1, c.B, c.T, c.F, c.C1, c.K, c.stride, pl, pl, D.T1, D.F1, st);
        if (rc == MI_ERR_UNSUPPORTED) {
            RUN(mi_conv2d_first_geo(feats, Gf(G_CONV1_W), Gf(G_CONV1_B), w.z1, c.B, c.T, c.F, c.C1, c.K, c.K, c.stride, c.stride, pl, pl, D.T1, D.F1, 0, st));
            RUN(mi_conv2d_first_geo(feats, Gf(G_GATE1_W), Gf(G_GATE1_B), w.g1, c.B, c.T, c.F, c.C1, c.K, c.K, c.stride, c.stride, pl, pl, D.T1, D.F1, 0, st));
            RUN(mi_gated_act_bf16(w.z1, c.C1, w.g1, c.C1, w.act1, c.C1, c.B, D.T1, D.F1, c.C1, 1, 0, st));
        } else if (rc != MI_OK) return rc;
        rc = c.gate_blk == 32 ? mi_conv2d_cl_geo_bf16(w.act1, Gw(G_CONV2_W), Gf(G_CONV2_B), w.act2, c.B, D.T1, D.F1, c.C1, c.C2, c.K, c.K, c.stride, c.stride, pl, pl, D.T2, D.F2, 1, 1, st)
                              : MI_ERR_UNSUPPORTED;
        if (rc == MI_ERR_UNSUPPORTED) {
            RUN(mi_conv2d_cl_geo_bf16(w.act1, Gw(G_CONV2_W), Gf(G_CONV2_B), w.z2, c.B, D.T1, D.F1, c.C1, 2 * c.C2, c.K, c.K, c.stride, c.stride, pl, pl, D.T2, D.F2, 0, 0, st));
            RUN(mi_gated_act_bf16(w.z2, 2 * c.C2, w.z2, 2 * c.C2, w.act2, c.C2, c.B, D.T2, D.F2, c.C2, 1, c.gate_blk, st));
        } else if (rc != MI_OK) return rc;
    } else {
        // GatedConv2dShared (extractors.py:35-54): the gate conv is (4K, K) / stride (4s, s) / padding (4p, p); conv_out.view(B, C, -1, 4, F) * gate.unsqueeze(3) needs the
        // conv's time axis divisible by 4 and a quarter of it to be the gate's — the reference raises otherwise, so does this
        const int KH = 4 * c.K, sg = 4 * c.stride, pg = 4 * c.pad;
        const int Tg1 = conv_out(c.T, KH, sg, 2 * pg), Tg2 = conv_out(D.T1, KH, sg, 2 * pg);
        if ((D.T1 % 4) != 0 || Tg1 != D.T1 / 4 || (D.T2 % 4) != 0 || Tg2 != D.T2 / 4) return MI_ERR_ARG;
        RUN(mi_conv2d_first_geo(feats, Gf(G_CONV1_W), Gf(G_CONV1_B), w.z1, c.B, c.T, c.F, c.C1, c.K, c.K, c.stride, c.stride, pl, pl, D.T1, D.F1, 0, st));
        RUN(mi_conv2d_first_geo(feats, Gf(G_GATE1_W), Gf(G_GATE1_B), w.g1, c.B, c.T, c.F, c.C1, KH, c.K, sg, c.stride, pg, pl, Tg1, D.F1, 0, st));
        RUN(mi_gated_act_bf16(w.z1, c.C1, w.g1, c.C1, w.act1, c.C1, c.B, D.T1, D.F1, c.C1, 4, 0, st));
        RUN(mi_conv2d_cl_bf16(w.act1, Gw(G_CONV2_W), Gf(G_CONV2_B), w.z2, c.B, D.T1, D.F1, c.C1, c.C2, c.K, c.K, c.stride, pl, pl, D.T2, D.F2, 0, st));
        RUN(mi_conv2d_cl_geo_bf16(w.act1, Gw(G_GATE2_W), Gf(G_GATE2_B), w.g2, c.B, D.T1, D.F1, c.C1, c.C2, KH, c.K, sg, c.stride, pg, pl, Tg2, D.F2, 0, 0, st));
        RUN(mi_gated_act_bf16(w.z2, c.C2, w.g2, c.C2, w.act2, c.C2, c.B, D.T2, D.F2, c.C2, 4, 0, st));
    }
    // Both Linears below are N = d GEMMs: in throughput mode they run on the 256 x 256 tile like the layers' (folded_layer's gv); a shape that kernel refuses keeps the product's call
    const int gv = c.wide_tiles ? 40 : 0;
    auto linear = [&](const bf16_t* A, long K, const void* W, const float* bias, float* C) {
        int rc = gv ? mi_gemm_bf16_v(A, K, W, K, bias, 1, C, d, 1, nullptr, 0, 1.f, 0, M, d, (int)K, 0, 0, gv, st) : MI_ERR_UNSUPPORTED;
        if (rc == MI_ERR_UNSUPPORTED) rc = mi_gemm_bf16(A, K, W, K, bias, 1, C, d, 1, nullptr, 0, 1.f, 0, M, d, (int)K, 0, 0, st);
        return rc;
    };
    // (B,C,T',F') -> transpose -> flatten -> Linear: act2 is already (B*T', F'*C) with the weight columns permuted to match
    RUN(linear(w.act2, (long)D.F2 * c.C2, Gw(G_FEOUT_W), Gf(G_FEOUT_B), w.feo));
    // feature projection: LN -> Linear (extractors.py:130-131; tf:328-333)
    RUN(mi_layernorm_chain(w.feo, d, nullptr, T2, nullptr, nullptr, 0.f, nullptr, 0, Gf(G_FP_LN_G), Gf(G_FP_LN_B), c.ln_eps,
                           w.a0, d, nullptr, 0, nullptr, nullptr, nullptr, 0, M, d, st));
    return linear(w.a0, d, Gw(G_FP_W), Gf(G_FP_B), w.x);
}

// x = src with padded frames zeroed (tf:662-665); first LayerNorm(s) of layer l
int Fwd::enter_layer(const float* src, int l) const {
    if (c.use_macaron)
        return mi_layernorm_chain(src, d, mask_len, T2, nullptr, nullptr, 0.f, w.x, d, Lf(l, FF1_LN_G), Lf(l, FF1_LN_B), LEPS,
                                  w.a0, d, nullptr, 0, nullptr, nullptr, nullptr, 0, M, d, st);
    return mi_layernorm_chain(src, d, mask_len, T2, nullptr, nullptr, 0.f, w.x, d, Lf(l, ATT_LN_G), Lf(l, ATT_LN_B), LEPS,
                              w.a1, d, nullptr, 0, Lf(l, MLP_LN_G), Lf(l, MLP_LN_B), w.a2, d, M, d, st);
}

// relative positions: p_l = linear_pos_l(table) for every layer (batch independent; tf:531-536)
int Fwd::project_positions(int layers) const {
    for (int l = 0; l < layers; ++l)
        RUN(mi_gemm_bf16(pos_table, d, Lw(l, ATT_WPOS), d, nullptr, 0, (bf16_t*)posp + (size_t)l * P * d, d, 0, nullptr, 0, 1.f, 0,
                         P, d, d, 0, 0, st));
    return MI_OK;
}

// the LDS-staged attention over qk = [Q | K | V] (head sizes 64 and 128)
int Fwd::attention_qkv(int l) const {
    return mi_attention_qkv_bf16(w.qk, 3 * d, w.qk + d, 3 * d, w.qk + 2 * d, 3 * d, posp_of(l), d, pos_u(l), pos_v(l),
                                 mask_len, w.ctx, d, c.B, T2, 0, 0, c.H, D.hd, scale, c.is_causal, st);
}

// CSGU of the local branch on stream sl (e_branchformer.py:184-222): h = [x_r | x_g] -> s = x_r * act(conv(LN(x_g)))
int Fwd::local_gate(int l, hipStream_t sl) const {
    const int kc = c.csgu_kernel;
    RUN(mi_row_stats_bf16(w.h + I / 2, I, I / 2, LEPS, w.stats, M, sl));
    if (!c.csgu_linear)
        return mi_csgu_bf16(w.h, I, w.stats, Lf(l, CSGU_LN_G), Lf(l, CSGU_LN_B), Lf(l, CSGU_W), Lf(l, CSGU_B), w.s, I / 2, c.B, T2, I / 2, kc, cpad, dil, c.csgu_act, sl);
    // conv -> Linear -> act -> gate (e_branchformer.py:196-201)
    RUN(mi_csgu_conv_bf16(w.h, I, w.stats, Lf(l, CSGU_LN_G), Lf(l, CSGU_LN_B), Lf(l, CSGU_W), Lf(l, CSGU_B), w.cv, I / 2, c.B, T2, I / 2, kc, cpad, dil, sl));
    RUN(mi_gemm_bf16(w.cv, I / 2, Lw(l, CSGU_LIN_W), I / 2, Lf(l, CSGU_LIN_B), 1, w.lin, I / 2, 0, nullptr, 0, 1.f, 0, M, I / 2, I / 2, 0, 0, sl));
    return mi_gate_act_mul_bf16(w.h, I, w.lin, I / 2, w.s, I / 2, M, I / 2, c.csgu_act, sl);
}

// merge (e_branchformer.py:296-304): m2 = cat + dwconv(cat); merge_proj follows in the layer
int Fwd::merge_dwconv(int l) const {
    const int km = c.merge_kernel;
    return mi_dwconv_residual_bf16(w.cat, 2 * d, Lf(l, MRG_DW_W), Lf(l, MRG_DW_B), w.m2, 2 * d, c.B, T2, 2 * d, km, (km - 1) / 2, st);
}

// One layer with LayerNorm kernels and plain GEMMs, from its first LayerNorm's output (a0, or a1 / a2 without macaron FFNs) to the LayerNorm(s) of the next consumer;
// the encoder's last layer ends before its final_layer_norm (encoder_exit).  Lt = L + extra_layers.
int Fwd::plain_layer(int l, int Lt) const {
    // layer mixing (bestrq.py:239-245): hidden_states[l] is this layer's input; the weight is read on the device
    if (c.layer_mixing && l < c.L) RUN(mi_axpy_dev_f32(w.mixed, w.x, (long)M * d, w.sw + l, l == 0, st));
    if (c.use_macaron) {   // x += 0.5 * FFN(LN(x))   e_branchformer.py:271-273
        RUN(mi_gemm_bf16(w.a0, d, Lw(l, FF1_W1), d, Lf(l, FF1_B1), 1, w.h, I, 0, nullptr, 0, 1.f, 1, M, I, d, 0, 0, st));
        RUN(mi_gemm_bf16(w.h, I, Lw(l, FF1_W2), I, Lf(l, FF1_B2), 1, w.x, d, 1, w.x, d, 0.5f, 0, M, d, I, 0, 0, st));
        RUN(mi_layernorm_chain(w.x, d, nullptr, T2, nullptr, nullptr, 0.f, nullptr, 0, Lf(l, ATT_LN_G), Lf(l, ATT_LN_B), LEPS,
                               w.a1, d, nullptr, 0, Lf(l, MLP_LN_G), Lf(l, MLP_LN_B), w.a2, d, M, d, st));
    }
    // the two branches read a1 / a2 and write disjoint buffers (qk, ctx, cat[:, :d] | h, stats, s, cat[:, d:]): with branch_overlap the
    // local one is enqueued on the side stream between a fork and a join event
    const bool ovl = c.branch_overlap && l < MAX_OVL_LAYERS && side_ready();
    hipStream_t sl = ovl ? g_side : st;
    if (ovl) { (void)hipEventRecord(g_fork[l], st); (void)hipStreamWaitEvent(g_side, g_fork[l], 0); }
    // global branch (e_branchformer.py:281-288)
    const bf16_t* qk_in = w.a1;
    if (c.pos_type == 2) {
        const float* rot_cos = (const float*)pos_table;      // [cos (T2, hd) | sin (T2, hd)]
        RUN(mi_rotary_bf16(w.a1, d, w.a1r, d, rot_cos, rot_cos ? rot_cos + (size_t)T2 * D.hd : nullptr, M, T2, c.H, D.hd, st));
        qk_in = w.a1r;
    }
    if (D.hd == 64 || D.hd == 128) {
        // fused [Q|K|V] projection (weights are packed [Wq;Wk;Wv]); rotary feeds Q,K from the rotated input only
        if (c.pos_type == 2) {
            RUN(mi_gemm_bf16(qk_in, d, Lw(l, ATT_WQK), d, Lf(l, ATT_BQK), 1, w.qk, 3 * d, 0, nullptr, 0, 1.f, 0, M, 2 * d, d, 0, 0, st));
            RUN(mi_gemm_bf16(w.a1, d, Lw(l, ATT_WV), d, Lf(l, ATT_BV), 1, w.qk + 2 * d, 3 * d, 0, nullptr, 0, 1.f, 0, M, d, d, 0, 0, st));
        } else {
            RUN(mi_gemm_bf16(w.a1, d, Lw(l, ATT_WQK), d, Lf(l, ATT_BQK), 1, w.qk, 3 * d, 0, nullptr, 0, 1.f, 0, M, 3 * d, d, 0, 0, st));
        }
        RUN(attention_qkv(l));
    } else {
        RUN(mi_gemm_bf16(qk_in, d, Lw(l, ATT_WQK), d, Lf(l, ATT_BQK), 1, w.qk, 3 * d, 0, nullptr, 0, 1.f, 0, M, 2 * d, d, 0, 0, st));
        // V^T = Wv · a1^T (+ bv per row), columns remapped to the time-padded (b*Tp + t) layout
        RUN(mi_gemm_bf16(Lw(l, ATT_WV), d, w.a1, d, Lf(l, ATT_BV), 2, w.vt, (long)c.B * D.Tp, 0, nullptr, 0, 1.f, 0, d, M, d,
                         T2, D.Tp, st));
        RUN(mi_attention_bf16(w.qk, 3 * d, w.qk + d, 3 * d, w.vt, (long)c.B * D.Tp, D.Tp, posp_of(l), d, pos_u(l), pos_v(l),
                              mask_len, w.ctx, d, c.B, T2, c.H, D.hd, scale, c.is_causal, st));
    }
    RUN(mi_gemm_bf16(w.ctx, d, Lw(l, ATT_WO), d, Lf(l, ATT_BO), 1, w.cat, 2 * d, 0, nullptr, 0, 1.f, 0, M, d, d, 0, 0, st));
    // local branch: cgMLP (e_branchformer.py:291-292, 184-222)
    RUN(mi_gemm_bf16(w.a2, d, Lw(l, MLP_W1), d, Lf(l, MLP_B1), 1, w.h, I, 0, nullptr, 0, 1.f, 1, M, I, d, 0, 0, sl));
    RUN(local_gate(l, sl));
    RUN(mi_gemm_bf16(w.s, I / 2, Lw(l, MLP_W2), I / 2, Lf(l, MLP_B2), 1, w.cat + d, 2 * d, 0, nullptr, 0, 1.f, 0, M, d, I / 2, 0, 0, sl));
    if (ovl) { (void)hipEventRecord(g_join[l], g_side); (void)hipStreamWaitEvent(st, g_join[l], 0); }
    RUN(merge_dwconv(l));
    RUN(mi_gemm_bf16(w.m2, 2 * d, Lw(l, MRG_W), 2 * d, Lf(l, MRG_B), 1, w.x, d, 1, w.x, d, 1.0f, 0, M, d, 2 * d, 0, 0, st));
    if (c.use_macaron) {   // e_branchformer.py:307-309
        RUN(mi_layernorm_chain(w.x, d, nullptr, T2, nullptr, nullptr, 0.f, nullptr, 0, Lf(l, FF2_LN_G), Lf(l, FF2_LN_B), LEPS,
                               w.a0, d, nullptr, 0, nullptr, nullptr, nullptr, 0, M, d, st));
        RUN(mi_gemm_bf16(w.a0, d, Lw(l, FF2_W1), d, Lf(l, FF2_B1), 1, w.h, I, 0, nullptr, 0, 1.f, 1, M, I, d, 0, 0, st));
        RUN(mi_gemm_bf16(w.h, I, Lw(l, FF2_W2), I, Lf(l, FF2_B2), 1, w.x, d, 1, w.x, d, 0.5f, 0, M, d, I, 0, 0, st));
    }
    // final_layer_norm (:312) chained with the next consumer's LayerNorm(s)
    if (l + 1 == c.L) return MI_OK;
    if (l + 1 == Lt)                                   // end of the additional layer: its final_layer_norm feeds the head directly
        return mi_layernorm_chain(w.x, d, nullptr, T2, nullptr, nullptr, 0.f, nullptr, 0, Lf(l, FIN_LN_G), Lf(l, FIN_LN_B), LEPS,
                                  w.hid, d, nullptr, 0, nullptr, nullptr, nullptr, 0, M, d, st);
    if (c.use_macaron)
        return mi_layernorm_chain(w.x, d, nullptr, T2, Lf(l, FIN_LN_G), Lf(l, FIN_LN_B), LEPS, w.x, d,
                                  Lf(l + 1, FF1_LN_G), Lf(l + 1, FF1_LN_B), LEPS, w.a0, d, nullptr, 0, nullptr, nullptr, nullptr, 0, M, d, st);
    return mi_layernorm_chain(w.x, d, nullptr, T2, Lf(l, FIN_LN_G), Lf(l, FIN_LN_B), LEPS, w.x, d,
                              Lf(l + 1, ATT_LN_G), Lf(l + 1, ATT_LN_B), LEPS, w.a1, d, nullptr, 0,
                              Lf(l + 1, MLP_LN_G), Lf(l + 1, MLP_LN_B), w.a2, d, M, d, st);
}

// One LayerNorm-folded layer (header: mi_ebf_config.ln_fold).  a0 holds bf16(x) of the CURRENT residual stream, lnst its per-row partial statistics: ONE pair per row at the
// layer's entry (written by mi_layernorm_fold), npg pairs after a producer GEMM's epilogue (FFN-out, merge).  The last layer ends before its final_layer_norm (encoder_exit).
int Fwd::folded_layer(int l) const {
    const int gv = c.wide_tiles ? 40 : 0;                     // kernel of the N = d GEMMs: 0 the product's 128 x 128, 40 the 256 x 256 tile (throughput mode)
    const int npg = c.wide_tiles ? d / 64 : d / 32;           // pairs a producer GEMM writes (one per 32 / 64 columns)
    // x += 0.5 * FFN(LN(x))   e_branchformer.py:271-273
    RUN(mi_gemm_lnfold_bf16(w.a0, d, Lw(l, FF1_WF), d, Lf(l, FF1_SF), Lf(l, FF1_CF), w.lnst, 1, LEPS, w.h, I, 1, M, I, d, st));
    RUN(mi_gemm_resid_stats_f32_v(w.h, I, Lw(l, FF1_W2), I, Lf(l, FF1_B2), w.x, d, w.x, d, 0.5f, w.a0, d, w.lnst, M, d, I, gv, st));
    // global branch: self_attn_layer_norm folded into [Q|K|V]   (e_branchformer.py:281-288)
    RUN(mi_gemm_lnfold_bf16(w.a0, d, Lw(l, QKV_WF), d, Lf(l, QKV_SF), Lf(l, QKV_CF), w.lnst, npg, LEPS, w.qk, 3 * d, 0, M, 3 * d, d, st));
    RUN(attention_qkv(l));
    RUN(mi_gemm_bf16_v(w.ctx, d, Lw(l, ATT_WO), d, Lf(l, ATT_BO), 1, w.cat, 2 * d, 0, nullptr, 0, 1.f, 0, M, d, d, 0, 0, gv, st));
    // local branch: cgMLP_layer_norm folded into channel_proj1   (e_branchformer.py:291-292, 184-222)
    RUN(mi_gemm_lnfold_bf16(w.a0, d, Lw(l, MLP_WF), d, Lf(l, MLP_SF), Lf(l, MLP_CF), w.lnst, npg, LEPS, w.h, I, 1, M, I, d, st));
    RUN(local_gate(l, st));
    RUN(mi_gemm_bf16_v(w.s, I / 2, Lw(l, MLP_W2), I / 2, Lf(l, MLP_B2), 1, w.cat + d, 2 * d, 0, nullptr, 0, 1.f, 0, M, d, I / 2, 0, 0, gv, st));
    // merge: x += merge_proj(m + dwconv(m)); the epilogue leaves bf16(x) and its statistics for ff2's folded LayerNorm
    RUN(merge_dwconv(l));
    RUN(mi_gemm_resid_stats_f32_v(w.m2, 2 * d, Lw(l, MRG_W), 2 * d, Lf(l, MRG_B), w.x, d, w.x, d, 1.0f, w.a0, d, w.lnst, M, d, 2 * d, gv, st));
    // x += 0.5 * FFN(LN(x))   e_branchformer.py:307-309
    RUN(mi_gemm_lnfold_bf16(w.a0, d, Lw(l, FF2_WF), d, Lf(l, FF2_SF), Lf(l, FF2_CF), w.lnst, npg, LEPS, w.h, I, 1, M, I, d, st));
    RUN(mi_gemm_bf16_v(w.h, I, Lw(l, FF2_W2), I, Lf(l, FF2_B2), 1, w.x, d, 1, w.x, d, 0.5f, 0, M, d, I, 0, 0, gv, st));
    if (l + 1 == c.L) return MI_OK;
    // final_layer_norm (:312): the new residual stream, its bf16 copy and statistics for the next layer
    return mi_layernorm_fold(w.x, d, nullptr, T2, Lf(l, FIN_LN_G), Lf(l, FIN_LN_B), LEPS, w.x, d, w.a0, d, w.lnst, M, d, st);
}

// After layer L-1: final_layer_norm (:312) chained with encoder.layer_norm -> hid (the head's input) and last_hidden; then the CTC fine-tuning head of a BEST-RQ
// encoder (bestrq.py:229-279), which mixes the hidden states and / or enters the additional layer
int Fwd::encoder_exit(int l, float* last_hidden) const {
    const bool tune = c.layer_mixing || c.extra_layers;
    float* lh = (last_hidden || !tune) ? last_hidden : w.lh;     // the fine-tuning head needs the fp32 rows even when the caller does not
    RUN(mi_layernorm_chain(w.x, d, nullptr, T2, Lf(l, FIN_LN_G), Lf(l, FIN_LN_B), LEPS, nullptr, 0,
                           Gf(G_ENC_LN_G), Gf(G_ENC_LN_B), c.ln_eps, w.hid, d, lh, d, nullptr, nullptr, nullptr, 0, M, d, st));
    if (!tune) return MI_OK;
    const float* top = lh;
    if (c.layer_mixing) {
        RUN(mi_axpy_dev_f32(w.mixed, lh, (long)M * d, w.sw + c.L, 0, st));
        top = w.mixed;
    }
    return c.extra_layers ? enter_layer(top, c.L) : mi_add2_cast_bf16(top, d, nullptr, 0, w.hid, d, M, d, 1.f, st);
}

// CTC head: lm_head ⊕ blank_projection, blank LAST (e_branchformer.py:456-457), in its three forms: per-frame argmax (`best`), logits with their row log-sum-exp, logits.
// The fused forms (mi_gemm_argmax_bf16, mi_gemm_lse_f32) may refuse a shape; the head GEMM + a row pass then does the same.
int Fwd::ctc_head(void* logits, float* lse, float* lse_workspace, int* best, float* amax_workspace) const {
    if (!best && !logits) return MI_OK;
    const long ldl = c.logits_ld > 0 ? c.logits_ld : c.V + 1;
    int rc = MI_ERR_UNSUPPORTED;
    if (best && amax_workspace) rc = mi_gemm_argmax_bf16(w.hid, d, Gw(G_HEAD_W), d, Gf(G_HEAD_B), best, amax_workspace, M, c.V + 1, d, st);
    else if (!best && lse) rc = mi_gemm_lse_f32(w.hid, d, Gw(G_HEAD_W), d, Gf(G_HEAD_B), (float*)logits, ldl, lse, lse_workspace, M, c.V + 1, d, st);
    if (rc != MI_ERR_UNSUPPORTED) return rc;
    if (!logits) return MI_ERR_UNSUPPORTED;
    RUN(mi_gemm_bf16(w.hid, d, Gw(G_HEAD_W), d, Gf(G_HEAD_B), 1, logits, ldl, c.logits_f32, nullptr, 0, 1.f, 0, M, c.V + 1, d, 0, 0, st));
    if (best) return mi_row_argmax(logits, ldl, c.logits_f32 ? 0 : 1, c.V + 1, best, M, st);
    return lse ? mi_row_lse(logits, ldl, 0, c.V + 1, lse, M, st) : MI_OK;
}

}  // namespace

void launch_subsampled_lengths(const int* lengths, int T, int B, int K, int stride, int pad_total, int layers, int tmax, int* inner, int* outer, hipStream_t st) {
    hipLaunchKernelGGL(subsampled_lengths_kernel, dim3(cdiv(B, 64)), dim3(64), 0, st, lengths, T, B, K, stride, pad_total, layers, tmax, inner, outer);
}

extern "C" size_t mi_ebf_workspace_bytes(const mi_ebf_config* cfg) { return sizable(cfg) ? carve(*cfg, dims(*cfg), nullptr).bytes : 0; }

// posp: (L, 2*T2-1, d) bf16 projected relative positions, (re)computed from pos_table when compute_posp != 0
// hidden_states (nullable): (L+1, B*T2, d) fp32 = the tuple HF returns for output_hidden_states (tf:685-713): the input of every encoder layer, then the
// encoder's last hidden state (after encoder.layer_norm); needs last_hidden.  Device-to-device copies on the same stream, only when asked for.
// lse / lse_workspace (both or neither; fp32 logits only): lse (B*T2) fp32 = the row log-sum-exp of the logits out of the head GEMM's epilogue (mi_gemm_lse_f32;
// lse_workspace >= mi_gemm_lse_workspace_floats(B*T2, V+1) floats) — what the CTC loss needs beside the logits, without a second pass over them.
extern "C" int mi_gemm_lse_f32(const void* A, long lda, const void* W, long ldw, const float* bias, float* C, long ldc, float* lse, float* workspace,
                               int M, int N, int K, hipStream_t stream);
extern "C" int mi_row_lse(const void* x, long ld, int dtype, int V, float* lse, int M, hipStream_t stream);
// best (nullable; mi_ebf_forward_greedy): (B*T2) int32 = the per-frame argmax over the V+1 classes.  With amax_workspace the head is mi_gemm_argmax_bf16 and no logits
// exist; otherwise, or outside that kernel's shapes, the head GEMM runs into `logits` (here a scratch the caller lends) and mi_row_argmax reads it.
static int ebf_forward_body(const mi_ebf_config* cfg, const void* const* weights, const float* feats, const int* feat_lengths, const void* pos_table, void* posp, int compute_posp,
                            void* workspace, size_t workspace_bytes, float* last_hidden, void* logits, int* inner_len, int* outer_len, float* hidden_states,
                            float* lse, float* lse_workspace, int* best, float* amax_workspace, hipStream_t st) {
    if (!cfg || cfg->H <= 0) return MI_ERR_ARG;       // before anything divides by H
    MI_ENTER();
    const mi_ebf_config& c = *cfg;
    if ((lse != nullptr) != (lse_workspace != nullptr) || (lse && (!logits || !c.logits_f32))) return MI_ERR_ARG;
    if (hidden_states && !last_hidden) return MI_ERR_ARG;
    if (best && !amax_workspace && !logits) return MI_ERR_ARG;
    if (best && !logits && ((c.d % 64) != 0 || c.d < 128)) return MI_ERR_UNSUPPORTED;      // the fused head's K: known before the encoder runs
    if (c.B <= 0 || c.T <= 0 || c.L <= 0 || c.d % c.H || c.I % 2) return MI_ERR_ARG;
    if (c.extra_layers < 0 || c.extra_layers > 1 || (c.layer_mixing && c.L + 1 > 1024)) return MI_ERR_ARG;
    const int Lt = c.L + c.extra_layers;      // the fine-tuning head's additional layer (bestrq.py:247-274) is layer L of the weight table
    const Dims D = dims(c);
    if (D.T2 <= 0) return MI_ERR_ARG;
    const Ws w = carve(c, D, workspace);
    if (w.bytes > workspace_bytes) return MI_ERR_ARG;
    int* inner = inner_len ? inner_len : w.lens;
    int* outer = outer_len ? outer_len : w.lens + c.B;
    launch_subsampled_lengths(feat_lengths, c.T, c.B, c.K, c.stride, c.is_causal ? c.K - 1 : 2 * c.pad, 2, D.T2, inner, outer, st);
    const Fwd f(c, D, w, weights, st, feat_lengths ? inner : nullptr, pos_table, posp);

    RUN(f.front_end(feats));
    if (!c.ln_fold) RUN(f.enter_layer(w.x, 0));
    if (c.layer_mixing) RUN(mi_softmax_vec_f32(f.Gf(G_MIX_W), c.L + 1, w.sw, st));
    if (c.pos_type == 1 && compute_posp) RUN(f.project_positions(Lt));
    if (c.ln_fold) {
        if (c.pos_type == 2 || !c.use_macaron || c.extra_layers || c.layer_mixing || c.csgu_linear || (D.hd != 64 && D.hd != 128)) return MI_ERR_ARG;
        // entry: zero padded frames once (tf:662-665); x, bf16(x), statistics
        RUN(mi_layernorm_fold(w.x, c.d, f.mask_len, D.T2, nullptr, nullptr, 0.f, w.x, c.d, w.a0, c.d, w.lnst, D.M, c.d, st));
    }
    for (int l = 0; l < Lt; ++l) {
        if (l < c.L) RUN(f.keep_hidden(hidden_states, l, w.x));
        RUN(c.ln_fold ? f.folded_layer(l) : f.plain_layer(l, Lt));
        if (l + 1 == c.L) RUN(f.encoder_exit(l, last_hidden));
    }
    RUN(f.ctc_head(logits, lse, lse_workspace, best, amax_workspace));
    RUN(f.keep_hidden(hidden_states, c.L, last_hidden));
    MI_CHECK_LAUNCH();
    return MI_OK;
}

extern "C" int mi_ebf_forward_lse(const mi_ebf_config* cfg, const void* const* weights, const float* feats, const int* feat_lengths, const void* pos_table, void* posp, int compute_posp,
                                  void* workspace, size_t workspace_bytes, float* last_hidden, void* logits, int* inner_len, int* outer_len, float* hidden_states, float* lse, float* lse_workspace, hipStream_t st) {
    return ebf_forward_body(cfg, weights, feats, feat_lengths, pos_table, posp, compute_posp, workspace, workspace_bytes, last_hidden, logits, inner_len, outer_len,
                            hidden_states, lse, lse_workspace, nullptr, nullptr, st);
}

extern "C" int mi_ebf_forward_greedy(const mi_ebf_config* cfg, const void* const* weights, const float* feats, const int* feat_lengths, const void* pos_table, void* posp, int compute_posp,
                                     void* workspace, size_t workspace_bytes, float* last_hidden, int* best, float* argmax_workspace, void* head_scratch, int* inner_len, int* outer_len, hipStream_t st) {
    if (!best) return MI_ERR_ARG;
    return ebf_forward_body(cfg, weights, feats, feat_lengths, pos_table, posp, compute_posp, workspace, workspace_bytes, last_hidden, head_scratch, inner_len, outer_len,
                            nullptr, nullptr, nullptr, best, argmax_workspace, st);
}

extern "C" int mi_ebf_forward_hs(const mi_ebf_config* cfg, const void* const* weights, const float* feats, const int* feat_lengths, const void* pos_table, void* posp, int compute_posp,
                                 void* workspace, size_t workspace_bytes, float* last_hidden, void* logits, int* inner_len, int* outer_len, float* hidden_states, hipStream_t st) {
    return ebf_forward_body(cfg, weights, feats, feat_lengths, pos_table, posp, compute_posp, workspace, workspace_bytes, last_hidden, logits, inner_len, outer_len,
                            hidden_states, nullptr, nullptr, nullptr, nullptr, st);
}

extern "C" int mi_ebf_forward(const mi_ebf_config* cfg, const void* const* weights, const float* feats, const int* feat_lengths, const void* pos_table, void* posp, int compute_posp,
                              void* workspace, size_t workspace_bytes, float* last_hidden, void* logits, int* inner_len, int* outer_len, hipStream_t st) {
    return ebf_forward_body(cfg, weights, feats, feat_lengths, pos_table, posp, compute_posp, workspace, workspace_bytes, last_hidden, logits, inner_len, outer_len,
                            nullptr, nullptr, nullptr, nullptr, nullptr, st);
}
