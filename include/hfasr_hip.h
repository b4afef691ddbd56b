/* libhfasr_hip.so — C ABI of the MI355X (gfx950) hot path behind the BUTSpeechFIT/huggingface_asr model surface.
 *
 * The reference is 100 % Python and has no FFI of its own: its "plug-in" boundary is
 * HuggingFace's Auto-class registry (reference src/utilities/bind.py:36-58).  This header is the C boundary
 * that sits directly below that Python surface: one entry point per tensor op of the hot path, plus one
 * whole-encoder driver.  Every function
 *   - takes raw device pointers, element strides and sizes (no torch types), and a hipStream_t,
 *   - enqueues kernels on that stream and returns immediately (no allocation, no synchronisation,
 *     no global state; workspaces are passed in, so calls are hipGraph-capturable),
 *   - returns 0 (MI_OK) or a negative error code (MI_ERR_ARG -1, MI_ERR_LAUNCH -2, MI_ERR_UNSUPPORTED -3).
 * bf16 buffers are raw 2-byte bfloat16; "ld" arguments are row strides in ELEMENTS.
 * The reference-side binding is the ctypes loader in huggingface_asr_amd/_lib.py.
 */
#ifndef HFASR_HIP_H
#define HFASR_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ihipStream_t* mi_stream_t; /* = hipStream_t */

/* diagnostics: text of the last failed kernel launch on the calling thread ("" if none). */
const char* mi_last_error(void);

/* profiling facility (off by default; process-global, not thread-safe, not for production): while enabled, every launch of a dense contraction (GEMM /
 * implicit-GEMM conv) is started with hipExtLaunchKernelGGL and a start / stop event pair, i.e. its duration is the dispatch's own begin -> end timestamps —
 * what rocprofv3 --kernel-trace reports for the same launch — for bench.py's roofline.achieved. */
int mi_profile_create(int capacity);
void mi_profile_enable(int on);
void mi_profile_reset(void);
int mi_profile_count(void);
int mi_profile_summary(double* total_ms, double* total_flops);
int mi_profile_calibrate(mi_stream_t stream, int n, double* median_ms);   /* event pair around an EMPTY kernel, median of n: what the bracket adds + the empty kernel's ~1.3 us */
int mi_profile_summary_family(int family, double* total_ms, double* total_flops, int* launches);   /* family < 0: all; 0 gemm8p, 1 gemm8p+GELU, 2 gemm8p conv, 3 gemm8p fp32 out, 4 gemm8p128, 5 gemm_glds, 6 generic, 7 gemm8p argmax epilogue, 8 gemm8p cross-entropy epilogues */

/* ---- nn.Linear / lm_head / projections: C[M,N] = epi(A[M,K] * W[N,K]^T), bf16 in, fp32 accumulate (MFMA).
 * replaces: every nn.Linear on the path — reference src/models/encoders/e_branchformer.py:96-98,139,212-216,247,456-457;
 *           src/models/extractors.py:108,131; transformers wav2vec2_conformer FFN (modeling :350-357).
 * bias_mode 0 none / 1 per column / 2 per row; act 0 none / 1 gelu(erf);
 * resid != NULL: out = resid[m*ldr+n] + alpha*(acc+bias); out_f32 selects fp32 or bf16 C.
 * col_T/col_Tp != 0: output column n is remapped to (n / col_T) * col_Tp + n % col_T (time-padded V^T). */
int mi_gemm_bf16(const void* A, long lda, const void* W, long ldw, const float* bias, int bias_mode,
                 void* C, long ldc, int out_f32, const float* resid, long ldr, float alpha, int act,
                 int M, int N, int K, int col_T, int col_Tp, mi_stream_t stream);
/* the same with an explicit kernel selection (A/B runs, tests that must reach a kernel below the size its default dispatch picks it at): 0 = the product's
 * dispatch (= mi_gemm_bf16), 40 / 41 = phase-interleaved kernels wherever supported / never, 42 / 47 = the 128x128 phase kernel (pipelined / two-segment form),
 * 30 / 31 = the older 128x128 LDS-DMA tiles (persistent / one block per tile); 48 = the product's dispatch (as 0) without the tail-round split: with variant 0 a GEMM
 * whose 256x256 tiles leave a last round of the 256 CUs less than half full runs that round's rows on 128x128 tiles (same bits; callers with several batches in flight pass 48).
 * Per call — the library keeps no kernel-selection state. */
int mi_gemm_bf16_v(const void* A, long lda, const void* W, long ldw, const float* bias, int bias_mode,
                   void* C, long ldc, int out_f32, const float* resid, long ldr, float alpha, int act,
                   int M, int N, int K, int col_T, int col_Tp, int variant, mi_stream_t stream);

/* ---- Conv2d sub-sampling, second layer (C->C, KxK, stride s) as implicit GEMM over a channels-last activation.
 * replaces: src/models/extractors.py:71-96 (layers >= 1) incl. the causal left-padded form src/models/streaming_modules.py:31-55. */
int mi_conv2d_cl_bf16(const void* in, const void* weight, const float* bias, void* out,
                      int B, int Tin, int Fin, int Cin, int Cout, int KH, int KW, int stride,
                      int pad_t, int pad_f, int Tout, int Fout, int act, mi_stream_t stream);
int mi_conv2d_cl_bf16_v(const void* in, const void* weight, const float* bias, void* out,
                        int B, int Tin, int Fin, int Cin, int Cout, int KH, int KW, int stride,
                        int pad_t, int pad_f, int Tout, int Fout, int act, int variant, mi_stream_t stream);   /* variant: as mi_gemm_bf16_v */

/* ---- Conv2d sub-sampling, first layer (1->C) + GELU over the padded (B,T,F) fp32 log-mel layout; output channels-last bf16.
 * replaces: src/models/extractors.py:71-96 (layer 0) and :111. */
int mi_conv2d_first_gelu(const float* x, const float* w, const float* bias, void* out_cl_bf16,
                         int B, int T, int F, int C, int K, int stride, int pad_t, int pad_f,
                         int T1, int F1, mi_stream_t stream);

/* ---- context-aware Conv2d sub-sampling: `context_awareness_type` = "gated" / "gated_shared" (src/models/extractors.py:23-65; selected by
 *      recipes_v0.0.1/librispeech_aed/train_gated_baseline.sh:94, train_small_baseline_fp32_gated.sh:96).
 * GatedConv2d (:23-32): conv(x) * sigmoid(gate(x)), same geometry; GatedConv2dShared (:35-54): the gate is a (4k, k) / stride (4s, s) / padding (4p, p) conv, one
 * gate row per four output time steps (the conv's time axis must be divisible by 4: the reference's `view` raises otherwise).  The layer's GELU follows the product. */
/* Conv2d(1 -> C) of general geometry over the (B,T,F) fp32 features -> channels-last bf16; act 1: GELU, 0: raw pre-activation (operand of mi_gated_act_bf16) */
int mi_conv2d_first_geo(const float* x, const float* w, const float* bias, void* out_cl_bf16, int B, int T, int F, int C,
                        int KH, int KW, int stride_t, int stride_f, int pad_t, int pad_f, int T1, int F1, int act, mi_stream_t stream);
/* GatedConv2d as the first layer, fused (3x3): out = GELU((conv + b) * sigmoid(gate + bg)); MI_ERR_UNSUPPORTED for other kernel sizes (run the two raw convs + mi_gated_act_bf16) */
int mi_conv2d_first_gated_gelu(const float* x, const float* w, const float* bias, const float* gw, const float* gbias, void* out_cl_bf16,
                               int B, int T, int F, int C, int K, int stride, int pad_t, int pad_f, int T1, int F1, mi_stream_t stream);
/* mi_conv2d_cl_bf16 with separate time / frequency strides; gated != 0: GatedConv2d as ONE implicit GEMM — weight (2*Cout, KH*KW*Cin) / bias (2*Cout) hold conv and gate
 * filters interleaved in blocks of 32 output channels ([conv c0..c0+31 ; gate c0..c0+31]), out (B,Tout,Fout,Cout) = GELU((conv + b) * sigmoid(gate + bg)) in the epilogue
 * (act must be 1; Cout % 128 == 0, Cin % 64 == 0, else MI_ERR_UNSUPPORTED: run it with gated = 0, act = 0 into a (M, 2*Cout) buffer + mi_gated_act_bf16(blk = 32)). */
int mi_conv2d_cl_geo_bf16(const void* in, const void* weight, const float* bias, void* out, int B, int Tin, int Fin, int Cin, int Cout, int KH, int KW,
                          int stride_t, int stride_f, int pad_t, int pad_f, int Tout, int Fout, int act, int gated, mi_stream_t stream);
/* out (B*T*Fq, C) bf16 = GELU(z * sigmoid(g)), gate row of (b,t,f) = (b, t / share, f).  blk = 0: z (B*T*Fq, C), g (B*(T/share)*Fq, C) plain columns;
 * blk > 0: z == g is the output of one stacked GEMM whose columns are interleaved [conv blk | gate blk] per 2*blk (share must be 1). */
int mi_gated_act_bf16(const void* z, long ldz, const void* g, long ldg, void* out, long ldo, int B, int T, int Fq, int C, int share, int blk, mi_stream_t stream);

/* C (M,N) = [resid +] alpha * dropout(A W^T + b) from one launch of the 128 x 128 GEMM: fp32 out with optional fp32 residual (mask of mi_dropout_add_f32 for element m*N + n)
 * or bf16 out (resid NULL, alpha 1; mask and rounding of mi_dropout's bf16 form).  N % 128 == 0, K % 128 == 0, K >= 320, else MI_ERR_UNSUPPORTED.
 * replaces: a Linear followed by nn.Dropout under autograd (tf wav2vec2_conformer :355-357 output_dense + output_dropout; e_branchformer.py:288, 301). */
int mi_gemm_dropout_bf16(const void* A, long lda, const void* W, long ldw, const float* bias, void* C, long ldc, int out_f32, const float* resid, long ldr,
                         float alpha, float drop_p, unsigned seed, unsigned stream_id, int M, int N, int K, mi_stream_t stream);
/* Training epilogues of the 256 x 256 GEMM: the FFN's activation passes ride the GEMMs next to them (bit-identical to the GEMM + mi_act[_dropout]_{fwd,bwd}_bf16 pair).
 * forward: pre (M,N) bf16 = A W^T + b, h (M,N) bf16 = dropout(act(pre)); kind 1 erf-GELU / 2 tanh-GELU; drop_p = 0: none; mask of mi_dropout for (seed, stream_id).
 * backward: dX (M,N) bf16 = dropout(bf16(dY Wt^T)) * act'(pre), Wt (N,K) the transposed weight.  N % 256 == 0, K % 64 == 0, K >= 128, else MI_ERR_UNSUPPORTED.
 * replaces: Wav2Vec2ConformerFeedForward's intermediate_dense + intermediate_act_fn + intermediate_dropout (tf wav2vec2_conformer :350-354) and their autograd backward. */
int mi_gemm_act_fwd_bf16(const void* A, long lda, const void* W, long ldw, const float* bias, void* pre, long ldp, void* h, long ldh, int kind,
                         float drop_p, unsigned seed, unsigned stream_id, int M, int N, int K, mi_stream_t stream);
int mi_gemm_act_bwd_bf16(const void* dY, long ldy, const void* Wt, long ldw, const void* pre, long ldp, void* dX, long ldx, int kind,
                         float drop_p, unsigned seed, unsigned stream_id, int M, int N, int K, mi_stream_t stream);
/* ---- LayerNorm folded into the GEMMs around it (the engine's `ln_fold` path).  replaces: the same nn.LayerNorm + nn.Linear pairs as mi_layernorm_chain + mi_gemm_bf16
 *      (e_branchformer.py:233,236,242,261 in front of tf wav2vec2_conformer :350-357, e_branchformer.py:96-98,212), evaluated as
 *      LN(x) W^T + b = rstd (bf16(x) W'^T) - rstd mu s + (W beta + b),  W' = bf16(W diag(gamma)),  s_n = sum_k W'[n,k].
 * mi_gemm_lnfold_bf16: the consumer GEMM (256x256 phase kernel; MI_ERR_UNSUPPORTED for shapes it does not take); stats = per-row partial (sum, sumsq) pairs of x, row stride
 *   32 floats, npart pairs.  mi_gemm_resid_stats_f32: the producer — C fp32 = resid + alpha (A W^T + b), plus C2 = bf16(C) and the partial statistics of the rows it stores
 *   (one pair per 32 columns; 128x128 phase kernel).  mi_layernorm_fold: y = [LN](mask(x)) as fp32 + bf16 + statistics pair 0 (npart = 1).
 *   The statistics record: row m owns floats [32 m, 32 m + 32) of `stats` (16-B aligned), pair s = floats 2 s (sum) and 2 s + 1 (sum of squares); npart = 1 or 4, 8, 12, 16.
 *   mi_gemm_lnfold_bf16 reads floats 0 .. 2 npart - 1 of the records of rows 0 .. M - 1 and no other row's; with npart = 1 its 16-B load also covers floats 2 and 3 of the
 *   record, whose VALUES it ignores: they, like every float from 2 npart on, may hold anything, NaN and Inf bit patterns included, and need not be initialised.  The producers
 *   write exactly the pairs they own — mi_layernorm_fold floats 0 and 1, mi_gemm_resid_stats_f32 floats 0 .. 2 (N / 32) - 1 (variant 40: 2 (N / 64) - 1) — of rows 0 .. M - 1. */
int mi_gemm_lnfold_bf16(const void* xb, long lda, const void* Wf, long ldw, const float* colsum, const float* cbias, const float* stats, int npart, float eps,
                        void* C, long ldc, int act, int M, int N, int K, mi_stream_t stream);
int mi_gemm_resid_stats_f32(const void* A, long lda, const void* W, long ldw, const float* bias, float* C, long ldc, const float* resid, long ldr, float alpha,
                            void* C2, long ldc2, float* stats_out, int M, int N, int K, mi_stream_t stream);
/* the same with the kernel chosen by the caller: variant 40 = the 256 x 256 tile (N % 256 == 0; partial statistics then come one pair per 64 columns), 0 = as above */
int mi_gemm_resid_stats_f32_v(const void* A, long lda, const void* W, long ldw, const float* bias, float* C, long ldc, const float* resid, long ldr, float alpha,
                              void* C2, long ldc2, float* stats_out, int M, int N, int K, int variant, mi_stream_t stream);
int mi_layernorm_fold(const float* x, long ldx, const int* lengths, int T, const float* g1, const float* b1, float eps1, float* y32, long ldy,
                      void* yb_bf16, long ldyb, float* stats, int M, int d, mi_stream_t stream);

/* ---- LayerNorm chain on the fp32 residual stream (see csrc/norm.hip).
 * replaces: nn.LayerNorm at e_branchformer.py:233,236,242,257,261; feature projection LN (extractors.py:130);
 *           encoder.layer_norm (wav2vec2_conformer :707); zeroing of padded frames (:662-665) via `lengths`. */
int mi_layernorm_chain(const float* x, long ldx, const int* lengths, int T,
                       const float* g1, const float* b1, float eps1, float* y32, long ldy,
                       const float* ga, const float* ba, float eps2, void* outa_bf16, long lda,
                       float* outa_f32, long lda32,
                       const float* gb, const float* bb, void* outb_bf16, long ldb,
                       int M, int d, mi_stream_t stream);

/* ---- fp32 -> bf16 cast of a (M,d) state (A operand of a following GEMM). */
int mi_cast_f32_bf16(const float* x, long ldx, void* out, long ldo, int M, int d, mi_stream_t stream);

/* ---- rotary embedding of the Q/K projection input. replaces: wav2vec2_conformer _apply_rotary_embedding (:509-526). */
int mi_rotary_bf16(const void* x, long ldx, void* out, long ldo, const float* cos_t, const float* sin_t,
                   int M, int T, int H, int hd, mi_stream_t stream);

/* ---- fused self-attention (relative-position / rotary / plain), key-padding + optional causal mask.
 * replaces: Wav2Vec2EBranchformerSelfAttention.forward e_branchformer.py:100-138 and
 *           _apply_relative_embeddings wav2vec2_conformer :528-565.  pos == NULL: no relative term. */
int mi_attention_bf16(const void* q, long ldq, const void* k, long ldk, const void* vt, long ldvt, int Tp,
                      const void* pos, long ldp, const float* bias_u, const float* bias_v,
                      const int* lengths, void* out, long ldo, int B, int T, int H, int hd,
                      float scale, int causal, mi_stream_t stream);

/* LDS-staged form for head sizes 64 / 128: q, k, v are columns of ONE fused (B*T, 3d) projection (all [row][hd]),
 * no transposed V copy; the position rows / K / V tiles are shared by the 4 waves of a 128-query block. */
int mi_attention_qkv_bf16(const void* q, long ldq, const void* k, long ldk, const void* v, long ldv,
                          const void* pos, long ldp, const float* bias_u, const float* bias_v,
                          const int* lengths, void* out, long ldo, int B, int T, int Tk, long kv_bstride, int H, int hd,
                          float scale, int causal, mi_stream_t stream);
/* A/B form of mi_attention_qkv_bf16: variant 0 = the library's choice (the eight-wave kernel: two waves per SIMD, the wave pair of a query group splits the keys),
 * except with relative positions at head size 64), 1 = the four-wave kernel of rounds 1-3, 2 = the eight-wave kernel.  Measurement (tools/attn_ab.py) and tests (tests/test_gpu_attention_probes.py) only; no product
 * call site passes a non-zero variant. */
int mi_attention_qkv_bf16_v(const void* q, long ldq, const void* k, long ldk, const void* v, long ldv,
                            const void* pos, long ldp, const float* bias_u, const float* bias_v,
                            const int* lengths, void* out, long ldo, int B, int T, int Tk, long kv_bstride, int H, int hd,
                            float scale, int causal, int variant, mi_stream_t stream);
/* (kv_bstride = elements between batches of k/v, 0 = Tk*ld (KV caches are (B, Lmax, d)); T = queries per batch, Tk = keys per batch, 0 = T: cross-attention over encoder frames and KV-cache decoding use Tk != T;
 *  with causal != 0 query i sees keys <= i + (Tk - T); causal with 0 < Tk < T leaves the first queries without a key and is MI_ERR_ARG, here and in the
 *  mi_attention_x_* entries below.) */

/* Training form of the above (self-attention only, Tk = T): also leaves each row's log-sum-exp of the scaled scores (log2 domain) in lse (B, H, T) fp32,
 * which mi_attention_qkv_bwd_probs needs.  replaces: the forward half of Wav2Vec2EBranchformerSelfAttention under autograd, e_branchformer.py:105-138. */
int mi_attention_qkv_lse_bf16(const void* q, long ldq, const void* k, long ldk, const void* v, long ldv,
                              const void* pos, long ldp, const float* bias_u, const float* bias_v,
                              const int* lengths, void* out, long ldo, float* lse, int B, int T, int H, int hd,
                              float scale, int causal, float drop_p, unsigned seed, unsigned stream_id, mi_stream_t stream);
/* (drop_p > 0: attention-probability dropout, e_branchformer.py:132 — the normaliser keeps every key, the context sums the survivors / (1 - p); mask of mi_dropout for the
 *  logical element ((h*B + b)*T + i)*T + j of the (H,B,T,T) probabilities, the one mi_attn_softmax_fwd draws) */
/* First half of the attention backward (what autograd derives from e_branchformer.py:105-138 and the rel-shift of tf wav2vec2_conformer :528-565): one walk over
 * the keys recomputes the scores, P = 2^(S - lse), dP = dctx V^T, dS = P (dP - dctx·ctx) scale, and leaves bf16
 *   prob, ds (H, B, T, ldsr)   and   dbd (H, B, T, ldbd), dbd[i][T-1-i+j + pad] = ds[i][j]  (the gradient of the un-shifted position scores; null without pos).
 * It also accumulates the query gradient over the walk: dq (B*T, lddq) bf16 = dS K + dBD P, and the per-wave column sums of the two terms in
 * dsum_u / dsum_v (B, 4 ceil(T/128), H*hd) fp32 (summed over their first two axes: the pos_bias_u / pos_bias_v gradients; unused without pos).
 * dsum_v == dsum_u + H*hd selects the interleaved layout: ONE (B * 4 ceil(T/128), 2 H*hd) buffer whose rows are [u | v] — the shape mi_ln_partial_reduce_many sums
 * (desc kind 0 with d = H*hd, dgamma = the pos_bias_u gradient, dbeta = the pos_bias_v gradient), so the reduction can leave with a later launch.
 * ldsr, ldbd multiples of 32 with ldsr >= T rounded up to 32 and ldbd >= pad + 2T - 1; 0 <= pad < 32 with (T - 32 + pad) % 32 == 0.  Every element is written
 * (but see flags).
 * qu_out / qv_out (both or neither, with pos only; else null): (B*T, ldqb) bf16 = q + pos_bias_u / q + pos_bias_v, the walk's own A fragments — the operands of the
 * dK = dS^T (q + u) and d(positions) = dBD^T (q + v) products that follow, which a pass of their own used to make.
 * flags bit 0, sparse writes: the zeros nobody reads are not written — `dbd` must be a buffer the caller zero-filled ONCE and that only this entry writes (a row's
 * relative positions outside its maximal band are the same for every launch), and columns of prob / ds from the key length rounded up to 128 on must never be read
 * (mi_bgemm_sparse_bf16 with m_valid = lengths does not read them).  Other bits must be 0. */
int mi_attention_qkv_bwd_probs(const void* q, long ldq, const void* k, long ldk, const void* v, long ldv,
                               const void* pos, long ldp, const float* bias_u, const float* bias_v, const int* lengths,
                               const void* ctx, long ldo, const void* dctx, long ldd, const float* lse,
                               void* prob, void* ds, long ldsr, void* dbd, long ldbd, int pad,
                               void* dq, long lddq, float* dsum_u, float* dsum_v, void* qu_out, void* qv_out, long ldqb,
                               int B, int T, int H, int hd, float scale, int causal, float drop_p, unsigned seed, unsigned stream_id, int flags, mi_stream_t stream);
/* Attention backward for the fused (B*T, 3d) projection with no (H, B, T, T) tensor in HBM (attn_bwd_fused.hip): no relative positions, no dropout, hd 64 / 128.
 * P and dS are recomputed from q, k and the forward's lse (mi_attention_qkv_lse_bf16); dq / dk / dv are row views of one (B*T, ldg) bf16 buffer, every row written.
 * workspace: >= B*T*H*4 bytes.  No atomics: the result is bitwise reproducible. */
int mi_attention_qkv_bwd_fused(const void* q, const void* k, const void* v, long ldqkv, const int* lengths,
                               const void* ctx, long ldo, const void* dctx, long ldd, const float* lse,
                               void* dq, void* dk, void* dv, long ldg, void* workspace, size_t ws_bytes,
                               int B, int T, int H, int hd, float scale, mi_stream_t stream);
/* the two entries above for Tq != Tk and separate q / k / v operands, no relative positions: the GPT-2 decoder's causal self-attention and its cross-attention over the
 * encoder frames in training (multi_head_gpt2.py:80-170).  lse (B, H, Tq); prob / ds (H, B, Tq, ldsr) bf16, ldsr % 32 == 0, ldsr >= Tk rounded up to 32; dq = dS K. */
int mi_attention_x_lse_bf16(const void* q, long ldq, const void* k, long ldk, const void* v, long ldv, const int* lengths, void* out, long ldo, float* lse,
                            int B, int Tq, int Tk, int H, int hd, float scale, int causal, float drop_p, unsigned seed, unsigned stream_id, mi_stream_t stream);
int mi_attention_x_bwd_probs(const void* q, long ldq, const void* k, long ldk, const void* v, long ldv, const int* lengths, const void* ctx, long ldo,
                             const void* dctx, long ldd, const float* lse, void* prob, void* ds, long ldsr, void* dq, long lddq,
                             int B, int Tq, int Tk, int H, int hd, float scale, int causal, float drop_p, unsigned seed, unsigned stream_id, mi_stream_t stream);
/* (drop_p / seed / stream_id as given to the forward: prob then holds the DROPPED probabilities, ds the gradient through the un-dropped softmax) */

/* ---- cgMLP gate: per-row LN statistics + fused LN -> depthwise conv(time) -> gate.
 * replaces: ConvolutionalSpatialGatingUnit.forward e_branchformer.py:184-204. */
int mi_row_stats_bf16(const void* x, long ldx, int d, float eps, float* stats, int M, mi_stream_t stream);
int mi_csgu_bf16(const void* u, long ldu, const float* stats, const float* gamma, const float* beta,
                 const float* w, const float* bias, void* out, long ldo,
                 int B, int T, int C, int K, int pad_left, int dilation, int act, mi_stream_t stream);

/* ---- merge block depthwise conv + residual. replaces: e_branchformer.py:296-299. */
int mi_dwconv_residual_bf16(const void* m, long ldm, const float* w, const float* bias, void* out, long ldo,
                            int B, int T, int C, int K, int pad_left, mi_stream_t stream);
/* the split CSGU form — `csgu_use_linear_after_conv` (e_branchformer.py:172-175,196-201: conv -> Linear -> act -> gate) and, on the training path, any
   csgu_activation other than identity:  conv alone (out = dwconv(LN(x_g)) + b), then [a GEMM], then out = x_r * act(g)  (act: 0 identity, 1 gelu, 2 relu, 3 silu) */
int mi_csgu_conv_bf16(const void* u, long ldu, const float* stats, const float* gamma, const float* beta, const float* w, const float* bias,
                      void* out, long ldo, int B, int T, int C, int K, int pad_left, int dilation, mi_stream_t stream);
int mi_gate_act_mul_bf16(const void* r, long ldr, const void* g, long ldg, void* out, long ldo, long M, int C, int act, mi_stream_t stream);
/* dr = ds * act(g),  dg = ds * x_r * act'(g) */
int mi_gate_act_mul_bwd_bf16(const void* r, long ldr, const void* g, long ldg, const void* ds, long ldds, void* dr, long lddr, void* dg, long lddg,
                             long M, int C, int act, mi_stream_t stream);

/* ---- log-mel front end. replaces: CustomFeatureExtractor.__call__ (src/utilities/feature_extractors.py:51-61) =
 *      Speech2TextFeatureExtractor._extract_fbank_features / utterance_cmvn (transformers) / global_normalize (:47-49). */
int mi_fbank_f64(const float* wave, long ldw, const int* num_samples, int N, const double* window,
                 const double* twiddle, const double* mel_t, const int* mel_lo, const int* mel_hi,
                 float* out, int T_out, int B, int nmel, double mel_floor, double preemph, mi_stream_t stream);
/* replaces: DataPreprocessingManagerCallback.default_transform's array handling (src/utilities/callbacks.py:108-118: audio_object_stripper =
   np.trim_zeros, src/utilities/data_utils.py:173-177, then zero-pad to >= min_len = 8000 samples) for clips that are already on the device. */
int mi_trim_zeros_pad_f32(const float* wave, long ldw, const int* num_samples, int N, int B, int min_len, float* out, long ldo, int N_out,
                          int* first, int* valid, int* eff_len, mi_stream_t stream);
int mi_cmvn_utterance(float* x, const int* frames, int B, int T, int nmel, int norm_means, int norm_vars,
                      float pad, mi_stream_t stream);
int mi_cmvn_global(float* x, long total, int nmel, const float* means, const float* stds, mi_stream_t stream);

/* ---- CTC tail. replaces: log_softmax + F.ctc_loss at e_branchformer.py:472-488. */
int mi_row_lse(const void* x, long ld, int dtype, int V, float* lse, int M, mi_stream_t stream);
/* the CTC head (reference e_branchformer.py:456-457, 472-488: lm_head + blank projection, then log_softmax) as ONE pass over the logits: C (M,N) fp32 = A W^T + b with
 * the rows' log-sum-exp lse (M) — the GEMM's epilogue leaves a (max, sum exp) pair per row and 64 columns in `workspace` (mi_gemm_lse_workspace_floats(M, N) floats), a small
 * second launch merges them.  lse equals mi_row_lse's up to the order of the sums.  MI_ERR_UNSUPPORTED outside the 256 x 256 kernel's shapes (K % 64, K >= 128, 16-B aligned
 * operands, ldc % 4 == 0): the caller runs mi_gemm_bf16 + mi_row_lse. */
size_t mi_gemm_lse_workspace_floats(int M, int N);
int mi_gemm_lse_f32(const void* A, long lda, const void* W, long ldw, const float* bias, float* C, long ldc, float* lse, float* workspace,
                    int M, int N, int K, mi_stream_t stream);
/* ---- CTC greedy transcription. replaces: ctc_greedy_decode (src/utilities/eval_utils.py:37-43: torch.argmax, then a Python groupby over a device tensor), the step
 * between the CTC head and a transcript in src/trainers/train_ctc_asr.py:77-85.
 * best[m] = argmax over the V1 columns of row m with torch.argmax's rules: the lowest index among equal maxima, a NaN beats every number (the first NaN wins), an
 * all -inf row gives 0.  dtype 0 fp32 / 1 bf16; one pass over the rows. */
int mi_row_argmax(const void* x, long ld, int dtype, int V1, int* best, int M, mi_stream_t stream);
/* best (B, T) int32 -> frame t of utterance b is kept iff t < n_b, best != blank and (t == 0 or best[t] != best[t-1]); n_b = lengths[b] (int32, clamped to [0, T]) or T
 * when lengths is null.  tokens (B, T) int32 (tokens_dtype 0) / int64 (1): the kept ids in order, then pad_id; n_tokens (B) int32; frames (B, T) int32 (nullable): the
 * frame each kept token starts at, then -1.  tokens must not alias best.  One block per utterance, any T, no atomics. */
int mi_ctc_collapse(const int* best, int B, int T, const int* lengths, int blank, long pad_id, void* tokens, int tokens_dtype, int* n_tokens, int* frames,
                    mi_stream_t stream);
/* the two above over logits (B, T, V1) with element strides (ld_batch, ld_row); best (B, T) int32: scratch of the caller, left holding the per-frame classes */
int mi_ctc_greedy(const void* logits, long ld_row, long ld_batch, int dtype, int B, int T, int V1, const int* lengths, int blank, long pad_id,
                  int* best, void* tokens, int tokens_dtype, int* n_tokens, int* frames, mi_stream_t stream);

/* ---- CTC prefix beam search (csrc/ctc_beam.hip, whose header states the semantics): the sum-over-alignments search, NOT a clone of the flashlight decoder behind the
 * reference's ctc_beam_decode (src/utilities/eval_utils.py:46-62).  Two launches.
 * mi_ctc_beam_cut: one pass over logits (B, T, V1) fp32 (dtype 0) / bf16 (1) with element strides (ld_batch, ld_row), rows t < n_b only (n_b = lengths[b] clamped to
 * [0, T], or T when lengths is null): lse (B, T) the rows' log-sum-exp, lp_blank (B, T) = x[blank] - lse, cut_lp / cut_id (B, T, K) the min(K, V1 - 1) non-blank classes
 * with the largest logits as (x - lse, class), best first, equal values by lower class (entries past V1 - 1: -inf / -1).
 * mi_ctc_beam_walk: one block per utterance walks its frames with W hypotheses over the cut (the same logits, lengths, blank and K as the cut) and writes the nbest <= W
 * best, best first: tokens (B, nbest, T) int32 (tokens_dtype 0) / int64 (1) then pad_id, n_tokens (B, nbest) int32, scores (B, nbest) fp32, frames (B, nbest, T) int32
 * (nullable): the frame at which each token's prefix first entered the beam, then -1; rows beyond the hypotheses that exist: 0, -inf, pad_id / -1.  workspace:
 * mi_ctc_beam_workspace_bytes(B, T, W) bytes, 16-B aligned, contents irrelevant before and after.  No float atomics: bit-identical run to run.
 * MI_ERR_ARG before any launch: W or K outside 1..64, nbest outside 1..W, blank outside [0, V1), V1 < 2.  MI_ERR_UNSUPPORTED: V1 > 2^20 or T W >= 2^22 - 2. */
size_t mi_ctc_beam_workspace_bytes(int B, int T, int W);
int mi_ctc_beam_cut(const void* logits, long ld_row, long ld_batch, int dtype, int B, int T, int V1, const int* lengths, int blank, int K, float* lse, float* lp_blank,
                    float* cut_lp, int* cut_id, mi_stream_t stream);
int mi_ctc_beam_walk(const void* logits, long ld_row, long ld_batch, int dtype, int B, int T, int V1, const int* lengths, int blank, long pad_id, int W, int K, int nbest,
                     const float* lse, const float* lp_blank, const float* cut_lp, const int* cut_id, void* workspace, size_t workspace_bytes, void* tokens,
                     int tokens_dtype, int* n_tokens, float* scores, int* frames, mi_stream_t stream);
/* ---- CTC prefix beam search on a stream (csrc/ctc_beam_stream.hip, whose header states the semantics): the walk above suspended between calls.  After every call the
 * beam is bit for bit the beam mi_ctc_beam_walk holds after the same number of frames of the concatenated logits, for every partition of the frames into calls.
 * mi_ctc_beam_stream_state_bytes: bytes of the state of B streams of at most max_frames frames with W hypotheses: per stream a 16-word header, the beam (7 x 64 words),
 * the node arena (1 + max_frames W nodes of 16 B) and the node table (the power of two >= 2 (1 + max_frames W) 64-bit words).  Host arithmetic; 0 for arguments the
 * walk refuses.
 * mi_ctc_beam_stream_reset: every stream back to its start (the empty hypothesis, score 0; nothing walked, nothing committed; the node table zeroed — the walk never
 * clears it).  state: 16-B aligned, state_bytes >= the above.
 * mi_ctc_beam_stream_walk: walks the n_valid[b] (clamped to [0, T_call]; T_call when null) first rows of this call's logits (B, T_call, V1) (dtype, strides, blank, W,
 * K as mi_ctc_beam_walk; lse / lp_blank / cut_lp / cut_id: mi_ctc_beam_cut's tables for THESE rows).  T_call = 0 is a call without frames (logits and tables may be
 * null).  A stream never walks past max_frames frames.  Then the committed prefix — the longest common prefix of all hypotheses of the beam; with final = 1 the whole
 * best hypothesis — is appended to committed / committed_frames (B, max_frames) int32 (token, and the frame at which its prefix entered the beam); n_committed (B) its
 * length, n_new (B) the tokens this call appended.  tokens not null (required with final = 1): the nbest best as mi_ctc_beam_walk writes them, rows max_frames wide
 * (tokens (B, nbest, max_frames), n_tokens, scores (B, nbest), frames nullable); null: no backtrace.  No float atomics: bit-identical run to run; a stream's result
 * does not depend on the rest of the batch.  MI_ERR_ARG before any launch as mi_ctc_beam_walk, and for final outside {0, 1}, final without tokens, a state that is too
 * small or not 16-B aligned; MI_ERR_UNSUPPORTED: V1 > 2^20 or max_frames W >= 2^22 - 2. */
size_t mi_ctc_beam_stream_state_bytes(int B, int max_frames, int W);
int mi_ctc_beam_stream_reset(void* state, size_t state_bytes, int B, int max_frames, int W, mi_stream_t stream);
int mi_ctc_beam_stream_walk(const void* logits, long ld_row, long ld_batch, int dtype, int B, int T_call, int V1, const int* n_valid, int blank, long pad_id, int W, int K,
                            int nbest, const float* lse, const float* lp_blank, const float* cut_lp, const int* cut_id, void* state, size_t state_bytes, int max_frames,
                            int final, int* committed, int* committed_frames, int* n_committed, int* n_new, void* tokens, int tokens_dtype, int* n_tokens,
                            float* scores, int* frames, mi_stream_t stream);
/* ---- ... on the slots of a session pool (csrc/ctc_beam_pool.hip, whose header states the semantics): the beam stream above per slot, each slot with rows, an end and
 * a start of its own.  State: mi_ctc_beam_stream_state_bytes(S, max_frames, W), started once by mi_ctc_beam_stream_reset.
 * mi_ctc_beam_stream_reset_slot: one slot back to a stream start, enqueued on `stream`, no synchronisation: its header, start beam and arena root are written and its
 * node table — and nothing else — is zeroed: a memset of 8 table_words(max_frames, W) bytes per call (256 KiB at max_frames = 1500, W = 10; 2 MiB at W = 64).  No
 * other slot is written.  MI_ERR_ARG: slot outside [0, S), and what mi_ctc_beam_stream_reset refuses.
 * mi_ctc_beam_stream_walk_slots: A records of five ints [slot, row0, n, final, out], given twice as the pool's tables are: records_host is checked, records_dev (the
 * same ints on the DEVICE) is read by the kernel.  logits (rows, V1) compact with row stride ld_row; lse / lp_blank / cut_lp / cut_id: mi_ctc_beam_cut's tables over
 * those rows (B = 1, T = rows, ld_batch = 0); rows = 0: all five may be null.  A record walks rows [row0, row0 + n) as the next frames of its slot (never past
 * max_frames; n = 0 leaves the beam as read), then appends the committed prefix — with final = 1 the rest of the best hypothesis — to row `slot` of committed /
 * committed_frames (S, max_frames) and writes n_committed / n_new (S) at `slot`.  out >= 0: the nbest best are backtraced into row `out` of tokens (R, nbest,
 * max_frames) int32 (tokens_dtype 0) / int64 (1), n_tokens / scores (R, nbest), frames (R, nbest, max_frames; nullable); out = -1: no backtrace.  Nothing of a slot
 * that no record names is read or written.  No float atomics; a slot's result does not depend on the other records, their order or its slot index.
 * MI_ERR_ARG before any launch: a slot outside [0, S) or named twice; row0 / n negative or row0 + n > rows; final outside {0, 1}; out outside [-1, R) or used twice;
 * final = 1 with out = -1; A outside 1..S; R outside 0..A; R > 0 without tokens / n_tokens / scores; and whatever mi_ctc_beam_stream_walk refuses.
 * MI_ERR_UNSUPPORTED as mi_ctc_beam_stream_walk. */
int mi_ctc_beam_stream_reset_slot(void* state, size_t state_bytes, int S, int max_frames, int W, int slot, mi_stream_t stream);
int mi_ctc_beam_stream_walk_slots(const void* logits, long ld_row, int dtype, int rows, int V1, int blank, long pad_id, int W, int K, int nbest, const float* lse,
                                  const float* lp_blank, const float* cut_lp, const int* cut_id, void* state, size_t state_bytes, int S, int max_frames,
                                  const int* records_host, int A, const int* records_dev, int* committed, int* committed_frames, int* n_committed, int* n_new,
                                  void* tokens, int tokens_dtype, int* n_tokens, float* scores, int* frames, int R, mi_stream_t stream);
/* ---- Contextual biasing of the CTC prefix beam search (csrc/ctc_beam_bias.hip, whose header states the semantics): the three searches above with a phrase list.  A
 * hypothesis is selected and ranked by score + weight (float)n, n the credit of its label prefix in the phrase automaton; `scores` stay the CTC log-probabilities.
 * The context, the same arguments in every entry: bias_col (V1) int32 a token's alphabet column (0: in no phrase), bias_tab (S, A1) int32 the word (dn << 16) | next
 * per (state, column), 1 <= S <= 4096, 1 <= A1 <= 1024, S A1 <= 2^20, weight finite (huggingface_asr_amd/ctc_bias.py compiles them).  The kernels clamp every index
 * they read from the tables into the tables.  credit: int32, a row of nbest beside every row of scores = n per hypothesis, 0 for rows that do not exist.
 * mi_ctc_beam_walk_bias: mi_ctc_beam_walk (the cut is mi_ctc_beam_cut as it is; the same workspace) with the context and credit (B, nbest).
 * mi_ctc_beam_bias_stream_state_bytes: mi_ctc_beam_stream_state_bytes + 512 B: behind the unbiased state, per stream the carried (state, credit) of its 64 hypotheses.
 * mi_ctc_beam_bias_stream_reset / _walk: mi_ctc_beam_stream_reset / _walk on that state; credit (B, nbest) is written wherever the n best are (required with tokens).
 * mi_ctc_beam_bias_stream_reset_slot / _walk_slots: mi_ctc_beam_stream_reset_slot / _walk_slots on that state (S slots; the automaton's states are S_bias); credit
 * (R, nbest), required with R > 0.  One context per pool; a stream or session keeps its context from start to end.
 * MI_ERR_ARG before any launch: whatever the unbiased counterpart refuses, null tables, S, A1 or S A1 outside the limits, a weight that is not finite, a missing credit.
 * MI_ERR_UNSUPPORTED as the counterpart.  With weight = 0 every output equals the counterpart's, bit for bit. */
int mi_ctc_beam_walk_bias(const void* logits, long ld_row, long ld_batch, int dtype, int B, int T, int V1, const int* lengths, int blank, long pad_id, int W, int K,
                          int nbest, const float* lse, const float* lp_blank, const float* cut_lp, const int* cut_id, void* workspace, size_t workspace_bytes, void* tokens,
                          int tokens_dtype, int* n_tokens, float* scores, int* frames, const int* bias_col, const int* bias_tab, int S, int A1, float weight, int* credit,
                          mi_stream_t stream);
size_t mi_ctc_beam_bias_stream_state_bytes(int B, int max_frames, int W);
int mi_ctc_beam_bias_stream_reset(void* state, size_t state_bytes, int B, int max_frames, int W, mi_stream_t stream);
int mi_ctc_beam_bias_stream_walk(const void* logits, long ld_row, long ld_batch, int dtype, int B, int T_call, int V1, const int* n_valid, int blank, long pad_id, int W,
                                 int K, int nbest, const float* lse, const float* lp_blank, const float* cut_lp, const int* cut_id, void* state, size_t state_bytes,
                                 int max_frames, int final, int* committed, int* committed_frames, int* n_committed, int* n_new, void* tokens, int tokens_dtype,
                                 int* n_tokens, float* scores, int* frames, const int* bias_col, const int* bias_tab, int S, int A1, float weight, int* credit,
                                 mi_stream_t stream);
int mi_ctc_beam_bias_stream_reset_slot(void* state, size_t state_bytes, int S, int max_frames, int W, int slot, mi_stream_t stream);
int mi_ctc_beam_bias_stream_walk_slots(const void* logits, long ld_row, int dtype, int rows, int V1, int blank, long pad_id, int W, int K, int nbest, const float* lse,
                                       const float* lp_blank, const float* cut_lp, const int* cut_id, void* state, size_t state_bytes, int S, int max_frames,
                                       const int* records_host, int A, const int* records_dev, int* committed, int* committed_frames, int* n_committed, int* n_new,
                                       void* tokens, int tokens_dtype, int* n_tokens, float* scores, int* frames, int R, const int* bias_col, const int* bias_tab,
                                       int S_bias, int A1, float weight, int* credit, mi_stream_t stream);
/* ---- CTC forced alignment (csrc/ctc_align.hip, whose header states the exact semantics): the best (Viterbi) path of a given transcript, one launch, one block per
 * utterance.  Arguments as mi_ctc_loss_fwd: logits (B, T, V1) fp32 (dtype 0) / bf16 (1) with element strides (ld_b, ld_t), lse (B*T) the rows' log-sum-exp, labels
 * (B, U) int64 (negative entries are padding wherever they stand), in_len (B) int32 clamped to [0, T].  Out: path (B, T) int32 = the class of every frame t < n_b on
 * the best path, then -1; score (B) fp32 = that path's log-probability; tgt_len (B) int32; start / end (B, U) int32 = token u emits on frames [start, end), then -1;
 * token_lp (B, U) fp32 = the sum of the token's log-probabilities over those frames, then 0 (the last three nullable as a group).  Infeasible utterances (too few
 * frames, a label >= V1 or == blank, a best score of -inf): score -inf, path / start / end -1, token_lp 0.  workspace: mi_ctc_align_workspace_bytes(B, T, U) bytes
 * (0 where the backpointers fit in LDS: workspace may then be null), 16-B aligned, contents irrelevant before and after.  No atomics: bit-identical run to run.
 * MI_ERR_ARG before any launch: V1 < 2, blank outside [0, V1), T < 1, U < 0, B < 1, a bad dtype, a workspace too small or misaligned.  MI_ERR_UNSUPPORTED: U > 1023
 * or T > 2^20. */
size_t mi_ctc_align_workspace_bytes(int B, int T, int U);
int mi_ctc_align(const void* logits, long ld_b, long ld_t, int dtype, const float* lse, int T, const long* labels, int U, const int* in_len, int blank, int V1, int B,
                 void* workspace, size_t workspace_bytes, int* path, float* score, int* tgt_len, int* start, int* end, float* token_lp, mi_stream_t stream);
/* the CTC head without its logits: best[m] = argmax_n (A W^T + b)[m][n] out of the 256 x 256 GEMM's epilogue, which leaves one (max, index) pair per row and 64 columns
 * in `workspace` (mi_gemm_argmax_workspace_floats(M, N) floats) and stores no C; a small second launch folds a row's pairs.  Equals mi_row_argmax over the fp32 output of
 * mi_gemm_bf16 on the same operands.  MI_ERR_UNSUPPORTED outside that kernel's shapes (K % 64, K >= 128, 16-B aligned operands): the caller runs mi_gemm_bf16 into a
 * scratch + mi_row_argmax. */
size_t mi_gemm_argmax_workspace_floats(int M, int N);
int mi_gemm_argmax_bf16(const void* A, long lda, const void* W, long ldw, const float* bias, int* best, float* workspace, int M, int N, int K, mi_stream_t stream);
/* ---- Language-model head with the cross-entropy in its epilogue. replaces: proj_out (the tied (V, d) embedding) + CrossEntropyLoss of transformers'
 * WhisperForConditionalGeneration.forward under train_enc_dec_asr.py, forward and backward, without the (M, N) fp32 logits (1.5 GB at Whisper-small, 16 x 448 rows).
 * forward: labels (M) int64, negative = ignored (CrossEntropyLoss's ignore_index; a label >= N counts as ignored too).  The 256 x 256 GEMM's epilogue leaves the LSE partials
 * in `workspace` (mi_gemm_lse_workspace_floats(M, N) floats) and target[m] = the logit of class labels[m] (rows without a valid label: not written); a merge launch gives
 * lse[m] and nll[m] = lse[m] - target[m] (exactly 0 for ignored rows), one block sums them in a fixed order: acc = [sum, count of valid rows] (written, not added to).
 * backward: the accumulators are recomputed, dlogits (M, ldo) bf16 = g[m] * (exp(x - lse[m]) - [n == labels[m]]) for n < N and zeros for N <= n < ldo (ldo % 8 == 0:
 * mi_ce_label_smoothing_bwd's layout); g (M) fp32 = 0 for ignored rows, else weight / count.  No float atomics.  MI_ERR_UNSUPPORTED outside the 256 x 256 kernel's
 * shapes (K % 64, K >= 128, 16-B aligned operands, 32-bit source offsets; backward: ldo <= 256 * ceil(N / 256)): the caller materialises the logits. */
int mi_gemm_ce_f32(const void* A, long lda, const void* W, long ldw, const float* bias, const long* labels, float* acc, float* lse, float* nll, float* target,
                   float* workspace, int M, int N, int K, mi_stream_t stream);
int mi_gemm_ce_bwd_bf16(const void* A, long lda, const void* W, long ldw, const float* bias, const long* labels, const float* lse, const float* g,
                        void* dlogits, long ldo, int M, int N, int K, mi_stream_t stream);
int mi_ctc_loss_fwd(const void* logits, long ld_b, long ld_t, int dtype, const float* lse, int T,
                    const long* labels, int U, const int* in_len, int blank, int B,
                    int reduction, int zero_infinity, float* nll, int* tgt_len, float* loss, mi_stream_t stream);

/* ---- joint CTC/attention decoding: batched CTC prefix scores on device.
 * replaces: CTCPrefixScoreTH.__call__ / index_select_state (src/decoding/ctc_scorer.py:58-207) as driven by
 *           CTCRescorerLogitsProcessor.__call__ (:324-354).  x: (B,T,O) padded log-posteriors; r: (T,2,B*W) forward variables. */
int mi_ctc_prefix_prepare(const void* logits, long ld_b, long ld_t, int dtype, const int* lens, int B, int T, int O,
                          int blank, int W, float* lse_scratch, float* x_out, float* r0_out, mi_stream_t stream);
int mi_ctc_prefix_score(const float* x, int B, int T, int O, int blank, int W, const float* r_prev, const long* last_ids,
                        long ld_last, int out_len, const float* s_prev, float* psi_out, float* scores_out, mi_stream_t stream);
/* one processor call after the first = select along (beam 0 of every utterance, last token of every hypothesis) + score with s_prev = psi_old[beam 0 row, last token],
   from one call (no index tensors in between; ctc_scorer.py:327-330 -> :58-207).  r_prev / psi are the state the next call passes as r_old / psi_old. */
int mi_ctc_prefix_advance(const float* x, int B, int T, int O, int blank, int W, const float* r_old, const long* last_old, long ld_last_old, int out_len_old,
                          const float* psi_old, const long* last, long ld_last, int out_len, float* r_prev, float* psi, float* scores, mi_stream_t stream);
/* the same step in ONE scan when the chains of every (hypothesis, token) may be kept between calls: r_all (T, 2, B*W, O) is written by this call and passed as r_prev
   (rp_full = 1, with psi_old) to the next; rp_full = 0: r_prev is mi_ctc_prefix_prepare's (T, 2, B*W) and psi_old is null (first token).  ctc_scorer.py:58-207. */
int mi_ctc_prefix_score_full(const float* x, int B, int T, int O, int blank, int W, const float* r_prev, int rp_full, const float* psi_old, const long* last,
                             long ld_last, int out_len, float* r_all, float* psi, float* scores, mi_stream_t stream);

/* ---- GPT-2 cross-attention decoder helpers (the rest of the decoder runs on the shared LN / GEMM / attention entry points).
 * replaces: GPT2Model embeddings (wte + wpe) and the fixed-position variant src/models/embeddings.py:33-86;
 *           the shifted, label-smoothed CE of src/models/decoders/multi_head_gpt2.py:138-158. */
int mi_embed_tokens(const long* ids, const float* wte, float scale, const float* pos, int pos_offset, int U, int d,
                    int M, int V, float* out, mi_stream_t stream);
/* acc[0] += sum of the valid rows' losses, acc[1] += their count; row_loss: B * (U - shift) floats of workspace (the rows' losses, NaN where the target is ignored),
 * summed by one block in a fixed order: no float atomics, the loss is bit-reproducible. */
int mi_ce_label_smoothing(const float* logits, long ld, const long* labels, int B, int U, int shift, int V, float eps,
                          float* acc, float* row_loss, mi_stream_t stream);

/* ---- training step: backward + optimizer building blocks.
 * replaces: torch autograd of the modules above under HF Trainer's bf16 autocast + torch.optim.AdamW + clip_grad_norm_
 *           (src/utilities/training_utils.py:93-115 GradAwareTrainer.training_step; recipes .../train_small_baseline.sh:43,53-58).
 * Activations bf16, residual stream / parameter gradients fp32; parameter gradients ACCUMULATE (+=). */
int mi_transpose_bf16(const void* in, long ld_in, void* out, long ld_out, int M, int N, int Mp, mi_stream_t stream);
int mi_transpose_many_bf16(const void* descs, int count, mi_stream_t stream);   /* descs: device array of {const void* in; void* out; int M, N, Mp, pad;} */
/* out[n] += sum_m x[m][n] (dtype 0 f32, 1 bf16).  workspace: mi_colsum_workspace_floats(M, N) floats — per-chunk column sums, added in chunk order by a second kernel.
 * (Round 4: every parameter-gradient reduction of the training step is ordered — per-block partial rows + a fixed-order sum, csrc/common.hpp rows_reduce_kernel — so the
 *  backward is bit-reproducible run to run; rounds 1-3 ended these sums in float atomics.) */
size_t mi_colsum_workspace_floats(int M, int N);
int mi_colsum(const void* x, long ld, int dtype, int M, int N, float* out, float* workspace, mi_stream_t stream);
/* out (N) bf16 = column sums of x (M, N) f32, rows added in order (M small: the per-group partials of d(posp), train.py `_attention_bwd`) */
int mi_colsum_cast_bf16(const float* x, long ld, int M, int N, void* out, mi_stream_t stream);
/* out_a (N) += column sums of a (M, N), out_b (N) += column sums of b (M, N): fp32, rows added in a fixed order (the pos_bias_u / pos_bias_v gradients from the attention
   backward's per-wave partials; tf wav2vec2_conformer :466-470) */
int mi_colsum2_acc_f32(const float* a, const float* b, long ld, int M, int N, float* out_a, float* out_b, mi_stream_t stream);
int mi_act_fwd_bf16(const void* pre, long ldp, void* out, long ldo, int M, int N, int kind, mi_stream_t stream);
int mi_act_bwd_bf16(const void* dy, long lddy, const void* pre, long ldp, void* dx, long lddx, int M, int N, int kind,
                    mi_stream_t stream);
/* the same with the FFN's activation dropout (tf wav2vec2_conformer :353 `intermediate_dropout`) applied in the pass: out = dropout(act(pre)),
 * dx = dropout(dy) * act'(pre); mask and rounding points of mi_dropout on the (M, N) matrix, i.e. bit-identical to the two-pass form. */
int mi_act_dropout_fwd_bf16(const void* pre, long ldp, void* out, long ldo, int M, int N, int kind, float p, unsigned seed, unsigned stream_id,
                            mi_stream_t stream);
int mi_act_dropout_bwd_bf16(const void* dy, long lddy, const void* pre, long ldp, void* dx, long lddx, int M, int N, int kind, float p,
                            unsigned seed, unsigned stream_id, mi_stream_t stream);
size_t mi_layernorm_bwd_workspace_floats(int d);
int mi_layernorm_bwd(const void* x, long ldx, int x_bf16, const float* gamma, float eps, const void* dy, long lddy, int dy_f32,
                     void* dx, long lddx, int dx_bf16, int accumulate, float* dgamma, float* dbeta, float* workspace, int M, int d,
                     mi_stream_t stream);
/* deferred form: the per-block (dgamma | dbeta) partial rows stay in `partial` (*nblk rows of 2 d floats; size as mi_layernorm_bwd_workspace_floats) and are reduced
   later, up to 24 entries per launch, by mi_ln_partial_reduce_many (dgamma[c] += sum, dbeta[c] += sum; fixed summation order, no atomics) */
typedef struct { const float* partial; int nblk, d; float* dgamma; float* dbeta; int kind; } mi_lnred_desc;
/* kind 0: a LayerNorm's rows as above.  kind = K (1..31): the tap-gradient partials a depthwise-conv backward left in its workspace (mi_csgu_bwd_bf16 /
 * mi_dwconv_residual_bwd_bf16 called with dw == NULL): nblk rows of d * 32 floats, d = channels; dgamma = the (d, K) tap gradient, dbeta = the (d) bias gradient or NULL;
 * dgamma[c * K + k] += sum_rows partial[row][c * 32 + k] (k < K), dbeta[c] += sum_rows partial[row][c * 32 + 31] */
int mi_layernorm_bwd_partial(const void* x, long ldx, int x_bf16, const float* gamma, float eps, const void* dy, long lddy, int dy_f32,
                             void* dx, long lddx, int dx_bf16, int accumulate, float* partial, int* nblk, int M, int d, mi_stream_t stream);
/* as mi_layernorm_bwd_partial, and in the same pass cast (M,d) bf16 = alpha * dropout(dx) of the finished rows — the bf16 operand of the linear backward that follows
 * (drop_p = 0: the scaled cast; mask of mi_dropout for (seed, stream_id), element m*d + c) */
int mi_layernorm_bwd_partial_cast(const void* x, long ldx, int x_bf16, const float* gamma, float eps, const void* dy, long lddy, int dy_f32,
                                  void* dx, long lddx, int dx_bf16, int accumulate, float* partial, int* nblk, void* cast, long ldcast, float alpha,
                                  float drop_p, unsigned seed, unsigned stream_id, int M, int d, mi_stream_t stream);
/* two LayerNorms of the SAME rows x with the same eps (the layer's two branch norms on x1, reference e_branchformer.py:273,292) in one pass:
 * dx (+)= dLN1/dx . dy + dLN2/dx . dy2 (linear in dy * gamma: x, its statistics and the old dx are read once); the two (dgamma | dbeta) partial sets go to
 * `partial` / `partial2` (*nblk rows each) for mi_ln_partial_reduce_many.  d <= 512.  cast may be NULL; otherwise as in mi_layernorm_bwd_partial_cast. */
int mi_layernorm_bwd_dual_partial(const void* x, long ldx, int x_bf16, float eps, const float* gamma, const void* dy, long lddy, int dy_f32,
                                  const float* gamma2, const void* dy2, long lddy2, int dy2_f32, void* dx, long lddx, int dx_bf16, int accumulate,
                                  float* partial, float* partial2, int* nblk, void* cast, long ldcast, float alpha, float drop_p, unsigned seed,
                                  unsigned stream_id, int M, int d, mi_stream_t stream);
int mi_ln_partial_reduce_many(const mi_lnred_desc* descs, int n, mi_stream_t stream);
int mi_axpy_f32(float* a, const float* b, long n, float alpha, mi_stream_t stream);
int mi_scale_f32(float* a, long n, float alpha, mi_stream_t stream);
/* a *= *alpha_dev (a device scalar; a 16-B aligned); a no-op launch when it is exactly 1: the autograd bridge's d(loss) factor (autograd_bridge.py) */
int mi_scale_dev_f32(float* a, long n, const float* alpha_dev, mi_stream_t stream);
int mi_add2_cast_bf16(const float* a, long lda, const float* b, long ldb, void* out, long ldo, int M, int N, float alpha,
                      mi_stream_t stream);
int mi_add_rowvec_bf16(const void* x, long ldx, const float* vec, void* out, long ldo, int M, int N, mi_stream_t stream);
/* out_u = bf16(x + u), out_v = bf16(x + v) from one read of x (q + pos_bias_u / q + pos_bias_v: e_branchformer's relative-position attention, tf wav2vec2_conformer :466-470) */
int mi_add_rowvec2_bf16(const void* x, long ldx, const float* u, const float* v, void* out_u, void* out_v, long ldo, int M, int N, mi_stream_t stream);
/* valid frame counts behind `layers` Conv2d sub-sampling layers (kernel, stride, pad on the time axis) for B utterances: inner[b] = min(count with padding, tmax) — the
 * encoder's masks —, outer[b] = count without padding — the CTC loss's input lengths (reference: e_branchformer.py _get_feat_extract_output_lengths; floor division) */
int mi_subsampled_lengths_i32(const int* lengths, int B, int kernel, int stride, int pad, int layers, int tmax, int* inner, int* outer, mi_stream_t stream);
int mi_mask_rows_f32(float* x, long ld, const int* lengths, int T, int M, int N, mi_stream_t stream);
/* in-model SpecAugment of the encoder input (tf wav2vec2_conformer _mask_hidden_states :1086-1130): time_mask (M) / feat_mask (B, N) bytes */
int mi_spec_mask_apply(float* x, long ld, const unsigned char* time_mask, const float* embed, const unsigned char* feat_mask, int T, int M, int N,
                       mi_stream_t stream);
int mi_spec_mask_bwd(float* dx, long ld, const unsigned char* time_mask, float* dembed, const unsigned char* feat_mask, int T, int M, int N,
                     float* workspace /* ceil(M / 128) * N floats when dembed is given */, mi_stream_t stream);
/* ---- layer mixing of the CTC fine-tuning head — replaces src/models/bestrq.py:239-245
 *      (`(torch.stack(hidden_states) * softmax(per_layer_weights)[:, None, None, None]).sum(0)`) and its autograd backward.
 *  mi_softmax_vec_f32:      s = softmax(w), n <= 1024.        mi_softmax_vec_bwd_f32:  dw += s * (g - <s, g>)  (g_l = <d mixed, hidden_l>).
 *  mi_axpy_dev_f32:         a = (overwrite ? 0 : a) + alpha[0] * b  with the coefficient read from DEVICE memory (no host round trip).
 *  mi_dot_f32:              out[0] += <a, b>  (caller zeroes out; bit-reproducible; workspace: 1024 floats). */
int mi_softmax_vec_f32(const float* w, int n, float* s, mi_stream_t stream);
int mi_softmax_vec_bwd_f32(const float* s, const float* g, int n, float* dw, mi_stream_t stream);
int mi_axpy_dev_f32(float* a, const float* b, long n, const float* alpha, int overwrite, mi_stream_t stream);
int mi_dot_f32(const float* a, const float* b, long n, float* out, float* workspace /* 1024 floats */, mi_stream_t stream);
int mi_sumsq_f32(const float* x, long n, float* sumsq, float* workspace /* 1024 floats */, mi_stream_t stream);
/* norm_coef_skip (3 floats): [sqrt(sumsq), clip coefficient min(1, max_norm / (norm + 1e-6)), skip flag].  skip = 1 (and coef 0) when the norm is not
 * finite or exceeds skip_above > 0 — GradAwareTrainer.training_step drops such a step (src/utilities/training_utils.py:81,101-115). mi_adamw_step
 * given this array leaves parameters and moments untouched when skip is set. */
int mi_clip_coef(const float* sumsq, float max_norm, float skip_above, float* norm_coef_skip, mi_stream_t stream);
int mi_adamw_step(float* p, const float* g, float* m, float* v, const unsigned char* decay, long n, float lr, float beta1,
                  float beta2, float eps, float weight_decay, int step, const float* norm_coef, void* mirror_bf16,
                  mi_stream_t stream);
/* weight-gradient GEMM dW (n_store, K) fp32 += dY[:, :N]^T · X (contraction over the rows of both operands, split over M) */
size_t mi_gemm_tn_workspace_bytes(int M, int N, int K);
int mi_gemm_tn_bf16(const void* dY, long ldy, const void* X, long ldx, float* dW, long ldo, float* db /* optional bias gradient */, int M, int N,
                    int K, int n_store, void* workspace, size_t workspace_bytes, int variant /* 0 = product tile (128 x 128); 1 = 128 x 64 for A/B */, mi_stream_t stream);
/* Conv2d weight gradient without an im2col buffer: dW (n_store, KH*KW*Cin) fp32 += dY[:, :N]^T · im2col(x); x (B,Tin,Fin,Cin) bf16 channels-last, dY rows (b,to,fo),
 * k = (kh*KW + kw)*Cin + c, square stride, leading pads (pad_t, pad_f); Cin % 128 == 0 else MI_ERR_UNSUPPORTED; workspace: mi_gemm_tn_workspace_bytes(B*Tout*Fout, N, KH*KW*Cin).
 * replaces: the weight gradient autograd derives for the second Conv2d of extractors.py:82-89. */
int mi_conv2d_wgrad_cl_bf16(const void* dY, long ldy, const void* x, float* dW, long ldo, float* db, int B, int Tin, int Fin, int Cin, int KH, int KW,
                            int stride, int pad_t, int pad_f, int Tout, int Fout, int N, int n_store, void* workspace, size_t workspace_bytes, mi_stream_t stream);
/* grouped form: the weight-gradient GEMMs of one encoder layer (n <= 48 problems, host arrays of length n) as ONE launch — together their 128 x 128 output tiles fill the
 * chip without splitting M, so every block adds its tile into dW in place: no slabs, no reduce pass, no workspace.  Use it for >= ~256 tiles in total. */
int mi_gemm_tn_group_bf16(int n, const void* const* dY, const long* ldy, const void* const* X, const long* ldx, float* const* dW, const long* ldo,
                          float* const* db, const int* M, const int* N, const int* K, const int* n_store, int tile_k, mi_stream_t stream);
/* the same with overwrite != 0: every dW_i / db_i is written (= instead of +=) — for targets known to hold zeros (a training step's first backward after the gradients
 * were cleared; each target the output of exactly one problem): the kernel's epilogue then has no dependent read of its output tile */
int mi_gemm_tn_group_ow_bf16(int n, const void* const* dY, const long* ldy, const void* const* X, const long* ldx, float* const* dW, const long* ldo,
                             float* const* db, const int* M, const int* N, const int* K, const int* n_store, int tile_k, int overwrite, mi_stream_t stream);
/* (tile_k: k extent of the 256-row output tiles: 128, 256, or 0 = 256 when the problems then still have >= 200 tiles between them, else 128) */
/* strided batched GEMM C[z1,z2] = alpha * A[z1,z2] · B[z1,z2]^T (+ C): the per-(utterance, head) products of attention backward */
int mi_bgemm_bf16(const void* A, long a_z1, long a_z2, long a_m, long a_k, const void* B, long b_z1, long b_z2, long b_n, long b_k,
                  void* C, long c_z1, long c_z2, long c_m, int out_f32, int accumulate, float alpha, int Z1, int Z2, int M, int N,
                  int K, mi_stream_t stream);
/* mi_bgemm_bf16 for an A operand banded along K: K = band_cg * band_T rows, row (u, i) of A non-zero only in columns [band_a - i, band_a - i + band_T) — the
 * un-shifted relative-position gradient dBD of mi_attention_qkv_bwd_probs in the d(positions) product.  All-zero k tiles are skipped (same result); band_T = 0: no band. */
int mi_bgemm_band_bf16(const void* A, long a_z1, long a_z2, long a_m, long a_k, const void* B, long b_z1, long b_z2, long b_n, long b_k,
                       void* C, long c_z1, long c_z2, long c_m, int out_f32, int accumulate, float alpha, int Z1, int Z2, int M, int N, int K,
                       int band_T, int band_a, int band_cg, mi_stream_t stream);
/* ... and with m_valid (Z2 ints on the device, or NULL): rows m >= m_valid[z2] of A are zero for batch entry z2 (keys beyond an utterance's length in the dV = P^T dctx and
 * dK = dS^T q products): those M tiles of C are stored as zeros (left alone when accumulating) without being read or multiplied. */
int mi_bgemm_sparse_bf16(const void* A, long a_z1, long a_z2, long a_m, long a_k, const void* B, long b_z1, long b_z2, long b_n, long b_k,
                         void* C, long c_z1, long c_z2, long c_m, int out_f32, int accumulate, float alpha, int Z1, int Z2, int M, int N, int K,
                         int band_T, int band_a, int band_cg, const int* m_valid, mi_stream_t stream);
/* softmax stage of attention (e_branchformer.py:100-135, tf wav2vec2_conformer:528-565 relative shift), head-major (H,B,Tq,Tk) */
int mi_attn_softmax_fwd(const float* ac, const float* bd, const int* lengths, void* prob, void* prob_drop, int H, int B, int Tq, int Tk,
                        long ld_s, long ld_p, float scale, int causal, float drop_p, unsigned seed, unsigned stream_id, mi_stream_t stream);
int mi_attn_softmax_bwd(const void* prob, const float* dp, void* ds, void* dbd, int H, int B, int Tq, int Tk, long ld_s, long ld_p,
                        float scale, float drop_p, unsigned seed, unsigned stream_id, mi_stream_t stream);
/* dropout with counter-based masks (torch.nn.Dropout sites of e_branchformer.py:132,203,288,301,451, tf wav2vec2_conformer :353,356,674,
 * GPT-2 embd/attn/resid): keep(idx) is a pure function of (seed, stream_id, logical element index) — see csrc/dropout.hip */
int mi_dropout(const void* x, long ldx, int in_dtype, void* out, long ldo, int out_dtype, int M, int N, float alpha, float p, unsigned seed,
               unsigned stream_id, mi_stream_t stream);
int mi_dropout_add_f32(float* y, long ldy, const float* resid, long ldr, const float* t, long ldt, int M, int N, float alpha, float p,
                       unsigned seed, unsigned stream_id, mi_stream_t stream);
/* depthwise-conv / conv front-end gradients (e_branchformer.py:184-204,296-304; extractors.py:71-113) */
/* the two depthwise-conv backward entries below: dw == NULL leaves the per-utterance tap-gradient partials in `workspace` un-reduced (rows = B, or B * ceil(T / 64) for the
 * dilated form) for a later mi_ln_partial_reduce_many (desc kind = K) — several layers' reductions in one launch */
int mi_csgu_bwd_bf16(const void* u, long ldu, const float* stats, const float* gamma, const float* beta, const float* w,
                     const float* bias, const void* ds, long ldds, void* dr, long lddr, void* dgn, long lddgn, float* dw,
                     float* db, int B, int T, int C, int K, int pad_left, int dilation /* 1, or the causal form's (K-1)/2 */,
                     float* workspace /* B*C*32 floats or NULL */, mi_stream_t stream);
int mi_dwconv_residual_bwd_bf16(const void* m, long ldm, const float* w, const void* dy, long lddy, void* dm, long lddm,
                                float* dw, float* db, int B, int T, int C, int K, int pad_left, int dilation, float* workspace, mi_stream_t stream);
int mi_im2col_cl_bf16(const void* in, void* col, int B, int Tin, int Fin, int Cin, int KH, int KW, int stride, int pad_t,
                      int pad_f, int Tout, int Fout, mi_stream_t stream);
int mi_conv2d_first_bwd(const float* x, const float* w, const float* bias, const void* dcol, float* dw, float* db, int B, int T,
                        int F, int C, int K, int stride, int pad_t, int pad_f, int T1, int F1, int K2, int stride2, int pad2_t,
                        int pad2_f, int T2, int F2, float* workspace /* mi_conv2d_first_bwd_workspace_floats: one partial row per block */, mi_stream_t stream);
size_t mi_conv2d_first_bwd_workspace_floats(int B, int C, int T1, int F1);
/* The second Conv2d's INPUT gradient (3x3, stride 2; what autograd derives for extractors.py:82-89's second layer) as four stride-1 implicit-GEMM convolutions, one per
 * parity class of (t1 + pad_t, f1 + pad_f), instead of one GEMM into the gradient of the im2col operand (9 C1 columns per output position of conv2) and a col2im gather:
 *   mi_conv2d_s2k3_dgrad_elems      bf16 elements of the four phase buffers, back to back; 0 = geometry not supported (keep mi_gemm_bf16 + mi_conv2d_first_bwd)
 *   mi_conv2d_s2k3_dgrad_pack_bf16  wT (9*C1 rows (kh,kw,c), C2 columns, row stride ldwt) -> the four phase weight matrices (9*C1*C2 elements), once per weight update
 *   mi_conv2d_s2k3_dgrad_bf16       dY2 (B,T2,F2,C2) contiguous -> phases
 *   mi_conv2d_first_bwd_phases      mi_conv2d_first_bwd reading the phase buffers (one 16-B load per position and 8 channels instead of up to four) */
size_t mi_conv2d_s2k3_dgrad_elems(int B, int T1, int F1, int C1, int T2, int F2, int pad_t, int pad_f);
int mi_conv2d_s2k3_dgrad_pack_bf16(const void* wT, long ldwt, void* packed, int C1, int C2, mi_stream_t stream);
int mi_conv2d_s2k3_dgrad_bf16(const void* dY2, const void* packed, void* phases, int B, int T1, int F1, int C1, int T2, int F2, int C2, int pad_t, int pad_f,
                              mi_stream_t stream);
int mi_conv2d_first_bwd_phases(const float* x, const float* w, const float* bias, const void* phases, float* dw, float* db, int B, int T, int F, int C, int K,
                               int stride, int pad_t, int pad_f, int T1, int F1, int pad2_t, int pad2_f, int T2, int F2,
                               float* workspace /* mi_conv2d_first_bwd_workspace_floats */, mi_stream_t stream);
/* backward pieces of the context-aware front ends (extractors.py:23-65), un-fused: im2col / col2im with separate strides, the backward of mi_gated_act_bf16
 * (dz = dout GELU'(y) sigmoid(g), dg = sum over the shared rows of dout GELU'(y) z sigmoid(g)(1 - sigmoid(g)), y = z sigmoid(g)), and the weight / bias gradient of a
 * Conv2d(1 -> C) of geometry (3,3) or (12,3) from the gradient of its raw output. */
int mi_im2col_cl_geo_bf16(const void* in, void* col, int B, int Tin, int Fin, int Cin, int KH, int KW, int stride_t, int stride_f, int pad_t,
                          int pad_f, int Tout, int Fout, mi_stream_t stream);
int mi_col2im_cl_bf16(const void* dcol, void* din, int B, int Tin, int Fin, int Cin, int KH, int KW, int stride_t, int stride_f, int pad_t, int pad_f,
                      int Tout, int Fout, int accumulate, mi_stream_t stream);
int mi_gated_act_bwd_bf16(const void* dout, long lddo, const void* z, long ldz, const void* g, long ldg, void* dz, long lddz, void* dg, long lddg,
                          int B, int T, int Fq, int C, int share, mi_stream_t stream);
int mi_conv2d_first_wgrad(const float* x, const void* dy, float* dw, float* db, int B, int T, int F, int C, int KH, int KW, int stride_t, int stride_f,
                          int pad_t, int pad_f, int T1, int F1, float* workspace /* mi_conv2d_first_wgrad_workspace_floats */, mi_stream_t stream);
size_t mi_conv2d_first_wgrad_workspace_floats(int B, int C, int KH, int KW, int T1, int F1);
/* loss gradients: F.ctc_loss backward composed with log_softmax (e_branchformer.py:472-488); label-smoothed CE of the decoder
 * heads (multi_head_gpt2.py:138-158); embedding scatter (embeddings.py:33-62) */
size_t mi_ctc_bwd_workspace_bytes(int B, int T, int U);
int mi_ctc_loss_bwd(const void* logits, long ld_b, long ld_t, int dtype, const float* lse, int T, const long* labels, int U,
                    const int* in_len, int blank, int B, int reduction, const float* nll, float gscale, void* workspace,
                    size_t workspace_bytes, void* dlogits, long ldo, mi_stream_t stream);
/* loss AND gradient from one pair of recursions (the training step): as mi_ctc_loss_bwd, but the per-utterance negative log-likelihood comes OUT of the call (its own alpha
 * recursion: nll_out (B), tgt_len_out (B), loss_out (1, nullable) = the reduced loss of mi_ctc_loss_fwd with the same reduction / zero_infinity semantics) instead of
 * going in — no forward loss kernel.  MI_ERR_UNSUPPORTED for targets of more than 63 labels (the caller runs mi_ctc_loss_fwd + mi_ctc_loss_bwd). */
int mi_ctc_loss_bwd_nll(const void* logits, long ld_b, long ld_t, int dtype, const float* lse, int T, const long* labels, int U,
                        const int* in_len, int blank, int B, int reduction, int zero_infinity, float gscale, void* workspace,
                        size_t workspace_bytes, void* dlogits, long ldo, float* nll_out, int* tgt_len_out, float* loss_out, mi_stream_t stream);
/* the reduction of mi_ctc_loss_fwd alone */
int mi_ctc_reduce(const float* nll, const int* tgt_len, int B, int reduction, int zero_infinity, float* loss, mi_stream_t stream);
int mi_ce_label_smoothing_bwd(const float* logits, long ld, const long* labels, int B, int U, int shift, int V, float eps,
                              float weight, const float* acc, void* dlogits, long ldo, mi_stream_t stream);
/* ---- mixing fine-tuning of the DeCRED decoder (csrc/mix_loss.hip; multi_head_gpt2_mixing.py:111-131, modes scalar / linear): the mean unsmoothed cross-entropy of
 * z[r, v] = sum_h mix[h, v] L_h[r, v] against labels shifted by one (ignore < 0), and d mix, from the H per-head fp32 logit matrices (head h, row r, column v at
 * logits[h * head_stride + r * ld + v]; columns [V, ld) are never read).  mix: (H, V) when mix_per_col, else (H); 1 <= H <= 8.  Neither z nor its gradient is
 * materialised.  fwd: lse (M), row_loss (M) workspace, acc[0] = sum of the valid rows' losses, acc[1] = their count.  bwd: d mix of acc[0] / acc[1] from fwd's lse / acc;
 * rows reduced in fixed chunks, partials added in chunk order — no float atomics, bit-reproducible. */
int mi_mix_ce_fwd(const float* logits, long ld, long head_stride, int H, const float* mix, int mix_per_col, const long* labels, int B, int U, int V,
                  float* lse, float* row_loss, float* acc, mi_stream_t stream);
size_t mi_mix_ce_bwd_workspace_floats(int M, int H, int V);
int mi_mix_ce_bwd(const float* logits, long ld, long head_stride, int H, const float* mix, int mix_per_col, const long* labels, int B, int U, int V,
                  const float* lse, const float* acc, float* workspace, size_t workspace_floats, float* dmix, mi_stream_t stream);
/* as gathers (a block per 16 vocabulary entries / per position adds its rows in order: no atomics).  heavy_id: an entry expected on a large share of the rows (the padding
 * token of the shifted decoder input) is summed as a masked column sum instead, or -1; workspace: mi_embed_tokens_bwd_workspace_bytes(M, d, V) bytes; d <= 1024 */
size_t mi_embed_tokens_bwd_workspace_bytes(int M, int d, int V);
int mi_embed_tokens_bwd(const long* ids, const float* dx, float scale, int pos_offset, int U, int d, int M, int V, float* dwte,
                        float* dwpe, int heavy_id, void* workspace, mi_stream_t stream);

/* ---- feature-level SpecAugment on the device (src/augmentations/spec_aug.py:40-137: bicubic time warp + frequency / time masks) */
int mi_specaug_f32(const float* x, float* out, int B, int T, int F, const int* params, int nf, int nt, float pad_value, mi_stream_t stream);

/* Speed perturbation = polyphase sinc resampling of a (B, N) fp32 waveform batch by orig/nw (both divided by their gcd), the arithmetic of
 * torchaudio.transforms.SpeedPerturbation which the reference's training pre-processing names first (configs/default_data_preprocessing2d.json:3-19;
 * torchaudio functional.py `speed` / `_apply_sinc_resample_kernel`).  kernel: (nw, 2*width + orig) fp32 table built by the host;
 * N_out must equal ceil(nw * N / orig); lengths / out_lengths (B) int32 or NULL (out = ceil(len * nw / orig)). */
int mi_speed_resample_f32(const float* wave, long ld, const int* lengths, int B, int N, int orig, int nw, const float* kernel, int width,
                          float* out, long ld_out, int N_out, int* out_lengths, mi_stream_t stream);

/* ---- BEST-RQ pre-training (src/models/bestrq.py:66-97): random-projection quantizer targets, noise masking of the encoder input */
int mi_rpq_targets(const float* x, long ldx, const float* P, const float* CB, long* targets, int M, int in_dim, int cd, int C, int books,
                   mi_stream_t stream);
int mi_mask_noise_f32(float* x, long ld, const unsigned char* time_mask, int M, int N, float std, unsigned seed, unsigned stream_id,
                      mi_stream_t stream);

/* ---- GPT-2 decoder token step as one call (KV cache, cross-attention over cached encoder K/V) + beam re-ordering of the caches.
 * replaces: GPT2LMMultiHeadModel.forward with past_key_values (multi_head_gpt2.py:80-170; tf gpt2 :262-310) and `_reorder_cache`.
 * cross_kv == NULL: the block without cross-attention (ln_1, causal self-attention over the cache, ln_2, MLP) — transformers' GPT2LMHeadModel with a cache, the
 * external language model of shallow fusion (src/decoding/shallow_fussion.py re-runs it over the whole prefix per token).  The weight table keeps 5 + 18 L entries,
 * the six cross entries of a layer (lnc_g/b, wq, bq, wco, bco) are not read and may be NULL; T_enc and enc_len are ignored.  Every step form applies: the fused form
 * then takes two launches per layer instead of three. */
typedef struct {
    int d, H, L, V;
    float eps;
    int step_form;      /* token step with one new token per row and <= 8 rows: 0 = the fused form (three launches per layer, csrc/decoder_fused.hip) where it applies
                           (head size 64, d <= 512), 1 = always one launch per op (the cross-check; what every other shape runs); 2 = the streaming form
                           (csrc/linear_rows.hip) for one new token per row and <= 64 rows, one launch per op elsewhere */
    int act;            /* MLP activation: 0 = gelu_new (GPT-2), 1 = erf-GELU (Whisper); the fused and GEMV forms are gelu_new only: act 1 runs form 1 or 2 */
} mi_gpt2_config;
size_t mi_gpt2_step_workspace_bytes(const mi_gpt2_config* cfg, int B, int U);
int mi_gpt2_step(const mi_gpt2_config* cfg, const void* const* weights, const long* ids_new, int B, int U, int past, int Lmax,
                 void* const* kcache, void* const* vcache, const void* const* cross_kv, int T_enc, const int* enc_len, float emb_scale,
                 void* workspace, size_t workspace_bytes, float* logits, long ld_logits, mi_stream_t stream);
/* mi_gpt2_step with a nullable fp32 head_bias (V) added to the logits (0 / -inf: transformers' SuppressTokens processors).  The Whisper decoder
 * (transformers WhisperDecoder.forward with a cache) is this step with act = 1 and [Wq; Wk; Wv] packed, the K bias zero. */
int mi_decoder_step(const mi_gpt2_config* cfg, const void* const* weights, const long* ids_new, int B, int U, int past, int Lmax,
                    void* const* kcache, void* const* vcache, const void* const* cross_kv, int T_enc, const int* enc_len, float emb_scale,
                    const float* head_bias, void* workspace, size_t workspace_bytes, float* logits, long ld_logits, mi_stream_t stream);
/* mi_decoder_step for beam search whose hypotheses share their utterance's encoder frames: the B rows are B / beams utterances x `beams` hypotheses (row = utterance *
 * beams + k), cross_kv holds L pointers to (B / beams * T_enc, 2d) and enc_len is (B / beams) — the cross K/V of an utterance exist once, not once per hypothesis.
 * beams > 1 needs U == 1, B % beams == 0 and cross_kv; the step then runs one launch per op whatever the row count, its cross-attention as B / beams batches of
 * `beams` queries (the teacher-forced forward's call).  beams == 1 is mi_decoder_step.  KV caches, logits and workspace are per row, as there. */
int mi_decoder_step_beams(const mi_gpt2_config* cfg, const void* const* weights, const long* ids_new, int B, int beams, int U, int past, int Lmax,
                          void* const* kcache, void* const* vcache, const void* const* cross_kv, int T_enc, const int* enc_len, float emb_scale,
                          const float* head_bias, void* workspace, size_t workspace_bytes, float* logits, long ld_logits, mi_stream_t stream);
/* mi_decoder_step_beams with a multi-tap head: logits = sum_h A_h hidden[taps[h]] (+ head_bias) as one head GEMM with K = n_taps * d.  Serves the reference's
 * GPT2LMMultiHeadModelMixing (multi_head_gpt2_mixing.py:101-121, all three mixing modes) and `average_logits` of GPT2LMMultiHeadModel (multi_head_gpt2.py:129-136), whose
 * mixing parameters the engine folds into the head at load time.  weights[4] is the folded head (V, n_taps * d) bf16; taps (n_taps ints in HOST memory, 1 <= n_taps <= 8):
 * 0 = the embedding output, l = the residual stream after l blocks (no LayerNorm), L = ln_f of the last block's output — transformers' `hidden_states[l]`.  Column block h
 * of the head's input row is the bf16-rounded stream of tap h at the last new position.  Workspace: mi_decoder_step_taps_workspace_bytes.  At <= 8 rows the step runs
 * its GEMV form (while n_taps * d <= 2048, the GEMV kernel's K; beyond it one launch per op) whatever step_form says (the fused form keeps a layer's stream inside its launches); beams as in mi_decoder_step_beams. */
size_t mi_decoder_step_taps_workspace_bytes(const mi_gpt2_config* cfg, int B, int U, int n_taps);
int mi_decoder_step_taps(const mi_gpt2_config* cfg, const void* const* weights, const long* ids_new, int B, int beams, int U, int past, int Lmax,
                         void* const* kcache, void* const* vcache, const void* const* cross_kv, int T_enc, const int* enc_len, float emb_scale,
                         const float* head_bias, const int* taps, int n_taps, void* workspace, size_t workspace_bytes, float* logits, long ld_logits, mi_stream_t stream);
/* Rows-streaming linear (csrc/linear_rows.hip): y = act(x W^T + b) for 1 <= M <= 64 rows, any N, K % 8 == 0; x (M, K) and W (N, K) bf16, 16-B aligned, ldx % 8 == ldw % 8 == 0.
 * act 0 none / 1 erf-GELU / 2 gelu_new.  Exactly one of out32 / out16: out32 (M, ldo32) fp32 = y, or out32 += y when accumulate (the in-place residual add); out16 (M, ldo16)
 * bf16, and with kcache != NULL (N == 3 dkv, M % U == 0) columns [dkv, 2 dkv) / [2 dkv, 3 dkv) of row m = b U + u also go to kcache / vcache (.., Lmax, dkv) at row
 * past + u of sequence b.  workspace: mi_linear_rows_workspace_bytes(M, N, K) bytes (0 when the launch is not split over K).  No float atomics: bit-reproducible, and a
 * row's result does not depend on the other rows. */
size_t mi_linear_rows_workspace_bytes(int M, int N, int K);
int mi_linear_rows(const void* x, long ldx, const void* W, long ldw, const float* bias, int act, float* out32, long ldo32, int accumulate, void* out16, long ldo16,
                   void* kcache, void* vcache, int U, int past, int Lmax, int dkv, int M, int N, int K, void* workspace, size_t workspace_bytes, mi_stream_t stream);
/* One step of greedy decoding between two token steps (transformers GenerationMixin greedy loop): tok = done[b] ? pad : best[b]; ids[b, col] = new_tok[b] = tok;
 * done[b] |= tok == eos; done_host (nullable; pinned, device-mapped memory) receives the flags. */
int mi_greedy_advance(const int* best, long* ids, long ld_ids, int col, long eos, long pad, int* done, long* new_tok, int* done_host, int B, mi_stream_t stream);
/* Whisper's timestamp rules + argmax for one greedy step (csrc/whisper_rules.hip): best[b] = argmax(WhisperTimeStampLogitsProcessor(ids[b, :cur_len], logits[b])) of
 * transformers (generation/logits_process.py), mi_row_argmax's rules (lowest index among equal maxima; a row with nothing finite left gives 0).  logits (B, ld) fp32, the
 * first V columns of a row (suppression already applied as -inf); ids (B, ld_ids) int64, of which [begin_index, cur_len) are the sampled tokens; timestamp_begin =
 * no_timestamps_token_id + 1; max_initial_timestamp_index -1 = None; detect_from_logprob: the processor's _detect_timestamp_from_logprob.  One read of the row, no
 * atomics: bit-reproducible. */
int mi_whisper_timestamp_argmax(const float* logits, long ld, int V, const long* ids, long ld_ids, int begin_index, int cur_len, int no_timestamps_token_id,
                                int eos_token_id, int max_initial_timestamp_index, int detect_from_logprob, int* best, int B, mi_stream_t stream);
/* The scores of one beam-search step under Whisper's rules (csrc/whisper_rules.hip), for mi_beam_step / mi_beam_step_wide, which form logit - lse themselves.  transformers'
 * `_beam_search` applies log_softmax to the RAW logits and the processors to the log-probabilities, so per row (one block): lse[r] = log-sum-exp of the raw row — equal to
 * mi_row_lse's bit for bit — and, in place, -inf in every column that `suppress` ((V) fp32 of 0 / -inf, nullable: SuppressTokens[AtBegin]LogitsProcessor) or
 * WhisperTimeStampLogitsProcessor masks for the row's history; every other value is not written.  logits (rows, ld) fp32 WITHOUT a head bias; ids, begin_index, cur_len and
 * the timestamp parameters as in mi_whisper_timestamp_argmax; no_timestamps_token_id < 0: no timestamp rules (ids may be NULL).  No atomics: bit-reproducible. */
int mi_whisper_beam_scores(float* logits, long ld, int V, const long* ids, long ld_ids, int begin_index, int cur_len, const float* suppress,
                           int no_timestamps_token_id, int eos_token_id, int max_initial_timestamp_index, int detect_from_logprob, float* lse, int rows,
                           mi_stream_t stream);
int mi_kv_cache_reorder(const void* const* src_k, const void* const* src_v, void* const* dst_k, void* const* dst_v, const long* beam_idx,
                        int L, int BW, int rows, int Lmax, int d, mi_stream_t stream);

/* One beam-search step of joint CTC / attention decoding on the device (csrc/beam_step.hip): what the reference gets per token from transformers' beam loop on the host
   (src/models/ctc_encoder_plus_autoregressive_decoder.py:360-482; processors src/decoding/ctc_scorer.py:259-365; the loop itself: transformers/generation/utils.py
   `_beam_search` of the installed 5.x, the rules tests/golden/gen_*.npz pin from the reference's own generate()).
   cand = ((1 - w)(logits - lse, pad -> logzero when mask_pad) + w ctc) + beam_scores  [ctc null: no mix];  top 2W per utterance, best first, ties by lower index;
   a candidate stops when its token is EOS or cur_len + 1 >= max_length; the first W that did not stop become the next beams: ids (B*W, Lmax) re-ordered in place + the
   new token at column cur_len, new_tok / beam_idx / beam_scores (B*W) written; stopped candidates among the first W ranks enter the kept hypotheses with
   score / denom (denom = (cur_len + 1 - prompt) ** length_penalty as fp32, computed by the caller): fin_score / fin_len (B, W), fin_tok (B, W, Lmax), nfin (B) hold the
   best W, best first.  done[b] is set when W are kept and beam_scores[b, 0] / heur_denom cannot beat the worst of them (heur_denom = (hypothetical length) **
   length_penalty: cur_len, or max_length - prompt for early_stopping 2 = "never" with a positive penalty), when early_stopping is 1 (True) and W are kept, or at
   max_length; a done utterance only emits pad tokens from beam b*W.
   top_s / top_i (B, 2W) optional; done_out (B) optional: the flags after the step, written for the host (pinned, device-mapped memory).  W <= 16, W * V < 2^24. */
int mi_beam_step(const float* logits, long ldl, const float* lse, const float* ctc, float w_att, float w_ctc, int mask_pad, int pad, int eos, int B, int W, int V,
                 int cur_len, int max_length, int Lmax, float denom, float heur_denom, int early_stopping, long* ids, float* beam_scores, long* new_tok, long* beam_idx,
                 int* done, int* nfin, float* fin_score, int* fin_len, long* fin_tok, float* top_s, int* top_i, int* done_out, mi_stream_t stream);
/* mi_beam_step with the shallow-fusion term of an external language model (src/decoding/shallow_fussion.py:41-53, appended behind the CTC processor,
   ctc_encoder_plus_autoregressive_decoder.py:398-403): lm_logits (B*W, ld_lm) fp32 logits of the LM for the same prefixes, lm_lse (B*W) their row log-sum-exp, w_lm the weight.
   One rounding per operation, in the reference's order:
       s = logit - lse;  pad -> logzero when mask_pad;  [ctc: s = w_att s + w_ctc ctc];  l = lm_logit - lm_lse;  m = w_lm l;  s = s + m;  cand = s + beam_score
   lm_logits == NULL: no term (lm_lse, w_lm ignored) — exactly mi_beam_step, which is this call with the LM off.  Same limits. */
int mi_beam_step_lm(const float* logits, long ldl, const float* lse, const float* ctc, float w_att, float w_ctc, int mask_pad, int pad, int eos, int B, int W, int V,
                    int cur_len, int max_length, int Lmax, float denom, float heur_denom, int early_stopping, long* ids, float* beam_scores, long* new_tok, long* beam_idx,
                    int* done, int* nfin, float* fin_score, int* fin_len, long* fin_tok, float* top_s, int* top_i, int* done_out,
                    const float* lm_logits, long ld_lm, const float* lm_lse, float w_lm, mi_stream_t stream);
/* mi_beam_step_lm for wide beams and long outputs (csrc/beam_step_wide.hip): the same arguments, rules, arithmetic and outputs, W <= 64, W * V < 2^24, no limit on
   max_length / Lmax (ids and kept hypotheses move through LDS in column chunks instead of living there).  Two launches: every (utterance, beam) row selects its
   min(2W, V) best candidates (exact radix select on order-preserving keys), one block per utterance merges them, walks the top 2W and moves the state.  A candidate
   value of -0 is reported as +0 in top_s.  The table between the two launches is allocated by the library per (device, stream) at the first call and when a later call
   needs more (hipMalloc: do not make the first call inside a stream capture); MI_ERR_LAUNCH when that fails. */
int mi_beam_step_wide(const float* logits, long ldl, const float* lse, const float* ctc, float w_att, float w_ctc, int mask_pad, int pad, int eos, int B, int W, int V,
                      int cur_len, int max_length, int Lmax, float denom, float heur_denom, int early_stopping, long* ids, float* beam_scores, long* new_tok, long* beam_idx,
                      int* done, int* nfin, float* fin_score, int* fin_len, long* fin_tok, float* top_s, int* top_i, int* done_out,
                      const float* lm_logits, long ld_lm, const float* lm_lse, float w_lm, mi_stream_t stream);

/* ---- Whisper-style front end + glue (BASELINE config 4).  replaces: transformers WhisperFeatureExtractor numpy path
 *      (selected by configs/default_data_preprocessing_whisper.json:20-29) and the conv/position prologue of WhisperEncoder. */
/* scratch: B * frames * nmel + B floats (frames = n_samples / 160): the log-mel before the clamp, then the per-clip maxima. */
int mi_whisper_logmel(const float* wave, long ldw, const int* num_samples, int n_samples, const double* window,
                      const double* twiddle, const double* mel_t, int nmel, int B, float* scratch,
                      float* out_features, void* out_cl_bf16, mi_stream_t stream);
int mi_transpose_cast_bct_btc(const float* x, void* out_bf16, int B, int C, int T, mi_stream_t stream);
int mi_add_positions(const void* a_bf16, const float* pos, float* x, int M, int T, int d, mi_stream_t stream);

/* ---- whole encoder + CTC head: Wav2Vec2EBranchformerForCTC.forward (e_branchformer.py:422-496), eval mode. */
typedef struct {
    int B, T, F;                 /* padded log-mel input (B,T,F) fp32 */
    int d, H, I, L, V;           /* hidden, heads, intermediate, layers, vocab (blank excluded) */
    int C1, C2, K, stride, pad;  /* Conv2d sub-sampling: 1->C1->C2, KxK, stride, padding */
    int is_causal;
    int pos_type;                /* 0 none, 1 relative, 2 rotary */
    int csgu_kernel, merge_kernel, csgu_act, use_macaron;
    float ln_eps;                /* feature-projection / encoder LayerNorm eps (layer LNs use 1e-5) */
    int logits_f32;              /* 1: fp32 logits, 0: bf16 logits */
    int logits_ld;               /* row stride of the logits buffer in elements (0 = V+1); a multiple of 8 keeps the stores 16-B wide */
    int branch_overlap;          /* experimental, default 0: run each layer's local (cgMLP) branch on a library-owned side stream beside the
                                    attention branch (one forward in flight at a time); see DESIGN.md 'Concurrent kernels' before enabling */
    /* CTC fine-tuning head of a BEST-RQ encoder — BestRQEBranchformerForCTC.forward, src/models/bestrq.py:239-274 */
    int extra_layers;            /* 0 | 1: `finetune_with_additional_layer` — one more layer (weight-table layer index L) between the encoder's
                                    final LayerNorm and the head: padded frames zeroed, same key mask and position table, no LayerNorm after it */
    int layer_mixing;            /* `finetune_with_layer_mixing`: softmax(per_layer_weights, global slot 14)-weighted sum of the L+1 hidden states
                                    (the input of every layer + the final LayerNorm's output) replaces the last hidden state */
    int csgu_linear;             /* `csgu_use_linear_after_conv` (e_branchformer.py:172-175,198-199): a Linear (layer slots CSGU_LIN_W bf16 (I/2, I/2) / CSGU_LIN_B) between
                                    the CSGU conv and its activation */
    int context_mode;            /* `context_awareness_type` (extractors.py:57-65) of a non-causal encoder: 0 plain conv (None and every unknown string, as the reference's dict
                                    lookup resolves them), 1 "gated", 2 "gated_shared".  Global slots: GATE1_W (15) f32 (C1, KH*KW), GATE1_B (16), and for mode 2 GATE2_W (17) bf16
                                    (C2, 12*3*C1), GATE2_B (18).  Mode 1: CONV2_W / CONV2_B hold conv AND gate, (2*C2, 9*C1) / (2*C2), interleaved in blocks of `gate_blk` channels */
    int gate_blk;                /* mode 1: 32 (the fused epilogue's packing; needs C2 % 32 == 0) or C2 (conv rows, then gate rows) */
    int ln_fold;                 /* 1: the LayerNorms in front of the FFN-in / QKV / cgMLP-in GEMMs are folded into those GEMMs (LN(x) W^T = rstd (x W'^T) - rstd mu s + c, W' = W diag(gamma)):
                                    the N = d GEMMs that produce the residual stream also emit its bf16 copy and per-row partial statistics, the consumers take those instead of
                                    a LayerNorm kernel's output — one LayerNorm launch per layer instead of three.  Needs the layer slots *_WF / *_SF / *_CF (engine.py LS), relative
                                    or no positions, macaron FFNs, d in {256, 512}, I % 256 == 0, no fine-tuning head.  0: LayerNorm kernels + plain GEMMs. */
    int wide_tiles;              /* throughput mode (with ln_fold): the N = d GEMMs of a layer (FFN out x2, attention out, cgMLP out, merge) and of the front end (the conv
                                    sub-sampling's output Linear, the feature projection) run on 256 x 256 tiles too — a quarter
                                    of the blocks of the 128 x 128 kernel (64 per launch at M = 8000, d = 512), 2x the FLOP per ingested byte.  Alone such a launch leaves most
                                    of the chip idle; it is meant for several independent steps in flight on their own streams (huggingface_asr_amd/pipeline.py), whose kernels
                                    then share the chip by CU instead of taking turns on all of it.  Same results as 0 up to the summation order of the row statistics. */
} mi_ebf_config;

/* weight-table slot indices: enum G / enum LS in huggingface_asr_amd/csrc/ebf_layout.hpp, mirrored by G / LS in huggingface_asr_amd/engine.py — the table is an array of device pointers. */
enum { MI_EBF_GLOBAL_SLOTS = 24, MI_EBF_LAYER_SLOTS = 64 };

size_t mi_ebf_workspace_bytes(const mi_ebf_config* cfg);

/* feats (B,T,F) fp32; feat_lengths (B) int32 valid frames (attention_mask.sum(-1)) or NULL;
 * pos_table: relative: (2*T2-1, d) bf16 sinusoid table; rotary: fp32 [cos (T2,hd) | sin (T2,hd)]; none: NULL;
 * posp: (L, 2*T2-1, d) bf16 scratch for the projected relative positions, recomputed when compute_posp != 0
 *       (it depends only on the weights and T2, so callers cache it across calls at inference);
 * workspace: mi_ebf_workspace_bytes(cfg) bytes, ZERO-INITIALISED ONCE by the caller (time padding of V^T);
 * outputs: last_hidden (B*T2, d) fp32 (nullable), logits (B*T2, V+1) fp32|bf16 (nullable),
 *          inner_len/outer_len (B) int32 (mask lengths / CTC input lengths, nullable).
 * With cfg->extra_layers the weight table holds L+1 layers and posp (L+1, 2*T2-1, d); last_hidden stays the ENCODER's last hidden state. */
int mi_ebf_forward(const mi_ebf_config* cfg, const void* const* weights, const float* feats, const int* feat_lengths,
                   const void* pos_table, void* posp, int compute_posp, void* workspace, size_t workspace_bytes,
                   float* last_hidden, void* logits, int* inner_len, int* outer_len, mi_stream_t stream);
/* the same, additionally filling hidden_states (L+1, B*T2, d) fp32 = HuggingFace's `output_hidden_states` tuple (transformers wav2vec2_conformer :685-713): the
 * input of every encoder layer, then the last hidden state; needs last_hidden != NULL. */
int mi_ebf_forward_hs(const mi_ebf_config* cfg, const void* const* weights, const float* feats, const int* feat_lengths,
                      const void* pos_table, void* posp, int compute_posp, void* workspace, size_t workspace_bytes,
                      float* last_hidden, void* logits, int* inner_len, int* outer_len, float* hidden_states, mi_stream_t stream);
/* the same, additionally leaving lse (B*T2) fp32 = the row log-sum-exp of the fp32 logits (the log_softmax of reference e_branchformer.py:472-488 is never materialised: the
 * CTC loss takes the logits and this vector) out of the head GEMM's epilogue — mi_gemm_lse_f32; lse_workspace: mi_gemm_lse_workspace_floats(B*T2, V+1) floats.
 * lse and lse_workspace both or neither; needs fp32 logits. */
int mi_ebf_forward_lse(const mi_ebf_config* cfg, const void* const* weights, const float* feats, const int* feat_lengths,
                       const void* pos_table, void* posp, int compute_posp, void* workspace, size_t workspace_bytes,
                       float* last_hidden, void* logits, int* inner_len, int* outer_len, float* hidden_states,
                       float* lse, float* lse_workspace, mi_stream_t stream);
/* the encoder + CTC head ending in the per-frame classes instead of logits: best (B*T2) int32 = argmax over the V+1 classes (mi_row_argmax's rules) — what
 * mi_ctc_collapse turns into token ids.  argmax_workspace (mi_gemm_argmax_workspace_floats(B*T2, V+1) floats, nullable): the head runs as mi_gemm_argmax_bf16 and writes
 * no logits.  head_scratch ((B*T2, logits_ld) in the config's logits dtype — engine.transcribe always sets logits_f32 for this call, so both head forms rank the same fp32 values —, nullable): where the head runs as mi_gemm_bf16 + mi_row_argmax — when argmax_workspace is
 * null or the shape is outside the fused kernel's (hidden size d: d % 64 != 0 or d < 128).  Checked before anything runs: both null is MI_ERR_ARG, a head outside
 * the fused kernel's shapes without head_scratch is MI_ERR_UNSUPPORTED. */
int mi_ebf_forward_greedy(const mi_ebf_config* cfg, const void* const* weights, const float* feats, const int* feat_lengths,
                          const void* pos_table, void* posp, int compute_posp, void* workspace, size_t workspace_bytes,
                          float* last_hidden, int* best, float* argmax_workspace, void* head_scratch, int* inner_len, int* outer_len, mi_stream_t stream);

/* ---- streaming inference for the causal (is_causal) encoder + CTC head: a stateful chunk step (csrc/stream.hip, whose header states the exact semantics).
 * replaces: nothing the reference runs — it trains streaming models (src/models/streaming_modules.py, recipes *_streaming.sh) and decodes them on whole utterances; the step
 * returns, piece by piece, the logits mi_ebf_forward returns for the utterance alone.  Opt-in; nothing above changes.  DESIGN.md §4 'Streaming'. */
/* attention of n_q new queries over a (B, Lmax, .) K/V cache of n_k >= n_q keys per stream, the causal diagonal at the end: query i sees keys j <= n_k - n_q + i.
 * q (B*n_q, ldq) bf16; k / v rows of the cache (row stride ldk == ldv, batch stride kv_bstride, elements; 16-B aligned, strides % 8 == 0); pos (>= n_k rows, ldp) bf16 = the
 * projected sinusoid of distance i - j in row i - j, with bias_u / bias_v (H*hd) — all three or none (plain attention; rotary is applied upstream); out (B*n_q, ldo) bf16.
 * ref: the probabilities are rounded to bf16 for the PV product as 2^(s - m); m = 0: the row maximum; 1 / 2 / 3: the running reference of the full forward's kernel walking
 * 32-key tiles — mi_attention_bf16's, the four-wave and the eight-wave form of mi_attention_qkv_bf16 —, which keeps a streamed layer closest to that forward.
 * MI_ERR_UNSUPPORTED: hd outside {16, 64, 128}, n_k > 8192.  No atomics; a stream's rows do not depend on the other streams. */
int mi_attention_chunk_bf16(const void* q, long ldq, const void* k, long ldk, const void* v, long ldv, long kv_bstride, const void* pos, long ldp,
                            const float* bias_u, const float* bias_v, void* out, long ldo, int B, int n_q, int n_k, int H, int hd, float scale, int ref, mi_stream_t stream);
/* stateful depthwise conv over time: in (B, n_new, ld_in) bf16 = rows [p, p + n_new) of every stream; ring (B, Hr, C) bf16 = rows [p - Hr, p) at slot t % Hr, advanced by
 * the same launch (modes 0 / 2 also ring_stats (B, ceil(C/64), Hr, 2) fp32); out (B, n_out, ld_out) bf16 = rows [o0, o0 + n_out).  Tap k reads row t - left + k*dil;
 * rows < 0, >= p + n_new and >= end[b] (end (B) int32, nullable) read as zero.  mode 0 CSGU: out = x_r * act(conv(LN(x_g)) + b) with the rows' given (mean, rstd) `stats`
 * (B*n_new, 2), gamma / beta, mul = x_r of the output rows (needs o0 == p, n_out == n_new), act 0..3 as mi_csgu_bf16; mode 1 MERGE: out = m + conv(m) + b; mode 2: the
 * conv of mode 0 alone (csgu_use_linear_after_conv).  MI_ERR_ARG: a window that leaves [p - Hr, p + n_new) (beyond the end only with `end`). */
int mi_dwconv_stream_bf16(const void* in, long ld_in, const void* mul, long ld_mul, const float* stats, const float* gamma, const float* beta,
                          const float* w, const float* bias, void* ring, float* ring_stats, const int* end, void* out, long ld_out,
                          int B, int C, int K, int dil, int left, int Hr, int p, int n_new, int o0, int n_out, int mode, int act, mi_stream_t stream);
/* mi_ctc_collapse across calls: best (B, T) int32; frames t < n_b count (n_b = n_valid[b] - offset clamped to [0, T]; T when n_valid is null); a frame is kept iff its
 * class is not blank and differs from the class before it — for t = 0 prev[b], the last class of the previous call (-1 at stream start); prev is updated.
 * ids (B, T) int32: the newly emitted tokens then -1; n_ids (B). */
int mi_ctc_collapse_stream(const int* best, int B, int T, const int* n_valid, int offset, int blank, int* prev, int* ids, int* n_ids, mi_stream_t stream);
/* the driver.  cfg as for mi_ebf_forward with B = streams, T = 4 * chunk_frames, fp32 logits; same weight table.  Refused (size 0 / MI_ERR_ARG / MI_ERR_UNSUPPORTED): a
 * non-causal config, a front end other than 3x3 / stride 2 / padding 1, the fine-tuning head, head sizes outside {16, 64, 128}, max_frames > 8192.
 * state: mi_ebf_stream_state_bytes bytes (host arithmetic; linear in max_frames) — caches, histories and the step's scratch; mi_ebf_stream_reset starts the streams
 * (relative positions: pos_table (max_frames, d) bf16 = the sinusoid of distance 0 .. max_frames - 1, projected per layer into the state).
 * mi_ebf_stream_step: feats (B, 4*chunk_frames, F) fp32; rows: HOST array of 2*(L+1) ints = (lo, hi) of the input rows of every layer and of the emitted rows
 * (streaming.plan); ends (B) int32 device, non-null exactly in the last step: every stream's frame count; pos_table: rotary fp32 [cos (max_frames, hd) | sin], else
 * unused.  For the n_out emitted frames: logits (B, n_out, logits_ld) fp32, best (B, n_out) int32, ids (B, n_out) int32 then -1, n_ids (B).  One call advances every
 * layer; no host round trip. */
size_t mi_ebf_stream_state_bytes(const mi_ebf_config* cfg, int chunk_frames, int max_frames);
int mi_ebf_stream_reset(const mi_ebf_config* cfg, const void* const* weights, int chunk_frames, int max_frames, const void* pos_table, void* state, size_t state_bytes,
                        mi_stream_t stream);
int mi_ebf_stream_step(const mi_ebf_config* cfg, const void* const* weights, int chunk_frames, int max_frames, const void* pos_table, void* state, size_t state_bytes,
                       const float* feats, const int* rows, const int* ends, float* logits, int* best, int* ids, int* n_ids, mi_stream_t stream);

/* ---- streaming session pool: S slots over one stream state (cfg.B = S), each with a position of its own; in a step a slot feeds a chunk, finishes or is idle, and is
 * reusable after it finishes (csrc/stream_pool.hip, whose header states the exact semantics).  The per-slot forms of the five kernels above that hold per-stream position
 * take a table of per-slot descriptors — twice: tab_host is checked (MI_ERR_ARG), tab_dev holds the same words on the device and is what the kernel reads.  Rows of the
 * active slots lie compactly one after another; the caches, rings and carried classes are indexed by slot.  No atomics.  DESIGN.md §4 'Session pool'. */
/* copy table, 7 ints per entry: src slot, src row, src modulus (0: no wrap), dst slot, dst row, dst modulus, rows.  src (src_slots, src_rows, src_ld), dst likewise; W
 * 4-byte words of a row are copied; strides in 4-byte words. */
int mi_copy_rows_slots(const void* src, long src_bs, long src_ld, int src_slots, int src_rows, void* dst, long dst_bs, long dst_ld, int dst_slots, int dst_rows,
                       const int* tab_host, const int* tab_dev, int A, int W, mi_stream_t stream);
/* mi_attention_chunk_bf16 per slot; 4 ints per entry: first query row (the prefix sum of the n_q before it), n_q, n_k, slot.  q / out (sum n_q, .) compact; k / v the
 * (slots, kv_rows, .) cache.  The grid runs over the total queries, the LDS is sized by the largest n_k. */
int mi_attention_chunk_slots_bf16(const void* q, long ldq, const void* k, long ldk, const void* v, long ldv, long kv_bstride, int slots, int kv_rows, const void* pos, long ldp,
                                  const float* bias_u, const float* bias_v, void* out, long ldo, const int* tab_host, const int* tab_dev, int A, int H, int hd, float scale,
                                  int ref, mi_stream_t stream);
/* mi_dwconv_stream_bf16 per slot; 8 ints per entry: slot, first in row, first out row, p, n_new, o0, n_out, end (0x7fffffff: none).  in / stats / mul / out compact; ring
 * (slots, Hr, C), ring_stats (slots, ceil(C/64), Hr, 2).  Only a slot with an end may read past its fed rows as zero. */
int mi_dwconv_stream_slots_bf16(const void* in, long ld_in, const void* mul, long ld_mul, const float* stats, const float* gamma, const float* beta, const float* w,
                                const float* bias, void* ring, float* ring_stats, int slots, void* out, long ld_out, const int* tab_host, const int* tab_dev, int A,
                                int C, int K, int dil, int left, int Hr, int mode, int act, mi_stream_t stream);
/* mi_rotary_bf16 with the position of a row = its slot's p + its index within the slot; 3 ints per entry: first row, rows, p.  cos_t / sin_t (tmax, hd) fp32. */
int mi_rotary_slots_bf16(const void* x, long ldx, void* out, long ldo, const float* cos_t, const float* sin_t, int tmax, const int* tab_host, const int* tab_dev,
                         int A, int H, int hd, mi_stream_t stream);
/* mi_ctc_collapse_stream per slot; 3 ints per entry: slot, first frame, frames.  best / ids compact, prev (slots), n_ids (A); an entry of zero frames keeps its carried class. */
int mi_ctc_collapse_slots(const int* best, int blank, int* prev, int slots, int* ids, int* n_ids, const int* tab_host, const int* tab_dev, int A, mi_stream_t stream);
/* the pool's driver.  State: mi_ebf_stream_state_bytes with cfg.B = slots, started once by mi_ebf_stream_reset.
 * mi_ebf_stream_slot_pieces: (offset, bytes of one slot's slice) of the 3 + 5 L persistent pieces (x_hist, c1_hist, prev; per layer kv, csgu, csgu_stats, cat, pend);
 *   -> their number (out may be null).  Host only.
 * mi_ebf_stream_reset_slot: one slot back to a stream start — its slices zero, its carried class -1 — in one launch on `stream`; no other slot is written.
 * records (HOST), A x (2 + 3 (L + 1)) ints: slot, end (the slot's own end when it finishes, else -1), then (lo, hi, off) of the slot's input rows of layer 0 .. L-1 and
 *   of the rows it emits: streaming.plan of the slot's own history, off = the sum of the earlier records' hi - lo at that layer.
 * mi_ebf_stream_slots_table: the records, checked, expanded into the words the step's kernels read -> their count (table null: only counted).  Host only; the caller
 *   uploads them, the step's one host-to-device transfer.
 * mi_ebf_stream_step_slots: feats (A, 4*chunk_frames, F) fp32 (a tail zero-padded); table: those words on the DEVICE.  Outputs compact in record order: logits
 *   (sum n_out, logits_ld) fp32, best / ids (sum n_out) int32 (ids: a record's new tokens then -1 in its n_out places), n_ids (A).  Attention is the per-slot chunk kernel
 *   everywhere (without a relative term at head sizes 64 / 128 with ref 3). */
int mi_ebf_stream_slot_pieces(const mi_ebf_config* cfg, int chunk_frames, int max_frames, long* out, int capacity);
int mi_ebf_stream_reset_slot(const mi_ebf_config* cfg, int chunk_frames, int max_frames, void* state, size_t state_bytes, int slot, mi_stream_t stream);
int mi_ebf_stream_slots_table(const mi_ebf_config* cfg, int chunk_frames, int max_frames, const int* records, int A, int* table, int capacity);
int mi_ebf_stream_step_slots(const mi_ebf_config* cfg, const void* const* weights, int chunk_frames, int max_frames, const void* pos_table, void* state, size_t state_bytes,
                             const float* feats, const int* records, int A, const int* table, int table_len, float* logits, int* best, int* ids, int* n_ids,
                             mi_stream_t stream);

/* ---- streaming from audio: the stateful log-mel front end of the streams and the pool (csrc/fbank_stream.hip, whose header states the exact semantics).  S slots, each
 * a carry of at most 399 samples (two buffers, a ping-pong the host chooses) and a ring of fifo_frames feature frames; state = [carry (S, 2, 400) | fifo (S, R, nmel)] fp32.
 * Every count and position is the caller's host arithmetic; no call synchronises or reads device memory.  Pushed in pieces of any size, a session's frames are bit for
 * bit mi_fbank_f64's (then mi_cmvn_global's) of its whole audio.  Records come twice as the pool's tables do: rec_host is checked, rec_dev is what the kernel reads.
 * mi_fbank_stream_state_bytes: S * (2 * 400 + R * nmel) * 4; 0 when refused (a count < 1, nmel > 127).  Host only.
 * mi_fbank_stream_push: one launch.  samples: n_samples values, fp32 in [-1, 1] (sample_dtype 0) or int16 PCM (1: (float)s / 32768.0f, exact).  Record (8 ints): slot,
 *   N_prev, n_new, offset of the new samples in `samples`, ring write position, frames held by the ring, current carry buffer (0 / 1), 0.  Frames T(N_prev) ..
 *   T(N_prev + n_new) - 1 (T(N) = N < 400 ? 0 : 1 + (N - 400) / 160) go to the ring, with normalize 1 as (x - means[f]) / stds[f]; the new carry, samples [160 T(N), N),
 *   goes to the other carry buffer.  n_new = 0: the slot is untouched.  Tables, mel_floor, preemph as mi_fbank_f64's.
 * mi_fbank_stream_pop: one launch.  Record (3 ints): slot, ring read position, n <= rows.  out (A, rows, nmel) fp32: the n frames, then zero rows.
 * MI_ERR_ARG before any launch: a slot out of range or named twice, a ring overrun, positions outside the ring, samples outside the buffer, nmel > 127, normalize 1
 * without tables, a state too small. */
size_t mi_fbank_stream_state_bytes(int slots, int fifo_frames, int nmel);
int mi_fbank_stream_push(void* state, size_t state_bytes, int slots, int fifo_frames, int nmel, const void* samples, long n_samples, int sample_dtype,
                         const int* rec_host, const int* rec_dev, int A, const double* window, const double* twiddle, const double* mel_t, const int* mel_lo,
                         const int* mel_hi, const float* means, const float* stds, int normalize, double mel_floor, double preemph, mi_stream_t stream);
int mi_fbank_stream_pop(const void* state, size_t state_bytes, int slots, int fifo_frames, int nmel, const int* rec_host, const int* rec_dev, int A, float* out,
                        int rows, mi_stream_t stream);

/* ---- precision = "fp32" inference mode (csrc/gemm_f32.hip, csrc/encoder_f32.hip): the encoder + CTC head with every operand, activation and weight in fp32 — what the
 * reference's decode recipes (no --bf16) compute.  Opt-in; nothing above changes.  DESIGN.md §4 'fp32 inference mode'. */
/* C (M,N) = resid + alpha * act(A (M,K) · W (N,K)^T + bias), all fp32, row-major with leading dimensions; act 0 none / 1 erf-GELU (exact erff) / 2 gelu_new (exact tanhf); bias, resid nullable,
 * resid may alias C.  f32-input MFMA (v_mfma_f32_32x32x2_f32), LDS-tiled; any M, N, K >= 1 (edges zero-filled / guarded).  An element is the k-ordered fmaf chain over
 * its row of A and its row of W: no split-K, no atomics, run-to-run bit-identical. */
int mi_gemm_f32(const float* A, long lda, const float* W, long ldw, const float* bias, float* C, long ldc, const float* resid, long ldr,
                float alpha, int act, int M, int N, int K, mi_stream_t stream);
/* y = LayerNorm(x) with fp32 statistics (two passes) and fp32 output; lengths (nullable): rows at t >= lengths[b] (row = b*T + t) are zeroed first, x_out (nullable, may
 * alias x) receives the rows after that zeroing.  y may alias x. */
int mi_layernorm_f32(const float* x, long ldx, const int* lengths, int T, float* x_out, long ldxo, const float* gamma, const float* beta, float eps,
                     float* y, long ldy, int M, int d, mi_stream_t stream);
int mi_rotary_f32(const float* x, long ldx, float* y, long ldy, const float* cos_t, const float* sin_t, int M, int T, int H, int hd, mi_stream_t stream);
/* depthwise Conv1d over time on (B*T, C) rows, weight (C, K): v[t,c] = bias[c] + sum_k w[c,k] x[t - pad_left + k*dilation, c], zero outside [0, T).
 * mode 0: y = v; 1: y = gate * act(v) (CSGU; act 0 identity, 1 gelu, 2 relu, 3 silu); 2: y = x + v (the merge's residual). */
int mi_dwconv_f32(const float* x, long ldx, const float* w, const float* bias, const float* gate, long ldg, float* y, long ldy,
                  int B, int T, int C, int K, int pad_left, int dilation, int act, int mode, mi_stream_t stream);
int mi_gate_act_mul_f32(const float* r, long ldr, const float* g, long ldg, float* s, long lds, int M, int N, int act, mi_stream_t stream);
/* the two Conv2d + GELU layers of the front end in fp32, same geometry arguments as mi_conv2d_first_gelu / mi_conv2d_cl_bf16; activations channels-last fp32.
 * mi_conv2d_cl_f32 is an implicit GEMM: the (kh, kw, cin) window is gathered inside mi_gemm_f32's A load, no im2col buffer exists. */
int mi_conv2d_first_gelu_f32(const float* x, const float* w, const float* bias, float* out_cl, int B, int T, int F, int C, int K, int stride,
                             int pad_t, int pad_f, int T1, int F1, mi_stream_t stream);
int mi_conv2d_cl_f32(const float* in, const float* weight, const float* bias, float* out, int B, int Tin, int Fin, int Cin, int Cout, int K, int stride,
                     int pad_t, int pad_f, int Tout, int Fout, int act, mi_stream_t stream);
/* fp32 attention (e_branchformer.py:74-141): fp32 scores materialised in workspace, fp32 softmax, fp32 P·V.  posp (2T-1, H*hd) / bias_u / bias_v: all three or none.
 * A key >= lengths[b], or above the diagonal when causal, contributes exactly 0.  The workspace is walked in chunks of utterances (of query rows when one utterance
 * alone does not fit): mi_attention_f32_workspace_bytes never exceeds MI_ATTENTION_F32_SCORES_BYTES (or one query row, if that is larger), whatever B and T. */
#define MI_ATTENTION_F32_SCORES_BYTES (64L << 20)
size_t mi_attention_f32_workspace_bytes(int B, int T, int H, int hd, int relative);
int mi_attention_f32(const float* q, long ldq, const float* k, long ldk, const float* v, long ldv, const float* posp, long ldp, const float* bias_u,
                     const float* bias_v, const int* lengths, float* out, long ldo, int B, int T, int H, int hd, float scale, int causal,
                     void* workspace, size_t workspace_bytes, mi_stream_t stream);
/* mi_ebf_forward in fp32: the same config struct and the same slot order, EVERY slot (matrices included) pointing at fp32; pos_table: the relative sinusoid table in
 * fp32 (rotary: as above); posp (L, 2*T2-1, d) fp32; logits (B*T2, logits_ld or V+1) fp32.  Layer order and residual arithmetic are those of mi_ebf_forward's un-folded
 * branch.  MI_ERR_UNSUPPORTED, before anything is launched, for context_mode != 0, layer_mixing, extra_layers, ln_fold, wide_tiles, branch_overlap
 * (mi_ebf_f32_workspace_bytes returns 0 for those).  The workspace needs no initialisation. */
size_t mi_ebf_f32_workspace_bytes(const mi_ebf_config* cfg);
int mi_ebf_forward_f32(const mi_ebf_config* cfg, const void* const* weights, const float* feats, const int* feat_lengths,
                       const void* pos_table, void* posp, int compute_posp, void* workspace, size_t workspace_bytes,
                       float* last_hidden, float* logits, int* inner_len, int* outer_len, mi_stream_t stream);

/* ---- precision = "fp32" for the joint model's decoder (csrc/decoder_f32.hip): the GPT-2 token step with fp32 weights, caches, cross tables and activations.  Opt-in;
 * nothing above changes (mi_gemm_f32 gains act 2 = gelu_new with the exact tanhf; its other values keep their bits).  DESIGN.md §4 'fp32 inference mode'. */
/* Rows-streaming fp32 linear, the counterpart of mi_linear_rows: out = act(x W^T + b), or out += that when accumulate (the in-place residual add), for 1 <= M <= 64
 * rows, any N; x (M, K), W (N, K), out (M, ldo) fp32; x and W 16-B aligned, ldx % 4 == ldw % 4 == 0.  K % 4 != 0 is MI_ERR_UNSUPPORTED, checked before anything else.
 * act 0 none / 2 gelu_new.  kcache != NULL (N == 3 dkv, M % U == 0): columns [dkv, 2 dkv) / [2 dkv, 3 dkv) of row m = b U + u also go to the fp32 kcache / vcache
 * (.., Lmax, dkv) at row past + u of sequence b.  W is the 32-row operand of v_mfma_f32_32x32x2_f32: each weight byte is read once per launch.  The launch spreads over N
 * and, where that leaves fewer blocks than CUs, over K (fp32 partials in workspace, added in slice order by a second launch): no float atomics, bit-reproducible, and a
 * row's result depends on that row alone, whatever M is.  workspace: mi_linear_rows_f32_workspace_bytes(M, N, K) bytes (0 when the launch is not split over K). */
size_t mi_linear_rows_f32_workspace_bytes(int M, int N, int K);
int mi_linear_rows_f32(const float* x, long ldx, const float* W, long ldw, const float* bias, int act, float* out, long ldo, int accumulate,
                       float* kcache, float* vcache, int U, int past, int Lmax, int dkv, int M, int N, int K, void* workspace, size_t workspace_bytes,
                       mi_stream_t stream);
/* fp32 attention of B batches of Tq queries over Tk keys (cross-attention, KV-cache steps): q (B*Tq, >= H*hd), head h at columns [h*hd, (h+1)*hd); k / v rows with strides
 * ldk / ldv, batch stride kv_bstride floats (0: Tk * ldk, which then needs ldk == ldv).  The B batches are B / beams utterances x `beams` hypotheses that read ONE K / V
 * table (and one entry of lengths) per utterance: batch b reads table b / beams.  lengths (B / beams) valid keys or NULL; causal: query i sees keys j <= i + Tk - Tq.
 * Scores, softmax (expf, division by the sum) and P V in fp32; a key outside the valid set contributes exactly 0 and is not read; a row with no key at all is uniform
 * over all Tk keys (as mi_attention_f32).  hd 64 or 128 and Tk <= 15360 (a row's scores live in LDS), else MI_ERR_UNSUPPORTED.  No atomics: bit-reproducible. */
int mi_attention_general_f32(const float* q, long ldq, const float* k, long ldk, const float* v, long ldv, const int* lengths, float* out, long ldo,
                             int B, int beams, int Tq, int Tk, long kv_bstride, int H, int hd, float scale, int causal, mi_stream_t stream);
/* mi_decoder_step_beams in fp32: the same config struct, pointer-table order (5 globals, 18 per layer) and argument meaning, EVERY slot pointing at fp32 (matrices
 * (out, in) included; slot 4 may be slot 0 itself: the tied head).  kcache / vcache: L pointers to (B, Lmax, d) fp32; cross_kv: L pointers to (B / beams * T_enc, 2d) fp32,
 * shared by an utterance's `beams` hypotheses (beams == 1: one table per row); enc_len (B / beams) or NULL.  U > 1 (a prompt) returns the last position's logits.  Up to 64
 * rows the linears stream their weights (mi_linear_rows_f32), above they run as mi_gemm_f32.  cfg->act must be 0 (gelu_new), step_form is ignored.  Head sizes other than
 * 64 / 128 are MI_ERR_UNSUPPORTED, checked before any pointer is read.  The workspace (mi_decoder_step_f32_workspace_bytes) needs no initialisation.  Beam
 * re-ordering of the fp32 caches: mi_kv_cache_reorder, a row copy in units of 2-byte elements, called with d = 2 * cfg->d. */
size_t mi_decoder_step_f32_workspace_bytes(const mi_gpt2_config* cfg, int B, int U);
int mi_decoder_step_f32(const mi_gpt2_config* cfg, const void* const* weights, const long* ids_new, int B, int beams, int U, int past, int Lmax,
                        void* const* kcache, void* const* vcache, const void* const* cross_kv, int T_enc, const int* enc_len, float emb_scale,
                        const float* head_bias, void* workspace, size_t workspace_bytes, float* logits, long ld_logits, mi_stream_t stream);
/* ---- Two-pass joint decoding (csrc/rescore.hip, whose header states the exact semantics): a CTC n-best rescored by one teacher-forced decoder pass.  No counterpart
 * in the reference.  No atomics, fixed summation order: bit-identical run to run.
 * mi_rescore_pack: tokens (B, N, Tt) int32 (tokens_dtype 0) / int64 (1), n_tokens (B, N) int32, ctc (B, N) fp32 -> ids, labels (B*N, U) int64 and len (B*N) int32.  Row
 * r = b N + n exists iff ctc[r] is finite, 0 <= k = n_tokens[r] <= min(U - 1, Tt) and its k tokens lie in [0, V): ids = [start, t_0 .. t_{k-1}, pad ..], labels =
 * [t_0 .. t_{k-1}, eos, -100 ..], len = k + 1; otherwise ids = [start, pad ..], labels = -100, len = 0.
 * mi_rows_nll_f32: nll[m] = lse[m] - x[m * ld + labels[m]], exactly 0 for labels[m] < 0 or >= V (x (M, ld >= V) fp32).
 * mi_rescore_select: one block per utterance, N <= 64.  att[n] = -(((nll[0] + nll[1]) + nll[2]) ...) over u < len[n], ascending; total[n] = (w_ctc * ctc[n] + w_att *
 * att[n]) / denom[len[n]], each multiply, the add and the divide rounded once (denom: U + 1 fp32 values from the host).  len = 0 (or outside [0, U]) and NaN totals
 * count as -inf; descending total, equal totals by lower n.  For the best K <= N, best first: order (B, K) int32 = n, total / att / ctc_out (B, K), token_lp (B, K, U) =
 * -nll then 0, out_tokens (B, K, U) int64 = the tokens, eos, then pad, out_n (B, K) int32 = the token count, out_frames (B, K, U) int32 = frames (B, N, Tt) then -1
 * (frames and out_frames both null or both given).
 * MI_ERR_ARG before any launch: a null operand, B / N / Tt / V / U < 1, N > 64, K outside 1..N, a bad tokens_dtype. */
int mi_rescore_pack(const void* tokens, int tokens_dtype, const int* n_tokens, const float* ctc, int B, int N, int Tt, int V, int U, long start, long eos, long pad,
                    long* ids, long* labels, int* len, mi_stream_t stream);
int mi_rows_nll_f32(const float* x, long ld, const float* lse, const long* labels, int V, float* nll, int M, mi_stream_t stream);
int mi_rescore_select(const float* nll, const int* len, const float* ctc, const float* denom, float w_ctc, float w_att, int B, int N, int U, int K, const void* tokens,
                      int tokens_dtype, int Tt, const int* frames, long eos, long pad, int* order, float* total, float* att, float* ctc_out, float* token_lp,
                      long* out_tokens, int* out_n, int* out_frames, mi_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
