// Streaming inference for the causal E-Branchformer + CTC models (is_causal = True; reference src/models/streaming_modules.py, recipes
// pretrain_bestrq_ebranchformer_base_full_streaming.sh / finetune_full_czech_streaming.sh): a stateful chunk step that, fed an utterance piece by piece, returns for
// every encoder frame the logits the full-utterance forward (mi_ebf_forward) returns for that utterance alone.  bf16 path, rounding points of Fwd::plain_layer.
//
// Semantics (normative)
//  * A stream batch is B streams advanced in lock-step.  A step takes (B, 4*C, F) fp32 feature frames; C = the chunk size in encoder frames, fixed when the state is
//    created, 4 = the product of the conv strides.  The last step (`finish`) takes 0 .. 4*C valid frames per stream (the rest zero) and flushes.  A stream may end only
//    inside that last step; independent start / end times per slot are out of scope.
//  * After n feature frames the front end has produced a_0 = out_frames(n) frames; n = 4k gives k (causal geometry: conv1 frame i reads input 2i-2 .. 2i, conv2 the
//    same over conv1).  State: the last two input frames and the last two conv1 output frames per stream, zero at stream start — a zero history is exactly the left
//    padding of CausalConv2d (streaming_modules.py:31-55).
//  * The reference's causal layer is NOT strictly causal: depthwise_conv_fusion (e_branchformer.py:248-256) keeps its symmetric padding r = (merge_conv_kernel-1)/2,
//    so a layer looks r frames ahead and a stack of L layers L*r frames.  The engine carries that as per-layer lag.  Layer l has an input frontier a_l; given new
//    input rows [a_l', a_l):
//      - everything row-wise runs on those rows: macaron FFN, the LayerNorms, QKV, output projections, cgMLP projections;
//      - K and V are appended to the layer's cache (capacity max_frames);
//      - the query at absolute frame i attends keys j <= i; relative positions use the projected sinusoid of distance i - j (its content depends on the distance
//        only: tf wav2vec2_conformer :531-536 slices one table around its centre); rotary uses absolute position i;
//        (kernel: mi_attention_chunk_bf16 below with relative positions and at head size 16; without a relative term at head sizes 64 / 128 the full forward's own
//        mi_attention_qkv_bf16, which takes a cache when there is no position term);
//      - the CSGU conv reads LN(x_g) at t - (K-1)*dil + k*dil from a history of (K-1)*dil rows (dil = (K-1)/2, the reference's quirk); rows before frame 0 are zero;
//      - the new cat = [att | cgmlp] rows are pushed into the merge history;
//      - the layer emits rows [a_{l+1}', a_{l+1}) with a_{l+1} = max(0, a_l - r): for those, m2 = cat + dwconv(cat) sees cat rows up to +r, merge_proj adds the
//        pending residual rows, then the second macaron FFN and the final LayerNorm run;
//      - in `finish`, a_{l+1} = a_l = max_b n_b for every l, and cat rows at or beyond stream b's end n_b = out_frames(its frames) count as zero — what the full
//        forward of the unpadded utterance pads with.  Rows a stream emits at or beyond n_b are not results.
//  * Per-layer state: the K/V cache, the CSGU history (raw bf16 x_g rows with their (mean, rstd)), the merge history of 2r cat rows, and at most r pending residual
//    rows in fp32, the residual stream's dtype.
//  * A step returns logits (B, n_out, V+1) for the newly final frames and the CTC greedy tokens newly emitted (the collapse carries the last class across steps).
//    Row counts come from the caller's plan (host): `rows` holds (lo, hi) of every layer's input and of the emitted rows; no host round trip inside a step.
//  * No atomics; a stream's result does not depend on the rest of the batch (every kernel here works per stream, the GEMMs per row).
#include "ebf_layout.hpp"

namespace {

constexpr float LEPS = 1e-5f;      // nn.LayerNorm default of the layers (encoder.hip)

// ------------------------------------------------------------------------------------------------ rows between compact buffers, caches and rings
// dst[b][(dst_row0 + i) % dst_mod][:W] = src[b][(src_row0 + i) % src_mod][:W] for i < n (mod 0: no wrap); W, the row strides (ld) and batch strides (bs) in 4-byte words
__global__ __launch_bounds__(256) void copy_rows_kernel(const uint32_t* __restrict__ src, long src_bs, long src_ld, int src_row0, int src_mod, uint32_t* __restrict__ dst, long dst_bs,
                                                        long dst_ld, int dst_row0, int dst_mod, int n, int W, int B) {
    const long total = (long)B * n * W;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int w = (int)(i % W);
        const int r = (int)((i / W) % n);
        const int b = (int)(i / ((long)W * n));
        int rs = src_row0 + r, rd = dst_row0 + r;
        if (src_mod > 0) rs %= src_mod;
        if (dst_mod > 0) rd %= dst_mod;
        dst[b * dst_bs + rd * dst_ld + w] = src[b * src_bs + rs * src_ld + w];
    }
}

int copy_rows_ld(const void* src, long src_bs, long src_ld, int src_row0, int src_mod, void* dst, long dst_bs, long dst_ld, int dst_row0, int dst_mod, int n, int W, int B,
                 hipStream_t st) {
    if (n <= 0 || W <= 0 || B <= 0) return MI_OK;
    const long total = (long)B * n * W;
    const int grid = (int)((total + 255) / 256 < 2048 ? (total + 255) / 256 : 2048);
    hipLaunchKernelGGL(copy_rows_kernel, dim3(grid), dim3(256), 0, st, (const uint32_t*)src, src_bs, src_ld, src_row0, src_mod, (uint32_t*)dst, dst_bs, dst_ld,
                       dst_row0, dst_mod, n, W, B);
    MI_CHECK_LAUNCH();
    return MI_OK;
}
// the same for dense rows (row stride = W)
int copy_rows(const void* src, long src_bs, int src_row0, int src_mod, void* dst, long dst_bs, int dst_row0, int dst_mod, int n, int W, int B, hipStream_t st) {
    return copy_rows_ld(src, src_bs, W, src_row0, src_mod, dst, dst_bs, W, dst_row0, dst_mod, n, W, B, st);
}

// ------------------------------------------------------------------------------------------------ chunk attention
// One wave per (stream, head, query); a block holds four consecutive queries.  Query i of the n_q new rows stands at absolute frame n_k - n_q + i and sees keys
// j <= that frame of the (B, Lmax, .) cache.  Scores in fp32 over bf16 operands ((q + u), (q + v) rounded to bf16 as the full kernels' A operands are); the
// un-normalised probabilities are rounded to bf16 for the PV product and the normaliser is summed from the un-rounded ones, as in the full kernels.  Those kernels
// walk the keys in tiles of 32 and exponentiate against a running reference m (any m gives the same quotient, but bf16(2^(s - m)) depends on it), so the rounding of a
// probability depends on the walk.  `ref` selects whose walk the rounding follows, which is what keeps a streamed layer closest to the full forward's:
//   0  one reference, the row maximum (no tiling)
//   1  attn_kernel's (mi_attention_bf16, head size 16): m = the maximum of all tiles so far, natural-log domain
//   2  attn_lds_kernel's (four waves; head size 64 with relative positions): exp2 domain, m moves to max(m, tile maximum) only when that exceeds m + 11
//   3  attn8_kernel's (eight waves; every other 64 / 128 case): as 2, but the even and the odd tiles are two walks with a reference each
// (the full kernels move m for all 32 queries of a wave when one of them asks; that coupling between queries is not reproduced.)
struct AttnArgs {
    const bf16_t* q; long ldq;
    const bf16_t* k; const bf16_t* v; long ldkv, kv_bs;
    const bf16_t* pos; long ldp;             // (>= n_k, .) projected sinusoids by distance, or null
    const float* u; const float* vb;
    bf16_t* out; long ldo;
    int n_q, n_k, H, nkp, ntp, ref;          // nkp: n_k rounded up to 4 (a wave's score row); ntp: tiles of 32 keys + 1, rounded up to 4
    float scale;
};

template <int HD>
__device__ __forceinline__ float dot_row(const float* __restrict__ a, const bf16_t* __restrict__ row) {
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < HD; c += 8) {
        const bf16x8 kv = *reinterpret_cast<const bf16x8*>(row + c);
#pragma unroll
        for (int e = 0; e < 8; ++e) s = fmaf(a[c + e], bf2f(kv[e]), s);
    }
    return s;
}

template <int HD>
__global__ __launch_bounds__(256) void attn_chunk_kernel(AttnArgs p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    float* sc = reinterpret_cast<float*>(smem) + (size_t)wave * (p.nkp + 2 * HD + 2 * p.ntp);
    float* qu = sc + p.nkp;
    float* qv = qu + HD;
    float* tm = qv + HD;                       // tile maxima
    float* mr = tm + p.ntp;                    // the reference each tile is exponentiated against; [ntile] = the largest of them
    const int h = blockIdx.y, b = blockIdx.z;
    const int iq = blockIdx.x * 4 + wave;
    const bool live = iq < p.n_q;
    const int i = live ? iq : p.n_q - 1;
    const bf16_t* qrow = p.q + ((long)b * p.n_q + i) * p.ldq + h * HD;
    for (int c = lane; c < HD; c += 64) {
        const float qf = bf2f(qrow[c]);
        qu[c] = p.pos ? bf2f(f2bf(qf + p.u[h * HD + c])) : qf;
        qv[c] = p.pos ? bf2f(f2bf(qf + p.vb[h * HD + c])) : 0.f;
    }
    __syncthreads();
    const int ia = p.n_k - p.n_q + i;          // absolute frame of the query = index of its last key
    const int nkeys = ia + 1;
    const bf16_t* kb = p.k + (long)b * p.kv_bs + h * HD;
    const bf16_t* vbp = p.v + (long)b * p.kv_bs + h * HD;
    const bool e2 = p.ref >= 2;                // exp2 domain: the score carries scale * log2(e)
    const float sc2 = e2 ? p.scale * 1.4426950408889634f : p.scale;
    for (int j = lane; j < nkeys; j += 64) {
        float s = dot_row<HD>(qu, kb + (long)j * p.ldkv);
        if (p.pos) s += dot_row<HD>(qv, p.pos + (long)(ia - j) * p.ldp + h * HD);
        sc[j] = s * sc2;
    }
    __syncthreads();
    const int ntile = (nkeys + 31) >> 5;
    for (int t = lane; t < ntile; t += 64) {
        float mx = -INFINITY;
        const int je = min(32 * t + 32, nkeys);
        for (int j = 32 * t; j < je; ++j) mx = fmaxf(mx, sc[j]);
        tm[t] = mx;
    }
    __syncthreads();
    if (lane == 0) {                           // the walk(s) over the tiles: a few dozen steps
        float m0 = -1e30f, m1 = -1e30f, top = -1e30f;
        if (p.ref == 0)
            for (int t = 0; t < ntile; ++t) m0 = fmaxf(m0, tm[t]);
        for (int t = 0; t < ntile; ++t) {
            float& m = (p.ref == 3 && (t & 1)) ? m1 : m0;
            if (p.ref == 1) m = fmaxf(m, tm[t]);
            else if (p.ref >= 2 && tm[t] > m + 11.f) m = fmaxf(m, tm[t]);
            mr[t] = m;
            top = fmaxf(top, m);
        }
        mr[ntile] = top;
    }
    __syncthreads();
    const float top = mr[ntile];
    float l = 0.f;
    for (int j = lane; j < nkeys; j += 64) {
        const float m = mr[j >> 5];
        float e, w;
        if (e2) { e = __builtin_amdgcn_exp2f(sc[j] - m); w = __builtin_amdgcn_exp2f(m - top); }
        else if (p.ref == 1) { e = __expf(sc[j] - m); w = __expf(m - top); }
        else { e = expf(sc[j] - m); w = 1.f; }
        l += e * w;                            // the walk's accumulators are rescaled in fp32 when its reference moves: the weight of an older tile
        sc[j] = bf2f(f2bf(e)) * w;
    }
    l = wave_sum(l);
    __syncthreads();
    // PV: a group of LPG lanes owns the head's columns (DPL per lane), the 64 / LPG groups split the keys and are folded in a fixed order
    constexpr int DPL = HD > 64 ? HD / 64 : 1, LPG = HD / DPL, G = 64 / LPG;
    const int g = lane / LPG, cl = lane % LPG;
    float acc[DPL];
#pragma unroll
    for (int e = 0; e < DPL; ++e) acc[e] = 0.f;
    for (int j = g; j < nkeys; j += G) {
        const float pj = sc[j];
        const bf16_t* vr = vbp + (long)j * p.ldkv;
#pragma unroll
        for (int e = 0; e < DPL; ++e) acc[e] = fmaf(pj, bf2f(vr[cl + e * LPG]), acc[e]);
    }
#pragma unroll
    for (int o = LPG; o < 64; o <<= 1)
#pragma unroll
        for (int e = 0; e < DPL; ++e) acc[e] += __shfl_xor(acc[e], o, 64);
    if (live && g == 0) {
        bf16_t* orow = p.out + ((long)b * p.n_q + iq) * p.ldo + h * HD;
#pragma unroll
        for (int e = 0; e < DPL; ++e) orow[cl + e * LPG] = f2bf(acc[e] / l);
    }
}

// ------------------------------------------------------------------------------------------------ stateful depthwise conv over time
// A block owns 64 channels of one stream for ALL rows of the call (a depthwise conv never mixes channels), so it may read its slice of the ring, compute, and — after
// a block barrier — overwrite that slice with the call's last rows: no other block reads or writes those channels.  The ring holds rows [p - Hr, p) at slot t % Hr.
// mode 0 CSGU: out = x_r * act(bias + sum_k w_k LN(x_g)[t - left + k dil]),  LN from the given (mean, rstd) of each row and gamma / beta; the ring keeps the raw rows
//              and a per-channel-tile copy of their statistics.      mode 2 conv-only: the same without act and gate (csgu_use_linear_after_conv).
// mode 1 MERGE: out = m[t] + bias + sum_k w_k m[t - left + k],  rows at or beyond end[b] (when given) and rows not yet fed count as zero.
// The sum runs from the bias through the taps k = 0 .. K-1 in order, as dwconv_time_kernel's (conv.hip).
struct DwsArgs {
    const bf16_t* in; long ld_in;            // the call's new rows [p, p + n_new), compact (B, n_new, .)
    const bf16_t* mul; long ld_mul;          // CSGU: x_r of the output rows
    const float* stats;                      // CSGU / conv-only: (B * n_new, 2)
    const float* gamma; const float* beta; const float* w; const float* bias;
    bf16_t* ring; float* ring_stats;         // (B, Hr, C) ; (B, ceil(C / 64), Hr, 2)
    const int* end;                          // (B) or null
    bf16_t* out; long ld_out;                // rows [o0, o0 + n_out), compact (B, n_out, .)
    int B, C, K, dil, left, Hr, p, n_new, o0, n_out, mode, act;
};

__global__ __launch_bounds__(256) void dwconv_stream_kernel(DwsArgs a) {
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int b = blockIdx.y, ct = blockIdx.x, c = ct * 64 + tx;
    const bool cok = c < a.C;
    const bool ln = a.mode != 1;
    const int endb = a.end ? a.end[b] : 0x7fffffff;
    const int hi = a.p + a.n_new;
    const bf16_t* nin = a.in + (long)b * a.n_new * a.ld_in;
    const float* nst = ln ? a.stats + (long)b * a.n_new * 2 : nullptr;
    bf16_t* ring = a.ring + (long)b * a.Hr * a.C;
    float* rst = ln ? a.ring_stats + ((long)b * gridDim.x + ct) * a.Hr * 2 : nullptr;
    float g = 1.f, be = 0.f, bias = 0.f;
    if (cok) {
        if (ln) { g = a.gamma[c]; be = a.beta[c]; }
        if (a.bias) bias = a.bias[c];
    }
    auto fetch = [&](int t) -> float {
        if (t < 0 || t >= hi || t >= endb || t < a.p - a.Hr) return 0.f;       // zero padding is applied to the conv INPUT (post-LN)
        float v, mean, rstd;
        if (t >= a.p) {
            v = bf2f(nin[(long)(t - a.p) * a.ld_in + c]);
            if (ln) { mean = nst[2 * (t - a.p)]; rstd = nst[2 * (t - a.p) + 1]; }
        } else {
            const int s = t % a.Hr;
            v = bf2f(ring[(long)s * a.C + c]);
            if (ln) { mean = rst[2 * s]; rstd = rst[2 * s + 1]; }
        }
        return ln ? (v - mean) * rstd * g + be : v;
    };
    if (cok) {
        const float* wc = a.w + (long)c * a.K;
        for (int j = ty; j < a.n_out; j += 4) {
            const int t = a.o0 + j;
            float acc = bias;
            for (int k = 0; k < a.K; ++k) acc = fmaf(wc[k], fetch(t - a.left + k * a.dil), acc);
            const long orow = (long)b * a.n_out + j;
            float o;
            if (a.mode == 1) {
                o = fetch(t) + acc;
            } else if (a.mode == 0) {
                if (a.act == 1) acc = gelu_erf(acc);
                else if (a.act == 2) acc = fmaxf(acc, 0.f);
                else if (a.act == 3) acc = acc / (1.f + __expf(-acc));
                o = bf2f(a.mul[orow * a.ld_mul + c]) * acc;
            } else {
                o = acc;
            }
            a.out[orow * a.ld_out + c] = f2bf(o);
        }
    }
    __syncthreads();
    // advance the ring: the last min(n_new, Hr) rows of the call
    const int t0 = a.n_new > a.Hr ? hi - a.Hr : a.p;
    for (int t = t0 + ty; t < hi; t += 4) {
        const int s = t % a.Hr;
        if (cok) ring[(long)s * a.C + c] = nin[(long)(t - a.p) * a.ld_in + c];
        if (ln && tx < 2) rst[2 * s + tx] = nst[2 * (t - a.p) + tx];
    }
}

// ------------------------------------------------------------------------------------------------ CTC collapse with a carried class
// best (B, T) int32: frame t < n_b of stream b is kept iff best != blank and best != the class before it, which for t = 0 is prev[b] (the last class of the
// previous call; -1 at stream start).  ids (B, T) int32: the kept classes in order, then -1; n_ids (B); prev[b] becomes the class of frame n_b - 1.  One wave per stream.
__global__ __launch_bounds__(64) void ctc_collapse_stream_kernel(const int* __restrict__ best, int T, const int* __restrict__ n_valid, int offset, int blank,
                                                                 int* __restrict__ prev, int* __restrict__ ids, int* __restrict__ n_ids) {
    const int b = blockIdx.x, lane = threadIdx.x;
    int n = n_valid ? n_valid[b] - offset : T;
    n = n < 0 ? 0 : (n > T ? T : n);
    const int* row = best + (long)b * T;
    int* out = ids + (long)b * T;
    const int carried = prev[b];
    int count = 0;
    for (int base = 0; base < n; base += 64) {
        const int t = base + lane;
        bool keep = false;
        int c = blank;
        if (t < n) {
            c = row[t];
            const int before = t == 0 ? carried : row[t - 1];
            keep = c != blank && c != before;
        }
        const unsigned long long mask = __ballot(keep);
        if (keep) out[count + __popcll(mask & ((1ull << lane) - 1ull))] = c;
        count += __popcll(mask);
    }
    for (int t = count + lane; t < T; t += 64) out[t] = -1;
    if (lane == 0) {
        n_ids[b] = count;
        if (n > 0) prev[b] = row[n - 1];
    }
}

// ------------------------------------------------------------------------------------------------ the driver's state
struct Geo {
    int B, C, Lmax, L, d, I, H, hd, F, F1, F2, C1, C2, V1, r, Hc, dil, Kc, Km, N, ctiles;
    long ldl;
};

bool geometry(const mi_ebf_config* c, int C, int Lmax, Geo& g) {
    if (!c || c->B <= 0 || c->H <= 0 || c->L <= 0 || c->d <= 0 || (c->d % c->H) || (c->I % 2) || C <= 0 || Lmax <= 0) return false;
    if (c->K != 3 || c->stride != 2 || c->pad != 1 || !c->is_causal || c->T != 4 * C) return false;      // the front-end state (two rows per conv) is that of 3 x 3 / stride 2
    if (c->merge_kernel < 1 || !(c->merge_kernel & 1) || c->csgu_kernel < 1 || !(c->csgu_kernel & 1)) return false;
    g.B = c->B; g.C = C; g.Lmax = Lmax; g.L = c->L; g.d = c->d; g.I = c->I; g.H = c->H; g.hd = c->d / c->H; g.F = c->F;
    g.F1 = conv_out(c->F, 3, 2, 2); g.F2 = conv_out(g.F1, 3, 2, 2); g.C1 = c->C1; g.C2 = c->C2; g.V1 = c->V + 1;
    g.Km = c->merge_kernel; g.r = (g.Km - 1) / 2; g.Kc = c->csgu_kernel; g.dil = (g.Kc - 1) / 2; g.Hc = (g.Kc - 1) * g.dil;
    g.N = C + g.L * g.r;                     // most rows a layer takes or emits in one step (the flush)
    g.ctiles = (g.I / 2 + 63) / 64;
    g.ldl = c->logits_ld > 0 ? c->logits_ld : g.V1;
    return g.F2 > 0;
}

struct LayerState { bf16_t *kv, *csgu, *cat; float *csgu_stats, *pend; };
struct St {
    float* x_hist; bf16_t* c1_hist; int* prev; bf16_t* posp; LayerState* ls;      // ls: host array of L entries
    size_t persistent;                                                            // bytes reset() clears
    float *featcat, *feo, *fp, *x, *xo, *res, *stats;
    bf16_t *act1n, *act1c, *act2, *a0, *a1, *a2, *a1r, *h, *qk, *ctx, *cat, *m2, *s, *cv, *lin, *hid;
    size_t bytes;
};

St carve_state(const mi_ebf_config& c, const Geo& g, void* base, LayerState* ls) {
    Carver k{(char*)base, 0};
    auto bf = [&](size_t n) { return (bf16_t*)k.take(n * 2 + 16); };
    auto f32 = [&](size_t n) { return (float*)k.take(n * 4 + 16); };
    St s;
    const size_t B = g.B, d = g.d, I = g.I;
    s.x_hist = f32(B * 2 * g.F);
    s.c1_hist = bf(B * 2 * g.F1 * g.C1);
    s.prev = (int*)k.take(B * 4);
    s.ls = ls;
    for (int l = 0; l < g.L; ++l) {
        LayerState t;
        t.kv = bf(B * g.Lmax * 2 * d);
        t.csgu = bf(B * g.Hc * (I / 2));
        t.csgu_stats = f32(B * g.ctiles * g.Hc * 2);
        t.cat = bf(B * 2 * g.r * 2 * d);
        t.pend = f32(B * (size_t)(g.r + g.N) * d);
        if (ls) ls[l] = t;
    }
    s.persistent = k.off;
    s.posp = c.pos_type == 1 ? bf((size_t)g.L * g.Lmax * d) : nullptr;
    const size_t M = B * g.N, Mc = B * g.C;
    s.featcat = f32(B * (4 * g.C + 2) * g.F);
    s.act1n = bf(B * 2 * g.C * g.F1 * g.C1); s.act1c = bf(B * (2 * g.C + 2) * g.F1 * g.C1); s.act2 = bf(Mc * g.F2 * g.C2);
    s.feo = f32(Mc * d); s.fp = f32(Mc * d);
    s.x = f32(M * d); s.xo = f32(M * d); s.res = f32(M * d); s.stats = f32(M * 2);
    s.a0 = bf(M * d); s.a1 = bf(M * d); s.a2 = bf(M * d); s.a1r = bf(M * d);
    s.h = bf(M * I); s.qk = bf(M * 3 * d); s.ctx = bf(M * d); s.cat = bf(M * 2 * d); s.m2 = bf(M * 2 * d); s.s = bf(M * (I / 2));
    s.cv = s.lin = nullptr;
    if (c.csgu_linear) { s.cv = bf(M * (I / 2)); s.lin = bf(M * (I / 2)); }
    s.hid = bf(M * d);
    s.bytes = k.off;
    return s;
}

bool supported(const mi_ebf_config& c, const Geo& g) {
    return !c.extra_layers && !c.layer_mixing && !c.context_mode && (g.hd == 16 || g.hd == 64 || g.hd == 128) && g.Lmax <= 8192 && g.L <= 64;
}

}  // namespace

// q (B * n_q, ldq) bf16: the new rows' queries; k / v: a (B, Lmax, .) cache with row stride ldkv and batch stride kv_bstride (elements) holding n_k >= n_q keys per
// stream, the new rows' own keys last (the causal diagonal at the end); pos (>= n_k rows, ldp) bf16: the projected sinusoid of distance i - j in row i - j with
// bias_u / bias_v (H*hd) fp32, or all three null (plain attention; rotary is applied upstream); out (B * n_q, ldo) bf16.  hd 16 / 64 / 128, n_k <= 8192.
// ref 0 .. 3: whose walk over the keys the rounding of the probabilities follows (attn_chunk_kernel).
extern "C" int mi_attention_chunk_bf16(const void* q, long ldq, const void* k, long ldk, const void* v, long ldv, long kv_bstride, const void* pos, long ldp,
                                       const float* bias_u, const float* bias_v, void* out, long ldo, int B, int n_q, int n_k, int H, int hd, float scale,
                                       int ref, hipStream_t stream) {
    MI_ENTER();
    if (!q || !k || !v || !out || B <= 0 || n_q <= 0 || n_k < n_q || H <= 0 || ldk != ldv || ref < 0 || ref > 3) return MI_ERR_ARG;
    if ((pos != nullptr) != (bias_u != nullptr) || (pos != nullptr) != (bias_v != nullptr)) return MI_ERR_ARG;
    if ((ldk % 8) || (kv_bstride % 8) || (pos && (ldp % 8)) || ((uintptr_t)k & 15) || ((uintptr_t)v & 15) || ((uintptr_t)pos & 15)) return MI_ERR_ARG;
    if ((hd != 16 && hd != 64 && hd != 128) || n_k > 8192 || H > 65535 || B > 65535) return MI_ERR_UNSUPPORTED;
    AttnArgs a{(const bf16_t*)q, ldq, (const bf16_t*)k, (const bf16_t*)v, ldk, kv_bstride, (const bf16_t*)pos, ldp, bias_u, bias_v, (bf16_t*)out, ldo,
               n_q, n_k, H, (n_k + 3) / 4 * 4, ((n_k + 31) / 32 + 1 + 3) / 4 * 4, ref, scale};
    const size_t lds = (size_t)4 * (a.nkp + 2 * hd + 2 * a.ntp) * sizeof(float);
    const dim3 grid(cdiv(n_q, 4), H, B);
#define LAUNCH_ATTN(HD)                                                                                              \
    do {                                                                                                             \
        if (lds > 65536 && !ensure_dynamic_lds<HD>((const void*)attn_chunk_kernel<HD>, 4 * (8192 + 2 * HD + 2 * 260) * sizeof(float))) return MI_ERR_LAUNCH; \
        hipLaunchKernelGGL(attn_chunk_kernel<HD>, grid, dim3(256), lds, stream, a);                                   \
    } while (0)
    if (hd == 16) LAUNCH_ATTN(16);
    else if (hd == 64) LAUNCH_ATTN(64);
    else LAUNCH_ATTN(128);
#undef LAUNCH_ATTN
    MI_CHECK_LAUNCH();
    return MI_OK;
}

// in (B, n_new, ld_in) bf16: rows [p, p + n_new) of every stream; ring (B, Hr, C) bf16 (+ ring_stats (B, ceil(C/64), Hr, 2) fp32 in modes 0 / 2): rows [p - Hr, p) at slot
// t % Hr, advanced by this launch; out (B, n_out, ld_out) bf16: rows [o0, o0 + n_out).  Tap k reads row t - left + k * dil; rows < 0, >= p + n_new, >= end[b] (end
// nullable) read as zero.  Needs o0 - left >= p - Hr and o0 + n_out - 1 - left + (K - 1) dil <= p + n_new - 1 + (end ? left : 0): checked.  mode 0 CSGU (mul = x_r of the
// output rows, stats (B * n_new, 2), gamma, beta, act 0..3), 1 MERGE (out = m + conv(m); stats, gamma, beta, mul null), 2 conv only.  Hr = 0 (K = 1): ring may be null.
extern "C" int mi_dwconv_stream_bf16(const void* in, long ld_in, const void* mul, long ld_mul, const float* stats, const float* gamma, const float* beta,
                                     const float* w, const float* bias, void* ring, float* ring_stats, const int* end, void* out, long ld_out,
                                     int B, int C, int K, int dil, int left, int Hr, int p, int n_new, int o0, int n_out, int mode, int act, hipStream_t stream) {
    MI_ENTER();
    if (B <= 0 || C <= 0 || K <= 0 || dil <= 0 || left < 0 || Hr < 0 || p < 0 || n_new < 0 || o0 < 0 || n_out < 0 || mode < 0 || mode > 2 || act < 0 || act > 3) return MI_ERR_ARG;
    if (!w || (n_new > 0 && !in) || (n_out > 0 && !out) || (Hr > 0 && !ring)) return MI_ERR_ARG;
    if (mode != 1 && (!gamma || !beta || (n_new > 0 && !stats) || (Hr > 0 && !ring_stats))) return MI_ERR_ARG;
    if (mode == 0 && !mul) return MI_ERR_ARG;
    if (n_out > 0 && (o0 - left < p - Hr || (long)o0 + n_out - 1 - left + (long)(K - 1) * dil > (long)p + n_new - 1 + (end ? left : 0))) return MI_ERR_ARG;
    if (B > 65535) return MI_ERR_UNSUPPORTED;
    if (n_new == 0 && n_out == 0) return MI_OK;
    DwsArgs a{(const bf16_t*)in, ld_in, (const bf16_t*)mul, ld_mul, stats, gamma, beta, w, bias, (bf16_t*)ring, ring_stats, end, (bf16_t*)out, ld_out,
              B, C, K, dil, left, Hr, p, n_new, o0, n_out, mode, act};
    // Hr == 0 (K = 1): no row is read from the ring (fetch refuses t < p - Hr first) and none is written
    hipLaunchKernelGGL(dwconv_stream_kernel, dim3(cdiv(C, 64), B), dim3(256), 0, stream, a);
    MI_CHECK_LAUNCH();
    return MI_OK;
}

// best (B, T) int32 per-frame classes of one call; frames t < n_b count, n_b = n_valid[b] - offset clamped to [0, T], or T when n_valid is null.  prev (B) int32: the
// class of the last frame before this call (-1 at stream start), updated; ids (B, T) int32: the newly emitted tokens, then -1; n_ids (B).  ids must not alias best.
extern "C" int mi_ctc_collapse_stream(const int* best, int B, int T, const int* n_valid, int offset, int blank, int* prev, int* ids, int* n_ids, hipStream_t stream) {
    MI_ENTER();
    if (!best || !prev || !ids || !n_ids || B <= 0 || T <= 0 || ids == best) return MI_ERR_ARG;
    hipLaunchKernelGGL(ctc_collapse_stream_kernel, dim3(B), dim3(64), 0, stream, best, T, n_valid, offset, blank, prev, ids, n_ids);
    MI_CHECK_LAUNCH();
    return MI_OK;
}

// bytes of the state of a stream batch: cfg as for mi_ebf_forward with B = streams, T = 4 * chunk_frames; the per-layer caches, rings and the step's scratch.  0: a
// configuration the step refuses.  Host arithmetic only.
extern "C" size_t mi_ebf_stream_state_bytes(const mi_ebf_config* cfg, int chunk_frames, int max_frames) {
    Geo g;
    if (!geometry(cfg, chunk_frames, max_frames, g) || !supported(*cfg, g)) return 0;
    return carve_state(*cfg, g, nullptr, nullptr).bytes;
}

// stream start: zero histories, caches and the carried class (-1); relative positions: pos_table (max_frames, d) bf16 = the sinusoid of distance 0 .. max_frames-1 is
// projected by every layer's linear_pos into the state.
extern "C" int mi_ebf_stream_reset(const mi_ebf_config* cfg, const void* const* weights, int chunk_frames, int max_frames, const void* pos_table, void* state,
                                   size_t state_bytes, hipStream_t st) {
    MI_ENTER();
    Geo g;
    if (!geometry(cfg, chunk_frames, max_frames, g) || !state || !weights) return MI_ERR_ARG;
    if (!supported(*cfg, g)) return MI_ERR_UNSUPPORTED;
    LayerState ls[64];
    const St s = carve_state(*cfg, g, state, ls);
    if (s.bytes > state_bytes || (cfg->pos_type == 1 && !pos_table)) return MI_ERR_ARG;
    if (hipMemsetAsync(state, 0, s.persistent, st) != hipSuccess) return MI_ERR_LAUNCH;
    if (hipMemsetAsync(s.prev, 0xFF, (size_t)g.B * 4, st) != hipSuccess) return MI_ERR_LAUNCH;
    if (cfg->pos_type == 1) {
        const Slots t{weights};
        for (int l = 0; l < g.L; ++l)
            RUN(mi_gemm_bf16(pos_table, g.d, t.Lw(l, ATT_WPOS), g.d, nullptr, 0, s.posp + (size_t)l * g.Lmax * g.d, g.d, 0, nullptr, 0, 1.f, 0, g.Lmax, g.d, g.d, 0, 0, st));
    }
    return MI_OK;
}

// One step of every layer.  feats (B, 4*C, F) fp32 (zero beyond a stream's valid frames in the last step); rows: HOST array of 2 * (L + 1) ints, (lo, hi) of the input
// rows of layer 0 .. L-1 and of the rows the last layer emits (huggingface_asr_amd/streaming.py `plan`); ends (B) int32 on the device, the last step only: n_b, else null;
// pos_table: rotary: fp32 [cos (max_frames, hd) | sin (max_frames, hd)], else unused.  Outputs for the n_out = rows[2L+1] - rows[2L] emitted frames: logits
// (B, n_out, logits_ld) fp32, best (B, n_out) int32 per-frame classes, ids (B, n_out) int32 newly emitted tokens then -1, n_ids (B).  n_out = 0: nothing is written.
extern "C" int mi_ebf_stream_step(const mi_ebf_config* cfg, const void* const* weights, int chunk_frames, int max_frames, const void* pos_table, void* state,
                                  size_t state_bytes, const float* feats, const int* rows, const int* ends, float* logits, int* best, int* ids, int* n_ids, hipStream_t st) {
    MI_ENTER();
    Geo g;
    if (!geometry(cfg, chunk_frames, max_frames, g) || !state || !weights || !feats || !rows) return MI_ERR_ARG;
    const mi_ebf_config& c = *cfg;
    if (!supported(c, g)) return MI_ERR_UNSUPPORTED;
    if (!c.logits_f32 || (c.pos_type == 2 && !pos_table) || c.pos_type < 0 || c.pos_type > 2) return MI_ERR_ARG;
    LayerState ls[64];
    const St s = carve_state(c, g, state, ls);
    if (s.bytes > state_bytes) return MI_ERR_ARG;
    const int B = g.B, C = g.C, d = g.d, I = g.I, L = g.L, r = g.r;
    // the plan, checked: frontiers never decrease, a layer takes and emits at most N rows, nothing runs past the caches, the merge window stays inside its history
    for (int l = 0; l <= L; ++l) {
        const int lo = rows[2 * l], hi = rows[2 * l + 1];
        if (lo < 0 || hi < lo || hi - lo > g.N || hi > g.Lmax) return MI_ERR_ARG;
        if (l == 0 && hi - lo > C) return MI_ERR_ARG;
        if (l > 0 && (hi > rows[2 * l - 1] || lo > rows[2 * l - 2] || rows[2 * l - 2] - lo > r || (!ends && hi != (rows[2 * l - 1] > r ? rows[2 * l - 1] - r : 0)))) return MI_ERR_ARG;
        if (l > 0 && ends && hi != rows[2 * l - 1]) return MI_ERR_ARG;
    }
    const int n_out = rows[2 * L + 1] - rows[2 * L];
    if (n_out > 0 && (!logits || !best || !ids || !n_ids)) return MI_ERR_ARG;
    const Slots W{weights};
    const float scale = 1.0f / sqrtf((float)g.hd);

    // ---- front end on [2 history rows | the new rows] of each conv's input, no time padding: the history IS the left padding (zero at stream start)
    const long wF = g.F, wA = (long)g.F1 * g.C1 / 2;                   // row widths in 4-byte words
    if ((g.F1 * g.C1) % 2) return MI_ERR_UNSUPPORTED;
    RUN(copy_rows(s.x_hist, 2 * wF, 0, 0, s.featcat, (4 * C + 2) * wF, 0, 0, 2, (int)wF, B, st));
    RUN(copy_rows(feats, 4 * C * wF, 0, 0, s.featcat, (4 * C + 2) * wF, 2, 0, 4 * C, (int)wF, B, st));
    RUN(copy_rows(s.featcat, (4 * C + 2) * wF, 4 * C, 0, s.x_hist, 2 * wF, 0, 0, 2, (int)wF, B, st));
    RUN(mi_conv2d_first_gelu(s.featcat, W.Gf(G_CONV1_W), W.Gf(G_CONV1_B), s.act1n, B, 4 * C + 2, g.F, g.C1, 3, 2, 0, 2, 2 * C, g.F1, st));
    RUN(copy_rows(s.c1_hist, 2 * wA, 0, 0, s.act1c, (2 * C + 2) * wA, 0, 0, 2, (int)wA, B, st));
    RUN(copy_rows(s.act1n, 2 * C * wA, 0, 0, s.act1c, (2 * C + 2) * wA, 2, 0, 2 * C, (int)wA, B, st));
    RUN(copy_rows(s.act1c, (2 * C + 2) * wA, 2 * C, 0, s.c1_hist, 2 * wA, 0, 0, 2, (int)wA, B, st));
    RUN(mi_conv2d_cl_bf16(s.act1c, W.Gw(G_CONV2_W), W.Gf(G_CONV2_B), s.act2, B, 2 * C + 2, g.F1, g.C1, g.C2, 3, 3, 2, 0, 2, C, g.F2, 1, st));
    const int Mc = B * C;
    RUN(mi_gemm_bf16(s.act2, (long)g.F2 * g.C2, W.Gw(G_FEOUT_W), (long)g.F2 * g.C2, W.Gf(G_FEOUT_B), 1, s.feo, d, 1, nullptr, 0, 1.f, 0, Mc, d, g.F2 * g.C2, 0, 0, st));
    RUN(mi_layernorm_chain(s.feo, d, nullptr, C, nullptr, nullptr, 0.f, nullptr, 0, W.Gf(G_FP_LN_G), W.Gf(G_FP_LN_B), c.ln_eps, s.a0, d, nullptr, 0, nullptr, nullptr, nullptr, 0, Mc, d, st));
    RUN(mi_gemm_bf16(s.a0, d, W.Gw(G_FP_W), d, W.Gf(G_FP_B), 1, s.fp, d, 1, nullptr, 0, 1.f, 0, Mc, d, d, 0, 0, st));
    const int n0 = rows[1] - rows[0];
    RUN(copy_rows(s.fp, (long)C * d, 0, 0, s.x, (long)n0 * d, 0, 0, n0, d, B, st));           // the first n0 of the C new frames are frames of the utterance(s)

    // ---- the layers: x holds layer l's new input rows, compact (B, n_in, d)
    for (int l = 0; l < L; ++l) {
        const int p = rows[2 * l], a = rows[2 * l + 1], o0 = rows[2 * l + 2], o1 = rows[2 * l + 3];
        const int n_in = a - p, n_o = o1 - o0, M = B * n_in, Mo = B * n_o;
        const LayerState& t = ls[l];
        const int Rp = r + g.N;                                            // the pending-residual ring: rows [o0, a) always fit
        if (n_in > 0) {
            // first LayerNorm(s) of the layer on its input rows (the previous layer's final_layer_norm output, or the feature projection)
            if (c.use_macaron) {       // x += 0.5 * FFN(LN(x))   e_branchformer.py:271-273
                RUN(mi_layernorm_chain(s.x, d, nullptr, n_in, nullptr, nullptr, 0.f, nullptr, 0, W.Lf(l, FF1_LN_G), W.Lf(l, FF1_LN_B), LEPS, s.a0, d, nullptr, 0, nullptr, nullptr, nullptr, 0, M, d, st));
                RUN(mi_gemm_bf16(s.a0, d, W.Lw(l, FF1_W1), d, W.Lf(l, FF1_B1), 1, s.h, I, 0, nullptr, 0, 1.f, 1, M, I, d, 0, 0, st));
                RUN(mi_gemm_bf16(s.h, I, W.Lw(l, FF1_W2), I, W.Lf(l, FF1_B2), 1, s.x, d, 1, s.x, d, 0.5f, 0, M, d, I, 0, 0, st));
            }
            RUN(mi_layernorm_chain(s.x, d, nullptr, n_in, nullptr, nullptr, 0.f, nullptr, 0, W.Lf(l, ATT_LN_G), W.Lf(l, ATT_LN_B), LEPS, s.a1, d, nullptr, 0,
                                   W.Lf(l, MLP_LN_G), W.Lf(l, MLP_LN_B), s.a2, d, M, d, st));
            // the residual of the merge: rows [p, a) into the pending ring
            RUN(copy_rows(s.x, (long)n_in * d, 0, 0, t.pend, (long)Rp * d, p, Rp, n_in, d, B, st));
            // global branch: Q | K | V of the new rows, K | V appended to the cache, chunk attention over the cache
            const bf16_t* qk_in = s.a1;
            if (c.pos_type == 2) {
                const float* cs = (const float*)pos_table;
                RUN(mi_rotary_bf16(s.a1, d, s.a1r, d, cs + (size_t)p * g.hd, cs + ((size_t)g.Lmax + p) * g.hd, M, n_in, g.H, g.hd, st));
                qk_in = s.a1r;
                RUN(mi_gemm_bf16(qk_in, d, W.Lw(l, ATT_WQK), d, W.Lf(l, ATT_BQK), 1, s.qk, 3 * d, 0, nullptr, 0, 1.f, 0, M, 2 * d, d, 0, 0, st));
                RUN(mi_gemm_bf16(s.a1, d, W.Lw(l, ATT_WV), d, W.Lf(l, ATT_BV), 1, s.qk + 2 * d, 3 * d, 0, nullptr, 0, 1.f, 0, M, d, d, 0, 0, st));
            } else {
                RUN(mi_gemm_bf16(s.a1, d, W.Lw(l, ATT_WQK), d, W.Lf(l, ATT_BQK), 1, s.qk, 3 * d, 0, nullptr, 0, 1.f, 0, M, 3 * d, d, 0, 0, st));
            }
            // cache rows [p, a) = the [K | V] columns of the new rows (d words out of rows 3d/2 words apart)
            RUN(copy_rows_ld(s.qk + d, (long)n_in * 3 * d / 2, 3 * d / 2, 0, 0, t.kv, (long)g.Lmax * d, d, p, 0, n_in, d, B, st));
            const bf16_t* posp = c.pos_type == 1 ? s.posp + (size_t)l * g.Lmax * d : nullptr;
            if (!posp && (g.hd == 64 || g.hd == 128)) {
                // without a relative term the full forward's own kernel takes a cache (Tk != T, the causal diagonal at the end): the same key tiles, the same MFMA
                // sums per (query, key) — the streamed contexts are the full forward's bit for bit as long as no query of a wave moves the softmax reference late
                RUN(mi_attention_qkv_bf16(s.qk, 3 * d, t.kv, 2 * d, t.kv + d, 2 * d, nullptr, 0, nullptr, nullptr, nullptr, s.ctx, d, B, n_in, a, (long)g.Lmax * 2 * d, g.H, g.hd,
                                          scale, 1, st));
            } else {                  // relative positions (mi_attention_qkv_bf16 refuses them with Tk != T) and head size 16
                RUN(mi_attention_chunk_bf16(s.qk, 3 * d, t.kv, 2 * d, t.kv + d, 2 * d, (long)g.Lmax * 2 * d, posp, d, posp ? W.Lf(l, ATT_U) : nullptr, posp ? W.Lf(l, ATT_V) : nullptr,
                                            s.ctx, d, B, n_in, a, g.H, g.hd, scale, g.hd == 16 ? 1 : (g.hd == 64 ? 2 : 3), st));       // the full forward's kernel for this shape
            }
            RUN(mi_gemm_bf16(s.ctx, d, W.Lw(l, ATT_WO), d, W.Lf(l, ATT_BO), 1, s.cat, 2 * d, 0, nullptr, 0, 1.f, 0, M, d, d, 0, 0, st));
            // local branch: cgMLP with the stateful CSGU conv
            RUN(mi_gemm_bf16(s.a2, d, W.Lw(l, MLP_W1), d, W.Lf(l, MLP_B1), 1, s.h, I, 0, nullptr, 0, 1.f, 1, M, I, d, 0, 0, st));
            RUN(mi_row_stats_bf16(s.h + I / 2, I, I / 2, LEPS, s.stats, M, st));
            if (!c.csgu_linear) {
                RUN(mi_dwconv_stream_bf16(s.h + I / 2, I, s.h, I, s.stats, W.Lf(l, CSGU_LN_G), W.Lf(l, CSGU_LN_B), W.Lf(l, CSGU_W), W.Lf(l, CSGU_B), t.csgu, t.csgu_stats, nullptr,
                                          s.s, I / 2, B, I / 2, g.Kc, g.dil, g.Hc, g.Hc, p, n_in, p, n_in, 0, c.csgu_act, st));
            } else {
                RUN(mi_dwconv_stream_bf16(s.h + I / 2, I, nullptr, 0, s.stats, W.Lf(l, CSGU_LN_G), W.Lf(l, CSGU_LN_B), W.Lf(l, CSGU_W), W.Lf(l, CSGU_B), t.csgu, t.csgu_stats, nullptr,
                                          s.cv, I / 2, B, I / 2, g.Kc, g.dil, g.Hc, g.Hc, p, n_in, p, n_in, 2, 0, st));
                RUN(mi_gemm_bf16(s.cv, I / 2, W.Lw(l, CSGU_LIN_W), I / 2, W.Lf(l, CSGU_LIN_B), 1, s.lin, I / 2, 0, nullptr, 0, 1.f, 0, M, I / 2, I / 2, 0, 0, st));
                RUN(mi_gate_act_mul_bf16(s.h, I, s.lin, I / 2, s.s, I / 2, M, I / 2, c.csgu_act, st));
            }
            RUN(mi_gemm_bf16(s.s, I / 2, W.Lw(l, MLP_W2), I / 2, W.Lf(l, MLP_B2), 1, s.cat + d, 2 * d, 0, nullptr, 0, 1.f, 0, M, d, I / 2, 0, 0, st));
        }
        if (n_in == 0 && n_o == 0) continue;
        // merge: push the new cat rows, m2 = cat + dwconv(cat) for the rows whose lookahead is complete (all pending ones in the last step)
        RUN(mi_dwconv_stream_bf16(s.cat, 2 * d, nullptr, 0, nullptr, nullptr, nullptr, W.Lf(l, MRG_DW_W), W.Lf(l, MRG_DW_B), t.cat, nullptr, ends, s.m2, 2 * d,
                                  B, 2 * d, g.Km, 1, r, 2 * r, p, n_in, o0, n_o, 1, 0, st));
        if (n_o == 0) continue;
        RUN(copy_rows(t.pend, (long)Rp * d, o0, Rp, s.res, (long)n_o * d, 0, 0, n_o, d, B, st));
        RUN(mi_gemm_bf16(s.m2, 2 * d, W.Lw(l, MRG_W), 2 * d, W.Lf(l, MRG_B), 1, s.xo, d, 1, s.res, d, 1.0f, 0, Mo, d, 2 * d, 0, 0, st));
        if (c.use_macaron) {   // e_branchformer.py:307-309
            RUN(mi_layernorm_chain(s.xo, d, nullptr, n_o, nullptr, nullptr, 0.f, nullptr, 0, W.Lf(l, FF2_LN_G), W.Lf(l, FF2_LN_B), LEPS, s.a0, d, nullptr, 0, nullptr, nullptr, nullptr, 0, Mo, d, st));
            RUN(mi_gemm_bf16(s.a0, d, W.Lw(l, FF2_W1), d, W.Lf(l, FF2_B1), 1, s.h, I, 0, nullptr, 0, 1.f, 1, Mo, I, d, 0, 0, st));
            RUN(mi_gemm_bf16(s.h, I, W.Lw(l, FF2_W2), I, W.Lf(l, FF2_B2), 1, s.xo, d, 1, s.xo, d, 0.5f, 0, Mo, d, I, 0, 0, st));
        }
        if (l + 1 < L)         // final_layer_norm (:312): the next layer's input rows
            RUN(mi_layernorm_chain(s.xo, d, nullptr, n_o, W.Lf(l, FIN_LN_G), W.Lf(l, FIN_LN_B), LEPS, s.x, d, nullptr, nullptr, 0.f, nullptr, 0, nullptr, 0, nullptr, nullptr, nullptr, 0, Mo, d, st));
        else                   // chained with encoder.layer_norm -> the head's input
            RUN(mi_layernorm_chain(s.xo, d, nullptr, n_o, W.Lf(l, FIN_LN_G), W.Lf(l, FIN_LN_B), LEPS, nullptr, 0, W.Gf(G_ENC_LN_G), W.Gf(G_ENC_LN_B), c.ln_eps, s.hid, d, nullptr, 0,
                                   nullptr, nullptr, nullptr, 0, Mo, d, st));
    }
    if (n_out == 0) return MI_OK;
    // ---- CTC head, per-frame classes, collapse with the carried class
    const int Mo = B * n_out;
    RUN(mi_gemm_bf16(s.hid, d, W.Gw(G_HEAD_W), d, W.Gf(G_HEAD_B), 1, logits, g.ldl, 1, nullptr, 0, 1.f, 0, Mo, g.V1, d, 0, 0, st));
    RUN(mi_row_argmax(logits, g.ldl, 0, g.V1, best, Mo, st));
    return mi_ctc_collapse_stream(best, B, n_out, ends, rows[2 * L], c.V, s.prev, ids, n_ids, st);
}
