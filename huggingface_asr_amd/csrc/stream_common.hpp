// What the lock-step stream step (stream.hip) and the session pool (stream_pool.hip) share, written once: the bodies of the three kernels that hold per-stream
// position — chunk attention, the stateful depthwise conv, the CTC collapse with a carried class —, the layout of the state and the check of a step's plan (the launch
// sequence of a step is stream_step.hpp's).  A lock-step kernel hands a body the batch-wide scalars of its call, a pool kernel the entry of its slot's descriptor: the
// arithmetic of a row is the same instructions either way, which is what the pool's bit-equality with a stream of one rests on.  Internal: nothing here is exported.
#pragma once
#include "ebf_layout.hpp"

namespace {

constexpr float LEPS = 1e-5f;      // nn.LayerNorm default of the layers (encoder.hip)

// ------------------------------------------------------------------------------------------------ chunk attention
// One wave per (stream, head, query).  The query at absolute frame ia sees keys j <= ia of its stream's cache.  Scores in fp32 over bf16 operands ((q + u), (q + v)
// rounded to bf16 as the full kernels' A operands are); the un-normalised probabilities are rounded to bf16 for the PV product and the normaliser is summed from the
// un-rounded ones, as in the full kernels.  Those kernels walk the keys in tiles of 32 and exponentiate against a running reference m (any m gives the same quotient,
// but bf16(2^(s - m)) depends on it), so the rounding of a probability depends on the walk.  `ref` selects whose walk the rounding follows, which is what keeps a
// streamed layer closest to the full forward's:
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
    int n_q, n_k, H, nkp, ntp, ref;          // nkp: (the largest) n_k rounded up to 4 (a wave's score row); ntp: tiles of 32 keys + 1, rounded up to 4
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

// the wave's query: qrow its head's HD columns, kb / vbp its stream's cache at the head's columns, ia its absolute frame, orow where the context goes (null: a wave
// past the last query, which still walks to the block barriers), sc the wave's nkp + 2 HD + 2 ntp floats of LDS.  Every wave of a block calls this.
template <int HD>
__device__ __forceinline__ void attn_chunk_row(const AttnArgs& p, float* sc, const bf16_t* qrow, const bf16_t* kb, const bf16_t* vbp, int ia, bf16_t* orow, int h, int lane) {
    float* qu = sc + p.nkp;
    float* qv = qu + HD;
    float* tm = qv + HD;                       // tile maxima
    float* mr = tm + p.ntp;                    // the reference each tile is exponentiated against; [ntile] = the largest of them
    for (int c = lane; c < HD; c += 64) {
        const float qf = bf2f(qrow[c]);
        qu[c] = p.pos ? bf2f(f2bf(qf + p.u[h * HD + c])) : qf;
        qv[c] = p.pos ? bf2f(f2bf(qf + p.vb[h * HD + c])) : 0.f;
    }
    __syncthreads();
    const int nkeys = ia + 1;
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
    if (orow && g == 0) {
#pragma unroll
        for (int e = 0; e < DPL; ++e) orow[cl + e * LPG] = f2bf(acc[e] / l);
    }
}

// ------------------------------------------------------------------------------------------------ stateful depthwise conv over time
// A block owns 64 channels of one stream for ALL rows of the call (a depthwise conv never mixes channels), so it may read its slice of the ring, compute, and — after
// a block barrier — overwrite that slice with the call's last rows: no other block reads or writes those channels.  The ring holds rows [p - Hr, p) at slot t % Hr.
// mode 0 CSGU: out = x_r * act(bias + sum_k w_k LN(x_g)[t - left + k dil]),  LN from the given (mean, rstd) of each row and gamma / beta; the ring keeps the raw rows
//              and a per-channel-tile copy of their statistics.      mode 2 conv-only: the same without act and gate (csgu_use_linear_after_conv).
// mode 1 MERGE: out = m[t] + bias + sum_k w_k m[t - left + k],  rows at or beyond the stream's end (when given) and rows not yet fed count as zero.
// The sum runs from the bias through the taps k = 0 .. K-1 in order, as dwconv_time_kernel's (conv.hip).
struct DwsArgs {
    const bf16_t* in; long ld_in;            // the call's new rows [p, p + n_new), compact
    const bf16_t* mul; long ld_mul;          // CSGU: x_r of the output rows
    const float* stats;                      // CSGU / conv-only: (rows of `in`, 2)
    const float* gamma; const float* beta; const float* w; const float* bias;
    bf16_t* ring; float* ring_stats;         // (B, Hr, C) ; (B, ceil(C / 64), Hr, 2)
    const int* end;                          // lock-step: (B) or null
    bf16_t* out; long ld_out;                // rows [o0, o0 + n_out), compact
    int B, C, K, dil, left, Hr, p, n_new, o0, n_out, mode, act;       // p, n_new, o0, n_out: lock-step, the whole batch's
};
// one stream's share of a call: its new rows (and their statistics), its ring (and the channel tile's ring statistics), x_r and the output at its first output row
struct DwsStream {
    const bf16_t* nin; const float* nst; bf16_t* ring; float* rst; const bf16_t* mul; bf16_t* out;
    int end, p, n_new, o0, n_out;            // end: 0x7fffffff = none
};

__device__ __forceinline__ void dwconv_stream_body(const DwsArgs& a, const DwsStream& s, int ct) {
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int c = ct * 64 + tx;
    const bool cok = c < a.C;
    const bool ln = a.mode != 1;
    const int endb = s.end;
    const int hi = s.p + s.n_new;
    const bf16_t* nin = s.nin;
    const float* nst = s.nst;
    bf16_t* ring = s.ring;
    float* rst = s.rst;
    float g = 1.f, be = 0.f, bias = 0.f;
    if (cok) {
        if (ln) { g = a.gamma[c]; be = a.beta[c]; }
        if (a.bias) bias = a.bias[c];
    }
    auto fetch = [&](int t) -> float {
        if (t < 0 || t >= hi || t >= endb || t < s.p - a.Hr) return 0.f;       // zero padding is applied to the conv INPUT (post-LN)
        float v, mean, rstd;
        if (t >= s.p) {
            v = bf2f(nin[(long)(t - s.p) * a.ld_in + c]);
            if (ln) { mean = nst[2 * (t - s.p)]; rstd = nst[2 * (t - s.p) + 1]; }
        } else {
            const int sl = t % a.Hr;
            v = bf2f(ring[(long)sl * a.C + c]);
            if (ln) { mean = rst[2 * sl]; rstd = rst[2 * sl + 1]; }
        }
        return ln ? (v - mean) * rstd * g + be : v;
    };
    if (cok) {
        const float* wc = a.w + (long)c * a.K;
        for (int j = ty; j < s.n_out; j += 4) {
            const int t = s.o0 + j;
            float acc = bias;
            for (int k = 0; k < a.K; ++k) acc = fmaf(wc[k], fetch(t - a.left + k * a.dil), acc);
            float o;
            if (a.mode == 1) {
                o = fetch(t) + acc;
            } else if (a.mode == 0) {
                if (a.act == 1) acc = gelu_erf(acc);
                else if (a.act == 2) acc = fmaxf(acc, 0.f);
                else if (a.act == 3) acc = acc / (1.f + __expf(-acc));
                o = bf2f(s.mul[(long)j * a.ld_mul + c]) * acc;
            } else {
                o = acc;
            }
            s.out[(long)j * a.ld_out + c] = f2bf(o);
        }
    }
    __syncthreads();
    // advance the ring: the last min(n_new, Hr) rows of the call
    const int t0 = s.n_new > a.Hr ? hi - a.Hr : s.p;
    for (int t = t0 + ty; t < hi; t += 4) {
        const int sl = t % a.Hr;
        if (cok) ring[(long)sl * a.C + c] = nin[(long)(t - s.p) * a.ld_in + c];
        if (ln && tx < 2) rst[2 * sl + tx] = nst[2 * (t - s.p) + tx];
    }
}

// ------------------------------------------------------------------------------------------------ CTC collapse with a carried class
// row: the per-frame classes of one stream's call, of which the first n count; frame t is kept iff its class is not blank and differs from the class before it, which
// for t = 0 is *prev (the last class of the previous call; -1 at stream start).  out (T): the kept classes in order, then -1; *n_ids their count; *prev becomes the
// class of frame n - 1.  One wave.
__device__ __forceinline__ void ctc_collapse_row(const int* __restrict__ row, int n, int T, int blank, int* __restrict__ prev, int* __restrict__ out, int* __restrict__ n_ids, int lane) {
    const int carried = *prev;
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
        *n_ids = count;
        if (n > 0) *prev = row[n - 1];
    }
}

// ------------------------------------------------------------------------------------------------ the drivers' state
struct Geo {
    int B, C, Lmax, L, d, I, H, hd, F, F1, F2, C1, C2, V1, r, Hc, dil, Kc, Km, N, ctiles;
    long ldl;
};

inline bool geometry(const mi_ebf_config* c, int C, int Lmax, Geo& g) {
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

// every persistent piece is (B, ...): stream b's slice of a piece is `slot` bytes at b * slot
struct LayerState { bf16_t *kv, *csgu, *cat; float *csgu_stats, *pend; };
struct St {
    float* x_hist; bf16_t* c1_hist; int* prev; bf16_t* posp; LayerState* ls;      // ls: host array of L entries
    size_t persistent;                                                            // bytes reset() clears
    float *featcat, *feo, *fp, *x, *xo, *res, *stats;
    bf16_t *act1n, *act1c, *act2, *a0, *a1, *a2, *a1r, *h, *qk, *ctx, *cat, *m2, *s, *cv, *lin, *hid;
    size_t bytes;
};

inline St carve_state(const mi_ebf_config& c, const Geo& g, void* base, LayerState* ls) {
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

inline bool supported(const mi_ebf_config& c, const Geo& g) {
    return !c.extra_layers && !c.layer_mixing && !c.context_mode && (g.hd == 16 || g.hd == 64 || g.hd == 128) && g.Lmax <= 8192 && g.L <= 64;
}

// Are (lo, hi) of entries 0 .. L (entry l at lo_hi[l * stride], the lock-step step's plan or a record of a pool step) a step streaming.plan could have produced, in a
// finish or not?  Frontiers never decrease, an entry holds at most N rows (entry 0: C), none past the caches, the merge window stays inside its history, a layer emits up to a_l - r (finish: a_l).
inline bool plan_ok(const Geo& g, const int* lo_hi, int stride, bool finish) {
    for (int l = 0; l <= g.L; ++l) {
        const int lo = lo_hi[l * stride], hi = lo_hi[l * stride + 1];
        const int plo = l ? lo_hi[(l - 1) * stride] : lo, phi = l ? lo_hi[(l - 1) * stride + 1] : hi;      // the entry before
        if (lo < 0 || hi < lo || hi - lo > (l ? g.N : g.C) || hi > g.Lmax) return false;
        if (l && (hi > phi || lo > plo || plo - lo > g.r || hi != (finish ? phi : (phi > g.r ? phi - g.r : 0)))) return false;
    }
    return true;
}

}  // namespace
