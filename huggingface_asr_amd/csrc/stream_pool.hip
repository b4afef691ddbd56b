// Streaming session pool for the causal E-Branchformer + CTC models: S slots over the state of stream.hip (whose header states what a stream step computes), each with
// a position of its own.  The kernels here are the per-slot forms of stream.hip's: they take a device table of per-slot descriptors where those take batch-wide scalars,
// and run the same bodies (stream_common.hpp).  The launch sequence of a step is stream_step.hpp's, the one the lock-step stream runs: mi_ebf_stream_step_slots hands
// it the PerSlot policy below, through which that body copies rows, rotates, attends, convolves and collapses at every slot's own position.
//
// Semantics (normative)
//  * The state is mi_ebf_stream_state_bytes' for cfg.B = S slots: every persistent piece is (S, ...), the scratch holds S * (C + L*r) rows.
//  * A slot is started by mi_ebf_stream_reset_slot: zero histories and rings, carried class -1.  One launch on the caller's stream, no synchronisation; no byte of any
//    other slot is written.  (mi_ebf_stream_reset of stream.hip starts all S slots and, with relative positions, projects the position table: call it once first.)
//  * In a step a slot either feeds one chunk of 4*C feature frames, finishes (a tail of 0 .. 4*C frames, zero-padded to 4*C; every frame still inside its L*r frames of
//    lookahead becomes final), or is idle.  Only the A active slots appear in the step's records; nothing of an idle slot's state is read or written.
//  * The row ranges are the caller's host arithmetic (huggingface_asr_amd/streaming.py `pool_table`): record i = [slot, end, (lo, hi, off) x (L + 1)], where (lo, hi) of
//    entry l < L are the slot's input rows of layer l and those of entry L the rows it emits — streaming.plan of the slot's OWN history, in a finish with its own end
//    as every frontier —, end = that end in a finish and -1 otherwise, and off = the sum of the earlier records' hi - lo at that layer: the rows of all active slots
//    lie compactly one after another in the step's scratch, so every GEMM, LayerNorm, row-statistics pass and the head run once on the sum of the rows.  A slot that
//    flushes does not make the others pay for C + L*r rows.  The records are checked (MI_ERR_ARG: frontiers that decrease, a slot past max_frames, offsets that are not
//    the prefix sums, a slot named twice).
//  * No count comes back from the device.  mi_ebf_stream_slots_table expands the records into the kernels' descriptor tables (host arithmetic); the caller uploads those
//    words once — the step's only host-to-device transfer — and hands the step both the records (host) and the table (device).
//  * Outputs are compact in record order: logits (sum n_out, logits_ld) fp32, best (sum n_out), ids (sum n_out): record i's newly emitted tokens then -1 in its n_out
//    places, n_ids (A).  The collapse carries the slot's last class across its steps.
//  * Attention is the per-slot chunk kernel everywhere, one launch per layer, with the lock-step step's ref; without a relative term at head sizes 64 / 128, where
//    that step runs the full forward's mi_attention_qkv_bf16 (one (T, Tk) per launch: no use to slots at different positions), with ref = 3, that kernel's walk.
//  * No atomics; a session's result does not depend on the other slots, on its slot index or on idle steps (every kernel here works per slot, the GEMMs per row).
#include <vector>

#include "stream_step.hpp"

namespace {

// words per entry of the kernels' tables
constexpr int CPW = 7;      // copy: src slot, src row, src modulus (0: none), dst slot, dst row, dst modulus, rows
constexpr int ATW = 4;      // attention: first query row (compact), n_q, n_k, slot
constexpr int DWW = 8;      // depthwise conv: slot, first in row, first out row (compact), p, n_new, o0, n_out, end (0x7fffffff: none)
constexpr int ROW = 3;      // rotary: first row (compact), rows, p
constexpr int COW = 3;      // collapse: slot, first frame (compact), frames
constexpr int NONE = 0x7fffffff;
// the step's table: sections of A entries each
constexpr int FRONT_COPIES = 6;                                   // history gather | feats | x_hist scatter | conv-1 rows | c1_hist scatter | feature projection -> x
constexpr int LAYER_WORDS = 3 * CPW + ATW + 2 * DWW + ROW;        // pending in | K|V append | pending out | attention | CSGU conv | merge conv | rotary
inline long table_words(int A, int L) { return (long)A * (FRONT_COPIES * CPW + (long)L * LAYER_WORDS + COW); }

// ------------------------------------------------------------------------------------------------ rows between compact buffers, caches and rings
// entry e: dst[dslot][(drow + i) % dmod][:W] = src[sslot][(srow + i) % smod][:W] for i < n; W, the row strides (ld) and slot strides (bs) in 4-byte words
__global__ __launch_bounds__(256) void copy_rows_slots_kernel(const uint32_t* __restrict__ src, long src_bs, long src_ld, uint32_t* __restrict__ dst, long dst_bs, long dst_ld,
                                                              const int* __restrict__ tab, int W) {
    const int* e = tab + (long)blockIdx.y * CPW;
    const int ss = e[0], sr = e[1], sm = e[2], ds = e[3], dr = e[4], dm = e[5], n = e[6];
    const long total = (long)n * W;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int w = (int)(i % W);
        const int r = (int)(i / W);
        int rs = sr + r, rd = dr + r;
        if (sm > 0) rs %= sm;
        if (dm > 0) rd %= dm;
        dst[ds * dst_bs + rd * dst_ld + w] = src[ss * src_bs + rs * src_ld + w];
    }
}

// nmax: the most rows of an entry (sizes the grid; host arithmetic)
int copy_rows_slots(const void* src, long src_bs, long src_ld, void* dst, long dst_bs, long dst_ld, const int* tab, int A, int nmax, int W, hipStream_t st) {
    if (A <= 0 || nmax <= 0 || W <= 0) return MI_OK;
    const long total = (long)nmax * W;
    const int gx = (int)((total + 255) / 256 < 1024 ? (total + 255) / 256 : 1024);
    hipLaunchKernelGGL(copy_rows_slots_kernel, dim3(gx, A), dim3(256), 0, st, (const uint32_t*)src, src_bs, src_ld, (uint32_t*)dst, dst_bs, dst_ld, tab, W);
    MI_CHECK_LAUNCH();
    return MI_OK;
}

// ------------------------------------------------------------------------------------------------ chunk attention, per slot
// The grid runs over the step's total queries, four per block; a wave finds its query's entry by walking the table (the entries are in compact order).  p.q / p.out
// are compact; p.k / p.v the (S, Lmax, .) cache; p.nkp / p.ntp are those of the step's largest n_k.
template <int HD>
__global__ __launch_bounds__(256) void attn_chunk_slots_kernel(AttnArgs p, const int* __restrict__ tab, int A, int total_q) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    float* sc = reinterpret_cast<float*>(smem) + (size_t)wave * (p.nkp + 2 * HD + 2 * p.ntp);
    const int h = blockIdx.y;
    const int gq = blockIdx.x * 4 + wave;
    const bool live = gq < total_q;
    const int g = live ? gq : total_q - 1;
    int e = 0;
    while (e < A - 1 && g >= tab[e * ATW] + tab[e * ATW + 1]) ++e;
    const int q0 = tab[e * ATW], n_q = tab[e * ATW + 1], n_k = tab[e * ATW + 2], slot = tab[e * ATW + 3];
    const int ia = n_k - n_q + (g - q0);       // absolute frame of the query = index of its last key
    const bf16_t* qrow = p.q + (long)g * p.ldq + h * HD;
    bf16_t* orow = live ? p.out + (long)gq * p.ldo + h * HD : nullptr;
    attn_chunk_row<HD>(p, sc, qrow, p.k + (long)slot * p.kv_bs + h * HD, p.v + (long)slot * p.kv_bs + h * HD, ia, orow, h, lane);
}

int attention_chunk_slots(AttnArgs a, const int* tab, int A, int total_q, int max_nk, int hd, hipStream_t st) {
    if (total_q <= 0) return MI_OK;
    a.nkp = (max_nk + 3) / 4 * 4;
    a.ntp = ((max_nk + 31) / 32 + 1 + 3) / 4 * 4;
    const size_t lds = (size_t)4 * (a.nkp + 2 * hd + 2 * a.ntp) * sizeof(float);
    const dim3 grid(cdiv(total_q, 4), a.H);
#define LAUNCH_ATTN(HD)                                                                                              \
    do {                                                                                                             \
        if (lds > 65536 && !ensure_dynamic_lds<HD>((const void*)attn_chunk_slots_kernel<HD>, 4 * (8192 + 2 * HD + 2 * 260) * sizeof(float))) return MI_ERR_LAUNCH; \
        hipLaunchKernelGGL(attn_chunk_slots_kernel<HD>, grid, dim3(256), lds, st, a, tab, A, total_q);                \
    } while (0)
    if (hd == 16) LAUNCH_ATTN(16);
    else if (hd == 64) LAUNCH_ATTN(64);
    else LAUNCH_ATTN(128);
#undef LAUNCH_ATTN
    MI_CHECK_LAUNCH();
    return MI_OK;
}

// ------------------------------------------------------------------------------------------------ stateful depthwise conv, per slot
// a.in / a.stats / a.mul / a.out compact; a.ring / a.ring_stats (S, ...); grid (channel tiles, A)
__global__ __launch_bounds__(256) void dwconv_stream_slots_kernel(DwsArgs a, const int* __restrict__ tab) {
    const int ct = blockIdx.x;
    const int* e = tab + (long)blockIdx.y * DWW;
    const int slot = e[0], in0 = e[1], out0 = e[2];
    const bool ln = a.mode != 1;
    DwsStream s;
    s.end = e[7]; s.p = e[3]; s.n_new = e[4]; s.o0 = e[5]; s.n_out = e[6];
    if (s.n_new == 0 && s.n_out == 0) return;
    s.nin = a.in + (long)in0 * a.ld_in;
    s.nst = ln ? a.stats + (long)in0 * 2 : nullptr;
    s.ring = a.ring + (long)slot * a.Hr * a.C;
    s.rst = ln ? a.ring_stats + ((long)slot * gridDim.x + ct) * a.Hr * 2 : nullptr;
    s.mul = a.mul ? a.mul + (long)out0 * a.ld_mul : nullptr;
    s.out = a.out + (long)out0 * a.ld_out;
    dwconv_stream_body(a, s, ct);
}

int dwconv_stream_slots(const DwsArgs& a, const int* tab, int A, hipStream_t st) {
    if (A <= 0) return MI_OK;
    hipLaunchKernelGGL(dwconv_stream_slots_kernel, dim3(cdiv(a.C, 64), A), dim3(256), 0, st, a, tab);
    MI_CHECK_LAUNCH();
    return MI_OK;
}

// ------------------------------------------------------------------------------------------------ rotary, position = the slot's p + the row's index within the slot
// out[.., h, c] = x*cos[t][c] + rot(x)*sin[t][c], rot = cat(-x[hd/2:], x[:hd/2]) (norm.hip rotary_kernel, which takes t = row % T); grid (blocks, A)
__global__ __launch_bounds__(256) void rotary_slots_kernel(const bf16_t* __restrict__ x, long ldx, bf16_t* __restrict__ out, long ldo, const float* __restrict__ cs,
                                                           const float* __restrict__ sn, const int* __restrict__ tab, int H, int hd) {
    const int* e = tab + (long)blockIdx.y * ROW;
    const int r0 = e[0], n = e[1], p = e[2];
    const int half = hd >> 1;
    const long total = (long)n * H * half;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int c = (int)(i % half);
        const int h = (int)((i / half) % H);
        const int lr = (int)(i / ((long)half * H));
        const long row = r0 + lr;
        const int t = p + lr;
        const float x1 = bf2f(x[row * ldx + h * hd + c]), x2 = bf2f(x[row * ldx + h * hd + half + c]);
        const float c1 = cs[t * hd + c], s1 = sn[t * hd + c], c2 = cs[t * hd + half + c], s2 = sn[t * hd + half + c];
        out[row * ldo + h * hd + c] = f2bf(x1 * c1 - x2 * s1);
        out[row * ldo + h * hd + half + c] = f2bf(x2 * c2 + x1 * s2);
    }
}

int rotary_slots(const bf16_t* x, long ldx, bf16_t* out, long ldo, const float* cs, const float* sn, const int* tab, int A, int nmax, int H, int hd, hipStream_t st) {
    if (A <= 0 || nmax <= 0) return MI_OK;
    const long total = (long)nmax * H * (hd / 2);
    const int gx = (int)((total + 255) / 256 < 1024 ? (total + 255) / 256 : 1024);
    hipLaunchKernelGGL(rotary_slots_kernel, dim3(gx, A), dim3(256), 0, st, x, ldx, out, ldo, cs, sn, tab, H, hd);
    MI_CHECK_LAUNCH();
    return MI_OK;
}

// ------------------------------------------------------------------------------------------------ CTC collapse with a carried class, per slot
// best / ids compact; prev (S); n_ids (A); one wave per entry
__global__ __launch_bounds__(64) void ctc_collapse_slots_kernel(const int* __restrict__ best, int blank, int* __restrict__ prev, int* __restrict__ ids, int* __restrict__ n_ids,
                                                                const int* __restrict__ tab) {
    const int* e = tab + (long)blockIdx.x * COW;
    ctc_collapse_row(best + e[1], e[2], e[2], blank, prev + e[0], ids + e[1], n_ids + blockIdx.x, threadIdx.x);
}

// ------------------------------------------------------------------------------------------------ per-slot reset
// the persistent pieces of the state: 3 in front (x_hist, c1_hist, prev), then 5 per layer (kv, csgu, csgu_stats, cat, pend) a constant stride apart
struct Pieces {
    long head_off[3], head_bytes[3];         // offset of the piece in the state; bytes of ONE slot's slice
    long layer_off[5], layer_bytes[5];       // layer 0's
    long layer_stride;
    int L;
};

Pieces pieces(const mi_ebf_config& c, const Geo& g) {
    char* const base = reinterpret_cast<char*>(4096);      // never dereferenced: carve_state hands out base + offset
    LayerState ls[64];
    const St s = carve_state(c, g, base, ls);
    auto off = [&](const void* p) { return (long)((const char*)p - base); };
    const long d = g.d, I = g.I;
    Pieces P;
    P.L = g.L;
    P.head_off[0] = off(s.x_hist); P.head_bytes[0] = 2L * g.F * 4;
    P.head_off[1] = off(s.c1_hist); P.head_bytes[1] = 2L * g.F1 * g.C1 * 2;
    P.head_off[2] = off(s.prev); P.head_bytes[2] = 4;
    P.layer_off[0] = off(ls[0].kv); P.layer_bytes[0] = (long)g.Lmax * 2 * d * 2;
    P.layer_off[1] = off(ls[0].csgu); P.layer_bytes[1] = (long)g.Hc * (I / 2) * 2;
    P.layer_off[2] = off(ls[0].csgu_stats); P.layer_bytes[2] = (long)g.ctiles * g.Hc * 2 * 4;
    P.layer_off[3] = off(ls[0].cat); P.layer_bytes[3] = 2L * g.r * 2 * d * 2;
    P.layer_off[4] = off(ls[0].pend); P.layer_bytes[4] = (long)(g.r + g.N) * d * 4;
    P.layer_stride = g.L > 1 ? off(ls[1].kv) - off(ls[0].kv) : 0;
    return P;
}

// grid (blocks, 3 + 5 L pieces): the slot's slice of a piece becomes zero, that of `prev` -1
__global__ __launch_bounds__(256) void reset_slot_kernel(char* __restrict__ state, Pieces P, int slot) {
    const int k = blockIdx.y;
    long off, bytes;
    if (k < 3) { off = P.head_off[k]; bytes = P.head_bytes[k]; }
    else { off = P.layer_off[(k - 3) % 5] + (long)((k - 3) / 5) * P.layer_stride; bytes = P.layer_bytes[(k - 3) % 5]; }
    char* dst = state + off + (long)slot * bytes;
    const uint32_t fill = k == 2 ? 0xFFFFFFFFu : 0u;
    const long i0 = (long)blockIdx.x * 256 + threadIdx.x, step = (long)gridDim.x * 256;
    if ((((uintptr_t)dst | (uintptr_t)bytes) & 15) == 0) {
        const uint4 v{fill, fill, fill, fill};
        for (long i = i0; i < bytes / 16; i += step) reinterpret_cast<uint4*>(dst)[i] = v;
    } else {
        for (long i = i0; i < bytes / 4; i += step) reinterpret_cast<uint32_t*>(dst)[i] = fill;
    }
}

// ------------------------------------------------------------------------------------------------ the step's records, checked, and their expansion
constexpr int RW(int L) { return 2 + 3 * (L + 1); }
struct Rec {
    const int* w;
    int slot() const { return w[0]; }
    int end() const { return w[1]; }
    int lo(int l) const { return w[2 + 3 * l]; }
    int hi(int l) const { return w[3 + 3 * l]; }
    int off(int l) const { return w[4 + 3 * l]; }
    int n(int l) const { return hi(l) - lo(l); }
};

// streaming.plan's invariants per slot (plan_ok, which mi_ebf_stream_step asks of its one plan), distinct slots, a finish at the slot's own end, prefix-sum offsets
int check_records(const Geo& g, const int* rec, int A) {
    if (!rec || A < 1 || A > g.B) return MI_ERR_ARG;
    const int L = g.L;
    std::vector<char> seen(g.B, 0);
    std::vector<long> sum(L + 1, 0);
    for (int i = 0; i < A; ++i) {
        const Rec e{rec + (long)i * RW(L)};
        if (e.slot() < 0 || e.slot() >= g.B || seen[e.slot()]++) return MI_ERR_ARG;
        const bool fin = e.end() >= 0;
        if (e.end() < -1 || (fin && e.end() != e.hi(0)) || !plan_ok(g, e.w + 2, 3, fin)) return MI_ERR_ARG;
        for (int l = 0; l <= L; ++l) {
            if (e.off(l) != sum[l]) return MI_ERR_ARG;
            sum[l] += e.n(l);
        }
    }
    return MI_OK;
}

void put_copy(int* w, int ss, int sr, int sm, int ds, int dr, int dm, int n) { w[0] = ss; w[1] = sr; w[2] = sm; w[3] = ds; w[4] = dr; w[5] = dm; w[6] = n; }

// section s of the front (A copy entries each), the sections of layer l, the collapse
inline long front_at(int A, int s) { return (long)A * s * CPW; }
inline long layer_at(int A, int L, int l) { return (long)A * (FRONT_COPIES * CPW + (long)l * LAYER_WORDS); }
inline long collapse_at(int A, int L) { return layer_at(A, L, L); }
enum { L_PEND_IN = 0, L_KV = CPW, L_PEND_OUT = 2 * CPW, L_ATT = 3 * CPW, L_CSGU = 3 * CPW + ATW, L_MERGE = 3 * CPW + ATW + DWW, L_ROT = 3 * CPW + ATW + 2 * DWW };   // x A

void expand(const Geo& g, const int* rec, int A, int* t) {
    const int L = g.L, C = g.C, Rp = g.r + g.N;
    for (int i = 0; i < A; ++i) {
        const Rec e{rec + (long)i * RW(L)};
        const int s = e.slot();
        put_copy(t + front_at(A, 0) + i * CPW, s, 0, 0, i, 0, 0, 2);                 // the slot's two history rows in front of its new rows (both convs)
        put_copy(t + front_at(A, 1) + i * CPW, i, 0, 0, i, 2, 0, 4 * C);             // the features behind them
        put_copy(t + front_at(A, 2) + i * CPW, i, 4 * C, 0, s, 0, 0, 2);             // the last two rows back into x_hist
        put_copy(t + front_at(A, 3) + i * CPW, i, 0, 0, i, 2, 0, 2 * C);             // conv 1's rows behind its history
        put_copy(t + front_at(A, 4) + i * CPW, i, 2 * C, 0, s, 0, 0, 2);             // the last two rows back into c1_hist
        put_copy(t + front_at(A, 5) + i * CPW, i, 0, 0, 0, e.off(0), 0, e.n(0));     // the first n0 of the C projected frames are frames of the session
        for (int l = 0; l < L; ++l) {
            int* w = t + layer_at(A, L, l);
            const int p = e.lo(l), n_in = e.n(l), o0 = e.lo(l + 1), n_o = e.n(l + 1);
            put_copy(w + (long)A * L_PEND_IN + i * CPW, 0, e.off(l), 0, s, p, Rp, n_in);
            put_copy(w + (long)A * L_KV + i * CPW, 0, e.off(l), 0, s, p, 0, n_in);
            put_copy(w + (long)A * L_PEND_OUT + i * CPW, s, o0, Rp, 0, e.off(l + 1), 0, n_o);
            int* a = w + (long)A * L_ATT + i * ATW;
            a[0] = e.off(l); a[1] = n_in; a[2] = e.hi(l); a[3] = s;
            int* c = w + (long)A * L_CSGU + i * DWW;
            c[0] = s; c[1] = e.off(l); c[2] = e.off(l); c[3] = p; c[4] = n_in; c[5] = p; c[6] = n_in; c[7] = NONE;
            int* m = w + (long)A * L_MERGE + i * DWW;
            m[0] = s; m[1] = e.off(l); m[2] = e.off(l + 1); m[3] = p; m[4] = n_in; m[5] = o0; m[6] = n_o; m[7] = e.end() >= 0 ? e.end() : NONE;
            int* ro = w + (long)A * L_ROT + i * ROW;
            ro[0] = e.off(l); ro[1] = n_in; ro[2] = p;
        }
        int* co = t + collapse_at(A, L) + i * COW;
        co[0] = s; co[1] = e.off(L); co[2] = e.n(L);
    }
}

bool slot_ok(int s, int slots) { return s >= 0 && s < slots; }

// Where the A active slots of a pool step stand (stream_step.hpp's policy): each at rows of its own — the sections of the step's table on the device —, with the host
// sums and maxima of the records, which size the launches
struct PerSlot {
    int A, L; const int* table; hipStream_t st;
    std::vector<int> tot, mostn, mostk;      // per entry: the rows of all records, the most of one; per layer: the most keys of a record that has queries
    PerSlot(const int* records, int A_, int L_, const int* table_, hipStream_t st_) : A(A_), L(L_), table(table_), st(st_), tot(L_ + 1, 0), mostn(L_ + 1, 0), mostk(L_, 0) {
        for (int i = 0; i < A; ++i)
            for (int l = 0; l <= L; ++l) {
                const Rec e{records + (long)i * RW(L)};
                tot[l] += e.n(l);
                mostn[l] = e.n(l) > mostn[l] ? e.n(l) : mostn[l];
                if (l < L && e.n(l) > 0 && e.hi(l) > mostk[l]) mostk[l] = e.hi(l);
            }
    }
    const int* front(int sec) const { return table + front_at(A, sec); }
    const int* layer(int l, int sec) const { return table + layer_at(A, L, l) + (long)A * sec; }      // sec: L_PEND_IN ..
    int streams() const { return A; }
    int rows(int l) const { return tot[l]; }
    int history_in_front(const void* hist, void* cat, int n_new, int W) const { return copy_rows_slots(hist, 2L * W, W, cat, (long)(n_new + 2) * W, W, front(0), A, 2, W, st); }
    int new_rows_behind(int conv, const void* src, void* cat, int n_new, int W) const { return copy_rows_slots(src, (long)n_new * W, W, cat, (long)(n_new + 2) * W, W, front(conv ? 3 : 1), A, n_new, W, st); }
    int history_back(int conv, const void* cat, int n_new, void* hist, int W) const { return copy_rows_slots(cat, (long)(n_new + 2) * W, W, hist, 2L * W, W, front(conv ? 4 : 2), A, 2, W, st); }
    int first_frames(const float* fp, float* x, int C, int d) const { return copy_rows_slots(fp, (long)C * d, d, x, 0, d, front(5), A, mostn[0], d, st); }
    int pending_in(int l, const float* x, float* pend, int Rp, int d) const { return copy_rows_slots(x, 0, d, pend, (long)Rp * d, d, layer(l, L_PEND_IN), A, mostn[l], d, st); }
    int pending_out(int l, const float* pend, float* res, int Rp, int d) const { return copy_rows_slots(pend, (long)Rp * d, d, res, 0, d, layer(l, L_PEND_OUT), A, mostn[l + 1], d, st); }
    int kv_append(int l, const bf16_t* kv, bf16_t* cache, int Lmax, int d) const { return copy_rows_slots(kv, 0, 3 * d / 2, cache, (long)Lmax * d, d, layer(l, L_KV), A, mostn[l], d, st); }
    int rotary(int l, const bf16_t* x, bf16_t* out, int d, const float* cs, const float* sn, int H, int hd) const { return rotary_slots(x, d, out, d, cs, sn, layer(l, L_ROT), A, mostn[l], H, hd, st); }
    int attention(int l, const AttnArgs& a, int hd) const { return attention_chunk_slots(a, layer(l, L_ATT), A, tot[l], mostk[l], hd, st); }
    int csgu_conv(int l, const DwsArgs& a) const { return dwconv_stream_slots(a, layer(l, L_CSGU), A, st); }
    int merge_conv(int l, const DwsArgs& a) const { return dwconv_stream_slots(a, layer(l, L_MERGE), A, st); }
    int collapse(const int* best, int blank, int* prev, int* ids, int* n_ids) const {
        hipLaunchKernelGGL(ctc_collapse_slots_kernel, dim3(A), dim3(64), 0, st, best, blank, prev, ids, n_ids, table + collapse_at(A, L));
        MI_CHECK_LAUNCH();
        return MI_OK;
    }
};

}  // namespace

// ---- the per-slot kernels as entries of their own.  Each takes its table twice: tab_host is checked, tab_dev (the same words on the device) is what the kernel reads.

// entry e of the table (7 ints): src slot, src row, src modulus (0: no wrap), dst slot, dst row, dst modulus, n rows.  src (src_slots, src_rows, src_ld) and dst likewise,
// W 4-byte words per row copied, strides in 4-byte words; a row range must lie inside its slot (rows < the modulus when it wraps, modulus <= rows).
extern "C" int mi_copy_rows_slots(const void* src, long src_bs, long src_ld, int src_slots, int src_rows, void* dst, long dst_bs, long dst_ld, int dst_slots, int dst_rows,
                                  const int* tab_host, const int* tab_dev, int A, int W, hipStream_t stream) {
    MI_ENTER();
    if (!src || !dst || !tab_host || !tab_dev || A <= 0 || W <= 0 || W > src_ld || W > dst_ld || src_slots <= 0 || dst_slots <= 0) return MI_ERR_ARG;
    int nmax = 0;
    for (int i = 0; i < A; ++i) {
        const int* e = tab_host + (long)i * CPW;
        if (!slot_ok(e[0], src_slots) || !slot_ok(e[3], dst_slots) || e[1] < 0 || e[4] < 0 || e[2] < 0 || e[5] < 0 || e[6] < 0) return MI_ERR_ARG;
        if (e[2] > src_rows || e[5] > dst_rows || (e[2] == 0 && (long)e[1] + e[6] > src_rows) || (e[5] == 0 && (long)e[4] + e[6] > dst_rows)) return MI_ERR_ARG;
        if ((e[2] > 0 && e[6] > e[2]) || (e[5] > 0 && e[6] > e[5])) return MI_ERR_ARG;      // a wrapped range that laps itself
        nmax = e[6] > nmax ? e[6] : nmax;
    }
    return copy_rows_slots(src, src_bs, src_ld, dst, dst_bs, dst_ld, tab_dev, A, nmax, W, stream);
}

// mi_attention_chunk_bf16 per slot.  entry e (4 ints): first query row, n_q, n_k, slot; q / out (sum n_q, .) compact, the first rows the prefix sums of n_q; k / v the
// (slots, kv_rows, .) cache; a slot's n_k >= n_q keys, its new rows' own last.  The LDS is sized by the largest n_k.
extern "C" int mi_attention_chunk_slots_bf16(const void* q, long ldq, const void* k, long ldk, const void* v, long ldv, long kv_bstride, int slots, int kv_rows, const void* pos,
                                             long ldp, const float* bias_u, const float* bias_v, void* out, long ldo, const int* tab_host, const int* tab_dev, int A, int H,
                                             int hd, float scale, int ref, hipStream_t stream) {
    MI_ENTER();
    if (!q || !k || !v || !out || !tab_host || !tab_dev || A <= 0 || H <= 0 || ldk != ldv || ref < 0 || ref > 3 || slots <= 0 || kv_rows <= 0) return MI_ERR_ARG;
    if ((pos != nullptr) != (bias_u != nullptr) || (pos != nullptr) != (bias_v != nullptr)) return MI_ERR_ARG;
    if ((ldk % 8) || (kv_bstride % 8) || (pos && (ldp % 8)) || ((uintptr_t)k & 15) || ((uintptr_t)v & 15) || ((uintptr_t)pos & 15)) return MI_ERR_ARG;
    if ((hd != 16 && hd != 64 && hd != 128) || H > 65535) return MI_ERR_UNSUPPORTED;
    int total = 0, max_nk = 0;
    for (int i = 0; i < A; ++i) {
        const int* e = tab_host + (long)i * ATW;
        if (e[0] != total || e[1] < 0 || e[2] < e[1] || e[2] > kv_rows || !slot_ok(e[3], slots)) return MI_ERR_ARG;
        if (e[2] > 8192) return MI_ERR_UNSUPPORTED;
        total += e[1];
        if (e[1] > 0 && e[2] > max_nk) max_nk = e[2];
    }
    AttnArgs a{(const bf16_t*)q, ldq, (const bf16_t*)k, (const bf16_t*)v, ldk, kv_bstride, (const bf16_t*)pos, ldp, bias_u, bias_v, (bf16_t*)out, ldo, 0, 0, H, 0, 0, ref, scale};
    return attention_chunk_slots(a, tab_dev, A, total, max_nk, hd, stream);
}

// mi_dwconv_stream_bf16 per slot.  entry e (8 ints): slot, first in row, first out row, p, n_new, o0, n_out, end (0x7fffffff: none); in / stats / mul / out compact, ring
// (slots, Hr, C) and ring_stats (slots, ceil(C/64), Hr, 2).  The windows are checked per entry as mi_dwconv_stream_bf16 checks its one.
extern "C" int mi_dwconv_stream_slots_bf16(const void* in, long ld_in, const void* mul, long ld_mul, const float* stats, const float* gamma, const float* beta, const float* w,
                                           const float* bias, void* ring, float* ring_stats, int slots, void* out, long ld_out, const int* tab_host, const int* tab_dev, int A,
                                           int C, int K, int dil, int left, int Hr, int mode, int act, hipStream_t stream) {
    MI_ENTER();
    if (!tab_host || !tab_dev || A <= 0 || A > 65535 || slots <= 0 || C <= 0 || K <= 0 || dil <= 0 || left < 0 || Hr < 0 || mode < 0 || mode > 2 || act < 0 || act > 3) return MI_ERR_ARG;
    if (!w || !in || !out || (Hr > 0 && !ring)) return MI_ERR_ARG;
    if (mode != 1 && (!gamma || !beta || !stats || (Hr > 0 && !ring_stats))) return MI_ERR_ARG;
    if (mode == 0 && !mul) return MI_ERR_ARG;
    for (int i = 0; i < A; ++i) {
        const int* e = tab_host + (long)i * DWW;
        const int p = e[3], n_new = e[4], o0 = e[5], n_out = e[6];
        const bool has_end = e[7] != NONE;
        if (!slot_ok(e[0], slots) || e[1] < 0 || e[2] < 0 || p < 0 || n_new < 0 || o0 < 0 || n_out < 0 || e[7] < 0) return MI_ERR_ARG;
        if (n_out > 0 && (o0 - left < p - Hr || (long)o0 + n_out - 1 - left + (long)(K - 1) * dil > (long)p + n_new - 1 + (has_end ? left : 0))) return MI_ERR_ARG;
    }
    DwsArgs a{(const bf16_t*)in, ld_in, (const bf16_t*)mul, ld_mul, stats, gamma, beta, w, bias, (bf16_t*)ring, ring_stats, nullptr, (bf16_t*)out, ld_out,
              slots, C, K, dil, left, Hr, 0, 0, 0, 0, mode, act};
    return dwconv_stream_slots(a, tab_dev, A, stream);
}

// mi_rotary_bf16 with the position of a row = its slot's p + its index within the slot.  entry e (3 ints): first row, rows, p; cos_t / sin_t (tmax, hd) fp32.
extern "C" int mi_rotary_slots_bf16(const void* x, long ldx, void* out, long ldo, const float* cos_t, const float* sin_t, int tmax, const int* tab_host, const int* tab_dev,
                                    int A, int H, int hd, hipStream_t stream) {
    MI_ENTER();
    if (!x || !out || !cos_t || !sin_t || !tab_host || !tab_dev || A <= 0 || A > 65535 || H <= 0 || hd <= 0 || (hd & 1)) return MI_ERR_ARG;
    int nmax = 0;
    for (int i = 0; i < A; ++i) {
        const int* e = tab_host + (long)i * ROW;
        if (e[0] < 0 || e[1] < 0 || e[2] < 0 || (long)e[2] + e[1] > tmax) return MI_ERR_ARG;
        nmax = e[1] > nmax ? e[1] : nmax;
    }
    return rotary_slots((const bf16_t*)x, ldx, (bf16_t*)out, ldo, cos_t, sin_t, tab_dev, A, nmax, H, hd, stream);
}

// mi_ctc_collapse_stream per slot.  entry e (3 ints): slot, first frame, frames; best / ids compact (ids: the entry's newly emitted tokens then -1 in its `frames` places),
// prev (slots) the carried classes, n_ids (A).  An entry of zero frames leaves its slot's carried class alone.  ids must not alias best.
extern "C" int mi_ctc_collapse_slots(const int* best, int blank, int* prev, int slots, int* ids, int* n_ids, const int* tab_host, const int* tab_dev, int A, hipStream_t stream) {
    MI_ENTER();
    if (!best || !prev || !ids || !n_ids || !tab_host || !tab_dev || A <= 0 || slots <= 0 || ids == best) return MI_ERR_ARG;
    for (int i = 0; i < A; ++i) {
        const int* e = tab_host + (long)i * COW;
        if (!slot_ok(e[0], slots) || e[1] < 0 || e[2] < 0) return MI_ERR_ARG;
        for (int j = 0; j < i; ++j)
            if (tab_host[(long)j * COW] == e[0]) return MI_ERR_ARG;      // two waves on one carried class
    }
    hipLaunchKernelGGL(ctc_collapse_slots_kernel, dim3(A), dim3(64), 0, stream, best, blank, prev, ids, n_ids, tab_dev);
    MI_CHECK_LAUNCH();
    return MI_OK;
}

// ---- the pool's driver

// the persistent pieces of a state (cfg.B = slots): out = (offset, bytes of one slot's slice) pairs, 3 + 5 L of them — x_hist, c1_hist, prev, then per layer kv, csgu,
// csgu_stats, cat, pend; slot s of a piece is bytes [offset + s * slice, offset + (s + 1) * slice).  -> the number of pieces (out may be null), < 0: refused.  Host only.
extern "C" int mi_ebf_stream_slot_pieces(const mi_ebf_config* cfg, int chunk_frames, int max_frames, long* out, int capacity) {
    Geo g;
    if (!geometry(cfg, chunk_frames, max_frames, g)) return MI_ERR_ARG;
    if (!supported(*cfg, g)) return MI_ERR_UNSUPPORTED;
    const int n = 3 + 5 * g.L;
    if (!out) return n;
    if (capacity < n) return MI_ERR_ARG;
    const Pieces P = pieces(*cfg, g);
    for (int k = 0; k < n; ++k) {
        out[2 * k] = k < 3 ? P.head_off[k] : P.layer_off[(k - 3) % 5] + (long)((k - 3) / 5) * P.layer_stride;
        out[2 * k + 1] = k < 3 ? P.head_bytes[k] : P.layer_bytes[(k - 3) % 5];
    }
    return n;
}

// slot `slot` back to a stream start: its slice of every persistent piece zero, its carried class -1.  One launch on `stream`; the other slots are not touched.
extern "C" int mi_ebf_stream_reset_slot(const mi_ebf_config* cfg, int chunk_frames, int max_frames, void* state, size_t state_bytes, int slot, hipStream_t stream) {
    MI_ENTER();
    Geo g;
    if (!geometry(cfg, chunk_frames, max_frames, g) || !state || slot < 0 || slot >= g.B) return MI_ERR_ARG;
    if (!supported(*cfg, g)) return MI_ERR_UNSUPPORTED;
    if (carve_state(*cfg, g, nullptr, nullptr).bytes > state_bytes) return MI_ERR_ARG;
    const Pieces P = pieces(*cfg, g);
    long most = 0;
    for (int k = 0; k < 5; ++k) most = P.layer_bytes[k] > most ? P.layer_bytes[k] : most;
    const int gx = (int)(most / 16 / 256 + 1 < 256 ? most / 16 / 256 + 1 : 256);
    hipLaunchKernelGGL(reset_slot_kernel, dim3(gx, 3 + 5 * g.L), dim3(256), 0, stream, (char*)state, P, slot);
    MI_CHECK_LAUNCH();
    return MI_OK;
}

// the records of a step (header above; A x (2 + 3 (L + 1)) ints, HOST) expanded into the words the step's kernels read: -> their count (table null: only counted), or
// MI_ERR_ARG for records that fail the checks / a capacity too small.  Host arithmetic only.
extern "C" int mi_ebf_stream_slots_table(const mi_ebf_config* cfg, int chunk_frames, int max_frames, const int* records, int A, int* table, int capacity) {
    Geo g;
    if (!geometry(cfg, chunk_frames, max_frames, g)) return MI_ERR_ARG;
    if (!supported(*cfg, g)) return MI_ERR_UNSUPPORTED;
    RUN(check_records(g, records, A));
    const long words = table_words(A, g.L);
    if (words > 0x7fffffffL) return MI_ERR_UNSUPPORTED;
    if (!table) return (int)words;
    if (capacity < words) return MI_ERR_ARG;
    expand(g, records, A, table);
    return (int)words;
}

// One step of the pool (stream_step.hpp).  cfg.B = slots; feats (A, 4*C, F) fp32, record i's chunk (a tail zero-padded); records (HOST) and table (DEVICE: mi_ebf_stream_slots_table's
// words for these records, table_len >= their count) as the header says; pos_table as mi_ebf_stream_step's.  Outputs compact in record order (header).  sum n_out = 0:
// nothing is written.
extern "C" int mi_ebf_stream_step_slots(const mi_ebf_config* cfg, const void* const* weights, int chunk_frames, int max_frames, const void* pos_table, void* state,
                                        size_t state_bytes, const float* feats, const int* records, int A, const int* table, int table_len, float* logits,
                                        int* best, int* ids, int* n_ids, hipStream_t st) {
    MI_ENTER();
    Geo g;
    if (!geometry(cfg, chunk_frames, max_frames, g) || !state || !weights || !feats || !table) return MI_ERR_ARG;
    const mi_ebf_config& c = *cfg;
    if (!supported(c, g)) return MI_ERR_UNSUPPORTED;
    if (!c.logits_f32 || (c.pos_type == 2 && !pos_table) || c.pos_type < 0 || c.pos_type > 2) return MI_ERR_ARG;
    RUN(check_records(g, records, A));
    if (table_len < table_words(A, g.L)) return MI_ERR_ARG;
    const PerSlot at(records, A, g.L, table, st);
    const Step<PerSlot> step(c, g, state, weights, at, pos_table, st);
    if (step.s.bytes > state_bytes) return MI_ERR_ARG;
    return step.run(feats, logits, best, ids, n_ids);
}
