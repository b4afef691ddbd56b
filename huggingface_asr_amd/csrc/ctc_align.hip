// CTC forced alignment on gfx950: the best (Viterbi) path of a given transcript through the CTC head's log-probabilities, the frames each token occupies and
// the log-probability each token collects there.  The alpha recursion of ctc.hip in the max semiring, plus backpointers and a backtrace; one block per
// utterance, one launch for the batch, no host synchronisation, no atomics: bit-identical run to run.
//
// SEMANTICS (exact: tests/ctc_align_ref.py `viterbi32` restates them in numpy float32 and is compared bit for bit)
//   target l_0 .. l_{n-1} = the non-negative entries of the utterance's label row, in order; n_b = in_len clamped to [0, T];
//   lp[t][c]   = fp32( float(x[t][c]) - lse[t] )                                            (one subtraction; the only thing ever read from the logits)
//   states     s = 0 .. 2n, blank at even s, label l_{s>>1} at odd s                        (the "extended" sequence)
//   delta[0][0] = lp[0][blank], delta[0][1] = lp[0][l_0], every other state -inf
//   delta[t][s] = fp32( max( delta[t-1][s], delta[t-1][s-1], delta[t-1][s-2] if s is odd, s >= 3 and l_{s>>1} != l_{(s>>1)-1} ) + lp[t][class of s] )
//   among equal maxima the first in the order stay, s-1, s-2 wins (a candidate replaces the current best only when it is strictly greater)
//   the path ends in the larger of states 2n and 2n-1, in 2n when they are equal; score = that delta[n_b-1][.]; the backpointers give the states of the
//   earlier frames.  path[t] = the class of frame t's state.  Token u emits on the frames whose state is 2u+1 — consecutive ones, [start[u], end[u]) —
//   and token_lp[u] = fp32 sum, starting from 0.0f and in time order, of lp[t][l_u] over them.
//   There is no multiplication anywhere, so nothing can be contracted into an fma: both kernel forms below execute the same subtraction, the same
//   comparisons and the same addition per cell, and give the same bits.
//   n = 0: every frame is blank.  n_b = 0 and n = 0: score 0, nothing else to say.
//   INFEASIBLE utterances are no error: n_b < n + (number of u with l_u == l_{u-1}), n_b = 0 with n > 0, a label >= V1 or == blank (never used as a
//   column), or a best score that is not above -inf.  They get score -inf, path -1 on every frame, start / end -1 and token_lp 0 on every entry.
//   Past the lengths: path[t >= n_b] = -1, start / end [u >= n] = -1, token_lp[u >= n] = 0.  tgt_len = n always.
//   NaN logits or lse: the result is unspecified; the kernel terminates and stays in bounds (a NaN never wins a comparison, states only move down and
//   are clamped at 0).
//
// BACKPOINTERS: 2 bits per (t, s) — 0 stay, 1 from s-1, 2 from s-2 — 16 to a word: word [t >> 3][p] holds the pair of states (2p, 2p+1) over eight
// frames, frame t's four bits at (t & 7) * 4 (blank state low).  The thread that owns a pair of states for the whole utterance therefore builds its
// words in a register, with no cross-lane traffic, and stores one every eight frames: to LDS when ceil(T / 8) * PS words fit beside the kernel's
// other LDS (PS = pairs per row: 64 in the wave form, 256 * ceil((U + 1) / 256) in the block form; mi_ctc_align_workspace_bytes then returns 0),
// otherwise to `workspace` with ordinary vector stores.  Which of the two is a template parameter of the kernel: a pointer chosen at run time becomes a
// generic one, and its flat operations wait on both memory counters inside the serial loops.
//
// TWO FORMS of the recursion, chosen on the host from U (the label row's width):
//   wave form, U <= 63 (at most 127 states): the block gathers lp[t][l_p] (64 label columns) and lp[t][blank] for up to 256 frames into LDS in
//     parallel (65 values per frame: every even state shares the blank's) — the only traffic on the logits — then ONE wave runs the recursion with the states (2 lane, 2 lane + 1) in registers.  State 2 lane - 1
//     comes from one whole-wave DPP shift; state 2 lane is the lane's own: a frame costs two LDS reads (prefetched), one DPP move, three compares and
//     two adds, no barrier and no memory round trip.
//   block form, 64 <= U <= 1023: 256 threads, thread i owns the pairs i, i + 256, ...; delta lives in LDS, double-buffered, ONE barrier per frame.  Each
//     thread loads its own columns for eight frames ahead into registers (the next eight are in flight while these eight are consumed).
// BACKTRACE (one wave): the word a frame needs is selected with v_readlane from a 64-pair window (lane j holds the word of pair top - j) that was loaded
// four 8-frame rows ahead — the state moves down by at most two per frame, so a window loaded 40 frames early still covers it.  The serial path holds a
// readlane, a shift, a mask and a subtraction per frame; no load depends on the previous frame's decision.  It leaves the STATE of every frame in
// `path` (collected in a register, lane t & 63, and stored 64 frames at a time: no store sits between a window's load and its use); the block then derives start / end (a thread per frame, from the states of its neighbours), rewrites the states as classes, and sums
// token_lp (a thread per token over its own frames, in time order, sixteen loads in flight: the one place single values of the logits are read a second
// time, and a serial tail as long as the longest token's span — DESIGN.md has its measured cost).
//
// BOUNDS (MI_ERR_UNSUPPORTED beyond): U <= 1023, T <= 2^20.
#include "common.hpp"

namespace {

constexpr int ALIGN_LDS_BUDGET = 144 * 1024;      // of the CU's 160 KiB
constexpr int ALIGN_MAX_U = 1023, ALIGN_MAX_T = 1 << 20, ALIGN_WAVE_U = 63, ALIGN_WAVE_TCH = 256;

struct AlignPlan {
    int wave;            // 1: wave form
    int ps;              // pairs per backpointer row
    int tch;             // wave form: frames gathered per chunk (a multiple of 8)
    int nblk;            // backpointer rows: ceil(T / 8)
    size_t work_bytes;   // lp staging (wave) / delta double buffer (block); the tail's start / end arrays alias it
    size_t bp_bytes;     // per utterance
    int bp_in_lds;
    size_t lds;
};
inline AlignPlan align_plan(int T, int U) {
    AlignPlan p;
    p.wave = U <= ALIGN_WAVE_U;
    p.ps = p.wave ? 64 : 256 * ((U + 1 + 255) / 256);
    p.nblk = (T + 7) / 8;
    p.tch = p.nblk * 8 < ALIGN_WAVE_TCH ? p.nblk * 8 : ALIGN_WAVE_TCH;
    p.work_bytes = p.wave ? ((size_t)p.tch * 65 * sizeof(float) + 15) / 16 * 16 : (size_t)4 * p.ps * sizeof(float);
    p.bp_bytes = (size_t)p.nblk * p.ps * sizeof(unsigned);
    const size_t fixed = 8 * sizeof(int) + (size_t)p.ps * sizeof(int) + p.work_bytes;
    p.bp_in_lds = fixed + p.bp_bytes <= (size_t)ALIGN_LDS_BUDGET;
    p.lds = fixed + (p.bp_in_lds ? p.bp_bytes : 0);
    return p;
}

__device__ __forceinline__ float align_shr1(float v, float fill) {   // lane i <- lane i-1, lane 0 <- fill
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(fill), __float_as_int(v), 0x138 /*wave_shr:1*/, 0xF, 0xF, false));
}

// one cell pair: the new blank state 2p and label state 2p+1 from the previous frame's (2p-1, 2p, 2p+1); returns the pair's four backpointer bits
__device__ __forceinline__ unsigned align_cell(float pm, float& d0, float& d1, bool skip, bool vb, bool vl, float lb, float ll) {
    float bb = d0; unsigned cb = 0;
    if (pm > bb) { bb = pm; cb = 1; }
    float bl = d1; unsigned cl = 0;
    if (d0 > bl) { bl = d0; cl = 1; }
    if (skip && pm > bl) { bl = pm; cl = 2; }
    d0 = vb ? bb + lb : -INFINITY;
    d1 = vl ? bl + ll : -INFINITY;
    return cb | (cl << 2);
}

struct AlignArgs {
    const void* logits; long ld_b, ld_t;
    const float* lse; int T;
    const long* labels; int U;
    const int* in_len; int blank, V1;
    unsigned* ws; long ws_words;                 // per-utterance stride of the workspace backpointers (words); ws null: they live in LDS
    int ps, tch;
    int* path; float* score; int* tgt_len; int* start; int* end; float* token_lp;
};

// hdr: [0] n, [1] infeasible, [2] final state, [3] score bits
template <typename T, bool WAVE, bool INWS>
__global__ __launch_bounds__(256) void ctc_align_kernel(const AlignArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    int* hdr = reinterpret_cast<int*>(smem);                                   // [8]
    int* lab = hdr + 8;                                                        // [ps]: the target's labels
    char* work = reinterpret_cast<char*>(lab + a.ps);
    const size_t work_bytes = WAVE ? ((size_t)a.tch * 65 * sizeof(float) + 15) / 16 * 16 : (size_t)4 * a.ps * sizeof(float);
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // backpointers [nblk][ps]: in the workspace (INWS) or in LDS behind the work area — a template parameter, so that each form has its own load / store
    // instructions (a pointer chosen at run time becomes a generic one: flat operations, and their waits on both counters, in the serial loops)
    unsigned* gbp = INWS ? a.ws + (long)b * a.ws_words : nullptr;
    unsigned* lbp = reinterpret_cast<unsigned*>(work + work_bytes);
    auto bp_store = [&](long i, unsigned v) { if (INWS) gbp[i] = v; else lbp[i] = v; };
    const int U = a.U, Tmax = a.T, blank = a.blank, ps = a.ps;
    const int nb = min(max(a.in_len[b], 0), Tmax);
    const T* lg = reinterpret_cast<const T*>(a.logits) + (long)b * a.ld_b;
    const float* ls = a.lse + (long)b * Tmax;
    const long* lrow = a.labels + (long)b * U;
    int* path = a.path + (long)b * Tmax;
    const bool spans = a.start != nullptr;
    int* start = spans ? a.start + (long)b * U : nullptr;
    int* end = spans ? a.end + (long)b * U : nullptr;
    float* tlp = spans ? a.token_lp + (long)b * U : nullptr;

    // ---- the target: compaction of the non-negative labels (wave 0, 64 at a time), then the count of adjacent equal ones
    if (wave == 0) {
        int n = 0, bad = 0;
        for (int u0 = 0; u0 < U; u0 += 64) {
            const int u = u0 + lane;
            const long v = u < U ? lrow[u] : -1;
            const bool keep = v >= 0;
            const unsigned long long m = __ballot(keep);
            if (keep) lab[n + __popcll(m & ((1ull << lane) - 1ull))] = (v >= a.V1 || v == blank) ? -1 : (int)v;
            bad |= __ballot(keep && (v >= a.V1 || v == blank)) != 0ull;
            n += __popcll(m);
        }
        if (lane == 0) { hdr[0] = n; hdr[1] = bad; }
    }
    __syncthreads();
    const int n = hdr[0];
    if (wave == 0) {
        int rep = 0;
        for (int p0 = 1; p0 < n; p0 += 64) {
            const int p = p0 + lane;
            rep += __popcll(__ballot(p < n && lab[p] == lab[p - 1]));
        }
        if (lane == 0) hdr[1] = (hdr[1] || nb < n + rep || (nb == 0 && n > 0)) ? 1 : 0;
    }
    __syncthreads();
    if (tid == 0) a.tgt_len[b] = n;
    // the documented fill past the lengths
    for (int t = nb + tid; t < Tmax; t += 256) path[t] = -1;
    if (spans)
        for (int u = n + tid; u < U; u += 256) { start[u] = -1; end[u] = -1; tlp[u] = 0.f; }
    bool infeasible = hdr[1] != 0;
    if (!infeasible && nb == 0) {                  // n = 0 as well: the empty path
        if (tid == 0) a.score[b] = 0.f;
        return;
    }

    if (!infeasible) {
        // ---- forward: delta and backpointers
        if (WAVE) {
            float* lpl = reinterpret_cast<float*>(work);                       // [tch][64]: lp of label p at chunk frame tt
            float* lpb = lpl + (size_t)a.tch * 64;                             // [tch]: lp of the blank
            const bool vb = lane <= n, vl = lane < n;
            const bool skip = lane >= 1 && vl && lab[lane] != lab[lane - 1];
            float d0 = -INFINITY, d1 = -INFINITY;
            unsigned acc = 0;
            for (int tc = 0; tc < nb; tc += a.tch) {
                const int nt = min(a.tch, nb - tc);
                {   // gather: a thread keeps its label column and walks the chunk's frames, 16 loads in flight (ctc.hip's alpha kernel)
                    constexpr int UN = 16;
                    const int p = tid & 63, tsub = tid >> 6;
                    const long col = p < n ? lab[p] : blank;
                    for (int t = tsub; t < nt; t += 4 * UN) {
                        float v[UN], l[UN];
#pragma unroll
                        for (int u = 0; u < UN; ++u) {
                            const int tt = min(t + 4 * u, nt - 1);             // clamped: branch-free loads
                            v[u] = (float)lg[(long)(tc + tt) * a.ld_t + col];
                            l[u] = ls[tc + tt];
                        }
#pragma unroll
                        for (int u = 0; u < UN; ++u)                           // unconditional: a clamped frame is written again with its own value (a condition here
                            lpl[min(t + 4 * u, nt - 1) * 64 + p] = v[u] - l[u];   // makes the compiler sink the loads into branches, one round trip each)
                    }
                    for (int tt = tid; tt < nt; tt += 256) lpb[tt] = (float)lg[(long)(tc + tt) * a.ld_t + blank] - ls[tc + tt];
                }
                __syncthreads();
                if (wave == 0) {
                    float lln = lpl[lane], lbn = lpb[0];
                    for (int t8 = 0; t8 < nt; t8 += 8) {                       // a backpointer row at a time (chunks start at multiples of 8): static bit positions
#pragma unroll
                        for (int j = 0; j < 8; ++j) {
                            const int tt = t8 + j;
                            if (tt < nt) {                                     // uniform
                                const float ll = lln, lb = lbn;
                                const int tn = min(tt + 1, nt - 1);
                                lln = lpl[tn * 64 + lane]; lbn = lpb[tn];      // the next frame's values: their LDS latency leaves the serial chain
                                if (tc + tt == 0) {
                                    d0 = lane == 0 ? lb : -INFINITY;
                                    d1 = (lane == 0 && vl) ? ll : -INFINITY;
                                } else {
                                    const float pm = align_shr1(d1, -INFINITY);    // delta[2 lane - 1]
                                    acc |= align_cell(pm, d0, d1, skip, vb, vl, lb, ll) << (j * 4);
                                }
                            }
                        }
                        bp_store((long)((tc + t8) >> 3) * 64 + lane, acc);
                        acc = 0;
                    }
                }
                __syncthreads();
            }
            if (wave == 0) {
                const float vhi = __shfl(d0, n, 64);
                const float vlo = n >= 1 ? __shfl(d1, n - 1, 64) : -INFINITY;
                if (lane == 0) {
                    const bool lo = vlo > vhi;
                    hdr[2] = lo ? 2 * n - 1 : 2 * n;
                    hdr[3] = __float_as_int(lo ? vlo : vhi);
                }
            }
        } else {
            float* dl = reinterpret_cast<float*>(work);                        // [2][2 ps]: delta of frame t in half t & 1
            const int kp = ps >> 8;                                            // pairs per thread, 1..4
            long col[4]; bool skip[4], vb[4], vl[4]; unsigned acc[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int p = tid + 256 * k;
                vb[k] = k < kp && p <= n; vl[k] = k < kp && p < n;
                col[k] = vl[k] ? lab[p] : blank;
                skip[k] = vl[k] && p >= 1 && lab[p] != lab[p - 1];
                acc[k] = 0;
            }
            float xn[4][8] = {}, bn[8], ln[8];                                 // the next eight frames' logits (own label columns, blank) and lse
            auto load8 = [&](int c) {
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const long t = min(8 * c + j, nb - 1);
                    const T* row = lg + t * a.ld_t;
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        if (k < kp) xn[k][j] = (float)row[col[k]];
                    bn[j] = (float)row[blank];
                    ln[j] = ls[t];
                }
            };
            const int nchunk = (nb + 7) >> 3;
            load8(0);
            for (int c = 0; c < nchunk; ++c) {
                float xc[4][8], bc[8], lc[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
#pragma unroll
                    for (int k = 0; k < 4; ++k) xc[k][j] = xn[k][j];
                    bc[j] = bn[j]; lc[j] = ln[j];
                }
                if (c + 1 < nchunk) load8(c + 1);
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int t = 8 * c + j;
                    if (t < nb) {                                              // uniform
                        const float* A = dl + ((j & 1) ^ 1) * 2 * ps;          // (8 c is even: the frame's parity is j's)
                        float* Bn = dl + (j & 1) * 2 * ps;
                        const float lb = bc[j] - lc[j];
#pragma unroll
                        for (int k = 0; k < 4; ++k) {
                            if (k < kp) {
                                const int p = tid + 256 * k;
                                const float ll = xc[k][j] - lc[j];
                                float d0, d1;
                                if (t == 0) {
                                    d0 = p == 0 ? lb : -INFINITY;
                                    d1 = (p == 0 && vl[k]) ? ll : -INFINITY;
                                } else {
                                    const float pm = p >= 1 ? A[2 * p - 1] : -INFINITY;
                                    d0 = A[2 * p]; d1 = A[2 * p + 1];
                                    acc[k] |= align_cell(pm, d0, d1, skip[k], vb[k], vl[k], lb, ll) << (j * 4);
                                }
                                Bn[2 * p] = d0; Bn[2 * p + 1] = d1;
                            }
                        }
                        __syncthreads();                                       // the frame's one barrier
                    }
                }
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (k < kp) { bp_store((long)c * ps + tid + 256 * k, acc[k]); acc[k] = 0; }
            }
            if (tid == 0) {
                const float* A = dl + ((nb - 1) & 1) * 2 * ps;
                const float vhi = A[2 * n], vlo = n >= 1 ? A[2 * n - 1] : -INFINITY;
                const bool lo = vlo > vhi;
                hdr[2] = lo ? 2 * n - 1 : 2 * n;
                hdr[3] = __float_as_int(lo ? vlo : vhi);
            }
        }
        __syncthreads();
        const float sc = __int_as_float(hdr[3]);
        infeasible = !(sc > -INFINITY);
        if (!infeasible && tid == 0) a.score[b] = sc;
    }
    if (infeasible) {
        if (tid == 0) a.score[b] = -INFINITY;
        for (int t = tid; t < nb; t += 256) path[t] = -1;
        if (spans)
            for (int u = tid; u < n; u += 256) { start[u] = -1; end[u] = -1; tlp[u] = 0.f; }
        return;
    }

    // ---- backtrace: wave 0 leaves the state of every frame in path
    int* sst = reinterpret_cast<int*>(work);                                   // [ps] start / [ps] end of every token: they alias the forward's staging, which is done with
    int* sen = sst + ps;
    for (int u = tid; u < n; u += 256) { sst[u] = 0; sen[u] = 0; }             // (a path out of NaNs may skip a token: its span stays empty and in bounds)
    if (wave == 0) {
        int s = __builtin_amdgcn_readfirstlane(hdr[2]);
        int kb = (nb - 1) >> 3;
        unsigned w0 = 0, w1 = 0, w2 = 0, w3 = 0;
        int p0 = 0, p1 = 0, p2 = 0, p3 = 0;
        auto window = [&](unsigned& w, int& pt, int row) {                     // lane j <- the word of pair (s >> 1) - j of backpointer row `row`
            pt = s >> 1;
            if (row >= 0) {
                const long i = (long)row * ps + max(pt - lane, 0);
                if (INWS) w = gbp[i]; else w = lbp[i];
            }
        };
        int sreg = 0;                                                          // lane j: the state of frame (t & ~63) + j, stored 64 frames at a time
        auto walk = [&](unsigned w, int pt, int row) {
            for (int t = min(row * 8 + 7, nb - 1); t >= row * 8; --t) {
                sreg = lane == (t & 63) ? s : sreg;
                const unsigned word = (unsigned)__builtin_amdgcn_readlane((int)w, (pt - (s >> 1)) & 63);
                const int code = (int)((word >> ((t & 7) * 4 + (s & 1) * 2)) & 3u);          // frame 0's bits are 0
                s = max(s - code, 0);
            }
            if ((row & 7) == 0 && row * 8 + lane < nb) path[row * 8 + lane] = sreg;
        };
        window(w0, p0, kb); window(w1, p1, kb - 1); window(w2, p2, kb - 2); window(w3, p3, kb - 3);
        while (kb >= 0) {
            walk(w0, p0, kb); window(w0, p0, kb - 4); if (--kb < 0) break;
            walk(w1, p1, kb); window(w1, p1, kb - 4); if (--kb < 0) break;
            walk(w2, p2, kb); window(w2, p2, kb - 4); if (--kb < 0) break;
            walk(w3, p3, kb); window(w3, p3, kb - 4); --kb;
        }
    }
    __syncthreads();

    // ---- spans from the states (a thread per frame), then classes into path and token_lp (a thread per token)
    for (int t = tid; spans && t < nb; t += 256) {
        const int s = path[t];
        if (s & 1) {
            if (t == 0 || path[t - 1] != s) sst[s >> 1] = t;
            if (t == nb - 1 || path[t + 1] != s) sen[s >> 1] = t + 1;
        }
    }
    __syncthreads();
    for (int t = tid; t < nb; t += 256) {
        const int s = path[t];
        path[t] = (s & 1) ? lab[s >> 1] : blank;
    }
    if (spans)
        for (int u = tid; u < n; u += 256) {
            const int t0 = sst[u], t1 = sen[u];
            const long col = lab[u];
            float acc = 0.f;
            for (int t = t0; t < t1; t += 16) {                                // sixteen loads in flight (clamped, so branch-free), added in time order
                float v[16], l[16];
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    const int tt = min(t + j, t1 - 1);
                    v[j] = (float)lg[(long)tt * a.ld_t + col];
                    l[j] = ls[tt];
                }
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    const float sum = acc + (v[j] - l[j]);
                    acc = t + j < t1 ? sum : acc;
                }
            }
            start[u] = t0; end[u] = t1; tlp[u] = acc;
        }
}

}  // namespace

// bytes of `workspace` mi_ctc_align needs for (B, T, U): 0 where the backpointers fit in LDS (and for shapes the call refuses)
extern "C" size_t mi_ctc_align_workspace_bytes(int B, int T, int U) {
    if (B < 1 || T < 1 || U < 0 || U > ALIGN_MAX_U || T > ALIGN_MAX_T) return 0;
    const AlignPlan p = align_plan(T, U);
    return p.bp_in_lds ? 0 : (size_t)B * p.bp_bytes;
}

extern "C" int mi_ctc_align(const void* logits, long ld_b, long ld_t, int dtype, const float* lse, int T,
                            const long* labels, int U, const int* in_len, int blank, int V1, int B,
                            void* workspace, size_t workspace_bytes,
                            int* path, float* score, int* tgt_len, int* start, int* end, float* token_lp, hipStream_t stream) {
    MI_ENTER();
    if (V1 < 2 || blank < 0 || blank >= V1 || T < 1 || U < 0 || B < 1 || (dtype != 0 && dtype != 1)) return MI_ERR_ARG;
    if (!logits || !lse || !in_len || !path || !score || !tgt_len || (U > 0 && !labels)) return MI_ERR_ARG;
    const int nspan = (start != nullptr) + (end != nullptr) + (token_lp != nullptr);
    if (nspan != 0 && nspan != 3) return MI_ERR_ARG;                           // nullable as a group
    if (U > ALIGN_MAX_U || T > ALIGN_MAX_T) return MI_ERR_UNSUPPORTED;
    const AlignPlan p = align_plan(T, U);
    const size_t need = p.bp_in_lds ? 0 : (size_t)B * p.bp_bytes;
    if (need && (!workspace || workspace_bytes < need || (reinterpret_cast<uintptr_t>(workspace) & 15))) return MI_ERR_ARG;
    AlignArgs a;
    a.logits = logits; a.ld_b = ld_b; a.ld_t = ld_t; a.lse = lse; a.T = T; a.labels = labels; a.U = U; a.in_len = in_len; a.blank = blank; a.V1 = V1;
    a.ws = need ? reinterpret_cast<unsigned*>(workspace) : nullptr; a.ws_words = (long)(p.bp_bytes / sizeof(unsigned));
    a.ps = p.ps; a.tch = p.tch;
    a.path = path; a.score = score; a.tgt_len = tgt_len; a.start = start; a.end = end; a.token_lp = token_lp;
#define ALIGN_LAUNCH(TY, WV, WS)                                                                                                                                  \
    do {                                                                                                                                                          \
        if (!ensure_dynamic_lds<sizeof(TY) * 4 + WV * 2 + WS>(reinterpret_cast<const void*>(ctc_align_kernel<TY, WV, WS>), ALIGN_LDS_BUDGET)) return MI_ERR_LAUNCH; \
        hipLaunchKernelGGL((ctc_align_kernel<TY, WV, WS>), dim3(B), dim3(256), p.lds, stream, a);                                                                 \
    } while (0)
#define ALIGN_FORMS(TY)                                                                                                     \
    do {                                                                                                                    \
        if (p.wave) { if (need) ALIGN_LAUNCH(TY, true, true); else ALIGN_LAUNCH(TY, true, false); }                         \
        else        { if (need) ALIGN_LAUNCH(TY, false, true); else ALIGN_LAUNCH(TY, false, false); }                       \
    } while (0)
    if (dtype == 0) ALIGN_FORMS(float); else ALIGN_FORMS(bf16_t);
#undef ALIGN_FORMS
#undef ALIGN_LAUNCH
    MI_CHECK_LAUNCH();
    return MI_OK;
}
