// Whisper's timestamp rules inside the greedy token loop on gfx950: transformers' `WhisperTimeStampLogitsProcessor` (generation/logits_process.py) followed by the
// argmax, as one launch per token that reads the step's fp32 logits once and writes the chosen token for mi_greedy_advance.
//
// Every rule of the processor masks a contiguous range of columns decided by the row's history, so a row reduces to two column intervals — the text tokens and the
// timestamp tokens that survive — found from a backward scan of the sampled tokens ids[b, begin : cur):
//   1. <|notimestamps|> (= timestamp_begin - 1) is never allowed;
//   2. pairing: last token a timestamp and the one before it too (or there is only one sampled token) -> no timestamp; last a timestamp after text -> nothing below EOS;
//   3. monotonicity: no timestamp below the last one sampled (the equal one stays allowed only to close a segment, i.e. after text);
//   4. first generated position: timestamps only, none beyond timestamp_begin + max_initial_timestamp_index;
//   5. if logsumexp(timestamps) > max(text) over the surviving columns (log_softmax's normaliser is the same on both sides and cancels), the text goes too.
// One pass: per thread the best key (common.hpp argmax_*: torch.argmax's order) of each interval and an online log-sum-exp of the timestamp interval; wave reductions by
// xor shuffles, then the four waves' partials through LDS, combined in wave order by every thread — no atomics, the result is a fixed function of the inputs.  A row in
// which nothing finite survives gives 0, as torch.argmax over a row of -inf.
// Beam search takes the same rules as a mask over the step's logits plus the raw row's log-sum-exp (mi_whisper_beam_scores, further down).
#include "common.hpp"
#include "row_lse.hpp"
#include "../../include/hfasr_hip.h"

namespace {

struct TsArgs {
    const float* logits; long ld; int V;
    const long* ids; long ld_ids; int begin, cur;
    int no_ts, eos, max_initial, detect;
    int* best;
};

struct Lse { float m, s; };                                          // sum exp(x) = s * exp(m); the empty sum is (-inf, 0)

__device__ __forceinline__ Lse lse_push(Lse a, float x) {
    if (x == -INFINITY) return a;
    if (x > a.m) return Lse{x, a.s * expf(a.m - x) + 1.f};            // (a.m = -inf: exp(-inf) = 0, a.s = 0)
    return Lse{a.m, a.s + expf(x - a.m)};
}
__device__ __forceinline__ Lse lse_join(Lse a, Lse b) {
    const float M = fmaxf(a.m, b.m);
    if (M == -INFINITY) return Lse{-INFINITY, 0.f};
    return Lse{M, a.s * expf(a.m - M) + b.s * expf(b.m - M)};
}

struct Part { amax_t text, ts; Lse l; };

__device__ __forceinline__ void fold(Part& p, float v, int i, int t_lo, int t_hi, int s_lo, int s_hi) {
    if (i >= t_lo && i < t_hi) p.text = argmax_max(p.text, argmax_key(v, i));
    if (i >= s_lo && i < s_hi) { p.ts = argmax_max(p.ts, argmax_key(v, i)); p.l = lse_push(p.l, v); }
}

// The surviving intervals [t_lo, t_hi) of text and [s_lo, s_hi) of timestamps of one row under rules 1-4, by the whole 256-thread block (one barrier; s_pos: 4 ints of LDS)
__device__ __forceinline__ void ts_intervals(const long* seq, int begin, int cur, int V, int no_ts, int eos, int max_initial, int* s_pos, int& t_lo, int& t_hi, int& s_lo,
                                             int& s_hi) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tb = no_ts + 1, n = cur - begin;
    // history: position of the last sampled timestamp (backward scan: a thread stops at its first hit), -1 when there is none
    int pos = -1;
    for (int j = cur - 1 - tid; j >= begin; j -= 256)
        if (seq[j] >= tb) { pos = j; break; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) pos = max(pos, __shfl_xor(pos, o, 64));
    if (lane == 0) s_pos[wave] = pos;
    __syncthreads();
    pos = max(max(s_pos[0], s_pos[1]), max(s_pos[2], s_pos[3]));
    const bool last_ts = n >= 1 && seq[cur - 1] >= tb;
    const bool pen_ts = n < 2 || seq[cur - 2] >= tb;
    t_lo = 0; t_hi = no_ts < V ? no_ts : V; s_lo = tb; s_hi = V;
    if (last_ts) {
        if (pen_ts) s_hi = 0;
        else { t_lo = max(t_lo, eos); s_lo = max(s_lo, eos); }
    }
    if (pos >= 0) {
        const long tl = seq[pos] + ((last_ts && !pen_ts) ? 0 : 1);
        s_lo = max(s_lo, (int)(tl < (long)V ? tl : (long)V));
    }
    if (n == 0) {
        t_hi = 0;
        if (max_initial >= 0 && max_initial < V) s_hi = min(s_hi, tb + max_initial + 1);      // (an index past the vocabulary masks nothing)
    }
}

__global__ __launch_bounds__(256) void whisper_timestamp_argmax_kernel(TsArgs a) {
    __shared__ int s_pos[4];
    __shared__ amax_t s_text[4], s_ts[4];
    __shared__ float s_m[4], s_s[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, row = blockIdx.x;
    int t_lo, t_hi, s_lo, s_hi;
    ts_intervals(a.ids + (long)row * a.ld_ids, a.begin, a.cur, a.V, a.no_ts, a.eos, a.max_initial, s_pos, t_lo, t_hi, s_lo, s_hi);
    // one pass over the row
    const float* xr = a.logits + (long)row * a.ld;
    Part p{ARGMAX_EMPTY, ARGMAX_EMPTY, Lse{-INFINITY, 0.f}};
    int covered = 0;
    if ((reinterpret_cast<uintptr_t>(xr) & 15) == 0) {
        const int nvec = a.V / 4;
        const f32x4* xv = reinterpret_cast<const f32x4*>(xr);
        int q = tid;
        for (; q + 256 < nvec; q += 512) {                            // two 16-B loads in flight per lane
            const f32x4 v0 = xv[q], v1 = xv[q + 256];
#pragma unroll
            for (int e = 0; e < 4; ++e) fold(p, v0[e], q * 4 + e, t_lo, t_hi, s_lo, s_hi);
#pragma unroll
            for (int e = 0; e < 4; ++e) fold(p, v1[e], (q + 256) * 4 + e, t_lo, t_hi, s_lo, s_hi);
        }
        for (; q < nvec; q += 256) {
            const f32x4 v = xv[q];
#pragma unroll
            for (int e = 0; e < 4; ++e) fold(p, v[e], q * 4 + e, t_lo, t_hi, s_lo, s_hi);
        }
        covered = nvec * 4;
    }
    for (int c = covered + tid; c < a.V; c += 256) fold(p, xr[c], c, t_lo, t_hi, s_lo, s_hi);
    // wave reductions (every lane ends with the wave's values), then the four waves in order
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        p.text = argmax_max(p.text, __shfl_xor(p.text, o, 64));
        p.ts = argmax_max(p.ts, __shfl_xor(p.ts, o, 64));
        p.l = lse_join(p.l, Lse{__shfl_xor(p.l.m, o, 64), __shfl_xor(p.l.s, o, 64)});
    }
    if (lane == 0) { s_text[wave] = p.text; s_ts[wave] = p.ts; s_m[wave] = p.l.m; s_s[wave] = p.l.s; }
    __syncthreads();
    if (tid == 0) {
        amax_t kt = s_text[0], ks = s_ts[0];
        Lse l{s_m[0], s_s[0]};
        for (int w = 1; w < 4; ++w) { kt = argmax_max(kt, s_text[w]); ks = argmax_max(ks, s_ts[w]); l = lse_join(l, Lse{s_m[w], s_s[w]}); }
        const float ts_lse = l.s > 0.f ? l.m + logf(l.s) : -INFINITY;
        const float text_max = kt == ARGMAX_EMPTY ? -INFINITY : argmax_value(kt);
        amax_t k = (a.detect && ts_lse > text_max) ? ks : argmax_max(kt, ks);
        const bool finite = k != ARGMAX_EMPTY && argmax_value(k) != -INFINITY;      // (a NaN compares unequal: it wins, as in torch.argmax)
        a.best[row] = finite ? argmax_index(k) : 0;
    }
}

// ---- beam search.  transformers' `_beam_search` takes log_softmax of the RAW logits first and hands the log-probabilities to the processors, so a suppressed column counts
// in the normaliser and the greedy path's -inf head bias cannot be used.  Per row this kernel gives the beam-step kernels (which form logit - lse themselves) both halves:
// lse of the raw row, and the row with -inf in every column the processors mask — begin-suppress / suppress (`sup`, 0 / -inf, nullable), then the timestamp rules above
// (off when no_ts < 0) — every other value left as it is, not even re-written.  Rule 5 is decided on the surviving columns with the greedy kernel's arithmetic (lse_push /
// lse_join, waves combined in order): the normaliser is the same on both sides and cancels.
// Phases, one block per row: (A) all 256 threads read the row once (16-B loads where the row is aligned): the raw maximum, the best surviving text value, the online
// log-sum-exp of the surviving timestamps;  (A') wave 0 runs mi_row_lse's sum pass (row_lse.hpp) under that maximum, over a row that is now in cache — the same code on
// the same column order, so lse[row] is mi_row_lse's bit for bit;  (B) after a barrier (the row is rewritten in place, and (A') must have read it whole) every thread
// stores -inf to the masked columns of its share: 16-B stores where four neighbours go together, nothing is loaded but `sup`.  No atomics, no scratch.
struct BeamScoreArgs {
    float* logits; long ld; int V;
    const long* ids; long ld_ids; int begin, cur;
    const float* sup;
    int no_ts, eos, max_initial, detect;
    float* lse;
};

struct Stat { float rmax, tmax; Lse l; };

__device__ __forceinline__ void fold_stat(Stat& p, float v, bool suppressed, int i, int t_lo, int t_hi, int s_lo, int s_hi) {
    p.rmax = fmaxf(p.rmax, v);
    if (suppressed) return;
    if (i >= t_lo && i < t_hi) p.tmax = fmaxf(p.tmax, v);
    if (i >= s_lo && i < s_hi) p.l = lse_push(p.l, v);
}

__global__ __launch_bounds__(256) void whisper_beam_scores_kernel(BeamScoreArgs a) {
    __shared__ int s_pos[4];
    __shared__ float s_r[4], s_t[4], s_m[4], s_s[4];
    __shared__ float s_mx;
    __shared__ int s_drop;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, row = blockIdx.x;
    int t_lo = 0, t_hi = a.V, s_lo = a.V, s_hi = a.V;                  // rules off: everything is text, nothing is a timestamp
    if (a.no_ts >= 0) ts_intervals(a.ids + (long)row * a.ld_ids, a.begin, a.cur, a.V, a.no_ts, a.eos, a.max_initial, s_pos, t_lo, t_hi, s_lo, s_hi);
    float* xr = a.logits + (long)row * a.ld;
    const bool vec = (reinterpret_cast<uintptr_t>(xr) & 15) == 0 && (a.sup == nullptr || (reinterpret_cast<uintptr_t>(a.sup) & 15) == 0);
    const int nvec = vec ? a.V / 4 : 0;
    // (A) one read of the row
    Stat p{-INFINITY, -INFINITY, Lse{-INFINITY, 0.f}};
    {
        const f32x4* xv = reinterpret_cast<const f32x4*>(xr);
        const f32x4* sv = reinterpret_cast<const f32x4*>(a.sup);
        for (int q = tid; q < nvec; q += 256) {
            const f32x4 v = xv[q];
            f32x4 s = {0.f, 0.f, 0.f, 0.f};
            if (a.sup) s = sv[q];
#pragma unroll
            for (int e = 0; e < 4; ++e) fold_stat(p, v[e], s[e] == -INFINITY, q * 4 + e, t_lo, t_hi, s_lo, s_hi);
        }
        for (int c = nvec * 4 + tid; c < a.V; c += 256) fold_stat(p, xr[c], a.sup && a.sup[c] == -INFINITY, c, t_lo, t_hi, s_lo, s_hi);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        p.rmax = fmaxf(p.rmax, __shfl_xor(p.rmax, o, 64));
        p.tmax = fmaxf(p.tmax, __shfl_xor(p.tmax, o, 64));
        p.l = lse_join(p.l, Lse{__shfl_xor(p.l.m, o, 64), __shfl_xor(p.l.s, o, 64)});
    }
    if (lane == 0) { s_r[wave] = p.rmax; s_t[wave] = p.tmax; s_m[wave] = p.l.m; s_s[wave] = p.l.s; }
    __syncthreads();
    if (tid == 0) {
        float r = s_r[0], t = s_t[0];
        Lse l{s_m[0], s_s[0]};
        for (int w = 1; w < 4; ++w) { r = fmaxf(r, s_r[w]); t = fmaxf(t, s_t[w]); l = lse_join(l, Lse{s_m[w], s_s[w]}); }
        const float ts_lse = l.s > 0.f ? l.m + logf(l.s) : -INFINITY;
        s_mx = r;
        s_drop = (a.detect && a.no_ts >= 0 && ts_lse > t) ? 1 : 0;
    }
    __syncthreads();
    // (A') the raw row's log-sum-exp: mi_row_lse's sum pass by one wave
    if (wave == 0) {
        const float r = wave_row_lse_given_max(xr, a.V, s_mx, lane);
        if (lane == 0) a.lse[row] = r;
    }
    if (s_drop) t_hi = t_lo;                                           // rule 5: the text goes
    __syncthreads();
    // (B) -inf into the masked columns
    const float NI = -INFINITY;
    {
        f32x4* xv = reinterpret_cast<f32x4*>(xr);
        const f32x4* sv = reinterpret_cast<const f32x4*>(a.sup);
        for (int q = tid; q < nvec; q += 256) {
            f32x4 s = {0.f, 0.f, 0.f, 0.f};
            if (a.sup) s = sv[q];
            bool m[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int c = q * 4 + e;
                m[e] = s[e] == -INFINITY || !((c >= t_lo && c < t_hi) || (c >= s_lo && c < s_hi));
            }
            if (m[0] && m[1] && m[2] && m[3]) xv[q] = f32x4{NI, NI, NI, NI};
            else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (m[e]) xr[q * 4 + e] = NI;
            }
        }
        for (int c = nvec * 4 + tid; c < a.V; c += 256)
            if ((a.sup && a.sup[c] == -INFINITY) || !((c >= t_lo && c < t_hi) || (c >= s_lo && c < s_hi))) xr[c] = NI;
    }
}

}  // namespace

extern "C" int mi_whisper_beam_scores(float* logits, long ld, int V, const long* ids, long ld_ids, int begin_index, int cur_len, const float* suppress,
                                      int no_timestamps_token_id, int eos_token_id, int max_initial_timestamp_index, int detect_from_logprob, float* lse, int rows,
                                      hipStream_t stream) {
    MI_ENTER();
    if (!logits || !lse || rows <= 0 || V <= 0 || ld < V) return MI_ERR_ARG;
    if (no_timestamps_token_id >= 0) {
        if (!ids || begin_index < 0 || cur_len < begin_index || cur_len > ld_ids) return MI_ERR_ARG;
        if (no_timestamps_token_id >= V || eos_token_id < 0 || eos_token_id > V || max_initial_timestamp_index < -1) return MI_ERR_ARG;
    }
    BeamScoreArgs a{logits, ld, V, ids, ld_ids, begin_index, cur_len, suppress, no_timestamps_token_id < 0 ? -1 : no_timestamps_token_id, eos_token_id,
                    max_initial_timestamp_index, detect_from_logprob ? 1 : 0, lse};
    hipLaunchKernelGGL(whisper_beam_scores_kernel, dim3(rows), dim3(256), 0, stream, a);
    MI_CHECK_LAUNCH();
    return MI_OK;
}

extern "C" int mi_whisper_timestamp_argmax(const float* logits, long ld, int V, const long* ids, long ld_ids, int begin_index, int cur_len, int no_timestamps_token_id,
                                           int eos_token_id, int max_initial_timestamp_index, int detect_from_logprob, int* best, int B, hipStream_t stream) {
    MI_ENTER();
    if (!logits || !ids || !best || B <= 0 || V <= 0 || ld < V) return MI_ERR_ARG;
    if (begin_index < 0 || cur_len < begin_index || cur_len > ld_ids) return MI_ERR_ARG;
    if (no_timestamps_token_id < 0 || no_timestamps_token_id >= V || eos_token_id < 0 || eos_token_id > V || max_initial_timestamp_index < -1) return MI_ERR_ARG;
    TsArgs a{logits, ld, V, ids, ld_ids, begin_index, cur_len, no_timestamps_token_id, eos_token_id, max_initial_timestamp_index, detect_from_logprob ? 1 : 0, best};
    hipLaunchKernelGGL(whisper_timestamp_argmax_kernel, dim3(B), dim3(256), 0, stream, a);
    MI_CHECK_LAUNCH();
    return MI_OK;
}
