// The frame body of the Kaldi-style log-mel filterbank (fbank.hip states what it restates): one wave computes one frame of 400 samples.  Shared by the one-shot
// kernel (fbank.hip fbank_kernel: a frame's samples lie in the clip) and the streaming push kernel (fbank_stream.hip: they lie partly in the slot's carry, partly in
// the new samples), so that the two cannot drift: the way a sample is fetched is the body's only parameter.
#pragma once
#include "common.hpp"

namespace fbank_body {

constexpr int FRAME = 400, HOP = 160, NFFT = 512, NBINS = 257;
constexpr int MEL_W = 640;                                              // LDS slots for the packed mel weights (>= 2 * NBINS + a triangle's slack)
constexpr int NZ = NFFT / 2;                                            // the complex transform has 256 points: two 4-KiB buffers per wave, 36 KiB per block -> 4 blocks per CU
constexpr size_t LDS_BYTES = (4 * 2 * NZ + NZ) * sizeof(double2) + MEL_W * sizeof(double) + 256 * sizeof(int);     // a block of four waves

// frames of N samples (snip edges)
__host__ __device__ inline int num_frames(int N) { return N >= FRAME ? 1 + (N - FRAME) / HOP : 0; }

struct Tables {
    const double* window;                // (400)
    const double* twiddle;               // (256, 2)  exp(-2*pi*i*k/512)
    const double* mel_t;                 // (nmel, 257) dense transposed filterbank
    const int* mel_lo; const int* mel_hi;   // (nmel) non-zero bin range [lo, hi)
    int nmel; double mel_floor; double preemph;
};

// a block's view of its LDS after `setup`
struct Lds {
    double2* buf0; double2* buf1;        // the wave's two FFT buffers
    double2* twl;                        // [NFFT/2] twiddles, shared by the four waves (an LDS read instead of a global load per butterfly)
    double* mwt;                         // [MEL_W] the mel triangles' non-zero spans, packed back to back
    int* moff;                           // [nmel + 1] (nmel <= 127)
    int* mlo_s;                          // [nmel]: the spans' first bins
    bool mel_lds;
};

__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// once per block of 256 threads (every thread calls it: it holds block barriers)
__device__ __forceinline__ Lds setup(char* smem, const Tables& p) {
    const int wave = threadIdx.x >> 6;
    Lds s;
    s.buf0 = reinterpret_cast<double2*>(smem) + wave * 2 * NZ;
    s.buf1 = s.buf0 + NZ;
    s.twl = reinterpret_cast<double2*>(smem) + 4 * 2 * NZ;
    for (int i = threadIdx.x; i < NFFT / 2; i += 256) s.twl[i] = double2{p.twiddle[2 * i], p.twiddle[2 * i + 1]};
    // the mel triangles' non-zero spans, packed back to back in LDS (every bin lies under at most two triangles: <= 2 * 257 weights): the filter loop of step 5 read its
    // weights from global memory, one dependent L2 round trip per bin of the longest span (~40) and frame — most of the kernel's time
    s.mwt = reinterpret_cast<double*>(s.twl + NFFT / 2);
    s.moff = reinterpret_cast<int*>(s.mwt + MEL_W);
    s.mlo_s = s.moff + 128;
    if ((int)threadIdx.x < p.nmel) { s.mlo_s[threadIdx.x] = p.mel_lo[threadIdx.x]; s.moff[threadIdx.x + 1] = max(p.mel_hi[threadIdx.x] - p.mel_lo[threadIdx.x], 0); }
    __syncthreads();
    if (threadIdx.x == 0) {
        int o = 0;
        for (int f = 0; f < p.nmel; ++f) { const int n = s.moff[f + 1]; s.moff[f] = o; o += n; }
        s.moff[p.nmel] = o;
    }
    __syncthreads();
    const int mtot = s.moff[p.nmel];
    s.mel_lds = mtot <= MEL_W;
    if (s.mel_lds)
        for (int i = threadIdx.x; i < mtot; i += 256) {                  // one load per thread: the filter of slot i by bisection of the offsets
            int lo = 0, hi = p.nmel - 1;
            while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (s.moff[mid] <= i) lo = mid; else hi = mid - 1; }
            s.mwt[i] = p.mel_t[(long)lo * NBINS + s.mlo_s[lo] + (i - s.moff[lo])];
        }
    __syncthreads();
    return s;
}

// One frame by one wave.  fetch(n), 0 <= n < 400: sample n of the frame, float32 in [-1, 1].  o (nmel): the frame's log-mel energies; with means / stds (both or
// neither; the one-shot kernel passes none) each is stored as (x - mean) / std — global_norm_kernel's two float32 operations in its order, a subtraction and a division.
template <typename Fetch>
__device__ __forceinline__ void frame(const Tables& p, const Lds& L, int lane, Fetch fetch, float* o, const float* means, const float* stds) {
    double2* const buf0 = L.buf0;
    double2* const buf1 = L.buf1;
    const double2* const twl = L.twl;
    // 1. load (x * 2^15 in float32, then float64), DC offset.  Lane owns the sample PAIRS (2m, 2m+1), m = lane + 64 i: the real 512-point
    //    transform is done as a complex 256-point FFT of z[m] = x[2m] + i x[2m+1] and unpacked afterwards (half the butterflies)
    double xa[4], xb[4], xp[4];
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int n0 = 2 * (lane + 64 * i), n1 = n0 + 1;
        xa[i] = (n0 < FRAME) ? (double)(fetch(n0) * 32768.0f) : 0.0;
        xb[i] = (n1 < FRAME) ? (double)(fetch(n1) * 32768.0f) : 0.0;
        xp[i] = (n0 >= 1 && n0 < FRAME) ? (double)(fetch(n0 - 1) * 32768.0f) : 0.0;
        s += xa[i] + xb[i];
    }
    const double mean = wave_sum_d(s) / (double)FRAME;
    // 2. pre-emphasis on the DC-removed frame, window, into the FFT buffer (zero padded to 512 samples = 256 pairs)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int m = lane + 64 * i, n0 = 2 * m, n1 = n0 + 1;
        double v0 = 0.0, v1 = 0.0;
        if (n0 < FRAME) {
            const double c0 = xa[i] - mean;
            v0 = ((n0 == 0) ? c0 * (1.0 - p.preemph) : c0 - p.preemph * (xp[i] - mean)) * p.window[n0];
            if (n1 < FRAME) v1 = ((xb[i] - mean) - p.preemph * c0) * p.window[n1];
        }
        buf0[m] = double2{v0, v1};
    }
    wave_lds_sync();
    // 3. Stockham radix-4 DIF, 256 points = 4 stages, one butterfly per lane and stage.  w(j) = exp(-2 pi i j / 256) from the 512th-root table.
    auto w256 = [&](int j) { const double2 t = twl[2 * (j & 127)]; return (j & 128) ? double2{-t.x, -t.y} : t; };
    auto cmul = [](double2 a, double2 b) { return double2{a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x}; };
    double2* src = buf0;
    double2* dst = buf1;
    int nn = 256, st = 1;
#pragma unroll
    for (int stage = 0; stage < 4; ++stage) {
        const int n4 = nn >> 2;
        const int q = lane & (st - 1), pp = lane / st;         // butterfly `lane`: 0..63 = (n/4) * s
        const double2 a = src[q + st * pp], b = src[q + st * (pp + n4)], c = src[q + st * (pp + 2 * n4)], d = src[q + st * (pp + 3 * n4)];
        const double2 apc = {a.x + c.x, a.y + c.y}, amc = {a.x - c.x, a.y - c.y};
        const double2 bpd = {b.x + d.x, b.y + d.y}, bmd = {b.x - d.x, b.y - d.y};
        const int j = pp * st;                                 // exp(-2 pi i pp / nn) = w256(pp * st)
        dst[q + st * (4 * pp + 0)] = double2{apc.x + bpd.x, apc.y + bpd.y};
        dst[q + st * (4 * pp + 1)] = cmul(double2{amc.x + bmd.y, amc.y - bmd.x}, w256(j));          // a - i b - c + i d
        dst[q + st * (4 * pp + 2)] = cmul(double2{apc.x - bpd.x, apc.y - bpd.y}, w256(2 * j));
        dst[q + st * (4 * pp + 3)] = cmul(double2{amc.x - bmd.y, amc.y + bmd.x}, w256(3 * j));      // a + i b - c - i d
        wave_lds_sync();
        double2* tmp = src; src = dst; dst = tmp;
        nn = n4; st <<= 2;
    }
    // 4. unpack the real transform, X[k] = E[k] + W512^k O[k] with E = (Z[k] + conj Z[256-k]) / 2, O = (Z[k] - conj Z[256-k]) / (2i), and take the
    //    power of the complex64-rounded spectrum (kept in LDS: dst reused as 257 doubles)
    double* pw = reinterpret_cast<double*>(dst);
    double pk[5];
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        const int k = lane + 64 * i;
        pk[i] = 0.0;
        if (k < NBINS) {
            const double2 zk = src[k & 255], zc = src[(256 - k) & 255];
            const double2 e = {0.5 * (zk.x + zc.x), 0.5 * (zk.y - zc.y)};
            const double2 o2 = {0.5 * (zk.y + zc.y), -0.5 * (zk.x - zc.x)};             // (zk - conj zc) / (2i)
            const double2 wk = (k < 256) ? twl[k] : double2{-1.0, 0.0};
            const double2 ow = cmul(o2, wk);
            const double re = (double)(float)(e.x + ow.x), im = (double)(float)(e.y + ow.y);
            pk[i] = re * re + im * im;                  // (|X|^2 directly: sqrt-then-square of the reference differs from it by one float64 rounding, 1e-16 relative; a float64
                                                        // square root is ~20 instructions of the ~850 per frame that bound this kernel — PMC: f64 VALU issue = its duration)
        }
    }
    wave_lds_sync();                                            // every lane has read Z before dst/src are reused for the powers
#pragma unroll
    for (int i = 0; i < 5; ++i) { const int k = lane + 64 * i; if (k < NBINS) pw[k] = pk[i]; }
    wave_lds_sync();
    // 5. mel filters, floor, log
    for (int f = lane; f < p.nmel; f += 64) {
        const int lo = L.mlo_s[f], hi = lo + (L.moff[f + 1] - L.moff[f]);
        double acc = 0.0;
        if (L.mel_lds) {
            const double* mw = L.mwt + L.moff[f] - lo;
            for (int k = lo; k < hi; ++k) acc += pw[k] * mw[k];       // same products in the same order as the global-memory form
        } else {
            const double* mt = p.mel_t + (long)f * NBINS;
            for (int k = lo; k < hi; ++k) acc += pw[k] * mt[k];
        }
        const float v = logf((float)fmax(acc, p.mel_floor));     // float32 log of the float64 energy: within 1 ulp (1e-6 absolute) of float32(log64(acc)); the float64 log was ~60 instructions per value
        o[f] = means ? (v - means[f]) / stds[f] : v;
    }
    wave_lds_sync();
}

}  // namespace fbank_body
