// Exact top-k selection for one block, shared by the kernels that pick a few best candidates out of thousands (beam_step_wide.hip, ctc_beam.hip): candidates become
// 56-bit keys whose unsigned order IS (value descending, index ascending), and a radix select over LDS histograms finds the k-th key.  Integer counts only: the outcome
// does not depend on the order in which threads arrive.
#pragma once
#include "common.hpp"

typedef unsigned long long u64;

__device__ __forceinline__ unsigned ord_key(float v) {
    unsigned b = __builtin_bit_cast(unsigned, v);
    b = b == 0x80000000u ? 0u : b;
    return b ^ ((unsigned)((int)b >> 31) | 0x80000000u);
}
__device__ __forceinline__ float ord_value(unsigned k) { return __builtin_bit_cast(float, (k & 0x80000000u) ? (k ^ 0x80000000u) : ~k); }
__device__ __forceinline__ u64 cand_key(unsigned hi, int e) { return ((u64)hi << 24) | (u64)(0xFFFFFFu - (unsigned)e); }
__device__ __forceinline__ int key_index(u64 k) { return (int)(0xFFFFFFu - (unsigned)(k & 0xFFFFFFull)); }

// The k-th largest of the block's keys (k >= 1, at most as many as there are keys; all keys distinct): `each(f)` calls f(key) for every key the thread owns.  On
// return the k largest are exactly those with (key >> shift) >= thr.  Most significant digit first; a pass counts the digits of the keys that match the digits chosen so
// far, wave 0 finds the bin in which the k-th falls (a suffix sum over the 256 bins, four per lane); the search ends as soon as that bin is taken whole — after the four
// value digits unless candidates tie there.  hist: 256 ints, ctl: 3 ints of LDS.  Every thread of the block calls it.
template <typename Each>
__device__ __forceinline__ void radix_select(Each&& each, int k, int* hist, int* ctl, u64& thr, int& thr_shift) {
    const int tid = threadIdx.x, lane = tid & 63;
    u64 prefix = 0;
    int shift = 48, rem = k;
    for (;;) {
        if (tid < 256) hist[tid] = 0;
        __syncthreads();
        each([&](u64 key) {
            if (shift == 48 || (key >> (shift + 8)) == prefix) atomicAdd(&hist[(int)(key >> shift) & 255], 1);
        });
        __syncthreads();
        if (tid < 64) {
            const int c0 = hist[4 * lane], c1 = hist[4 * lane + 1], c2 = hist[4 * lane + 2], c3 = hist[4 * lane + 3];
            const int mine = c0 + c1 + c2 + c3;
            int incl = mine;                                           // keys in this lane's bins and every higher lane's
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int t = __shfl_down(incl, o, 64);
                if (lane + o < 64) incl += t;
            }
            const int a3 = incl - mine, a2 = a3 + c3, a1 = a2 + c2, a0 = a1 + c1;      // keys above bin 4 lane + j
            const int cs[4] = {c0, c1, c2, c3}, as[4] = {a0, a1, a2, a3};
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (as[j] < rem && rem <= as[j] + cs[j]) { ctl[0] = 4 * lane + j; ctl[1] = rem - as[j]; ctl[2] = cs[j]; }
        }
        __syncthreads();
        const int cnt = ctl[2];
        prefix = (prefix << 8) | (u64)(unsigned)ctl[0];
        rem = ctl[1];
        if (rem == cnt || shift == 0) break;
        shift -= 8;
    }
    thr = prefix;
    thr_shift = shift;
}
