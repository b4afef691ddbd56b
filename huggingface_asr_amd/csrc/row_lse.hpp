// The sum pass of a row's log-sum-exp by ONE wave, given the row's maximum: lane l adds exp(x[c] - mx) over its columns c = l, l + 64, ... in order, then the wave's sum.
// mi_row_lse (csrc/ctc.hip) and mi_whisper_beam_scores (csrc/whisper_rules.hip) both run this code, so their values agree bit for bit: mi_row_lse's register-resident
// form for short rows adds the same terms in the same order (its padding adds exp(-inf) = 0, which changes no partial sum), and a maximum is exact in any order.
#pragma once
#include "common.hpp"

template <typename T>
__device__ __forceinline__ float wave_row_lse_given_max(const T* __restrict__ xr, int V, float mx, int lane) {
    float s = 0.f;
    for (int c = lane; c < V; c += 64) s += __expf((float)xr[c] - mx);
    s = wave_sum(s);
    return mx + __logf(s);
}
