// The fp32 GEMM of the precision = "fp32" inference mode (gemm_f32.hip): argument block shared by the public entry mi_gemm_f32 and the
// internal callers of encoder_f32.hip (batched attention products, conv #2 as an implicit GEMM).
#pragma once
#include <hip/hip_runtime.h>

// C[z] (M, N) = resid + alpha * act(A[z] (M, K) · W[z]^T + bias),   z = zb * nh + zh  (blockIdx.z): operand z starts at base + zb * s?b + zh * s?h.
// W is (N, K) row-major (ldw = its row stride), or with w_kn the (K, N) row-major matrix itself (C = A · W: the P · V product of the attention).
// conv != 0: A is not a matrix but a channels-last activation (B, T1, F1, C1); row m = (b, t2, f2), column k = (kh, kw, c) is gathered in the A load
// (zero outside the image), which makes the kernel an implicit-GEMM Conv2d without an im2col buffer.
struct GemmF32Args {
    const float* A; long lda, sAb, sAh;
    const float* W; long ldw, sWb, sWh; int w_kn;
    const float* bias;
    const float* resid; long ldr;
    float* C; long ldc, sCb, sCh;
    float alpha; int act;          // act: 0 none, 1 erf-GELU (exact erff), 2 gelu_new (exact tanhf)
    int M, N, K, nz, nh;
    int conv, T1, F1, C1, KW, stride, pt, pf, T2, F2;
};

int gemm_f32_launch(const GemmF32Args& a, hipStream_t st);
