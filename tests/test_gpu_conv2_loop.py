"""conv #2 of the front end (mi_conv2d_cl_bf16: 3 x 3, stride 2, 256 -> 256 channels as an implicit GEMM) at a shape of a few tiles: B = 2, T1 = 34, F1 = 40 gives
M = 2 * 17 * 20 = 680 output rows = two full 256-row tiles and a partial one, with taps in the zero padding on all four edges (symmetric padding) or doubled in front
(the causal form).  Checked against a float64 numpy restatement of the convolution on the bf16-rounded inputs, with the bound the float conv test of
tests/test_gpu_gemm_forms.py applies to this entry point (gemm_cases.BF16_ATOL / BF16_RTOL).  The default dispatch runs a shape this small on the 128 x 128 LDS-DMA
kernel; variant 40 forces the 256 x 256 phase kernel — the kernel the bench-size conv #2 runs on — so both K loops are covered.  The gated packing
(mi_conv2d_cl_geo_bf16, conv and gate rows in one GEMM) runs the same loop with the product in its epilogue."""
import math

import numpy as np
import pytest
import torch

import gemm_cases as G

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, T1, F1, C1, C2 = 2, 34, 40, 256, 256

_erf = np.frompyfunc(math.erf, 1, 1)


def gelu64(x):
    return 0.5 * x * (1.0 + _erf(x / math.sqrt(2.0)).astype(np.float64))


def bf16_round(a):
    return torch.from_numpy(a).to(torch.bfloat16)


def conv64(x, w, b, causal):
    """x (B, T, F, Cin), w (Cout, 3, 3, Cin), b (Cout) float64 -> (B, T', F', Cout): 3 x 3, stride 2, one zero on every side — or two in front of each axis (causal)"""
    lo, hi = (2, 0) if causal else (1, 1)
    xp = np.pad(x, ((0, 0), (lo, hi), (lo, hi), (0, 0)))
    To, Fo = (xp.shape[1] - 3) // 2 + 1, (xp.shape[2] - 3) // 2 + 1
    y = np.zeros((x.shape[0], To, Fo, w.shape[0]))
    for kh in range(3):
        for kw in range(3):
            y += xp[:, kh:kh + 2 * To:2, kw:kw + 2 * Fo:2, :][:, :To, :Fo] @ w[:, kh, kw, :].T
    return y + b


@pytest.fixture(scope="module")
def operands():
    rng = np.random.default_rng(2304)
    x = bf16_round(rng.standard_normal((B, T1, F1, C1)).astype(np.float32))
    w = bf16_round((rng.standard_normal((2 * C2, 3, 3, C1)) / math.sqrt(9 * C1)).astype(np.float32))      # rows [0, C2): the conv; [C2, 2 C2): the gate of the gated case
    b = rng.standard_normal(2 * C2).astype(np.float32)
    return x, w, b


@pytest.fixture(scope="module")
def references(operands):
    x, w, b = operands
    x64, w64, b64 = x.double().numpy(), w.double().numpy(), b.astype(np.float64)
    pre = {causal: conv64(x64, w64, b64, causal) for causal in (False, True)}
    return pre


def within_bf16_bound(got, want):
    err = np.abs(got.double().cpu().numpy() - want)
    ratio = float((err / (G.BF16_ATOL + G.BF16_RTOL * np.abs(want))).max())
    print(f"RATIO {ratio:.3f} max err {err.max():.5f}")
    return ratio <= 1.0


@pytest.mark.parametrize("variant", [0, 40], ids=["default_dispatch", "phase_kernel_256"])
@pytest.mark.parametrize("causal", [False, True], ids=["padded", "causal"])
def test_conv2_against_float64(operands, references, causal, variant):
    from huggingface_asr_amd import ops
    x, w, b = operands
    wp = w[:C2].reshape(C2, 9 * C1).contiguous().to(DEV)
    bias = torch.from_numpy(b[:C2]).to(DEV)
    got = ops.conv2d_cl(x.to(DEV), wp, bias, causal=causal, variant=variant)
    assert got.shape == (B, 17, 20, C2)
    assert within_bf16_bound(got, gelu64(references[causal][..., :C2]))
    assert torch.equal(got, ops.conv2d_cl(x.to(DEV), wp, bias, causal=causal, variant=variant))
    raw = ops.conv2d_cl(x.to(DEV), wp, bias, causal=causal, act="none", variant=variant)
    assert within_bf16_bound(raw, references[causal][..., :C2])


def test_gated_packing_against_float64(operands, references):
    """GatedConv2d's second layer as one GEMM: W rows interleaved [32 conv | 32 gate], GELU((conv + b) * sigmoid(gate + bg)) in the epilogue"""
    from huggingface_asr_amd import ops
    x, w, b = operands
    nb = C2 // 32
    flat = w.reshape(2 * C2, 9 * C1)
    wp = torch.stack([flat[:C2].view(nb, 32, -1), flat[C2:].view(nb, 32, -1)], 1).reshape(2 * C2, -1).contiguous().to(DEV)
    bt = torch.from_numpy(b)
    bp = torch.stack([bt[:C2].view(nb, 32), bt[C2:].view(nb, 32)], 1).reshape(2 * C2).contiguous().to(DEV)
    got = ops.conv2d_cl_geo(x.to(DEV), wp, bp, act="gelu", gated=True)
    pre = references[False]
    want = gelu64(pre[..., :C2] / (1.0 + np.exp(-pre[..., C2:])))
    assert got.shape == want.shape
    assert within_bf16_bound(got, want)
    assert torch.equal(got, ops.conv2d_cl_geo(x.to(DEV), wp, bp, act="gelu", gated=True))
