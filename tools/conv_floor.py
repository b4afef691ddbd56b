"""What bounds conv #2's K loop?  Times the implicit-GEMM conv (gemm8p_kernel<true, 1>: B = 32, T1 = 500, F1 = 40, C1 = C2 = 256, 3 x 3, stride 2 -> 625 tiles of
256 x 256, K = 2304) beside the DENSE instantiation of the same kernel on the same tiles (M = 160 000, N = 256, K = 2304, GELU) on whatever build HFASR_HIP_LIB names:
the product, and the GEMM_FLOOR = 1..4 builds of `bash tools/gemm_floor_ab.sh build` (1 staging alone, 2 fragment reads + MFMAs alone, 3 staging + MFMAs, 4 staging +
reads).  Both move the same bytes per K tile through the same ring; a difference in the staging-only build is the conv's A-side address stream.

    HFASR_HIP_LIB=tools/bin/libhfasr_floor1.so python tools/conv_floor.py

Per launch: median of 7 batches of 20 back-to-back launches; per K tile: launch time / (3 rounds of tiles x 36 K tiles) — 625 tiles on 256 CUs are 2.44 rounds, the
third one partly empty, for both kernels alike.
"""
import os, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from huggingface_asr_amd import ops

dev = "cuda:0"
torch.manual_seed(0)
B, T1, F1, C = 32, 500, 40, 256
x = torch.randn(B, T1, F1, C, device=dev).to(torch.bfloat16)
wp = (torch.randn(C, 9 * C, device=dev) * 0.02).to(torch.bfloat16)
b = torch.randn(C, device=dev) * 0.1
M = B * (T1 // 2) * (F1 // 2)
a = torch.randn(M, 9 * C, device=dev).to(torch.bfloat16)
out = torch.empty((M, C), device=dev, dtype=torch.bfloat16)


def timed(run):
    run(); torch.cuda.synchronize()
    ts = []
    for _ in range(7):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(20):
            run()
        e1.record(); torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3 / 20)
    return sorted(ts)[len(ts) // 2]


print(os.environ.get("HFASR_HIP_LIB", "product build"))
for name, run in (("conv2", lambda: ops.conv2d_cl(x, wp, b)), ("dense", lambda: ops.gemm(a, wp, b, out=out, act="gelu", variant=48))):      # 48: one launch of 625 tiles (no tail-round split)
    t = timed(run)
    print(f"{name} M={M} N={C} K={9 * C}: {t:7.2f} us per launch, {t / (3 * 36):6.3f} us per K tile", flush=True)
