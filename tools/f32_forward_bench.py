#!/usr/bin/env python
"""What the fp32 inference mode costs: base encoder + CTC head, 32 x 10 s, `precision="fp32"` next to the default bf16 mode, alternated in ONE process.

    python tools/f32_forward_bench.py [--steps 20] [--rounds 5] [--warmup 5] [--out profiles/f32_forward_bench.txt]

Legs (device events around `steps` consecutive forwards, run F B F B ... for `rounds` rounds; reported: the mean step time over all rounds and the spread =
max - min of the per-round means, which is the run's own noise):
  F  EBranchformerEngine(precision="fp32").forward(want_hidden=False)
  B  EBranchformerEngine().forward(want_hidden=False)                       the path bench.py times
Then, the same way, where the fp32 step's time goes — the step's own operator calls replayed alone through huggingface_asr_amd/ops_f32.py on the step's shapes:
  L  every Linear of one forward through mi_gemm_f32 (front-end out, feature projection, per layer FFN x 4, QKV, attention out, cgMLP x 2, merge; the head)
  A  the 16 attentions (mi_attention_f32: scores, softmax, P.V — its three products are the same GEMM kernel, batched)
  C  the two Conv2d layers of the front end (conv #2 is the same GEMM kernel with the im2col gather in its A load)
`rest` = F - L - A - C: LayerNorms, depthwise convs / CSGU, launch gaps.

For orientation only (no bar): 72.0 GFLOP per utterance x 32 = 2.3 TFLOP per step = 14.9 ms at the 155 TF/s the f32-input MFMA measures."""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from huggingface_asr_amd import ops_f32 as O, shapes, synth  # noqa: E402
from huggingface_asr_amd.engine import EBranchformerEngine  # noqa: E402

DEV = "cuda:0"
MFMA_F32_TFS = 155.0        # measured rate of v_mfma_f32_32x32x2_f32 on the MI355X


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out")
    a = ap.parse_args()

    cfg = dict(shapes.BASE, ctc_zero_infinity=True, ctc_loss_reduction="mean")
    B, T = 32, 1000
    sd = {k: torch.from_numpy(v) for k, v in synth.state_dict_numpy(shapes.param_shapes(cfg), 0).items()}
    feats = torch.from_numpy(synth.normal(1, "feats", (B, T, 80), 1.0)).to(DEV)
    lens = torch.tensor([998 - 37 * (i % 9) for i in range(B)], dtype=torch.int32, device=DEV)
    engines = {}
    for name, kw in (("F", dict(precision="fp32")), ("B", {})):
        engines[name] = EBranchformerEngine(cfg, DEV, **kw)
        engines[name].load_state_dict(sd)
    del sd

    d, I, H, L, V1 = cfg["hidden_size"], cfg["intermediate_size"], cfg["num_attention_heads"], cfg["num_hidden_layers"], cfg["vocab_size"] + 1
    C1, C2 = cfg["conv_dim"]
    T2 = engines["F"].out_frames(T)
    M, F2 = B * T2, 20
    z = lambda *s: torch.full(s, 0.01, dtype=torch.float32, device=DEV)
    # (M, N, K, act, count per forward) of the Linears
    linears = [(M, d, F2 * C2, "none", 1), (M, d, d, "none", 1), (M, I, d, "gelu", 3 * L), (M, d, I, "none", 2 * L), (M, 3 * d, d, "none", L), (M, d, d, "none", L),
               (M, d, I // 2, "none", L), (M, d, 2 * d, "none", L), (2 * T2 - 1, d, d, "none", 0), (M, V1, d, "none", 1)]      # (the position projection is cached: 0 per step)
    lin_ops = [(z(m, k), z(n, k), z(n), z(m, n), act, cnt) for m, n, k, act, cnt in linears if cnt]
    gflop = sum(2.0 * m * n * k * cnt for m, n, k, _, cnt in linears) / 1e9
    qkv, pos, u = z(M, 3 * d), z(2 * T2 - 1, d), z(d)
    x80, w1, b1, w2, b2 = z(B, T, 80), z(C1, 9), z(C1), z(C2, 9 * C1), z(C2)

    def leg_l():
        for av, wv, bv, out, act, cnt in lin_ops:
            for _ in range(cnt):
                O.gemm(av, wv, bv, out, act=act)

    def leg_a():
        for _ in range(L):
            O.attention(qkv[:, :d], qkv[:, d:2 * d], qkv[:, 2 * d:], B, T2, H, pos=pos, bias_u=u, bias_v=u, lengths=None)

    def leg_c():
        O.conv2d_cl(O.conv2d_first_gelu(x80, w1, b1), w2, b2)

    legs = dict(F=lambda: engines["F"].forward(feats, lens, want_hidden=False), B=lambda: engines["B"].forward(feats, lens, want_hidden=False),
                L=leg_l, A=leg_a, C=leg_c)

    def timed(fn, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / n

    for fn in legs.values():
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()
    per_round = {k: [] for k in legs}
    for _ in range(a.rounds):
        for k, fn in legs.items():
            per_round[k].append(timed(fn, a.steps if k in "FB" else max(1, a.steps // 4)))
    mean = {k: sum(v) / len(v) for k, v in per_round.items()}
    spread = {k: max(v) - min(v) for k, v in per_round.items()}
    rest = mean["F"] - mean["L"] - mean["A"] - mean["C"]
    lines = [f"base encoder + CTC head, {B} x {T / 100:.0f} s, {a.rounds} rounds x {a.steps} steps, legs alternated in one process (ms per step: mean, spread of the round means)"]
    for k, what in (("F", "precision=fp32 forward"), ("B", "precision=bf16 forward (default)"), ("L", "  fp32: the Linears through mi_gemm_f32"),
                    ("A", "  fp32: the 16 attentions (mi_attention_f32)"), ("C", "  fp32: the Conv2d front end")):
        lines.append(f"{k}  {what:<48s} {mean[k]:8.3f}  +- {spread[k]:.3f}")
    lines.append(f"   {'  fp32: rest (LayerNorm, depthwise convs, gaps)':<48s} {rest:8.3f}")
    lines.append(f"fp32 / bf16 = {mean['F'] / mean['B']:.2f}x; Linears: {gflop:.0f} GFLOP per step = {gflop / mean['L']:.1f} TF/s in mi_gemm_f32 "
                 f"({100 * mean['L'] / mean['F']:.0f} % of the fp32 step; with the attention's and conv #2's products, which run the same kernel: "
                 f"{100 * (mean['L'] + mean['A'] + mean['C']) / mean['F']:.0f} %); floor at {MFMA_F32_TFS:.0f} TF/s for 2304 GFLOP: {2304 / MFMA_F32_TFS:.1f} ms")
    lines.append(json.dumps(dict(tool="f32_forward_bench", B=B, T=T, steps=a.steps, rounds=a.rounds, mean_ms=mean, spread_ms=spread, rest_ms=rest,
                                 linear_gflop=gflop, linear_tfs=gflop / mean["L"], fp32_over_bf16=mean["F"] / mean["B"])))
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
