#!/usr/bin/env python
"""What the fp32 inference mode costs in joint decoding, and what the rows-streaming fp32 linear buys over mi_gemm_f32 at decoding's row counts.

    python tools/f32_decode_bench.py [--rounds 5] [--warmup 2] [--max-length 32] [--out profiles/f32_decode_bench.txt]

1. The config-5 shape (tests/config5_model.py: E-Branchformer-base encoder + 8 x 512 GPT-2 decoder, V = 5001), one 10 s utterance, `generate` greedy and with 5
   beams, ctc_weight 0.3, seeded weights (no EOS before max_length: every decode runs max_length - 1 token steps).  JointAEDEngine(precision="fp32") next to the
   default engine, alternated in ONE process for `rounds` rounds; wall time around the whole call (encoder, cross K/V, token loop, the copy of the result).  Reported:
   ms per decode and ms per token (= decode / steps), mean over the rounds and the spread (max - min) of the rounds, which is the run's own noise.
2. Per decoder linear shape (N, K) at M = 1, 5 and 50 rows: mi_linear_rows_f32 next to mi_gemm_f32 (the kernel the step would otherwise run), device events around
   `iters` consecutive calls of the C entries (arguments prepared once), alternated for `rounds` rounds; beside them the weight bytes of the shape and the rate at which the rows kernel reads them.
No bar is fixed in advance; the table decides `rows_route` in csrc/decoder_f32.hip (a shape where the rows kernel is not faster belongs to mi_gemm_f32)."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import config5_model as C5  # noqa: E402
from huggingface_asr_amd import _lib, ops_f32 as O, synth  # noqa: E402
from huggingface_asr_amd.decoder import JointAEDEngine, generate  # noqa: E402

DEV = "cuda:0"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=2000)
    ap.add_argument("--max-length", type=int, default=32)
    ap.add_argument("--out")
    a = ap.parse_args()

    sd = C5.state_dict(0)
    engines = {}
    for prec in ("fp32", "bf16"):
        engines[prec] = JointAEDEngine(C5.ENC_CFG, C5.DEC_CFG, C5.JCFG, DEV, precision=prec)
        engines[prec].load_state_dict(sd)
    del sd
    feats = torch.from_numpy(synth.normal(1, "feats", (1, 1000, 80), 1.0)).to(DEV)
    flen = torch.tensor([1000], dtype=torch.int32, device=DEV)

    def decode(prec, W):
        stats = {}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        generate(engines[prec], feats, flen, num_beams=W, max_length=a.max_length, ctc_weight=0.3, eos_token_id=1, stats=stats)
        return (time.perf_counter() - t0) * 1e3, stats["steps"]

    lines = [f"config-5 shape, one 10 s utterance, generate to max_length = {a.max_length}, ctc_weight 0.3; {a.rounds} rounds, precisions alternated in one process "
             f"(ms: mean +- spread of the rounds)"]
    res = {}
    for W in (1, 5):
        for prec in engines:
            for _ in range(a.warmup):
                decode(prec, W)
        per = {p: [] for p in engines}
        steps = {}
        for _ in range(a.rounds):
            for prec in engines:
                ms, steps[prec] = decode(prec, W)
                per[prec].append(ms)
        for prec in engines:
            m, s = sum(per[prec]) / len(per[prec]), max(per[prec]) - min(per[prec])
            res[f"W{W}_{prec}"] = dict(decode_ms=m, spread_ms=s, steps=steps[prec], token_ms=m / steps[prec])
            lines.append(f"W = {W}  precision={prec}   {m:8.2f} +- {s:5.2f} ms per decode   {m / steps[prec]:7.3f} ms per token   ({steps[prec]} steps)")
        lines.append(f"W = {W}  fp32 / bf16 = {res[f'W{W}_fp32']['decode_ms'] / res[f'W{W}_bf16']['decode_ms']:.2f}x")

    # ---- the decoder's linear shapes, rows kernel next to the tiled GEMM
    d, V = C5.D, C5.V
    shapes_nk = [("qkv", 3 * d, d), ("attn out / q / cross out", d, d), ("mlp fc (gelu_new)", 4 * d, d), ("mlp proj", d, 4 * d), ("head", V, d)]

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / a.iters * 1e3          # us

    lines.append(f"decoder linears, fp32, us per launch ({a.iters} launches per leg, {a.rounds} rounds alternated; mean +- spread): mi_linear_rows_f32 | mi_gemm_f32 | "
                 f"weight bytes | rows kernel's rate over them")
    table = []
    L_ = _lib.lib()
    for what, N, K in shapes_nk:
        w, b = torch.full((N, K), 0.01, device=DEV), torch.full((N,), 0.01, device=DEV)
        act = "gelu_new" if "gelu" in what else "none"
        for M in (1, 5, 50):
            x, out = torch.full((M, K), 0.01, device=DEV), torch.empty((M, N), device=DEV)
            # the C entries themselves, arguments prepared once: a wrapper's allocation and checks per call would be most of a 10 us launch
            nws = O.linear_rows_workspace_bytes(M, N, K)
            ws = torch.empty((max(nws, 4),), dtype=torch.uint8, device=DEV)
            st = torch.cuda.current_stream().cuda_stream
            rows_args = (x.data_ptr(), K, w.data_ptr(), K, b.data_ptr(), 2 if act == "gelu_new" else 0, out.data_ptr(), N, 0, None, None, 1, 0, 0, 0, M, N, K, ws.data_ptr(), nws, st)
            gemm_args = (x.data_ptr(), K, w.data_ptr(), K, b.data_ptr(), out.data_ptr(), N, None, 0, 1.0, 2 if act == "gelu_new" else 0, M, N, K, st)
            legs = dict(rows=lambda: L_.mi_linear_rows_f32(*rows_args), gemm=lambda: L_.mi_gemm_f32(*gemm_args))
            assert legs["rows"]() == 0 and legs["gemm"]() == 0
            for fn in legs.values():
                for _ in range(5):
                    fn()
            per = {k: [] for k in legs}
            for _ in range(a.rounds):
                for k, fn in legs.items():
                    per[k].append(timed(fn))
            mean = {k: sum(v) / len(v) for k, v in per.items()}
            spread = {k: max(v) - min(v) for k, v in per.items()}
            nbytes = N * K * 4
            table.append(dict(what=what, M=M, N=N, K=K, rows_us=mean["rows"], gemm_us=mean["gemm"], rows_spread=spread["rows"], gemm_spread=spread["gemm"], weight_bytes=nbytes))
            lines.append(f"{what:<26s} M={M:<3d} N={N:<5d} K={K:<5d} {mean['rows']:8.2f} +- {spread['rows']:5.2f} | {mean['gemm']:8.2f} +- {spread['gemm']:5.2f} | "
                         f"{nbytes / 2 ** 20:6.2f} MiB | {nbytes / mean['rows'] / 1e3:7.1f} GB/s | gemm / rows = {mean['gemm'] / mean['rows']:.2f}x | ksplit {max(1, nws // (4 * M * N))}")
    lost = [f"{t['what']} M={t['M']}" for t in table if t["rows_us"] >= t["gemm_us"]]
    lines.append("shapes where the rows kernel is not faster than mi_gemm_f32: " + (", ".join(lost) if lost else "none"))
    lines.append(json.dumps(dict(tool="f32_decode_bench", max_length=a.max_length, rounds=a.rounds, decode=res, linears=table)))
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
