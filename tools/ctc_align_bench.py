#!/usr/bin/env python
"""What CTC forced alignment costs next to the loss's alpha recursion (the same dependency chain, no backpointers) and next to the forward: base encoder + CTC
head, 32 x 10 s, the configuration's own V1, targets of ~40 and ~120 labels, and one long shape (T = 1500, 400 labels) whose backpointers go through the
workspace.  One step at a time on one stream, every leg alternated in ONE process.

    python tools/ctc_align_bench.py [--steps 50] [--rounds 5] [--warmup 10] [--out profiles/ctc_align_bench.txt]

  forward        engine.forward(want_hidden=False): the logits only
  engine.align   engine.align(): forward + row_lse + mi_ctc_align (targets of ~40 labels)
  row_lse        ops.row_lse over the forward's logits (what both kernels below are handed)
  align N        mi_ctc_align alone over the forward's logits, targets of ~N labels (N = 40: the wave form; 120: the block form), buffers made once
  loss N         mi_ctc_loss_fwd alone on identical inputs (N = 40: its wave form, fp32, halved chain; 120: its block form, float64)
  align long     mi_ctc_align, synthetic logits (4, 1500, 501), 400 labels: block form, backpointers in the workspace
  loss long      mi_ctc_loss_fwd on identical inputs
  align span     mi_ctc_align on the long shape with ONE label whose class dominates every frame: the token spans all 1500 frames, the longest serial token_lp sum
                 (one thread adds 1500 values in time order at the tail of the launch); `align short` is the same call on the unmodified logits (a span of a few frames)

Device events around `steps` consecutive calls of a leg; the legs run in turn for `rounds` rounds.  Reported per leg: the mean over all rounds and the spread
(max - min of the per-round means).  Back-to-back launches: a leg's time includes its launch gaps."""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from huggingface_asr_amd import _lib, ops, shapes, synth  # noqa: E402
from huggingface_asr_amd.engine import EBranchformerEngine  # noqa: E402

DEV = "cuda:0"


def targets(B, n, V, seed):
    """(B, n + 8) int64: n - (b % 5) labels per row (no two equal neighbours), then -100"""
    g = np.random.default_rng(seed)
    lab = np.full((B, n + 8), -100, dtype=np.int64)
    for b in range(B):
        prev = -1
        for u in range(n - b % 5):
            c = int(g.integers(0, V))
            while c == prev:
                c = int(g.integers(0, V))
            lab[b, u] = prev = c
    return torch.from_numpy(lab).to(DEV)


def align_call(logits, lse, labels, lens):
    L = _lib.lib()
    B, T, V1 = logits.shape
    U = labels.shape[1]
    nbytes = int(L.mi_ctc_align_workspace_bytes(B, T, U))
    ws = torch.empty((max(nbytes, 16),), device=DEV, dtype=torch.uint8)
    path, start, end = (torch.empty(s, device=DEV, dtype=torch.int32) for s in ((B, T), (B, U), (B, U)))
    score, tlp, tl = torch.empty((B,), device=DEV), torch.empty((B, U), device=DEV), torch.empty((B,), device=DEV, dtype=torch.int32)

    def call():
        rc = L.mi_ctc_align(logits.data_ptr(), logits.stride(0), logits.stride(1), 0, lse.data_ptr(), T, labels.data_ptr(), U, lens.data_ptr(), V1 - 1, V1, B,
                            ws.data_ptr() if nbytes else None, nbytes, path.data_ptr(), score.data_ptr(), tl.data_ptr(), start.data_ptr(), end.data_ptr(), tlp.data_ptr(),
                            ops._stream())
        _lib.check(rc, "mi_ctc_align")
        return score
    return call, nbytes


def loss_call(logits, lse, labels, lens):
    L = _lib.lib()
    B, T, V1 = logits.shape
    U = labels.shape[1]
    nll, tl, loss = torch.empty((B,), device=DEV), torch.empty((B,), device=DEV, dtype=torch.int32), torch.empty((1,), device=DEV)

    def call():
        rc = L.mi_ctc_loss_fwd(logits.data_ptr(), logits.stride(0), logits.stride(1), 0, lse.data_ptr(), T, labels.data_ptr(), U, lens.data_ptr(), V1 - 1, B, 1, 1,
                               nll.data_ptr(), tl.data_ptr(), loss.data_ptr(), ops._stream())
        _lib.check(rc, "mi_ctc_loss_fwd")
        return nll
    return call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out")
    a = ap.parse_args()

    cfg = dict(shapes.BASE, ctc_zero_infinity=True, ctc_loss_reduction="mean")
    B, T, V1 = 32, 1000, cfg["vocab_size"] + 1
    eng = EBranchformerEngine(cfg, DEV)
    eng.load_state_dict({k: torch.from_numpy(v) for k, v in synth.state_dict_numpy(shapes.param_shapes(cfg), 0).items()})
    feats = torch.from_numpy(synth.normal(1, "feats", (B, T, 80), 1.0)).to(DEV)
    lens = torch.tensor([998 - 37 * (i % 9) for i in range(B)], dtype=torch.int32, device=DEV)
    fwd = eng.forward(feats, lens, want_hidden=False)
    logits, outer = fwd["logits"], fwd["outer_len"].contiguous()
    T2 = logits.shape[1]
    lse = ops._row_lse_3d(logits)

    legs = {"forward": lambda: eng.forward(feats, lens, want_hidden=False)}
    lab40 = targets(B, 40, V1 - 1, 40)
    legs["engine.align"] = lambda: eng.align(feats, lens, lab40)
    legs["row_lse"] = lambda: ops._row_lse_3d(logits)
    where = {}
    for n in (40, 120):
        lab = targets(B, n, V1 - 1, n)
        legs[f"align {n}"], ws = align_call(logits, lse, lab, outer)
        legs[f"loss {n}"] = loss_call(logits, lse, lab, outer)
        where[f"align {n}"] = "workspace" if ws else "LDS"
        sc, nll = legs[f"align {n}"]().clone(), legs[f"loss {n}"]().clone()
        assert torch.isfinite(sc).all() and (sc <= -nll + 1e-3).all(), "the best path's log-probability exceeds the sum over all paths"
    TL, NL, VL = 1500, 400, 501
    xl = torch.from_numpy((np.random.default_rng(7).standard_normal((4, TL, VL)) * 3.0).astype(np.float32)).to(DEV)
    lsel, labl, lensl = ops._row_lse_3d(xl), targets(4, NL, VL - 1, 400), torch.full((4,), TL, dtype=torch.int32, device=DEV)
    legs["align long"], ws = align_call(xl, lsel, labl, lensl)
    legs["loss long"] = loss_call(xl, lsel, labl, lensl)
    where["align long"] = "workspace" if ws else "LDS"
    xs = xl.clone()
    xs[:, :, 7] += 30.0
    one = torch.full((4, 8), -100, dtype=torch.int64, device=DEV)
    one[:, 0] = 7
    legs["align span"], ws = align_call(xs, ops._row_lse_3d(xs), one, lensl)
    legs["align short"], _ = align_call(xl, lsel, one, lensl)
    where["align span"] = where["align short"] = "workspace" if ws else "LDS"

    def timed(fn, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / n

    for _ in range(a.warmup):
        for fn in legs.values():
            fn()
    torch.cuda.synchronize()
    per = {k: [] for k in legs}
    for _ in range(a.rounds):
        for k, fn in legs.items():
            per[k].append(timed(fn, a.steps))
    mean = {k: sum(v) / len(v) for k, v in per.items()}
    ratio = {f"align {k} / loss {k}": round(mean[f"align {k}"] / mean[f"loss {k}"], 3) for k in ("40", "120", "long")}
    ratio["align span / align short"] = round(mean["align span"] / mean["align short"], 3)
    ratio["engine.align / forward"] = round(mean["engine.align"] / mean["forward"], 4)
    res = dict(tool="ctc_align_bench", device=torch.cuda.get_device_name(0), batch=B, seconds=10, frames=T2, classes=V1, logits_dtype=str(logits.dtype), steps=a.steps,
               rounds=a.rounds, longest_utterance_frames=int(outer.max()), long_shape=[4, TL, VL, NL], backpointers=where,
               mean_ms={k: round(v, 5) for k, v in mean.items()}, spread_ms={k: round(max(v) - min(v), 5) for k, v in per.items()}, ratios=ratio)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("tools/ctc_align_bench.py: base encoder + CTC head, 32 x 10 s, times in ms per call (mean over the rounds; spread = max - min of the round means)\n")
            f.write(f"device: {res['device']}; {a.rounds} rounds x {a.steps} calls per leg after {a.warmup} warm-up calls; logits {V1} classes {logits.dtype}, "
                    f"{T2} frames, longest utterance {res['longest_utterance_frames']}; long shape: 4 x {TL} frames x {VL} classes, {NL} labels\n")
            for k in legs:
                extra = f"   backpointers in {where[k]}" if k in where else ""
                f.write(f"  {k:<13} {mean[k]:9.4f}   spread {res['spread_ms'][k]:.4f}{extra}\n")
            for k, v in ratio.items():
                f.write(f"  {k}: {v}\n")
            f.write(line + "\n")


if __name__ == "__main__":
    main()
