#!/usr/bin/env python
"""What CTC prefix beam search costs next to the greedy transcript: base encoder + CTC head, 32 x 10 s, the configuration's own V1, beams 5 / 10 / 64, one
step at a time on one stream, every leg alternated in ONE process.

    python tools/ctc_beam_bench.py [--steps 50] [--rounds 5] [--warmup 10] [--out profiles/ctc_beam_bench.txt]
    python tools/ctc_beam_bench.py --bias 100 --out profiles/ctc_bias_bench.txt      (also the biased walk and call, N random 3-token phrases, weight 1.5)
    python tools/ctc_beam_bench.py --trace-beams 10 --steps 20      (the two launches only, for `rocprofv3 --kernel-trace --stats -- python tools/ctc_beam_bench.py ...`)

  forward      engine.forward(want_hidden=False): the logits only
  greedy       engine.transcribe(): the argmax out of the head GEMM's epilogue + the collapse
  cut W        launch A alone (mi_ctc_beam_cut, token_topk = W) over the forward's logits; its bytes/s are the logits' size (valid rows only) over its time
  walk W       launch B alone (mi_ctc_beam_walk) over a cut made once; us per frame = its time over the longest utterance's frames (one block per utterance, side by side)
  beams W      engine.transcribe(beams=W): forward + cut + walk
  walk W bias  (--bias N) launch B with the bias policy (mi_ctc_beam_walk_bias) over the same cut: what contextual biasing costs over `walk W`
  beams W bias (--bias N) engine.transcribe(beams=W, bias=)

Device events around `steps` consecutive calls of a leg; the legs run in turn for `rounds` rounds.  Reported per leg: the mean over all rounds and the spread
(max - min of the per-round means) — the forward's spread is the run's own noise.  Back-to-back launches: a leg's time includes its launch gaps."""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from huggingface_asr_amd import _lib, ops, shapes, synth  # noqa: E402
from huggingface_asr_amd.engine import EBranchformerEngine  # noqa: E402

DEV = "cuda:0"
HBM_PEAK_TBS = 8.0          # MI355X HBM3E peak (MI355X_MICROARCH.md)
BEAMS = (5, 10, 64)


def walk_call(logits, lengths, blank, W, cut, bias=None):
    """launch B alone over a finished cut: the C entry with buffers made once; bias (a CtcBias): the biased entry"""
    L = _lib.lib()
    B, T, V1 = logits.shape
    K = cut["lp"].shape[-1]
    nbytes = int(L.mi_ctc_beam_workspace_bytes(B, T, W))
    ws = torch.empty((nbytes,), device=DEV, dtype=torch.uint8)
    tokens = torch.empty((B, 1, T), device=DEV, dtype=torch.int64)
    n, scores = torch.empty((B, 1), device=DEV, dtype=torch.int32), torch.empty((B, 1), device=DEV, dtype=torch.float32)
    credit = torch.empty((B, 1), device=DEV, dtype=torch.int32)

    def call_bias():
        col, tab = bias.to(DEV)
        rc = L.mi_ctc_beam_walk_bias(logits.data_ptr(), logits.stride(1), logits.stride(0), 0 if logits.dtype == torch.float32 else 1, B, T, V1, lengths.data_ptr(), blank, 0,
                                     W, K, 1, cut["lse"].data_ptr(), cut["lp_blank"].data_ptr(), cut["lp"].data_ptr(), cut["ids"].data_ptr(), ws.data_ptr(), nbytes,
                                     tokens.data_ptr(), 1, n.data_ptr(), scores.data_ptr(), None, col.data_ptr(), tab.data_ptr(), bias.S, bias.A1, bias.weight,
                                     credit.data_ptr(), ops._stream())
        _lib.check(rc, "mi_ctc_beam_walk_bias")
        return tokens, n, scores
    if bias is not None:
        return call_bias

    def call():
        rc = L.mi_ctc_beam_walk(logits.data_ptr(), logits.stride(1), logits.stride(0), 0 if logits.dtype == torch.float32 else 1, B, T, V1, lengths.data_ptr(), blank, 0,
                                W, K, 1, cut["lse"].data_ptr(), cut["lp_blank"].data_ptr(), cut["lp"].data_ptr(), cut["ids"].data_ptr(), ws.data_ptr(), nbytes,
                                tokens.data_ptr(), 1, n.data_ptr(), scores.data_ptr(), None, ops._stream())
        _lib.check(rc, "mi_ctc_beam_walk")
        return tokens, n, scores
    return call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--trace-beams", type=int)
    ap.add_argument("--bias", type=int, help="N random 3-token phrases: adds the biased walk and the biased call beside the unbiased ones")
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
    valid_rows, longest = int(outer.sum()), int(outer.max())
    logits_bytes = valid_rows * V1 * logits.element_size()

    bias = None
    if a.bias:
        import numpy as np

        from huggingface_asr_amd.ctc_bias import CtcBias
        bias = CtcBias(np.random.default_rng(0).integers(0, V1 - 1, size=(a.bias, 3)).tolist(), 1.5, V1, V1 - 1)
    legs = {"forward": lambda: eng.forward(feats, lens, want_hidden=False), "greedy": lambda: eng.transcribe(feats, lens, pad_id=0)}
    for W in BEAMS if a.trace_beams is None else (a.trace_beams,):
        cut = ops.ctc_beam_cut(logits, V1 - 1, min(W, V1 - 1), outer)
        legs[f"cut {W}"] = (lambda W=W: ops.ctc_beam_cut(logits, V1 - 1, min(W, V1 - 1), outer))
        legs[f"walk {W}"] = walk_call(logits, outer, V1 - 1, W, cut)
        legs[f"beams {W}"] = (lambda W=W: eng.transcribe(feats, lens, pad_id=0, beams=W))
        tokens, n, _ = legs[f"walk {W}"]()
        whole = legs[f"beams {W}"]()
        assert torch.equal(whole["n_tokens"], n[:, 0]) and torch.equal(whole["tokens"], tokens[:, 0]), "the stand-alone walk and transcribe(beams=) differ"
        if bias is not None:
            legs[f"walk {W} bias"] = walk_call(logits, outer, V1 - 1, W, cut, bias)
            legs[f"beams {W} bias"] = (lambda W=W: eng.transcribe(feats, lens, pad_id=0, beams=W, bias=bias))
            tokens, n, _ = legs[f"walk {W} bias"]()
            whole = legs[f"beams {W} bias"]()
            assert torch.equal(whole["n_tokens"], n[:, 0]) and torch.equal(whole["tokens"], tokens[:, 0]), "the stand-alone biased walk and transcribe(beams=, bias=) differ"
    if a.trace_beams is not None:
        legs = {k: v for k, v in legs.items() if k.startswith(("cut", "walk"))}

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
    res = dict(tool="ctc_beam_bench", device=torch.cuda.get_device_name(0), batch=B, seconds=10, frames=T2, classes=V1, logits_dtype=str(logits.dtype), steps=a.steps, rounds=a.rounds,
               valid_rows=valid_rows, longest_utterance_frames=longest, logits_bytes=logits_bytes,
               mean_ms={k: round(v, 5) for k, v in mean.items()},
               spread_ms={k: round(max(v) - min(v), 5) for k, v in per.items()},
               cut_tb_per_s={k: round(logits_bytes / mean[k] / 1e9, 3) for k in mean if k.startswith("cut")}, hbm_peak_tb_per_s=HBM_PEAK_TBS,
               walk_us_per_frame={k: round(mean[k] * 1e3 / longest, 3) for k in mean if k.startswith("walk")})
    if bias is not None:
        res.update(bias=dict(phrases=len(bias.phrases), states=bias.S, columns=bias.A1, weight=bias.weight),
                   bias_walk_over_unbiased={f"walk {W}": round(mean[f"walk {W} bias"] / mean[f"walk {W}"], 4) for W in BEAMS if f"walk {W} bias" in mean})
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("tools/ctc_beam_bench.py: base encoder + CTC head, 32 x 10 s, times in ms per call (mean over the rounds; spread = max - min of the round means)\n")
            f.write(f"device: {res['device']}; {a.rounds} rounds x {a.steps} calls per leg after {a.warmup} warm-up calls; logits {V1} classes {logits.dtype}, "
                    f"{valid_rows} valid rows = {logits_bytes / 1e6:.1f} MB, longest utterance {longest} frames\n")
            for k in legs:
                extra = f"   {res['cut_tb_per_s'][k]:.3f} TB/s of logits (HBM peak {HBM_PEAK_TBS})" if k in res["cut_tb_per_s"] else \
                        f"   {res['walk_us_per_frame'][k]:.3f} us per frame" if k in res["walk_us_per_frame"] else ""
                f.write(f"  {k:<13} {mean[k]:9.4f}   spread {res['spread_ms'][k]:.4f}{extra}\n")
            if bias is not None:
                f.write(f"bias: {len(bias.phrases)} phrases of 3 tokens, {bias.S} states x {bias.A1} columns, weight {bias.weight}; biased walk / unbiased walk: "
                        + ", ".join(f"{W} beams {res['bias_walk_over_unbiased'][f'walk {W}']:.3f}" for W in BEAMS if f"walk {W}" in res["bias_walk_over_unbiased"]) + "\n")
            f.write(line + "\n")


if __name__ == "__main__":
    main()
