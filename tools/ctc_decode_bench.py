#!/usr/bin/env python
"""What a transcript costs next to the logits: base encoder + CTC head, 32 x 10 s, one step at a time on one stream, four legs alternated in ONE process.

    python tools/ctc_decode_bench.py [--steps 200] [--rounds 5] [--warmup 20] [--out FILE.json]
    python tools/ctc_decode_bench.py --trace-leg D --steps 20        (one leg only, for `rocprofv3 --kernel-trace --stats -- python tools/ctc_decode_bench.py ...`)
    python tools/ctc_decode_bench.py --argmax-pass                   (the stand-alone argmax pass over the (8000, 5001) fp32 logits against its traffic floor)

  A  engine.forward(want_hidden=False): logits only — the path bench.py times, unchanged by the transcription work: the yardstick
  B  A + torch.argmax(-1) + mi_ctc_collapse: what a careful user of the logits could do
  C  transcribe(head_argmax=False): head GEMM into a scratch, mi_row_argmax, mi_ctc_collapse
  D  transcribe(head_argmax=True): the argmax out of the head GEMM's epilogue, no logits written

Device events around `steps` consecutive steps of a leg; the legs run A B C D A B C D ... for `rounds` rounds.  Reported per leg: the mean step time over all
rounds and the spread (max - min of the per-round means); leg A's spread is the run's own noise, what D has to be judged against.  One JSON line."""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from huggingface_asr_amd import ops, shapes, synth  # noqa: E402
from huggingface_asr_amd.engine import EBranchformerEngine  # noqa: E402

DEV = "cuda:0"
HBM_PEAK_TBS = 8.0          # MI355X HBM3E peak (MI355X_MICROARCH.md)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--trace-leg", choices=list("ABCD"))
    ap.add_argument("--argmax-pass", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()

    cfg = dict(shapes.BASE, ctc_zero_infinity=True, ctc_loss_reduction="mean")
    B, T, V1 = 32, 1000, cfg["vocab_size"] + 1
    eng = EBranchformerEngine(cfg, DEV)
    eng.load_state_dict({k: torch.from_numpy(v) for k, v in synth.state_dict_numpy(shapes.param_shapes(cfg), 0).items()})
    feats = torch.from_numpy(synth.normal(1, "feats", (B, T, 80), 1.0)).to(DEV)
    lens = torch.tensor([998 - 37 * (i % 9) for i in range(B)], dtype=torch.int32, device=DEV)

    def leg_a():
        return eng.forward(feats, lens, want_hidden=False)

    def leg_b():
        o = eng.forward(feats, lens, want_hidden=False)
        return ops.ctc_collapse(torch.argmax(o["logits"], -1).to(torch.int32), V1 - 1, 0, o["outer_len"])

    def leg_c():
        eng.head_argmax = False
        return eng.transcribe(feats, lens, pad_id=0)

    def leg_d():
        eng.head_argmax = True
        return eng.transcribe(feats, lens, pad_id=0)

    legs = dict(A=leg_a, B=leg_b, C=leg_c, D=leg_d)

    def timed(fn, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / n

    if a.argmax_pass:
        logits = eng.forward(feats, lens, want_hidden=False)["logits"]
        x = logits.reshape(B * logits.shape[1], V1)
        for _ in range(a.warmup):
            ops.row_argmax(x)
        ms = timed(lambda: ops.row_argmax(x), a.steps)
        nbytes = x.shape[0] * V1 * 4
        res = dict(tool="ctc_decode_bench", mode="argmax_pass", rows=x.shape[0], classes=V1, logits_bytes=nbytes, ms=round(ms, 5),
                   tb_per_s=round(nbytes / ms / 1e9, 3), hbm_peak_tb_per_s=HBM_PEAK_TBS, note="back-to-back launches: includes launch gaps; the kernel trace has the kernel's own time")
    elif a.trace_leg:
        for _ in range(a.warmup):
            legs[a.trace_leg]()
        res = dict(tool="ctc_decode_bench", mode="trace", leg=a.trace_leg, steps=a.steps, ms=round(timed(legs[a.trace_leg], a.steps), 5))
    else:
        ref = leg_c()
        got = leg_d()
        assert eng._head_fusable(), "the bench size must run the fused head"
        assert all(torch.equal(ref[k], got[k]) for k in ("best", "tokens", "n_tokens")), "fused and unfused transcripts differ"
        for _ in range(a.warmup):
            for fn in legs.values():
                fn()
        torch.cuda.synchronize()
        per = {k: [] for k in legs}
        for _ in range(a.rounds):
            for k, fn in legs.items():
                per[k].append(timed(fn, a.steps))
        T2 = ref["best"].shape[1]
        res = dict(tool="ctc_decode_bench", mode="legs", batch=B, seconds=10, steps=a.steps, rounds=a.rounds,
                   mean_ms={k: round(sum(v) / len(v), 5) for k, v in per.items()},
                   spread_ms={k: round(max(v) - min(v), 5) for k, v in per.items()},
                   rounds_ms={k: [round(t, 5) for t in v] for k, v in per.items()},
                   logits_bytes_not_written=B * T2 * eng._config_struct(B, T, 80).logits_ld * 4,
                   mean_tokens=float(got["n_tokens"].float().mean()))
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
